"""Large records and clip triangles binned by the record set-up kernel itself (RasterParams::binInSetup).

With CHORDVIS_BIN_IN_SETUP=1 (the default) the set-up wave that makes a record touching more than 2x2 tiles bins it into every
tile of the conservative corner test, and clips and bins the clip triangles of its clusters once its clusters are done; no
raster_clip_and_bin_large_kernel is launched.  CHORDVIS_BIN_IN_SETUP=0 brings back the lists and that launch.  Each case is
rendered in two child interpreters (the switch is read once per process), every frame is held to the oracle, and the two runs
to each other: image, largeRecords, clipTriangles, binEntries, trianglesSubmitted, overflow 0.  Cases:
  * floor / floor_2: a camera just above a floor patch -- clip triangles and large records in the first pass;
  * masked_floor: the same with an alpha-tested floor -- masked clip triangles (texture coordinates through the clipper);
  * ground: config 3's street at 1280 x 720 from a hand above the ground, moving -- the second pass has clip triangles and
    large records, and a light second pass takes only the tiles its bins touched."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import orc
from chord_amd import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("floor", "floor_2", "masked_floor", "ground")
STATS = ("largeRecords", "clipTriangles", "binEntries", "trianglesSubmitted", "overflow", "kernelLaunches")


def case(name):
    """(scene, [cameras], flags): the frames of a case, rendered in order on one context."""
    if name == "floor":
        scene, cam = scenes.floor_under_camera(width=256, height=192)
        return scene, [cam, cam.moved((0.05, 0.0, -0.1))], H.ALL_FLAGS
    if name == "floor_2":
        scene, cam = scenes.floor_under_camera((1.3, 0.15, -2.0), (-0.4, -0.3, -1.0), 320, 180)
        return scene, [cam], 0
    if name == "masked_floor":
        scene, cam = scenes.masked_floor_under_camera()
        return scene, [cam, cam.moved((0.0, 0.02, -0.05))], H.ALL_FLAGS
    if name == "ground":
        scene, _ = scenes.config3_street(1280, 720)
        g = scenes.Camera((-62.0, 0.25, 3.0), (1.0, -0.02, -0.04), 1280, 720)
        f = np.array(g.front, dtype=np.float64)
        f /= np.linalg.norm(f)
        return scene, [g.moved(tuple(0.3 * i * f)) for i in range(4)], H.ALL_FLAGS
    raise ValueError(name)


def _inputs(scene, cam, last_cam):
    from chord_amd import lib as L
    view0, _ = L.make_views(last_cam)
    view, iv = L.make_views(cam, view0)
    return view, iv, L.fill_objects(scene, cam, last_cam).copy()


def run_case(name, out_path):
    from chord_amd.renderer import VisibilityRenderer
    scene, cams, flags = case(name)
    r = VisibilityRenderer(0)
    r.upload_scene(scene)
    r.allocate_gbuffer(cams[0].width, cams[0].height)
    res = {}
    for i, cam in enumerate(cams):
        view, iv, objs = _inputs(scene, cam, cams[i - 1] if i else cam)
        r.update_objects(objs)
        r.set_view(view, iv, flags)
        r.render_frame()
        st = r.stats()
        res["vis%d" % i] = r.read_visibility()
        res["stats%d" % i] = np.array([sum(st[k]) if isinstance(st[k], list) else st[k] for k in STATS], np.int64)
        res["passes%d" % i] = np.array(st["largeRecords"] + st["clipTriangles"], np.int64)
    r.close()
    np.savez(out_path, **res)


def _child_main(out_dir):
    for name in CASES:
        run_case(name, os.path.join(out_dir, name + ".npz"))
    print(json.dumps({"ok": True}))


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    out = {}
    for value in ("1", "0"):
        d = str(tmp_path_factory.mktemp("bin_in_setup_" + value))
        env = dict(os.environ)
        env["CHORDVIS_BIN_IN_SETUP"] = value
        code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_bin_in_setup as T; T._child_main(%r)" % (ROOT, os.path.join(ROOT, "tests"), d)
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, "child (CHORDVIS_BIN_IN_SETUP=%s) failed:\n%s\n%s" % (value, p.stdout[-2000:], p.stderr[-4000:])
        out[value] = d
    return out


@pytest.mark.parametrize("name", CASES)
def test_binning_in_setup_matches_oracle_and_the_binner_launch(runs, name):
    scene, cams, flags = case(name)
    got = {v: np.load(os.path.join(d, name + ".npz")) for v, d in runs.items()}
    prev = None
    large = clipped = 0
    for i, cam in enumerate(cams):
        view, iv, objs = _inputs(scene, cam, cams[i - 1] if i else cam)
        want = orc.frame(scene.with_objects(objs), view, iv, flags, prev_hzb_min=prev)
        for v, g in got.items():
            what = "%s frame %d, CHORDVIS_BIN_IN_SETUP=%s" % (name, i, v)
            H.assert_vis_equal(g["vis%d" % i], want["vis"], cam.width, cam.height, what)
            s = dict(zip(STATS, g["stats%d" % i].tolist()))
            assert s["overflow"] == 0 and s["trianglesSubmitted"] == want["stats"].trianglesSubmitted, (what, s)
        on, off = (dict(zip(STATS, got[v]["stats%d" % i].tolist())) for v in ("1", "0"))
        for k in ("largeRecords", "clipTriangles", "binEntries", "trianglesSubmitted"):
            assert on[k] == off[k], (name, i, k, on[k], off[k])
        assert np.array_equal(got["1"]["passes%d" % i], got["0"]["passes%d" % i]), (name, i)
        # the binner launch is gone: at least one launch fewer per frame
        assert on["kernelLaunches"] <= off["kernelLaunches"] - 1, (name, i, on, off)
        large += on["largeRecords"]
        clipped += on["clipTriangles"]
        prev = want["hzb_min"]
    assert large + clipped > 0, (name, large, clipped)       # (the case takes the paths it is there for)
