"""Light later passes that take only the tiles their bins touched (launch_raster: RasterParams::tileTouched).

Every reservation of a bin slot goes through bin_alloc, and the one that draws a tile's slot 0 sets the tile's bit in the pass's
mask; the direct tile kernel of such a pass launches at most one workgroup per tile slot and takes set bits w, w + G, ... as its
items (touched_tile), the tiles behind the G-th set bit one each.  Sequences of config 3 frames are rendered in child interpreters
with CHORDVIS_TILE_TOUCHED (read once per process) at 1 (the default: touched tiles, a grid of the device's tile slots), 8 (at
most 8 workgroups: nearly every workgroup takes further items) and 0 (the direct form over every tile).  Each frame is held to
the oracle -- image, list 0, the four stage counts, triangles, the history HZB's min / max / valid range -- and the three runs to
each other, down to the second pass's per-tile bin counts.  Sequences:
  * sky: two frames looking up into the empty sky -- a light second pass that touches no tile at all -- between street views;
  * moving: along the street -- a light second pass with a few hundred touched tiles;
  * blocks: the same with every cluster set up as pixel blocks (DBG_FORCE_BLOCKS): tiles touched by blocks only;
  * ground: a hand above the ground, moving -- second-pass triangles through the near plane (clipper) and across many tiles
    (large binner);
  * cut: light, then two heavy second passes (every object 'was' 500 m further down the view in the frame before), then light
    again -- the heavy / light reports must steer the host back and forth."""
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
W, HH = 1280, 720
DBG_FORCE_BLOCKS = 65536
SEQUENCES = ("sky", "moving", "blocks", "ground", "cut")


def _scene():
    return scenes.config3_street(W, HH)


def sequence(name, scene, cam0):
    """[(camera, previous camera, previous local_to_world or None, debug flags)] of one sequence."""
    f = np.array(cam0.front, dtype=np.float64)
    f /= np.linalg.norm(f)
    if name == "sky":
        sky = scenes.Camera(cam0.position, (0.2, 0.95, 0.1), W, HH)
        cams = [cam0, cam0.moved(tuple(0.5 * f)), cam0.moved(tuple(1.0 * f)), sky, sky, cam0.moved(tuple(1.5 * f))]
    elif name in ("moving", "blocks", "cut"):
        cams = [cam0.moved(tuple(0.5 * i * f)) for i in range(7 if name == "cut" else 5)]
    elif name == "ground":
        g = scenes.Camera((-62.0, 0.25, 3.0), (1.0, -0.02, -0.04), W, HH)
        fg = np.array(g.front, dtype=np.float64)
        fg /= np.linalg.norm(fg)
        cams = [g.moved(tuple(0.3 * i * fg)) for i in range(5)]
    else:
        raise ValueError(name)
    out = []
    for i, cam in enumerate(cams):
        last = None
        if name == "cut" and i in (3, 4):
            fc = np.array(cam.front, dtype=np.float64)
            fc /= np.linalg.norm(fc)
            last = scene.local_to_world.copy()
            last[:, 12:15] += 500.0 * fc                                  # glm column-major: the translation column
        out.append((cam, cams[i - 1] if i else cam, last, DBG_FORCE_BLOCKS if name == "blocks" else 0))
    return out


def _frame_inputs(scene, cam, last_cam, last):
    from chord_amd import lib as L
    view0, _ = L.make_views(last_cam)
    view, iv = L.make_views(cam, view0)
    objs = (L.fill_objects(scene, cam, last_cam, last) if last is not None else L.fill_objects(scene, cam, last_cam)).copy()
    return view, iv, objs


def run_sequence(name, out_path):
    """Render one sequence on a fresh context; every frame's results go to out_path (npz)."""
    from chord_amd import lib as L
    from chord_amd.renderer import VisibilityRenderer
    scene, cam0 = _scene()
    r = VisibilityRenderer(0)
    r.upload_scene(scene)
    r.allocate_gbuffer(W, HH)
    tiles = ((W + 63) // 64) * ((HH + 63) // 64)
    res = {}
    for i, (cam, last_cam, last, debug) in enumerate(sequence(name, scene, cam0)):
        view, iv, objs = _frame_inputs(scene, cam, last_cam, last)
        r.set_debug(debug)
        r.update_objects(objs)
        r.set_view(view, iv, H.ALL_FLAGS)
        r.render_frame()
        st = r.stats()
        mn, mx, rng = r.read_hzb(r.history_hzb())
        bins = np.zeros(tiles, np.uint32)
        ticks = np.zeros(tiles * 9, np.uint64)
        assert L.lib.chordvis_debug_tile_profile(r._ctx, 1, ticks.ctypes.data, bins.ctypes.data, tiles * 9) == 0
        res["vis%d" % i] = r.read_visibility()
        res["cmds%d" % i] = r.read_cmds(r.last_frame_cmds())
        res["counts%d" % i] = np.array([st["countInstanceCulled"], st["countStage0Visible"], st["countStage0Rejected"],
                                        st["countStage1Visible"], st["trianglesSubmitted"], st["overflow"]], np.int64)
        res["hzb%d" % i] = np.concatenate([mn.view(np.uint16).ravel(), mx.view(np.uint16).ravel(), rng.view(np.uint16).ravel()])
        res["bins%d" % i] = bins
    r.close()
    np.savez(out_path, **res)


def _child_main(out_dir):
    for name in SEQUENCES:
        run_sequence(name, os.path.join(out_dir, name + ".npz"))
    print(json.dumps({"ok": True}))


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    """{switch value: directory of the sequences' npz files}, one child interpreter per value."""
    out = {}
    for value in ("1", "8", "0"):
        d = str(tmp_path_factory.mktemp("touched_" + value))
        env = dict(os.environ)
        env["CHORDVIS_TILE_TOUCHED"] = value
        code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_touched_tiles as T; T._child_main(%r)" % (ROOT, os.path.join(ROOT, "tests"), d)
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, "child (CHORDVIS_TILE_TOUCHED=%s) failed:\n%s\n%s" % (value, p.stdout[-2000:], p.stderr[-4000:])
        out[value] = d
    return out


@pytest.mark.parametrize("name", SEQUENCES)
def test_touched_tile_passes_match_oracle_and_the_full_direct_form(runs, name):
    scene, cam0 = _scene()
    got = {v: np.load(os.path.join(d, name + ".npz")) for v, d in runs.items()}
    prev = None
    stage1 = []
    for i, (cam, last_cam, last, _) in enumerate(sequence(name, scene, cam0)):
        view, iv, objs = _frame_inputs(scene, cam, last_cam, last)
        want = orc.frame(scene.with_objects(objs), view, iv, H.ALL_FLAGS, prev_hzb_min=prev)
        want_hzb = np.concatenate([want["hzb_min"].view(np.uint16).ravel(), want["hzb_max"].view(np.uint16).ravel(),
                                   want["valid_range"].view(np.uint16).ravel()])
        for v, g in got.items():
            what = "%s frame %d, CHORDVIS_TILE_TOUCHED=%s" % (name, i, v)
            H.assert_vis_equal(g["vis%d" % i], want["vis"], W, HH, what)
            assert np.array_equal(g["cmds%d" % i], want["cmds"]), what + ": list 0"
            c = g["counts%d" % i]
            assert c[5] == 0 and c[4] == want["stats"].trianglesSubmitted, what
            if prev is not None:
                assert c[:4].tolist() == want["counts"].tolist(), what
            assert np.array_equal(g["hzb%d" % i], want_hzb), what + ": history HZB"
            assert np.array_equal(g["bins%d" % i], got["0"]["bins%d" % i]), what + ": second-pass bin counts"
        stage1.append((int(want["counts"][3]), int(np.count_nonzero(got["1"]["bins%d" % i]))))
        prev = want["hzb_min"]
    # what each sequence is there for
    touched = [t for _, t in stage1[1:]]
    if name == "sky":
        assert stage1[4] == (0, 0) and stage1[2][1] > 8, stage1
    elif name in ("moving", "blocks", "ground"):
        assert all(t > 8 for t in touched[1:]) and all(s <= 1024 for s, _ in stage1[1:]), stage1
    elif name == "cut":
        assert stage1[3][0] > 1024 and stage1[4][0] > 1024 and all(s <= 1024 for s, _ in stage1[5:]), stage1
