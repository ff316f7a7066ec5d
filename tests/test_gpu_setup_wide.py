"""Light later passes set up by the wide kernel (raster_setup_wide_kernel: one 256-thread workgroup per cluster).

launch_raster takes the wide kernel for a later pass that the latest report calls light (the direct tile form); CHORDVIS_SETUP_WIDE=0
(read once per process) keeps raster_setup_kernel everywhere.  Sequences of config 3 frames at 1280 x 720 are rendered in two child
interpreters, one per value, every frame is held to the oracle -- image, list 0, the four stage counts, triangles, the history HZB's
min / max / valid range -- and the two runs to each other: largeRecords, clipTriangles, binEntries, trianglesSubmitted, overflow and
the second pass's per-tile bin counts.  Sequences:
  * sky: frames looking up into the empty sky -- a light second pass with no cluster at all -- between street views;
  * ground: a hand above the ground, moving; in frame 2 every object 'was' 500 m further down the view, so the ground near the
    camera goes through a second pass that the host still takes for light -- records across many tiles (large records) in
    the wide kernel;
  * floor / masked_floor: a camera just above a floor patch (opaque / alpha-tested), where frame 2's objects 'were' 500 m away:
    the clip triangles (near plane) go through a light second pass -- the clipper at the end of the wide kernel;
  * masked: config 3 with alpha-tested materials, moving -- the masked instantiation;
  * cut: light, then two heavy second passes (every object 'was' 500 m further down the view in the frame before), then light
    again -- the first heavy pass is still announced light, so the wide kernel gets a list of several thousand clusters.
Each child records which set-up kernel every pass launched (chordvis_debug_setup_kernels), and the test asserts that the frames a
sequence is there for ran the wide kernel (and that CHORDVIS_SETUP_WIDE=0 never does).  A list longer than TILE_DIRECT_MAX_CLUSTERS
is set up by the wide kernel one wave per cluster (RasterParams::wideMax); CHORDVIS_SETUP_WIDE=N above 1 moves that limit to N:
  * a third child runs every sequence with the limit out of reach, so the long lists of ground and cut (large records, thousands of
    clusters) go through the wide form itself;
  * the edge: cut is rendered with the limit at its light frame 2's own second-pass count n and at n - 1 -- that frame's list is then
    exactly at the limit (the wide form) and one above it (the wave form), the 1 024 / 1 025 edge of the product limit.
Depth-only views never take the wide kernel (their passes are not direct: launch_raster's laterOk)."""
import ctypes
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
SEQUENCES = ("sky", "ground", "floor", "masked_floor", "masked", "cut")
STATS = ("largeRecords", "clipTriangles", "binEntries", "trianglesSubmitted", "overflow")


def _scene(name):
    if name == "floor":
        return scenes.floor_under_camera(width=256, height=192)
    if name == "masked_floor":
        return scenes.masked_floor_under_camera()
    return scenes.config3_street(W, HH, masked=(name == "masked"))


def sequence(name, scene, cam0):
    """[(camera, previous camera, previous local_to_world or None)] of one sequence."""
    f = np.array(cam0.front, dtype=np.float64)
    f /= np.linalg.norm(f)
    if name == "sky":
        sky = scenes.Camera(cam0.position, (0.2, 0.95, 0.1), W, HH)
        cams = [cam0, cam0.moved(tuple(0.5 * f)), sky, sky, cam0.moved(tuple(1.0 * f))]
    elif name in ("masked", "cut"):
        cams = [cam0.moved(tuple(0.5 * i * f)) for i in range(7 if name == "cut" else 4)]
    elif name == "ground":
        g = scenes.Camera((-62.0, 0.25, 3.0), (1.0, -0.02, -0.04), W, HH)
        fg = np.array(g.front, dtype=np.float64)
        fg /= np.linalg.norm(fg)
        cams = [g.moved(tuple(0.3 * i * fg)) for i in range(5)]
    elif name in ("floor", "masked_floor"):
        cams = [cam0.moved((0.02 * i, 0.0, -0.05 * i)) for i in range(4)]
    else:
        raise ValueError(name)
    out = []
    for i, cam in enumerate(cams):
        last = None
        if (name == "cut" and i in (3, 4)) or (name == "ground" and i == 2) or (name in ("floor", "masked_floor") and i == 2):
            fc = np.array(cam.front, dtype=np.float64)
            fc /= np.linalg.norm(fc)
            last = scene.local_to_world.copy()
            last[:, 12:15] += 500.0 * fc                                  # glm column-major: the translation column
        out.append((cam, cams[i - 1] if i else cam, last))
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
    scene, cam0 = _scene(name)
    r = VisibilityRenderer(0)
    r.upload_scene(scene)
    r.allocate_gbuffer(cam0.width, cam0.height)
    tiles = ((cam0.width + 63) // 64) * ((cam0.height + 63) // 64)
    res = {}
    for i, (cam, last_cam, last) in enumerate(sequence(name, scene, cam0)):
        view, iv, objs = _frame_inputs(scene, cam, last_cam, last)
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
                                        st["countStage1Visible"]], np.int64)
        res["stats%d" % i] = np.array([sum(st[k]) if isinstance(st[k], list) else st[k] for k in STATS], np.int64)
        res["passes%d" % i] = np.array(st["largeRecords"] + st["clipTriangles"], np.int64)
        res["hzb%d" % i] = np.concatenate([mn.view(np.uint16).ravel(), mx.view(np.uint16).ravel(), rng.view(np.uint16).ravel()])
        res["bins%d" % i] = bins
        wide = (ctypes.c_uint32 * 2)()
        assert L.lib.chordvis_debug_setup_kernels(r._ctx, wide) == 0
        res["wide%d" % i] = np.array(list(wide), np.int64)
    r.close()
    np.savez(out_path, **res)


def _child_main(out_dir, names=SEQUENCES):
    for name in names:
        run_sequence(name, os.path.join(out_dir, name + ".npz"))
    print(json.dumps({"ok": True}))


NO_LIMIT = "100000000"


def _run_child(tmp_path_factory, value, names=SEQUENCES):
    d = str(tmp_path_factory.mktemp("setup_wide_" + value))
    env = dict(os.environ)
    env["CHORDVIS_SETUP_WIDE"] = value
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_setup_wide as T; T._child_main(%r, %r)" % (
        ROOT, os.path.join(ROOT, "tests"), d, tuple(names))
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, "child (CHORDVIS_SETUP_WIDE=%s) failed:\n%s\n%s" % (value, p.stdout[-2000:], p.stderr[-4000:])
    return d


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    """{switch value: directory of the sequences' npz files}, one child interpreter per value."""
    return {value: _run_child(tmp_path_factory, value) for value in ("1", "0", NO_LIMIT)}


def _oracle_frames(name):
    """[(camera, oracle frame)] of a sequence, in order (each frame with the history of the one before)."""
    scene, cam0 = _scene(name)
    out, prev = [], None
    for cam, last_cam, last in sequence(name, scene, cam0):
        view, iv, objs = _frame_inputs(scene, cam, last_cam, last)
        want = orc.frame(scene.with_objects(objs), view, iv, H.ALL_FLAGS, prev_hzb_min=prev)
        out.append((cam, want))
        prev = want["hzb_min"]
    return out


@pytest.mark.parametrize("name", SEQUENCES)
def test_wide_setup_matches_oracle_and_the_wave_form(runs, name):
    got = {v: np.load(os.path.join(d, name + ".npz")) for v, d in runs.items()}
    _purpose(name, _check_frames(name, got))


def _check_frames(name, got):
    """Every frame of every run against the oracle, and every run against the wave form's (CHORDVIS_SETUP_WIDE=0) counters and bins."""
    prev = None
    stage1 = []
    for i, (cam, want) in enumerate(_oracle_frames(name)):
        want_hzb = np.concatenate([want["hzb_min"].view(np.uint16).ravel(), want["hzb_max"].view(np.uint16).ravel(),
                                   want["valid_range"].view(np.uint16).ravel()])
        for v, g in got.items():
            what = "%s frame %d, CHORDVIS_SETUP_WIDE=%s" % (name, i, v)
            H.assert_vis_equal(g["vis%d" % i], want["vis"], cam.width, cam.height, what)
            assert np.array_equal(g["cmds%d" % i], want["cmds"]), what + ": list 0"
            s = dict(zip(STATS, g["stats%d" % i].tolist()))
            assert s["overflow"] == 0 and s["trianglesSubmitted"] == want["stats"].trianglesSubmitted, (what, s)
            if prev is not None:
                assert g["counts%d" % i].tolist() == want["counts"].tolist(), what
            assert np.array_equal(g["hzb%d" % i], want_hzb), what + ": history HZB"
        off = dict(zip(STATS, got["0"]["stats%d" % i].tolist()))
        for v in got:
            on = dict(zip(STATS, got[v]["stats%d" % i].tolist()))
            for k in STATS:
                assert on[k] == off[k], (name, i, v, k, on[k], off[k])
            assert np.array_equal(got[v]["passes%d" % i], got["0"]["passes%d" % i]), (name, i, v)
            assert np.array_equal(got[v]["bins%d" % i], got["0"]["bins%d" % i]), (name, i, v, "second-pass bin counts")
            assert got[v]["wide%d" % i][0] == 0 and (v != "0" or got[v]["wide%d" % i][1] == 0), (name, i, v, got[v]["wide%d" % i])
        stage1.append((int(want["counts"][3]), got["0"]["passes%d" % i].tolist(), int(max(g["wide%d" % i][1] for g in got.values()))))
        prev = want["hzb_min"]
    return stage1


def _purpose(name, stage1):
    """What each sequence is there for (stage1: [(second-pass clusters, [large0, large1, clip0, clip1], wide kernel launched)]).
    Frame 0 has no report yet and frame 1 sees frame 0's, which was not a direct pass: the first light-announced pass is frame 2's."""
    if name == "sky":
        assert stage1[3][0] == 0 and stage1[1][0] > 0 and stage1[3][2] == 1, stage1
    elif name == "ground":
        assert stage1[2][0] > 1024 and stage1[2][1][1] > 0 and stage1[2][2] == 1, stage1      # second-pass large records
    elif name in ("floor", "masked_floor"):
        assert 0 < stage1[2][0] <= 1024 and stage1[2][1][3] > 0 and stage1[2][2] == 1, stage1   # second-pass clip triangles
    elif name == "masked":
        assert all(0 < s <= 1024 for s, _, _ in stage1[1:]) and all(w == 1 for _, _, w in stage1[2:]), stage1
    elif name == "cut":
        assert stage1[3][0] > 1024 and stage1[4][0] > 1024 and all(s <= 1024 for s, _, _ in stage1[5:]), stage1
        assert stage1[3][2] == 1 and stage1[4][2] == 0, stage1          # announced light (the wide kernel, a long list), then heavy


@pytest.fixture(scope="module")
def edge_runs(gpu, tmp_path_factory):
    """cut rendered with the wide form's limit at the second-pass count n of its light frame 2, and at n - 1."""
    n = int(_oracle_frames("cut")[2][1]["counts"][3])
    assert n > 2, n
    return n, {value: _run_child(tmp_path_factory, value, ("cut",)) for value in ("0", str(n), str(n - 1))}


def test_wide_setup_at_the_edge_of_its_limit(edge_runs):
    n, runs = edge_runs
    got = {v: np.load(os.path.join(d, "cut.npz")) for v, d in runs.items()}
    _check_frames("cut", got)
    for v in (str(n), str(n - 1)):
        assert got[v]["wide2"].tolist() == [0, 1], (v, got[v]["wide2"])   # frame 2: the wide kernel, n clusters at / above its limit
