"""Meshlets of every shape the contract allows (up to 255 vertices / 128 triangles, tests/meshlet_shapes.py) through every set-up
kernel, the clipper, the depth-only pass, sharded frames and the resolve, bit for bit against the oracle.

Which kernel a test is there for, and the read-out that shows it ran:
  * record kernel (raster_setup_kernel; the vertex loop past 128 of raster_setup_body): test_record_kernel -- triangleRecords > 0,
    pixelBlocks == 0, chordvis_debug_setup_kernels == [0, 0];
  * block kernel and its hand-off of clusters of more than 128 vertices (raster_setup_blocks_kernel, leftCmds / leftCount):
    test_block_kernel_hands_large_clusters_over -- pixelBlockBytes > 0 and triangleRecords > 0 in one frame;
  * wide kernel (raster_setup_wide_kernel): test_wide_kernel -- chordvis_debug_setup_kernels()[1] == 1 on the frame whose clusters
    all go through the second pass, countStage1Visible == every cluster;
  * clipper (clip_triangle): the `near` cases of test_wide_kernel -- clipTriangles[0] > 0 (first pass, record kernel) and
    clipTriangles[1] > 0 (second pass, wide kernel), all of them triangles of clusters of more than 128 vertices
    (tests/test_meshlet_shapes.py) --, and test_clipper_with_the_separate_binner_launch (CHORDVIS_BIN_IN_SETUP=0, a child);
  * depth-only pass: test_depth_view -- depth_view_stats: overflow 0, pixelBlockBytes > 0 under FORCE_BLOCKS;
  * sharded: test_sharded_block_frames -- pixelBlockBytes and triangleRecords on the ranks;
  * resolve kernels: test_resolve.
tests/test_meshlet_shapes.py shows on the oracle alone that each scene has what its test needs."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import meshlet_shapes as MS
import orc
import spec_resolve_np as SR
from chord_amd import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORCE_BLOCKS, FORCE_HOT = 65536, 262144
_SCENES = {}


def setup(variant):
    """(scene, camera, view, iv) of a variant, object records filled for a still frame (the frame before: the same); made once --
    tests that change the object records work on scene.with_objects copies."""
    if variant not in _SCENES:
        from chord_amd import lib as L
        sc, cam = MS.scene(variant)
        view0, _ = L.make_views(cam)
        view, iv = L.make_views(cam, view0)
        L.fill_objects(sc, cam, cam)
        _SCENES[variant] = (sc, cam, view, iv)
    return _SCENES[variant]


def _renderer(sc, cam, view, iv, debug=0, cull_mode=0):
    from chord_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(0)
    if cull_mode:
        r.set_cull_mode(cull_mode)
    r.upload_scene(sc)
    r.allocate_gbuffer(cam.width, cam.height)
    r.set_view(view, iv, H.ALL_FLAGS)
    if debug:
        r.set_debug(debug)
    return r


def _setup_kernels(r):
    from chord_amd import lib as L
    wide = (C.c_uint32 * 2)()
    assert L.lib.chordvis_debug_setup_kernels(r._ctx, wide) == 0
    return list(wide)


def _check_frame(r, want, cam, what, counts=True):
    """Image, list 0, overflow, submitted triangles, stage counts and the history HZB (min, max, valid range) of the frame just rendered."""
    H.assert_vis_equal(r.read_visibility(), want["vis"], cam.width, cam.height, what)
    st = r.stats()
    assert st["overflow"] == 0, (what, st["overflow"])
    assert st["trianglesSubmitted"] == want["stats"].trianglesSubmitted, (what, st["trianglesSubmitted"], want["stats"].trianglesSubmitted)
    assert np.array_equal(r.read_cmds(r.last_frame_cmds()), want["cmds"]), what + ": list 0"
    if counts:
        got = [st["countInstanceCulled"], st["countStage0Visible"], st["countStage0Rejected"], st["countStage1Visible"]]
        assert got == want["counts"].tolist(), (what, got, want["counts"].tolist())
    mn, mx, rng = r.read_hzb(r.history_hzb())
    assert np.array_equal(mn, want["hzb_min"]), what + ": history HZB min"
    assert np.array_equal(mx, want["hzb_max"]), what + ": history HZB max"
    assert np.array_equal(rng, want["valid_range"]), what + ": history valid range"
    return st


@pytest.mark.parametrize("cull_mode", [0, 1], ids=["flat_cull", "bvh_cull"])
def test_record_kernel(gpu, cull_mode):
    """plain, frame 0 and the two-pass frame 1, set up by raster_setup_kernel; with the hierarchical cull as well (the helper's
    primitives carry BVH nodes)."""
    sc, cam, view, iv = setup("plain")
    assert sc.bvh_nodes is not None
    r = _renderer(sc, cam, view, iv, cull_mode=cull_mode)
    prev = None
    for frame in range(2):
        want = orc.frame(sc, view, iv, H.ALL_FLAGS, prev_hzb_min=prev)
        r.render_frame()
        st = _check_frame(r, want, cam, "plain frame %d, cull mode %d" % (frame, cull_mode), counts=frame > 0)
        assert st["triangleRecords"] > 0 and st["pixelBlocks"] == 0 and _setup_kernels(r) == [0, 0], (st["triangleRecords"], st["pixelBlocks"])
        assert want["stats"].trianglesSubmitted == sum(T for _, T in MS.SHAPES)
        prev = want["hzb_min"]
    r.close()


@pytest.mark.parametrize("debug", [FORCE_BLOCKS, FORCE_BLOCKS | FORCE_HOT], ids=["blocks", "hot_blocks"])
def test_block_kernel_hands_large_clusters_over(gpu, debug):
    """tiny under a forced dense launch: the clusters of at most 128 vertices become pixel blocks, those of more are handed to the
    record kernel through the left-over list -- two frames on one context (a left-over count that survived frame 0 would show in
    frame 1), then plain on the same context without the flag."""
    sc, cam, view, iv = setup("tiny")
    r = _renderer(sc, cam, view, iv, debug=debug)
    prev = None
    for frame in range(2):
        want = orc.frame(sc, view, iv, H.ALL_FLAGS, prev_hzb_min=prev)
        r.render_frame()
        st = _check_frame(r, want, cam, "tiny frame %d, debug %d" % (frame, debug), counts=frame > 0)
        assert st["pixelBlockBytes"] > 0 and st["pixelBlocks"] > 0, "no pixel blocks formed"
        assert st["triangleRecords"] > 0, "the clusters of more than 128 vertices left no records"
        prev = want["hzb_min"]
    psc, pcam, pview, piv = setup("plain")
    r.set_debug(0)
    r.upload_scene(psc)
    r.allocate_gbuffer(pcam.width, pcam.height)
    r.set_view(pview, piv, H.ALL_FLAGS)
    r.reset_history()
    want = orc.frame(psc, pview, piv, H.ALL_FLAGS)
    r.render_frame()
    st = _check_frame(r, want, pcam, "plain after the block frames", counts=False)
    assert st["pixelBlocks"] == 0
    r.close()


@pytest.mark.parametrize("variant", ["plain", "masked", "near"])
def test_wide_kernel(gpu, variant):
    """Frames 0 and 1 still; frame 2 a cut (meshlet_shapes.cut_last: every cluster is rejected by the first pass and goes
    through a second pass that the host still takes for light -- raster_setup_wide_kernel, a workgroup per cluster); frame 3 still
    again.  near: the clip triangles of the large clusters go through the record kernel's clipper in frames 0, 1, 3 and through
    the wide kernel's in frame 2."""
    sc, cam, view, iv, seq = _cut_sequence(variant)
    r = _renderer(sc, cam, view, iv)
    prev = None
    clip = []
    for frame, objs in enumerate(seq):
        fsc = sc.with_objects(objs)
        want = orc.frame(fsc, view, iv, H.ALL_FLAGS, prev_hzb_min=prev)
        r.update_objects(objs)
        r.render_frame()
        st = _check_frame(r, want, cam, "%s frame %d" % (variant, frame), counts=frame > 0)
        wide = _setup_kernels(r)
        assert wide[0] == 0, wide
        if frame == 2:
            assert wide[1] == 1, "pass 1 of the cut was not set up by the wide kernel"
            assert st["countStage0Visible"] == 0 and st["countStage1Visible"] == len(want["cmds"]) > 0
            assert max(int(sc.meshlets[c["meshletId"]]["vertexTriangleCount"]) & 0xFF for c in want["cmds"]) == 255
        clip.append(list(st["clipTriangles"]))
        if variant == "masked":
            assert want["stats"].fragmentsClipped > 0
        prev = want["hzb_min"]
    if variant == "near":
        assert clip[0][0] > 0 and clip[2][1] > 0 and clip[2][0] == 0, clip       # the clipper behind the record kernel, then behind the wide kernel
        assert sum(sum(c) for c in clip) > 0
    else:
        assert clip == [[0, 0]] * 4, clip
    r.close()


def _cut_sequence(variant):
    """(scene, camera, view, iv, [object records of the four frames]): still, still, the cut, still."""
    from chord_amd import lib as L
    sc, cam, view, iv = setup(variant)
    still = sc.objects.copy()
    cut = L.fill_objects(sc.with_objects(sc.objects.copy()), cam, cam, MS.cut_last(sc, cam)).copy()
    return sc, cam, view, iv, (still, still, cut, still)


def _near_child(out_path):
    """The near sequence on a fresh context in this process (whose CHORDVIS_BIN_IN_SETUP the parent chose); results to out_path."""
    sc, cam, view, iv, seq = _cut_sequence("near")
    r = _renderer(sc, cam, view, iv)
    res = {}
    for frame, objs in enumerate(seq):
        r.update_objects(objs)
        r.render_frame()
        st = r.stats()
        res["vis%d" % frame] = r.read_visibility()
        res["st%d" % frame] = np.array([st["overflow"], st["trianglesSubmitted"]] + list(st["clipTriangles"]) + _setup_kernels(r), np.int64)
    r.close()
    np.savez(out_path, **res)


def test_clipper_with_the_separate_binner_launch(gpu, tmp_path):
    """near's four frames with CHORDVIS_BIN_IN_SETUP=0 (read once per process: a child interpreter): the clip triangles of the large
    clusters are listed by the set-up kernels and clipped and binned by raster_clip_and_bin_large_kernel."""
    out = str(tmp_path / "near.npz")
    env = dict(os.environ)
    env["CHORDVIS_BIN_IN_SETUP"] = "0"
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_meshlet_shapes as T; T._near_child(%r)" % (ROOT, os.path.join(ROOT, "tests"), out)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, "child failed:\n%s\n%s" % (p.stdout[-2000:], p.stderr[-4000:])
    got = np.load(out)
    sc, cam, view, iv, seq = _cut_sequence("near")
    prev = None
    for frame, objs in enumerate(seq):
        want = orc.frame(sc.with_objects(objs), view, iv, H.ALL_FLAGS, prev_hzb_min=prev)
        prev = want["hzb_min"]
        H.assert_vis_equal(got["vis%d" % frame], want["vis"], cam.width, cam.height, "near frame %d, CHORDVIS_BIN_IN_SETUP=0" % frame)
        overflow, submitted, clip0, clip1, wide0, wide1 = got["st%d" % frame].tolist()
        assert overflow == 0 and submitted == want["stats"].trianglesSubmitted, (frame, overflow, submitted)
        assert (clip1 > 0 and clip0 == 0) if frame == 2 else clip0 > 0, (frame, clip0, clip1, wide0, wide1)


DEPTH_CASES = [("clamped", "plain", True, (0.0, 0.0), 0), ("clamped_biased", "plain", True, (-48.0, -1.25), 0),
               ("unclamped", "plain", False, (0.0, 0.0), 0), ("near_clamped", "near", True, (0.0, 0.0), 0),
               ("near_unclamped", "near", False, (0.0, 0.0), 0),
               ("tiny_blocks", "tiny", True, (0.0, 0.0), FORCE_BLOCKS), ("tiny_blocks_biased", "tiny", True, (-48.0, -1.25), FORCE_BLOCKS)]


@pytest.mark.parametrize("name,variant,clamp,bias,debug", DEPTH_CASES, ids=[c[0] for c in DEPTH_CASES])
def test_depth_view(gpu, name, variant, clamp, bias, debug):
    """One 256 x 256 depth-only view from the main camera's position: instance cull for the view, renderMeshDepth, against
    orc.instance_culling / orc.raster_depth."""
    from chord_amd import lib as L
    sc, cam, view, iv = setup(variant)
    dim = 256
    _, div = L.make_views(scenes.Camera(cam.position, cam.front, dim, dim))
    r = _renderer(sc, cam, view, iv, debug=debug)
    r.allocate_depth_views(dim, 1)
    r.set_instance_views(div)
    got_list = r.instance_culling_view(0)
    want_cmds = orc.instance_culling(sc, view, div, H.ALL_FLAGS)
    assert np.array_equal(r.read_cmds(got_list), want_cmds), name + ": culled list"
    assert max(int(sc.meshlets[c["meshletId"]]["vertexTriangleCount"]) & 0xFF for c in want_cmds) == 255
    target = r.render_mesh_depth(0, got_list, clamp, bias[0], bias[1])
    want_depth, wst = orc.raster_depth(sc, div, want_cmds, dim, dim, clamp, bias[0], bias[1])
    got_depth = r.read_depth(target)
    bad = np.nonzero(got_depth.view(np.uint32) != want_depth.view(np.uint32))[0]
    assert len(bad) == 0, "%s: %d texels differ, first %d: %r vs %r" % (name, len(bad), bad[0], got_depth[bad[0]], want_depth[bad[0]])
    st = r.depth_view_stats()
    assert st["overflow"] == 0 and (want_depth > 0).sum() > 1000
    if debug:
        assert st["pixelBlockBytes"] > 0 and st["triangleRecords"] > 0, (st["pixelBlockBytes"], st["triangleRecords"])
    if variant == "near":
        assert wst.trianglesClipped > 0
    # the main view is untouched by the depth pass
    r.render_frame()
    want = orc.frame(sc, view, iv, H.ALL_FLAGS)
    H.assert_vis_equal(r.read_visibility(), want["vis"], cam.width, cam.height, name + ": main view after the depth pass")
    r.close()


def test_sharded_block_frames(gpu):
    """tiny as a two-rank frame on one device under FORCE_BLOCKS: the rank-filtered list and the left-over list in one launch; every
    rank ends with the oracle's image."""
    sc, cam, view, iv = setup("tiny")
    w, h = cam.width, cam.height
    ctxs = H.sharded_contexts(sc, view, iv, w, h, H.ALL_FLAGS, 2, "checker", debug_of_rank=lambda rk: FORCE_BLOCKS)
    assert len(set(ctxs[0].tile_owners().tolist())) == 2
    prev = None
    for frame in range(2):
        want = orc.frame(sc, view, iv, H.ALL_FLAGS, prev_hzb_min=prev)
        prev = want["hzb_min"]
        H.sharded_frame(ctxs)
        for rk, r in enumerate(ctxs):
            what = "tiny frame %d rank %d of 2" % (frame, rk)
            H.assert_vis_equal(r.read_visibility(), want["vis"], w, h, what)
            st = r.stats()
            assert st["overflow"] == 0, what
            assert st["pixelBlockBytes"] > 0 and st["triangleRecords"] > 0, (what, st["pixelBlockBytes"], st["triangleRecords"])
            mn, mx, rng = r.read_hzb(r.history_hzb())
            assert np.array_equal(mn, want["hzb_min"]) and np.array_equal(mx, want["hzb_max"]) and np.array_equal(rng, want["valid_range"]), what
            if frame == 1:
                assert np.array_equal(r.read_cmds(r.last_frame_cmds()), want["cmds"]), what
    for r in ctxs:
        r.close()


def test_resolve(gpu):
    """chordvis_resolve_attributes of the plain frame against tests/spec_resolve_np.py: the resolve fetches the triangle's three
    vertices (position and uv) through the same local indices."""
    import torch
    sc, cam, view, iv = setup("plain")
    r = _renderer(sc, cam, view, iv)
    r.render_frame()
    want_frame = orc.frame(sc, view, iv, H.ALL_FLAGS)
    H.assert_vis_equal(r.read_visibility(), want_frame["vis"], cam.width, cam.height, "plain")
    names = ["barycentrics", "uv", "positionRS", "baryDdx", "baryDdy", "uvGrad", "motionVector"]
    out = r.resolve_attributes(names=names)
    torch.cuda.synchronize()
    got = {n: t.cpu().numpy().view(np.uint32) for n, t in out.items()}
    del out                   # (the tensors are recorded on the context's stream: they must be gone before close() destroys it)
    want = SR.resolve(sc, want_frame["vis"], want_frame["cmds"], view, iv, cam.width, cam.height, names=names)
    for n in names:
        wv = np.ascontiguousarray(want[n]).view(np.uint32)
        bad = np.argwhere(got[n].reshape(wv.shape) != wv)
        assert len(bad) == 0, "%s: %d values differ, first at %s" % (n, len(bad), bad[0])
    assert np.unique(got["uv"].reshape(-1, 2), axis=0).shape[0] > 1000, "real texture coordinates"
    r.close()
