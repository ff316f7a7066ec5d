"""chordvis_query_bounds through the C ABI on the GPU.  Every comparison is word-for-word equality with
tests/spec_bounds_query_np.py (no tolerance anywhere): the result records, the visible list and its count -- against the chain of a
rendered frame, against a chain whose every level holds its own constant, without a chain, in both phases, at list lengths around
every step of the two kernel forms and of their grid-stride loops, at the capacity edges of the list output, for a caller's tensor on
another stream, on the ranks of a sharded frame, and for every refusal.  The two status bits are also held to the oracle directly."""
import ctypes as C

import numpy as np
import pytest

from chord_amd import lib as L, records as R

import bounds_scenes as B
import helpers as H
import spec_bounds_query_np as S

pytestmark = pytest.mark.gpu

BOXES = 2000
GUARD = 0x5A5A5A5A
LONG_LIST = 65536                                      # the switch between the two kernel forms (kernels_cull.hip HZB_CULL_LONG_LIST)
TWO_WORKGROUPS = 16777216                              # chordvis_set_debug: grids of at most two workgroups


def _frames(r, scene, cam_last, cam, first, second):
    """the two frames of bounds_scenes.two_frames on a context that holds the scene"""
    B.fill_for(scene, cam_last)
    r.update_objects(scene.objects)
    r.set_view(first[0], first[1], H.ALL_FLAGS)
    r.render_frame()
    B.fill_for(scene, cam, cam_last)
    r.update_objects(scene.objects)
    r.set_view(second[0], second[1], H.ALL_FLAGS)
    r.render_frame()


@pytest.fixture(scope="module")
def world(gpu):
    """small_test_scene at 160 x 96 rendered for two frames with a moved camera, the boxes, and the spec's answers for them against
    the chain the second frame left (read back once), in both phases and without a chain."""
    import orc
    from chord_amd.renderer import VisibilityRenderer
    w, h = 160, 96
    scene, cam_last, cam, first, second = B.two_frames(w, h)
    r = VisibilityRenderer(0)
    B.fill_for(scene, cam_last)
    r.upload_scene(scene)
    r.allocate_gbuffer(w, h)
    _frames(r, scene, cam_last, cam, first, second)
    hzb = r.history_hzb()
    chain = r.read_hzb(hzb)[0]
    queries, _ = B.make_boxes(cam, cam_last, BOXES, seed=11)
    view, iv = second
    want = {(phase, chained): S.query_bounds(view, iv, queries, phase, hzb.desc if chained else None, chain if chained else None)
            for phase in (0, 1) for chained in (False, True)}
    B.fill_for(scene, cam_last)
    f0 = orc.frame(scene, first[0], first[1], H.ALL_FLAGS)
    B.fill_for(scene, cam, cam_last)
    f1 = orc.frame(scene, view, iv, H.ALL_FLAGS, prev_hzb_min=f0["hzb_min"])
    out = dict(r=r, scene=scene, cams=(cam_last, cam), views=(first, second), hzb=hzb, chain=chain, queries=queries, want=want,
               oracle_chain=f1["hzb_min"], oracle_vis=f1["vis"])
    yield out
    r.close()


def _same(got, want, what):
    res, vis, n = got
    wres, wvis, wn = want
    if res is not None:
        a, b = res.view(np.uint32).reshape(-1, 4), wres.view(np.uint32).reshape(-1, 4)
        assert a.shape == b.shape, (what, a.shape, b.shape)
        bad = np.flatnonzero((a != b).any(axis=1))
        assert len(bad) == 0, "%s: %d records differ; first %d got %s want %s" % (what, len(bad), bad[0], a[bad[0]], b[bad[0]])
    if n is not None:
        assert n == wn, "%s: visible count %d, spec %d" % (what, n, wn)
    if vis is not None:
        assert len(vis) == wn and np.array_equal(vis, wvis), "%s: the visible list's indices or order" % what


def _tiled(want, count):
    """the spec's answer for the boxes repeated to `count` queries"""
    res, vis, _ = want
    n = len(res)
    seen = np.zeros(n, dtype=bool)
    seen[vis] = True
    idx = np.flatnonzero(np.resize(seen, count)).astype(np.uint32)
    return np.resize(res, count), idx, len(idx)


# ---- 1. the answers -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("phase", (1, 0))
def test_rendered_chain_equals_the_spec_and_the_oracle(world, phase):
    r, q = world["r"], world["queries"]
    got = r.query_bounds(q, world["hzb"], phase)
    _same(got, world["want"][phase, True], "phase %d, history chain" % phase)
    _same(r.query_bounds(q, None, phase), world["want"][phase, False], "phase %d, no chain" % phase)
    # the oracle, directly: its own chain of the same two frames, the equivalent one-meshlet scene
    view, iv = world["views"][1]
    inside, seen = B.oracle_answers(q, view, iv, phase, world["hzb"].desc, world["oracle_chain"])
    st = got[0]["status"]
    assert np.array_equal((st & R.BOUNDS_IN_FRUSTUM) != 0, inside)
    assert np.array_equal(((st & R.BOUNDS_UNOCCLUDED) != 0)[inside], seen[inside])
    assert not got[0][~inside].view(np.uint8).any()
    cls = S.classes(inside, st, S.top_level(160, 96) - 1)
    assert all(cls[k].any() for k in ("frustum_culled", "occluded", "visible", "near", "empty_rect", "top_levels")), {k: int(v.sum()) for k, v in cls.items()}
    if phase == 0:
        assert (cls["offscreen"] & inside).any()


def test_level_constant_chain_at_129x67(gpu):
    import orc
    from chord_amd.renderer import VisibilityRenderer
    w, h = 129, 67
    scene, cam_last, cam, _, (view, iv) = B.two_frames(w, h)
    queries, _ = B.make_boxes(cam, cam_last, BOXES, seed=12)
    desc = orc.hzb_desc(w, h)
    chain = B.level_chain(desc, S.tests(view, iv, queries, 1)[2])
    r = VisibilityRenderer(0)
    r.upload_scene(scene)
    r.allocate_gbuffer(w, h)
    r.set_view(view, iv, 0)                            # (no cull flag set: a query tests all the same)
    r.upload_history_hzb(chain)
    hzb = r.history_hzb()
    assert bytes(hzb.desc) == bytes(desc)
    for phase in (1, 0):
        want = S.query_bounds(view, iv, queries, phase, desc, chain)
        got = r.query_bounds(queries, hzb, phase)
        _same(got, want, "level chain, phase %d" % phase)
        levels = (got[0]["status"] >> R.BOUNDS_LEVEL_SHIFT) & R.BOUNDS_LEVEL_MASK
        assert set(levels.tolist()) == set(range(S.top_level(w, h) + 1))
        inside, seen = B.oracle_answers(queries, view, iv, phase, desc, chain)
        assert np.array_equal((got[0]["status"] & R.BOUNDS_IN_FRUSTUM) != 0, inside)
        assert np.array_equal(((got[0]["status"] & R.BOUNDS_UNOCCLUDED) != 0)[inside], seen[inside])
    r.close()


def test_no_scene_and_no_gbuffer_are_needed(gpu, world):
    from chord_amd.renderer import VisibilityRenderer
    view, iv = world["views"][1]
    r = VisibilityRenderer(0)
    r.set_view(view, iv, H.ALL_FLAGS)
    _same(r.query_bounds(world["queries"], None, 1), world["want"][1, False], "a bare context")
    r.close()


# ---- 2. list lengths ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", (0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, LONG_LIST, LONG_LIST + 1))
def test_counts(world, count):
    r = world["r"]
    q = np.resize(world["queries"], count)
    _same(r.query_bounds(q, world["hzb"], 1), _tiled(world["want"][1, True], count), "%d queries" % count)
    if count in (9, 257, LONG_LIST + 1):
        _same(r.query_bounds(q, world["hzb"], 0), _tiled(world["want"][0, True], count), "%d queries, phase 0" % count)


def test_a_list_longer_than_the_grid(world):
    """one count above the cap of the one-query-per-thread form's grid (two 1 024-thread workgroups per CU): its workgroups take a
    second step.  (The eight-lane form's cap -- 32 workgroups of 32 queries per CU -- lies above the lists it is given.)"""
    import torch
    r = world["r"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    count = cus * 2 * 1024 + 1031
    assert cus * 32 * 32 >= LONG_LIST
    q = np.resize(world["queries"], count)
    _same(r.query_bounds(q, world["hzb"], 1), _tiled(world["want"][1, True], count), "%d queries" % count)


@pytest.mark.parametrize("count", (257, BOXES, LONG_LIST + 4500))
def test_grid_stride_loops_of_both_forms_and_of_the_scatter(world, count):
    r = world["r"]
    q = np.resize(world["queries"], count)
    r.set_debug(TWO_WORKGROUPS)
    try:
        for phase in (1, 0):
            _same(r.query_bounds(q, world["hzb"], phase), _tiled(world["want"][phase, True], count), "%d queries on two workgroups, phase %d" % (count, phase))
    finally:
        r.set_debug(0)


# ---- 3. outputs ---------------------------------------------------------------------------------------------------------------

def _device(values, dtype=np.uint32):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(values, dtype=dtype).view(np.int32).copy()).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def test_capacity_edges_leave_the_guard_word_alone(world):
    import torch
    r = world["r"]
    _, wvis, wn = world["want"][1, True]
    q = _device(world["queries"].view(np.uint32))
    assert wn > 2
    for capacity in (0, wn - 1, wn):
        out = _device(np.full(capacity + 2, GUARD))
        base = out.data_ptr()
        rc = L.lib.chordvis_query_bounds(r._ctx, C.byref(world["hzb"]), 1, q.data_ptr(), BOXES, None,
                                         base + 4 if capacity else None, base, capacity)
        assert rc == L.OK, r.last_error()
        r.sync()
        host = out.cpu().numpy().view(np.uint32)
        assert host[0] == wn, "the count word holds the full number"
        assert np.array_equal(host[1:1 + capacity], wvis[:capacity])
        assert host[1 + capacity] == GUARD, "a word behind `capacity` was written"


def test_results_only_list_only_and_a_tensor_on_another_stream(world):
    import torch
    r = world["r"]
    want = world["want"][1, True]
    res, vis, n = r.query_bounds(world["queries"], world["hzb"], 1, capacity=0, want_count=False)
    assert n is None and len(vis) == 0
    _same((res, None, None), want, "results only")
    res, vis, n = r.query_bounds(world["queries"], world["hzb"], 1, want_results=False)
    assert res is None
    _same((None, vis, n), want, "list only")
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        staged = torch.from_numpy(world["queries"].view(np.uint8).copy()).to(dev, non_blocking=True)
        q = staged.clone()                             # made on the side stream: the call has to wait for it
        got = r.query_bounds(q, world["hzb"], 1)
    _same(got, want, "a CUDA tensor made on another stream")
    del q, staged
    torch.cuda.synchronize()


# ---- 4. the frame, and a sharded frame ----------------------------------------------------------------------------------------

def _third_frame(r):
    # (the device has finished the second frame in both contexts: which raster kernels a frame launches follows the bin lengths the
    # last FINISHED frame reported to the host, and the queries' read-backs waited for it in one context only)
    r.sync()
    r.render_frame()
    st = {k: v for k, v in r.stats().items() if not k.startswith("ms") and k not in ("framesTimed", "stampsPerFrame")}
    return r.read_visibility(), r.read_cmds(r.last_frame_cmds()), st


def test_queries_leave_the_frame_alone(world):
    from chord_amd.renderer import VisibilityRenderer
    scene = world["scene"]
    (cam_last, cam), (first, second) = world["cams"], world["views"]
    got = []
    for asked in (False, True):
        r = VisibilityRenderer(0)
        B.fill_for(scene, cam_last)
        r.upload_scene(scene)
        r.allocate_gbuffer(160, 96)
        _frames(r, scene, cam_last, cam, first, second)
        if asked:
            hzb = r.history_hzb()
            for phase in (0, 1):
                _same(r.query_bounds(world["queries"], hzb, phase), world["want"][phase, True], "before the third frame")
                r.query_bounds(world["queries"], None, phase)
        got.append(_third_frame(r))
        r.close()
    assert np.array_equal(got[0][0], got[1][0]), "visibility words"
    assert np.array_equal(got[0][1], got[1][1]), "the frame's command list"
    assert got[0][2] == got[1][2], "stats"


def test_sharded_ranks_answer_as_the_unsharded_context(world):
    scene = world["scene"]
    (cam_last, cam), (first, second) = world["cams"], world["views"]
    B.fill_for(scene, cam_last)
    ctxs = H.sharded_contexts(scene, first[0], first[1], 160, 96, H.ALL_FLAGS, 2)
    H.sharded_frame(ctxs, sharded_cull=False)
    B.fill_for(scene, cam, cam_last)
    for r in ctxs:
        r.update_objects(scene.objects)
        r.set_view(second[0], second[1], H.ALL_FLAGS)
    H.sharded_frame(ctxs)
    for rk, r in enumerate(ctxs):
        hzb = r.history_hzb()
        for phase in (1, 0):
            _same(r.query_bounds(world["queries"], hzb, phase), world["want"][phase, True], "rank %d, phase %d" % (rk, phase))
    for r in ctxs:
        r.close()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_rule_and_the_context_renders_on(world):
    import orc
    from chord_amd.renderer import VisibilityRenderer
    scene = world["scene"]
    (cam_last, cam), (first, (view, iv)) = world["cams"], world["views"]
    r = VisibilityRenderer(0)                          # (a context of its own: it renders a third frame at the end)
    B.fill_for(scene, cam_last)
    r.upload_scene(scene)
    r.allocate_gbuffer(160, 96)
    _frames(r, scene, cam_last, cam, first, (view, iv))
    hzb = r.history_hzb()
    q = _device(world["queries"].view(np.uint32))
    res = _device(np.zeros(4 * BOXES))
    out = _device(np.zeros(BOXES + 1))
    qp, rp, vp, cp = q.data_ptr(), res.data_ptr(), out.data_ptr() + 4, out.data_ptr()

    def refused(ctx, words, *args):
        assert L.lib.chordvis_query_bounds(ctx._ctx, *args) == L.E_INVALID, words
        msg = ctx.last_error()
        assert "query_bounds" in msg and all(w in msg for w in words), msg

    bare = VisibilityRenderer(0)
    refused(bare, ("no view",), None, 1, qp, BOXES, rp, vp, cp, BOXES)
    bare.close()
    h = C.byref(hzb)
    refused(r, ("phase",), h, 2, qp, BOXES, rp, vp, cp, BOXES)
    refused(r, ("phase",), h, -1, qp, BOXES, rp, vp, cp, BOXES)
    refused(r, ("deviceQueries", "NULL"), h, 1, None, BOXES, rp, vp, cp, BOXES)
    refused(r, ("outputs", "NULL"), h, 1, qp, BOXES, None, None, None, 0)
    refused(r, ("deviceVisible", "capacity"), h, 1, qp, BOXES, rp, None, cp, 4)
    no_texels = L.HZB()
    C.memmove(C.byref(no_texels), C.byref(hzb), C.sizeof(L.HZB))
    no_texels.minTexels = None
    refused(r, ("minTexels",), C.byref(no_texels), 1, qp, BOXES, rp, vp, cp, BOXES)
    other = L.HZB()
    C.memmove(C.byref(other), C.byref(hzb), C.sizeof(L.HZB))
    other.desc = L.hzb_desc(320, 192)
    refused(r, ("desc", "chordvis_hzb_desc"), C.byref(other), 1, qp, BOXES, rp, vp, cp, BOXES)
    C.memmove(C.byref(other), C.byref(hzb), C.sizeof(L.HZB))
    other.desc.mipCount += 1
    refused(r, ("desc", "chordvis_hzb_desc"), C.byref(other), 1, qp, BOXES, rp, vp, cp, BOXES)
    refused(r, ("16-byte",), h, 1, qp + 4, BOXES - 1, rp, vp, cp, BOXES)
    # nothing was written by a refused call, and the count of an empty list is written
    assert not res.cpu().numpy().any() and not out.cpu().numpy().any()
    out.fill_(7)
    assert L.lib.chordvis_query_bounds(r._ctx, h, 1, None, 0, None, None, cp, 0) == L.OK
    r.sync()
    assert out.cpu().numpy()[0] == 0 and out.cpu().numpy()[1] == 7
    # the context is as good as before: the same view's next frame is the oracle's
    want = orc.frame(scene, view, iv, H.ALL_FLAGS, prev_hzb_min=world["oracle_chain"])
    r.render_frame()
    assert np.array_equal(r.read_visibility(), want["vis"])
    r.close()
