"""chordvis_bin_bounds through the C ABI on the GPU.  Every comparison is word-for-word equality with tests/spec_bounds_tiles_np.py (no
tolerance anywhere) of all four outputs -- tile counts, tile items (with the words the call must not write), tile depth bounds and
totals: on caller-owned synthetic, all-zero and all-one images with hand-made records aimed at the edges of the pair test, at three
image sizes and all four tile sizes; at record counts around every chunk and workgroup step, with and without the debug bit; with
so many records across one block that its candidate list fills and is flushed mid-stream; beyond maxPerTile; with generated boxes and the far side; on a rendered frame behind chordvis_query_bounds in both phases, which it must
leave untouched; on the ranks of a sharded frame; and for every refusal."""
import ctypes as C
import functools

import numpy as np
import pytest

from chord_amd import lib as L, records as R, scenes

import bounds_scenes as B
import bounds_tiles_cases as K
import helpers as H
import spec_bounds_query_np as Q
import spec_bounds_tiles_np as S

pytestmark = pytest.mark.gpu

SIZES = ((64, 64), (160, 96), (641, 377))
TILES = (8, 16, 32, 64)
NEAR, FAR = R.BOUNDS_TILES_NEAR, R.BOUNDS_TILES_FAR
SMALL_STEPS = 33554432                                 # chordvis_set_debug: two workgroups, record chunks of 64


@functools.lru_cache(maxsize=None)
def _words(w, h, kind):
    """The image `kind` ("synthetic", "zeros", "ones") as visibility words; the low words are random: nothing may look at them."""
    depth = {"zeros": np.zeros, "ones": np.ones}[kind]((h, w), dtype=np.float32) if kind != "synthetic" else H.synthetic_depth(w, h, 6)
    low = np.random.default_rng([w, h, 41]).integers(0, 1 << 32, w * h, dtype=np.uint32)
    words = H.synthetic_words(depth, low)
    words.setflags(write=False)
    return words


@pytest.fixture(scope="module")
def contexts(gpu):
    """Per image size a context WITHOUT a scene whose visibility image is a caller-owned tensor, and the view of that size."""
    from chord_amd.renderer import VisibilityRenderer
    made = {}

    def get(w, h):
        if (w, h) not in made:
            _, _, view, iv = H.setup_scene(lambda: scenes.small_test_scene(w, h))
            r = VisibilityRenderer(0)
            img = H.CallerVisibility(r, w, h)
            r.set_view(view, iv, H.ALL_FLAGS)
            made[w, h] = (r, img, view, iv)
        return made[w, h]
    yield get
    for r, _, _, _ in made.values():
        r.close()


def _same(got, want, what):
    for k in ("counts", "depth", "totals", "items"):
        if got[k] is None:
            continue
        a, b = got[k], want[k]
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        if not np.array_equal(a, b):
            at = np.argwhere(a != b)[0]
            raise AssertionError("%s: %s differs in %d words; first at %s: got %#x want %#x" % (what, k, int((a != b).sum()), at.tolist(), int(a[tuple(at)]), int(b[tuple(at)])))


# ---- 1. synthetic images, hand-made records ----------------------------------------------------------------------------------

@pytest.mark.parametrize("T", TILES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_handmade_records_on_synthetic_and_constant_images(contexts, size, T):
    w, h = size
    r, img, _, _ = contexts(w, h)
    cap = 16
    rejected_by_depth = 0
    for kind in ("synthetic", "zeros", "ones"):
        words = _words(w, h, kind)
        img.write(words)
        results = K.handmade_results(w, h, T, S.tile_depth(words, w, h, T), 257, seed=1)
        assert set((results["status"][::3] & 31).tolist()) == set(range(32)), "every combination of the status bits"
        plain = S.bin_bounds(words, w, h, results, T, cap, 0)
        for flags in (0, NEAR):
            want = plain if flags == 0 else S.bin_bounds(words, w, h, results, T, cap, flags)
            got = r.bin_bounds(results, None, T, cap, 1, flags)
            assert got["tiles"] == S.tile_count(w, h, T)[1:]
            _same(got, want, "%dx%d T %d %s flags %d" % (w, h, T, kind, flags))
            if flags and kind != "zeros":
                rejected_by_depth += int(plain["totals"][1]) - int(want["totals"][1])
        if kind == "zeros":
            assert np.array_equal(S.bin_bounds(words, w, h, results, T, cap, NEAR)["counts"], plain["counts"]), "nothing lies behind an empty tile"
    assert rejected_by_depth > 0, "the near side rejected nothing"


@pytest.mark.parametrize("count", (0, 1, 63, 64, 65, 257, 1000))
def test_counts_with_and_without_the_debug_bit(contexts, count):
    w, h = 160, 96
    r, img, _, _ = contexts(w, h)
    words = _words(w, h, "synthetic")
    img.write(words)
    cap = 8
    try:
        for T in TILES:
            results = K.handmade_results(w, h, T, S.tile_depth(words, w, h, T), count, seed=2)
            want = S.bin_bounds(words, w, h, results, T, cap, NEAR)
            for debug in (0, SMALL_STEPS):
                r.set_debug(debug)
                _same(r.bin_bounds(results, None, T, cap, 1, NEAR), want, "%d records, T %d, debug %d" % (count, T, debug))
            if count == 0:
                assert not want["counts"].any() and not want["totals"].any() and (want["items"] == S.FILL).all()
    finally:
        r.set_debug(0)


@pytest.mark.parametrize("T", TILES)
def test_a_candidate_list_that_fills_is_flushed_mid_stream(contexts, T):
    """2 000 records that all take part, 1 500 of them across the whole screen: every block's candidate list (512 slots) fills before
    the stream ends, at both chunk sizes, and is flushed with the tiles' counts and the ascending order carried on -- with lists far
    shorter and longer than what a tile keeps."""
    w, h = 160, 96
    r, img, _, _ = contexts(w, h)
    words = _words(w, h, "synthetic")
    img.write(words)
    results = K.piled_results(w, h, T, S.tile_depth(words, w, h, T), 2000, seed=5)
    assert K.midstream_flushes(results, w, h, K.CHUNK) >= 2 and K.midstream_flushes(results, w, h, K.CHUNK_DEBUG) >= 2
    try:
        for cap in (16, 2400):
            for flags in (0, NEAR):
                want = S.bin_bounds(words, w, h, results, T, cap, flags)
                assert want["counts"].max() > K.CANDIDATE_SLOTS and (want["totals"][2] == len(want["counts"])) == (cap == 16)
                for debug in (0, SMALL_STEPS):
                    r.set_debug(debug)
                    _same(r.bin_bounds(results, None, T, cap, 1, flags), want, "piled records, T %d, maxPerTile %d, flags %d, debug %d" % (T, cap, flags, debug))
    finally:
        r.set_debug(0)


def test_ten_overlapping_records_with_room_for_four(contexts):
    w, h = 160, 96
    r, img, _, _ = contexts(w, h)
    words = _words(w, h, "synthetic")
    img.write(words)
    results = np.zeros(14, dtype=R.BOUNDS_RESULT)
    results["status"] = R.BOUNDS_IN_FRUSTUM | R.BOUNDS_UNOCCLUDED
    results["status"][[1, 4, 7, 12]] = (R.BOUNDS_IN_FRUSTUM, R.BOUNDS_UNOCCLUDED, 0, R.BOUNDS_NEAR)      # these four take no part
    results["nearestZ"] = 1.0
    results["rect"] = (40, 40, 41, 41)                                      # pixels of tile (2, 2) at T = 16
    for debug in (0, SMALL_STEPS):
        r.set_debug(debug)
        got = r.bin_bounds(results, None, 16, 4, 1, NEAR, item_fill=0x5A5A5A5A)
        r.set_debug(0)
        t = 2 * got["tiles"][0] + 2
        assert got["counts"][t] == 10 and got["counts"].sum() == 10
        assert got["items"][t].tolist() == [0, 2, 3, 5], "the first four, ascending"
        others = np.delete(got["items"], t, axis=0)
        assert (others == 0x5A5A5A5A).all(), "a word of another tile's items was written"
        assert got["totals"].tolist() == [10, 10, 1, 10]
        # room for exactly ten and for more: the words behind the ten stay
        got = r.bin_bounds(results, None, 16, 12, 1, 0, item_fill=0x5A5A5A5A)
        assert got["items"][t].tolist() == [0, 2, 3, 5, 6, 8, 9, 10, 11, 13] + [0x5A5A5A5A] * 2 and got["totals"].tolist() == [10, 10, 0, 10]


def test_each_output_alone_and_tensors_on_the_device(contexts):
    import torch
    w, h, T, cap = 160, 96, 32, 6
    r, img, _, _ = contexts(w, h)
    words = _words(w, h, "synthetic")
    img.write(words)
    results = K.handmade_results(w, h, T, S.tile_depth(words, w, h, T), 300, seed=4)
    want = S.bin_bounds(words, w, h, results, T, cap, NEAR)
    only = dict(want_counts=False, want_depth=False, want_totals=False)
    _same(r.bin_bounds(results, None, T, 0, 1, NEAR, **dict(only, want_counts=True)), want, "counts alone")
    _same(r.bin_bounds(results, None, T, 0, 1, NEAR, **dict(only, want_depth=True)), want, "depth alone")
    got = r.bin_bounds(results, None, T, 0, 1, NEAR, **dict(only, want_totals=True))
    assert got["totals"][[0, 1, 3]].tolist() == want["totals"][[0, 1, 3]].tolist() and got["totals"][2] == (want["counts"] > 0).sum()
    _same(r.bin_bounds(results, None, T, cap, 1, NEAR, **only), want, "items alone")
    _same(r.bin_bounds(np.zeros(0, dtype=R.BOUNDS_RESULT), None, T, 0, 1, 0, **dict(only, want_depth=True)), want, "depth alone, no records")
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        t = torch.from_numpy(results.view(np.uint8).copy()).to(dev, non_blocking=True).clone()   # made on another stream: the call waits
        _same(r.bin_bounds(t, None, T, cap, 1, NEAR), want, "a CUDA tensor made on another stream")
    del t
    torch.cuda.synchronize()


# ---- 2. generated boxes and the far side -------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ("synthetic", "zeros"))
def test_generated_boxes_near_and_far_on_a_synthetic_and_an_empty_image(contexts, kind):
    w, h = K.RENDERED_SIZE
    r, img, _, _ = contexts(w, h)
    _, cam_last, cam, _, (view, iv) = B.two_frames(w, h)
    r.set_view(view, iv, 0)
    queries, _ = B.make_boxes(cam, cam_last, 500, seed=31)
    words = _words(w, h, kind)
    img.write(words)
    for phase in (1, 0):
        results = Q.query_bounds(view, iv, queries, phase)[0]             # (no chain: everything on screen is unoccluded)
        farz = S.far_z(view, iv, queries, phase, results["status"])
        for T, flags in ((8, NEAR | FAR), (64, FAR)):
            want = S.bin_bounds(words, w, h, results, T, 32, flags, farz)
            for debug in (0, SMALL_STEPS):
                r.set_debug(debug)
                got = r.bin_bounds(results, queries, T, 32, phase, flags)
                r.set_debug(0)
                _same(got, want, "%s image, phase %d, T %d, flags %d, debug %d" % (kind, phase, T, flags, debug))
            if kind == "zeros":
                takes_part = S.participates(results)
                near_records = int((takes_part & ((results["status"] & R.BOUNDS_NEAR) != 0)).sum())
                assert 0 < near_records < takes_part.sum() and (want["counts"] == near_records).all(), "an empty tile keeps the NEAR records only"
    r.set_view(*contexts(w, h)[2:], H.ALL_FLAGS)


# ---- 3. a rendered frame ------------------------------------------------------------------------------------------------------

def _two_frames(r, scene, cam_last, cam, first, second):
    B.fill_for(scene, cam_last)
    r.update_objects(scene.objects)
    r.set_view(first[0], first[1], H.ALL_FLAGS)
    r.render_frame()
    B.fill_for(scene, cam, cam_last)
    r.update_objects(scene.objects)
    r.set_view(second[0], second[1], H.ALL_FLAGS)
    r.render_frame()


def _frame_state(r):
    st = {k: v for k, v in r.stats().items() if not k.startswith("ms") and k not in ("framesTimed", "stampsPerFrame")}
    return r.read_visibility().tobytes(), r.read_cmds(r.last_frame_cmds()).tobytes(), r.read_hzb(r.history_hzb())[0].tobytes(), st


def test_rendered_frame_behind_query_bounds_and_the_frame_is_left_alone(gpu):
    import torch
    from chord_amd.renderer import VisibilityRenderer
    w, h = K.RENDERED_SIZE
    T, cap = K.RENDERED_TILE, K.RENDERED_MAX_PER_TILE
    scene, cam_last, cam, first, second, queries = K.rendered_boxes()
    view, iv = second
    r = VisibilityRenderer(0)
    B.fill_for(scene, cam_last)
    r.upload_scene(scene)
    r.allocate_gbuffer(w, h)
    _two_frames(r, scene, cam_last, cam, first, second)
    hzb = r.history_hzb()
    before = _frame_state(r)
    words = np.frombuffer(before[0], dtype=np.uint64)
    dev = torch.device("cuda", 0)
    for phase in (1, 0):
        results = r.query_bounds(queries, hzb, phase)[0]
        farz = S.far_z(view, iv, queries, phase, results["status"])
        want = S.bin_bounds(words, w, h, results, T, cap, NEAR | FAR, farz)
        assert want["totals"][2] > 0 and (want["counts"] < cap).any()
        _same(r.bin_bounds(results, queries, T, cap, phase, NEAR | FAR), want, "rendered frame, phase %d" % phase)
        # the same, chained on the device: the results never leave it
        q = torch.from_numpy(queries.view(np.uint8).copy()).to(dev)
        res = torch.zeros(4 * len(queries), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        assert L.lib.chordvis_query_bounds(r._ctx, C.byref(hzb), phase, q.data_ptr(), len(queries), res.data_ptr(), None, None, 0) == L.OK, r.last_error()
        for debug in (0, SMALL_STEPS):
            r.set_debug(debug)
            _same(r.bin_bounds(res, q, T, cap, phase, NEAR | FAR), want, "rendered frame chained on the device, phase %d, debug %d" % (phase, debug))
            r.set_debug(0)
        for T2 in (8, 64):
            _same(r.bin_bounds(res, q, T2, cap, phase, NEAR | FAR), S.bin_bounds(words, w, h, results, T2, cap, NEAR | FAR, farz), "rendered frame, T %d" % T2)
        # (the wrapper recorded the context's stream on both tensors: they go back to the allocator while that stream exists)
        del q, res
        torch.cuda.synchronize()
    after = _frame_state(r)
    assert before[0] == after[0], "the visibility image"
    assert before[1] == after[1], "the frame's command list"
    assert before[2] == after[2], "the history chain"
    assert before[3] == after[3], "chordvis_stats"
    r.close()


def test_sharded_ranks_bin_the_whole_resolved_image(gpu):
    w, h = K.RENDERED_SIZE
    scene, cam_last, cam, first, second, queries = K.rendered_boxes()
    view, iv = second
    B.fill_for(scene, cam_last)
    ctxs = H.sharded_contexts(scene, first[0], first[1], w, h, H.ALL_FLAGS, 2)
    H.sharded_frame(ctxs, sharded_cull=False)
    B.fill_for(scene, cam, cam_last)
    for r in ctxs:
        r.update_objects(scene.objects)
        r.set_view(view, iv, H.ALL_FLAGS)
    H.sharded_frame(ctxs)
    images = [r.read_visibility() for r in ctxs]
    assert np.array_equal(images[0], images[1])
    for rk, r in enumerate(ctxs):
        results = r.query_bounds(queries, r.history_hzb(), 1)[0]
        farz = S.far_z(view, iv, queries, 1, results["status"])
        want = S.bin_bounds(images[rk], w, h, results, 16, 100, NEAR | FAR, farz)
        _same(r.bin_bounds(results, queries, 16, 100, 1, NEAR | FAR), want, "rank %d" % rk)
    for r in ctxs:
        r.close()


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_rule(contexts):
    import torch
    from chord_amd.renderer import VisibilityRenderer
    w, h = 160, 96
    r, img, view, iv = contexts(w, h)
    words = _words(w, h, "synthetic")
    img.write(words)
    dev = torch.device("cuda", 0)
    n = 40
    res = torch.zeros(4 * n + 4, dtype=torch.int32, device=dev)
    qry = torch.zeros(40 * n + 4, dtype=torch.int32, device=dev)
    tiles = S.tile_count(w, h, 8)[0]
    outs = [torch.full((k,), 0x11111111, dtype=torch.int32, device=dev) for k in (tiles, tiles * 4, tiles * 2, 4)]
    torch.cuda.synchronize()
    full = L.BoundsTiles(*(t.data_ptr() for t in outs))

    def refused(ctx, words_, desc, results, queries, count, out):
        rc = L.lib.chordvis_bin_bounds(ctx._ctx, C.byref(desc) if desc is not None else None, results, queries, count,
                                       C.byref(out) if out is not None else None)
        assert rc == L.E_INVALID, words_
        msg = ctx.last_error()
        assert "bin_bounds" in msg and all(x in msg for x in words_), msg

    D = L.BoundsTilesDesc
    rp, qp = res.data_ptr(), qry.data_ptr()
    refused(r, ("desc", "NULL"), None, rp, qp, n, full)
    refused(r, ("out", "NULL"), D(8, 4, 1, NEAR), rp, qp, n, None)
    refused(r, ("outputs", "NULL"), D(8, 4, 1, NEAR), rp, qp, n, L.BoundsTiles(None, None, None, None))
    for T in (0, 4, 12, 128):
        refused(r, ("tileSize",), D(T, 4, 1, NEAR), rp, qp, n, full)
    refused(r, ("flags",), D(8, 4, 1, 4), rp, qp, n, full)
    refused(r, ("flags",), D(8, 4, 1, NEAR | FAR | 0x80000000), rp, qp, n, full)
    refused(r, ("phase",), D(8, 4, 2, NEAR), rp, qp, n, full)
    refused(r, ("FAR", "deviceQueries"), D(8, 4, 1, FAR), rp, None, n, full)
    refused(r, ("deviceResults", "NULL"), D(8, 4, 1, NEAR), None, qp, n, full)
    refused(r, ("tileItems", "maxPerTile"), D(8, 0, 1, NEAR), rp, qp, n, full)
    refused(r, ("tiles * maxPerTile",), D(8, (1 << 32) // tiles + 1, 1, NEAR), rp, qp, n, full)
    refused(r, ("16-byte",), D(8, 4, 1, NEAR), rp + 4, qp, n, full)
    refused(r, ("16-byte",), D(8, 4, 1, NEAR | FAR), rp, qp + 8, n, full)
    bare = VisibilityRenderer(0)
    refused(bare, ("G-buffer",), D(8, 4, 1, NEAR), rp, qp, n, full)
    bare.allocate_gbuffer(w, h)
    refused(bare, ("no view",), D(8, 4, 1, NEAR), rp, qp, n, full)
    # a camera view of another size than the instance view's (chordvis_set_view holds only the latter to the image) ...
    mixed = view.copy()
    mixed["renderDimension"][0, 0] += 1
    bare.set_view(mixed, iv, 0)
    refused(bare, ("renderDimension",), D(8, 4, 1, NEAR), rp, qp, n, full)
    bare.close()
    # ... and a view set before an image of another size was allocated
    early = VisibilityRenderer(0)
    _, _, view2, iv2 = H.setup_scene(lambda: scenes.small_test_scene(320, 200))
    early.set_view(view2, iv2, 0)
    early.allocate_gbuffer(w, h)
    refused(early, ("renderDimension",), D(8, 4, 1, NEAR), rp, qp, n, full)
    early.close()
    # nothing was written by a refused call; the largest stride that is allowed passes the checks (no items asked for)
    r.sync()
    assert all((t.cpu().numpy().view(np.uint32) == 0x11111111).all() for t in outs)
    no_items = L.BoundsTiles(outs[0].data_ptr(), None, outs[2].data_ptr(), outs[3].data_ptr())
    assert L.lib.chordvis_bin_bounds(r._ctx, C.byref(D(8, ((1 << 32) - 1) // tiles, 1, NEAR)), rp, None, n, C.byref(no_items)) == L.OK, r.last_error()
    r.sync()
    assert not outs[0].cpu().numpy().any() and not outs[3].cpu().numpy().any()
    assert np.array_equal(outs[2].cpu().numpy().view(np.uint32).reshape(-1, 2), S.tile_depth(words, w, h, 8))
