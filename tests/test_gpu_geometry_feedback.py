"""chordvis_geometry_feedback, chordvis_visible_clusters and their read-backs through the C ABI on the GPU.  Every comparison is exact
equality with tests/spec_geometry_feedback_np.py (integers: no tolerance anywhere): the seven count arrays, the seen bitmap and the
visible-cluster list (records and count) on rendered frames (a small scene, two moving frames under general transforms, a masked
scene, a 2-rank sharded frame), on synthetic caller-owned images that hold ids no frame holds, on a caller's command list with
records that name no object / no meshlet, over every lattice of strides 2, 4 and 8, across accumulating calls and resets, under the
debug switch that shrinks the workgroups' count tables, at the capacity edges of the list output, and for every refusal."""
import ctypes as C

import numpy as np
import pytest

from chord_amd import lib as L, records as R, scenes

import helpers as H
import spec_geometry_feedback_np as SG

pytestmark = pytest.mark.gpu

SMALL_TABLES = 8388608                                 # chordvis_set_debug: two entries per count table
GUARD = 0x5A5A5A5A


def _renderer(scene, w, h, caller_image=False):
    from chord_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(0)
    r.upload_scene(scene)
    img = H.CallerVisibility(r, w, h) if caller_image else r.allocate_gbuffer(w, h)
    return (r, img) if caller_image else r


def _same(got, want, what):
    for k in SG.ARRAYS + ("seen",):
        g, x = got[k], want[k]
        assert g.shape == x.shape and g.dtype == np.uint32, (what, k, g.shape, x.shape)
        if not np.array_equal(g, x):
            bad = np.argwhere(g != x)
            raise AssertionError("%s: %s differs at %d places; first %s got %d want %d" % (what, k, len(bad), bad[0], g[tuple(bad[0])], x[tuple(bad[0])]))
    assert got["total"] == len(want["visible"]), "%s: visible count %d, spec %d" % (what, got["total"], len(want["visible"]))
    assert np.array_equal(got["visible"], want["visible"]), "%s: the visible list's records or order" % what


def _read(r, handle):
    """The arrays, the bitmap and the visible list as the library reports them now."""
    got = r.read_geometry_feedback()
    got["seen"] = r.read_geometry_feedback_seen()
    got["visible"], got["total"] = r.visible_clusters(drawed_meshlet_cmd=handle)
    return got


def _spec(r, scene, words, cmds, count, stride=1, offset=(0, 0)):
    return SG.geometry_feedback(scene, words, cmds, count, r.width, r.height, r.last_frame_cmds().capacity, stride, offset)


def _one_call(r, scene, words, cmds, handle, what, count=None, stride=1, offset=(0, 0)):
    """reset, one call, everything against the spec; returns the spec's result"""
    r.reset_geometry_feedback()
    r.geometry_feedback(stride, offset, handle)
    want = _spec(r, scene, words, cmds, len(cmds) if count is None else count, stride, offset)
    _same(_read(r, handle), want, what)
    assert SG.identities(want) == [], what
    return want


def _frame_inputs(r):
    handle = r.last_frame_cmds()
    return r.read_visibility(), r.read_cmds(handle), handle


def _device_words(values, device):
    """int32 torch tensor holding uint32 `values`, complete before any other stream reads it"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint32).view(np.int32).copy()).to(torch.device("cuda", device))
    torch.cuda.synchronize()
    return t


# ---- 1. rendered frames ----------------------------------------------------------------------------------------------------------------

def test_small_scene_frames(gpu):
    w, h = 160, 96
    scene, cam, view, iv = H.setup_scene(scenes.small_test_scene, w, h)
    r = _renderer(scene, w, h)
    r.set_view(view, iv, H.ALL_FLAGS)
    for frame in range(2):
        r.render_frame()
        words, cmds, handle = _frame_inputs(r)
        want = _one_call(r, scene, words, cmds, handle, "small scene frame %d" % frame)
        assert want["totals"][1] > 0.3 * w * h and want["totals"][2] == 0 and 0 < len(want["visible"]) < len(cmds)
        _one_call(r, scene, words, cmds, handle, "small scene frame %d stride 2" % frame, stride=2, offset=(1, 0))
    r.set_debug(SMALL_TABLES)                                          # a rendered case with the tables full
    under = _one_call(r, scene, words, cmds, handle, "small scene, two-entry tables")
    assert np.array_equal(under["objectPixels"], want["objectPixels"])
    r.set_debug(0)
    r.close()


def test_two_moving_frames_under_general_transforms(gpu):
    w, h = 640, 360
    scene, cam, _ = scenes.general_transform_scene(w, h)
    cams = scenes.general_cameras(cam)
    r = _renderer(scene, w, h)
    prev = None
    for k in range(2):
        view, iv = H.moving_frame(scene, cams, k, prev)
        prev = view
        r.update_objects(scene.objects)
        r.set_view(view, iv, H.ALL_FLAGS)
        r.render_frame()
        words, cmds, handle = _frame_inputs(r)
        want = _one_call(r, scene, words, cmds, handle, "general transforms frame %d" % k)
        # what tests/test_geometry_feedback_spec.py asserts of the oracle's frames, on the frame compared here
        assert ((want["lodSubmitted"] > 0).sum(axis=1) >= 2).any() and len(want["visible"]) < len(cmds)
        if k == 1:
            assert ((want["objectSubmitted"] > 0) & (want["objectPixels"] == 0)).any()
    _one_call(r, scene, words, cmds, handle, "general transforms frame 1 stride 4", stride=4, offset=(1, 2))
    r.close()


def test_masked_scene(gpu):
    w, h = 320, 200
    scene, cam, view, iv = H.setup_scene(scenes.masked_test_scene, w, h)
    r = _renderer(scene, w, h)
    r.set_view(view, iv, H.ALL_FLAGS)
    r.render_frame()
    words, cmds, handle = _frame_inputs(r)
    want = _one_call(r, scene, words, cmds, handle, "masked scene")
    alpha = scene.materials["alphaMode"][scene.objects["GLTFMaterialData"]]
    assert (want["objectPixels"][alpha == R.ALPHA_MASK] > 0).any() and not want["objectPixels"][alpha == R.ALPHA_BLEND].any()
    r.close()


def test_sharded_ranks_count_the_resolved_image(gpu):
    w, h, ranks = 160, 96, 2
    scene, cam, view, iv = H.setup_scene(scenes.small_test_scene, w, h)
    ctxs = H.sharded_contexts(scene, view, iv, w, h, H.ALL_FLAGS, ranks)
    H.sharded_frame(ctxs, sharded_cull=False)
    H.sharded_frame(ctxs)
    whole = None
    for rk, r in enumerate(ctxs):
        words, cmds, handle = _frame_inputs(r)
        want = _one_call(r, scene, words, cmds, handle, "rank %d" % rk)
        assert want["totals"][0] == w * h and want["totals"][1] > 0.3 * w * h
        if whole is not None:
            assert all(np.array_equal(want[k], whole[k]) for k in SG.ARRAYS), "both ranks count the same resolved image"
        whole = want
    for r in ctxs:
        r.close()


# ---- 2. synthetic images in a caller-owned buffer --------------------------------------------------------------------------------------

def _synthetic_context(w, h):
    """A context whose image is the caller's, with a frame rendered (the resolves' precondition) and the list of an instance cull"""
    scene, cam, view, iv = H.setup_scene(scenes.small_test_scene, w, h)
    r, img = _renderer(scene, w, h, caller_image=True)
    r.set_view(view, iv, H.ALL_FLAGS)
    r.render_frame()
    handle = r.instance_culling()
    cmds = r.read_cmds(handle)
    assert len(cmds) > 64 and np.array_equal(cmds["slot"], np.arange(len(cmds)))
    return scene, r, img, handle, cmds


def _tri_counts(scene, cmds):
    return (scene.meshlets["vertexTriangleCount"][cmds["meshletId"]].astype(np.int64) >> 8) & 0xFF


def _images(scene, cmds, w, h):
    """{name: low words}: the cases of the synthetic-image test"""
    n, px = len(cmds), w * h
    rng = np.random.default_rng([w, h])
    tcount = _tri_counts(scene, cmds)
    i = np.arange(px)
    cyc = i % n
    edge = rng.integers(0, 6, px)
    some = rng.integers(0, n, px)
    return {
        "one id everywhere": np.full(px, (n // 2 + 1) << 8 | 1),
        "every slot in turn": (cyc + 1) << 8 | (i // n) % np.maximum(tcount[cyc], 1),
        "ids at n - 1, n, n + 1 and 0xFFFFFF": np.select([edge == 0, edge == 1, edge == 2, edge == 3, edge == 4],
                                                          [n << 8, (n + 1) << 8, (n + 2) << 8, 0xFFFFFF << 8, 0xFFFFFFFF], (some + 1) << 8),
        "tri at the triangle count and at 255": np.select([edge < 2, edge < 4], [(some + 1) << 8 | tcount[some], (some + 1) << 8 | 255],
                                                           (some + 1) << 8 | (tcount[some] - 1)),
        "an empty image": np.zeros(px, dtype=np.int64),
    }


@pytest.mark.parametrize("w,h", [(129, 67), (64, 64)], ids=["129x67", "64x64"])
def test_synthetic_images(gpu, w, h):
    scene, r, img, handle, cmds = _synthetic_context(w, h)
    n = len(cmds)
    depth = H.synthetic_depth(w, h, 2)
    for name, low in _images(scene, cmds, w, h).items():
        words = H.synthetic_words(depth, low)
        img.write(words)
        want = _one_call(r, scene, words, cmds, handle, "%d x %d, %s" % (w, h, name))
        t = [int(v) for v in want["totals"]]
        assert t[0] == w * h
        if name == "one id everywhere":
            assert t[1:] == [w * h, 0, 1] and want["objectPixels"].max() == w * h
        elif name == "every slot in turn":
            assert t[1] == w * h and t[3] == min(n, w * h) and (want["objectVisible"] == want["objectSubmitted"]).all() == (n <= w * h)
        elif name.startswith("ids at"):
            assert t[2] > 0.5 * w * h and want["seen"][(n - 1) >> 5] >> ((n - 1) & 31) & 1, "id n names the last command; n + 1 and beyond name none"
        elif name.startswith("tri at"):
            assert t[2] > 0.5 * w * h and t[1] > 0.2 * w * h
        else:
            assert t[1:] == [0, 0, 0] and not want["seen"].any() and want["objectSubmitted"].sum() == n
        assert np.array_equal(img.read(), words), "nothing writes into the caller's image"
    # the same image under the two-entry tables, and through a list whose count word is 0
    words = H.synthetic_words(depth, _images(scene, cmds, w, h)["every slot in turn"])
    img.write(words)
    r.set_debug(SMALL_TABLES)
    _one_call(r, scene, words, cmds, handle, "%d x %d, every slot in turn, two-entry tables" % (w, h))
    _one_call(r, scene, words, cmds, handle, "%d x %d, stride 2, two-entry tables" % (w, h), stride=2, offset=(1, 1))
    r.set_debug(0)
    zero = _device_words([0], r.device)
    empty = L.CountAndCmd(zero.data_ptr(), handle.cmds, handle.capacity)
    want = _one_call(r, scene, words, cmds, empty, "%d x %d, a list of count 0" % (w, h), count=0)
    assert [int(v) for v in want["totals"]] == [w * h, 0, w * h, 0] and not want["objectSubmitted"].any()
    r.close()


def test_a_callers_list_with_records_that_name_nothing(gpu):
    w, h = 129, 67
    scene, r, img, handle, cmds = _synthetic_context(w, h)
    mine = cmds.copy()
    n = len(mine)
    no_object, no_meshlet, neither = 5, n // 2, n - 1
    mine["objectId"][no_object] = len(scene.objects)
    mine["meshletId"][no_meshlet] = len(scene.meshlets)
    mine["objectId"][neither], mine["meshletId"][neither] = 0xFFFFFFFF, 0xFFFFFFFF
    records = _device_words(mine.view(np.uint32), r.device)
    count = _device_words([n], r.device)
    listed = L.CountAndCmd(count.data_ptr(), records.data_ptr(), n)
    px = np.arange(w * h)
    low = ((px % n) + 1) << 8                                          # every command's triangle 0, the three bad ones included
    words = H.synthetic_words(H.synthetic_depth(w, h, 3), low)
    img.write(words)
    want = _one_call(r, scene, words, mine, listed, "a caller's list")
    bad = np.isin(px % n, (no_object, no_meshlet, neither))
    assert int(want["totals"][2]) == bad.sum() > 0 and int(want["totals"][1]) == (~bad).sum()
    assert int(want["objectSubmitted"].sum()) == n - 3 == int(want["lodSubmitted"].sum())
    assert not np.isin(want["visible"]["slot"], (no_object, no_meshlet, neither)).any() and len(want["visible"]) == n - 3
    for s in (no_object, no_meshlet, neither):
        assert not want["seen"][s >> 5] >> (s & 31) & 1
    # a count word past the capacity: n is the context's capacity (the caller's buffer holds that many records)
    cap = r.last_frame_cmds().capacity
    padded = np.zeros(cap, dtype=R.DRAW_CMD)
    padded[:n] = mine
    padded[n:] = mine[0]
    records2 = _device_words(padded.view(np.uint32), r.device)
    count2 = _device_words([cap + 7], r.device)
    listed2 = L.CountAndCmd(count2.data_ptr(), records2.data_ptr(), cap)
    want = _one_call(r, scene, words, padded, listed2, "a count past the capacity", count=cap + 7)
    assert want["n"] == cap and int(want["objectSubmitted"].sum()) == cap - 3
    r.close()


# ---- 3. lattices ------------------------------------------------------------------------------------------------------------------------

def test_every_lattice_of_strides_2_4_and_8(gpu):
    w, h = 129, 67
    scene, r, img, handle, cmds = _synthetic_context(w, h)
    words, _, _ = _frame_inputs(r)                                      # the rendered frame in the caller's image ...
    words = words.copy()
    rng = np.random.default_rng(9)
    at = rng.choice(w * h, 600, replace=False)                          # ... with ids past the list and bad triangles sprinkled in
    words[at[:300]] = np.uint64(0x3F000000) << np.uint64(32) | np.uint64((len(cmds) + 1) << 8)
    words[at[300:]] |= np.uint64(255)
    img.write(words)
    cmds = r.read_cmds(r.last_frame_cmds())
    handle = r.last_frame_cmds()
    whole = _one_call(r, scene, words, cmds, handle, "stride 1")
    assert whole["totals"][1] > 0.2 * w * h and whole["totals"][2] >= 300
    for stride in (2, 4, 8):
        for oy in range(stride):
            for ox in range(stride):
                r.reset_geometry_feedback()
                r.geometry_feedback(stride, (ox, oy), handle)
                want = _spec(r, scene, words, cmds, len(cmds), stride, (ox, oy))
                _same(_read(r, handle), want, "stride %d offset (%d, %d)" % (stride, ox, oy))
        r.reset_geometry_feedback()                                     # one reset, all stride^2 offsets: the lattices partition the image
        for oy in range(stride):
            for ox in range(stride):
                r.geometry_feedback(stride, (ox, oy), handle)
        got = r.read_geometry_feedback()
        for k in SG.PIXEL_ARRAYS:
            assert np.array_equal(got[k], whole[k]), (stride, k)
        assert np.array_equal(got["totals"][:3], whole["totals"][:3]), stride
        last = _spec(r, scene, words, cmds, len(cmds), stride, (stride - 1, stride - 1))
        assert np.array_equal(r.read_geometry_feedback_seen(), last["seen"]), "the bitmap is the last call's"
    r.close()


# ---- 4. accumulation ---------------------------------------------------------------------------------------------------------------------

def test_calls_accumulate_and_the_bitmap_is_the_latest_calls(gpu):
    w, h = 160, 96
    scene, cam, view, iv = H.setup_scene(scenes.small_test_scene, w, h)
    r = _renderer(scene, w, h)
    r.set_view(view, iv, H.ALL_FLAGS)
    r.render_frame()
    words, cmds, handle = _frame_inputs(r)
    one = _one_call(r, scene, words, cmds, handle, "one call")
    r.reset_geometry_feedback()
    r.geometry_feedback(1, (0, 0), handle)
    r.geometry_feedback(1, (0, 0), handle)
    got = _read(r, handle)
    twice = dict(one, **{k: one[k] * np.uint32(2) for k in SG.ARRAYS})
    _same(got, twice, "two calls")
    part = _spec(r, scene, words, cmds, len(cmds), 4, (2, 1))
    r.geometry_feedback(4, (2, 1), handle)
    got = _read(r, handle)
    summed = dict(part, **{k: twice[k] + part[k] for k in SG.ARRAYS})
    assert not np.array_equal(part["seen"], one["seen"])
    _same(got, summed, "three calls: the counts of all, the bitmap and the list of the third")
    r.reset_geometry_feedback()
    got = r.read_geometry_feedback()
    assert not any(a.any() for a in got.values()) and not r.read_geometry_feedback_seen().any(), "a reset zeroes everything"
    r.close()


# ---- 5. chordvis_visible_clusters at the capacity edges ------------------------------------------------------------------------------------

def test_visible_clusters_capacities(gpu):
    w, h = 160, 96
    scene, cam, view, iv = H.setup_scene(scenes.small_test_scene, w, h)
    r = _renderer(scene, w, h)
    r.set_view(view, iv, H.ALL_FLAGS)
    r.render_frame()
    words, cmds, handle = _frame_inputs(r)
    want = _one_call(r, scene, words, cmds, handle, "the frame")
    total = len(want["visible"])
    assert total > 8
    for capacity in (0, total, total - 1, 1, total + 5):
        out = _device_words(np.full(3 * (total + 8) + 1, GUARD, dtype=np.uint32), r.device)
        recs, got_total = r.visible_clusters(capacity, handle, out=out)
        host = out.cpu().numpy().view(np.uint32)
        kept = min(capacity, total)
        assert got_total == total == int(host[3 * capacity]), "capacity %d: the count word holds the total" % capacity
        assert np.array_equal(recs, want["visible"][:kept]), "capacity %d: the first records in list order" % capacity
        assert (host[3 * kept:3 * capacity] == GUARD).all() and (host[3 * capacity + 1:] == GUARD).all(), "capacity %d: a word beyond the permitted records changed" % capacity
    r.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------

def test_refusals(gpu):
    w, h = 64, 64
    scene, cam, view, iv = H.setup_scene(scenes.small_test_scene, w, h)
    r = _renderer(scene, w, h)
    r.set_view(view, iv, H.ALL_FLAGS)
    no, npr = len(scene.objects), len(scene.primitives)
    arrays = {n: np.zeros(no if n.startswith("object") else 4 if n == "totals" else npr * 16, np.uint32) for n in L.GEOMETRY_ARRAYS}
    fb = L.GeometryFeedback(**{n: a.ctypes.data for n, a in arrays.items()})
    out = _device_words(np.zeros(16, np.uint32), r.device)

    def refused(rc, text):
        assert rc == L.E_INVALID, rc
        assert text in L.lib.chordvis_last_error(r._ctx).decode(), L.lib.chordvis_last_error(r._ctx)

    def run(stride=1, ox=0, oy=0, pad=0, handle=None):
        d = L.GeometryFeedbackDesc(stride, (C.c_uint32 * 2)(ox, oy), pad)
        return L.lib.chordvis_geometry_feedback(r._ctx, handle or r.last_frame_cmds(), C.byref(d))

    def visible(handle=None):
        return L.lib.chordvis_visible_clusters(r._ctx, handle or r.last_frame_cmds(), out.data_ptr() + 4, out.data_ptr(), 1)

    refused(run(), "no frame rendered yet")
    r.render_frame()
    words = (r.last_frame_cmds().capacity + 31) // 32
    seen = np.zeros(words + 1, np.uint32)
    refused(run(), "no chordvis_geometry_feedback_reset since the last chordvis_upload_scene")
    refused(L.lib.chordvis_readback_geometry_feedback(r._ctx, C.byref(fb), no, npr), "no chordvis_geometry_feedback_reset")
    refused(L.lib.chordvis_geometry_feedback_seen(r._ctx, seen.ctypes.data, words), "no chordvis_geometry_feedback_reset")
    refused(visible(), "no chordvis_geometry_feedback since")
    r.reset_geometry_feedback()
    refused(visible(), "no chordvis_geometry_feedback since")
    refused(L.lib.chordvis_geometry_feedback(r._ctx, r.last_frame_cmds(), None), "null ChordGeometryFeedbackDesc")
    for stride in (0, 3, 5, 16):
        refused(run(stride=stride), "stride is 1, 2, 4 or 8")
    for stride, ox, oy in ((1, 1, 0), (2, 0, 2), (8, 8, 0), (4, 0, 0xFFFFFFFF)):
        refused(run(stride=stride, ox=ox, oy=oy), "each offset is 0 .. stride - 1")
    refused(run(pad=1), "pad is 0")
    for a, b in ((no - 1, npr), (no, npr + 1), (0, 0)):
        refused(L.lib.chordvis_readback_geometry_feedback(r._ctx, C.byref(fb), a, b), "are the uploaded scene's, %d and %d" % (no, npr))
    for n in (words - 1, words + 1, 0):
        refused(L.lib.chordvis_geometry_feedback_seen(r._ctx, seen.ctypes.data, n), "wordCount is ceil(capacity / 32), %d" % words)
    assert run() == L.OK and run(stride=8, ox=7, oy=7) == L.OK and visible() == L.OK
    assert L.lib.chordvis_readback_geometry_feedback(r._ctx, C.byref(fb), no, npr) == L.OK and arrays["objectPixels"].any()
    only = L.GeometryFeedback(totals=arrays["totals"].ctypes.data)     # NULL pointers: not wanted
    assert L.lib.chordvis_readback_geometry_feedback(r._ctx, C.byref(only), no, npr) == L.OK
    other = r.last_frame_cmds()
    records = _device_words(r.read_cmds(other).view(np.uint32), r.device)
    refused(visible(L.CountAndCmd(other.count, records.data_ptr(), other.capacity)), "not the one the latest chordvis_geometry_feedback was given")
    r.reset_geometry_feedback()
    refused(visible(), "no chordvis_geometry_feedback since")
    assert run() == L.OK and visible() == L.OK
    r.set_view(view, iv, H.ALL_FLAGS)                                  # a stale view, as chordvis_resolve_attributes refuses it
    refused(run(), "came after the frame")
    r.render_frame()
    assert run() == L.OK
    r.upload_scene(scene)                                              # a new scene upload drops the buffer
    r.allocate_gbuffer(w, h)
    r.set_view(view, iv, H.ALL_FLAGS)
    r.render_frame()
    refused(run(), "no chordvis_geometry_feedback_reset")
    refused(visible(), "no chordvis_geometry_feedback since")
    r.reset_geometry_feedback()
    assert run() == L.OK and visible() == L.OK
    r.close()
