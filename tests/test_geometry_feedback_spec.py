"""chordvis_geometry_feedback on the CPU (tests/spec_geometry_feedback_np.py): the vectorised spec equals a plain per-pixel loop
written from the header's definitions, the stated identities hold, the lattices of a stride partition the image, and the frames the
GPU comparison (tests/test_gpu_geometry_feedback.py) renders hold what it relies on.  No GPU."""
import functools

import numpy as np
import pytest

from chord_amd import records as R, scenes

import helpers as H
import spec_geometry_feedback_np as SG


def _loop(scene, words, cmds, count, w, h, capacity, stride, offset):
    """The definitions, one pixel and one command at a time."""
    n = min(count, capacity)
    n_obj, n_prim = len(scene.objects), len(scene.primitives)
    out = {k: np.zeros(n_obj, np.uint32) for k in ("objectPixels", "objectSubmitted", "objectVisible")}
    out.update({k: np.zeros((n_prim, 16), np.uint32) for k in ("lodPixels", "lodSubmitted", "lodVisible")})
    totals = [0, 0, 0, 0]
    seen = [False] * n

    def keys(i):
        o, m = int(cmds["objectId"][i]), int(cmds["meshletId"][i])
        if o >= n_obj or m >= len(scene.meshlets):
            return None
        return o, m, int(scene.objects["GLTFPrimitiveDetail"][o]), min(int(scene.meshlets["lod"][m]), 15)

    for y in range(h):
        for x in range(w):
            if x % stride != offset[0] or y % stride != offset[1]:
                continue
            totals[0] += 1
            low = int(words[y * w + x]) & 0xFFFFFFFF
            if low == 0:
                continue
            slot = ((low >> 8) & 0xFFFFFF) - 1
            k = keys(slot) if 0 <= slot < n else None
            if k is None or (low & 0xFF) >= ((int(scene.meshlets["vertexTriangleCount"][k[1]]) >> 8) & 0xFF):
                totals[2] += 1
                continue
            totals[1] += 1
            out["objectPixels"][k[0]] += 1
            out["lodPixels"][k[2], k[3]] += 1
            seen[slot] = True
    for i in range(n):
        k = keys(i)
        if k is None:
            assert not seen[i]
            continue
        out["objectSubmitted"][k[0]] += 1
        out["lodSubmitted"][k[2], k[3]] += 1
        if seen[i]:
            out["objectVisible"][k[0]] += 1
            out["lodVisible"][k[2], k[3]] += 1
    totals[3] = sum(seen)
    out["totals"] = np.array(totals, np.uint32)
    bitmap = np.zeros((capacity + 31) // 32, np.uint32)
    for i in range(n):
        if seen[i]:
            bitmap[i >> 5] |= np.uint32(1 << (i & 31))
    out["seen"] = bitmap
    out["visible"] = np.array([cmds[i] for i in range(n) if seen[i]], dtype=R.DRAW_CMD)
    return out


def _assert_same(got, want, what):
    for k in SG.ARRAYS + ("seen",):
        assert got[k].dtype == np.uint32 and np.array_equal(got[k], want[k]), (what, k)
    assert np.array_equal(got["visible"], want["visible"]), (what, "visible")


@functools.lru_cache(maxsize=None)
def _small_frame():
    import orc
    w, h = 160, 96
    scene, cam, view, iv = H.setup_scene(scenes.small_test_scene, w, h)
    return scene, orc.frame(scene, view, iv, H.ALL_FLAGS), w, h


def test_spec_equals_a_per_pixel_loop_on_a_rendered_frame(built_lib):
    scene, fr, w, h = _small_frame()
    cmds, cap = fr["cmds"], scene.lod0_meshlet_instances
    assert 2 < len(cmds) <= cap
    for stride, offset in ((1, (0, 0)), (2, (1, 0)), (4, (3, 2)), (8, (7, 7))):
        got = SG.geometry_feedback(scene, fr["vis"], cmds, len(cmds), w, h, cap, stride, offset)
        _assert_same(got, _loop(scene, fr["vis"], cmds, len(cmds), w, h, cap, stride, offset), (stride, offset))
        assert SG.identities(got) == [], (stride, offset)
        assert got["totals"][0] == len(range(offset[0], w, stride)) * len(range(offset[1], h, stride))
    whole = SG.geometry_feedback(scene, fr["vis"], cmds, len(cmds), w, h, cap)
    assert whole["totals"][1] > 0.3 * w * h and whole["totals"][2] == 0, "a rendered frame has no rejected pixel"
    bits = np.unpackbits(whole["seen"].view(np.uint8), bitorder="little")
    assert 0 < len(whole["visible"]) == bits.sum() and np.array_equal(whole["visible"]["slot"], np.flatnonzero(bits)), "slot i of the full list is command i"


def test_spec_equals_a_per_pixel_loop_on_ids_no_frame_holds(built_lib):
    """A 37 x 19 image of ids at and past the list's ends, triangle bytes at and past the meshlets' counts, an id field of 0 under a
    non-zero word, and a list with records that name no object / no meshlet; counts 0, in between and past the capacity."""
    scene, fr, _, _ = _small_frame()
    w, h = 37, 19
    cmds = fr["cmds"].copy()
    count = len(cmds)
    cmds["objectId"][3] = len(scene.objects)
    cmds["meshletId"][5] = len(scene.meshlets)
    cmds["objectId"][7] = 0xFFFFFFFF
    rng = np.random.default_rng(3)
    kind = rng.integers(0, 9, w * h)
    tcount = (scene.meshlets["vertexTriangleCount"][cmds["meshletId"].clip(0, len(scene.meshlets) - 1)].astype(np.int64) >> 8) & 0xFF
    some = rng.integers(0, count, w * h)
    low = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5, kind == 6, kind == 7],
                    [0, count << 8, (count + 1) << 8, 0xFFFFFFFF, 77, (some + 1) << 8 | tcount[some], (some + 1) << 8 | 255,
                     (rng.choice([3, 5, 7], w * h) + 1) << 8],
                    (some + 1) << 8 | rng.integers(0, 8, w * h)).astype(np.uint64)
    words = (np.uint64(0x3F000000) << np.uint64(32)) | low
    for n, cap in ((count, count + 9), (0, count), (count // 2, count), (count, count // 3), (count + 5, count)):
        for stride, offset in ((1, (0, 0)), (4, (1, 3))):
            got = SG.geometry_feedback(scene, words, cmds, n, w, h, cap, stride, offset)
            _assert_same(got, _loop(scene, words, cmds, n, w, h, cap, stride, offset), (n, cap, stride))
            assert SG.identities(got) == []
    full = SG.geometry_feedback(scene, words, cmds, count, w, h, count)
    rejected = np.isin(kind, (2, 3, 4, 5, 6, 7)).reshape(h, w)          # (kind 1 is the id of the last command: it contributes)
    assert not full["contributing"][rejected].any() and full["contributing"][(kind == 1).reshape(h, w)].all()
    assert full["totals"][2] >= rejected.sum() > 300 and full["totals"][1] > 100
    assert full["objectSubmitted"].sum() == count - 3


@pytest.mark.parametrize("stride", [2, 4, 8])
def test_the_offsets_of_a_stride_partition_the_image(built_lib, stride):
    scene, fr, w, h = _small_frame()
    cmds, cap = fr["cmds"], scene.lod0_meshlet_instances
    whole = SG.geometry_feedback(scene, fr["vis"], cmds, len(cmds), w, h, cap)
    parts = [SG.geometry_feedback(scene, fr["vis"], cmds, len(cmds), w, h, cap, stride, (ox, oy)) for oy in range(stride) for ox in range(stride)]
    for k in SG.PIXEL_ARRAYS:
        assert np.array_equal(sum(p[k].astype(np.int64) for p in parts), whole[k]), k
    assert np.array_equal(sum(p["totals"][:3].astype(np.int64) for p in parts), whole["totals"][:3])
    assert np.array_equal(np.bitwise_or.reduce([p["seen"] for p in parts]), whole["seen"])
    assert not np.logical_and.reduce([p["contributing"] for p in parts[:2]]).any()


# ---- the GPU cases are not vacuous (the oracle's frames alone) -----------------------------------------------------------------------

def test_general_transform_frames_meet_the_conditions_the_gpu_tests_rely_on(built_lib):
    """Frames 0 and 1 of scenes.general_transform_scene under scenes.general_cameras at 640 x 360, the two consecutive frames the GPU
    file renders.  Every condition holds in frame 1 (cameras[1]: the moved camera); frame 0 meets the first and the third too."""
    w, h = 640, 360
    scene, cam, _ = scenes.general_transform_scene(w, h)
    cams = scenes.general_cameras(cam)
    cap = scene.lod0_meshlet_instances
    for k, view, iv, fr in H.moving_sequence(scene, cams, frames=2):
        cmds = fr["cmds"]
        fb = SG.geometry_feedback(scene, fr["vis"], cmds, len(cmds), w, h, cap)
        assert SG.identities(fb) == [] and fb["totals"][2] == 0
        assert ((fb["lodSubmitted"] > 0).sum(axis=1) >= 2).any(), "frame %d: two LOD columns of one primitive are submitted" % k
        assert len(fb["visible"]) < fb["n"] == len(cmds), "frame %d: the visible list is shorter than the submitted one" % k
        if k == 1:
            assert ((fb["objectSubmitted"] > 0) & (fb["objectPixels"] == 0)).any(), "an object is submitted and owns no pixel"
            assert ((fb["lodVisible"] > 0).sum(axis=1) >= 2).any() and (fb["lodVisible"] < fb["lodSubmitted"]).any()
            quarter = SG.geometry_feedback(scene, fr["vis"], cmds, len(cmds), w, h, cap, 4, (1, 2))
            assert 0 < len(quarter["visible"]) < len(fb["visible"]), "a cluster that covers only off-lattice pixels is missed"


def test_a_masked_object_contributes_pixels(built_lib):
    import orc
    w, h = 320, 200
    scene, cam, view, iv = H.setup_scene(scenes.masked_test_scene, w, h)
    fr = orc.frame(scene, view, iv, H.ALL_FLAGS)
    fb = SG.geometry_feedback(scene, fr["vis"], fr["cmds"], len(fr["cmds"]), w, h, scene.lod0_meshlet_instances)
    alpha = scene.materials["alphaMode"][scene.objects["GLTFMaterialData"]]
    assert (fb["objectPixels"][alpha == R.ALPHA_MASK] > 0).any(), "a masked object owns pixels"
    assert (fb["objectSubmitted"][alpha == R.ALPHA_BLEND] > 0).any() and not fb["objectPixels"][alpha == R.ALPHA_BLEND].any(), "blended objects draw nothing"
    assert SG.identities(fb) == []
