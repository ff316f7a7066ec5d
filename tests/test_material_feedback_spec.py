"""chordvis_material_feedback and chordvis_set_texture_first_level on the CPU (tests/spec_material_feedback_np.py): the counts are a
partition of the pixels the material resolve samples, the lattice offsets partition the stride-1 counts, a trimmed power-of-two
texture gives the untrimmed images bit for bit under the header's three conditions (and one constructed pixel shows the documented
exception), and the test-local scenes hold what the GPU comparison relies on.  No GPU."""
import functools

import numpy as np
import pytest

from chord_amd import scenes

import feedback_scenes as FS
import helpers as H
import spec_material_aniso_np as SA
import spec_material_feedback_np as SF
import spec_material_np as SM

f32 = np.float32


@functools.lru_cache(maxsize=None)
def _frame(builder, w, h):
    import orc
    scene, cam, view, iv = H.setup_scene(builder, w, h) if builder is scenes.material_test_scene else H.setup_scene(builder)
    fr = orc.frame(scene, view, iv, H.ALL_FLAGS)
    return scene, view, iv, fr


@functools.lru_cache(maxsize=None)
def _stats(builder, w, h, n):
    scene, view, iv, fr = _frame(builder, w, h)
    return SF.resolve_stats(scene, fr["vis"], fr["cmds"], view, iv, w, h, n)


# ---- 1. the counts are the sampled (pixel, slot) pairs -----------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 16])
def test_row_sums_are_the_pbr_hit_pixels_times_their_textured_slots(built_lib, n):
    w, h = 65, 67
    scene, view, iv, fr = _frame(scenes.material_test_scene, w, h)
    st = _stats(scenes.material_test_scene, w, h, n)
    for stride, offset in ((1, (0, 0)), (2, (1, 0)), (4, (3, 2)), (8, (7, 7))):
        taps = SF.feedback_of(st, scene, w, 15, stride, offset)
        assert taps.shape == (len(scene.texture_images), 16) and taps.dtype == np.uint32
        # counted from the definition, not from the sampler's lists: PBR hit pixels on the lattice x slots that name a texture
        pix = np.flatnonzero(st["hit"] & st["pbr"])
        pix = pix[SF.on_lattice(pix, w, stride, offset)]
        want = np.zeros(len(scene.texture_images), dtype=np.int64)
        for slot in SM.SLOTS:
            tid = scene.materials[SM._TEX_FIELD[slot][0]][st["material"][pix]].astype(np.int64)
            named = tid < len(scene.texture_images)
            want += np.bincount(tid[named], minlength=len(want))
        assert np.array_equal(taps.sum(axis=1), want), (stride, offset)
        assert int(taps.sum()) == SF.pairs_on_lattice(st, w, 15, stride, offset)
        assert not taps[:, 15].any()
    assert SF.feedback_of(st, scene, w).sum() > 4000


@pytest.mark.parametrize("stride", [2, 4, 8])
def test_the_offsets_of_a_stride_partition_the_stride_1_counts(built_lib, stride):
    w, h = 65, 67
    scene, view, iv, fr = _frame(scenes.material_test_scene, w, h)
    st = _stats(scenes.material_test_scene, w, h, 1)
    whole = SF.feedback_of(st, scene, w).astype(np.int64)
    parts = [SF.feedback_of(st, scene, w, 15, stride, (ox, oy)).astype(np.int64) for oy in range(stride) for ox in range(stride)]
    assert np.array_equal(sum(parts), whole)
    assert sum(1 for p in parts if p.any()) == stride * stride
    masks = [SF.feedback_of(st, scene, w, bit).astype(np.int64) for bit in (1, 2, 4, 8)]
    assert np.array_equal(sum(masks), whole) and all(m.any() for m in masks)


# ---- 2. trimmed chains ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 16])
def test_trimmed_textures_give_the_untrimmed_images(built_lib, n):
    """loop_scene: power-of-two textures, samplers whose filters agree, every texture trimmed to the lowest level the frame taps"""
    w = h = FS.SIZE
    scene, view, iv, fr = _frame(FS.loop_scene, w, h)
    resolve = (lambda s: SM.resolve(s, fr["vis"], fr["cmds"], view, iv, w, h)) if n == 1 else \
              (lambda s: SA.resolve(s, fr["vis"], fr["cmds"], view, iv, w, h, max_aniso=n))
    taps = SF.feedback_of(_stats(FS.loop_scene, w, h, n), scene, w)
    first = FS.first_levels(taps)
    assert max(first) >= 2 and min(first) == 0, first            # (what tests/test_gpu_material_feedback.py's closed loop asserts)
    assert first[FS.T_FAR] >= 2 and first[FS.T_NEAR] == 0 and first[FS.T_TILTED] >= 1
    assert np.count_nonzero(taps[FS.T_TILTED]) >= 2, "the tilted plane taps more than one level"
    small = SF.trimmed(scene, first)
    for i, f in enumerate(first):
        a, b = scene.texture_images[i], small.texture_images[i]
        assert (b.width, b.height, b.mips) == (a.shape[1] >> f, a.shape[0] >> f, max(a.shape[:2]).bit_length() - f)
    whole, cut = resolve(scene), resolve(small)
    for name in SM.NAMES:
        assert np.array_equal(whole[name].view(np.uint32), cut[name].view(np.uint32)), name
        assert np.any(whole[name])
    # the rows of the trimmed scene are the untrimmed rows shifted down by `first`
    shifted = SF.feedback(small, fr["vis"], fr["cmds"], view, iv, w, h, 15, 1, (0, 0), n)
    for i, f in enumerate(first):
        assert np.array_equal(shifted[i, :16 - f], taps[i, f:]), i
    # one level too many changes the image
    over = list(first)
    over[FS.T_FAR] += 1
    worse = resolve(SF.trimmed(scene, over))
    assert any(not np.array_equal(whole[name].view(np.uint32), worse[name].view(np.uint32)) for name in SM.NAMES)


def test_the_documented_exception_takes_the_mag_filter():
    """One pixel whose lodq lies in (256 f - 128, 256 f] under LINEAR_MIPMAP_NEAREST: untrimmed it is minified (bilinear on level f),
    trimmed by f it is not (lodq' <= 0: the mag filter).  With NEAREST as the mag filter the two differ; with LINEAR they are equal."""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(16, 16, 4), dtype=np.uint8)
    from chord_amd import records as R
    chain, mips = R.mip_chain_rgba8(img)
    levels = SM.levels_of(chain, 16, 16, mips)
    f = 1
    d = f32(1.7 / 16.0)                                           # a footprint of 1.7 texels of level 0
    g = np.array([[d, 0.0, 0.0, d]], dtype=f32)
    u, v = np.array([0.37], dtype=f32), np.array([0.61], dtype=f32)
    lodq = int(SM.lodq_of(SM.footprint(g, 16, 16))[0])
    assert 256 * f - 128 < lodq <= 256 * f, lodq
    srgb, _ = SM.tables()
    out = {}
    for mag in (SM.NEAREST, SM.LINEAR):
        smp = (SM.LINEAR_MIPMAP_NEAREST, mag, SM.REPEAT, SM.REPEAT)
        st = {}
        whole = SM.sample(levels, smp, u, v, g, srgb, st)
        assert int(st["l0"][0]) == f                              # no tap below f: the second condition holds
        st = {}
        cut = SM.sample(levels[f:], smp, u, v, g, srgb, st)
        assert int(st["lodq"][0]) == lodq - 256 * f and int(st["l0"][0]) == 0
        out[mag] = np.array_equal(whole.view(np.uint32), cut.view(np.uint32))
    assert out == {SM.NEAREST: False, SM.LINEAR: True}


# ---- 3. what the GPU test's scene of small quads has to hold ---------------------------------------------------------------------------

def test_quads_scene_holds_what_the_gpu_test_relies_on(built_lib):
    w = h = FS.SIZE
    scene, view, iv, fr = _frame(FS.quads_scene, w, h)
    assert len(scene.materials) >= 8 and scene.normals is None and scene.tangents is None
    for n in (1, 16):
        st = _stats(FS.quads_scene, w, h, n)
        assert FS.quads_scene_conditions(scene, st, w, h) == [], n
    assert not np.array_equal(SF.feedback_of(_stats(FS.quads_scene, w, h, 1), scene, w), SF.feedback_of(_stats(FS.quads_scene, w, h, 16), scene, w))
