"""chordvis_material_feedback and chordvis_set_texture_first_level through the C ABI on the GPU.  The counts equal
tests/spec_material_feedback_np.py exactly (integers: no tolerance anywhere) over image sizes that are and are not multiples of the
16 x 4 wave block, lattices, slot masks, both anisotropies and both texture stores; accumulation, refusals, untouched neighbours;
trimmed chains read back as the tail of the untrimmed ones in every store and resolve to the spec of the smaller texture; and the
closed loop feedback -> first levels -> re-upload leaves the images bit-identical in less memory."""
import ctypes as C
import functools

import numpy as np
import pytest

from chord_amd import lib as L, records as R, scenes

import feedback_scenes as FS
import helpers as H
import spec_material_aniso_np as SA
import spec_material_feedback_np as SF
import spec_material_np as SM
import spec_texture_bc_np as BC
import spec_texture_mips_np as M

pytestmark = pytest.mark.gpu

MATERIAL_FORMATS = [BC.BC3, BC.BC3, BC.BC5, BC.BC1_RGB, BC.BC3]                          # albedo, noise, normal, ORM, emissive
SIZES = [(64, 64), (65, 67), (333, 201)]


def _renderer(scene, view, iv, w, h, store=L.TEXSTORE_EXPANDED, upload=True):
    from chord_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(0)
    r.set_material_texture_store(store)
    r.upload_scene(scene)
    if upload:
        r.upload_material_textures()
    r.allocate_gbuffer(w, h)
    r.set_view(view, iv, H.ALL_FLAGS)
    return r


def _taps(r, mask=15, stride=1, offset=(0, 0)):
    r.reset_material_feedback()
    r.material_feedback(mask, stride, offset)
    return r.read_material_feedback()


def _stats(scene, r, view, iv, n=1):
    return SF.resolve_stats(scene, r.read_visibility(), r.read_cmds(r.last_frame_cmds()), view, iv, r.width, r.height, n)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint32, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d counts differ; first (texture, level) = %s got %d want %d\ngot\n%s\nwant\n%s" % (
            what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])], got, want))


def _images(r, names=SM.NAMES):
    import torch
    out = r.resolve_attributes(names=list(names))
    torch.cuda.synchronize()
    return {n: t.cpu().numpy().view(np.uint32) for n, t in out.items()}


@functools.lru_cache(maxsize=None)
def _material_scene(w, h):
    scene, cam, view, iv = H.setup_scene(scenes.material_test_scene, w, h)
    return scene, view, iv


@functools.lru_cache(maxsize=None)
def _bc_material_scene(w, h):
    scene, view, iv = _material_scene(w, h)
    bc = BC.bc_scene(scene, MATERIAL_FORMATS)
    return bc, BC.decoded_twin(bc), view, iv


# ---- 1. spec equality ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_counts_equal_the_spec(gpu, w, h):
    """Frames 0 and 1, anisotropy 1 and 16, the texel store and a store of chains kept as blocks (the same block-compressed scene in
    both: the level rule reads sizes, never texels, and both contexts see the same frame)."""
    bc, twin, view, iv = _bc_material_scene(w, h)
    re, rb = _renderer(bc, view, iv, w, h, L.TEXSTORE_EXPANDED), _renderer(bc, view, iv, w, h, L.TEXSTORE_BLOCKS)
    assert re.material_texture_memory()[1] == 0 and rb.material_texture_memory()[0] == 0
    differ = False
    for frame in range(2):
        re.render_frame(); rb.render_frame()
        H.assert_vis_equal(rb.read_visibility(), re.read_visibility(), w, h, "frame %d, both stores" % frame)
        want = {}
        for n in (1, 16):
            want[n] = SF.feedback_of(_stats(twin, re, view, iv, n), twin, w)
            for r, store in ((re, "texels"), (rb, "blocks")):
                r.set_material_anisotropy(n)
                _same(_taps(r), want[n], "%d x %d frame %d anisotropy %d %s" % (w, h, frame, n, store))
        assert want[1].sum() == want[16].sum() > 0.2 * w * h
        assert np.count_nonzero(want[1]) >= 10
        differ |= not np.array_equal(want[1], want[16])
    assert differ, "the anisotropic sampler taps other levels somewhere"
    re.close(); rb.close()


# ---- 2. lattice ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", SIZES[:2], ids=["%dx%d" % s for s in SIZES[:2]])
def test_lattices(gpu, w, h):
    scene, view, iv = _material_scene(w, h)
    r = _renderer(scene, view, iv, w, h)
    r.render_frame()
    st = _stats(scene, r, view, iv)
    whole = _taps(r)
    _same(whole, SF.feedback_of(st, scene, w), "stride 1")
    for stride in (2, 4):
        total = np.zeros_like(whole)
        for oy in range(stride):
            for ox in range(stride):
                got = _taps(r, 15, stride, (ox, oy))
                _same(got, SF.feedback_of(st, scene, w, 15, stride, (ox, oy)), "stride %d offset (%d, %d)" % (stride, ox, oy))
                total += got
        _same(total, whole, "stride %d summed over its offsets" % stride)
    for off in ((0, 0), (7, 7), (0, 7)):                      # 64 x 64: an 8 x 8 lattice, less than one wave
        got = _taps(r, 15, 8, off)
        _same(got, SF.feedback_of(st, scene, w, 15, 8, off), "stride 8 offset %s" % (off,))
    assert _taps(r, 15, 8, (0, 0)).sum() > 0
    r.close()


# ---- 3. slot masks, 4. accumulation ------------------------------------------------------------------------------------------------------

def test_slot_masks_and_accumulation(gpu):
    w, h = 65, 67
    scene, view, iv = _material_scene(w, h)
    r = _renderer(scene, view, iv, w, h)
    r.render_frame()
    st = _stats(scene, r, view, iv)
    whole = _taps(r)
    total = np.zeros_like(whole)
    for bit in (L.FEEDBACK_BASECOLOR, L.FEEDBACK_EMISSIVE, L.FEEDBACK_NORMAL, L.FEEDBACK_METALROUGH):
        got = _taps(r, bit)
        _same(got, SF.feedback_of(st, scene, w, bit), "slot mask %d" % bit)
        assert got.any(), bit
        total += got
    _same(total, whole, "the four single-bit runs")
    _same(_taps(r, 5), SF.feedback_of(st, scene, w, 5), "slot mask 5")
    # two calls give twice the counts; different calls add up; a reset gives zeros
    r.reset_material_feedback()
    r.material_feedback(15, 1, (0, 0))
    r.material_feedback(15, 1, (0, 0))
    _same(r.read_material_feedback(), whole * np.uint32(2), "two calls")
    r.material_feedback(L.FEEDBACK_NORMAL, 2, (1, 0))
    _same(r.read_material_feedback(), whole * np.uint32(2) + SF.feedback_of(st, scene, w, 4, 2, (1, 0)), "three calls")
    r.reset_material_feedback()
    assert not r.read_material_feedback().any()
    r.close()


# ---- 5. a scene of many small quads ------------------------------------------------------------------------------------------------------

def test_small_quads_under_eight_materials(gpu):
    w = h = FS.SIZE
    scene, cam, view, iv = H.setup_scene(FS.quads_scene)
    r = _renderer(scene, view, iv, w, h)
    r.render_frame()
    r.render_frame()
    for n in (1, 16):
        st = _stats(scene, r, view, iv, n)
        assert FS.quads_scene_conditions(scene, st, w, h) == []
        want = SF.feedback_of(st, scene, w)
        r.set_material_anisotropy(n)
        _same(_taps(r), want, "small quads, anisotropy %d" % n)
        assert not want[FS.T_UNNAMED].any() and not want[FS.T_NON_PBR].any()
        _same(_taps(r, 15, 2, (1, 1)), SF.feedback_of(st, scene, w, 15, 2, (1, 1)), "small quads, stride 2")
        r.set_debug(4194304)                                       # two table entries per workgroup: adds that find the table full
        _same(_taps(r), want, "small quads, anisotropy %d, the table full" % n)
        r.set_debug(0)
    r.close()


# ---- 6. ids at and past the list's ends, and empty pixels, on a caller-owned image --------------------------------------------------------

def test_ids_past_the_list_and_empty_pixels(gpu):
    from chord_amd.renderer import VisibilityRenderer
    w, h = 64, 64
    scene, view, iv = _material_scene(w, h)
    r = VisibilityRenderer(0)
    r.upload_scene(scene)
    r.upload_material_textures()
    img = H.CallerVisibility(r, w, h)
    r.set_view(view, iv, H.ALL_FLAGS)
    r.render_frame()
    cmds = r.read_cmds(r.last_frame_cmds())
    count = len(cmds)
    assert count > 2
    rng = np.random.default_rng(11)
    # 0 empty, 1 slot 0, 2 slot count - 1, 3 slot count, 4 every bit set, 5 a triangle index past the meshlet's, 6 some slot in between
    kind = rng.integers(0, 7, w * h)
    mid = (rng.integers(0, count, w * h) + 1) << 8 | rng.integers(0, 128, w * h)          # (int64)
    low = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5],
                    [0, 1 << 8, count << 8, (count + 1) << 8, 0xFFFFFFFF, (1 << 8) | 255], mid).astype(np.uint64)
    assert all((kind == k).sum() > 100 for k in range(7))
    words = (np.uint64(0x3F000000) << np.uint64(32)) | low
    img.write(words)
    for n in (1, 16):
        st = SF.resolve_stats(scene, words, cmds, view, iv, w, h, n)
        assert not st["hit"][(kind == 0) | (kind == 3) | (kind == 4) | (kind == 5)].any() and st["hit"][kind == 1].all()
        r.set_material_anisotropy(n)
        want = SF.feedback_of(st, scene, w)
        assert want.sum() > 500
        _same(_taps(r), want, "synthetic ids, anisotropy %d" % n)
        _same(_taps(r, 15, 4, (1, 3)), SF.feedback_of(st, scene, w, 15, 4, (1, 3)), "synthetic ids, stride 4")
    assert np.array_equal(img.read(), words)
    r.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------

def test_refusals(gpu):
    w, h = 64, 64
    scene, view, iv = _material_scene(w, h)
    r = _renderer(scene, view, iv, w, h, upload=False)
    ntex = len(scene.texture_images)
    out = np.zeros((ntex, 16), np.uint32)

    def refused(rc, text):
        assert rc == L.E_INVALID, rc
        assert text in L.lib.chordvis_last_error(r._ctx).decode(), L.lib.chordvis_last_error(r._ctx)

    def run(mask=15, stride=1, ox=0, oy=0):
        d = L.FeedbackDesc(mask, stride, (C.c_uint32 * 2)(ox, oy))
        return L.lib.chordvis_material_feedback(r._ctx, r.last_frame_cmds(), C.byref(d))

    refused(L.lib.chordvis_material_feedback_reset(r._ctx), "no chordvis_upload_material_textures")
    refused(run(), "no frame rendered yet")
    r.render_frame()
    refused(run(), "no chordvis_upload_material_textures")
    refused(L.lib.chordvis_readback_material_feedback(r._ctx, out.ctypes.data, ntex), "no chordvis_upload_material_textures")
    r.upload_material_textures()
    refused(run(), "no chordvis_material_feedback_reset since the last chordvis_upload_material_textures")
    refused(L.lib.chordvis_readback_material_feedback(r._ctx, out.ctypes.data, ntex), "no chordvis_material_feedback_reset")
    r.reset_material_feedback()
    refused(L.lib.chordvis_material_feedback(r._ctx, r.last_frame_cmds(), None), "null ChordFeedbackDesc")
    for mask in (0, 16, 0xFFFFFFFF):
        refused(run(mask=mask), "slotMask is 1..15")
    for stride in (0, 3, 5, 16):
        refused(run(stride=stride), "stride is 1, 2, 4 or 8")
    for stride, ox, oy in ((1, 1, 0), (2, 0, 2), (8, 8, 0), (4, 0, 0xFFFFFFFF)):
        refused(run(stride=stride, ox=ox, oy=oy), "each offset is 0 .. stride - 1")
    for n in (ntex - 1, ntex + 1, 0):
        refused(L.lib.chordvis_readback_material_feedback(r._ctx, out.ctypes.data, n), "textureCount is the uploaded descriptor's, %d" % ntex)
    assert run() == L.OK and run(stride=8, ox=7, oy=7) == L.OK
    assert r.read_material_feedback().any()
    r.set_view(view, iv, H.ALL_FLAGS)                             # a stale view, as chordvis_resolve_material refuses it
    refused(run(), "came after the frame")
    r.render_frame()
    assert run() == L.OK
    r.upload_material_textures()                                  # a new upload drops the buffer
    refused(run(), "no chordvis_material_feedback_reset")
    r.reset_material_feedback()
    assert run() == L.OK and not np.array_equal(r.read_material_feedback(), out)
    r.close()


# ---- 8. nothing else moves ---------------------------------------------------------------------------------------------------------------

def test_images_frames_and_defaults_are_untouched(gpu):
    w, h = 65, 67
    scene, view, iv = _material_scene(w, h)
    r, plain = _renderer(scene, view, iv, w, h), _renderer(scene, view, iv, w, h)
    r.set_texture_first_level([2, 1, 3])
    r.set_texture_first_level(None)                               # no setting again
    r.upload_material_textures()
    for i in range(4):
        assert r.texture_first_level(i) == 0
    assert r.material_texture_memory() == plain.material_texture_memory()
    for i, img in enumerate(scene.texture_images):
        levels = max(img.shape[:2]).bit_length()
        assert r.material_texture_levels(i) == (0, levels)
        for l in range(levels):
            assert np.array_equal(r.readback_material_texture(i, l), plain.readback_material_texture(i, l)), (i, l)
    for frame in range(2):
        r.render_frame(); plain.render_frame()
        before = _images(r)
        vis = r.read_visibility()
        taps = _taps(r)
        r.material_feedback(15, 2, (1, 1))
        after = _images(r)
        for n in SM.NAMES:
            assert np.array_equal(before[n], after[n]), n
        assert np.array_equal(r.read_visibility(), vis)
        H.assert_vis_equal(vis, plain.read_visibility(), w, h, "frame %d beside a context that never ran feedback" % frame)
        assert taps.any()
    r.close(); plain.close()


# ---- 9. trimmed chains in every store ----------------------------------------------------------------------------------------------------

def _trim_textures():
    """[0] RGBA8, level 0 alone (the rest made under SRGB | COVERAGE); [1] a full BC3 chain; [2] a full RGBA8 chain of odd size; [3] a
    full RGBA8 chain (compressed at upload in mode BLOCKS); [4] BC3, two levels supplied, the rest made (and encoded in mode BLOCKS);
    [5] BC5, level 0 alone, the rest made.  -> (textures, mips settings, compress targets, finished level counts)"""
    rng = np.random.default_rng(40)
    level0 = rng.integers(0, 256, size=(32, 64, 4), dtype=np.uint8)
    level0[..., 3] = np.where(rng.random((32, 64)) < 0.4, rng.integers(0, 120, size=(32, 64)), level0[..., 3] | 128)
    two = [rng.integers(0, 256, size=(lh, lw, 4), dtype=np.uint8) for lw, lh in BC.level_dims(32, 16, 2)]
    textures = [R.TextureChain(level0.reshape(-1), 64, 32, 1, BC.RGBA8),
                R.bc_chain(rng.integers(0, 256, size=(32, 32, 4), dtype=np.uint8), BC.BC3),
                rng.integers(0, 256, size=(12, 20, 4), dtype=np.uint8),
                rng.integers(0, 256, size=(16, 16, 4), dtype=np.uint8),
                R.TextureChain(np.concatenate([R.encode_bc(l, BC.BC3) for l in two]), 32, 16, 2, BC.BC3),
                R.TextureChain(R.encode_bc(rng.integers(0, 256, size=(16, 16, 4), dtype=np.uint8), BC.BC5), 16, 16, 1, BC.BC5)]
    flags = M.SRGB | M.COVERAGE
    mips = [(L.TEXMIPS_FULL, flags, 128), (0, 0, 0), (0, 0, 0), (0, 0, 0), (L.TEXMIPS_FULL, flags, 128), (L.TEXMIPS_FULL, 0, 0)]
    compress = [0, 0, 0, BC.BC1_RGB, BC.BC3, 0]
    return textures, mips, compress, [7, 6, 5, 5, 6, 5]


def _trim_scene(textures):
    """small_test_scene at 64 x 64 with one opaque material per texture k -- base colour k (trilinear), emissive (k + 3) % 6
    (nearest mip level) --, given to the objects so that every texture covers hundreds of pixels"""
    base, cam = scenes.small_test_scene(64, 64, lods=1)
    assert len(textures) == 6 and len(base.objects) == 8
    mats = np.zeros(6, dtype=R.MATERIAL)
    mats[:] = base.materials[0]
    mats["alphaMode"] = R.ALPHA_OPAQUE
    for s in ("normalTexture", "metallicRoughnessTexture"):
        mats[s] = FS.NO_TEXTURE
    mats["baseColorId"], mats["baseColorSampler"] = np.arange(6), 0
    mats["emissiveTexture"], mats["emissiveSampler"] = (np.arange(6) + 3) % 6, 1
    mats["emissiveFactor"] = 1.0
    objs = base.objects.copy()
    objs["GLTFMaterialData"] = [0, 1, 3, 3, 5, 2, 4, 5]           # (objects 0, 1, 5 and 6 fill most of the view)
    smp = np.array([(R.FILTER_LINEAR_MIPMAP_LINEAR, R.FILTER_LINEAR, R.WRAP_REPEAT, R.WRAP_MIRRORED_REPEAT),
                    (R.FILTER_NEAREST_MIPMAP_NEAREST, R.FILTER_LINEAR, R.WRAP_CLAMP_TO_EDGE, R.WRAP_REPEAT)], dtype=R.SAMPLER)
    # (the scene has no texture coordinates of its own: a shear of the local positions, so that walls have a gradient too)
    x, y, z = (base.positions[:, k].astype(np.float64) for k in range(3))
    uv = np.ascontiguousarray(np.stack([x * 0.9 + y * 0.6, z * 0.8 + y * 0.5], axis=1), dtype=np.float32)
    scene = R.Scene(objs, base.primitives, mats, base.meshlets, base.groups, base.group_indices, base.meshlet_data, base.positions,
                    texcoord0=uv, textures=textures, samplers=smp, bvh_nodes=base.bvh_nodes)
    scene.local_to_world = base.local_to_world
    L.fill_objects(scene, cam)
    view, iv = L.make_views(cam)
    return scene, view, iv


def _trim_renderer(scene, view, iv, store, mips, compress, first):
    from chord_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(0)
    r.set_material_texture_store(store)
    r.set_texture_mips(mips)
    if store == L.TEXSTORE_BLOCKS:
        r.set_texture_compress(compress)
    r.set_texture_first_level(first)
    r.upload_scene(scene)
    r.upload_material_textures()
    r.allocate_gbuffer(64, 64)
    r.set_view(view, iv, H.ALL_FLAGS)
    return r


@pytest.mark.parametrize("store", [L.TEXSTORE_EXPANDED, L.TEXSTORE_BLOCKS], ids=["texels", "blocks"])
def test_trimmed_chains(gpu, store):
    textures, mips, compress, counts = _trim_textures()
    scene, view, iv = _trim_scene(textures)
    # which format each texture is kept in (0: texels)
    kept = [0, BC.BC3, 0, BC.BC1_RGB, BC.BC3, 0] if store == L.TEXSTORE_BLOCKS else [0] * 6
    whole = _trim_renderer(scene, view, iv, store, mips, compress, None)
    dims = [(t.shape[1], t.shape[0]) for t in textures]
    finished = []
    for i, n in enumerate(counts):
        assert whole.material_texture_levels(i) == (0, n)
        finished.append([whole.readback_material_texture(i, l) for l in range(n)])
    blocks = {i: whole.readback_material_blocks(i, kept[i], counts[i]) for i in range(6) if kept[i]}
    whole.render_frame()
    vis = whole.read_visibility()

    def chain_bytes(i, f):
        w, h = max(1, dims[i][0] >> f), max(1, dims[i][1] >> f)
        return L.texture_chain_bytes(kept[i], w, h, counts[i] - f)

    for first in ([1, 2, 1, 2, 1, 3], [2, 1, 3, 1, 3, 1], [99, 6, 5, 4, 0xFFFFFFFF, 5]):
        r = _trim_renderer(scene, view, iv, store, mips, compress, first)
        texel_bytes = block_bytes = 0
        for i, n in enumerate(counts):
            f = min(first[i], n - 1)
            assert r.texture_first_level(i) == first[i]
            assert r.material_texture_levels(i) == (f, n - f), (first, i)
            for l in range(n - f):
                got = r.readback_material_texture(i, l)
                assert got.shape == finished[i][f + l].shape and np.array_equal(got, finished[i][f + l]), (first, i, l)
            out = np.zeros(4, np.uint8)
            assert L.lib.chordvis_readback_material_texture(r._ctx, i, n - f, out.ctypes.data) == L.E_INVALID
            if kept[i]:
                skip = len(blocks[i]) - chain_bytes(i, f)
                assert np.array_equal(r.readback_material_blocks(i, kept[i], n), blocks[i][skip:]), (first, i)
                assert L.lib.chordvis_readback_material_blocks(r._ctx, i, np.zeros(1 << 14, np.uint8).ctypes.data, len(blocks[i])) == L.E_INVALID
                block_bytes += (chain_bytes(i, f) + 15) // 16 * 16
            else:
                texel_bytes += 4 * sum(lv.shape[0] * lv.shape[1] for lv in finished[i][f:])
        assert r.material_texture_memory() == (texel_bytes, block_bytes), first
        assert sum(r.material_texture_memory()) < sum(whole.material_texture_memory())
        if first[0] == 99:
            assert [r.material_texture_levels(i)[1] for i in range(6)] == [1, 1, 1, 1, 1, 1]
        # the frame does not read the setting; the images are the spec's, given the smaller textures
        r.render_frame()
        H.assert_vis_equal(r.read_visibility(), vis, 64, 64, "the frame of a trimmed context")
        small = SF.trimmed(scene, first, {i: finished[i] for i in range(6)})
        cmds = r.read_cmds(r.last_frame_cmds())
        for n in (1, 16):
            r.set_material_anisotropy(n)
            names = ("baseColor", "emissive")
            want = SM.resolve(small, vis, cmds, view, iv, 64, 64, names=names) if n == 1 else \
                SA.resolve(small, vis, cmds, view, iv, 64, 64, names=names, max_aniso=n)
            got = _images(r, names)
            for name in names:
                assert np.array_equal(got[name], np.ascontiguousarray(want[name]).view(np.uint32)), (first, n, name)
                assert np.any(got[name])
            _same(_taps(r), SF.feedback(small, vis, cmds, view, iv, 64, 64, 15, 1, (0, 0), n), "feedback rows of trimmed textures")
        r.close()
    whole.close()


# ---- 10. the closed loop -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("store", [L.TEXSTORE_EXPANDED, L.TEXSTORE_BLOCKS], ids=["texels", "blocks"])
def test_closed_loop(gpu, store):
    """feedback at stride 1 -> first = the lowest tapped level of each texture -> re-upload: the same images in less memory"""
    w = h = FS.SIZE
    scene, cam, view, iv = H.setup_scene(FS.loop_scene)
    if store == L.TEXSTORE_BLOCKS:
        scene = BC.bc_scene(scene, [BC.BC3, BC.BC1_RGB, BC.BC5])
    r = _renderer(scene, view, iv, w, h, store)
    r.render_frame()
    r.render_frame()
    vis = r.read_visibility()
    for n in (1, 16):
        r.set_material_anisotropy(n)
        r.set_texture_first_level(None)
        r.upload_material_textures()
        before, memory = _images(r), sum(r.material_texture_memory())
        first = FS.first_levels(_taps(r))
        assert max(first) >= 2 and min(first) == 0, first
        r.set_texture_first_level(first)
        r.upload_material_textures()
        assert [r.material_texture_levels(i)[0] for i in range(3)] == first
        after = _images(r)
        for name in SM.NAMES:
            assert np.array_equal(before[name], after[name]), (n, name)
            assert np.any(after[name]), name
        assert sum(r.material_texture_memory()) < memory
        assert np.array_equal(r.read_visibility(), vis)
        shifted = _taps(r)                                        # the rows now count from the first stored level
        assert FS.first_levels(shifted) == [0, 0, 0]
    r.close()
