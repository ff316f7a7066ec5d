"""chordvis_set_texture_compress through the C ABI on the GPU: RGBA8 textures block-compressed at upload under CHORD_TEXSTORE_BLOCKS.
The chains read back by chordvis_readback_material_blocks equal tests/spec_texture_encode_np.py byte for byte -- on the fixture's
blocks that is the reference importer's own output (tests/golden/texture_encode.npz) --, made levels follow spec_texture_mips_np, the
resolve images equal those of the spec-encoded chains supplied as BC input, word for word; the memory figures, the refusals and the
unchanged defaults."""
import os

import numpy as np
import pytest

from chord_amd import lib as L, records as R, scenes

import helpers as H
import spec_texture_bc_np as BC
import spec_texture_encode_np as E
import spec_texture_mips_np as M

pytestmark = pytest.mark.gpu

FORMATS = [BC.BC1_RGB, BC.BC3, BC.BC4, BC.BC5]
KEYS = {BC.BC1_RGB: "bc1", BC.BC3: "bc3", BC.BC4: "bc4", BC.BC5: "bc5"}
SIZES = [(1, 1), (2, 2), (4, 4), (5, 7), (8, 8), (20, 12)]                               # (width, height), full chains, all supplied
NO_TEXTURE = 0xFFFFFFFF
MATERIAL_FORMATS = [BC.BC3, BC.BC3, BC.BC5, BC.BC1_RGB, BC.BC3]                          # albedo, noise, normal, ORM, emissive
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "texture_encode.npz")


def _texture_scene(textures):
    """A small scene with one opaque material per texture, naming it as its base colour."""
    base, cam = scenes.small_test_scene(64, 48, lods=1)
    mats = np.zeros(len(textures), dtype=R.MATERIAL)
    mats[:] = base.materials[0]
    mats["alphaMode"] = R.ALPHA_OPAQUE
    for s in ("emissiveTexture", "normalTexture", "metallicRoughnessTexture"):
        mats[s] = NO_TEXTURE
    mats["baseColorId"] = np.arange(len(textures))
    objs = base.objects.copy()
    objs["GLTFMaterialData"] = 0
    return R.Scene(objs, base.primitives, mats, base.meshlets, base.groups, base.group_indices, base.meshlet_data, base.positions,
                   textures=textures, bvh_nodes=base.bvh_nodes)


def _renderer(scene, store, compress=None, mips=None, upload=True, materials_of=None):
    """materials_of: the scene whose textures the material upload takes (default: `scene`, as the frame's alpha test does)"""
    from chord_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(0)
    r.set_material_texture_store(store)
    if mips:
        r.set_texture_mips(mips)
    if compress:
        r.set_texture_compress(compress)
    r.upload_scene(scene)
    if upload:
        r.upload_material_textures(materials_of)
    return r


def _rgba8_chain(levels):
    h, w = levels[0].shape[:2]
    return R.TextureChain(M.chain_bytes(levels), w, h, len(levels), BC.RGBA8)


def _random_levels(rng, w, h, count):
    return [rng.integers(0, 256, size=(lh, lw, 4), dtype=np.uint8) for lw, lh in BC.level_dims(w, h, count)]


def _assert_chain(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError("%s: %d bytes differ; first at %d (8-byte unit %d): got %s want %s" % (
            what, len(bad), bad[0], bad[0] // 8, got[bad[0] // 8 * 8:bad[0] // 8 * 8 + 8], want[bad[0] // 8 * 8:bad[0] // 8 * 8 + 8]))


def _block_bytes(chains):
    """[(format, width, height, levels)] -> the block store's bytes"""
    return sum((L.texture_chain_bytes(f, w, h, n) + 15) // 16 * 16 for f, w, h, n in chains)


def _frames(r, cam, view, iv, count=2):
    r.allocate_gbuffer(cam.width, cam.height)
    r.set_view(view, iv, H.ALL_FLAGS)
    out = []
    for _ in range(count):
        r.render_frame()
        out.append(r.read_visibility())
    return out


def _resolve(r, names):
    import torch
    out = r.resolve_attributes(names=list(names))
    torch.cuda.synchronize()
    return {n: t.cpu().numpy().view(np.uint32) for n, t in out.items()}


# ---- 1. the encoded chains, byte for byte ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("format", FORMATS, ids=["bc1", "bc3", "bc4", "bc5"])
def test_encoded_chains_equal_the_spec(gpu, format):
    d = np.load(GOLDEN)
    blocks = d["blocks"]
    n = len(blocks)
    pages = (n + 255) // 256
    tiled = []                                                             # 64 x 64 textures of 16 x 16 fixture blocks, level 0 alone
    for p in range(pages):
        idx = np.arange(256 * p, 256 * p + 256) % n
        img = blocks[idx].reshape(16, 16, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(64, 64, 4)
        tiled.append(_rgba8_chain([np.ascontiguousarray(img)]))
    rng = np.random.default_rng(500 + format)
    full = [_random_levels(rng, w, h, max(w, h).bit_length()) for w, h in SIZES]
    level0 = rng.integers(0, 256, size=(32, 64, 4), dtype=np.uint8)
    level0[..., 3] = np.where(rng.random((32, 64)) < 0.4, rng.integers(0, 120, size=(32, 64)), level0[..., 3] | 128)
    textures = tiled + [_rgba8_chain(lv) for lv in full] + [_rgba8_chain([level0]), _rgba8_chain([level0])]
    flags = M.SRGB | M.COVERAGE
    mips = [(0, 0, 0)] * (len(textures) - 2) + [(L.TEXMIPS_FULL, 0, 0), (L.TEXMIPS_FULL, flags, 128)]
    r = _renderer(_texture_scene(textures), L.TEXSTORE_BLOCKS, [format] * len(textures), mips)
    for p in range(pages):                                                 # the reference's bytes directly
        idx = np.arange(256 * p, 256 * p + 256) % n
        _assert_chain(r.readback_material_blocks(p), d[KEYS[format]][idx].reshape(-1), "format %d, fixture page %d against the reference's bytes" % (format, p))
    for i, lv in enumerate(full, pages):
        _assert_chain(r.readback_material_blocks(i), E.encode_chain(lv, format), "format %d, full chain %d x %d" % (format, lv[0].shape[1], lv[0].shape[0]))
        for l, img in enumerate(BC.decode_chain(E.encode_chain(lv, format), lv[0].shape[1], lv[0].shape[0], len(lv), format)):
            assert np.array_equal(r.readback_material_texture(i, l), img), (format, i, l)
    for i, (fl, cut) in enumerate(((0, 0), (flags, 128)), pages + len(full)):
        want = M.build_chain([level0], M.FULL, fl, cut)
        assert len(want) == 7
        _assert_chain(r.readback_material_blocks(i), E.encode_chain(want, format), "format %d, 64 x 32 with made levels, flags %d" % (format, fl))
    chains = [(format, 64, 64, 1)] * pages + [(format, w, h, max(w, h).bit_length()) for w, h in SIZES] + [(format, 64, 32, 7)] * 2
    assert r.material_texture_memory() == (0, _block_bytes(chains))
    r.close()


# ---- 2., 3. a block-compressed source ----------------------------------------------------------------------------------------------

def _bc3_source():
    rng = np.random.default_rng(77)
    levels = _random_levels(rng, 32, 16, 2)
    levels[0][..., 3] = np.where(rng.random((16, 32)) < 0.5, 20, 230)
    data = np.concatenate([R.encode_bc(l, BC.BC3) for l in levels])      # (the tests' simple encoder: not what the library would write)
    return R.TextureChain(data, 32, 16, 2, BC.BC3)


def test_supplied_levels_stay_verbatim_and_made_levels_are_encoded(gpu):
    src = _bc3_source()
    flags = M.SRGB | M.COVERAGE
    r = _renderer(_texture_scene([src]), L.TEXSTORE_BLOCKS, [BC.BC3], [(L.TEXMIPS_FULL, flags, 128)])
    got = r.readback_material_blocks(0)
    levels = M.build_chain(BC.decode_chain(src.data, 32, 16, 2, BC.BC3), M.FULL, flags, 128)
    assert len(levels) == 6
    assert len(got) == L.texture_chain_bytes(BC.BC3, 32, 16, 6)
    _assert_chain(got[:len(src.data)], src.data, "the supplied levels")
    assert not np.array_equal(src.data, E.encode_chain(levels[:2], BC.BC3))            # (re-encoding them would have shown)
    _assert_chain(got[len(src.data):], E.encode_chain(levels[2:], BC.BC3), "the made levels")
    for l, img in enumerate(BC.decode_chain(got, 32, 16, 6, BC.BC3)):
        assert np.array_equal(r.readback_material_texture(0, l), img), l
    assert r.material_texture_memory() == (0, _block_bytes([(BC.BC3, 32, 16, 6)]))
    r.close()


@pytest.mark.parametrize("mips", [None, [(L.TEXMIPS_FULL, 0, 0)]], ids=["as supplied", "made levels"])
def test_another_block_format_is_refused(gpu, mips):
    r = _renderer(_texture_scene([_bc3_source()]), L.TEXSTORE_BLOCKS, [BC.BC1_RGB], mips, upload=False)
    with pytest.raises(L.ChordvisError, match="differs from its chordvis_set_texture_compress target"):
        r.upload_material_textures()
    t, b = L.C.c_uint64(7), L.C.c_uint64(7)
    assert L.lib.chordvis_material_texture_memory(r._ctx, L.C.byref(t), L.C.byref(b)) == L.E_INVALID      # nothing uploaded
    r.set_texture_compress([BC.BC3])                                       # the same source under its own format is fine
    r.upload_material_textures()
    r.close()


# ---- 4., 5. the material scene -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def material_scene():
    scene, cam, view, iv = H.setup_scene(scenes.material_test_scene, 320, 200)
    chains = []
    for img, f in zip(scene.texture_images, MATERIAL_FORMATS):
        data, mips = R.mip_chain_rgba8(img)
        h, w = img.shape[:2]
        chains.append(R.TextureChain(E.encode_chain(M.split_chain(data, w, h, mips), f), w, h, mips, f))
    return scene, scenes.with_textures(scene, chains), cam, view, iv


def test_material_scene_equals_the_spec_encoded_chains(gpu, material_scene):
    scene, encoded, cam, view, iv = material_scene
    # (both frames test the alpha of the encoded chains -- chordvis_upload_scene never encodes --, so the two contexts resolve the
    # same visibility; the material upload of the first takes the RGBA8 images and encodes them)
    rb = _renderer(encoded, L.TEXSTORE_BLOCKS, MATERIAL_FORMATS, materials_of=scene)
    re = _renderer(encoded, L.TEXSTORE_EXPANDED)
    chains = [(t.format, t.width, t.height, t.mips) for t in encoded.texture_images]
    assert rb.material_texture_memory() == (0, _block_bytes(chains))
    for i, t in enumerate(encoded.texture_images):
        _assert_chain(rb.readback_material_blocks(i), t.data, "material texture %d" % i)
    fb, fe = _frames(rb, cam, view, iv), _frames(re, cam, view, iv)
    H.assert_vis_equal(fb[1], fe[1], cam.width, cam.height, "encoded at upload against supplied as blocks")
    for n in (1, 8):
        rb.set_material_anisotropy(n)
        re.set_material_anisotropy(n)
        a, b = _resolve(rb, L.MATERIAL_CHANNELS), _resolve(re, L.MATERIAL_CHANNELS)
        assert len(a) == 4
        for k in L.MATERIAL_CHANNELS:
            assert np.any(a[k]), (n, k)
            if not np.array_equal(a[k], b[k]):
                bad = np.argwhere(a[k] != b[k])
                raise AssertionError("anisotropy %d %s: %d words differ; first %s" % (n, k, len(bad), bad[0]))
    rb.close(); re.close()


def test_memory_with_one_texture_left_as_texels(gpu, material_scene):
    scene, encoded, _, _, _ = material_scene
    targets = list(MATERIAL_FORMATS)
    targets[1] = 0
    r = _renderer(scene, L.TEXSTORE_BLOCKS, targets)
    t1 = encoded.texture_images[1]
    texels = sum(w * h for w, h in BC.level_dims(t1.width, t1.height, t1.mips))
    others = [(t.format, t.width, t.height, t.mips) for i, t in enumerate(encoded.texture_images) if i != 1]
    assert r.material_texture_memory() == (4 * texels, _block_bytes(others))
    data, mips = R.mip_chain_rgba8(scene.texture_images[1])
    for l, img in enumerate(M.split_chain(data, t1.width, t1.height, mips)):
        assert np.array_equal(r.readback_material_texture(1, l), img), l
    _assert_chain(r.readback_material_blocks(2), encoded.texture_images[2].data, "a neighbour of the texture left as texels")
    r.close()


# ---- 6. unchanged defaults ---------------------------------------------------------------------------------------------------------

def test_defaults_are_unchanged(gpu, material_scene):
    scene = material_scene[0]
    plain = _renderer(scene, L.TEXSTORE_BLOCKS)                            # never made the call
    unset = _renderer(scene, L.TEXSTORE_BLOCKS)
    unset.set_texture_compress(MATERIAL_FORMATS)
    unset.set_texture_compress(None)                                       # no setting again
    unset.upload_material_textures()
    expanded = _renderer(scene, L.TEXSTORE_EXPANDED, MATERIAL_FORMATS)     # a setting, ignored in mode EXPANDED
    assert plain.material_texture_memory()[1] == 0
    for r in (unset, expanded):
        assert r.material_texture_memory() == plain.material_texture_memory()
        for i, img in enumerate(scene.texture_images):
            for l in range(max(img.shape[0], img.shape[1]).bit_length()):
                assert np.array_equal(r.readback_material_texture(i, l), plain.readback_material_texture(i, l)), (i, l)
    out = np.zeros(1 << 20, np.uint8)
    for r in (plain, expanded):                                            # kept as texels: no blocks to read
        n = L.texture_chain_bytes(BC.BC3, 128, 128, 8)
        assert L.lib.chordvis_readback_material_blocks(r._ctx, 0, out.ctypes.data, n) == L.E_INVALID
        assert "not kept as blocks" in r.last_error()
    plain.close(); unset.close(); expanded.close()


def test_setting(gpu):
    from chord_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(0)
    assert r.texture_compress(0) == 0
    out = np.zeros(64, np.uint8)
    assert L.lib.chordvis_readback_material_blocks(r._ctx, 0, out.ctypes.data, 8) == L.E_INVALID          # nothing uploaded
    r.set_texture_compress([BC.BC1_RGB, 0, BC.BC5])
    for bad in ([5], [BC.BC3, 0xFFFFFFFF], [BC.BC3, 7, 0]):
        with pytest.raises(L.ChordvisError, match=r"0 \(none\), 1 \(BC1_RGB\), 2 \(BC3\), 3 \(BC4\), 4 \(BC5\)"):
            r.set_texture_compress(bad)
        assert [r.texture_compress(i) for i in range(4)] == [BC.BC1_RGB, 0, BC.BC5, 0], "the getter returns the last accepted array"
    rng = np.random.default_rng(9)
    lv = _random_levels(rng, 8, 8, 4)
    scene = _texture_scene([_rgba8_chain(lv)] * 3)
    r.set_material_texture_store(L.TEXSTORE_BLOCKS)
    r.upload_scene(scene)                                                  # kept across both uploads
    r.upload_material_textures()
    assert [r.texture_compress(i) for i in range(4)] == [BC.BC1_RGB, 0, BC.BC5, 0]
    _assert_chain(r.readback_material_blocks(0), E.encode_chain(lv, BC.BC1_RGB), "texture 0")
    _assert_chain(r.readback_material_blocks(2), E.encode_chain(lv, BC.BC5), "texture 2")
    n = L.texture_chain_bytes(BC.BC1_RGB, 8, 8, 4)
    assert L.lib.chordvis_readback_material_blocks(r._ctx, 0, out.ctypes.data, n + 8) == L.E_INVALID      # the wrong size
    assert L.lib.chordvis_readback_material_blocks(r._ctx, 1, out.ctypes.data, n) == L.E_INVALID          # kept as texels
    assert L.lib.chordvis_readback_material_blocks(r._ctx, 3, out.ctypes.data, n) == L.E_INVALID          # no such texture
    assert r.material_texture_memory() == (4 * 85, _block_bytes([(BC.BC1_RGB, 8, 8, 4), (BC.BC5, 8, 8, 4)]))
    r.set_texture_compress([])                                             # read by later uploads only
    _assert_chain(r.readback_material_blocks(0, BC.BC1_RGB, 4), E.encode_chain(lv, BC.BC1_RGB), "texture 0 after the setting is cleared")
    r.upload_material_textures()
    assert r.material_texture_memory() == (3 * 4 * 85, 0)
    r.close()
