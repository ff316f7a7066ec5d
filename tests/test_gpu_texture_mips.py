"""Mip chains made on the GPU at upload (chordvis_set_texture_mips) through the C ABI: every generated level bit for bit against
tests/spec_texture_mips_np.py, chains supplied in part, block-compressed sources, the masked frame under coverage-preserving alpha
against the same scene handed over with the spec-built chains (and against the oracle's), the refusals and the defaults."""

import numpy as np
import pytest

from chord_amd import lib as L, records as R, scenes

import helpers as H
import spec_texture_bc_np as BC
import spec_texture_mips_np as M

pytestmark = pytest.mark.gpu

SIZES = [(2, 2), (5, 3), (7, 9), (64, 64), (130, 66), (260, 4), (4, 260), (512, 256)]     # (width, height)
SETTINGS = [(0, 0), (M.SRGB, 0), (M.COVERAGE, 64), (M.COVERAGE, 200), (M.SRGB | M.COVERAGE, 128)]
NO_TEXTURE = 0xFFFFFFFF
FULL = L.TEXMIPS_FULL


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


def _level0(img):
    """An image handed over as level 0 alone."""
    return R.TextureChain(img.reshape(-1), img.shape[1], img.shape[0], 1)


def _renderer(scene, settings, materials=True):
    from chord_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(0)
    r.set_texture_mips(settings)
    r.upload_scene(scene)
    if materials:
        r.upload_material_textures()
    return r


def _check_levels(r, tid, want, what):
    for l, lv in enumerate(want):
        got = r.readback_material_texture(tid, l)
        assert got.shape == lv.shape, (what, l)
        if not np.array_equal(got, lv):
            bad = np.argwhere((got != lv).any(axis=2))
            raise AssertionError("%s level %d (%d x %d): %d texels differ; first (y, x) = %s got %s want %s" % (
                what, l, lv.shape[1], lv.shape[0], len(bad), bad[0], got[tuple(bad[0])], lv[tuple(bad[0])]))
    out = np.zeros(4, np.uint8)
    assert L.lib.chordvis_readback_material_texture(r._ctx, tid, len(want), out.ctypes.data) == L.E_INVALID, what


@pytest.fixture(scope="module")
def images():
    rng = np.random.default_rng(2024)
    return [rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8) for w, h in SIZES]


@pytest.mark.parametrize("flags,cutoff", SETTINGS, ids=["codes", "srgb", "coverage64", "coverage200", "srgb_coverage128"])
def test_levels_equal_the_spec(gpu, images, flags, cutoff):
    """(130, 66) and (512, 256) start with launches per level step and end in the workgroup that finishes a chain; the thin sizes
    keep a dimension at 1 over many levels; the others are made by that workgroup alone."""
    r = _renderer(_texture_scene([_level0(i) for i in images]), [(FULL, flags, cutoff)] * len(images))
    idle = True
    for tid, img in enumerate(images):
        ts = []
        want = M.build_chain([img], M.FULL, flags, cutoff, ts)
        assert len(want) == M.full_levels(img.shape[1], img.shape[0])
        idle = idle and all(t == cutoff for _, t in ts)
        _check_levels(r, tid, want, "flags %d %d x %d" % (flags, img.shape[1], img.shape[0]))
        if flags == 0:
            chain, mips = R.mip_chain_rgba8(img)
            _check_levels(r, tid, M.split_chain(chain, img.shape[1], img.shape[0], mips), "mip_chain_rgba8 %d x %d" % img.shape[1::-1])
    assert idle == (not flags & M.COVERAGE)                       # under COVERAGE some level's threshold is not the cutoff
    r.close()


def test_chains_supplied_in_part(gpu):
    rng = np.random.default_rng(31)
    three = [rng.integers(0, 256, size=(64 >> l, 64 >> l, 4), dtype=np.uint8) for l in range(3)]      # (not a box chain)
    two = [rng.integers(0, 256, size=(256 >> l, 256 >> l, 4), dtype=np.uint8) for l in range(2)]
    t3 = R.TextureChain(M.chain_bytes(three), 64, 64, 3)
    t2 = R.TextureChain(M.chain_bytes(two), 256, 256, 2)
    settings = [(FULL, 0, 0), (5, 0, 0), (2, 0, 0), (0, M.SRGB, 0), (FULL, M.SRGB | M.COVERAGE, 100), (3, M.COVERAGE, 100)]
    r = _renderer(_texture_scene([t3, t3, t3, t3, t2, t2]), settings)
    assert r.texture_mips(4) == (FULL, 3, 100, 0) and r.texture_mips(6) == (0, 0, 0, 0)
    _check_levels(r, 0, M.build_chain(three, M.FULL), "3 of 7 levels supplied")
    assert len(M.build_chain(three, M.FULL)) == 7
    _check_levels(r, 1, M.build_chain(three, 5), "levels = 5")
    assert len(M.build_chain(three, 5)) == 5
    _check_levels(r, 2, three, "levels = 2 <= mipCount")
    _check_levels(r, 3, three, "levels = 0")
    want = M.build_chain(two, M.FULL, M.SRGB | M.COVERAGE, 100)
    assert len(want) == 9 and np.array_equal(want[1], two[1])
    _check_levels(r, 4, want, "2 of 9 levels supplied, sRGB and coverage")
    _check_levels(r, 5, M.build_chain(two, 3, M.COVERAGE, 100), "levels = 3")
    r.close()


def test_block_compressed_sources(gpu):
    """Level 0 alone in BC3 / BC1_RGB: decoded on the device, then reduced; the chain is the spec's on the spec-decoded level 0."""
    rng = np.random.default_rng(32)
    cases = [(BC.BC3, 130, 66), (BC.BC3, 37, 21), (BC.BC1_RGB, 130, 66), (BC.BC1_RGB, 7, 9)]
    textures = []
    for f, w, h in cases:
        img = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
        textures.append(R.TextureChain(R.encode_bc(img, f), w, h, 1, f))
    r = _renderer(_texture_scene(textures), [(FULL, M.SRGB | M.COVERAGE, 128)] * len(cases))
    for tid, (t, (f, w, h)) in enumerate(zip(textures, cases)):
        level0 = BC.decode_chain(t.data, w, h, 1, f)
        want = M.build_chain(level0, M.FULL, M.SRGB | M.COVERAGE, 128)
        if f == BC.BC1_RGB:
            assert all((lv[..., 3] == 255).all() for lv in want)
        _check_levels(r, tid, want, "format %d %d x %d" % (f, w, h))
    r.close()
    # the alpha plane of the scene upload: BC3 alpha reduced and rescaled, BC1_RGB 255 through all L levels
    src, _ = scenes.masked_test_scene(160, 100)
    cut = [128, 114, 90]
    for f in (BC.BC3, BC.BC1_RGB):
        tex = [R.TextureChain(R.encode_bc(t, f), t.shape[1], t.shape[0], 1, f) for t in src.texture_images]
        r = _renderer(scenes.with_textures(src, tex), [(FULL, M.COVERAGE, c) for c in cut], materials=False)
        want = np.concatenate([M.chain_bytes(M.build_chain(BC.decode_chain(t.data, t.width, t.height, 1, f), M.FULL, M.COVERAGE, c))[3::4]
                               for t, c in zip(tex, cut)])
        got = r.read_alpha_plane(len(want))
        assert np.array_equal(got, want), (f, int((got != want).sum()))
        if f == BC.BC1_RGB:
            assert (got == 255).all()
        r.close()


def _two_frames(r, cam, view, iv):
    r.allocate_gbuffer(cam.width, cam.height)
    r.set_view(view, iv, H.ALL_FLAGS)
    out = []
    for _ in range(2):
        r.render_frame()
        out.append(r.read_visibility())
    return out


def _resolve(r, names):
    import torch
    out = r.resolve_attributes(names=names)
    torch.cuda.synchronize()
    return {n: t.cpu().numpy().view(np.uint32) for n, t in out.items()}


def test_masked_frame_under_coverage(gpu):
    """masked_test_scene with its textures handed over as level 0 alone and COVERAGE at the cutoffs of the materials that sample
    them (alphaCutOff / baseColorFactor.w as a code, rounded up: 0.5 / 1, 0.4 / 0.9, 0.35 / 1)."""
    import orc
    scene, cam, view, iv = H.setup_scene(scenes.masked_test_scene, 320, 200, attributes=True)
    w, h = cam.width, cam.height
    cut = [128, 114, 90]
    settings = [(FULL, M.COVERAGE, c) for c in cut]
    alone = scenes.with_textures(scene, [_level0(t) for t in scene.texture_images])
    chains, active = [], False
    for t, c in zip(scene.texture_images, cut):
        ts = []
        chains.append(M.build_chain([t], M.FULL, M.COVERAGE, c, ts))
        active = active or any(tp != c for _, tp in ts)
    assert active                                                 # the rescale is not idle
    twin = scenes.with_textures(scene, [R.TextureChain(M.chain_bytes(ch), ch[0].shape[1], ch[0].shape[0], len(ch)) for ch in chains])
    want_alpha = np.concatenate([M.chain_bytes(ch)[3::4] for ch in chains])

    r = _renderer(alone, settings)
    got_alpha = r.read_alpha_plane(len(want_alpha))
    assert np.array_equal(got_alpha, want_alpha), int((got_alpha != want_alpha).sum())
    for tid, ch in enumerate(chains):                             # the same alpha in the alpha bytes of the RGBA8 store
        _check_levels(r, tid, ch, "texture %d" % tid)
    got = _two_frames(r, cam, view, iv)
    rt = _renderer(twin, None)
    assert np.array_equal(rt.read_alpha_plane(len(want_alpha)), want_alpha)
    got_twin = _two_frames(rt, cam, view, iv)
    want0 = orc.frame(twin, view, iv, H.ALL_FLAGS)
    want1 = orc.frame(twin, view, iv, H.ALL_FLAGS, prev_hzb_min=want0["hzb_min"])
    for k, want in enumerate((want0, want1)):
        H.assert_vis_equal(got[k], got_twin[k], w, h, "frame %d against the GPU's frame of the twin" % k)
        H.assert_vis_equal(got[k], want["vis"], w, h, "frame %d against the oracle on the twin" % k)
    # the rescale reaches pixels: the plain box chain (what Scene builds from an image) gives another frame
    rp = _renderer(scene, None)
    plain = _two_frames(rp, cam, view, iv)
    assert not np.array_equal(plain[1], got[1])
    # ... and so does the same upload without COVERAGE, which is the plain box chain's frame
    rb = _renderer(alone, [(FULL, 0, 0)] * 3)
    box = _two_frames(rb, cam, view, iv)
    for k in range(2):
        H.assert_vis_equal(box[k], plain[k], w, h, "flags 0 frame %d against the host-built box chain's" % k)
    names = list(L.RESOLVE_CHANNELS) + list(L.SURFACE_CHANNELS) + list(L.MATERIAL_CHANNELS)
    assert len(names) == 15
    for n in (1, 8):
        for x in (r, rt):
            x.set_material_anisotropy(n)
        a, b = _resolve(r, names), _resolve(rt, names)
        for k in names:
            assert np.array_equal(a[k], b[k]), (n, k, int((a[k] != b[k]).sum()))
        assert np.any(a["baseColor"])
    for x in (r, rt, rp, rb):
        x.close()


def test_refusals_and_defaults(gpu):
    from chord_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(0)
    assert r.texture_mips(0) == (0, 0, 0, 0)
    good = [(FULL, M.SRGB | M.COVERAGE, 255), (3, 0, 999), (0, M.COVERAGE, 1)]          # (without COVERAGE the cutoff is ignored)
    r.set_texture_mips(good)
    for bad in [(FULL, 4, 0), (FULL, 0x80000000, 0), (FULL, M.COVERAGE, 0), (FULL, M.COVERAGE, 256), (FULL, M.SRGB | M.COVERAGE, 0),
                L.TextureMips(FULL, 0, 0, 1)]:
        with pytest.raises(L.ChordvisError, match=r"flags: 0, 1 .SRGB., 2 .COVERAGE. or 3; pad: 0; alphaCutoff8 with COVERAGE: 1..255"):
            r.set_texture_mips([(0, 0, 0), bad])
        assert [r.texture_mips(i) for i in range(4)] == [g + (0,) for g in good] + [(0, 0, 0, 0)]
    assert L.lib.chordvis_texture_mips(r._ctx, 0, None) == L.E_INVALID
    r.set_texture_mips(None)
    assert [r.texture_mips(i) for i in range(3)] == [(0, 0, 0, 0)] * 3
    r.set_texture_mips(good)
    assert L.lib.chordvis_set_texture_mips(r._ctx, (L.TextureMips * 1)(), 0) == L.OK
    assert r.texture_mips(0) == (0, 0, 0, 0)
    # nothing set: the stores are the host chains
    scene, cam = scenes.material_test_scene(160, 100)
    r.upload_scene(scene)
    r.upload_material_textures()
    for tid, (chain, mips) in enumerate(scene._tex_chains):
        t = scene.texture_images[tid]
        _check_levels(r, tid, M.split_chain(chain, t.shape[1], t.shape[0], mips), "texture %d" % tid)
    want = np.concatenate([c[3::4] for c, _ in scene._tex_chains[:2]])                  # the masked materials sample textures 0 and 1
    assert np.array_equal(r.read_alpha_plane(len(want)), want)
    # the setting survives both uploads, and a full chain supplied in full is left alone by it
    r.set_texture_mips([(FULL, M.SRGB | M.COVERAGE, 128)] * len(scene._tex_chains))
    r.upload_scene(scene)
    r.upload_material_textures()
    assert r.texture_mips(1) == (FULL, 3, 128, 0)
    for tid, (chain, mips) in enumerate(scene._tex_chains):
        t = scene.texture_images[tid]
        _check_levels(r, tid, M.split_chain(chain, t.shape[1], t.shape[0], mips), "texture %d" % tid)
    assert np.array_equal(r.read_alpha_plane(len(want)), want)
    r.close()


def test_generated_chain_past_the_texel_cap(gpu):
    """Thirteen 16384 x 16384 textures as level 0 alone stay below 4 G texels; their full chains do not.  Refused before any texel
    is read or stored (the thirteen descriptors share one host image of zero pages)."""
    n = 13
    assert n * 16384 * 16384 < 0xFFFFFFFF <= n * sum((16384 >> l) ** 2 for l in range(15))
    image = np.zeros(16384 * 16384 * 4, dtype=np.uint8)
    tex = R.TextureChain(image, 16384, 16384, 1)
    for masked in (False, True):
        scene = _texture_scene([tex] * n)
        if masked:
            scene.materials["alphaMode"] = R.ALPHA_MASK
        from chord_amd.renderer import VisibilityRenderer
        r = VisibilityRenderer(0)
        small = _texture_scene([np.full((4, 4, 4), 9, np.uint8)] * n)
        r.upload_scene(small)
        r.upload_material_textures()
        r.set_texture_mips([(FULL, 0, 0)] * n)
        if masked:
            with pytest.raises(L.ChordvisError, match="more than 4 G texels of alpha") as e:
                r.upload_scene(scene)
        else:
            r.scene = scene
            with pytest.raises(L.ChordvisError, match="upload_material_textures: more than 4 G texels") as e:
                r.upload_material_textures(scene)
            out = np.zeros(4 * 4 * 4, np.uint8)              # nothing kept, the earlier upload dropped
            assert L.lib.chordvis_readback_material_texture(r._ctx, 0, 0, out.ctypes.data) == L.E_INVALID
        assert "(-4)" in str(e.value)
        r.close()
