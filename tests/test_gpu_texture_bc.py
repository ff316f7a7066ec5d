"""Block-compressed textures (CHORD_TEXFMT_BC1_RGB / BC3 / BC4 / BC5) through the C ABI on the GPU: the expanded texels bit for bit
against tests/spec_texture_bc_np.py, the resolve images and the masked frames bit-equal to those of the decoded RGBA8 twin (and to
the oracle's), the alpha plane, the refusals, and RGBA8 uploads unchanged."""
import ctypes as C

import numpy as np
import pytest

from chord_amd import lib as L, records as R, scenes

import helpers as H
import spec_material_np as SM
import spec_texture_bc_np as BC

pytestmark = pytest.mark.gpu

FORMATS = [BC.BC1_RGB, BC.BC3, BC.BC4, BC.BC5]
SIZES = [(4, 4), (1, 1), (2, 2), (5, 3), (7, 9), (64, 64), (260, 4), (4, 260)]           # (width, height), full chains
NO_TEXTURE = 0xFFFFFFFF
SLOTS = ("baseColorId", "emissiveTexture", "normalTexture", "metallicRoughnessTexture")


def _texture_scene(textures, materials):
    """A small scene whose materials name `textures`: materials = [{slot name: texture id}], the slots not given name none."""
    base, cam = scenes.small_test_scene(64, 48, lods=1)
    mats = np.zeros(len(materials), dtype=R.MATERIAL)
    mats[:] = base.materials[0]
    mats["alphaMode"] = R.ALPHA_OPAQUE
    for k, named in enumerate(materials):
        for s in SLOTS:
            mats[s][k] = named.get(s, NO_TEXTURE)
    objs = base.objects.copy()
    objs["GLTFMaterialData"] = 0
    return R.Scene(objs, base.primitives, mats, base.meshlets, base.groups, base.group_indices, base.meshlet_data, base.positions,
                   textures=textures, bvh_nodes=base.bvh_nodes)


class _Textures:
    """`scene` under a texture table of its own: entries = {index: R.Texture} replace or extend the scene's."""

    def __init__(self, scene, entries):
        n = max(len(scene.texture_images), max(entries) + 1)
        self._keep = scene
        self._textures = (R.Texture * n)()
        for i in range(n):
            self._textures[i] = entries[i] if i in entries else scene._textures[i]
        d = scene.desc
        self.desc = R.SceneDesc(d.objects, d.objectCount, d.primitives, d.primitiveCount, d.materials, d.materialCount,
                                d.assets, d.assetCount, C.cast(self._textures, C.c_void_p), n, d.samplers, d.samplerCount)


def _random_chain(rng, w, h, format):
    mips = max(w, h).bit_length()
    return R.TextureChain(rng.integers(0, 256, size=BC.chain_bytes(w, h, mips, format), dtype=np.uint8), w, h, mips, format)


def _renderer(scene, materials=True):
    from chord_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(0)
    r.upload_scene(scene)
    if materials:
        r.upload_material_textures()
    return r


def _check_levels(r, tid, t, what):
    want = BC.decode_chain(t.data, t.width, t.height, t.mips, t.format)
    for l, lv in enumerate(want):
        got = r.readback_material_texture(tid, l)
        assert got.shape == lv.shape, (what, l)
        if not np.array_equal(got, lv):
            bad = np.argwhere((got != lv).any(axis=2))
            raise AssertionError("%s level %d (%d x %d): %d texels differ; first (y, x) = %s got %s want %s" % (
                what, l, lv.shape[1], lv.shape[0], len(bad), bad[0], got[tuple(bad[0])], lv[tuple(bad[0])]))


def _modes(t):
    """(blocks with first endpoint > second, blocks) per kind of block of a chain: {"colour": ..., "channel": ...}"""
    b = t.data.reshape(-1, BC.BLOCK_BYTES[t.format])
    out = {}
    if t.format in (BC.BC1_RGB, BC.BC3):
        c0, c1 = BC.colour_endpoints(b[:, -8:])
        out["colour"] = (int((c0 > c1).sum()), len(b))
    if t.format != BC.BC1_RGB:
        ch = b.reshape(-1, 8) if t.format == BC.BC5 else b[:, :8]
        out["channel"] = (int((ch[:, 0] > ch[:, 1]).sum()), len(ch))
    return out


@pytest.mark.parametrize("format", FORMATS, ids=["bc1", "bc3", "bc4", "bc5"])
def test_decode_equals_the_spec_on_random_blocks(gpu, format):
    """Every byte pattern is a valid block: random bytes reach the three-colour mode and both channel modes, which no encoder
    output here does."""
    rng = np.random.default_rng(1000 + format)
    textures = [_random_chain(rng, w, h, format) for w, h in SIZES]
    total = {}
    for t in textures:
        for kind, (first, n) in _modes(t).items():
            a, b = total.get(kind, (0, 0))
            total[kind] = (a + first, b + n)
    for kind, (first, n) in total.items():
        assert first * 4 >= n and (n - first) * 4 >= n, (kind, first, n)        # each mode: at least a quarter of the blocks
    scene = _texture_scene(textures, [{"baseColorId": i} for i in range(len(textures))])
    r = _renderer(scene)
    for i, t in enumerate(textures):
        _check_levels(r, i, t, "format %d %d x %d" % (format, t.width, t.height))
    r.close()


def test_mixed_scene(gpu):
    """RGBA8 and the four block formats in one upload, over all four material slots, plus a texture nothing names whose format is
    unknown and whose data is NULL: ignored by both uploads."""
    rng = np.random.default_rng(77)
    img = rng.integers(0, 256, size=(21, 37, 4), dtype=np.uint8)
    textures = [img, _random_chain(rng, 37, 21, BC.BC1_RGB), R.bc_chain(img, BC.BC3), _random_chain(rng, 6, 10, BC.BC4),
                _random_chain(rng, 64, 16, BC.BC5)]
    scene = _texture_scene(textures, [{"baseColorId": 0, "emissiveTexture": 1, "normalTexture": 2, "metallicRoughnessTexture": 3},
                                      {"baseColorId": 4}])
    odd = _Textures(scene, {5: R.Texture(None, 8, 8, 1, 999)})
    from chord_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(0)
    r.upload_scene(odd)
    r.scene = scene
    r.upload_material_textures(odd)
    chain, mips = R.mip_chain_rgba8(img)
    _check_levels(r, 0, R.TextureChain(chain, 37, 21, mips, BC.RGBA8), "rgba8")
    for i in range(1, 5):
        _check_levels(r, i, textures[i], "texture %d" % i)
    out = np.zeros(8 * 8 * 4, np.uint8)
    assert L.lib.chordvis_readback_material_texture(r._ctx, 5, 0, out.ctypes.data) == L.E_INVALID
    r.close()


def _resolve(r, names):
    import torch
    out = r.resolve_attributes(names=names)
    torch.cuda.synchronize()
    return {n: t.cpu().numpy().view(np.uint32) for n, t in out.items()}


def test_material_scene_equals_its_decoded_twin(gpu):
    """material_test_scene under BC3 base colour and emissive, BC5 normal and BC1 metallic-roughness textures: frames (its masked
    materials test the BC3 alpha) and all fifteen resolve images equal those of the spec-decoded RGBA8 twin, anisotropy 1 and 8."""
    scene, cam, view, iv = H.setup_scene(scenes.material_test_scene, 320, 200)
    bc = BC.bc_scene(scene, [BC.BC3, BC.BC3, BC.BC5, BC.BC1_RGB, BC.BC3])           # albedo, noise, normal, ORM, emissive
    twin = BC.decoded_twin(bc)
    names = list(L.RESOLVE_CHANNELS) + list(L.SURFACE_CHANNELS) + list(L.MATERIAL_CHANNELS)
    assert len(names) == 15
    rs = []
    for sc in (bc, twin):
        r = _renderer(sc)
        r.allocate_gbuffer(cam.width, cam.height)
        r.set_view(view, iv, H.ALL_FLAGS)
        r.render_frame()
        r.render_frame()
        rs.append(r)
    H.assert_vis_equal(rs[0].read_visibility(), rs[1].read_visibility(), cam.width, cam.height, "BC scene against its twin")
    for n in (1, 8):
        for r in rs:
            r.set_material_anisotropy(n)
        a, b = _resolve(rs[0], names), _resolve(rs[1], names)
        for k in names:
            assert np.array_equal(a[k], b[k]), (n, k, int((a[k] != b[k]).sum()))
        assert np.any(a["baseColor"]) and np.any(a["emissive"]) and np.any(a["pixelNormal"]) and np.any(a["roughMetalAO"])
    # the BC textures matter: the twin's base colour is not the uncompressed scene's
    r = _renderer(scene)
    r.allocate_gbuffer(cam.width, cam.height)
    r.set_view(view, iv, H.ALL_FLAGS)
    r.render_frame()
    r.render_frame()
    r.set_material_anisotropy(8)
    assert not np.array_equal(_resolve(r, ["baseColor"])["baseColor"], a["baseColor"])
    for x in rs + [r]:
        x.close()


def _two_frames(r, cam, view, iv):
    r.allocate_gbuffer(cam.width, cam.height)
    r.set_view(view, iv, H.ALL_FLAGS)
    out = []
    for _ in range(2):
        r.render_frame()
        out.append(r.read_visibility())
    return out


def test_masked_scene_under_bc3_base_colours(gpu):
    import orc
    bc3, bc1, cam, view, iv = BC.masked_scenes(320, 200)
    twin = BC.decoded_twin(bc3)
    w, h = cam.width, cam.height
    # the alpha plane: every level of the three textures (each sampled by a masked material), in texture order
    want_alpha = np.concatenate([BC.chain_rgba8(t.data, t.width, t.height, t.mips, t.format)[3::4] for t in bc3.texture_images])
    r = _renderer(bc3, materials=False)
    got_alpha = r.read_alpha_plane(len(want_alpha))
    assert np.array_equal(got_alpha, want_alpha), int((got_alpha != want_alpha).sum())
    got = _two_frames(r, cam, view, iv)
    want0 = orc.frame(twin, view, iv, H.ALL_FLAGS)
    want1 = orc.frame(twin, view, iv, H.ALL_FLAGS, prev_hzb_min=want0["hzb_min"])
    H.assert_vis_equal(got[0], want0["vis"], w, h, "BC3 frame 0 against the oracle on the twin")
    H.assert_vis_equal(got[1], want1["vis"], w, h, "BC3 frame 1 against the oracle on the twin")
    rt = _renderer(twin, materials=False)
    assert np.array_equal(rt.read_alpha_plane(len(want_alpha)), want_alpha)
    got_twin = _two_frames(rt, cam, view, iv)
    for k in range(2):
        H.assert_vis_equal(got[k], got_twin[k], w, h, "BC3 frame %d against the GPU's frame of the twin" % k)
    rt.close()
    # BC1_RGB base colours: alpha 255, as an RGBA8 scene whose alpha is 255 throughout
    src, _ = scenes.masked_test_scene(w, h)
    white = []
    for t in src.texture_images:
        t = t.copy()
        t[..., 3] = 255
        white.append(t)
    r1, rw = _renderer(bc1, materials=False), _renderer(scenes.with_textures(bc1, white), materials=False)
    assert (r1.read_alpha_plane(len(want_alpha)) == 255).all()
    f1, fw = _two_frames(r1, cam, view, iv), _two_frames(rw, cam, view, iv)
    for k in range(2):
        H.assert_vis_equal(f1[k], fw[k], w, h, "BC1 frame %d against the alpha-255 RGBA8 scene" % k)
    assert not np.array_equal(f1[1], got[1])
    r1.close(); rw.close()
    # a depth view of the BC3 scene: the child context shares the decoded alpha plane
    cfg = R.default_cascade_config(cascadeCount=3, realtimeCascadeCount=2, cascadeDim=256, cascadeEndDistance=14.0, farCascadeEndDistance=40.0)
    views = L.cascade_setup(cfg, view, iv, (0.35, -1.0, 0.25))
    r.allocate_depth_views(256, len(views))
    r.set_instance_views(views)
    lst = r.instance_culling_view(1)
    want_cmds = orc.instance_culling(twin, view, views[1:2], H.ALL_FLAGS)
    assert np.array_equal(r.read_cmds(lst), want_cmds)
    depth = r.read_depth(r.render_mesh_depth(1, lst, True, 0.0, 0.0))
    want_depth, st = orc.raster_depth(twin, views[1:2], want_cmds, 256, 256, True, 0.0, 0.0)
    assert st.fragmentsClipped > 0
    assert np.array_equal(depth.view(np.uint32), want_depth.view(np.uint32)), int((depth.view(np.uint32) != want_depth.view(np.uint32)).sum())
    r.close()


def test_refusals(gpu):
    from chord_amd.renderer import VisibilityRenderer
    scene, cam, view, iv = H.setup_scene(scenes.material_test_scene, 160, 100)
    bc = BC.bc_scene(scene, [BC.BC3, BC.BC3, BC.BC5, BC.BC1_RGB, BC.BC3])
    t0 = bc._textures[0]
    r = VisibilityRenderer(0)
    # upload_scene looks at the base colours of masked materials (textures 0 and 1 here), and at nothing else
    with pytest.raises(L.ChordvisError, match="unknown ChordTexture::format.*allowed: 0 .RGBA8., 1 .BC1_RGB., 2 .BC3., 3 .BC4., 4 .BC5."):
        r.upload_scene(_Textures(bc, {0: R.Texture(t0.rgba8, t0.width, t0.height, t0.mipCount, 5)}))
    t3 = bc._textures[3]
    unknown3 = _Textures(bc, {3: R.Texture(t3.rgba8, t3.width, t3.height, t3.mipCount, 0x80000001)})
    r.upload_scene(unknown3)                         # the ORM texture: no masked material samples it
    r.scene = bc
    r.allocate_gbuffer(cam.width, cam.height)
    r.set_view(view, iv, H.ALL_FLAGS)
    r.render_frame()
    with pytest.raises(L.ChordvisError, match="unknown ChordTexture::format.*allowed: 0 .RGBA8., 1 .BC1_RGB., 2 .BC3., 3 .BC4., 4 .BC5."):
        r.upload_material_textures(unknown3)         # ... but a material names it
    with pytest.raises(L.ChordvisError, match="no chordvis_upload_material_textures"):
        r.resolve_attributes(names=["baseColor"])
    r.upload_material_textures(bc)
    r.resolve_attributes(names=["baseColor"])
    with pytest.raises(L.ChordvisError, match="has no data"):
        r.upload_material_textures(_Textures(bc, {2: R.Texture(None, 64, 32, 7, BC.BC5)}))
    with pytest.raises(L.ChordvisError, match="no chordvis_upload_material_textures"):     # nothing kept, the earlier upload dropped
        r.resolve_attributes(names=["baseColor"])
    out = np.zeros(64 * 64 * 4, np.uint8)
    assert L.lib.chordvis_readback_material_texture(r._ctx, 0, 0, out.ctypes.data) == L.E_INVALID
    sixteen = _Textures(bc, {0: R.Texture(t0.rgba8, t0.width, t0.height, 16, BC.BC3)})        # (refused before any byte is read)
    with pytest.raises(L.ChordvisError, match="15 levels"):
        r.upload_material_textures(sixteen)
    with pytest.raises(L.ChordvisError, match="15 levels"):
        r.upload_scene(sixteen)
    r.close()
    # readback: an unnamed texture, a level out of range, a NULL pointer
    r = _renderer(_texture_scene([bc.texture_images[0], bc.texture_images[2]], [{"baseColorId": 0}]))
    assert r.readback_material_texture(0, 6).shape == (1, 1, 4)
    for tid, level in [(1, 0), (2, 0), (0, 7), (NO_TEXTURE, 0)]:
        assert L.lib.chordvis_readback_material_texture(r._ctx, tid, level, out.ctypes.data) == L.E_INVALID, (tid, level)
    assert L.lib.chordvis_readback_material_texture(r._ctx, 0, 0, None) == L.E_INVALID
    r.close()
    # the alpha plane of a scene without one
    r = _renderer(_texture_scene([bc.texture_images[0]], [{"baseColorId": 0}]), materials=False)
    assert L.lib.chordvis_debug_read(r._ctx, 7, 0, 1, out.ctypes.data) == L.E_INVALID
    r.close()


def test_rgba8_uploads_are_unchanged(gpu):
    """Formats all 0: the texel store, read through the new readback, is the host chain of every named texture."""
    scene, cam = scenes.material_test_scene(160, 100)
    r = _renderer(scene)
    for tid, (chain, mips) in enumerate(scene._tex_chains):
        t = scene.texture_images[tid]
        _check_levels(r, tid, R.TextureChain(chain, t.shape[1], t.shape[0], mips, BC.RGBA8), "texture %d" % tid)
    want = np.concatenate([c[3::4] for c, _ in scene._tex_chains[:2]])                  # the masked materials sample textures 0 and 1
    assert np.array_equal(r.read_alpha_plane(len(want)), want)
    r.close()
