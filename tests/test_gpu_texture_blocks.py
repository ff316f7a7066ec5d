"""chordvis_set_material_texture_store(CHORD_TEXSTORE_BLOCKS) through the C ABI on the GPU: block-compressed chains kept as blocks and
decoded by the material resolve's sampler.  Every level read back equals tests/spec_texture_bc_np.py's decode; the resolve images equal
those of mode EXPANDED and the numpy specs on the decoded RGBA8 twin, word for word (uint32 views; no tolerance anywhere); the memory
figures, the setting's life cycle, mixed uploads, and the existing kernels for stores that hold no kept chain."""
import numpy as np
import pytest

from chord_amd import lib as L, records as R, scenes

import helpers as H
import spec_material_aniso_np as SA
import spec_material_np as SM
import spec_resolve_np as SR
import spec_texture_bc_np as BC
import spec_texture_mips_np as M

pytestmark = pytest.mark.gpu

FORMATS = [BC.BC1_RGB, BC.BC3, BC.BC4, BC.BC5]
SIZES = [(4, 4), (1, 1), (2, 2), (5, 3), (7, 9), (64, 64), (260, 4), (4, 260)]           # (width, height), full chains
NO_TEXTURE = 0xFFFFFFFF
NAMES = list(L.RESOLVE_CHANNELS) + list(L.SURFACE_CHANNELS) + list(L.MATERIAL_CHANNELS)
MATERIAL_FORMATS = [BC.BC3, BC.BC3, BC.BC5, BC.BC1_RGB, BC.BC3]                          # albedo, noise, normal, ORM, emissive


def _random_chain(rng, w, h, format):
    mips = max(w, h).bit_length()
    return R.TextureChain(rng.integers(0, 256, size=BC.chain_bytes(w, h, mips, format), dtype=np.uint8), w, h, mips, format)


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


def _renderer(scene, store, mips=None):
    from chord_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(0)
    r.set_material_texture_store(store)                # (before the uploads: the setting survives them)
    if mips:
        r.set_texture_mips(mips)
    r.upload_scene(scene)
    r.upload_material_textures()
    return r


def _frames(r, cam, view, iv, count=2):
    r.allocate_gbuffer(cam.width, cam.height)
    r.set_view(view, iv, H.ALL_FLAGS)
    out = []
    for _ in range(count):
        r.render_frame()
        out.append(r.read_visibility())
    return out


def _resolve(r, names=NAMES):
    import torch
    out = r.resolve_attributes(names=list(names))
    torch.cuda.synchronize()
    return {n: t.cpu().numpy().view(np.uint32) for n, t in out.items()}


def _assert_images(got, want, what, names=NAMES):
    for n in names:
        w = np.ascontiguousarray(want[n]).view(np.uint32).reshape(got[n].shape)
        if not np.array_equal(got[n], w):
            bad = np.argwhere(got[n] != w)
            raise AssertionError("%s %s: %d words differ; first %s got %#010x want %#010x" % (what, n, len(bad), bad[0], got[n][tuple(bad[0])], w[tuple(bad[0])]))


def _spec(scene, r, view, iv, n):
    """the four material images of the numpy spec on the frame r holds (scene: RGBA8 textures only)"""
    vis, cmds = r.read_visibility(), r.read_cmds(r.last_frame_cmds())
    if n == 1:
        return SM.resolve(scene, vis, cmds, view, iv, r.width, r.height)
    return SA.resolve(scene, vis, cmds, view, iv, r.width, r.height, max_aniso=n)


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


def _block_bytes(textures):
    return sum((L.texture_chain_bytes(t.format, t.width, t.height, t.mips) + 15) // 16 * 16 for t in textures)


def _texel_bytes(dims):
    """4 x the texels of full-or-partial chains: dims = [(width, height, levels)]"""
    return 4 * sum(w * h for width, height, levels in dims for w, h in BC.level_dims(width, height, levels))


# ---- store and readback ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("format", FORMATS, ids=["bc1", "bc3", "bc4", "bc5"])
def test_kept_chains_read_back_as_the_spec_decodes_them(gpu, format):
    """Random block bytes reach the three-colour mode and both channel modes; every level of every kept chain, expanded by the
    readback, equals the spec; nothing is in the texel store."""
    rng = np.random.default_rng(2000 + format)
    textures = [_random_chain(rng, w, h, format) for w, h in SIZES]
    b = np.concatenate([t.data for t in textures]).reshape(-1, 8)
    if format in (BC.BC1_RGB, BC.BC3):
        c0, c1 = BC.colour_endpoints(b if format == BC.BC1_RGB else b[1::2])
        assert (c0 > c1).any() and (c0 <= c1).any()
    if format != BC.BC1_RGB:
        ch = b if format != BC.BC3 else b[0::2]
        assert (ch[:, 0] > ch[:, 1]).any() and (ch[:, 0] <= ch[:, 1]).any()
    r = _renderer(_texture_scene(textures), L.TEXSTORE_BLOCKS)
    assert r.material_texture_store() == L.TEXSTORE_BLOCKS
    for i, t in enumerate(textures):
        _check_levels(r, i, BC.decode_chain(t.data, t.width, t.height, t.mips, t.format), "format %d %d x %d" % (format, t.width, t.height))
    assert r.material_texture_memory() == (0, _block_bytes(textures))
    r.close()


# ---- the material scene ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def material_scene():
    scene, cam, view, iv = H.setup_scene(scenes.material_test_scene, 320, 200)
    bc = BC.bc_scene(scene, MATERIAL_FORMATS)
    return bc, BC.decoded_twin(bc), cam, view, iv


def test_material_scene_equals_mode_expanded_and_the_spec(gpu, material_scene):
    bc, twin, cam, view, iv = material_scene
    rb, re = _renderer(bc, L.TEXSTORE_BLOCKS), _renderer(bc, L.TEXSTORE_EXPANDED)
    fb, fe = _frames(rb, cam, view, iv), _frames(re, cam, view, iv)
    for k in range(2):                                                     # the alpha store is untouched by the setting
        H.assert_vis_equal(fb[k], fe[k], cam.width, cam.height, "frame %d, mode BLOCKS against mode EXPANDED" % k)
    chains = bc.texture_images
    assert rb.material_texture_memory() == (0, _block_bytes(chains))
    assert re.material_texture_memory() == (_texel_bytes([(t.width, t.height, t.mips) for t in chains]), 0)
    for n in (1, 8):
        rb.set_material_anisotropy(n)
        re.set_material_anisotropy(n)
        a, b = _resolve(rb), _resolve(re)
        assert len(a) == 15
        _assert_images(a, b, "anisotropy %d, mode BLOCKS against mode EXPANDED" % n)
        _assert_images(a, _spec(twin, rb, view, iv, n), "anisotropy %d, mode BLOCKS against the spec on the decoded twin" % n, SM.NAMES)
        for k in SM.NAMES:
            assert np.any(a[k]), (n, k)
    rb.close(); re.close()


# ---- block seams ----------------------------------------------------------------------------------------------------------------

SEAM_SIZES = [(5, 3), (7, 9), (37, 21), (260, 4)]
SEAM_WRAPS = [SM.REPEAT, SM.MIRRORED_REPEAT, SM.CLAMP_TO_EDGE]
SEAM_FILTERS = [(SM.NEAREST, SM.NEAREST), (SM.LINEAR, SM.LINEAR), (SM.LINEAR_MIPMAP_LINEAR, SM.LINEAR)]      # (minFilter, magFilter)
EVENTS = ("two blocks in x", "two blocks in y", "four blocks", "wrap from the last partial block to the first", "a tap on a 1 x 1 level",
          "a two-level blend")


def _seam_scene(width=320, height=200):
    """36 quads in a 6 x 6 grid in front of the camera, one per (size, wrap, filter): the quad's material samples the four
    random-block full chains of that size, one per format, in its four slots (which format sits in which slot rotates from quad to
    quad), all through the one sampler.  Texture coordinates run over several periods on both sides of 0; the quads of the
    mip-mapped sampler lean away from the camera, so their level of detail varies over the quad."""
    rng = np.random.default_rng(99)
    sb = scenes.SceneBuilder("block_seams", True)
    chains = []
    for f in FORMATS:
        for w, h in SEAM_SIZES:
            sb.add_texture(np.zeros((h, w, 4), np.uint8))                 # (replaced by the chain below)
            chains.append(_random_chain(rng, w, h, f))
    cell_w, cell_h = 12.6 / 6.0, 7.8 / 6.0
    px_w, px_h = width / 6.0, height / 6.0
    q = 0
    for si, (w, h) in enumerate(SEAM_SIZES):
        for wi, wrap in enumerate(SEAM_WRAPS):
            for fi, (min_f, mag_f) in enumerate(SEAM_FILTERS):
                smp = sb.add_sampler(min_f, mag_f, wrap, wrap)
                tex = [((k + q) % 4) * len(SEAM_SIZES) + si for k in range(4)]           # slot k: format (k + q) % 4 at this size
                mat = sb.add_material(1, 0, tex[0], smp, pbr=True, emissive=(tex[1], smp), normal=(tex[2], smp),
                                      metallic_roughness=(tex[3], smp), occlusion_strength=1.0)
                rate = 2.5 if fi == 2 else 0.4                                           # texels per pixel at the quad's near edge
                span = (max(rate * px_w / w, 1.5), max(rate * px_h / h, 1.5))
                pb = scenes.PrimitiveBuilder(True)
                pb.uv_scale = span
                x0, y0 = -6.3 + (q % 6) * cell_w, -3.9 + (q // 6) * cell_h
                lean = 2.5 if fi == 2 else 0.0
                pb.add_surface(scenes.plane_surface((x0, y0, 0.0), (0.97 * cell_w, 0.0, 0.0), (0.0, 0.97 * cell_h, -lean)), 1, 1, 1)
                for t in pb.texcoords:
                    t -= np.array([0.6 * span[0] + 0.13, 0.55 * span[1] + 0.29], dtype=np.float32)
                sb.add_object(sb.add_primitive(pb), material=mat)
                q += 1
    scene = scenes.with_textures(sb.build(), chains)
    cam = scenes.Camera((0.0, 0.0, 10.0), (0.0, 0.0, -1.0), width, height)
    L.fill_objects(scene, cam)
    view, iv = L.make_views(cam)
    return scene, cam, view, iv


def _seam_events(scene, twin, vis, cmds, view, iv, w, h):
    """{format: {event: pixels}} from the spec's side: the uv image, the sampler statistics and the level sizes"""
    stats = {}
    SM.resolve(twin, vis, cmds, view, iv, w, h, stats=stats)
    uv = SR.resolve(twin, vis, cmds, view, iv, w, h, names=("uv",))["uv"].reshape(-1, 2)
    lin = lambda f: f in (SM.LINEAR, SM.LINEAR_MIPMAP_NEAREST, SM.LINEAR_MIPMAP_LINEAR)
    out = {f: dict.fromkeys(EVENTS, 0) for f in FORMATS}
    for slot in SM.SLOTS:
        for st in stats["slots"][slot]:
            levels, (min_f, mag_f, wrap_s, wrap_t) = SM.slot_texture(twin, twin.materials[st["material"]], slot)
            t = scene.texture_images[int(scene.materials[st["material"]][SM._TEX_FIELD[slot][0]])]
            assert levels[0].shape == (t.height, t.width)
            ev = out[t.format]
            u, v = uv[st["pix"], 0], uv[st["pix"], 1]
            linear = np.where(st["lodq"] > 0, lin(min_f), lin(mag_f))
            ev[EVENTS[5]] += int((st["l1"] != st["l0"]).sum())
            for lv, use in ((st["l0"], np.ones(len(u), bool)), (st["l1"], st["l1"] != st["l0"])):
                for l in np.unique(lv[use]):
                    k = np.nonzero(use & (lv == l))[0]
                    W, Hh = max(1, t.width >> l), max(1, t.height >> l)
                    if W == 1 and Hh == 1:
                        ev[EVENTS[4]] += len(k)
                    k = k[linear[k]]
                    if not len(k):
                        continue
                    x0, _ = SM.texel_floor(u[k] * np.float32(W) - np.float32(0.5))
                    y0, _ = SM.texel_floor(v[k] * np.float32(Hh) - np.float32(0.5))
                    ix0, ix1 = SM.wrap(x0, W, wrap_s), SM.wrap(x0 + 1, W, wrap_s)
                    iy0, iy1 = SM.wrap(y0, Hh, wrap_t), SM.wrap(y0 + 1, Hh, wrap_t)
                    dx, dy = (ix0 >> 2) != (ix1 >> 2), (iy0 >> 2) != (iy1 >> 2)
                    ev[EVENTS[0]] += int((dx & ~dy).sum())
                    ev[EVENTS[1]] += int((dy & ~dx).sum())
                    ev[EVENTS[2]] += int((dx & dy).sum())
                    seam_x = (ix0 == W - 1) & (ix1 == 0) & (W % 4 != 0) & (W > 4)
                    seam_y = (iy0 == Hh - 1) & (iy1 == 0) & (Hh % 4 != 0) & (Hh > 4)
                    ev[EVENTS[3]] += int((seam_x | seam_y).sum())
    return out


def test_block_seams(gpu):
    import orc
    scene, cam, view, iv = _seam_scene()
    twin = BC.decoded_twin(scene)
    w, h = cam.width, cam.height
    uvs = scene.texcoord0
    assert uvs.min() < -2.0 and uvs.max() > 2.0                            # well outside [0, 1], negative included
    # on the CPU, before the GPU is involved: the oracle's frame of this view reaches every event in every format
    frame = orc.frame(twin, view, iv, H.ALL_FLAGS)
    events = _seam_events(scene, twin, frame["vis"], frame["cmds"], view, iv, w, h)
    for f in FORMATS:
        for e in EVENTS:
            assert events[f][e] > 0, (f, e, events[f])
    r = _renderer(scene, L.TEXSTORE_BLOCKS)
    _frames(r, cam, view, iv, 1)
    assert r.material_texture_memory() == (0, _block_bytes(scene.texture_images))
    for n in (1, 8):
        r.set_material_anisotropy(n)
        got = _resolve(r, SM.NAMES)
        _assert_images(got, _spec(twin, r, view, iv, n), "anisotropy %d against the spec on the decoded twin" % n, SM.NAMES)
        assert np.any(got["baseColor"]) and np.any(got["roughMetalAO"])
    r.close()


# ---- mixed upload ---------------------------------------------------------------------------------------------------------------

def test_mixed_upload(gpu, material_scene):
    """One upload holds an RGBA8 texture (albedo), three kept chains (BC3 noise, BC5 normal, BC1 ORM) and a BC3 texture that gets made
    levels (emissive: level 0 supplied, the rest made under SRGB | COVERAGE), which is therefore expanded whole."""
    bc, _, cam, view, iv = material_scene
    src, _ = scenes.material_test_scene(320, 200)
    albedo, emis = src.texture_images[0], src.texture_images[4]
    emis0 = R.TextureChain(R.encode_bc(emis, BC.BC3), emis.shape[1], emis.shape[0], 1, BC.BC3)
    kept = list(bc.texture_images[1:4])
    scene = scenes.with_textures(bc, [albedo] + kept + [emis0])
    mips = [(0, 0, 0)] * 4 + [(L.TEXMIPS_FULL, M.SRGB | M.COVERAGE, 128)]
    rb, re = _renderer(scene, L.TEXSTORE_BLOCKS, mips), _renderer(scene, L.TEXSTORE_EXPANDED, mips)
    want = M.build_chain(BC.decode_chain(emis0.data, emis0.width, emis0.height, 1, BC.BC3), M.FULL, M.SRGB | M.COVERAGE, 128)
    assert len(want) == 5
    _check_levels(rb, 4, want, "the BC3 texture with made levels")
    for tid, t in enumerate(kept, 1):
        _check_levels(rb, tid, BC.decode_chain(t.data, t.width, t.height, t.mips, t.format), "kept chain %d" % tid)
    chain, levels = R.mip_chain_rgba8(albedo)
    _check_levels(rb, 0, M.split_chain(chain, albedo.shape[1], albedo.shape[0], levels), "the RGBA8 texture")
    expanded = [(albedo.shape[1], albedo.shape[0], levels), (emis0.width, emis0.height, 5)]
    assert rb.material_texture_memory() == (_texel_bytes(expanded), _block_bytes(kept))
    assert re.material_texture_memory() == (_texel_bytes(expanded + [(t.width, t.height, t.mips) for t in kept]), 0)
    fb, fe = _frames(rb, cam, view, iv), _frames(re, cam, view, iv)
    H.assert_vis_equal(fb[1], fe[1], cam.width, cam.height, "mixed upload, mode BLOCKS against mode EXPANDED")
    for n in (1, 8):
        rb.set_material_anisotropy(n)
        re.set_material_anisotropy(n)
        a = _resolve(rb)
        _assert_images(a, _resolve(re), "mixed upload, anisotropy %d" % n)
        assert np.any(a["emissive"]) and np.any(a["pixelNormal"])
    rb.close(); re.close()


# ---- the setting ----------------------------------------------------------------------------------------------------------------

def test_setting(gpu, material_scene):
    from chord_amd.renderer import VisibilityRenderer
    bc = material_scene[0]
    chains = bc.texture_images
    rgba8 = _texel_bytes([(t.width, t.height, t.mips) for t in chains])
    r = VisibilityRenderer(0)
    assert r.material_texture_store() == L.TEXSTORE_EXPANDED == 0
    t, b = L.C.c_uint64(7), L.C.c_uint64(7)
    assert L.lib.chordvis_material_texture_memory(r._ctx, L.C.byref(t), L.C.byref(b)) == L.E_INVALID      # nothing uploaded
    r.set_material_texture_store(L.TEXSTORE_BLOCKS)
    for bad in (2, 3, 0xFFFFFFFF):
        with pytest.raises(L.ChordvisError, match=r"0 \(CHORD_TEXSTORE_EXPANDED\) or 1 \(CHORD_TEXSTORE_BLOCKS\)"):
            r.set_material_texture_store(bad)
        assert r.material_texture_store() == L.TEXSTORE_BLOCKS, "the getter returns the last accepted value"
    r.set_material_texture_store(L.TEXSTORE_EXPANDED)
    r.upload_scene(bc)
    assert L.lib.chordvis_material_texture_memory(r._ctx, L.C.byref(t), L.C.byref(b)) == L.E_INVALID
    r.upload_material_textures()
    assert r.material_texture_memory() == (rgba8, 0)
    r.set_material_texture_store(L.TEXSTORE_BLOCKS)                        # read by later uploads only
    assert r.material_texture_memory() == (rgba8, 0)
    assert L.lib.chordvis_material_texture_memory(r._ctx, None, None) == L.OK
    assert L.lib.chordvis_material_texture_memory(r._ctx, None, L.C.byref(b)) == L.OK and b.value == 0
    r.upload_material_textures()
    assert r.material_texture_memory() == (0, _block_bytes(chains))
    r.upload_scene(bc)                                                     # kept across the scene upload, which drops the store
    assert r.material_texture_store() == L.TEXSTORE_BLOCKS
    r.upload_material_textures()
    assert r.material_texture_memory() == (0, _block_bytes(chains))
    r.set_material_texture_store(L.TEXSTORE_EXPANDED)
    assert r.material_texture_memory() == (0, _block_bytes(chains))
    r.upload_material_textures()
    assert r.material_texture_memory() == (rgba8, 0)
    r.close()


# ---- the scope of the fallback --------------------------------------------------------------------------------------------------

def test_rgba8_textures_alone_take_the_existing_kernels(gpu):
    """Every texture RGBA8 in mode BLOCKS: nothing is kept as blocks, and the images are mode EXPANDED's."""
    scene, cam, view, iv = H.setup_scene(scenes.material_test_scene, 320, 200)
    rb, re = _renderer(scene, L.TEXSTORE_BLOCKS), _renderer(scene, L.TEXSTORE_EXPANDED)
    assert rb.material_texture_memory() == re.material_texture_memory()
    assert rb.material_texture_memory()[1] == 0 and rb.material_texture_memory()[0] == 4 * sum(len(c) // 4 for c, _ in scene._tex_chains)
    _frames(rb, cam, view, iv)
    _frames(re, cam, view, iv)
    for n in (1, 8):
        rb.set_material_anisotropy(n)
        re.set_material_anisotropy(n)
        _assert_images(_resolve(rb), _resolve(re), "RGBA8 textures alone, anisotropy %d" % n)
    rb.close(); re.close()
