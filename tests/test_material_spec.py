"""The pinned sampler and material arithmetic of chordvis_resolve_material on the CPU: the level of detail
against log2, the spec's sampler against an independent float64 restatement, exact known answers, the constant tables, the
tangent frame under stretched and mirrored transforms, and the conditions that keep the GPU comparison from passing on trivial
inputs.  No GPU."""
import json
import math
import os

import numpy as np
import pytest

from chord_amd import scenes

import helpers as H
import spec_material_np as SM
import spec_surface_np as SS

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = (SM.NEAREST, SM.LINEAR, SM.NEAREST_MIPMAP_NEAREST, SM.LINEAR_MIPMAP_NEAREST, SM.NEAREST_MIPMAP_LINEAR, SM.LINEAR_MIPMAP_LINEAR)
WRAPS = (SM.REPEAT, SM.CLAMP_TO_EDGE, SM.MIRRORED_REPEAT)


# ---- 1. level of detail ----------------------------------------------------------------------------------------------------

def test_lodq_is_half_log2_within_the_derived_bound():
    """|lodq / 256 - log2(rho2) / 2| <= 0.0431 + 3 / 512: the chord error of log2 on [1, 2) (0.0861) halved, plus the mantissa's
    truncation to 8 bits halved and the shift's own."""
    octave = np.linspace(1.0, 2.0, 4097)[:-1]
    rho2 = np.concatenate([octave * 2.0 ** e for e in range(-20, 21)]).astype(f32)
    q = SM.lodq_of(rho2).astype(np.float64) / 256.0
    err = np.abs(q - 0.5 * np.log2(rho2.astype(np.float64)))
    assert err.max() <= 0.0431 + 3.0 / 512.0, err.max()
    assert np.all(np.diff(SM.lodq_of(np.sort(rho2))) >= 0), "monotonic"
    odd = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -1.0], dtype=f32)
    assert np.all(SM.lodq_of(odd) == 0)
    assert SM.lodq_of(np.array([1.0], dtype=f32))[0] == 0 and SM.lodq_of(np.array([4.0], dtype=f32))[0] == 256
    assert SM.lodq_of(np.array([0.25], dtype=f32))[0] == -256


# ---- 2. the sampler against a float64 restatement ------------------------------------------------------------------------------

def _texture(w, h, seed):
    img = (scenes.pcg_hash(np.arange(w * h * 4, dtype=np.uint32) + np.uint32(seed)) & 0xFF).astype(np.uint8).reshape(h, w, 4)
    from chord_amd import records as R
    chain, mips = R.mip_chain_rgba8(img)
    return SM.levels_of(chain, w, h, mips), chain, mips


def _wrap64(i, n, mode):
    if mode == SM.CLAMP_TO_EDGE:
        return min(max(i, 0), n - 1)
    if mode == SM.MIRRORED_REPEAT:
        m = i % (2 * n)
        return m if m < n else 2 * n - 1 - m
    return i % n


def _ref_sample(chain, w, h, mips, sampler, u, v, g, table):
    """one pixel, float64, own loops: the pin restated from DESIGN.md"""
    min_f, mag_f, ws, wt = sampler
    lin = lambda f: f in (SM.LINEAR, SM.LINEAR_MIPMAP_NEAREST, SM.LINEAR_MIPMAP_LINEAR)
    lodq = int(SM.lodq_of(SM.footprint(np.array([g], dtype=f32), w, h))[0])       # (the level choice is integer work: shared)
    levels, linear, frac = [0], lin(mag_f), 0.0
    if lodq > 0:
        linear = lin(min_f)
        if min_f in (SM.NEAREST_MIPMAP_NEAREST, SM.LINEAR_MIPMAP_NEAREST):
            levels = [min((lodq + 128) >> 8, mips - 1)]
        elif min_f in (SM.NEAREST_MIPMAP_LINEAR, SM.LINEAR_MIPMAP_LINEAR):
            l0 = min(lodq >> 8, mips - 1)
            levels, frac = [l0, min(l0 + 1, mips - 1)], (lodq & 255) / 256.0
    offs, o = [], 0
    for l in range(mips):
        offs.append(o)
        o += max(1, w >> l) * max(1, h >> l)

    def texel(l, ix, iy):
        lw, lh = max(1, w >> l), max(1, h >> l)
        p = (offs[l] + _wrap64(iy, lh, wt) * lw + _wrap64(ix, lw, ws)) * 4
        b = chain[p:p + 4]
        k = float(f32(1.0 / 255.0))                     # (the decode is pinned as byte * (1 / 255) with the float32 constant)
        return np.array([table[b[0]], table[b[1]], table[b[2]], b[3] * k] if table is not None else [x * k for x in b], dtype=np.float64)

    def level(l):
        lw, lh = max(1, w >> l), max(1, h >> l)
        if not linear:
            return texel(l, math.floor(float(f32(u) * f32(lw))), math.floor(float(f32(v) * f32(lh))))
        # (the texel coordinate is part of the pin: u * fW - 0.5 in float32 decides the texel pair; its fraction is exact)
        x, y = float(f32(u) * f32(lw) - f32(0.5)), float(f32(v) * f32(lh) - f32(0.5))
        x0, y0 = math.floor(x), math.floor(y)
        fx, fy = x - x0, y - y0
        top = texel(l, x0, y0) * (1 - fx) + texel(l, x0 + 1, y0) * fx
        bot = texel(l, x0, y0 + 1) * (1 - fx) + texel(l, x0 + 1, y0 + 1) * fx
        return top * (1 - fy) + bot * fy
    c = level(levels[0])
    if len(levels) == 2 and levels[1] != levels[0]:
        c = c * (1 - frac) + level(levels[1]) * frac
    return c


@pytest.mark.parametrize("size", [(37, 21), (64, 64), (8, 64), (5, 1)], ids=lambda s: "%dx%d" % s)
def test_sampler_against_a_float64_restatement(size):
    w, h = size
    levels, chain, mips = _texture(w, h, 1234 + w)
    table, _ = SM.tables()
    n = 160
    rnd = lambda k: scenes.rand01(77 + w, np.arange(k * n, (k + 1) * n))
    u, v = (rnd(0) * 6.0 - 3.0).astype(f32), (rnd(1) * 6.0 - 3.0).astype(f32)
    # footprints from strong magnification to beyond the last level
    mag = (2.0 ** (rnd(2) * (mips + 3.0) - 2.0)) / max(w, h)
    g = np.stack([mag, mag * (rnd(3) - 0.5), mag * (rnd(4) - 0.5), mag * rnd(5)], axis=-1).astype(f32)
    reached_last = False
    for min_f in FILTERS:
        for mag_f in (SM.NEAREST, SM.LINEAR):
            for ws in WRAPS:
                wt = WRAPS[(WRAPS.index(ws) + 1 + FILTERS.index(min_f)) % 3]
                for tb in (None, table):
                    st = {}
                    got = SM.sample(levels, (min_f, mag_f, ws, wt), u, v, g, tb, st)
                    reached_last |= bool(np.any((st["l0"] == mips - 1) & (st["lodq"] > 0)))
                    for i in range(0, n, 4 if tb is None else 16):
                        want = _ref_sample(chain, w, h, mips, (min_f, mag_f, ws, wt), u[i], v[i], g[i], tb)
                        lin_i = min_f in (SM.LINEAR, SM.LINEAR_MIPMAP_NEAREST, SM.LINEAR_MIPMAP_LINEAR) if st["lodq"][i] > 0 else mag_f == SM.LINEAR
                        if not lin_i and st["l0"][i] == st["l1"][i]:
                            assert np.array_equal(got[i], want.astype(f32)), (min_f, mag_f, ws, wt, i)       # NEAREST: exact
                        else:
                            # values are in [0, 1]; float32 has 2^-24 per operation and a tap is < 16 operations
                            assert np.max(np.abs(got[i].astype(np.float64) - want)) <= 2.0 ** -20, (min_f, mag_f, ws, wt, i, got[i], want)
    assert reached_last


# ---- 3. exact known answers -------------------------------------------------------------------------------------------------

def test_a_constant_texture_returns_its_decoded_constant():
    from chord_amd import records as R
    table, _ = SM.tables()
    img = np.zeros((12, 20, 4), np.uint8)
    img[...] = (200, 17, 255, 90)
    chain, mips = R.mip_chain_rgba8(img)
    levels = SM.levels_of(chain, 20, 12, mips)
    n = 64
    u = (scenes.rand01(5, np.arange(n)) * 8 - 4).astype(f32)
    v = (scenes.rand01(6, np.arange(n)) * 8 - 4).astype(f32)
    g = (np.outer(2.0 ** np.linspace(-12, 6, n), [1.0, 0.3, -0.2, 0.9])).astype(f32)
    for min_f in FILTERS:
        for ws in WRAPS:
            lin = SM.sample(levels, (min_f, SM.LINEAR, ws, ws), u, v, g, None)
            assert np.array_equal(lin, np.tile((np.array([200, 17, 255, 90], dtype=f32) * f32(1.0 / 255.0)), (n, 1))), (min_f, ws)
            srgb = SM.sample(levels, (min_f, SM.NEAREST, ws, ws), u, v, g, table)
            assert np.array_equal(srgb, np.tile(np.array([table[200], table[17], table[255], f32(90) * f32(1.0 / 255.0)], dtype=f32), (n, 1)))


def _frame(builder, *a, **kw):
    import orc
    scene, cam, view, iv = H.setup_scene(builder, *a, **kw)
    fr = orc.frame(scene, view, iv, H.ALL_FLAGS)
    return scene, cam, view, iv, fr


def test_known_answers_of_the_material_arithmetic(built_lib):
    scene, cam, view, iv, fr = _frame(scenes.material_test_scene, 160, 100)
    w, h = cam.width, cam.height
    # normalFactorScale = 0 on every material: n = (0, 0, 1) exactly wherever z > 0, so pixelNormal is vertexNormal bit for bit
    mats = scene.materials.copy()
    mats["normalFactorScale"] = 0.0
    flat = scene.with_objects(materials=mats)
    st = {}
    got = SM.resolve(flat, fr["vis"], fr["cmds"], view, iv, w, h, stats=st)
    S = SS.resolve(flat, fr["vis"], fr["cmds"], view, iv, w, h)
    pbr = st["pbr"].reshape(h, w)
    # (z > 0: the maps of _pbr_textures hold unit normals, whose filtered xy stay inside the unit disc)
    assert np.array_equal(got["pixelNormal"][pbr].view(np.uint32), S["vertexNormal"][pbr].view(np.uint32))
    assert pbr.sum() > 0.5 * w * h
    # a material without metallic-roughness texture returns its factors; metallicFactor = 1 -> 0
    mat = st["material"].reshape(h, w)
    got = SM.resolve(scene, fr["vis"], fr["cmds"], view, iv, w, h)
    seen = 0
    for m in np.unique(mat[mat >= 0]):
        M = scene.materials[m]
        if int(M["materialType"]) != 1:
            assert not np.any(got["baseColor"][mat == m]) and not np.any(got["pixelNormal"][mat == m])
            assert not np.any(got["emissive"][mat == m]) and not np.any(got["roughMetalAO"][mat == m])
            seen |= 4
        elif int(M["metallicRoughnessTexture"]) >= len(scene.texture_images):
            mf = f32(M["metallicFactor"])
            want = np.array([M["roughnessFactor"], 0.0 if mf >= 1.0 else mf, 1.0, 0.0], dtype=f32)
            assert np.all(got["roughMetalAO"][mat == m] == want), m
            seen |= 2 if mf >= 1.0 else 1
    assert seen == 7, "a material with metallicFactor 1, one below 1 and one of another shading type are on screen"
    assert not np.any(got["baseColor"][mat < 0])


# ---- 4. the tables ----------------------------------------------------------------------------------------------------------

def test_tables_library_equals_fixture_equals_formula(built_lib):
    srgb, ap1 = SM.tables()
    lib_srgb, lib_ap1 = built_lib.material_constants()
    assert np.array_equal(lib_srgb.view(np.uint32), srgb.view(np.uint32)) and np.array_equal(lib_ap1.view(np.uint32), ap1.view(np.uint32))
    c = np.arange(256, dtype=np.float64) / 255.0
    want = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4).astype(f32)
    assert np.array_equal(srgb.view(np.uint32), want.view(np.uint32))
    # sRGB_2_AP1 = mul(XYZ_2_AP1, mul(D65_2_D60_CAT, sRGB_2_XYZ)) (colorspace.h:9-14,49-54,79-84,109) in float64, rounded once
    s2x = np.array([[0.4123907993, 0.3575843394, 0.1804807884], [0.2126390059, 0.7151686788, 0.0721923154], [0.0193308187, 0.1191947798, 0.9505321522]])
    cat = np.array([[1.0130349146, 0.0061052578, -0.0149709436], [0.0076982301, 0.9981633521, -0.0050320385], [-0.0028413174, 0.0046851567, 0.9245061375]])
    x2a = np.array([[1.6410233797, -0.3248032942, -0.2364246952], [-0.6636628587, 1.6153315917, 0.0167563477], [0.0117218943, -0.0082844420, 0.9883948585]])
    mul = lambda a, b: np.array([[(a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j] for j in range(3)] for i in range(3)])
    assert np.array_equal(ap1.view(np.uint32), mul(x2a, mul(cat, s2x)).astype(f32).view(np.uint32))
    assert abs(float(ap1.sum(axis=1).mean()) - 1.0) < 1e-3, "white stays (nearly) white"
    with open(os.path.join(ROOT, "tests", "golden", "material_tables.json")) as f:
        assert sorted(json.load(f)) == ["srgb_to_ap1_bits", "srgb_to_linear_bits"]


# ---- 5. geometry: the pixel normal in the face's tangent frame ---------------------------------------------------------------

def _flat_scene(l2w):
    """one flat square (normal +z, tangent +x, texture coordinates (x, 1 - y) tiled 2 x) under l2w, with the relief map"""
    n = 9
    g = np.linspace(-1.0, 1.0, n)
    X, Y = np.meshgrid(g, g)
    pos = np.stack([X.reshape(-1), Y.reshape(-1), np.zeros(n * n)], -1).astype(f32)
    uv = np.stack([(X.reshape(-1) + 1.0), (1.0 - Y.reshape(-1))], -1).astype(f32)
    idx = []
    for j in range(n - 1):
        for i in range(n - 1):
            a = j * n + i
            idx += [a, a + 1, a + n + 1, a, a + n + 1, a + n]
    scene = scenes.scene_from_meshes([(pos, np.array(idx, dtype=np.uint32), uv)], [l2w], attributes=True)
    return scene


def _relief_scene(l2w, cam):
    from chord_amd import lib as L, records as R
    base = _flat_scene(l2w)
    nm = scenes._pbr_textures(3)[2]
    mats = base.materials.copy()
    mats["normalTexture"], mats["normalSampler"], mats["normalFactorScale"] = 0, 0, 1.0
    mats["baseColorId"] = mats["emissiveTexture"] = mats["metallicRoughnessTexture"] = 0xFFFFFFFF
    mats["bTwoSided"] = 1
    smp = np.array([(SM.NEAREST, SM.NEAREST, SM.REPEAT, SM.REPEAT)], dtype=R.SAMPLER)
    scene = R.Scene(base.objects, base.primitives, mats, base.meshlets, base.groups, base.group_indices, base.meshlet_data, base.positions,
                    texcoord0=base.texcoord0, textures=[nm], samplers=smp, bvh_nodes=base.bvh_nodes, normals=base.normals, tangents=base.tangents)
    scene.local_to_world = base.local_to_world
    L.fill_objects(scene, cam)
    return scene, nm


@pytest.mark.parametrize("kind", ["stretched", "mirrored"])
def test_pixel_normal_in_the_faces_tangent_frame(built_lib, kind):
    import orc
    from chord_amd import lib as L
    S3 = np.diag([3.0, 1.0, 0.5, 1.0]) if kind == "stretched" else np.diag([-1.5, 1.0, 0.8, 1.0])
    l2w = scenes.translate(0.0, 0.2, -6.0) @ scenes.rotate_y(0.5) @ scenes.rotate_x(-0.3) @ S3
    cam = scenes.Camera((0.0, 0.3, 0.0), (0.0, -0.05, -1.0), 192, 128)
    scene, nm = _relief_scene(l2w, cam)
    view, iv = L.make_views(cam)
    fr = orc.frame(scene, view, iv, H.ALL_FLAGS)
    w, h = cam.width, cam.height

    def angles(tangents):
        st = {}
        got = SM.resolve(scene, fr["vis"], fr["cmds"], view, iv, w, h, names=("pixelNormal",), stats=st, tangents=tangents)
        hit = st["pbr"]
        assert hit.sum() > 0.1 * w * h
        uv = SM.SR.resolve(scene, fr["vis"], fr["cmds"], view, iv, w, h, names=("uv",))["uv"].reshape(-1, 2)[hit]
        # the float64 frame of the face as ChordSurfaceTargets defines it: N the inverse-transpose image of the face normal, T the
        # image of the tangent made orthogonal to N, B = cross(N, T) times the handedness the asset states
        M = l2w[:3, :3]
        N = np.linalg.inv(M).T @ np.array([0.0, 0.0, 1.0]); N /= np.linalg.norm(N)
        T = M @ np.array([1.0, 0.0, 0.0]); T = T - (T @ N) * N; T /= np.linalg.norm(T)
        t_ls = scene.tangents[0]
        B = np.cross(N, T) * float(t_ls[3])
        # the texel the NEAREST sampler reads, decoded in float64
        H_, W_ = nm.shape[:2]
        ix = np.mod(np.floor(uv[:, 0].astype(np.float64) * W_).astype(np.int64), W_)
        iy = np.mod(np.floor(uv[:, 1].astype(np.float64) * H_).astype(np.int64), H_)
        xy = nm[iy, ix, :2].astype(np.float64) / 255.0 * 2.0 - 1.0
        z = np.sqrt(np.maximum(0.0, 1.0 - (xy ** 2).sum(1)))
        n_t = np.concatenate([xy, z[:, None]], 1); n_t /= np.linalg.norm(n_t, axis=1, keepdims=True)
        p = got["pixelNormal"].reshape(-1, 4)[hit][:, :3].astype(np.float64)
        p /= np.linalg.norm(p, axis=1, keepdims=True)
        local = np.stack([p @ T, p @ B, p @ N], 1)
        return np.arctan2(np.linalg.norm(np.cross(local, n_t), axis=1), (local * n_t).sum(1)), float(t_ls[3])
    ang, wsign = angles(None)
    assert ang.max() < 1e-4, ang.max()
    assert np.all(scene.tangents[:, 3] == wsign)
    if kind == "mirrored":
        flipped = scene.tangents.copy()
        flipped[:, 3] *= -1.0
        bad, _ = angles(flipped)
        assert np.median(bad) > 0.05, "dropping the bitangent's sign must show"


# ---- 6. the GPU comparison cannot pass on trivial inputs ----------------------------------------------------------------------

def test_material_test_scene_exercises_the_sampler(built_lib):
    scene, cam, view, iv, fr = _frame(scenes.material_test_scene, 320, 200)
    w, h = cam.width, cam.height
    st = {}
    out = SM.resolve(scene, fr["vis"], fr["cmds"], view, iv, w, h, stats=st)
    pbr = st["pbr"]
    n = int(pbr.sum())
    assert n > 0.5 * w * h
    mag, two, last = (np.zeros(w * h, bool) for _ in range(3))
    wrapped, textured = {}, {}
    for slot, runs in st["slots"].items():
        t = np.zeros(w * h, bool)
        for s in runs:
            p = s["pix"]
            t[p] = True
            mag[p] |= s["lodq"] <= 0
            two[p] |= (s["l1"] != s["l0"]) & (s["f"] > 0)
            last[p] |= (np.maximum(s["l0"], s["l1"]) == s["last"]) & (s["lodq"] > 0)
            for mode, flags in s["wrapped"].items():
                wrapped.setdefault(mode, np.zeros(w * h, bool))[p] |= flags
        textured[slot] = t
    assert mag.sum() >= 0.10 * n and two.sum() >= 0.10 * n and last.sum() >= 0.01 * n, (mag.sum(), two.sum(), last.sum(), n)
    for mode in WRAPS:
        assert wrapped[mode].sum() >= 100, mode
    for slot in SM.SLOTS:
        assert (textured[slot] & pbr).sum() >= 0.10 * n and (pbr & ~textured[slot]).sum() >= 0.05 * n, slot
    S = SS.resolve(scene, fr["vis"], fr["cmds"], view, iv, w, h)
    N = S["vertexNormal"].reshape(-1, 4)[:, :3].astype(np.float64)
    P = out["pixelNormal"].reshape(-1, 4)[:, :3].astype(np.float64)
    cosang = (N * P).sum(1) / np.maximum(np.linalg.norm(N, axis=1) * np.linalg.norm(P, axis=1), 1e-30)
    assert (pbr & (cosang < math.cos(math.radians(5.0)))).sum() >= 0.10 * n
    assert (st["hit"] & ~pbr).sum() >= 1, "a covered pixel of materialType 0"
    for name, img in out.items():
        assert not np.isnan(img).any(), name
    used = set()
    for m in np.unique(st["material"][st["material"] >= 0]):
        for slot in SM.SLOTS:
            used.add(SM.slot_texture(scene, scene.materials[m], slot)[1][0])
    assert used >= set(FILTERS), "all six filter values across the slots"
