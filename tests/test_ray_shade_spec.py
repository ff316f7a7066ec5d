"""tests/spec_ray_shade_np.py (the specification of shading ray hits) held to a scalar, loop-written evaluation on one textured
triangle; its level rule at the edges of the level's range; renormalisation and the two-sided flip; every invalid-record rule; and
that the ray sets chosen for the four test scenes exercise what they are meant to.  CPU only."""
import math

import numpy as np
import pytest

from chord_amd import records as R

import ray_shade_cases as RC
import spec_material_np as SM
import spec_ray_shade_np as RS

f32 = np.float32


# ---- a scalar evaluation, written with loops over one hit at a time ---------------------------------------------------------------

def _wrap1(i, n, mode):
    if mode == SM.CLAMP_TO_EDGE:
        return min(max(i, 0), n - 1)
    if mode == SM.MIRRORED_REPEAT:
        m = i % (2 * n)
        return m if m < n else 2 * n - 1 - m
    return i % n


def _texel1(level, ix, iy, srgb):
    w = int(level[iy, ix])
    b = [(w >> (8 * k)) & 255 for k in range(4)]
    return [srgb[b[k]] if (srgb is not None and k < 3) else f32(b[k]) * f32(1.0 / 255.0) for k in range(4)]


def _level1(level, wrap_s, wrap_t, linear, u, v, srgb):
    H, W = level.shape
    if not linear:
        ix = _wrap1(int(math.floor(f32(u * f32(W)))), W, wrap_s)
        iy = _wrap1(int(math.floor(f32(v * f32(H)))), H, wrap_t)
        return _texel1(level, ix, iy, srgb)
    x, y = f32(f32(u * f32(W)) - f32(0.5)), f32(f32(v * f32(H)) - f32(0.5))
    x0, y0 = int(math.floor(x)), int(math.floor(y))
    fx, fy = f32(x - f32(x0)), f32(y - f32(y0))
    ix0, ix1, iy0, iy1 = _wrap1(x0, W, wrap_s), _wrap1(x0 + 1, W, wrap_s), _wrap1(y0, H, wrap_t), _wrap1(y0 + 1, H, wrap_t)
    a00, a10, a01, a11 = (_texel1(level, ix, iy, srgb) for ix, iy in ((ix0, iy0), (ix1, iy0), (ix0, iy1), (ix1, iy1)))
    out = []
    for k in range(4):
        top = f32(a00[k] + f32(f32(a10[k] - a00[k]) * fx))
        bot = f32(a01[k] + f32(f32(a11[k] - a01[k]) * fx))
        out.append(f32(top + f32(f32(bot - top) * fy)))
    return out


def _sample1(scene, M, slot, u, v, lod, srgb):
    levels, smp = SM.slot_texture(scene, M, slot)
    if levels is None:
        return None
    min_f, mag_f, wrap_s, wrap_t = smp
    lod = f32(lod)
    l = f32(0.0) if not (lod > 0) else lod
    l = l if l < f32(15.0) else f32(15.0)
    lodq = int(math.floor(l * 256.0))
    last = len(levels) - 1
    lin = lambda f: f in (SM.LINEAR, SM.LINEAR_MIPMAP_NEAREST, SM.LINEAR_MIPMAP_LINEAR)
    linear, l0, l1 = lin(mag_f), 0, 0
    if lodq > 0:
        linear = lin(min_f)
        if min_f in (SM.NEAREST_MIPMAP_NEAREST, SM.LINEAR_MIPMAP_NEAREST):
            l0 = l1 = min((lodq + 128) >> 8, last)
        elif min_f in (SM.NEAREST_MIPMAP_LINEAR, SM.LINEAR_MIPMAP_LINEAR):
            l0 = min(lodq >> 8, last)
            l1 = min(l0 + 1, last)
    c = _level1(levels[l0], wrap_s, wrap_t, linear, u, v, srgb)
    if l1 != l0:
        c1 = _level1(levels[l1], wrap_s, wrap_t, linear, u, v, srgb)
        f = f32(f32(lodq & 255) * f32(1.0 / 256.0))
        c = [f32(c[k] + f32(f32(c1[k] - c[k]) * f)) for k in range(4)]
    return c


def _norm1(v):
    l2 = f32(f32(f32(v[0] * v[0]) + f32(v[1] * v[1])) + f32(v[2] * v[2]))
    if not (l2 > 0):
        return [f32(0.0)] * 3
    s = f32(np.sqrt(l2))
    return [f32(x / s) for x in v]


def _shade1(scene, h, lod):
    """One hit on ray_shade_cases.triangle_scene (one meshlet, one triangle: vertices 0, 1, 2) -> the sixteen words"""
    out = np.zeros(1, dtype=RS.RAY_HIT_SURFACE)
    srgb, ap1 = SM.tables()
    obj = scene.objects[int(h["object"])]
    M = scene.materials[int(obj["GLTFMaterialData"])]
    u, v = f32(h["u"]), f32(h["v"])
    b = [f32(f32(f32(1.0) - u) - v), u, v]
    ip = lambda a0, a1, a2: f32(f32(f32(a0 * b[0]) + f32(a1 * b[1])) + f32(a2 * b[2]))
    uv = [ip(*[f32(scene.texcoord0[k, c]) for k in range(3)]) for c in range(2)]
    w = obj["translatedWorldToLocal"].astype(f32)                       # column-major: [r][c] = w[c * 4 + r]
    ns = []
    for k in range(3):
        x, y, z = (f32(t) for t in scene.normals[k])
        ns.append(_norm1([f32(f32(f32(x * w[j * 4 + 0]) + f32(y * w[j * 4 + 1])) + f32(z * w[j * 4 + 2])) for j in range(3)]))
    n = _norm1([ip(ns[0][c], ns[1][c], ns[2][c]) for c in range(3)])
    flags = 1 | (2 if int(h["status"]) & 2 else 0) | (4 if int(M["bTwoSided"]) else 0)
    if (flags & 6) == 6:
        n = [f32(-x) for x in n]
    if int(M["materialType"]) == 1:
        flags |= 8
        c = _sample1(scene, M, "baseColor", uv[0], uv[1], lod, srgb) or [f32(1.0)] * 4
        c = [f32(c[k] * f32(M["baseColorFactor"][k])) for k in range(4)]
        out["baseColor"][0] = [f32(f32(f32(ap1[i, 0] * c[0]) + f32(ap1[i, 1] * c[1])) + f32(ap1[i, 2] * c[2])) for i in range(3)] + [c[3]]
        e = _sample1(scene, M, "emissive", uv[0], uv[1], lod, srgb) or [f32(0.0)] * 4
        out["emissive"][0] = [f32(e[k] * f32(M["emissiveFactor"][k])) for k in range(3)]
        mr = _sample1(scene, M, "metallicRoughness", uv[0], uv[1], lod, None)
        if mr is None:
            mf = f32(M["metallicFactor"])
            out["roughness"], out["metallic"] = f32(M["roughnessFactor"]), (f32(0.0) if mf >= 1 else mf)
        else:
            out["roughness"], out["metallic"] = mr[1], mr[2]
    out["normal"][0], out["uv"][0], out["material"], out["flags"] = n, uv, int(obj["GLTFMaterialData"]), flags
    return out


@pytest.fixture(scope="module")
def tri():
    return RC.triangle_scene()


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1, 16)


def test_spec_equals_a_scalar_evaluation(tri):
    scene, cam = tri
    bary = [(0.25, 0.25), (0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.7, 0.1), (0.05, 0.9), (1.3, -0.2), (0.333, 0.333)]
    hits = np.concatenate([RC.hit(o, u, v, status=1 | (2 if (k + o) % 2 else 0)) for o in range(4) for k, (u, v) in enumerate(bary)])
    for lod in (0.0, 0.5, 1.0, 2.25, 20.0):
        got = RS.shade(scene, scene.objects, hits, lod=lod)
        want = np.concatenate([_shade1(scene, h, lod) for h in hits])
        assert np.array_equal(_words(got), _words(want)), "lod %g: hits %s differ" % (lod, np.flatnonzero((_words(got) != _words(want)).any(axis=1)))
    lods = np.linspace(-1.0, 5.0, len(hits)).astype(f32)
    got = RS.shade(scene, scene.objects, hits, lod=9.0, lods=lods)
    want = np.concatenate([_shade1(scene, h, l) for h, l in zip(hits, lods)])
    assert np.array_equal(_words(got), _words(want)), "per-hit lods"
    assert np.unique(_words(got), axis=0).shape[0] > len(hits) // 2


def test_level_rule():
    last = 4
    lods = np.array([0.0, 2.0 ** -9, 0.5, 1.0, 2.25, last, last + 3, 20.0, -1.0, np.nan, np.inf, -np.inf], dtype=f32)
    q = RS.lodq_of_level(lods)
    assert q.tolist() == [0, 0, 128, 256, 576, 1024, 1792, 3840, 0, 0, 3840, 0]
    lin, l0, l1, f = RS.levels_from_lodq(q, SM.LINEAR_MIPMAP_LINEAR, SM.NEAREST, last)
    assert l0.tolist() == [0, 0, 0, 1, 2, 4, 4, 4, 0, 0, 4, 0] and l1.tolist() == [0, 0, 1, 2, 3, 4, 4, 4, 0, 0, 4, 0]
    assert f.tolist() == [0, 0, 0.5, 0, 0.25, 0, 0, 0, 0, 0, 0, 0]
    assert lin.tolist() == [q_ > 0 for q_ in q.tolist()]                    # minified iff lodq > 0: the min filter is the linear one here
    lin, l0, l1, f = RS.levels_from_lodq(q, SM.NEAREST_MIPMAP_NEAREST, SM.LINEAR, last)
    assert l0.tolist() == [0, 0, 1, 1, 2, 4, 4, 4, 0, 0, 4, 0] and np.array_equal(l0, l1)
    assert lin.tolist() == [q_ <= 0 for q_ in q.tolist()]
    lin, l0, l1, f = RS.levels_from_lodq(q, SM.LINEAR, SM.NEAREST, last)    # no mip filtering: level 0 whatever the lod
    assert not l0.any() and not l1.any() and lin.tolist() == [q_ > 0 for q_ in q.tolist()]
    # the smallest level above 0 whose lodq is above 0 is 2^-8
    assert RS.lodq_of_level(np.array([2.0 ** -8, np.nextafter(f32(2.0 ** -8), f32(0.0))], dtype=f32)).tolist() == [1, 0]


def test_normal_is_renormalised_and_flipped(tri):
    scene, cam = tri
    hits = np.concatenate([RC.hit(o, 0.3, 0.4, status=s) for o in range(4) for s in (1, 3)])
    out = RS.shade(scene, scene.objects, hits)
    n = out["normal"].astype(np.float64)
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-6)
    # the interpolated vertex normals themselves are shorter than 1 (three different directions): normalising is not a no-op
    import spec_surface_np as SS
    w = np.swapaxes(scene.objects["translatedWorldToLocal"].astype(f32).reshape(-1, 4, 4), -1, -2)
    x, y, z = (scene.normals[:3, k] for k in range(3))
    for o in range(4):
        nv = SS.normalize(np.stack([(x * w[o, 0, j] + y * w[o, 1, j]) + z * w[o, 2, j] for j in range(3)], axis=-1))
        raw = (nv[0] * ((f32(1.0) - f32(0.3)) - f32(0.4)) + nv[1] * f32(0.3)) + nv[2] * f32(0.4)
        assert np.linalg.norm(raw.astype(np.float64)) < 0.98
        assert np.array_equal(out["normal"][2 * o], SS.normalize(raw))
    two = scene.materials["bTwoSided"][scene.objects["GLTFMaterialData"]] != 0
    assert two.tolist() == [False, True, True, False]
    for o in range(4):
        front, back = out[2 * o], out[2 * o + 1]
        assert np.array_equal(back["normal"], -front["normal"] if two[o] else front["normal"]), o
        assert back["flags"] == front["flags"] | RS.RAYSURF_BACK_FACE and bool(front["flags"] & RS.RAYSURF_TWO_SIDED) == bool(two[o])
        for k in ("baseColor", "emissive", "roughness", "metallic", "uv", "material"):
            assert np.array_equal(back[k], front[k]), (o, k)
    # a stream of zero normals, and a scene without normals: a zero normal
    zero = RS.shade(scene, scene.objects, hits[::2], normals=np.zeros_like(scene.normals))
    none = RS.shade(scene, scene.objects, hits[::2], normals=None)
    assert not zero["normal"].any() and not none["normal"].any() and np.array_equal(_words(zero), _words(none))
    # a material of another type: flags without PBR, zero material fields, normal and uv written
    other = out[6]
    assert other["flags"] == RS.RAYSURF_VALID and not other["baseColor"].any() and not other["emissive"].any() and other["roughness"] == 0 and other["metallic"] == 0
    assert other["normal"].any() and other["uv"].any() and other["material"] == scene.objects["GLTFMaterialData"][3]
    assert out[0]["flags"] == RS.RAYSURF_VALID | RS.RAYSURF_PBR
    # the material without textures: its factors
    plain = out[4]
    assert plain["roughness"] == f32(0.6) and plain["metallic"] == f32(0.25) and not plain["emissive"].any() and plain["baseColor"][3] == 1.0
    assert out[2]["metallic"] == 0.0 and out[2]["roughness"] == f32(0.35)    # metallicFactor 1 without a texture reads 0


def test_invalid_records(tri):
    scene, cam = tri
    good = RC.hit(1, 0.2, 0.2, status=3)
    for what, h in RC.invalid_hits(scene):
        out = RS.shade(scene, scene.objects, np.concatenate([good, h, good]), lod=1.5)
        assert not _words(out[1:2]).any(), what
        assert np.array_equal(_words(out[0:1]), _words(out[2:3])) and out[0]["flags"] & RS.RAYSURF_VALID, what
    # a vertex id one past the scene's vertices, and at 0xFFFFFFFF; a material index one past the table
    for vid in (len(scene.positions), 0xFFFFFFFF):
        data = scene.meshlet_data.copy()
        data[1] = vid
        bad = R.Scene(scene.objects, scene.primitives, scene.materials, scene.meshlets, scene.groups, scene.group_indices, data, scene.positions,
                      texcoord0=scene.texcoord0, textures=scene.texture_images, samplers=scene.samplers, normals=scene.normals, tangents=scene.tangents)
        assert not _words(RS.shade(bad, bad.objects, good)).any(), vid
    objs = scene.objects.copy()
    objs["GLTFMaterialData"][1] = len(scene.materials)
    assert not _words(RS.shade(scene, objs, good)).any()
    # (u, v) outside the triangle extrapolates and is valid
    out = RS.shade(scene, scene.objects, np.concatenate([RC.hit(0, 1.5, -0.75), RC.hit(0, -2.0, 4.0)]))
    assert (out["flags"] & RS.RAYSURF_VALID).all() and np.isfinite(out["uv"]).all()


@pytest.mark.parametrize("name", sorted(RC.SCENES))
def test_ray_sets_exercise_the_specification(name):
    """The pixel rays and the random rays of each test scene, traced by the ray specification: at least a fifth hit, every textured
    material the scene names is met by 16 hits or more, both faces occur on one-sided and on two-sided materials, and over the five
    level runs every mip-filtered slot reads two levels and every *_MIPMAP_LINEAR slot blends two (ray_shade_cases.vacuity)."""
    import spec_rays_np as S
    scene, cam, view, iv, rays = RC.case(name)
    hits = S.trace(scene, scene.objects, rays, meshlet_cull=True)
    runs = RC.shade_runs(scene, scene.objects, hits)
    bad = RC.vacuity(scene, name, hits, [(want, stats) for _, _, _, want, stats in runs])
    assert not bad, "%s: %s" % (name, "; ".join(bad))
    for _, _, _, want, _ in runs:
        assert not np.isnan(want.view(f32)).any()
