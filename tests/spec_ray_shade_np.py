"""The specification of shading ray hits -- material, normal and uv at the hit points of chordvis_trace_rays -- in numpy float32:
RayHitMaterialInfo::init of the reference's raytrace_shared.hlsli over this project's pinned sampler.  It defines the answer of the
library call that is to follow it; no kernel implements it yet.  One rounding per operation, no contraction.  Built on
spec_material_np (sample_level, levels_of, slot_texture, tables) and spec_surface_np (normalize), which it calls and does not restate.
TEST INFRASTRUCTURE: never imported by chord_amd/.

Per hit (records.RAY_HIT), against the object records `objects` (the array the frames read now) over `scene`:
  meshlet   the hit's meshlet is ASSET-RELATIVE (ChordRayHit::meshlet, as chordvis_trace_rays and chordvis_pixel_rays write it): an index
            into the meshlets of the asset of the OBJECT's primitive.  In a scene of several assets -- `scene` is then the one-asset twin
            of tests/multi_asset.py, the assets' arrays concatenated in the upload's order -- asset_meshlet_base[primitive] and
            asset_meshlet_count[primitive] give that asset's first meshlet in scene.meshlets and its meshlet count: the meshlet is read
            at base + meshlet.  A records.Scene as it stands is one asset: base 0, count len(scene.meshlets), the defaults.
  valid     status bit 0 set; u and v finite; object < len(objects); the object's primitive and material ids below their counts;
            meshlet < the meshlet count of the primitive's asset; triangle < the meshlet's triangle count; the triangle word, the three
            vertex-id words and the three vertex ids inside their arrays.  An invalid hit gives sixteen zero words.
  vertices  spec_surface_np.vertex_ids' walk from (object, meshlet, triangle): meshlet data at dataOffset, V vertex-id words, the
            triangle word at dataOffset + V + triangle, ids + the primitive's vertexOffset.  lod0IndicesOffset stays unread.
  b         ((1 - u) - v, u, v)
  uv        (uv0 * b.x + uv1 * b.y) + uv2 * b.z per component; (0, 0) for a scene without texture coordinates
  normal    per vertex nRS = normalize(mul(float4(nLS, 0), translatedWorldToLocal).xyz) (spec_surface_np.vertex_frames' statement),
            interpolated like uv, THEN normalised (raytrace_shared.hlsli:92); normalize gives 0 where the squared length is not above 0;
            negated when the material is two-sided and the hit a back face; zero for a scene without normals
  level     lod = lods[i] if given else lod; lodq = (int32) floor(min(max(lod, 0), 15) * 256), NaN -> 0; then spec_material_np.sample's
            item 3 from that lodq: minified iff lodq > 0, *_MIPMAP_NEAREST level min((lodq + 128) >> 8, last), *_MIPMAP_LINEAR levels
            l0 = min(lodq >> 8, last), l1 = min(l0 + 1, last), f = (lodq & 255) / 256, otherwise level 0; min / mag filter inside a level
  fields    baseColor = sample * baseColorFactor, rgb through sRGB -> AP1, white without a texture; emissive = sample.rgb * emissiveFactor,
            zero without one (NOT through sRGB -> AP1: the material resolve's path, a departure from the reference's hit shading);
            roughness, metallic = .g, .b of the metallic-roughness texture, or roughnessFactor, (metallicFactor >= 1 ? 0 : metallicFactor);
            a material whose materialType is not 1 leaves these zero and RAYSURF_PBR clear.
"""
import numpy as np

from chord_amd import records as R

import spec_material_np as SM
import spec_surface_np as SS

f32 = np.float32
u32 = np.uint32
# the record a shaded hit gives: 64 bytes, sixteen words; an invalid hit is sixteen zero words
RAY_HIT_SURFACE = np.dtype([("baseColor", f32, 4), ("emissive", f32, 3), ("roughness", f32), ("normal", f32, 3), ("metallic", f32),
                            ("uv", f32, 2), ("material", u32), ("flags", u32)])
assert RAY_HIT_SURFACE.itemsize == 64
# flags: the record is filled; copied from the hit's CHORD_RAY_BACK_FACE; the material's bTwoSided; materialType == 1
RAYSURF_VALID, RAYSURF_BACK_FACE, RAYSURF_TWO_SIDED, RAYSURF_PBR = 1, 2, 4, 8
MATERIAL_SLOTS = (("baseColor", True), ("emissive", True), ("metallicRoughness", False))


def lodq_of_level(lod):
    """float32 array of levels -> int32 lodq"""
    lod = np.asarray(lod, dtype=f32)
    with np.errstate(all="ignore"):
        l = np.where(lod > f32(0.0), lod, f32(0.0)).astype(f32)
        l = np.where(l < f32(15.0), l, f32(15.0)).astype(f32)
        return np.floor(l * f32(256.0)).astype(np.int32)


def levels_from_lodq(lodq, min_filter, mag_filter, last):
    """item 3 of spec_material_np's sampler from a given lodq: (linear (N,) bool, l0, l1 (N,) int64, f (N,) float32)"""
    is_lin = lambda f: f in (SM.LINEAR, SM.LINEAR_MIPMAP_NEAREST, SM.LINEAR_MIPMAP_LINEAR)
    lodq = np.asarray(lodq, dtype=np.int32)
    minified = lodq > 0
    linear = np.where(minified, is_lin(min_filter), is_lin(mag_filter))
    l0 = np.zeros(len(lodq), dtype=np.int64)
    l1 = l0.copy()
    if min_filter in (SM.NEAREST_MIPMAP_NEAREST, SM.LINEAR_MIPMAP_NEAREST):
        l0 = np.where(minified, np.minimum((lodq.astype(np.int64) + 128) >> 8, last), 0)
        l1 = l0.copy()
    elif min_filter in (SM.NEAREST_MIPMAP_LINEAR, SM.LINEAR_MIPMAP_LINEAR):
        l0 = np.where(minified, np.minimum(lodq.astype(np.int64) >> 8, last), 0)
        l1 = np.where(minified, np.minimum(l0 + 1, last), 0)
    f = (lodq & 255).astype(f32) * f32(1.0 / 256.0)
    return linear, l0, l1, f


def sample_lod(levels, sampler, u, v, lodq, srgb, stats=None):
    """One texture at an explicit lodq per element -> (N, 4) float32.  stats: a dict that receives l0, l1, f, last."""
    min_f, mag_f, wrap_s, wrap_t = (int(x) for x in sampler)
    last = len(levels) - 1
    linear, l0, l1, f = levels_from_lodq(lodq, min_f, mag_f, last)
    if stats is not None:
        stats.update(l0=l0, l1=l1, f=f, last=last, mip_filtered=min_f not in (SM.NEAREST, SM.LINEAR))
    out = np.zeros((len(u), 4), dtype=f32)
    with np.errstate(all="ignore"):
        for l in range(len(levels)):
            k = np.nonzero(l0 == l)[0]
            if not len(k):
                continue
            c0 = SM.sample_level(levels[l], wrap_s, wrap_t, linear[k], u[k], v[k], srgb)
            two = l1[k] != l
            if np.any(two):
                kk = k[two]
                c1 = SM.sample_level(levels[min(l + 1, last)], wrap_s, wrap_t, linear[kk], u[kk], v[kk], srgb)
                c0[two] = c0[two] + (c1 - c0[two]) * f[kk][:, None]
            out[k] = c0
    return out


def validate(scene, objects, hits, asset_meshlet_base=None, asset_meshlet_count=None):
    """(valid (N,) bool, vertex ids (N, 3) int64 -- zeros where invalid, material (N,) int64).  asset_meshlet_base /
    asset_meshlet_count: per primitive, the first meshlet and the meshlet count of its asset in scene.meshlets (None: one asset)."""
    hits = np.ascontiguousarray(hits, dtype=R.RAY_HIT).reshape(-1)
    n = len(hits)
    with np.errstate(all="ignore"):
        ok = ((hits["status"] & u32(1)) != 0) & np.isfinite(hits["u"]) & np.isfinite(hits["v"])
    o, mid, tri = hits["object"].astype(np.int64), hits["meshlet"].astype(np.int64), hits["triangle"].astype(np.int64)
    ok &= o < len(objects)
    o = np.where(ok, o, 0)
    prim = objects["GLTFPrimitiveDetail"][o].astype(np.int64)
    mat = objects["GLTFMaterialData"][o].astype(np.int64)
    ok &= (prim < len(scene.primitives)) & (mat < len(scene.materials))
    prim, mat = np.where(ok, prim, 0), np.where(ok, mat, 0)
    mbase = np.zeros(len(scene.primitives), dtype=np.int64) if asset_meshlet_base is None else np.asarray(asset_meshlet_base, dtype=np.int64)
    mcount = np.full(len(scene.primitives), len(scene.meshlets), dtype=np.int64) if asset_meshlet_count is None else \
        np.asarray(asset_meshlet_count, dtype=np.int64)
    assert len(mbase) == len(mcount) == len(scene.primitives)
    ok &= mid < mcount[prim]                               # asset-relative: below THAT asset's count
    mid = np.where(ok, mid + mbase[prim], 0)               # ... and read at base + meshlet
    ok &= mid < len(scene.meshlets)
    mid = np.where(ok, mid, 0)
    m = scene.meshlets[mid]
    V = (m["vertexTriangleCount"] & u32(0xFF)).astype(np.int64)
    T = ((m["vertexTriangleCount"] >> u32(8)) & u32(0xFF)).astype(np.int64)
    ok &= tri < T
    tri = np.where(ok, tri, 0)
    base = m["dataOffset"].astype(np.int64)
    words = len(scene.meshlet_data)
    at = base + V + tri
    ok &= at < words
    tri_word = scene.meshlet_data[np.where(ok, at, 0)]
    vb = scene.primitives["vertexOffset"][prim].astype(np.int64)
    vi = np.zeros((n, 3), dtype=np.int64)
    for k in range(3):
        at = base + ((tri_word >> u32(8 * k)) & u32(0xFF)).astype(np.int64)
        ok &= at < words
        vid = scene.meshlet_data[np.where(ok, at, 0)].astype(np.int64) + vb
        ok &= vid < len(scene.positions)
        vi[:, k] = vid
    vi[~ok] = 0
    return ok, vi, np.where(ok, mat, 0)


def shade(scene, objects, hits, lod=0.0, lods=None, normals="scene", stats=None, asset_meshlet_base=None, asset_meshlet_count=None):
    """RAY_HIT_SURFACE per hit.  objects: the records.OBJECT array the hits are shaded against; normals: the stream the device
    holds (default: the scene's; None: a scene uploaded without).  asset_meshlet_base / asset_meshlet_count: validate's.  stats: a dict that receives "slots": per sampled (material, slot) a
    dict of sample_lod's statistics with "hits" (the indices that sampled it) and "material"."""
    hits = np.ascontiguousarray(hits, dtype=R.RAY_HIT).reshape(-1)
    objects = np.ascontiguousarray(objects, dtype=R.OBJECT)
    n = len(hits)
    out = np.zeros(n, dtype=RAY_HIT_SURFACE)
    if stats is not None:
        stats["slots"] = []
    if n == 0:
        return out
    srgb, ap1 = SM.tables()
    valid, vi, mat = validate(scene, objects, hits, asset_meshlet_base, asset_meshlet_count)
    idx = np.nonzero(valid)[0]
    if not len(idx):
        return out
    normals = scene.normals if isinstance(normals, str) else normals
    h = hits[idx]
    vi, mat = vi[idx], mat[idx]
    with np.errstate(all="ignore"):
        hu, hv = h["u"].astype(f32), h["v"].astype(f32)
        b = np.stack([(f32(1.0) - hu) - hv, hu, hv], axis=-1).astype(f32)

        def interp(a):                                     # a (N, 3 vertices, C) -> (N, C)
            return (a[:, 0] * b[:, 0:1] + a[:, 1] * b[:, 1:2]) + a[:, 2] * b[:, 2:3]
        uv = np.zeros((len(idx), 2), dtype=f32)
        if scene.texcoord0 is not None:
            uv = interp(scene.texcoord0[vi]).astype(f32)
        nrm = np.zeros((len(idx), 3), dtype=f32)
        if normals is not None:
            w = objects["translatedWorldToLocal"][h["object"]].astype(f32).reshape(-1, 4, 4).transpose(0, 2, 1)    # [r][c]
            nl = np.asarray(normals, dtype=f32)[vi]
            x, y, z = nl[..., 0], nl[..., 1], nl[..., 2]
            w = w[:, None]
            nw = np.stack([(x * w[..., 0, j] + y * w[..., 1, j]) + z * w[..., 2, j] for j in range(3)], axis=-1)
            nrm = SS.normalize(interp(SS.normalize(nw.astype(f32))).astype(f32))
    two_sided = scene.materials["bTwoSided"][mat] != 0
    back = (h["status"] & u32(2)) != 0
    nrm = np.where((two_sided & back)[:, None], -nrm, nrm).astype(f32)
    flags = np.full(len(idx), RAYSURF_VALID, dtype=u32) | np.where(back, u32(RAYSURF_BACK_FACE), u32(0)) | \
        np.where(two_sided, u32(RAYSURF_TWO_SIDED), u32(0))
    lodq = lodq_of_level(np.full(n, lod, dtype=f32) if lods is None else np.asarray(lods, dtype=f32).reshape(-1))[idx]

    base = np.zeros((len(idx), 4), dtype=f32)
    emis = np.zeros((len(idx), 3), dtype=f32)
    rough = np.zeros(len(idx), dtype=f32)
    metal = np.zeros(len(idx), dtype=f32)
    for m in np.unique(mat):
        M = scene.materials[m]
        if int(M["materialType"]) != SM.PBR_TYPE:
            continue
        k = np.nonzero(mat == m)[0]
        flags[k] |= u32(RAYSURF_PBR)
        u, v, lq = uv[k, 0], uv[k, 1], lodq[k]

        def tex(slot, is_srgb):
            levels, smp = SM.slot_texture(scene, M, slot)
            if levels is None:
                return None
            st = None if stats is None else {"hits": idx[k], "material": int(m), "slot": slot}
            c = sample_lod(levels, smp, u, v, lq, srgb if is_srgb else None, st)
            if st is not None:
                stats["slots"].append(st)
            return c
        with np.errstate(all="ignore"):
            c = tex("baseColor", True)
            if c is None:
                c = np.ones((len(k), 4), dtype=f32)
            c = c * np.asarray(M["baseColorFactor"], dtype=f32)[None, :]
            r, g, bl = c[:, 0], c[:, 1], c[:, 2]
            base[k] = np.stack([(ap1[i, 0] * r + ap1[i, 1] * g) + ap1[i, 2] * bl for i in range(3)] + [c[:, 3]], axis=-1)
            c = tex("emissive", True)
            if c is None:
                c = np.zeros((len(k), 4), dtype=f32)
            emis[k] = c[:, :3] * np.asarray(M["emissiveFactor"], dtype=f32)[None, :]
            c = tex("metallicRoughness", False)
            if c is None:
                mf = f32(M["metallicFactor"])
                rough[k], metal[k] = f32(M["roughnessFactor"]), (f32(0.0) if mf >= f32(1.0) else mf)
            else:
                rough[k], metal[k] = c[:, 1], c[:, 2]
    out["baseColor"][idx], out["emissive"][idx], out["roughness"][idx] = base, emis, rough
    out["normal"][idx], out["metallic"][idx], out["uv"][idx] = nrm, metal, uv
    out["material"][idx], out["flags"][idx] = mat.astype(u32), flags
    return out
