"""The surface channels of chordvis_resolve_surface (include/chordvis.h ChordSurfaceTargets) restated in vectorised numpy float32:
nanite_shared.hlsli:157-175 (normalRS / tangentRS / bitangentRS of getTriangleMiscInfo) and material.hlsli:95-108 (their
interpolation).  TEST INFRASTRUCTURE: never imported by chord_amd/.

Per vertex, every + - * / sqrt a float32 array operation in source order (numpy rounds each one separately, no contraction):
  nRS = normalize(mul(float4(nLS, 0), translatedWorldToLocal).xyz)   component j = (x * m0j + y * m1j) + z * m2j (no w term)
  t   = mul(localToTranslatedWorld, float4(tLS.xyz, 0)).xyz          component i = (mi0 * x + mi1 * y) + mi2 * z
  tRS = normalize(t - dot(t, nRS) * nRS)
  bRS = cross(nRS, tRS) * tLS.w
normalize(v) = v / sqrt((x * x + y * y) + z * z) per component; a vector whose squared length is not above 0 gives 0.  Per pixel
(a0 * b.x + a1 * b.y) + a2 * b.z with the barycentrics of spec_resolve_np, not renormalised."""
import numpy as np

from spec_np import mat
import spec_resolve_np as SR

f32 = np.float32
u32 = np.uint32
NAMES = ("vertexNormal", "tangent", "bitangent")


def normalize(v):
    """v (..., 3) float32 -> v / sqrt(dot(v, v)) per component, 0 where dot(v, v) is not above 0"""
    l2 = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
    with np.errstate(all="ignore"):
        s = np.sqrt(l2)[..., None]
        out = v / s
    return np.where((l2 > f32(0.0))[..., None], out, f32(0.0)).astype(f32)


def vertex_frames(n_ls, t_ls, l2tw, tw2l):
    """n_ls (..., 3), t_ls (..., 4), the two matrices (..., 4, 4) indexed [r][c] -> nRS, tRS, bRS (..., 3) float32"""
    n_ls = np.asarray(n_ls, dtype=f32); t_ls = np.asarray(t_ls, dtype=f32)
    x, y, z = n_ls[..., 0], n_ls[..., 1], n_ls[..., 2]
    nw = np.stack([(x * tw2l[..., 0, j] + y * tw2l[..., 1, j]) + z * tw2l[..., 2, j] for j in range(3)], axis=-1)
    n = normalize(nw)
    tx, ty, tz, w = t_ls[..., 0], t_ls[..., 1], t_ls[..., 2], t_ls[..., 3]
    tw = np.stack([(l2tw[..., i, 0] * tx + l2tw[..., i, 1] * ty) + l2tw[..., i, 2] * tz for i in range(3)], axis=-1)
    d = (tw[..., 0] * n[..., 0] + tw[..., 1] * n[..., 1]) + tw[..., 2] * n[..., 2]
    t = normalize(tw - d[..., None] * n)
    b = np.stack([(n[..., 1] * t[..., 2] - n[..., 2] * t[..., 1]) * w,
                  (n[..., 2] * t[..., 0] - n[..., 0] * t[..., 2]) * w,
                  (n[..., 0] * t[..., 1] - n[..., 1] * t[..., 0]) * w], axis=-1)
    return n, t, b


def vertex_ids(scene, cmds, lows):
    """(object ids, (N, 3) scene vertex ids) per distinct low word, found as spec_resolve_np.triangle_setup finds them (entries
    whose word is not valid there point at object 0 / some vertex: their pixels are not hit)"""
    lows = np.asarray(lows, dtype=u32)
    slot = ((lows >> u32(8)) & u32(SR.MAX_INSTANCE_ID)).astype(np.int64) - 1
    tri = (lows & u32(0xFF)).astype(np.int64)
    cmd = np.asarray(cmds)[slot]
    o = cmd["objectId"].astype(np.int64)
    mid = cmd["meshletId"].astype(np.int64)
    ok = (o < len(scene.objects)) & (mid < len(scene.meshlets))
    o = np.where(ok, o, 0); mid = np.where(ok, mid, 0)
    m = scene.meshlets[mid]
    V = (m["vertexTriangleCount"] & u32(0xFF)).astype(np.int64)
    T = ((m["vertexTriangleCount"] >> u32(8)) & u32(0xFF)).astype(np.int64)
    tri = np.where(tri < T, tri, 0)
    base = m["dataOffset"].astype(np.int64)
    tri_word = scene.meshlet_data[base + V + tri]
    vb = scene.primitives["vertexOffset"][scene.objects["GLTFPrimitiveDetail"][o]].astype(np.int64)
    vi = np.stack([scene.meshlet_data[base + ((tri_word >> u32(8 * i)) & u32(0xFF)).astype(np.int64)].astype(np.int64) + vb for i in range(3)], -1)
    return o, vi


def resolve(scene, vis, cmds, view, iv, w, h, names=NAMES, normals=None, tangents=None):
    """{name: (h, w, 4) float32} as chordvis_resolve_surface writes the surface targets.  normals / tangents: the streams the
    device holds (default: the scene's; vertices without them read zeros)."""
    view = np.asarray(view).reshape(-1)[0]
    normals = scene.normals if normals is None else normals
    tangents = scene.tangents if tangents is None else tangents
    if normals is None:
        normals = np.zeros((len(scene.positions), 3), dtype=f32)
    if tangents is None:
        tangents = np.zeros((len(scene.positions), 4), dtype=f32)
    low = (np.asarray(vis, dtype=np.uint64).reshape(-1) & np.uint64(0xFFFFFFFF)).astype(u32)
    slot = ((low >> u32(8)) & u32(SR.MAX_INSTANCE_ID)).astype(np.int64) - 1
    covered = (low != 0) & (slot < len(cmds))
    out = {n: np.zeros((h * w, 4), dtype=f32) for n in names}
    idx = np.nonzero(covered)[0]
    if len(idx):
        keys, inv = np.unique(low[idx], return_inverse=True)
        with np.errstate(all="ignore"):
            S = SR.triangle_setup(scene, cmds, view, iv, keys)
            o, vi = vertex_ids(scene, cmds, keys)
            obj = scene.objects[o]
            n_rs, t_rs, b_rs = vertex_frames(normals[vi], tangents[vi], mat(obj["localToTranslatedWorld"])[:, None],
                                             mat(obj["translatedWorldToLocal"])[:, None])
        frames = {"vertexNormal": n_rs, "tangent": t_rs, "bitangent": b_rs}
        good = S["ok"][inv]
        pix, t = idx[good], inv[good]
        inv_w, inv_h = f32(view["renderDimension"][2]), f32(view["renderDimension"][3])
        x, y = (pix % w).astype(f32), (pix // w).astype(f32)
        su, sv = (x + f32(0.5)) * inv_w, (y + f32(0.5)) * inv_h
        pcx, pcy = f32(2.0) * (su - f32(0.5)), f32(2.0) * (f32(0.5) - sv)
        with np.errstate(all="ignore"):
            b, _, _ = SR.barycentrics(S["phs"][t], pcx, pcy, inv_w, inv_h)
            for n in names:
                out[n][pix, :3] = SR._interp(frames[n][t], b)
    return {n: a.reshape(h, w, 4) for n, a in out.items()}
