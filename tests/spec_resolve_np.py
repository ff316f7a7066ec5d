"""The per-pixel attribute resolve (include/chordvis.h chordvis_resolve_attributes) restated in vectorised numpy float32:
lighting.hlsl:278-371 / nanite_shared.hlsli:111-179 (getTriangleMiscInfo), base.hlsli:457-495 (calculateTriangleBarycentrics),
material.hlsli:41-64 (uv, uv gradients, positionRS, motion) and nanite_debug.hlsl:30-43,104-130 (debug colours).  TEST
INFRASTRUCTURE: never imported by chord_amd/.

The triangle set-up is done once per distinct low word (slot | triangle) and gathered per pixel; every + - * / is a float32
array operation in the order the HLSL writes it (numpy rounds each one separately, no contraction), so the result is the
kernel's bit for bit.  Scenes are records.Scene (one asset): a command's meshletId indexes scene.meshlets directly.

Two numberings of a meshlet: `cmds` here are always in the CONCATENATED one (an index into scene.meshlets), which for one asset is
also the asset-relative one of ChordDrawCmd::meshletId.  For a scene of several assets -- `scene` is then the one-asset twin of
tests/multi_asset.py and the caller has put the read-back list through to_concatenated -- asset_meshlet_base[primitive] is the first
meshlet of the primitive's asset: the meshlet debug views hash meshletId - base, the reference's asset-relative cmd.y
(kernels_resolve.hip); nothing else reads the base."""
import numpy as np

from spec_np import mat, mul_mm, mul_mv

f32 = np.float32
u32 = np.uint32
MAX_INSTANCE_ID = 0xFFFFFF
NAMES = ("barycentrics", "baryDdx", "baryDdy", "uv", "uvGrad", "positionRS", "motionVector", "debugRGBA8")
CHANNELS = {"barycentrics": 4, "baryDdx": 4, "baryDdy": 4, "uv": 2, "uvGrad": 4, "positionRS": 4, "motionVector": 2, "debugRGBA8": 1}
# kLODDebugColor, nanite_debug.hlsl:30-43
LOD_PALETTE = np.array([[1.0, 0.0, 0.0], [0.7, 0.3, 0.0], [0.4, 0.6, 0.0], [0.1, 0.9, 0.0], [0.0, 1.0, 0.2], [0.0, 0.5, 0.6],
                        [0.0, 0.1, 0.8], [0.0, 0.0, 1.0], [0.1, 0.1, 0.8], [0.2, 0.2, 0.6], [0.0, 0.4, 0.7], [0.2, 0.6, 0.3]], dtype=f32)
EMPTY_RGBA8 = 0xFF000000


def simple_hash(a):
    """base.hlsli:112-121 on uint32 arrays"""
    a = np.asarray(a, dtype=u32)
    a = (a + u32(0x7ed55d16)) + (a << u32(12))
    a = (a ^ u32(0xc761c23c)) ^ (a >> u32(19))
    a = (a + u32(0x165667b1)) + (a << u32(5))
    a = (a + u32(0xd3a2646c)) ^ (a << u32(9))
    a = (a + u32(0xfd7046c5)) + (a << u32(3))
    a = (a ^ u32(0xb55a4f09)) ^ (a >> u32(16))
    return a


def simple_hash_color(i):
    h = simple_hash(i)
    return np.stack([(h & u32(255)).astype(f32) / f32(255.0), ((h >> u32(8)) & u32(255)).astype(f32) / f32(255.0),
                     ((h >> u32(16)) & u32(255)).astype(f32) / f32(255.0)], axis=-1)


def pack_rgba8(c):
    """(uint)(saturate(c) * 255 + 0.5) per channel, alpha 255 (saturate = fmin(fmax(c, 0), 1): NaN -> 0, as on the device)"""
    q = (np.fmin(np.fmax(c, f32(0.0)), f32(1.0)) * f32(255.0) + f32(0.5)).astype(u32)
    return q[..., 0] | (q[..., 1] << u32(8)) | (q[..., 2] << u32(16)) | u32(EMPTY_RGBA8)


def _interp(a, b):
    """(a0 * b.x + a1 * b.y) + a2 * b.z per component: a (..., 3, k), b (..., 3) -> (..., k)"""
    return (a[..., 0, :] * b[..., 0:1] + a[..., 1, :] * b[..., 1:2]) + a[..., 2, :] * b[..., 2:3]


def triangle_setup(scene, cmds, view, iv, lows, use_no_jitter=False, vp_nj=None, vp_last_nj=None, asset_meshlet_base=None):
    """Per distinct low word: validity, the vertices' clip / translated-world / motion positions, uvs and the debug ids.
    asset_meshlet_base: per primitive, what the meshlet debug id subtracts (None: 0, one asset)."""
    lows = np.asarray(lows, dtype=u32)
    slot = ((lows >> u32(8)) & u32(MAX_INSTANCE_ID)).astype(np.int64) - 1
    tri = (lows & u32(0xFF)).astype(np.int64)
    cmd = np.asarray(cmds)[slot]
    o = cmd["objectId"].astype(np.int64)
    mid = cmd["meshletId"].astype(np.int64)
    ok = (o < len(scene.objects)) & (mid < len(scene.meshlets))
    o = np.where(ok, o, 0); mid = np.where(ok, mid, 0)
    m = scene.meshlets[mid]
    V = (m["vertexTriangleCount"] & u32(0xFF)).astype(np.int64)
    T = ((m["vertexTriangleCount"] >> u32(8)) & u32(0xFF)).astype(np.int64)
    ok &= tri < T
    tri = np.where(ok, tri, 0)
    base = m["dataOffset"].astype(np.int64)
    tri_word = scene.meshlet_data[base + V + tri]
    vb = scene.primitives["vertexOffset"][scene.objects["GLTFPrimitiveDetail"][o]].astype(np.int64)
    vi = np.stack([scene.meshlet_data[base + ((tri_word >> u32(8 * i)) & u32(0xFF)).astype(np.int64)].astype(np.int64) + vb for i in range(3)], -1)
    pos = scene.positions[vi]                                                    # (N, 3 vertices, 3)
    uv = scene.texcoord0[vi] if scene.texcoord0 is not None else np.zeros(vi.shape + (2,), dtype=f32)
    obj = scene.objects[o]
    M = mat(obj["localToTranslatedWorld"])
    Ml = mat(obj["localToTranslatedWorldLastFrame"])
    mvp = mul_mm(mat(np.asarray(iv["translatedWorldToClip"]).reshape(16))[None], M)
    if use_no_jitter:
        m_cur = mul_mm(mat(np.asarray(vp_nj, dtype=f32).reshape(16))[None], M)
        m_last = mul_mm(mat(np.asarray(vp_last_nj, dtype=f32).reshape(16))[None], Ml)
    else:
        m_cur = mvp
        m_last = mul_mm(mat(np.asarray(view["translatedWorldToClipLastFrame"]).reshape(16))[None], Ml)
    px, py, pz = pos[..., 0], pos[..., 1], pos[..., 2]
    per_vertex = lambda Mx: mul_mv(Mx[:, None], px, py, pz)                    # (N, 3, 4)
    cur, last = per_vertex(m_cur), per_vertex(m_last)
    hash_id = mid
    if asset_meshlet_base is not None:
        hash_id = mid - np.asarray(asset_meshlet_base, dtype=np.int64)[scene.objects["GLTFPrimitiveDetail"][o].astype(np.int64)]
    return dict(ok=ok, phs=per_vertex(mvp), prs=per_vertex(M)[..., :3], cur=cur[..., [0, 1, 3]], last=last[..., [0, 1, 3]], uv=uv,
                meshlet=(hash_id & 0xFFFFFFFF).astype(u32), tri_word=tri_word.astype(u32), lod=np.minimum(m["lod"], 11).astype(np.int64))


def barycentrics(phs, pcx, pcy, inv_w, inv_h):
    """calculateTriangleBarycentrics (base.hlsli:457-495): phs (N, 3, 4) clip positions, pixel clip (N,) -> (interp, ddx, ddy)"""
    rcp_w = f32(1.0) / phs[..., 3]                                               # (N, 3)
    pos_x, pos_y = phs[..., 0] * rcp_w, phs[..., 1] * rcp_w
    p120x, p120y = pos_x[:, [1, 2, 0]], pos_y[:, [1, 2, 0]]
    p201x, p201y = pos_x[:, [2, 0, 1]], pos_y[:, [2, 0, 1]]
    cdx = p201y - p120y
    cdy = p120x - p201x
    C = cdx * (pcx[:, None] - p120x) + cdy * (pcy[:, None] - p120y)
    G = C * rcp_w
    H = (C[:, 0] * rcp_w[:, 0] + C[:, 1] * rcp_w[:, 1]) + C[:, 2] * rcp_w[:, 2]
    rcp_h = f32(1.0) / H
    interp = G * rcp_h[:, None]
    gdx, gdy = cdx * rcp_w, cdy * rcp_w
    hdx = (cdx[:, 0] * rcp_w[:, 0] + cdx[:, 1] * rcp_w[:, 1]) + cdx[:, 2] * rcp_w[:, 2]
    hdy = (cdy[:, 0] * rcp_w[:, 0] + cdy[:, 1] * rcp_w[:, 1]) + cdy[:, 2] * rcp_w[:, 2]
    rh2 = (rcp_h * rcp_h)[:, None]
    ddx = ((gdx * H[:, None] - G * hdx[:, None]) * rh2) * (f32(2.0) * inv_w)
    ddy = ((gdy * H[:, None] - G * hdy[:, None]) * rh2) * (f32(-2.0) * inv_h)
    return interp, ddx, ddy


def resolve(scene, vis, cmds, view, iv, w, h, names=NAMES, use_no_jitter=False, vp_nj=None, vp_last_nj=None, debug_mode=0,
            chunk=1 << 20, extras=False, asset_meshlet_base=None):
    """{name: array} as chordvis_resolve_attributes writes it: (h, w, channels) float32, (h, w) uint32 for debugRGBA8.
    extras=True adds "hit" (h, w) bool and "phs" (h, w, 3, 4): the clip position interpolated with the barycentrics, with ddx and
    with ddy (what the tests check the raster against)."""
    view = np.asarray(view).reshape(-1)[0]
    iv = np.asarray(iv).reshape(-1)[0]
    low = (np.asarray(vis, dtype=np.uint64).reshape(-1) & np.uint64(0xFFFFFFFF)).astype(u32)
    slot = ((low >> u32(8)) & u32(MAX_INSTANCE_ID)).astype(np.int64) - 1
    covered = (low != 0) & (slot < len(cmds))
    out = {n: np.zeros((h * w, CHANNELS[n]), dtype=u32 if n == "debugRGBA8" else f32) for n in names}
    if "debugRGBA8" in out:
        out["debugRGBA8"][:] = EMPTY_RGBA8
    hit = np.zeros(h * w, dtype=bool)
    phs_out = np.zeros((h * w, 3, 4), dtype=f32) if extras else None
    idx = np.nonzero(covered)[0]
    if len(idx):
        keys, inv = np.unique(low[idx], return_inverse=True)
        with np.errstate(all="ignore"):
            S = triangle_setup(scene, cmds, view, iv, keys, use_no_jitter, vp_nj, vp_last_nj, asset_meshlet_base)
        inv_w, inv_h = f32(view["renderDimension"][2]), f32(view["renderDimension"][3])
        for c0 in range(0, len(idx), chunk):
            pix, t = idx[c0:c0 + chunk], inv[c0:c0 + chunk]
            good = S["ok"][t]
            pix, t = pix[good], t[good]
            hit[pix] = True
            x, y = (pix % w).astype(f32), (pix // w).astype(f32)
            su, sv = (x + f32(0.5)) * inv_w, (y + f32(0.5)) * inv_h
            pcx, pcy = f32(2.0) * (su - f32(0.5)), f32(2.0) * (f32(0.5) - sv)
            with np.errstate(all="ignore"):
                b, ddx, ddy = barycentrics(S["phs"][t], pcx, pcy, inv_w, inv_h)
                zero = np.zeros((len(pix), 1), dtype=f32)
                if "barycentrics" in out: out["barycentrics"][pix] = np.concatenate([b, zero], 1)
                if "baryDdx" in out: out["baryDdx"][pix] = np.concatenate([ddx, zero], 1)
                if "baryDdy" in out: out["baryDdy"][pix] = np.concatenate([ddy, zero], 1)
                uv = S["uv"][t]
                if "uv" in out: out["uv"][pix] = _interp(uv, b)
                if "uvGrad" in out: out["uvGrad"][pix] = np.concatenate([_interp(uv, ddx), _interp(uv, ddy)], 1)
                if "positionRS" in out: out["positionRS"][pix] = np.concatenate([_interp(S["prs"][t], b), zero + f32(1.0)], 1)
                if "motionVector" in out:
                    c, l = _interp(S["cur"][t], b), _interp(S["last"][t], b)
                    mx = (l[:, 0] / l[:, 2] - c[:, 0] / c[:, 2]) * f32(0.5)
                    my = (l[:, 1] / l[:, 2] - c[:, 1] / c[:, 2]) * f32(-0.5)
                    out["motionVector"][pix] = np.stack([mx, my], 1)
                if "debugRGBA8" in out:
                    lod_c = LOD_PALETTE[S["lod"][t]]
                    if debug_mode == 0: col = simple_hash_color(S["meshlet"][t])
                    elif debug_mode == 1: col = simple_hash_color(S["tri_word"][t])
                    elif debug_mode == 2: col = lod_c
                    elif debug_mode == 3: col = np.power(simple_hash_color(S["meshlet"][t]), f32(0.5)) * lod_c
                    else: col = b
                    out["debugRGBA8"][pix, 0] = pack_rgba8(col)
                if extras:
                    phs_out[pix, 0] = _interp(S["phs"][t], b)
                    phs_out[pix, 1] = _interp(S["phs"][t], ddx)
                    phs_out[pix, 2] = _interp(S["phs"][t], ddy)
    res = {n: (a.reshape(h, w) if n == "debugRGBA8" else a.reshape(h, w, CHANNELS[n])) for n, a in out.items()}
    if extras:
        res["hit"] = hit.reshape(h, w)
        res["phs"] = phs_out.reshape(h, w, 3, 4)
    return res
