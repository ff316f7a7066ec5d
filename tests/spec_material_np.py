"""The material channels of chordvis_resolve_material (include/chordvis.h ChordMaterialTargets) restated in vectorised numpy
float32: loadGLTFMetallicRoughnessPBRMaterial (material.hlsli:66-153) over the pinned sampler of DESIGN.md 2 item 9.  Built on
spec_resolve_np (uv, uvGrad, hit) and spec_surface_np (vertex normal, tangent, bitangent), which it calls.  TEST INFRASTRUCTURE:
never imported by chord_amd/.

The sampler, per texture slot of a pixel (every + - * / sqrt one float32 array operation, no contraction):
  1. footprint  ax = dudx * fW; ay = dvdx * fH; bx = dudy * fW; by = dvdy * fH; rho2 = max(ax*ax + ay*ay, bx*bx + by*by), fW / fH
     the float level-0 size.  Isotropic.
  2. lodq = ((int32)(bits(rho2) >> 15) - (127 << 8)) >> 1 (arithmetic); rho2 not finite, NaN or <= 0: lodq = 0.
  3. lodq <= 0: level 0 with magFilter.  Else minFilter: NEAREST / LINEAR level 0; *_MIPMAP_NEAREST level
     min((lodq + 128) >> 8, mips - 1); *_MIPMAP_LINEAR levels l0 = min(lodq >> 8, mips - 1), l1 = min(l0 + 1, mips - 1),
     f = float(lodq & 255) * (1 / 256), c0 + (c1 - c0) * f (the second level skipped when l1 == l0: the same value).
  4. inside a level per channel: nearest texel_floor(u * fW); bilinear at u * fW - 0.5, top + (bot - top) * fy; CLAMP_TO_EDGE /
     MIRRORED_REPEAT / REPEAT on the integer index; coordinates beyond +-1e9 (or NaN) read index 0 with weight 0.
  5. decode before filtering: byte * (1 / 255), or the sRGB table for rgb of base colour and emissive.
  6. no texture (id >= textureCount): base colour white, emissive 0; normal and metallic-roughness are branched on."""
import json
import os

import numpy as np

import spec_resolve_np as SR
import spec_surface_np as SS

f32 = np.float32
u32 = np.uint32
NAMES = ("baseColor", "emissive", "pixelNormal", "roughMetalAO")
SLOTS = ("baseColor", "emissive", "normal", "metallicRoughness")
_TEX_FIELD = {"baseColor": ("baseColorId", "baseColorSampler"), "emissive": ("emissiveTexture", "emissiveSampler"),
              "normal": ("normalTexture", "normalSampler"), "metallicRoughness": ("metallicRoughnessTexture", "metallicRoughnessSampler")}
NEAREST, LINEAR, NEAREST_MIPMAP_NEAREST, LINEAR_MIPMAP_NEAREST, NEAREST_MIPMAP_LINEAR, LINEAR_MIPMAP_LINEAR = 9728, 9729, 9984, 9985, 9986, 9987
REPEAT, CLAMP_TO_EDGE, MIRRORED_REPEAT = 10497, 33071, 33648
PBR_TYPE = 1                                     # kLightingType_GLTF_MetallicRoughnessPBR, base.h:423

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "material_tables.json")


def tables():
    """(sRGB8 -> linear (256,), sRGB_2_AP1 (3, 3)) float32 from the committed bit patterns"""
    with open(_GOLDEN) as f:
        t = json.load(f)
    return (np.array(t["srgb_to_linear_bits"], dtype=u32).view(f32), np.array(t["srgb_to_ap1_bits"], dtype=u32).view(f32).reshape(3, 3))


def lodq_of(rho2):
    """item 2 on a float32 array"""
    rho2 = np.asarray(rho2, dtype=f32)
    q = ((rho2.view(u32) >> u32(15)).astype(np.int32) - np.int32(127 << 8)) >> np.int32(1)
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(rho2) & (rho2 > f32(0.0)), q, np.int32(0)).astype(np.int32)


def footprint(grad, fw, fh):
    """item 1: grad (N, 4) = du/dx, dv/dx, du/dy, dv/dy -> rho2 (N,)"""
    with np.errstate(all="ignore"):
        ax, ay, bx, by = grad[:, 0] * f32(fw), grad[:, 1] * f32(fh), grad[:, 2] * f32(fw), grad[:, 3] * f32(fh)
        return np.maximum(ax * ax + ay * ay, bx * bx + by * by)


def texel_floor(x):
    with np.errstate(all="ignore"):
        ok = np.abs(x) < f32(1.0e9)
        return np.where(ok, np.floor(np.where(ok, x, f32(0.0))), 0).astype(np.int64), ok


def wrap(i, n, mode, counts=None):
    if counts is not None:
        counts[int(mode)] = counts.get(int(mode), 0) + ((i < 0) | (i >= n))
    if mode == CLAMP_TO_EDGE:
        return np.clip(i, 0, n - 1)
    if mode == MIRRORED_REPEAT:
        m = np.mod(i, 2 * n)
        return np.where(m < n, m, 2 * n - 1 - m)
    return np.mod(i, n)


def decode(words, srgb):
    """(N,) RGBA8 words -> (N, 4) float32; srgb: the table, or None for a linear slot"""
    b = np.stack([(words >> u32(8 * k)) & u32(255) for k in range(4)], axis=-1)
    lin = b.astype(f32) * f32(1.0 / 255.0)
    if srgb is not None:
        lin[:, :3] = srgb[b[:, :3]]
    return lin


def sample_level(level, wrap_s, wrap_t, linear, u, v, srgb, wrapped=None):
    """level: (H, W) uint32 words; linear: bool (N,); u, v float32 (N,) -> (N, 4)"""
    H, W = level.shape
    fw, fh = f32(W), f32(H)
    out = np.zeros((len(u), 4), dtype=f32)
    flat = level.reshape(-1)
    cs = None if wrapped is None else wrapped.setdefault("s", {})
    ct = None if wrapped is None else wrapped.setdefault("t", {})
    with np.errstate(all="ignore"):
        k = np.nonzero(~linear)[0]
        if len(k):
            ix, _ = texel_floor(u[k] * fw)
            iy, _ = texel_floor(v[k] * fh)
            sub = None if cs is None else ({}, {})
            out[k] = decode(flat[wrap(iy, H, wrap_t, None if sub is None else sub[1]) * W + wrap(ix, W, wrap_s, None if sub is None else sub[0])], srgb)
            if sub is not None:
                _note(wrapped, k, sub, wrap_s, wrap_t)
        k = np.nonzero(linear)[0]
        if len(k):
            x, y = u[k] * fw - f32(0.5), v[k] * fh - f32(0.5)
            x0, okx = texel_floor(x)
            y0, oky = texel_floor(y)
            fx = np.where(okx, x - x0.astype(f32), f32(0.0)).astype(f32)[:, None]
            fy = np.where(oky, y - y0.astype(f32), f32(0.0)).astype(f32)[:, None]
            sub = None if cs is None else ({}, {})
            ix0, ix1 = wrap(x0, W, wrap_s, None if sub is None else sub[0]), wrap(x0 + 1, W, wrap_s, None if sub is None else sub[0])
            iy0, iy1 = wrap(y0, H, wrap_t, None if sub is None else sub[1]), wrap(y0 + 1, H, wrap_t, None if sub is None else sub[1])
            a00, a10 = decode(flat[iy0 * W + ix0], srgb), decode(flat[iy0 * W + ix1], srgb)
            a01, a11 = decode(flat[iy1 * W + ix0], srgb), decode(flat[iy1 * W + ix1], srgb)
            top, bot = a00 + (a10 - a00) * fx, a01 + (a11 - a01) * fx
            out[k] = top + (bot - top) * fy
            if sub is not None:
                _note(wrapped, k, sub, wrap_s, wrap_t)
    return out


def _note(wrapped, k, sub, wrap_s, wrap_t):
    """wrapped["px"][mode]: per sampled element, whether an index left [0, n) before wrapping under that mode"""
    px = wrapped["px"]
    for d, mode in ((sub[0], wrap_s), (sub[1], wrap_t)):
        if int(mode) in d:
            px.setdefault(int(mode), np.zeros(wrapped["n"], dtype=bool))[k] |= d[int(mode)].astype(bool)


def levels_of(chain, width, height, mips):
    """ChordTexture::rgba8 (all levels back to back) -> [(H_l, W_l) uint32 words]"""
    words = np.ascontiguousarray(chain, dtype=np.uint8).reshape(-1, 4).copy().view(u32).reshape(-1)
    out, off = [], 0
    for l in range(mips):
        w, h = max(1, width >> l), max(1, height >> l)
        out.append(words[off:off + w * h].reshape(h, w))
        off += w * h
    return out


def sample(levels, sampler, u, v, grad, srgb, stats=None):
    """items 1-5 for one texture: levels from levels_of, sampler = (minFilter, magFilter, wrapS, wrapT) -> (N, 4) float32.
    stats: a dict that receives lodq, l0, l1, f and, under "wrapped", the per-element wrap flags by mode."""
    min_f, mag_f, wrap_s, wrap_t = (int(x) for x in sampler)
    is_lin = lambda f: f in (LINEAR, LINEAR_MIPMAP_NEAREST, LINEAR_MIPMAP_LINEAR)
    H0, W0 = levels[0].shape
    last = len(levels) - 1
    lodq = lodq_of(footprint(grad, W0, H0))
    minified = lodq > 0
    linear = np.where(minified, is_lin(min_f), is_lin(mag_f))
    l0 = np.zeros(len(u), dtype=np.int64)
    l1 = l0.copy()
    if min_f in (NEAREST_MIPMAP_NEAREST, LINEAR_MIPMAP_NEAREST):
        l0 = np.where(minified, np.minimum((lodq.astype(np.int64) + 128) >> 8, last), 0)
        l1 = l0.copy()
    elif min_f in (NEAREST_MIPMAP_LINEAR, LINEAR_MIPMAP_LINEAR):
        l0 = np.where(minified, np.minimum(lodq.astype(np.int64) >> 8, last), 0)
        l1 = np.where(minified, np.minimum(l0 + 1, last), 0)
    f = ((lodq & 255).astype(f32) * f32(1.0 / 256.0))[:, None]
    wrapped = None
    if stats is not None:
        wrapped = {"px": {}, "n": len(u)}
        stats.update(lodq=lodq, l0=l0, l1=l1, f=f[:, 0], last=last, wrapped=wrapped["px"])
    out = np.zeros((len(u), 4), dtype=f32)
    for l in range(len(levels)):
        k = np.nonzero(l0 == l)[0]
        if not len(k):
            continue
        w = None if wrapped is None else {"px": {}, "n": len(k)}
        c0 = sample_level(levels[l], wrap_s, wrap_t, linear[k], u[k], v[k], srgb, w)
        two = l1[k] != l
        if np.any(two):
            kk = k[two]
            w1 = None if wrapped is None else {"px": {}, "n": len(kk)}
            c1 = sample_level(levels[min(l + 1, last)], wrap_s, wrap_t, linear[kk], u[kk], v[kk], srgb, w1)
            c0[two] = c0[two] + (c1 - c0[two]) * f[kk]
            if w1 is not None:
                for mode, flags in w1["px"].items():
                    wrapped["px"].setdefault(mode, np.zeros(len(u), dtype=bool))[kk] |= flags
        out[k] = c0
        if w is not None:
            for mode, flags in w["px"].items():
                wrapped["px"].setdefault(mode, np.zeros(len(u), dtype=bool))[k] |= flags
    return out


def material_of_pixels(scene, vis, cmds):
    """per pixel the material index of the visible triangle's object (-1: empty, or id not below the list's count)"""
    low = (np.asarray(vis, dtype=np.uint64).reshape(-1) & np.uint64(0xFFFFFFFF)).astype(u32)
    slot = ((low >> u32(8)) & u32(SR.MAX_INSTANCE_ID)).astype(np.int64) - 1
    covered = (low != 0) & (slot < len(cmds))
    mat = np.full(len(low), -1, dtype=np.int64)
    o = np.asarray(cmds)["objectId"][slot[covered]].astype(np.int64)
    ok = o < len(scene.objects)
    m = np.full(len(o), -1, dtype=np.int64)
    m[ok] = scene.objects["GLTFMaterialData"][o[ok]]
    mat[covered] = m
    return mat


def slot_texture(scene, material, slot):
    """(levels, sampler) of a material's slot, or (None, sampler) when it names no texture (id >= textureCount)"""
    tf, sf = _TEX_FIELD[slot]
    tid, sid = int(material[tf]), int(material[sf])
    smp = tuple(int(scene.samplers[sid][k]) for k in ("minFilter", "magFilter", "wrapS", "wrapT")) if sid < len(scene.samplers) else (NEAREST, NEAREST, REPEAT, REPEAT)
    if tid >= len(scene.texture_images):
        return None, smp
    chain, mips = scene._tex_chains[tid]
    img = scene.texture_images[tid]
    return levels_of(chain, img.shape[1], img.shape[0], mips), smp


def resolve(scene, vis, cmds, view, iv, w, h, names=NAMES, stats=None, tangents=None, surface=None):
    """{name: (h, w, 4) float32} as chordvis_resolve_material writes the material targets.  stats: a dict that receives, per slot,
    the sampler's statistics of the pixels that sampled it ("pix" their flat indices), plus "pbr" / "hit" / "material" per pixel.
    tangents: the tangent stream the device holds (default: the scene's).  surface: precomputed spec_surface_np images."""
    srgb, ap1 = tables()
    A = SR.resolve(scene, vis, cmds, view, iv, w, h, names=("uv", "uvGrad"), extras=True)
    hit = A["hit"].reshape(-1)
    uv, grad = A["uv"].reshape(-1, 2), A["uvGrad"].reshape(-1, 4)
    S = surface if surface is not None else SS.resolve(scene, vis, cmds, view, iv, w, h, tangents=tangents)
    N, T, B = (S[n].reshape(-1, 4)[:, :3] for n in SS.NAMES)
    mat = material_of_pixels(scene, vis, cmds)
    mat = np.where(hit, mat, -1)
    out = {n: np.zeros((h * w, 4), dtype=f32) for n in names}
    if stats is not None:
        stats.update(hit=hit, material=mat, pbr=np.zeros(h * w, dtype=bool), slots={s: [] for s in SLOTS})
    for m in np.unique(mat[mat >= 0]):
        M = scene.materials[m]
        if int(M["materialType"]) != PBR_TYPE:
            continue
        pix = np.nonzero(mat == m)[0]
        if stats is not None:
            stats["pbr"][pix] = True
        u, v, g = uv[pix, 0], uv[pix, 1], grad[pix]

        def tex(slot, is_srgb):
            levels, smp = slot_texture(scene, M, slot)
            if levels is None:
                return None
            st = None if stats is None else {"pix": pix, "material": int(m)}
            c = sample(levels, smp, u, v, g, srgb if is_srgb else None, st)
            if st is not None:
                stats["slots"][slot].append(st)
            return c
        with np.errstate(all="ignore"):
            if "baseColor" in out:
                c = tex("baseColor", True)
                if c is None:
                    c = np.ones((len(pix), 4), dtype=f32)
                c = c * np.asarray(M["baseColorFactor"], dtype=f32)[None, :]
                r, gg, b = c[:, 0], c[:, 1], c[:, 2]
                out["baseColor"][pix] = np.stack([(ap1[i, 0] * r + ap1[i, 1] * gg) + ap1[i, 2] * b for i in range(3)] + [c[:, 3]], axis=-1)
            if "emissive" in out:
                c = tex("emissive", True)
                if c is None:
                    c = np.zeros((len(pix), 4), dtype=f32)
                out["emissive"][pix, :3] = c[:, :3] * np.asarray(M["emissiveFactor"], dtype=f32)[None, :]
            if "pixelNormal" in out:
                c = tex("normal", False)
                if c is None:
                    out["pixelNormal"][pix, :3] = N[pix]
                else:
                    tx, ty = c[:, 0] * f32(2.0) - f32(1.0), c[:, 1] * f32(2.0) - f32(1.0)
                    tz = np.sqrt(np.maximum(f32(0.0), f32(1.0) - (tx * tx + ty * ty)))
                    sc = f32(M["normalFactorScale"])
                    n = SS.normalize(np.stack([tx * sc, ty * sc, tz], axis=-1))
                    t_, b_, n_ = T[pix], B[pix], N[pix]
                    out["pixelNormal"][pix, :3] = (n[:, 0:1] * t_ + n[:, 1:2] * b_) + n[:, 2:3] * n_
            if "roughMetalAO" in out:
                c = tex("metallicRoughness", False)
                if c is None:
                    mf = f32(M["metallicFactor"])
                    out["roughMetalAO"][pix, :3] = np.array([f32(M["roughnessFactor"]), f32(0.0) if mf >= f32(1.0) else mf, f32(1.0)], dtype=f32)
                else:
                    ao = f32(M["occlusionTextureStrength"]) * c[:, 0] if int(M["bExistOcclusion"]) else np.ones(len(pix), dtype=f32)
                    out["roughMetalAO"][pix, :3] = np.stack([c[:, 1], c[:, 2], ao], axis=-1)
    return {n: a.reshape(h, w, 4) for n, a in out.items()}
