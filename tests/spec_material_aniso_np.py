"""chordvis_resolve_material under chordvis_set_material_anisotropy restated in vectorised numpy float32, on
top of spec_material_np, whose helpers (lodq_of, sample_level, levels_of, slot_texture, tables, material_of_pixels) and whose
composition per material it reuses unchanged.  TEST INFRASTRUCTURE: never imported by chord_amd/.

The sampler, per texture slot of a pixel, N = max_aniso in {1, 2, 4, 8, 16}, kmax = log2 N (every + - * one float32 array operation):
  1. ax = dudx * fW; ay = dvdx * fH; bx = dudy * fW; by = dvdy * fH; ra = ax*ax + ay*ay; rb = bx*bx + by*by (spec_material_np's).
  2. rmaj2 = max(ra, rb), rmin2 = min(ra, rb); the major axis is x (dudx, dvdx) when ra >= rb, else y (dudy, dvdy).
  3. lmaj = lodq_of(rmaj2), lmin = lodq_of(rmin2).
  4. k = 0 when ra or rb is not finite, rmaj2 is not above 0 (lmaj = 0 then), or lmaj <= 0.  Else
     k = min(kmax, (max(lmaj - lmin, 0) + 255) >> 8, (lmaj + 255) >> 8), the middle term kmax when rmin2 is not above 0.
  5. lodq' = max(lmaj - (k << 8), 0) chooses the level(s), f and the clamps as spec_material_np's item 3 does with lodq; the choice
     between minFilter and magFilter asks lmaj > 0.
  6. n = 1 << k taps, t_i = float(2i + 1 - n) * (1 / (2n)), u_i = u + dmaj_u * t_i, v_i = v + dmaj_v * t_i; each tap is items 3-5 of
     spec_material_np at (u_i, v_i); d = 0, d = d + (c_i - c_0) for i = 1 .. n - 1 in index order, result c_0 + d * (1 / n) (the mean
     about the first tap: equal taps give c_0 exactly).  k = 0: one tap at (u, v), no offset formed, c_0 as it is."""
import numpy as np

import spec_material_np as SM

f32 = np.float32
u32 = np.uint32
NAMES = SM.NAMES
ALLOWED = (1, 2, 4, 8, 16)


def axes(grad, fw, fh):
    """items 1-2: grad (N, 4) -> (ra, rb) float32"""
    with np.errstate(all="ignore"):
        ax, ay, bx, by = grad[:, 0] * f32(fw), grad[:, 1] * f32(fh), grad[:, 2] * f32(fw), grad[:, 3] * f32(fh)
        return ax * ax + ay * ay, bx * bx + by * by


def tap_plan(grad, fw, fh, max_aniso):
    """items 1-5 up to the level: dict of per-element k, lodq (= lodq'), lmaj, lmin, major_x (bool)"""
    assert max_aniso in ALLOWED, max_aniso
    kmax = ALLOWED.index(max_aniso)
    ra, rb = axes(np.asarray(grad, dtype=f32), fw, fh)
    with np.errstate(all="ignore"):
        finite = (ra < f32(np.inf)) & (rb < f32(np.inf))
        major_x = ra >= rb
        rmaj2 = np.where(finite, np.where(major_x, ra, rb), f32(0.0)).astype(f32)
        rmin2 = np.where(finite, np.where(major_x, rb, ra), f32(0.0)).astype(f32)
        valid = finite & (rmaj2 > f32(0.0))
        lmaj = np.where(valid, SM.lodq_of(rmaj2), 0).astype(np.int64)
        lmin = SM.lodq_of(rmin2).astype(np.int64)
        spread = np.where(rmin2 > f32(0.0), (np.maximum(lmaj - lmin, 0) + 255) >> 8, kmax)
    k = np.minimum(np.minimum(kmax, spread), (lmaj + 255) >> 8)
    k = np.where(valid & (lmaj > 0), k, 0).astype(np.int64)
    lodq = np.maximum(lmaj - (k << 8), 0)
    return dict(k=k, lodq=lodq.astype(np.int32), lmaj=lmaj.astype(np.int32), lmin=lmin.astype(np.int32), major_x=major_x & finite)


def _levels_at(levels, wrap_s, wrap_t, linear, l0, l1, f, u, v, srgb, wrapped):
    """spec_material_np.sample's loop over levels at given (l0, l1, f): the per-level pipeline and the two-level lerp"""
    last = len(levels) - 1
    out = np.zeros((len(u), 4), dtype=f32)
    for l in range(len(levels)):
        idx = np.nonzero(l0 == l)[0]
        if not len(idx):
            continue
        w = None if wrapped is None else {"px": {}, "n": len(idx)}
        c0 = SM.sample_level(levels[l], wrap_s, wrap_t, linear[idx], u[idx], v[idx], srgb, w)
        two = l1[idx] != l
        if np.any(two):
            kk = idx[two]
            w1 = None if wrapped is None else {"px": {}, "n": len(kk)}
            c1 = SM.sample_level(levels[min(l + 1, last)], wrap_s, wrap_t, linear[kk], u[kk], v[kk], srgb, w1)
            with np.errstate(all="ignore"):
                c0[two] = c0[two] + (c1 - c0[two]) * f[kk]
            if w1 is not None:
                for mode, flags in w1["px"].items():
                    wrapped.setdefault(mode, np.zeros(len(u), dtype=bool))[kk] |= flags
        out[idx] = c0
        if w is not None:
            for mode, flags in w["px"].items():
                wrapped.setdefault(mode, np.zeros(len(u), dtype=bool))[idx] |= flags
    return out


def sample(levels, sampler, u, v, grad, srgb, max_aniso, stats=None):
    """One texture: levels from SM.levels_of, sampler = (minFilter, magFilter, wrapS, wrapT) -> (N, 4) float32.
    stats: a dict that receives spec_material_np's entries (lodq is lodq') and k, lmaj, lmin, major_x, taps."""
    min_f, mag_f, wrap_s, wrap_t = (int(x) for x in sampler)
    is_lin = lambda flt: flt in (SM.LINEAR, SM.LINEAR_MIPMAP_NEAREST, SM.LINEAR_MIPMAP_LINEAR)
    u, v, grad = np.asarray(u, dtype=f32), np.asarray(v, dtype=f32), np.asarray(grad, dtype=f32)
    H0, W0 = levels[0].shape
    last = len(levels) - 1
    plan = tap_plan(grad, W0, H0, max_aniso)
    k, lodq = plan["k"], plan["lodq"].astype(np.int64)
    minified = plan["lmaj"] > 0
    linear = np.where(minified, is_lin(min_f), is_lin(mag_f))
    l0 = np.zeros(len(u), dtype=np.int64)
    l1 = l0.copy()
    if min_f in (SM.NEAREST_MIPMAP_NEAREST, SM.LINEAR_MIPMAP_NEAREST):
        l0 = np.where(minified, np.minimum((lodq + 128) >> 8, last), 0)
        l1 = l0.copy()
    elif min_f in (SM.NEAREST_MIPMAP_LINEAR, SM.LINEAR_MIPMAP_LINEAR):
        l0 = np.where(minified, np.minimum(lodq >> 8, last), 0)
        l1 = np.where(minified, np.minimum(l0 + 1, last), 0)
    f = ((lodq & 255).astype(f32) * f32(1.0 / 256.0))[:, None]
    wrapped = None
    if stats is not None:
        wrapped = {}
        stats.update(plan, l0=l0, l1=l1, f=f[:, 0], last=last, wrapped=wrapped, taps=np.int64(1) << k)
    out = np.zeros((len(u), 4), dtype=f32)
    for kv in np.unique(k):
        idx = np.nonzero(k == kv)[0]
        sub = None if wrapped is None else {}
        args = (levels, wrap_s, wrap_t, linear[idx], l0[idx], l1[idx], f[idx])
        if kv == 0:
            acc = _levels_at(*args, u[idx], v[idx], srgb, sub)
        else:
            n = 1 << int(kv)
            mx = plan["major_x"][idx]
            du, dv = np.where(mx, grad[idx, 0], grad[idx, 2]).astype(f32), np.where(mx, grad[idx, 1], grad[idx, 3]).astype(f32)
            c0, d = None, np.zeros((len(idx), 4), dtype=f32)
            with np.errstate(all="ignore"):
                for i in range(n):
                    t = f32(2 * i + 1 - n) * f32(1.0 / (2 * n))
                    c = _levels_at(*args, u[idx] + du * t, v[idx] + dv * t, srgb, sub)
                    if i == 0:
                        c0 = c
                    else:
                        d = d + (c - c0)
                acc = c0 + d * f32(1.0 / n)
        out[idx] = acc
        if sub is not None:
            for mode, flags in sub.items():
                wrapped.setdefault(mode, np.zeros(len(u), dtype=bool))[idx] |= flags
    return out


def resolve(scene, vis, cmds, view, iv, w, h, names=NAMES, stats=None, tangents=None, surface=None, max_aniso=1):
    """spec_material_np.resolve with every slot sampled by `sample` at max_aniso: the same composition per material, run with that
    module's sampler swapped for the duration of the call (its file stays as it is)."""
    assert max_aniso in ALLOWED, max_aniso
    keep = SM.sample
    SM.sample = lambda levels, smp, u, v, g, srgb, st=None: sample(levels, smp, u, v, g, srgb, max_aniso, st)
    try:
        return SM.resolve(scene, vis, cmds, view, iv, w, h, names=names, stats=stats, tangents=tangents, surface=surface)
    finally:
        SM.sample = keep
