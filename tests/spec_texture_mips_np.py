"""numpy restatement of the mip chains the library makes on the GPU at upload (chordvis_set_texture_mips).

Level l+1 from level l (sw x sh texels): max(1, sw >> 1) x max(1, sh >> 1) texels; texel (x, y) reads columns min(2x, sw-1) and
min(2x+1, sw-1), rows likewise (the clamp acts only where a dimension is 1; an odd dimension drops its last row / column).

  code channels (alpha always; r, g, b without SRGB): (sum of the four codes + 2) >> 2.
  r, g, b with SRGB: T = the library's 256-entry float32 sRGB8 -> linear table; v = ((t00 + t10) + (t01 + t11)) * 0.25f in
      float32 in that order; the code is the number of k in 1..255 with mid[k] <= v, mid[k] = (T[k-1] + T[k]) * 0.5f in float32.
  COVERAGE (alpha only, after the whole unscaled box chain exists; every generated level on its own): N0, P0 = texels of level 0
      as supplied and how many of them have a >= cutoff; for a level of N texels cnt(t) = texels with a >= t; t* = the largest
      t in 1..255 with cnt(t) * N0 >= P0 * N (1 if none); tlo = the smallest t with cnt(t) == cnt(t*); t' = clamp(cutoff, tlo,
      t*); a' = min(255, a * cutoff // t').  Supplied levels are never rescaled.
"""
import json
import os

import numpy as np

SRGB, COVERAGE, FULL = 1, 2, 0xFFFFFFFF

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "material_tables.json")
T = np.array(json.load(open(_GOLDEN))["srgb_to_linear_bits"], dtype=np.uint32).view(np.float32)
MID = np.zeros(256, dtype=np.float32)
MID[1:] = (T[:-1] + T[1:]) * np.float32(0.5)


def full_levels(width, height):
    return max(width, height).bit_length()


def level_count(width, height, mips, levels):
    """L: the levels a texture supplied with `mips` levels ends up with under ChordTextureMips::levels."""
    return mips if levels == 0 else max(mips, min(levels, full_levels(width, height)))


def next_level(img, flags=0):
    """(sh, sw, C) uint8 -> the next level (C = 4: RGBA; any C without SRGB)."""
    sh, sw = img.shape[:2]
    dh, dw = max(1, sh >> 1), max(1, sw >> 1)
    x0, x1 = np.minimum(2 * np.arange(dw), sw - 1), np.minimum(2 * np.arange(dw) + 1, sw - 1)
    y0, y1 = np.minimum(2 * np.arange(dh), sh - 1), np.minimum(2 * np.arange(dh) + 1, sh - 1)
    t00, t10, t01, t11 = img[y0][:, x0], img[y0][:, x1], img[y1][:, x0], img[y1][:, x1]
    out = ((t00.astype(np.uint32) + t10 + t01 + t11 + 2) >> 2).astype(np.uint8)
    if flags & SRGB:
        f = lambda t: T[t[..., :3]]
        v = ((f(t00) + f(t10)) + (f(t01) + f(t11))) * np.float32(0.25)
        assert v.dtype == np.float32
        out[..., :3] = np.searchsorted(MID[1:], v, "right")
    return out


def counts(alpha):
    """cnt[t] = texels with a >= t, t = 0..255 (Python-sized integers)."""
    hist = np.bincount(np.asarray(alpha, dtype=np.uint8).reshape(-1), minlength=256).astype(np.int64)
    return hist[::-1].cumsum()[::-1]


def coverage_threshold(alpha, n0, p0, cutoff):
    """t' of one generated level."""
    cnt = counts(alpha)
    n = int(np.asarray(alpha).size)
    ok = [t for t in range(1, 256) if int(cnt[t]) * n0 >= p0 * n]
    ts = max(ok) if ok else 1
    tlo = min(t for t in range(1, 256) if cnt[t] == cnt[ts])
    return min(max(cutoff, tlo), ts)


def rescale_alpha(alpha, cutoff, tp):
    return np.minimum(255, np.asarray(alpha).astype(np.uint32) * cutoff // tp).astype(np.uint8)


def build_chain(supplied, levels, flags=0, cutoff=0, thresholds=None):
    """supplied: the (h, w, 4) uint8 levels the host hands over, level 0 first.  Returns the L levels the upload stores.
    thresholds: a list that receives (level, t') of every generated level under COVERAGE."""
    h, w = supplied[0].shape[:2]
    out = [np.ascontiguousarray(l, dtype=np.uint8) for l in supplied]
    total = level_count(w, h, len(out), levels)
    while len(out) < total:
        out.append(next_level(out[-1], flags))
    if flags & COVERAGE:
        a0 = out[0][..., 3]
        n0, p0 = int(a0.size), int((a0 >= cutoff).sum())
        for l in range(len(supplied), total):
            tp = coverage_threshold(out[l][..., 3], n0, p0, cutoff)
            if thresholds is not None:
                thresholds.append((l, tp))
            out[l] = out[l].copy()
            out[l][..., 3] = rescale_alpha(out[l][..., 3], cutoff, tp)
    return out


def chain_bytes(levels):
    """The levels back to back as ChordTexture::rgba8 holds them."""
    return np.concatenate([l.reshape(-1) for l in levels])


def split_chain(data, width, height, mips):
    """The (h, w, 4) levels of an RGBA8 chain."""
    out, off = [], 0
    for l in range(mips):
        w, h = max(1, width >> l), max(1, height >> l)
        out.append(np.asarray(data[off:off + w * h * 4], dtype=np.uint8).reshape(h, w, 4))
        off += w * h * 4
    return out
