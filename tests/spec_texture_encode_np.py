"""numpy restatement of the block compression the library runs on the GPU at upload (chordvis_set_texture_compress; DESIGN.md 2
item 9(j)): what texture_encode_kernel writes for CHORD_TEXFMT_BC1_RGB / BC3 / BC4 / BC5.  The definition is that of the reference's
importer (stb_dxt at HIGHQUAL: two refinement rounds), float parts pinned: every float32 multiply, add and divide is rounded on its own
(numpy's float32 arithmetic does exactly that), nothing is fused.

    encode_blocks(blocks, format)       (n, 16, 4) uint8 RGBA texels, texel 4 * y + x  ->  (n, block bytes) uint8
    fill_blocks(img)                    (h, w, 4) level -> its ceil(w / 4) x ceil(h / 4) blocks, row-major: texel (x, y) of block
                                        (bx, by) is the level's texel ((4 bx + x) mod w, (4 by + y) mod h)
    encode_level(img, format)           the level's block bytes (flat uint8)
    encode_chain(levels, format)        the levels' block bytes back to back, as ChordTexture holds a chain

The four tables are derived here, not pasted:
    OMATCH5 / OMATCH6 [target] = (max code, min code): scanning mn, then mx, over the codes in ascending order, the first pair that
        minimises 100 |lerp13(e(mx), e(mn)) - target| + 3 |e(mx) - e(mn)|, lerp13(a, b) = (2 a + b) // 3, e5(c) = (33 c) >> 2,
        e6(c) = (65 c) >> 4.
    MID5 / MID6 [q] = the float32 nearest to (e(q) + e(q + 1)) / 510 rounded to six decimals; the last entry is 1.0.
"""
import numpy as np

RGBA8, BC1_RGB, BC3, BC4, BC5 = 0, 1, 2, 3, 4
BLOCK_BYTES = {BC1_RGB: 8, BC3: 16, BC4: 8, BC5: 16}

f32 = np.float32


def _expand5(c):
    return (c * 33) >> 2


def _expand6(c):
    return (c * 65) >> 4


def _omatch(size, expand):
    e = expand(np.arange(size, dtype=np.int64))
    mine, maxe = e[:, None], e[None, :]                                          # [mn, mx]
    lerp = (2 * maxe + mine) // 3
    err = np.abs(lerp[None] - np.arange(256)[:, None, None]) * 100 + np.abs(maxe - mine)[None] * 3
    first = err.reshape(256, -1).argmin(axis=1)                                  # (the first minimum in scan order: mn major)
    return np.stack([first % size, first // size], axis=1)                       # (max code, min code)


def _midpoints(size, expand):
    e = expand(np.arange(size, dtype=np.int64))
    out = np.ones(size, dtype=np.float32)
    for q in range(size - 1):
        out[q] = np.float32("%.6f" % ((int(e[q]) + int(e[q + 1])) / 510.0))
    return out


OMATCH5, OMATCH6 = _omatch(32, _expand5), _omatch(64, _expand6)
MID5, MID6 = _midpoints(32, _expand5), _midpoints(64, _expand6)


# ---- channel blocks: BC4 from .r, BC5 from .r and .g, the alpha of BC3 -----------------------------------------------------------

def encode_channel(v):
    """(n, 16) values -> (n, 8) bytes: [max, min, 48 index bits]."""
    v = np.asarray(v).astype(np.int64)
    mx, mn = v.max(axis=1), v.min(axis=1)
    dist = mx - mn
    dist4, dist2 = dist * 4, dist * 2
    bias = np.where(dist < 8, dist - 1, dist // 2 + 2) - mn * 7
    a = v * 7 + bias[:, None]
    t = a >= dist4[:, None]
    ind = np.where(t, 4, 0)
    a = a - np.where(t, dist4[:, None], 0)
    t = a >= dist2[:, None]
    ind = ind + np.where(t, 2, 0)
    a = a - np.where(t, dist2[:, None], 0)
    ind = ind + (a >= dist[:, None])
    ind = (-ind) & 7
    ind = ind ^ (2 > ind)
    bits = np.zeros(len(v), dtype=np.uint64)
    for i in range(16):
        bits |= ind[:, i].astype(np.uint64) << np.uint64(3 * i)
    out = np.zeros((len(v), 8), dtype=np.uint8)
    out[:, 0], out[:, 1] = mx, mn
    for j in range(6):
        out[:, 2 + j] = (bits >> np.uint64(8 * j)) & np.uint64(0xFF)
    return out


# ---- colour blocks: BC1_RGB, and BC3 after the alpha is forced to 255 ------------------------------------------------------------

def _mul8bit(a, b):
    t = a * b + 128
    return (t + (t >> 8)) >> 8


def _as16bit(rgb):
    return (_mul8bit(rgb[:, 0], 31) << 11) + (_mul8bit(rgb[:, 1], 63) << 5) + _mul8bit(rgb[:, 2], 31)


def _palette(c0, c1):
    """(n, 4, 3): the two endpoints expanded, then the 1/3 points by (2 a + b) // 3."""
    def expand(c):
        return np.stack([_expand5(c >> 11), _expand6((c >> 5) & 63), _expand5(c & 31)], axis=1)
    p0, p1 = expand(c0), expand(c1)
    return np.stack([p0, p1, (2 * p0 + p1) // 3, (2 * p1 + p0) // 3], axis=1)


def _match(rgb, c0, c1):
    """The projection match with its three cut points -> (n,) masks (int64 holding 32 bits)."""
    pal = _palette(c0, c1)
    d = pal[:, 0] - pal[:, 1]
    dots = (rgb * d[:, None, :]).sum(axis=2) * 2
    stops = (pal * d[:, None, :]).sum(axis=2)
    c0p, half, c3p = (stops[:, 1] + stops[:, 3])[:, None], (stops[:, 3] + stops[:, 2])[:, None], (stops[:, 2] + stops[:, 0])[:, None]
    idx = np.where(dots < half, np.where(dots < c0p, 1, 3), np.where(dots < c3p, 2, 0))
    mask = np.zeros(len(rgb), dtype=np.int64)
    for i in range(16):
        mask |= idx[:, i] << (2 * i)
    return mask


def _endpoints(rgb):
    """Mean, covariance, four power iterations in float32, the extreme points along the axis -> (max16, min16, where the axis fell
    back to luminance)."""
    n = len(rgb)
    mu = (rgb.sum(axis=1) + 8) >> 4
    lo, hi = rgb.min(axis=1), rgb.max(axis=1)
    d = rgb - mu[:, None, :]
    r, g, b = d[:, :, 0], d[:, :, 1], d[:, :, 2]
    cov = [(r * r).sum(axis=1), (r * g).sum(axis=1), (r * b).sum(axis=1), (g * g).sum(axis=1), (g * b).sum(axis=1), (b * b).sum(axis=1)]
    c = [x.astype(f32) / f32(255.0) for x in cov]
    vr, vg, vb = [(hi[:, k] - lo[:, k]).astype(f32) for k in range(3)]
    for _ in range(4):
        nr = (vr * c[0] + vg * c[1]) + vb * c[2]
        ng = (vr * c[1] + vg * c[3]) + vb * c[4]
        nb = (vr * c[2] + vg * c[4]) + vb * c[5]
        vr, vg, vb = nr, ng, nb
        assert vr.dtype == f32
    magn = np.maximum(np.maximum(np.abs(vr.astype(np.float64)), np.abs(vg.astype(np.float64))), np.abs(vb.astype(np.float64)))
    small = magn < 4.0
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(small, 0.0, 512.0 / np.where(small, 1.0, magn))
    axis = np.stack([np.where(small, 299, (vr.astype(np.float64) * s).astype(np.int64)),
                     np.where(small, 587, (vg.astype(np.float64) * s).astype(np.int64)),
                     np.where(small, 114, (vb.astype(np.float64) * s).astype(np.int64))], axis=1)
    dots = (rgb * axis[:, None, :]).sum(axis=2)
    imin, imax = dots.argmin(axis=1), dots.argmax(axis=1)                        # (the first of equal extremes)
    k = np.arange(n)
    return _as16bit(rgb[k, imax]), _as16bit(rgb[k, imin]), small


def _quantize(x, scale, mid):
    x = np.minimum(np.maximum(x, f32(0.0)), f32(1.0))
    q = (x * f32(scale)).astype(np.int64)
    return q + (x > mid[q])


_W1 = np.array([3, 0, 2, 1], dtype=np.int64)
_PRODS = np.array([0x090000, 0x000900, 0x040102, 0x010402], dtype=np.int64)


def _refine(rgb, mask):
    """One least-squares round -> (max16, min16) for the given index masks."""
    same = (mask ^ ((mask << 2) & 0xFFFFFFFF)) < 4                               # all 16 texels have one index: the system is singular
    avg = (rgb.sum(axis=1) + 8) >> 4
    smax = (OMATCH5[avg[:, 0], 0] << 11) | (OMATCH6[avg[:, 1], 0] << 5) | OMATCH5[avg[:, 2], 0]
    smin = (OMATCH5[avg[:, 0], 1] << 11) | (OMATCH6[avg[:, 1], 1] << 5) | OMATCH5[avg[:, 2], 1]
    step = (mask[:, None] >> (2 * np.arange(16))[None, :]) & 3
    w1 = _W1[step]
    akku = _PRODS[step].sum(axis=1)
    at1 = (w1[:, :, None] * rgb).sum(axis=1)
    at2 = 3 * rgb.sum(axis=1) - at1
    xx, yy, xy = akku >> 16, (akku >> 8) & 0xFF, akku & 0xFF
    det = xx * yy - xy * xy
    with np.errstate(divide="ignore"):
        f = (f32(3.0) / f32(255.0)) / np.where(same, 1, det).astype(f32)
    assert f.dtype == f32
    hi = [(at1[:, k] * yy - at2[:, k] * xy).astype(f32) * f for k in range(3)]
    lo = [(at2[:, k] * xx - at1[:, k] * xy).astype(f32) * f for k in range(3)]
    gmax = (_quantize(hi[0], 31, MID5) << 11) | (_quantize(hi[1], 63, MID6) << 5) | _quantize(hi[2], 31, MID5)
    gmin = (_quantize(lo[0], 31, MID5) << 11) | (_quantize(lo[1], 63, MID6) << 5) | _quantize(lo[2], 31, MID5)
    return np.where(same, smax, gmax), np.where(same, smin, gmin), same


def encode_colour(rgba, info=None):
    """(n, 16, 4) uint8 -> (n, 8) bytes.  The constancy test compares whole RGBA words.  info: a dict that receives boolean arrays
    'constant', 'luminance' (the axis fell back to (299, 587, 114)), 'singular' (a refinement round found one index for all 16
    texels) and 'swapped' (the block ended with max16 < min16)."""
    rgba = np.asarray(rgba, dtype=np.uint8).reshape(-1, 16, 4)
    n = len(rgba)
    rgb = rgba[:, :, :3].astype(np.int64)
    words = np.ascontiguousarray(rgba).view(np.uint32).reshape(n, 16)
    constant = (words == words[:, :1]).all(axis=1)
    max16, min16, luminance = _endpoints(rgb)
    mask = np.where(max16 != min16, _match(rgb, max16, min16), 0)
    active = ~constant
    singular = np.zeros(n, dtype=bool)
    for _ in range(2):
        last = mask
        nmax, nmin, same = _refine(rgb, mask)
        singular |= active & same
        changed = active & ((nmax != max16) | (nmin != min16))
        max16, min16 = np.where(active, nmax, max16), np.where(active, nmin, min16)
        flat = changed & (max16 == min16)
        mask = np.where(changed, np.where(flat, 0, _match(rgb, max16, min16)), mask)
        active = active & ~flat & (mask != last)
    c = rgb[:, 0]
    cmax = (OMATCH5[c[:, 0], 0] << 11) | (OMATCH6[c[:, 1], 0] << 5) | OMATCH5[c[:, 2], 0]
    cmin = (OMATCH5[c[:, 0], 1] << 11) | (OMATCH6[c[:, 1], 1] << 5) | OMATCH5[c[:, 2], 1]
    max16, min16, mask = np.where(constant, cmax, max16), np.where(constant, cmin, min16), np.where(constant, 0xAAAAAAAA, mask)
    swap = max16 < min16
    max16, min16, mask = np.where(swap, min16, max16), np.where(swap, max16, min16), np.where(swap, mask ^ 0x55555555, mask)
    if info is not None:
        info["constant"], info["singular"], info["swapped"] = constant, singular, swap
        info["luminance"] = ~constant & luminance
    out = np.zeros((n, 8), dtype=np.uint8)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = max16 & 0xFF, max16 >> 8, min16 & 0xFF, min16 >> 8
    for j in range(4):
        out[:, 4 + j] = (mask >> (8 * j)) & 0xFF
    return out


# ---- blocks, levels, chains ------------------------------------------------------------------------------------------------------

def encode_blocks(blocks, format, info=None):
    blocks = np.asarray(blocks, dtype=np.uint8).reshape(-1, 16, 4)
    if format == BC1_RGB:
        return encode_colour(blocks, info)
    if format == BC3:
        opaque = blocks.copy()
        opaque[:, :, 3] = 255
        return np.concatenate([encode_channel(blocks[:, :, 3]), encode_colour(opaque, info)], axis=1)
    if format == BC4:
        return encode_channel(blocks[:, :, 0])
    if format == BC5:
        return np.concatenate([encode_channel(blocks[:, :, 0]), encode_channel(blocks[:, :, 1])], axis=1)
    raise ValueError(format)


def fill_blocks(img):
    img = np.asarray(img, dtype=np.uint8)
    h, w = img.shape[:2]
    bw, bh = (w + 3) // 4, (h + 3) // 4
    full = img[np.arange(bh * 4) % h][:, np.arange(bw * 4) % w]
    return np.ascontiguousarray(full.reshape(bh, 4, bw, 4, 4).transpose(0, 2, 1, 3, 4)).reshape(-1, 16, 4)


def encode_level(img, format):
    return encode_blocks(fill_blocks(img), format).reshape(-1)


def encode_chain(levels, format):
    return np.concatenate([encode_level(l, format) for l in levels])
