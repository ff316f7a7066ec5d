"""The anisotropic sampler of chordvis_set_material_anisotropy on the CPU: N = 1 is the isotropic spec bit
for bit, known answers of the tap count and level, the spec against an independent float64 restatement of taps and sum, the error
against a supersampled footprint (lower at N = 8 than at N = 1), and the conditions that keep the GPU comparison from passing on
trivial inputs.  No GPU."""
import functools
import math

import numpy as np
import pytest

from chord_amd import records as R, scenes

import helpers as H
import spec_material_aniso_np as SA
import spec_material_np as SM

f32 = np.float32
FILTERS = (SM.NEAREST, SM.LINEAR, SM.NEAREST_MIPMAP_NEAREST, SM.LINEAR_MIPMAP_NEAREST, SM.NEAREST_MIPMAP_LINEAR, SM.LINEAR_MIPMAP_LINEAR)
WRAPS = (SM.REPEAT, SM.CLAMP_TO_EDGE, SM.MIRRORED_REPEAT)
MIP_LINEAR = (SM.NEAREST_MIPMAP_LINEAR, SM.LINEAR_MIPMAP_LINEAR)
MIP_NEAREST = (SM.NEAREST_MIPMAP_NEAREST, SM.LINEAR_MIPMAP_NEAREST)


@functools.lru_cache(maxsize=None)
def _frame(w, h):
    import orc
    scene, cam, view, iv = H.setup_scene(scenes.material_test_scene, w, h)
    fr = orc.frame(scene, view, iv, H.ALL_FLAGS)
    return scene, cam, view, iv, fr


@functools.lru_cache(maxsize=None)
def _resolved(w, h, n):
    scene, cam, view, iv, fr = _frame(w, h)
    st = {}
    out = SA.resolve(scene, fr["vis"], fr["cmds"], view, iv, w, h, stats=st, max_aniso=n)
    return out, st


# ---- 1. N = 1 is the isotropic sampler -----------------------------------------------------------------------------------------

def test_n1_is_the_isotropic_spec_and_k0_pixels_keep_their_bits(built_lib):
    w, h = 160, 100
    scene, cam, view, iv, fr = _frame(w, h)
    today = SM.resolve(scene, fr["vis"], fr["cmds"], view, iv, w, h)
    one, _ = _resolved(w, h, 1)
    for n in SM.NAMES:
        assert np.array_equal(one[n].view(np.uint32), today[n].view(np.uint32)), n
    assert SM.sample.__module__ == "spec_material_np", "the isotropic module's sampler is back in place"
    eight, st = _resolved(w, h, 8)
    image_of = {"baseColor": "baseColor", "emissive": "emissive", "normal": "pixelNormal", "metallicRoughness": "roughMetalAO"}
    some_differ, kept = False, 0
    for slot, runs in st["slots"].items():
        for s in runs:
            same = s["pix"][s["k"] == 0]
            a, b = eight[image_of[slot]].reshape(-1, 4).view(np.uint32), today[image_of[slot]].reshape(-1, 4).view(np.uint32)
            assert np.array_equal(a[same], b[same]), (slot, s["material"])
            kept += len(same)
            some_differ |= bool(np.any(a[s["pix"][s["k"] > 0]] != b[s["pix"][s["k"] > 0]]))
    assert some_differ and kept >= 1000, kept


# ---- 2. known answers ----------------------------------------------------------------------------------------------------------

def _plan(ax, ay, bx, by, n=8, size=64):
    g = np.array([[ax / size, ay / size, bx / size, by / size]], dtype=f32)        # (size a power of two: g * size is exact)
    p = SA.tap_plan(g, size, size, n)
    return int(p["k"][0]), int(p["lodq"][0]), bool(p["major_x"][0]), int(p["lmaj"][0])


def test_known_tap_counts_and_levels():
    # lodq_of(rho2) is half the piecewise-linear log2 in Q8: 16 -> 512, 64 -> 768, 258 -> 1025 (258 = 256 * (1 + 2 / 256))
    assert _plan(4, 0, 0, 4) == (0, 512, True, 512)                       # isotropic; the tie goes to x
    assert _plan(0, 4, 4, 0)[2] is True and _plan(0, 4, 4.5, 0)[2] is False and _plan(4.5, 0, 0, 4)[2] is True
    assert _plan(8, 0, 0, 4) == (1, 512, True, 768)                       # 2:1 -> two taps one level finer
    assert _plan(0, 4, 8, 0) == (1, 512, False, 768)                      # ... along y
    assert _plan(16, 0, 0, 4) == (2, 512, True, 1024)                     # 4:1 exactly: four taps
    assert _plan(16.07, 0, 0, 4) == (3, 257, True, 1025)                  # 4:1 + eps: the ceiling asks for eight
    assert _plan(16.07, 0, 0, 4, n=4) == (2, 513, True, 1025)             # ... capped by N = 4
    k, lodq, _, lmaj = _plan(400, 0, 0, 4)                                # 100:1 at N = 8
    assert lmaj == int(SM.lodq_of(np.array([160000.0], dtype=f32))[0]) == 2204 and (k, lodq) == (3, 2204 - 768)
    assert _plan(400, 0, 0, 4, n=16)[:2] == (4, 2204 - 1024) and _plan(400, 0, 0, 4, n=1)[:2] == (0, 2204)
    assert _plan(8, 0, 0, 0) == (3, 0, True, 768)                         # rmin2 == 0: kmax, then the texel cap (768 + 255) >> 8 = 3
    assert _plan(8, 0, 0, 0, n=16) == (3, 0, True, 768)
    assert _plan(0.5, 0, 0, 0.01)[:2] == (0, 0)                           # magnified but stretched: no taps
    assert _plan(1.0, 0, 0, 0.01)[:2] == (0, 0)                           # lmaj == 0
    assert _plan(1.5, 0, 0, 0.01) == (1, 0, True, 144)                    # the cap (144 + 255) >> 8 = 1 bites; lodq' clamps at 0
    assert _plan(3.0, 0, 0, 0.01)[:2] == (2, 0)                           # 9 -> lmaj 400: cap 2
    for bad in (np.inf, -np.inf, np.nan):
        for pos in range(4):
            d = [8.0, 0.0, 0.0, 4.0]
            d[pos] = bad
            assert _plan(*d)[:2] == (0, 0), (bad, pos)
    assert _plan(1e30, 0, 0, 4)[:2] == (0, 0)                              # ra overflows to inf


def _constant_levels():
    img = np.zeros((12, 20, 4), np.uint8)
    img[...] = (200, 17, 255, 90)
    chain, mips = R.mip_chain_rgba8(img)
    return SM.levels_of(chain, 20, 12, mips)


def test_a_constant_texture_returns_its_decoded_constant_at_every_n():
    """Equal taps: every c_i - c_0 is 0, so the result is c_0 (a running sum of the taps would not do: 3c rounds)."""
    table, _ = SM.tables()
    levels = _constant_levels()
    n = 64
    u = (scenes.rand01(5, np.arange(n)) * 8 - 4).astype(f32)
    v = (scenes.rand01(6, np.arange(n)) * 8 - 4).astype(f32)
    g = (np.outer(2.0 ** np.linspace(-12, 6, n), [1.0, 0.3, -0.02, 0.09])).astype(f32)
    g[::7] = g[::7][:, [2, 3, 0, 1]]
    g[5, 0], g[9, 3], g[13, 1] = np.inf, np.nan, -np.inf
    lin_want = np.tile((np.array([200, 17, 255, 90], dtype=f32) * f32(1.0 / 255.0)), (n, 1))
    srgb_want = np.tile(np.array([table[200], table[17], table[255], f32(90) * f32(1.0 / 255.0)], dtype=f32), (n, 1))
    for N in SA.ALLOWED:
        ks = set()
        for min_f in FILTERS:
            for ws in WRAPS:
                st = {}
                assert np.array_equal(SA.sample(levels, (min_f, SM.LINEAR, ws, ws), u, v, g, None, N, st), lin_want), (N, min_f, ws)
                assert np.array_equal(SA.sample(levels, (min_f, SM.NEAREST, ws, ws), u, v, g, table, N), srgb_want), (N, min_f, ws)
                ks |= set(np.unique(st["k"]).tolist())
                assert np.all(st["k"][[5, 9, 13]] == 0) and np.all(st["lodq"][[5, 9, 13]] == 0)
        assert ks == set(range(SA.ALLOWED.index(N) + 1)), (N, ks)


# ---- 3. taps and sum against a float64 restatement -------------------------------------------------------------------------------

def _texture(w, h, seed):
    img = (scenes.pcg_hash(np.arange(w * h * 4, dtype=np.uint32) + np.uint32(seed)) & 0xFF).astype(np.uint8).reshape(h, w, 4)
    chain, mips = R.mip_chain_rgba8(img)
    return SM.levels_of(chain, w, h, mips), chain, mips


def _wrap64(i, n, mode):
    if mode == SM.CLAMP_TO_EDGE:
        return min(max(i, 0), n - 1)
    if mode == SM.MIRRORED_REPEAT:
        m = i % (2 * n)
        return m if m < n else 2 * n - 1 - m
    return i % n


def _ref_aniso(chain, w, h, mips, sampler, u, v, g, table, N):
    """one pixel, float64, own loops: item 9(g) restated from DESIGN.md.  Shared with the spec: the integer work on bit patterns
    (lodq_of of the float32 squared lengths) and the float32 tap coordinate, both part of the pin.  Returns (colour, taps)."""
    min_f, mag_f, ws, wt = sampler
    lin = lambda f: f in (SM.LINEAR, SM.LINEAR_MIPMAP_NEAREST, SM.LINEAR_MIPMAP_LINEAR)
    ax, ay, bx, by = f32(g[0]) * f32(w), f32(g[1]) * f32(h), f32(g[2]) * f32(w), f32(g[3]) * f32(h)
    ra, rb = ax * ax + ay * ay, bx * bx + by * by
    kmax = int(math.log2(N))
    lmaj = k = 0
    if math.isfinite(ra) and math.isfinite(rb) and max(ra, rb) > 0:
        lmaj = int(SM.lodq_of(np.array([max(ra, rb)], dtype=f32))[0])
        if lmaj > 0:
            mid = kmax
            if min(ra, rb) > 0:
                mid = -((-max(lmaj - int(SM.lodq_of(np.array([min(ra, rb)], dtype=f32))[0]), 0)) // 256)      # ceiling of the octaves
            k = min(kmax, mid, -((-lmaj) // 256))
    lodq = max(lmaj - 256 * k, 0)
    levels, linear, frac = [0], lin(mag_f), 0.0
    if lmaj > 0:
        linear = lin(min_f)
        if min_f in MIP_NEAREST:
            levels = [min((lodq + 128) >> 8, mips - 1)]
        elif min_f in MIP_LINEAR:
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
        c = float(f32(1.0 / 255.0))
        return np.array([table[b[0]], table[b[1]], table[b[2]], b[3] * c] if table is not None else [x * c for x in b], dtype=np.float64)

    def level(l, uu, vv):
        lw, lh = max(1, w >> l), max(1, h >> l)
        if not linear:
            return texel(l, math.floor(float(f32(uu) * f32(lw))), math.floor(float(f32(vv) * f32(lh))))
        x, y = float(f32(uu) * f32(lw) - f32(0.5)), float(f32(vv) * f32(lh) - f32(0.5))
        x0, y0 = math.floor(x), math.floor(y)
        fx, fy = x - x0, y - y0
        top = texel(l, x0, y0) * (1 - fx) + texel(l, x0 + 1, y0) * fx
        bot = texel(l, x0, y0 + 1) * (1 - fx) + texel(l, x0 + 1, y0 + 1) * fx
        return top * (1 - fy) + bot * fy

    def tap(uu, vv):
        c = level(levels[0], uu, vv)
        if len(levels) == 2 and levels[1] != levels[0]:
            c = c * (1 - frac) + level(levels[1], uu, vv) * frac
        return c
    if k == 0:
        return tap(u, v), 1
    n = 2 ** k
    du, dv = (g[0], g[1]) if ra >= rb else (g[2], g[3])
    total = np.zeros(4)
    for i in range(n):
        t = f32((2 * i + 1 - n) / (2.0 * n))
        total += tap(f32(u) + f32(du) * t, f32(v) + f32(dv) * t)
    return total / n, n


@pytest.mark.parametrize("size", [(37, 21), (64, 64), (8, 64)], ids=lambda s: "%dx%d" % s)
def test_taps_and_sum_against_a_float64_restatement(size):
    w, h = size
    levels, chain, mips = _texture(w, h, 4321 + w)
    table, _ = SM.tables()
    n = 96
    rnd = lambda j: scenes.rand01(91 + w, np.arange(j * n, (j + 1) * n))
    u, v = (rnd(0) * 6.0 - 3.0).astype(f32), (rnd(1) * 6.0 - 3.0).astype(f32)
    # the longer derivative from magnified to beyond the last level, the shorter one 1 to 64 times shorter, either axis the longer
    mag = (2.0 ** (rnd(2) * (mips + 3.0) - 2.0)) / max(w, h)
    ratio = 2.0 ** (-6.0 * rnd(3))
    ang = rnd(4) * 2.0 * np.pi
    major = np.stack([mag * np.cos(ang), mag * np.sin(ang)], -1)
    minor = np.stack([-mag * ratio * np.sin(ang), mag * ratio * np.cos(ang)], -1) * np.where(rnd(5) < 0.5, -1.0, 1.0)[:, None]
    swap = rnd(6) < 0.5
    g = np.where(swap[:, None], np.concatenate([minor, major], 1), np.concatenate([major, minor], 1)).astype(f32)
    # which derivative is the longer one in level-0 texels, in float64 (away from ties)
    g64 = g.astype(np.float64)
    la, lb = (g64[:, 0] * w) ** 2 + (g64[:, 1] * h) ** 2, (g64[:, 2] * w) ** 2 + (g64[:, 3] * h) ** 2
    x_longer, clear = la > lb, np.abs(la - lb) > 1e-4 * np.maximum(la, lb)
    assert (x_longer & clear).sum() >= n // 4 and (~x_longer & clear).sum() >= n // 4
    seen = set()
    for N in (2, 8, 16):
        for min_f in FILTERS:
            for ws in WRAPS:
                wt = WRAPS[(WRAPS.index(ws) + 1 + FILTERS.index(min_f)) % 3]
                mag_f = (SM.NEAREST, SM.LINEAR)[(FILTERS.index(min_f) + WRAPS.index(ws)) % 2]
                tb = table if (WRAPS.index(ws) + FILTERS.index(min_f)) % 2 else None
                st = {}
                got = SA.sample(levels, (min_f, mag_f, ws, wt), u, v, g, tb, N, st)
                assert np.array_equal(st["major_x"][clear], x_longer[clear])
                for i in range(FILTERS.index(min_f) % 3, n, 3):
                    want, taps = _ref_aniso(chain, w, h, mips, (min_f, mag_f, ws, wt), u[i], v[i], g[i], tb, N)
                    assert taps == st["taps"][i] == 1 << st["k"][i]
                    seen.add(int(st["k"][i]))
                    # values are in [0, 1]; a tap is < 16 float32 operations of 2^-24 each (as in test_material_spec.py); per further tap
                    # one rounding of c_i - c_0 (<= 2^-24) and one of the partial sum d (|d| <= taps: <= taps * 2^-24, which the
                    # exact 1 / taps scales back to 2^-24); one more for the final add
                    bound = 2.0 ** -20 + (2 * taps + 1) * 2.0 ** -24
                    assert np.max(np.abs(got[i].astype(np.float64) - want)) <= bound, (N, min_f, ws, i, got[i], want)
    assert seen == {0, 1, 2, 3, 4}


# ---- 4. better, not just different ------------------------------------------------------------------------------------------------

def test_n8_is_closer_to_the_supersampled_footprint_than_n1(built_lib):
    """Pixels of the trilinear material (the ground, and a wall) whose base colour takes k >= 2 at N = 8.  Ground truth per pixel: the
    float64 mean of decoded level-0 texels at 16 x 16 points uv + s * A + t * B of the footprint parallelogram, s and t the centres
    of a regular grid on (-1/2, 1/2), then the base colour's factor and sRGB_2_AP1.  Measured at 320 x 200: mean
    absolute error over rgb 0.01760 at N = 1, 0.01148 at N = 8 (8960 pixels)."""
    w, h = 320, 200
    scene, cam, view, iv, fr = _frame(w, h)
    one, _ = _resolved(w, h, 1)
    eight, st = _resolved(w, h, 8)
    srgb, ap1 = SM.tables()
    run = [s for s in st["slots"]["baseColor"]
           if SM.slot_texture(scene, scene.materials[s["material"]], "baseColor")[1][0] == SM.LINEAR_MIPMAP_LINEAR][0]
    M = scene.materials[run["material"]]
    levels, smp = SM.slot_texture(scene, M, "baseColor")
    assert smp[2] == smp[3] == SM.REPEAT
    pix = run["pix"][run["k"] >= 2]
    assert len(pix) >= 1000, len(pix)
    A = SM.SR.resolve(scene, fr["vis"], fr["cmds"], view, iv, w, h, names=("uv", "uvGrad"))
    uv, g = A["uv"].reshape(-1, 2)[pix].astype(np.float64), A["uvGrad"].reshape(-1, 4)[pix].astype(np.float64)
    c = (np.arange(16) + 0.5) / 16.0 - 0.5
    s, t = (x.reshape(1, -1) for x in np.meshgrid(c, c))
    uu = uv[:, 0:1] + s * g[:, 0:1] + t * g[:, 2:3]
    vv = uv[:, 1:2] + s * g[:, 1:2] + t * g[:, 3:4]
    H0, W0 = levels[0].shape
    ix, iy = np.mod(np.floor(uu * W0).astype(np.int64), W0), np.mod(np.floor(vv * H0).astype(np.int64), H0)
    words = levels[0][iy, ix]
    rgb = np.stack([srgb.astype(np.float64)[(words >> np.uint32(8 * k)) & np.uint32(255)] for k in range(3)], -1).mean(axis=1)
    rgb = rgb * np.asarray(M["baseColorFactor"], dtype=np.float64)[None, :3]
    truth = rgb @ ap1.astype(np.float64).T
    err = lambda img: float(np.abs(img["baseColor"].reshape(-1, 4)[pix, :3].astype(np.float64) - truth).mean())
    e1, e8 = err(one), err(eight)
    print("mean absolute base-colour error over %d pixels with k >= 2: N = 1 %.5f, N = 8 %.5f" % (len(pix), e1, e8))
    assert e8 < e1, (e1, e8)


# ---- 5. the GPU comparison cannot pass on trivial inputs ------------------------------------------------------------------------------

def test_material_test_scene_exercises_every_tap_count(built_lib):
    scene, cam, view, iv, fr = _frame(320, 200)
    _, st16 = _resolved(320, 200, 16)
    _, st8 = _resolved(320, 200, 8)
    runs = lambda st: [(slot, s) for slot, rs in st["slots"].items() for s in rs]
    k16 = np.concatenate([s["k"] for _, s in runs(st16)])
    k8 = np.concatenate([s["k"] for _, s in runs(st8)])
    for k in range(5):
        assert (k16 == k).sum() >= 10, (k, (k16 == k).sum())
    for k in range(4):
        assert (k8 == k).sum() >= 100, (k, (k8 == k).sum())
    assert k8.max() == 3 and k16.max() == 4
    mx = np.concatenate([s["major_x"][s["k"] > 0] for _, s in runs(st8)])
    assert mx.sum() >= 100 and (~mx).sum() >= 100, (mx.sum(), (~mx).sum())
    kinds = set()
    for slot, s in runs(st8):
        if np.any(s["k"] >= 1):
            f = SM.slot_texture(scene, scene.materials[s["material"]], slot)[1][0]
            kinds.add("linear" if f in MIP_LINEAR else "nearest" if f in MIP_NEAREST else "none")
    assert kinds == {"linear", "nearest", "none"}, kinds
    # the level shift reaches the clamp at 0 and leaves the last level
    lod = np.concatenate([s["lodq"][s["k"] > 0] for _, s in runs(st8)])
    assert (lod == 0).sum() >= 10 and (lod > 0).sum() >= 100
