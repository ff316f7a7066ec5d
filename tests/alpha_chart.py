"""Sampler charts for the raster's alpha test: scenes of screen-space quads ("cells", two triangles each) whose pixel size, texture
coordinates and material pin ONE (texture, wrapS, wrapT, filter, level) case each.  Shared by tests/test_alpha_chart_spec.py (CPU: the
oracle alone -- every cell takes the level and filter it is named for, shows both outcomes of the alpha test, and differs under a
wrong sampler) and tests/test_gpu_alpha_chart.py (the kernels, bit for bit against the oracle).

Geometry.  A 256 x 192 target, the camera at the origin looking down -z.  A cell is an axis-aligned square of P = 16 px whose
corners lie on pixel borders (integer pixel coordinates: the snapped 24.8 coordinates are exact and a cell covers exactly 16 x 16
pixel centres), 4 px from its neighbours; an opaque backdrop quad lies behind all of them, so a clipped pixel shows the backdrop's
id.  Every material's cells are one hand-written LOD-0 meshlet (ray_deep_cases.meshlet_primitive), one object per material.  On
every second chart the materials are two-sided and every second cell is wound the other way: both set-up buckets and both signs of
the edge functions run.

Level.  level = floor(log2(ratio)) >> 1 with ratio = |uv cross| W H / (doubled pixel area / 65536) (oracle.c header item 9).  A cell
of level L on a W x H texture has uv legs a 2^L P / W and a 2^L P / H: the ratio is a^2 4^L, with a^2 = 1.5 in the middle of the
level's range [4^L, 4^(L + 1)), and a^2 = 0.4 for the magnified cell (ratio < 1: level 0, mag filter).  The uv square is sheared a
little -- u runs 1 / 13 of its leg along y, v 1 / 11 of its leg along x, the ratio 142 / 143 of the above --, so that no two rows
and no two columns of a cell sample a level at the same phase: a cell of a one-texel-wide level has 256 samples of it, not 16.

Origin.  The uv origin of a cell is (-1.37, -0.61) on every axis where the cell then leaves [0, 1] on both sides (legs above 2.37 /
1.61).  A cell of a low level of a large texture has legs far below 1 and would lie wholly outside [0, 1] there -- constant under
CLAMP_TO_EDGE --, so on such an axis the origin scales with the leg: the cell lies across the texture's edge at 0 (every second
cell: at 1) with 0.55 (u) or 0.45 (v) of the leg before the edge.  Either way every wrap mode matters in every cell.

Textures.  Finished chains (records.TextureChain) whose levels hold seeded noise INDEPENDENT of each other: box-filtered noise is
flat from the fourth level up (every texel near 0.5), and a fetch from a wrong level of independent noise is a wrong value.  The
noise is of two classes of bytes, one below and one above every threshold (noise_chain says why).  The 1 x 1 level holds byte 128;
the materials alternate between the thresholds 0.4 (factor 1, cut-off 0.4) and 0.6 (factor 0.8, cut-off 0.48), so the cells of a
1 x 1 level are kept under one and clipped under the other.

Charts (one frame each):
    64x64      power-of-two periods (masks); 7 levels
    37x21      period_mod on both axes: periods 37 / 74 / 21 / 42 and those of 18x10, 9x5, 4x2, 2x1, 1x1
    1x9, 9x1   levels one texel wide on one axis (period 1, mirrored period 2)
    16383x2    the largest non-power-of-two periods (16 383, 32 766) and dims words near 16 bits; levels 0 and 1
    16384x1    a 15-level chain: levels 0, 7, 13, 14 and a cell whose ratio asks for level 17 (the clamp to texMips - 1)
    64x64_edges  three small groups on the 64 x 64 texture, in a frame of their own (with the grid's 108 cells they do not fit):
               level boundaries (ratio exactly 1 and 4, and one ulp of a leg below), equality at the cut-off (a 16 x 16 ramp of the
               bytes 0 .. 255), wild coordinates (u W at +-1e9, beyond, inf, NaN)
Every chart has the nine (wrapS, wrapT) pairs under two filter pairs, (min NEAREST_MIPMAP_NEAREST, mag LINEAR) and
(min LINEAR_MIPMAP_LINEAR, mag NEAREST): 18 materials, each with a magnified cell and minified cells -- nearest and bilinear each
run as min and as mag filter, and a sampler with min and mag exchanged gives another image."""
import functools

import numpy as np

import ray_deep_cases
from chord_amd import lib as L, records as R, scenes
from helpers import _unproject

WIDTH, HEIGHT, P, GAP = 256, 192, 16, 4
AREA2 = (P * 256) ** 2                                    # |doubled area| of a cell's triangle in 24.8 sub-pixels
WRAPS = (R.WRAP_REPEAT, R.WRAP_CLAMP_TO_EDGE, R.WRAP_MIRRORED_REPEAT)
WRAP_NAME = {R.WRAP_REPEAT: "repeat", R.WRAP_CLAMP_TO_EDGE: "clamp", R.WRAP_MIRRORED_REPEAT: "mirror"}
FILTER_PAIRS = ((R.FILTER_NEAREST_MIPMAP_NEAREST, R.FILTER_LINEAR), (R.FILTER_LINEAR_MIPMAP_LINEAR, R.FILTER_NEAREST))
PAIR_NAME = ("min nearest/mag linear", "min linear/mag nearest")
PAIR_LINEAR = ({"min": 0, "mag": 1}, {"min": 1, "mag": 0})
THRESHOLDS = ((0.4, 1.0), (0.48, 0.8))                     # (alphaCutOff, alphaFactor) of even / odd materials: 0.4 and 0.6
ORIGIN, EDGE_SHARE = (-1.37, -0.61), (0.55, 0.45)
A2_MIN, A2_MAG = 1.5, 0.4
SHEAR = (13.0, 11.0)                                       # u runs 1 / 13 of its leg along y, v 1 / 11 of its leg along x
CUTOFF_BYTE = 128
MUTATIONS = ("wrapS", "wrapT", "filters", "cutoff")
F = np.float32


def mip_count(w, h):
    return max(w, h).bit_length()


def noise_chain(w, h, seed):
    """records.TextureChain of w x h: every level seeded noise of its own in alpha (and 200 in r, g, b).  A texel is of a low or a
    high class at random -- bytes 95 .. 100, just below both thresholds (0.4 and 0.6 of 255 are 102 and 153), or 155 .. 160, just
    above both.  A fetch of another texel is then another outcome in half of all cases, under either threshold; and a bilinear
    blend of a low and a high texel leaves the low side of 0.4 after an eighth of the way (the high side of 0.6 alike), far from
    the half-way point where NEAREST changes texels: over three eighths of a texel's width next to every change of class the two
    filters give different outcomes.  A level of at most 16 texels alternates the classes as a checker, so that every neighbour
    is a change of class -- with one step left out in the middle of an odd side, because an odd alternating row ends as it
    begins and MIRRORED_REPEAT and REPEAT would continue it alike.  The 1 x 1 level holds byte 128, between the thresholds."""
    rng = np.random.default_rng([seed, w, h])
    levels = []
    for lw, lh in R.level_dims(w, h, mip_count(w, h)):
        img = np.full((lh, lw, 4), 200, dtype=np.uint8)
        high = rng.integers(0, 2, (lh, lw))
        if lw * lh <= 16:
            x, y = np.arange(lw)[None, :], np.arange(lh)[:, None]
            high = (x + y + (x >= lw // 2) * (lw % 2) * (lw > 1) + (y >= lh // 2) * (lh % 2) * (lh > 1) + int(high[0, 0])) % 2
        img[..., 3] = np.where(high == 1, 155, 95) + rng.integers(0, 6, (lh, lw)) if lw * lh > 1 else 128
        levels.append(img.reshape(-1))
    return R.TextureChain(np.concatenate(levels), w, h, len(levels))


def ramp_chain():
    """16 x 16, alpha byte = 16 y + x: every byte 0 .. 255 once (the upper levels box-filtered, never sampled)."""
    img = np.full((16, 16, 4), 200, dtype=np.uint8)
    img[..., 3] = np.arange(256, dtype=np.uint8).reshape(16, 16)
    data, mips = R.mip_chain_rgba8(img)
    return R.TextureChain(data, 16, 16, mips)


class Cell:
    """One quad.  corners A (x0, y0), B (x0, y1), C (x1, y0), D (x1, y1); triangles (A, B, C) and (C, B, D), front-facing (negative
    doubled area in y-down screen space) unless `flip`.  uv: float32 (4, 2) at A, B, C, D.  want: per triangle the (level, "min" or
    "mag") it is named for.  material: the chart's material number.  wild: the axis (0 u, 1 v) that carries a value at or beyond the
    texel_floor guard, or None."""

    def __init__(self, texture, dims, material, group, label, uv, want, wild=None):
        self.texture, self.dims, self.material, self.group, self.label = texture, dims, material, group, label
        self.uv, self.want, self.wild = np.asarray(uv, dtype=F), list(want), wild
        self.flip, self.rect, self.chart = False, None, None
        self.object, self.first_triangle, self.scene_material = None, None, None     # filled by build()

    def corners(self):
        x0, y0 = self.rect
        return (x0, y0), (x0, y0 + P), (x0 + P, y0), (x0 + P, y0 + P)

    def triangles(self):
        """Per triangle the corner numbers, in the winding drawn."""
        return [(0, 2, 1), (2, 3, 1)] if self.flip else [(0, 1, 2), (2, 1, 3)]

    def level_dims(self, tri):
        lv = self.want[tri][0]
        return max(1, self.dims[0] >> lv), max(1, self.dims[1] >> lv)

    def texels(self):
        """The fewest texels of a level this cell samples."""
        return min(w * h for w, h in (self.level_dims(0), self.level_dims(1)))

    def linear(self, tri, exchanged=False):
        pair = 0 if self.group == "cutoff" else self.material // 9
        which = self.want[tri][1]
        if exchanged:
            which = "mag" if which == "min" else "min"
        return 0 if self.group == "cutoff" else PAIR_LINEAR[pair][which]

    def affected(self, mutation):
        """Whether the cell must differ from the unmutated image under `mutation`, by rule:
          - the cut-off cells sample inside [0, 1] under a NEAREST / NEAREST sampler: only the cut-off's ulp moves them, and it moves
            no other cell;
          - a wrap mode is nothing on an axis where every level the cell samples is one texel wide;
          - a wild value at or beyond the texel_floor guard (|u W| >= 1e9, inf, NaN) is texel 0 on its axis under every wrap mode:
            the wrap of the axis that carries it is exempt (the other axis and the filters are not);
          - the filters are nothing on a 1 x 1 level."""
        if mutation == "cutoff" or self.group == "cutoff":
            return mutation == "cutoff" and self.group == "cutoff"
        dims = [self.level_dims(0), self.level_dims(1)]
        if mutation == "filters":
            return any(w * h > 1 for w, h in dims)
        axis = 0 if mutation == "wrapS" else 1
        return self.wild != axis and any(d[axis] > 1 for d in dims)

    @property
    def name(self):
        if self.group == "cutoff":
            return "%s cutoff %s" % (self.texture, self.label)
        m = self.material % 9
        return "%s %s/%s, %s, %s %s" % (self.texture, WRAP_NAME[WRAPS[m // 3]], WRAP_NAME[WRAPS[m % 3]], PAIR_NAME[self.material // 9],
                                        self.group, self.label)


def _origin(leg, axis, at_one):
    if ORIGIN[axis] + leg > 1.0:
        return ORIGIN[axis]
    return (1.0 if at_one else 0.0) - EDGE_SHARE[axis] * leg


def _quad_uv(u0, v0, lu, lv, su=0.0, sv=0.0):
    """uv at A, B, C, D: legs lu along x and lv along y, sheared by su (u along y) and sv (v along x)."""
    return np.array([(u0, v0), (u0 + su, v0 + lv), (u0 + lu, v0 + sv), (u0 + lu + su, v0 + lv + sv)], dtype=F)


def _level_cell(texture, dims, material, a2, level, which, label, n, scale=1.0):
    a = np.sqrt(a2) * scale
    lu, lv = a * 2.0 ** level * P / dims[0], a * 2.0 ** level * P / dims[1]
    uv = _quad_uv(_origin(lu, 0, n & 1), _origin(lv, 1, n & 2), lu, lv, lu / SHEAR[0], lv / SHEAR[1])
    named = min(level, mip_count(*dims) - 1)
    return Cell(texture, dims, material, "grid", label, uv, [(named, which)] * 2)


def _grid(texture, dims, levels, extra=(), clamp=False):
    cells = []
    last = mip_count(*dims) - 1
    for m in range(18):
        cells.append(_level_cell(texture, dims, m, A2_MAG, 0, "mag", "magnified", len(cells)))
        for lv in list(levels) + ([extra[m % len(extra)]] if extra else []):
            cells.append(_level_cell(texture, dims, m, A2_MIN, lv, "min", "level %d" % lv, len(cells)))
        if clamp:        # legs 8 x those of the last level: the ratio asks for level last + 3
            c = _level_cell(texture, dims, m, A2_MIN, last, "min", "level %d asked %d" % (last, last + 3), len(cells), scale=8.0)
            cells.append(c)
    return cells


def _edge_cells():
    dims, tex, cells = (64, 64), "64x64", []
    # 1. level boundaries: origin (-1, -2) plus a quarter of a level-0 texel, every value exact in float32.  (At (-1, -2) itself the
    # pixel centres of the ratio-1 and ratio-4 cells are texel centres, where bilinear and nearest fetch the same value: the cell
    # could not tell which filter ran.  And a mirrored axis repeats after two periods: at -2 MIRRORED_REPEAT is REPEAT, so v is
    # not mirrored here.)
    tiny, quarter = 2.0 ** -24, 1.0 / 256.0
    for pair in (0, 1):
        m = pair * 9 + (0 if pair == 0 else 7)                   # (repeat, repeat) and (mirror, clamp)
        for lu, lv, level, which, label in ((0.25, 0.25, 0, "min", "ratio 1"), (0.25 - tiny, 0.25, 0, "mag", "ratio 1 - ulp"),
                                            (0.5, 0.5, 1, "min", "ratio 4"), (0.5 - tiny, 0.5, 0, "min", "ratio 4 - ulp")):
            uv = _quad_uv(-1.0 + quarter, -2.0 + quarter, lu, lv)
            assert float(uv[2, 0]) - float(uv[0, 0]) == lu and float(uv[1, 1]) - float(uv[0, 1]) == lv
            cells.append(Cell(tex, dims, m, "boundary", label, uv, [(level, which)] * 2))
    # 2. equality at the cut-off: the ramp 1 : 1 under NEAREST; pixel (x, y) of the cell samples byte 16 y + x
    for k, label in enumerate(("factor 1", "factor 0.9")):
        cells.append(Cell("ramp16", (16, 16), 18 + k, "cutoff", label, _quad_uv(0.0, 0.0, 1.0, 1.0), [(0, "min")] * 2))
    # 3. wild coordinates.  One u for all corners (zero uv area: ratio 0, level 0, mag filter); v across the edge at 0
    lv = np.sqrt(A2_MIN) * P / 64.0
    v0 = -EDGE_SHARE[1] * lv
    big = F(1.0e9)
    below, above = np.nextafter(big, F(0)), np.nextafter(big, F(np.inf))
    values = [("1e9 - ulp", below), ("1e9", big), ("1e9 + ulp", above), ("-(1e9 - ulp)", -below), ("-1e9", -big), ("-(1e9 + ulp)", -above),
              ("2e9", F(2.0e9)), ("64e30", F(1.0e30) * F(64))]
    n = 0
    for pair in (0, 1):
        for label, xw in values:                                  # xw = u W
            u = F(xw) / F(64)
            assert F(u * F(64)) == F(xw)
            uv = _quad_uv(0.0, v0, 0.0, lv, 0.0, lv / SHEAR[1]); uv[:, 0] = u
            # inside the guard the index is a multiple of 64: REPEAT gives texel 0 where CLAMP_TO_EDGE gives 63 (the positive one),
            # CLAMP_TO_EDGE 0 where MIRRORED_REPEAT gives 63 (the negative one) -- those two get that wrapS; the others any
            inside = abs(float(xw)) < 1.0e9
            m = pair * 9 + ((0 if xw > 0 else 3) + n % 3 if inside else n % 9)
            cells.append(Cell(tex, dims, m, "wild", "u W = " + label, uv, [(0, "mag")] * 2, wild=None if inside else 0)); n += 1
        # one corner inf / NaN.  In u at C: triangle (A, B, C) has cross = 0 * 0 - inf * lv (inf: the last level, min filter; NaN
        # for a NaN), triangle (C, B, D) has -inf * lv + inf * lv = NaN (level 0, mag filter).  In v at B alike.
        lu = np.sqrt(A2_MIN) * P / 64.0
        for label, val in (("+inf", F(np.inf)), ("-inf", F(-np.inf)), ("NaN", F(np.nan))):
            first = (0, "mag") if np.isnan(val) else (6, "min")
            uv = _quad_uv(-EDGE_SHARE[0] * lu, v0, lu, lv); uv[2, 0] = val
            cells.append(Cell(tex, dims, pair * 9 + n % 9, "wild", "u(C) = " + label, uv, [first, (0, "mag")], wild=0)); n += 1
            uv = _quad_uv(-EDGE_SHARE[0] * lu, v0, lu, lv); uv[1, 1] = val
            cells.append(Cell(tex, dims, pair * 9 + n % 9, "wild", "v(B) = " + label, uv, [first, (0, "mag")], wild=1)); n += 1
    return cells


class Chart:
    def __init__(self, name, textures, cells, two_sided, extra_materials=()):
        self.name, self.textures, self.cells, self.two_sided, self.extra_materials = name, textures, cells, two_sided, extra_materials
        for n, c in enumerate(cells):
            c.chart, c.flip = name, bool(two_sided and n % 2)


# seeds: any under which tests/test_alpha_chart_spec.py holds (its rules, not the seed, are the test)
SEEDS = {"64x64": 1, "37x21": 1, "1x9": 1, "9x1": 1, "16383x2": 1, "16384x1": 1}
CHART_NAMES = ("64x64", "37x21", "1x9", "9x1", "16383x2", "16384x1", "64x64_edges")


@functools.lru_cache(maxsize=None)
def _texture(name):
    if name == "ramp16":
        return ramp_chain()
    w, h = (int(s) for s in name.split("x"))
    return noise_chain(w, h, SEEDS[name])


def cutoff_values():
    """(alphaCutOff, alphaFactor) of the two cut-off materials: the tap of byte k is float(k) * (1 / 255.0f); A compares it with
    itself, B its product with 0.9 with that product: byte k gives exactly 0 (kept), byte k - 1 less (clipped)."""
    tap = F(CUTOFF_BYTE) * F(1.0 / 255.0)
    return (float(tap), 1.0), (float(F(tap * F(0.9))), float(F(0.9)))


def chart(name):
    """A fresh Chart (cells are filled in by build(), so they are not shared)."""
    two = name in CHART_NAMES[1::2]                             # every second chart two-sided
    if name == "64x64":
        return Chart(name, ["64x64"], _grid(name, (64, 64), (0, 1, 2, 6), extra=(3, 4, 5)), two)
    if name == "37x21":
        return Chart(name, ["37x21"], _grid(name, (37, 21), (0, 1, 2, 5), extra=(3, 4)), two)
    if name == "37x21_short":                                  # without the extra levels: what a 192-texel depth view holds
        return Chart(name, ["37x21"], _grid("37x21", (37, 21), (0, 1, 2, 5)), True)
    if name in ("1x9", "9x1"):
        w, h = (int(s) for s in name.split("x"))
        return Chart(name, [name], _grid(name, (w, h), (0, 1, 2, 3)), two)
    if name == "16383x2":
        return Chart(name, [name], _grid(name, (16383, 2), (0, 1)), two)
    if name == "16384x1":
        return Chart(name, [name], _grid(name, (16384, 1), (0, 7, 13, 14), clamp=True), two)
    assert name == "64x64_edges"
    return Chart(name, ["64x64", "ramp16"], _edge_cells(), two, extra_materials=cutoff_values())


class Built:
    """A chart scene set up for its camera: scene, cam, view, iv, the cells with their places, width, height."""

    def __init__(self, scene, cam, view, iv, cells, names):
        self.scene, self.cam, self.view, self.iv, self.cells, self.names = scene, cam, view, iv, cells, names
        self.width, self.height = cam.width, cam.height
        self.what = "+".join(names)

    def cell_at(self, x, y):
        for c in self.cells:
            if c.rect[0] <= x < c.rect[0] + P and c.rect[1] <= y < c.rect[1] + P:
                return c
        return None

    def object_image(self, vis, cmds):
        """Per pixel the object drawn there (-1: none), from visibility words and the frame's command list."""
        low = (np.asarray(vis, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)
        slot = ((low >> 8) & 0xFFFFFF) - 1
        obj = np.where(low != 0, np.asarray(cmds["objectId"], dtype=np.int64)[np.maximum(slot, 0)], -1)
        return obj.reshape(self.height, self.width)

    def pixels(self, cell, image):
        x0, y0 = cell.rect
        return image.reshape(self.height, self.width)[y0:y0 + P, x0:x0 + P]

    def first_difference(self, got, want):
        """'' when the images agree, else the first differing pixel and the cell it belongs to."""
        got, want = (np.asarray(a, dtype=np.uint64).reshape(self.height, self.width) for a in (got, want))
        bad = np.argwhere(got != want)
        if not len(bad):
            return ""
        y, x = bad[0]
        c = self.cell_at(x, y)
        return "%d pixels differ, first (x=%d, y=%d) in %s: got %#018x want %#018x" % (
            len(bad), x, y, "cell [%s]" % c.name if c else "no cell", int(got[y, x]), int(want[y, x]))


def mutate(scene, charts_cells, mutation):
    """Changes the scene's sampler / material records in place: wrapS or wrapT of every sampler to the next mode, min and mag
    filters exchanged, or the cut-off of the cut-off materials one ulp up."""
    smp, mats = scene.samplers, scene.materials
    if mutation in ("wrapS", "wrapT"):
        nxt = {WRAPS[i]: WRAPS[(i + 1) % 3] for i in range(3)}
        smp[mutation] = [nxt[int(w)] for w in smp[mutation]]
    elif mutation == "filters":
        smp["minFilter"], smp["magFilter"] = smp["magFilter"].copy(), smp["minFilter"].copy()
    else:
        assert mutation == "cutoff"
        for c in charts_cells:
            if c.group == "cutoff":
                m = c.scene_material
                mats["alphaCutOff"][m] = np.nextafter(mats["alphaCutOff"][m], F(np.inf))


def build(names, width=WIDTH, height=HEIGHT, gap=GAP, mutation=None):
    """The scene of one chart (a name) or of several (a sequence: chart k in a band of its own, `height` pixels high, below the one
    before; one texture table, one sampler table, every chart's materials)."""
    names = (names,) if isinstance(names, str) else tuple(names)
    charts = [chart(n) for n in names]
    full_height = height * len(charts)
    cam = scenes.Camera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), width, full_height)
    view, iv = L.make_views(cam)
    cols, rows = (width - gap - P) // (P + gap) + 1, (height - gap - P) // (P + gap) + 1
    cells, tris = [], []
    for band, ch in enumerate(charts):
        assert len(ch.cells) <= cols * rows, "%s: %d cells, room for %d" % (ch.name, len(ch.cells), cols * rows)
        for n, c in enumerate(ch.cells):
            c.rect = (gap + (n % cols) * (P + gap), band * height + gap + (n // cols) * (P + gap))
            corners = c.corners()
            tris += [tuple(corners[k] for k in t) for t in c.triangles()]
            cells.append(c)
    pos = _unproject(view, iv, tris, width, full_height)
    back = _unproject(view, iv, [((-8.0, -8.0), (-8.0, full_height + 8.0), (width + 8.0, -8.0)),
                                 ((width + 8.0, -8.0), (-8.0, full_height + 8.0), (width + 8.0, full_height + 8.0))],
                      width, full_height, dist0=16.0)
    sb = scenes.SceneBuilder("alpha_chart_" + "+".join(names))
    prim = ray_deep_cases.meshlet_primitive(back, [np.arange(6).reshape(2, 3)], (1,))
    sb.prims.append(prim)
    sb.add_object(0)                                           # object 0: the backdrop, opaque
    at = 0
    for ch in charts:
        tex = []
        for t in ch.textures:
            sb.textures.append(_texture(t)); tex.append(len(sb.textures) - 1)
        first_sampler = len(sb.samplers)
        for pair in FILTER_PAIRS:
            for ws in WRAPS:
                for wt in WRAPS:
                    sb.add_sampler(pair[0], pair[1], ws, wt)
        nearest = sb.add_sampler(R.FILTER_NEAREST, R.FILTER_NEAREST, R.WRAP_CLAMP_TO_EDGE, R.WRAP_CLAMP_TO_EDGE)
        by_material = {}
        for k, c in enumerate(ch.cells):
            by_material.setdefault(c.material, []).append((c, at + 2 * k))
        at += 2 * len(ch.cells)
        for m in sorted(by_material):
            if m < 18:
                cut, factor = THRESHOLDS[m % 2]
                mat = sb.add_material(int(ch.two_sided), R.ALPHA_MASK, tex[0], first_sampler + m, cut, factor)
            else:
                cut, factor = ch.extra_materials[m - 18]
                mat = sb.add_material(int(ch.two_sided), R.ALPHA_MASK, tex[1], nearest, cut, factor)
            p, uv = [], []
            for n, (c, tri0) in enumerate(by_material[m]):
                p.append(pos[3 * tri0: 3 * tri0 + 6])
                uv.append(np.concatenate([c.uv[list(t)] for t in c.triangles()]))
                c.first_triangle, c.scene_material, c.object = 2 * n, mat, len(sb.obj_prim)
            p = np.concatenate(p)
            prim = ray_deep_cases.meshlet_primitive(p, [np.arange(len(p)).reshape(-1, 3)], (1,))
            prim["texcoords"] = np.concatenate(uv).astype(F)
            sb.prims.append(prim)
            sb.add_object(len(sb.prims) - 1, material=mat)
    scene = sb.build()
    if mutation:
        mutate(scene, cells, mutation)
    L.fill_objects(scene, cam)
    return Built(scene, cam, view, iv, cells, names)
