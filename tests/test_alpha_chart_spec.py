"""The sampler charts of tests/alpha_chart.py against the oracle alone: every cell takes the level and the filter it is named for
(census), shows both outcomes of the alpha test, and differs in at least one pixel when its sampler is wrong in one respect
(discrimination) -- so a kernel that is wrong in one wrap mode, one filter or one level cannot give the oracle's image of the chart.
CPU only; the kernels are held to these images by tests/test_gpu_alpha_chart.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import alpha_chart as A
import helpers as H
import orc
from chord_amd import records as R


@functools.lru_cache(maxsize=None)
def _frame(name, mutation=None):
    b = A.build(name, mutation=mutation)
    want = orc.frame(b.scene, b.view, b.iv, H.ALL_FLAGS)
    return b, want, b.object_image(want["vis"], want["cmds"])


def test_charts_hold_what_they_claim():
    """The cases by count and the level shapes by name, from the chart tables themselves."""
    for name in A.CHART_NAMES[:-1]:
        cells = A.chart(name).cells
        grid = {(c.material, c.want[0]) for c in cells}
        assert {m for m, _ in grid} == set(range(18)), name                          # nine wrap pairs x two filter pairs
        for m in range(18):
            last = 1 if name == "16383x2" else A.mip_count(*cells[0].dims) - 1          # (16383x2: levels 0 and 1 only)
            assert (m, (0, "mag")) in grid and (m, (0, "min")) in grid and (m, (last, "min")) in grid, (name, m)
    dims = lambda name: sorted({c.level_dims(0) for c in A.chart(name).cells}, reverse=True)
    assert dims("64x64") == [(64, 64), (32, 32), (16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    assert dims("37x21") == [(37, 21), (18, 10), (9, 5), (4, 2), (2, 1), (1, 1)]
    assert dims("1x9") == [(1, 9), (1, 4), (1, 2), (1, 1)] and dims("9x1") == [(9, 1), (4, 1), (2, 1), (1, 1)]
    assert dims("16383x2") == [(16383, 2), (8191, 1)]
    assert dims("16384x1") == [(16384, 1), (128, 1), (2, 1), (1, 1)]
    b = A.build("16384x1")
    assert b.scene._textures[0].mipCount == 15 and A.mip_count(16383, 2) == 14
    labels = {c.label for c in A.chart("64x64_edges").cells}
    assert {"ratio 1", "ratio 1 - ulp", "ratio 4", "ratio 4 - ulp", "factor 1", "factor 0.9", "u W = 1e9 - ulp", "u W = 1e9", "u W = 1e9 + ulp",
            "u W = -(1e9 - ulp)", "u W = -1e9", "u W = -(1e9 + ulp)", "u W = 2e9", "u W = 64e30", "u(C) = +inf", "u(C) = -inf", "u(C) = NaN",
            "v(B) = +inf", "v(B) = -inf", "v(B) = NaN"} <= labels
    # both windings on the two-sided charts, one on the others
    for name in A.CHART_NAMES:
        ch = A.chart(name)
        assert {c.flip for c in ch.cells} == ({False, True} if ch.two_sided else {False}), name
    assert sum(A.chart(n).two_sided for n in A.CHART_NAMES) == 3


@pytest.mark.parametrize("name", A.CHART_NAMES)
def test_census_every_triangle_takes_the_level_and_filter_its_cell_is_named_for(name):
    b, want, _ = _frame(name)
    lin = C.c_int(-1)
    assert len(b.cells) >= 38
    for c in b.cells:
        x0, y0 = c.rect
        assert x0 >= 0 and y0 >= 0 and x0 + A.P <= b.width and y0 + A.P <= b.height
        mat = b.scene.materials[c.scene_material:c.scene_material + 1].copy()
        for t, tri in enumerate(c.triangles()):
            px = np.asarray([c.corners()[k] for k in tri], dtype=np.int64) * 256
            area2 = (px[1, 0] - px[0, 0]) * (px[2, 1] - px[0, 1]) - (px[2, 0] - px[0, 0]) * (px[1, 1] - px[0, 1])
            assert abs(int(area2)) == A.AREA2 and (area2 < 0) != c.flip                   # front faces have negative area
            u, v = np.ascontiguousarray(c.uv[list(tri), 0]), np.ascontiguousarray(c.uv[list(tri), 1])
            level = orc.lib.orc_mask_level(C.byref(b.scene.desc), mat.ctypes.data, A.AREA2, u.ctypes.data, v.ctypes.data, C.byref(lin))
            assert (level, lin.value) == (c.want[t][0], c.linear(t)), (c.name, t, level, lin.value)
    # the frame drew every cell's triangles and the backdrop's
    assert want["stats"].trianglesSubmitted == 2 * len(b.cells) + 2


@pytest.mark.parametrize("name", A.CHART_NAMES)
def test_both_outcomes_of_the_alpha_test(name):
    """Every cell whose levels have at least 4 texels keeps some pixels and loses some to the backdrop; cells of smaller levels do
    so over their (texture, level) group."""
    b, want, obj = _frame(name)
    groups = {}
    for c in b.cells:
        px = b.pixels(c, obj)
        kept, lost = px == c.object, px == 0
        assert (kept | lost).all(), c.name
        if c.texels() >= 4:
            assert kept.any() and lost.any(), (c.name, int(kept.sum()), int(lost.sum()))
        else:
            g = groups.setdefault((c.texture, max(c.want[0][0], c.want[1][0])), [False, False])
            g[0], g[1] = g[0] or bool(kept.any()), g[1] or bool(lost.any())
    assert all(k and l for k, l in groups.values()), groups
    assert want["stats"].fragmentsClipped > 0


def test_cut_off_keeps_the_equal_byte_and_clips_the_one_below():
    b, want, obj = _frame("64x64_edges")
    cells = [c for c in b.cells if c.group == "cutoff"]
    assert len(cells) == 2
    byte = np.arange(256).reshape(16, 16)                     # the byte pixel (x, y) of the cell samples: 16 y + x
    for c in cells:
        kept = b.pixels(c, obj) == c.object
        assert kept[byte == A.CUTOFF_BYTE].all() and not kept[byte == A.CUTOFF_BYTE - 1].any(), c.name
        assert np.array_equal(kept, byte >= A.CUTOFF_BYTE), c.name
    (cut_a, fac_a), (cut_b, fac_b) = A.cutoff_values()
    tap = np.float32(A.CUTOFF_BYTE) * np.float32(1.0 / 255.0)
    assert np.float32(tap * np.float32(fac_a)) - np.float32(cut_a) == 0 and np.float32(tap * np.float32(fac_b)) - np.float32(cut_b) == 0


@pytest.mark.parametrize("name,mutation", [(n, m) for n in A.CHART_NAMES for m in A.MUTATIONS if m != "cutoff" or n == "64x64_edges"])
def test_a_wrong_sampler_changes_every_affected_cell(name, mutation):
    """One mutation at a time -- wrapS or wrapT to the next mode, min and mag filter exchanged, the cut-off one ulp up --: every cell
    the mutation bears on (alpha_chart.Cell.affected states the exemptions) differs from the unmutated image in at least one pixel."""
    b, want, _ = _frame(name)
    affected = [c for c in b.cells if c.affected(mutation)]
    if mutation in ("wrapS", "wrapT") and b.cells[0].dims[mutation == "wrapT"] == 1:
        assert not affected                                   # (a texture one texel wide on that axis has no wrap to get wrong)
        return
    assert len(affected) == 2 if mutation == "cutoff" else len(affected) >= len(b.cells) // 3
    mb, mwant, _ = _frame(name, mutation)
    same = [c.name for c, mc in zip(b.cells, mb.cells) if c.affected(mutation) and np.array_equal(b.pixels(c, want["vis"]), mb.pixels(mc, mwant["vis"]))]
    assert not same, "%s: %d of %d affected cells look the same under a mutated %s: %s" % (name, len(same), len(affected), mutation, same[:6])


def test_the_two_chart_scene_and_the_depth_view_scene_draw_their_cells():
    """The scenes of the two further GPU tests, on the oracle: every cell of both bands is drawn and alpha-tested with its own
    chart's material (the kept pixels carry its object), and the square 192-texel depth view holds the 90 cells of its chart."""
    b = A.build(("64x64", "37x21"))
    want = orc.frame(b.scene, b.view, b.iv, H.ALL_FLAGS)
    obj = b.object_image(want["vis"], want["cmds"])
    assert b.scene.desc.textureCount == 2 and want["stats"].trianglesSubmitted == 2 * 216 + 2
    for c in b.cells:
        px = b.pixels(c, obj)
        assert ((px == c.object) | (px == 0)).all() and (c.texels() < 4 or ((px == c.object).any() and (px == 0).any())), c.name
        assert b.scene.materials["baseColorId"][c.scene_material] == (c.chart == "37x21")
    d = A.build("37x21_short", width=A.HEIGHT, height=A.HEIGHT, gap=3)
    flags = R.FLAG_FRUSTUM_CULL | R.FLAG_CONE_CULL
    cmds = orc.instance_culling(d.scene, d.view, d.iv[0:1], flags)
    depth, st = orc.raster_depth(d.scene, d.iv[0:1], cmds, A.HEIGHT, A.HEIGHT, True, 0.0, 0.0)
    assert len(d.cells) == 90 and st.trianglesSubmitted == 182 and st.fragmentsClipped > 0
    back = depth.reshape(A.HEIGHT, A.HEIGHT)[0, 0]                # the backdrop's depth (reverse z: nearer is larger)
    for c in d.cells:
        px = d.pixels(c, depth)
        kept = px > 1.3 * back                                    # (the backdrop is 16 units away, the farthest cell under 8)
        assert (px > 0.9 * back).all() and (c.texels() < 4 or (kept.any() and not kept.all())), c.name


def test_first_difference_names_the_cell():
    b, want, _ = _frame("37x21")
    assert b.first_difference(want["vis"], want["vis"]) == ""
    c = b.cells[40]
    got = want["vis"].copy().reshape(b.height, b.width)
    got[c.rect[1] + 3, c.rect[0] + 5] ^= np.uint64(1)
    msg = b.first_difference(got, want["vis"])
    assert c.name in msg and "x=%d, y=%d" % (c.rect[0] + 5, c.rect[1] + 3) in msg
