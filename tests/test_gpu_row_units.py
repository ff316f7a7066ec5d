"""GPU: the tile kernel's row units -- how an entry's units are listed (list_units and the masked listing, one unit per pixel row),
the span bounds of a row, the two-pixel trips of the int32 scan -- on hand-made triangles, one frame each, word for word against
the oracle (visibility image and HZB), in the manner of tests/test_gpu_span_bounds.py, whose scene builder this file uses.

The cases run whatever library is built.  The product lists one unit per pixel row of an entry (the segment of the unit word is
always 0: a row of the 64-pixel tile is one segment) and keeps the ladder form of the bounds and per-unit reciprocals.  The variant
with an entry's step reciprocals stored once (three more entry words, a 16-bit unit list: what the two-batch case was written for)
was rejected and its code is in the history at commit bb3c4eb (profiles/r11_row_units.txt); the measurement variant
-DSPAN_STRAIGHT=1 (the bounds as selects) is covered by these cases only when the library is built with its switch.

Targets of a few tiles whose right and bottom tiles are cut: 136 x 72 (3 x 2 tiles, 8 columns and 8 rows in the last ones) and
328 x 136 (6 x 3).  The shapes are given tile-local, in pixels, and placed at several tile origins:
  ZERO     exactly horizontal and exactly vertical edges (zero steps of the row loop), on and between pixel centres
  SLIVERS  spans that are empty on some rows and one pixel on others
  ENDS     rows that start at even and at odd local x and end at local x = 62 and 63: the second pixel of a two-pixel trip then
           falls on the row's padding word, in the next tile or right of the screen
  CROWD    one tile with more than 512 row-unit entries (two batches) of which one batch holds more than 4 096 units (two rounds
           of the unit list): whole-tile triangles of the wide kinds, large and small ones of the int32 kind among them, so that
           int32 entries sit at every position of both batches and their units in both rounds."""
import numpy as np
import pytest

import helpers as H
import orc
from chord_amd import records as R
from test_gpu_span_bounds import _scene

SMALL = (136, 72)
WIDE = (328, 136)

# ---- shapes, tile-local pixels (x right, y down); every one larger than the tiny threshold (a bbox of 8 px) -------------------
ZERO = [
    ((4.5, 3.5), (34.5, 3.5), (4.5, 23.5)),             # horizontal top edge and vertical left edge through pixel centres
    ((40.0, 2.0), (60.0, 2.0), (60.0, 22.0)),           # horizontal top, vertical right, between centres
    ((6.5, 30.5), (6.5, 50.5), (30.5, 50.5)),           # vertical left, horizontal bottom (top-left rule: bottom row out)
    ((36.25, 28.75), (58.25, 40.5), (36.25, 52.25)),    # one vertical edge on a quarter pixel
    ((10.5, 56.5), (50.5, 56.5), (30.5, 62.5)),         # a flat one: horizontal edge, six rows
]
SLIVERS = [
    ((2.25, 2.25), (2.5, 2.25), (50.25, 40.75)),        # long and thin: its middle rows cover no pixel
    ((60.25, 3.75), (61.0, 3.5), (12.25, 60.25)),       # the other diagonal
    ((3.25, 60.25), (58.75, 57.5), (58.75, 57.75)),     # nearly horizontal: most of its columns on one or two rows
    ((20.25, 10.25), (21.0, 10.25), (20.75, 55.5)),     # nearly vertical: one pixel per row, or none
]
ENDS = [
    ((10.0, 4.5), (64.0, 16.5), (10.0, 28.5)),          # rows start at local x 10 (even); the tip reaches column 63
    ((11.0, 30.5), (64.0, 40.5), (11.0, 50.5)),         # ... at 11 (odd)
    ((20.5, 2.5), (63.0, 2.5), (63.0, 30.5)),           # vertical edge at 63.0: rows end at column 62, starts of both parities
    ((21.5, 34.5), (64.0, 34.5), (64.0, 62.5)),         # vertical edge at 64.0: rows end at column 63
    ((1.0, 40.5), (63.0, 52.5), (2.0, 63.5)),           # rows of odd and even length from column 1
]


def _placed(shapes, origins):
    return [tuple((x + ox, y + oy) for (x, y) in tri) for (ox, oy) in origins for tri in shapes]


def _shapes(w, h):
    """ZERO, SLIVERS and ENDS at the first tile, at the tile left of the cut column (ENDS then end against the cut tile) and
    shifted so that they run into the cut right column / bottom row of the target and off its edges."""
    tx, ty = (w // 64 - 1) * 64, (h // 64 - 1) * 64
    tris = _placed(ZERO + SLIVERS + ENDS, [(0, 0), (tx, ty)])
    tris += _placed(ENDS + ZERO[:2], [(w - 40, 0), (tx, h - 36)])            # through the cut tiles, off the right / bottom edge
    return tris


def _crowd():
    """For tile (0, 0): 100 triangles that cover it whole (vertices more than 64 px apart: the wide kinds, 64 units each), 30 large
    int32-kind triangles (60 rows each) and 420 small ones (5-6 rows) in layers on a 10 x 10 grid, interleaved in mesh order."""
    big = [((-70.5 + 0.25 * (k % 7), -10.5), (140.5, -12.5 + 0.5 * (k % 5)), (30.5 + k % 3, 200.5)) for k in range(100)]
    large = [((2.5 + 0.25 * (k % 4), 2.5), (62.5, 4.5 + 0.5 * (k % 6)), (4.5, 62.5 - 0.25 * (k % 8))) for k in range(30)]
    small = []
    for k in range(420):
        x, y = 1.0 + 6.0 * (k % 10), 1.0 + 6.0 * ((k // 10) % 10)
        j = 0.25 * (k // 100)
        small.append(((x + 0.25 + j, y + 0.25), (x + 5.25, y + 0.75 + j), (x + 1.75 - j, y + 5.25)))
    tris, n = [], max(len(big), len(large), len(small))
    for k in range(n):                                   # interleaved: every kind at every position of the bin
        for lst, every in ((small, 1), (big, 4), (large, 14)):
            if k % every == 0 and k // every < len(lst):
                tris.append(lst[k // every])
    for lst in (small, big, large):
        assert all(t in tris for t in lst)
    return tris


def _tile0_load(tris):
    """(row-unit entries, units) of tile (0, 0) by the tile kernel's rules: clipped bbox of more than 8 px, one unit per row."""
    entries = units = 0
    for tri in tris:
        xs, ys = [v[0] for v in tri], [v[1] for v in tri]
        x0, x1 = max(int(np.ceil(min(xs) - 0.5)), 0), min(int(np.ceil(max(xs) - 0.5)) - 1, 63)
        y0, y1 = max(int(np.ceil(min(ys) - 0.5)), 0), min(int(np.ceil(max(ys) - 0.5)) - 1, 63)
        if x1 >= x0 and y1 >= y0 and (x1 - x0 + 1) * (y1 - y0 + 1) > 8:
            entries += 1
            units += y1 - y0 + 1
    return entries, units


def _assert_two_batches_two_rounds(tris, copies=1):
    """Tile (0, 0) under `tris`, every triangle drawn `copies` times (the scene modes draw one, two or three): 513 .. 1 023 entries
    (two batches; below the threshold at which the tiny-triangle area grows), and so many units that one of the two batches holds
    more than 4 096 of them however the entries fall (one of two holds at least half)."""
    entries, units = _tile0_load(tris)
    entries, units = entries * copies, units * copies
    assert 512 < entries < 1024, entries
    assert (units + 1) // 2 > 4096, (entries, units)


def test_crowd_fills_two_batches_and_two_rounds():
    """The meshes of the CROWD cases are what they claim by the kernel's own arithmetic (no GPU), in every mode they are drawn
    in: opaque and sharded (one entry per triangle), masked (two: a one-sided copy and the two-sided one behind it) and the
    depth view (cull mode none: the two one-sided copies and the two-sided one, and two should a copy be culled)."""
    _assert_two_batches_two_rounds(_crowd())
    _assert_two_batches_two_rounds(_shapes(*SMALL) + _crowd())
    _assert_two_batches_two_rounds(_crowd()[::2], 2)
    for copies in (2, 3):
        _assert_two_batches_two_rounds(_shapes(136, 136) + _crowd()[::2], copies)


def test_shapes_are_what_they_are_there_for():
    """Each group alone through the oracle (no GPU; together they overlap and hide one another's edges): pixel centres on the
    zero-step edges are covered on the top-left side only, rows end at columns 62 and 63 and start at even and odd x, the slivers
    leave rows of no pixel between rows of one."""
    w, h = SMALL

    def image(shapes):
        scene, cam, view, iv = _scene(shapes, "pair", w, h)
        return orc.frame(scene, view, iv, H.ALL_FLAGS)["vis"].reshape(h, w) != 0
    vis = image(ZERO)
    assert vis[3, 4] and not vis[3, 3] and vis[3, 33] and not vis[3, 34] and not vis[2, 10]        # top and left edge in, the far vertex out
    assert vis[49, 6] and not vis[49, 5] and not vis[50, 10]                                       # left edge in, bottom edge out
    assert vis[2, 40] and vis[2, 59] and not vis[2, 60] and not vis[1, 50]                         # edges between centres
    vis = image(ENDS)
    assert vis[10, 62] and not vis[10, 63] and vis[40, 63] and not vis[40, 64]                     # rows that end at column 62 and at 63
    assert vis[10, 10] and not vis[10, 9] and vis[40, 11] and not vis[40, 10]                      # ... that start at even and at odd x
    starts = np.argmax(vis[3:30, 20:64], axis=1)
    assert (starts % 2 == 0).any() and (starts % 2 == 1).any()
    vis = image(SLIVERS)
    per_row = vis[11:55, 19:23].sum(axis=1)                                                        # the nearly vertical one
    assert (per_row == 0).any() and (per_row == 1).any() and per_row.max() <= 2
    per_row = vis[3:40, 0:52].sum(axis=1)                                                          # the long thin one
    assert (per_row == 0).any() and (per_row == 1).any()


def _frame(scene, cam, view, iv, what, flags=H.ALL_FLAGS):
    """One frame against the oracle: visibility words, both HZB chains, the valid range."""
    from chord_amd.renderer import VisibilityRenderer
    w, h = cam.width, cam.height
    want = orc.frame(scene, view, iv, flags)
    assert (want["vis"] != 0).sum() > 100, what + ": the oracle's frame is all but empty"
    r = VisibilityRenderer(0)
    r.upload_scene(scene)
    r.allocate_gbuffer(w, h)
    r.set_view(view, iv, flags)
    r.render_frame()
    H.assert_vis_equal(r.read_visibility(), want["vis"], w, h, what)
    mn, mx, rng = r.read_hzb(r.history_hzb())
    assert np.array_equal(mn, want["hzb_min"]) and np.array_equal(mx, want["hzb_max"]) and np.array_equal(rng, want["valid_range"]), what + ": HZB"
    st = r.stats()
    assert st["overflow"] == 0 and st["trianglesSubmitted"] == want["stats"].trianglesSubmitted
    r.close()
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["pair", "two_sided"])
@pytest.mark.parametrize("dims", [SMALL, WIDE], ids=["136x72", "328x136"])
def test_zero_steps_slivers_and_row_ends_match_the_oracle(gpu, dims, mode):
    """(a), (b), (c): both windings one-sided ("pair": each orientation sign, so both assignments of the top-left bias) and
    alternating windings two-sided."""
    w, h = dims
    scene, cam, view, iv = _scene(_shapes(w, h), mode, w, h)
    _frame(scene, cam, view, iv, "shapes %dx%d %s" % (w, h, mode))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["pair", "two_sided"])
def test_two_batches_and_two_unit_rounds_match_the_oracle(gpu, mode):
    """(d) on 136 x 72: tile (0, 0) runs two batches (the second rewrites the entry words and the unit list of the first), and
    units 4 096 .. of the full batch go through a unit list that was written twice."""
    w, h = SMALL
    _assert_two_batches_two_rounds(_crowd())
    scene, cam, view, iv = _scene(_crowd(), mode, w, h)
    _frame(scene, cam, view, iv, "crowd " + mode)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["shapes", "crowd"])
def test_masked_instantiation_on_the_same_meshes(gpu, name):
    """(e) masked: the meshes under alpha-tested materials (masked_rows through the same list and the same bounds), beside opaque
    units of the same batch where the material keeps everything."""
    w, h = SMALL
    tris = _shapes(w, h) if name == "shapes" else _crowd()[::2]
    if name == "crowd":
        _assert_two_batches_two_rounds(tris, 2)         # (every second triangle: masked mode draws each twice)
    scene, cam, view, iv = _scene(tris, "masked", w, h)
    want = _frame(scene, cam, view, iv, "masked " + name)
    assert want["stats"].fragmentsClipped > 0, "no fragment failed the alpha test"


@pytest.mark.gpu
@pytest.mark.parametrize("clamp", [True, False], ids=["clamped", "unclamped"])
def test_depth_instantiation_on_the_same_meshes(gpu, clamp):
    """(e) depth: a square depth-only view of 136 texels (two tiles and 8 texels each way) on the shapes and half the crowd,
    through the entry points of tests/test_depth_views.py."""
    from chord_amd.renderer import VisibilityRenderer
    dim = 136
    tris = _shapes(dim, dim) + _crowd()[::2]
    _assert_two_batches_two_rounds(tris, 2)             # (the scene's three copies of a triangle: at least two are drawn)
    scene, cam, view, iv = _scene(tris, "masked", dim, dim)
    flags = R.FLAG_FRUSTUM_CULL | R.FLAG_CONE_CULL
    views = iv.copy()
    r = VisibilityRenderer(0)
    r.upload_scene(scene)
    r.allocate_gbuffer(dim, dim)
    r.set_view(view, iv, flags)
    r.allocate_depth_views(dim, 1)
    r.set_instance_views(views)
    lst = r.instance_culling_view(0)
    want_cmds = orc.instance_culling(scene, view, views[0:1], flags)
    assert np.array_equal(H.sort_cmds(r.read_cmds(lst)), H.sort_cmds(want_cmds))
    target = r.render_mesh_depth(0, lst, clamp, 0.0, 0.0)
    want, st = orc.raster_depth(scene, views[0:1], want_cmds, dim, dim, clamp, 0.0, 0.0)
    assert (want > 0).sum() > 100
    got = r.read_depth(target)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert len(bad) == 0, "%d texels differ, first %d: %r vs %r" % (len(bad), bad[0], got[bad[0]], want[bad[0]])
    assert r.depth_view_stats()["overflow"] == 0
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tile_map", ["default", "checker"])
def test_sharded_instantiation_on_the_same_meshes(gpu, tile_map):
    """(e) sharded: two ranks on one device (the all-gathers as device-to-device copies, helpers.sharded_frame), the shapes and the
    whole crowd (one entry per triangle: the owner of tile (0, 0) runs two batches and two unit rounds on it); every rank ends with
    the oracle's image and HZB."""
    w, h = SMALL
    tris = _shapes(w, h) + _crowd()
    _assert_two_batches_two_rounds(tris)
    scene, cam, view, iv = _scene(tris, "pair", w, h)
    want = orc.frame(scene, view, iv, H.ALL_FLAGS)
    ctxs = H.sharded_contexts(scene, view, iv, w, h, H.ALL_FLAGS, 2, tile_map)
    H.sharded_frame(ctxs, sharded_cull=False)
    for rk, r in enumerate(ctxs):
        H.assert_vis_equal(r.read_visibility(), want["vis"], w, h, "rank %d" % rk)
        mn, mx, rng = r.read_hzb(r.history_hzb())
        assert np.array_equal(mn, want["hzb_min"]) and np.array_equal(mx, want["hzb_max"]) and np.array_equal(rng, want["valid_range"])
        assert r.stats()["overflow"] == 0
    for r in ctxs:
        r.close()
