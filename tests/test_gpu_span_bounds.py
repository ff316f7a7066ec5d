"""GPU: the row-span bounds of the tile kernel (chord_amd/csrc/span_bounds.h) on hand-made triangles whose edges run exactly
through pixel centres, along tile columns 0 and 63, off the target's right edge and far into the guard band -- where a bound
that is one step too tight loses a pixel.  One frame each, bit for bit against the oracle, like tests/test_gpu_parity.py.

The vertices are given in pixels of a 200 x 136 target (right and bottom edges inside a tile, width no multiple of 64), on
half- or quarter-pixel positions, and unprojected through the camera's own matrix; _scene asserts that they project back onto
those positions to well within half a sub-pixel (1 / 512 px), so the snapped 24.8 coordinates are the intended ones.

The int64 edge kind needs a vertex at or beyond 2^25 sub-pixels (131 072 px); the guard band ends at 512.5 target widths, which
is 102 500 px at a width of 200: on that target the far vertices of GUARD give the fp64 kind, and the same triangles are
rendered once more, stretched, on a 328 x 136 target (168 100 px of guard band) as GUARD_328, where they are of the int64 kind."""
import numpy as np
import pytest

import helpers as H
import orc
from chord_amd import records as R
from chord_amd import scenes
from helpers import _unproject

W, HGT = 200, 136
W_WIDE = 328

# ---- triangles, in pixels (x right, y down) ---------------------------------------------------------------------------------
# int32 kind: larger than the tiny threshold (bbox of 8 px), vertices at most 64 px apart
NARROW = [
    ((10.5, 5.5), (40.5, 15.5), (20.5, 35.5)),          # every edge through pixel centres (slopes 1/3, 3, -1)
    ((70.5, 10.5), (70.5, 40.5), (100.5, 40.5)),        # a vertical edge through centres and a horizontal one (zero steps) at the bottom
    ((110.5, 10.5), (150.5, 10.5), (130.5, 45.5)),      # a horizontal edge at the top (top-left rule: covered)
    ((160.5, 5.5), (190.5, 5.5), (190.5, 50.5)),        # vertical on the right
    ((10.25, 70.25), (10.5, 70.25), (58.25, 110.75)),   # a sliver: its middle rows cover no pixel
    ((40.5, 112.5), (64.0, 100.5), (64.0, 130.5)),      # spans that end in column 63 of a tile (vertical edge on the tile border)
    ((64.0, 66.5), (64.0, 96.5), (100.5, 80.5)),        # spans that start in column 0 of a tile
    ((-20.5, 40.5), (30.5, 50.5), (-10.5, 66.5)),       # off the left edge: spans start at the clamp to step 0; crosses a tile border in y
    ((110.5, 60.5), (150.5, 70.5), (120.5, 100.5)),     # across the tile border at x = 128 and y = 64: both in one triangle
    ((170.5, 80.5), (215.5, 95.5), (180.5, 133.5)),     # off the right edge: spans end at pixel column 199 (tile column 7)
    ((130.5, 120.5), (160.5, 118.5), (150.5, 150.5)),   # off the bottom edge
]
# wide kinds: vertices more than 64 px apart
WIDE = [
    ((20.5, 50.5), (230.5, 100.5), (90.5, 130.5)),      # several tiles, ends at pixel column 199
    ((130.5, 2.5), (200.0, 20.5), (140.5, 48.5)),       # a vertex on the target's right edge
    ((5.5, 3.5), (75.5, 3.5), (5.5, 45.5)),             # horizontal and vertical edges through centres, 70 px wide
]
# guard band: vertices far off screen (no plane clips them)
GUARD = [
    ((-60000.5, 30.5), (150.5, 20.5), (70000.5, 60000.5)),
    ((100.5, -65000.5), (180.5, 60.5), (-97000.5, 130.5)),
]
# the same on the 328-px target, a vertex of each beyond 131 072 px (the guard band ends at 69 700 px in y)
GUARD_328 = [
    ((-150000.5, 30.5), (150.5, 20.5), (140000.5, 60000.5)),
    ((100.5, -65000.5), (300.5, 60.5), (-160000.5, 130.5)),
]


def _scene(tris, mode, w=W, h=HGT):
    """mode "pair": every triangle once per winding, one-sided (each copy is drawn where the other is culled: both orientation
    signs, so both assignments of the top-left bias); "two_sided": one copy, alternating windings, two-sided; "masked": as "pair"
    and "two_sided" together under the alpha-tested materials of scenes.masked_test_scene."""
    from chord_amd import lib as L
    cam = scenes.Camera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), w, h)
    view, iv = L.make_views(cam)
    pos = _unproject(view, iv, tris, w, h)
    n = len(tris)
    fwd = np.arange(3 * n, dtype=np.uint32)
    rev = fwd.reshape(n, 3)[:, ::-1].reshape(-1).copy()
    alt = fwd.reshape(n, 3).copy(); alt[1::2] = alt[1::2, ::-1]; alt = alt.reshape(-1)
    flat = np.asarray([v for tri in tris for v in tri], dtype=np.float64)
    uv = np.stack([(flat[:, 0] % 4096.0) / 23.0, (flat[:, 1] % 4096.0) / 17.0], -1).astype(np.float32)
    eye = np.eye(4)
    if mode == "pair":
        scene = scenes.scene_from_meshes([(pos, fwd, uv), (pos, rev, uv)], [eye, eye], two_sided_of_object=[0, 0])
    elif mode == "two_sided":
        scene = scenes.scene_from_meshes([(pos, alt, uv)], [eye], two_sided_of_object=[1])
    else:
        base = scenes.scene_from_meshes([(pos, fwd, uv), (pos, rev, uv), (pos, alt, uv)], [eye, eye, scenes.translate(0.0, 0.0, -0.001)])
        ms, _ = scenes.masked_test_scene()
        objs = base.objects.copy()
        objs["GLTFMaterialData"] = [1, 1, 2]          # one-sided checker (both windings), two-sided noise just behind it
        scene = R.Scene(objs, base.primitives, ms.materials, base.meshlets, base.groups, base.group_indices, base.meshlet_data, base.positions,
                        name="span_masked", texcoord0=base.texcoord0, textures=ms.texture_images, samplers=ms.samplers, bvh_nodes=base.bvh_nodes)
        scene.local_to_world = base.local_to_world
        assert (scene.materials["alphaMode"][[1, 2]] == R.ALPHA_MASK).all()
    L.fill_objects(scene, cam)
    return scene, cam, view, iv


def _frame(scene, cam, view, iv, what, flags=H.ALL_FLAGS):
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
    st = r.stats()
    assert st["overflow"] == 0 and st["trianglesSubmitted"] == want["stats"].trianglesSubmitted
    r.close()
    return want


CASES = [("narrow", NARROW), ("wide", WIDE), ("guard", GUARD), ("all", NARROW + WIDE + GUARD)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["pair", "two_sided"])
@pytest.mark.parametrize("name,tris", CASES, ids=[c[0] for c in CASES])
def test_opaque_spans_match_the_oracle(gpu, name, tris, mode):
    scene, cam, view, iv = _scene(tris, mode)
    want = _frame(scene, cam, view, iv, "%s %s" % (name, mode))
    vis = want["vis"].reshape(HGT, W)
    if name == "narrow":
        # what the shapes are there for, from the oracle's image: pixel centres on the edges through them are covered on the
        # top-left side only; columns 63 / 64 and 199 are reached; the sliver leaves empty rows between covered ones
        assert vis[20, 70] != 0 and vis[40, 80] == 0 and vis[10, 130] != 0            # left edge in, bottom edge out, top edge in
        assert vis[115, 63] != 0 and vis[115, 64] == 0 and vis[80, 64] != 0 and vis[80, 63] == 0
        assert vis[95, 199] != 0 and vis[50, 0] != 0 and vis[135, 150] != 0
        rows = (vis[70:100, 8:48] != 0).any(axis=1)
        assert rows.any() and not rows.all()


@pytest.mark.gpu
def test_guard_band_triangles_of_the_int64_kind(gpu):
    """GUARD_328 on a 328 x 136 target: vertices beyond 2^25 sub-pixels, inside the guard band."""
    scene, cam, view, iv = _scene(GUARD_328 + NARROW[:2], "pair", W_WIDE, HGT)
    _frame(scene, cam, view, iv, "guard 328")
    scene, cam, view, iv = _scene(GUARD_328 + NARROW[:2], "two_sided", W_WIDE, HGT)
    _frame(scene, cam, view, iv, "guard 328 two-sided")


@pytest.mark.gpu
def test_floor_under_camera_at_the_same_size(gpu):
    """scenes.floor_under_camera: clipped triangles whose vertices the clipper leaves on the guard band."""
    scene, cam, view, iv = H.setup_scene(lambda: scenes.floor_under_camera(width=W, height=HGT))
    _frame(scene, cam, view, iv, "floor_under_camera")
    scene, cam, view, iv = H.setup_scene(lambda: scenes.floor_under_camera(width=W_WIDE, height=HGT))
    _frame(scene, cam, view, iv, "floor_under_camera 328")


@pytest.mark.gpu
@pytest.mark.parametrize("name,tris,w", [("narrow", NARROW, W), ("wide", WIDE + GUARD, W), ("guard_328", GUARD_328 + NARROW[:2], W_WIDE)],
                         ids=["narrow", "wide", "guard_328"])
def test_masked_spans_match_the_oracle(gpu, name, tris, w):
    """The same triangles alpha-tested: masked_rows<int32_t> (vertices at most 64 px apart) and masked_rows<int64_t>."""
    scene, cam, view, iv = _scene(tris, "masked", w, HGT)
    want = _frame(scene, cam, view, iv, "masked " + name)
    assert want["stats"].fragmentsClipped > 0, "no fragment failed the alpha test"


@pytest.mark.gpu
@pytest.mark.parametrize("clamp,bias", [(True, (0.0, 0.0)), (True, (-48.0, -1.25)), (False, (0.0, 0.0))], ids=["clamped", "clamped_biased", "unclamped"])
def test_depth_only_view_of_the_same_meshes(gpu, clamp, bias):
    """The DEPTH instantiation (cull mode none, clamp, bias) through the entry points of tests/test_depth_views.py: a square
    depth view of 136 texels (two tiles and 8 texels each way) looking at NARROW + WIDE + GUARD placed for that view."""
    from chord_amd.renderer import VisibilityRenderer
    dim = HGT
    tris = [t for t in NARROW + WIDE + GUARD]
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
    target = r.render_mesh_depth(0, lst, clamp, bias[0], bias[1])
    want, st = orc.raster_depth(scene, views[0:1], want_cmds, dim, dim, clamp, bias[0], bias[1])
    assert (want > 0).sum() > 100
    got = r.read_depth(target)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert len(bad) == 0, "%d texels differ, first %d: %r vs %r" % (len(bad), bad[0], got[bad[0]], want[bad[0]])
    assert r.depth_view_stats()["overflow"] == 0
    r.close()
