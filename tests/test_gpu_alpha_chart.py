"""GPU: the raster's alpha test (raster_device.h mask_level_filter / write_mask_ext / alpha_level / sample_alpha, texel_wrap.h,
the DMatLevel table of chordvis_upload_scene) on the sampler charts of tests/alpha_chart.py: every (wrapS, wrapT) pair under both
filter pairs, at the levels, level shapes and periods the charts name, at the level boundaries, at equality with the cut-off and
at wild texture coordinates.  One 256 x 192 frame per chart, bit for bit against the oracle; tests/test_alpha_chart_spec.py shows
on the CPU that every cell takes the case it is named for and that a sampler wrong in one respect changes the oracle's image."""
import numpy as np
import pytest

import alpha_chart as A
import helpers as H
import orc
from chord_amd import records as R

pytestmark = pytest.mark.gpu


def _render(b, flags=H.ALL_FLAGS):
    from chord_amd.renderer import VisibilityRenderer
    want = orc.frame(b.scene, b.view, b.iv, flags)
    assert want["stats"].fragmentsClipped > 0 and want["stats"].trianglesSubmitted == 2 * len(b.cells) + 2
    r = VisibilityRenderer(0)
    try:
        r.upload_scene(b.scene)
        r.allocate_gbuffer(b.width, b.height)
        r.set_view(b.view, b.iv, flags)
        r.render_frame()
        got = r.read_visibility()
        st = r.stats()
    finally:
        r.close()
    diff = b.first_difference(got, want["vis"])
    assert not diff, "%s: %s" % (b.what, diff)
    H.assert_vis_equal(got, want["vis"], b.width, b.height, b.what)
    assert st["overflow"] == 0 and st["trianglesSubmitted"] == want["stats"].trianglesSubmitted


@pytest.mark.parametrize("name", A.CHART_NAMES)
def test_chart_matches_the_oracle(gpu, name):
    _render(A.build(name))


def test_two_charts_in_one_scene(gpu):
    """64x64 and 37x21 in one scene, one band of the target each: a texture table of two, two charts' materials and samplers, and
    level bases (DMatLevel::base) of the second texture that do not start at 0."""
    b = A.build(("64x64", "37x21"))
    assert b.height == 2 * A.HEIGHT and len(b.scene.texture_images) == 2 and len(b.cells) == 216
    assert {c.scene_material for c in b.cells if c.chart == "37x21"}.isdisjoint(c.scene_material for c in b.cells if c.chart == "64x64")
    _render(b)


def test_37x21_chart_through_a_depth_only_view(gpu):
    """The MASKED x DEPTH instantiation through the entry points of test_gpu_span_bounds.py::test_depth_only_view_of_the_same_meshes:
    a square depth view of 192 texels.  (The chart without its two extra levels per material, and 3 texels between cells instead of
    4: 90 cells on 192 x 192.)"""
    from chord_amd.renderer import VisibilityRenderer
    dim = A.HEIGHT
    b = A.build("37x21_short", width=dim, height=dim, gap=3)
    assert len(b.cells) == 90 and b.scene.materials["bTwoSided"][1:].all()
    flags = R.FLAG_FRUSTUM_CULL | R.FLAG_CONE_CULL
    views = b.iv.copy()
    want_cmds = orc.instance_culling(b.scene, b.view, views[0:1], flags)
    want, st = orc.raster_depth(b.scene, views[0:1], want_cmds, dim, dim, True, 0.0, 0.0)
    assert st.fragmentsClipped > 0 and (want > 0).sum() > 100
    r = VisibilityRenderer(0)
    try:
        r.upload_scene(b.scene)
        r.allocate_gbuffer(dim, dim)
        r.set_view(b.view, b.iv, flags)
        r.allocate_depth_views(dim, 1)
        r.set_instance_views(views)
        lst = r.instance_culling_view(0)
        assert np.array_equal(H.sort_cmds(r.read_cmds(lst)), H.sort_cmds(want_cmds))
        target = r.render_mesh_depth(0, lst, True, 0.0, 0.0)
        got = r.read_depth(target)
        overflow = r.depth_view_stats()["overflow"]
    finally:
        r.close()
    diff = b.first_difference(got.view(np.uint32), want.view(np.uint32))
    assert not diff, "depth view: " + diff
    assert overflow == 0
