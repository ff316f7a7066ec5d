"""Every consumer of chordvis_upload_scene's concatenation on a scene of SEVERAL assets (tests/multi_asset.py: three assets of different
sizes, objects and primitives interleaved, so no base but the first asset's is 0), held exactly -- uint32 views, no tolerance -- to
the oracle and the numpy specifications on the scene's one-asset twin.  The only translation is MultiAssetScene.to_asset_relative /
to_concatenated where the ABI says a record is asset-relative: ChordDrawCmd::meshletId as chordvis_readback_cmds returns it and
ChordRayHit::meshlet.  tests/test_multi_asset_spec.py holds on the CPU that these comparisons can fail and that their inputs are not
empty."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import multi_asset as MA
import orc
import pixel_rays_cases as PC
import spec_geometry_feedback_np as SGF
import spec_material_feedback_np as SF
import spec_material_np as SM
import spec_pixel_rays_np as PR
import spec_ray_shade_np as RS
import spec_rays_np as S
import spec_resolve_np as SR
import spec_surface_np as SS
import test_gpu_gbuffer as TG
from chord_amd import lib as L, records as R
from test_depth_views import LIGHT

pytestmark = pytest.mark.gpu
u32, f32 = np.uint32, np.float32
FW, FH = MA.FW, MA.FH


def _setup(builder=MA.three_assets):
    ms, cam = builder()
    view, iv = MA.filled(ms, cam)
    return ms, cam, view, iv


def _renderer(scene, w=0, h=0, textures=False, store=None, cull_mode=0):
    from chord_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(0)
    if store is not None:
        r.set_material_texture_store(store)
    r.upload_scene(scene)
    if textures:
        r.upload_material_textures()
    if w:
        r.allocate_gbuffer(w, h)
    if cull_mode:
        r.set_cull_mode(cull_mode)
    return r


def _refused(call, match):
    with pytest.raises(L.ChordvisError, match=match):
        call()


def _check_frame(r, ms, want, what, with_stats=True, objects=None):
    """tests/test_gpu_cull_paths.py's _check_frame with the one translation: the read-back list is asset-relative, the oracle's list on
    the twin concatenated.  Returns the read-back list."""
    H.assert_vis_equal(r.read_visibility(), want["vis"], FW, FH, what)
    got = r.read_cmds(r.last_frame_cmds())
    rel = ms.to_asset_relative(want["cmds"], objects)
    assert len(got) == len(rel), "%s: list 0 (%d vs %d commands)" % (what, len(got), len(rel))
    if not np.array_equal(got, rel):
        k = int(np.flatnonzero(got != rel)[0])
        raise AssertionError("%s: list 0 differs at %d records; first %d: got %r want %r (concatenated %r)"
                             % (what, (got != rel).sum(), k, got[k], rel[k], want["cmds"][k]))
    if with_stats:
        st = r.stats()
        counts = [st["countInstanceCulled"], st["countStage0Visible"], st["countStage0Rejected"], st["countStage1Visible"]]
        assert counts == [int(c) for c in want["counts"]], "%s: stage counts %s, oracle %s" % (what, counts, list(want["counts"]))
        assert st["trianglesSubmitted"] == want["stats"].trianglesSubmitted and st["overflow"] == 0, what
        mn, mx, rng = r.read_hzb(r.history_hzb())
        assert np.array_equal(mn, want["hzb_min"]), what + ": history HZB min"
        assert np.array_equal(mx, want["hzb_max"]), what + ": history HZB max"
        assert np.array_equal(rng, want["valid_range"]), what + ": history valid range"
    return got


def _list_is_telling(ms, got, want_cmds, objects=None):
    """Every asset is in the list, and for assets 1 and 2 the asset-relative id is another number than the concatenated one."""
    objs = ms.objects if objects is None else objects
    own = ms.asset_of_primitive[objs["GLTFPrimitiveDetail"][got["objectId"]].astype(np.int64)]
    assert all((own == a).sum() > 20 for a in range(1, 3)), np.bincount(own, minlength=3)
    assert (got["meshletId"][own > 0] != want_cmds["meshletId"][own > 0]).all()
    return own


# ---- 1. frames -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cull_mode", [0, 1], ids=["flat", "hierarchical"])
def test_two_frames_equal_the_oracle(gpu, cull_mode):
    """Frame 0 without a history, frame 1 under a moved camera with frame 0's chain: visibility words, the read-back command list
    (chordvis_readback_cmds' subtraction of DPrim::assetMeshletBase, here with bases that are not 0), stage counts and the HZB chain."""
    ms, cam, view, iv = _setup()
    r = _renderer(ms, FW, FH, cull_mode=cull_mode)
    try:
        r.set_view(view, iv, H.ALL_FLAGS)
        want0 = orc.frame(ms.spec, view, iv, H.ALL_FLAGS)
        r.render_frame()
        got = _check_frame(r, ms, want0, "frame 0", with_stats=False)
        own = _list_is_telling(ms, got, want0["cmds"])
        assert (own == 0).sum() > 20
        cam1 = cam.moved((0.15, 0.05, -0.1))
        L.fill_objects(ms, cam1, cam)
        view1, iv1 = L.make_views(cam1, view)
        r.update_objects(ms.objects)
        r.set_view(view1, iv1, H.ALL_FLAGS)
        want1 = orc.frame(ms.spec, view1, iv1, H.ALL_FLAGS, prev_hzb_min=want0["hzb_min"])
        assert want1["counts"][2] > 0 or want1["counts"][3] > 0 or want1["counts"][1] < want1["counts"][0], "the history culls something"
        r.render_frame()
        got = _check_frame(r, ms, want1, "frame 1")
        _list_is_telling(ms, got, want1["cmds"])
    finally:
        r.close()


def test_an_asset_without_a_bvh_refuses_the_hierarchical_cull(gpu):
    ms, cam, view, iv = _setup(MA.two_assets_one_without_bvh)
    r = _renderer(ms, FW, FH)
    try:
        _refused(lambda: r.set_cull_mode(1), "primitives without a BVH")
        r.set_view(view, iv, H.ALL_FLAGS)
        want0 = orc.frame(ms.spec, view, iv, H.ALL_FLAGS)
        r.render_frame()
        _check_frame(r, ms, want0, "flat frame 0", with_stats=False)
        r.render_frame()
        got = _check_frame(r, ms, orc.frame(ms.spec, view, iv, H.ALL_FLAGS, prev_hzb_min=want0["hzb_min"]), "flat frame 1")
        own = ms.asset_of_object[got["objectId"]]
        assert (own == 0).sum() > 20 and (own == 1).sum() > 20
    finally:
        r.close()


# ---- 2. resolves -----------------------------------------------------------------------------------------------------------------

def _images(r, names, desc=None):
    import torch
    out = r.resolve_attributes(names=list(names), desc=desc)
    torch.cuda.synchronize()
    return {n: t.cpu().numpy().view(u32) for n, t in out.items()}


def _same_images(got, want, what):
    for n, g in got.items():
        wv = np.ascontiguousarray(want[n]).view(u32).reshape(g.shape)
        if not np.array_equal(g, wv):
            bad = np.argwhere(g != wv)
            raise AssertionError("%s %s: %d texels differ; first %s got %r want %r" % (what, n, len(bad), bad[0], g[tuple(bad[0][:2])], wv[tuple(bad[0][:2])]))


def _frame_inputs(r, ms, w=FW, h=FH):
    """(visibility words, the list in the twin's numbering, per pixel the asset of its object or -1)"""
    vis = r.read_visibility()
    cmds = ms.to_concatenated(r.read_cmds(r.last_frame_cmds()))
    low = (vis & np.uint64(0xFFFFFFFF)).astype(np.int64)
    slot = np.where(low != 0, ((low >> 8) & 0xFFFFFF) - 1, 0)
    owner = np.where(low != 0, ms.asset_of_object[cmds["objectId"][slot]], -1).reshape(h, w)
    assert all((owner == a).sum() >= 0.05 * (owner >= 0).sum() for a in range(3))
    return vis, cmds, owner


def test_attributes_surface_and_debug_views(gpu):
    """chordvis_resolve_attributes' eight images and chordvis_resolve_surface's three, then the four debug views: the meshlet colours
    (modes 0 and 3) hash the asset-relative id."""
    ms, cam, view, iv = _setup()
    r = _renderer(ms, FW, FH)
    try:
        r.set_view(view, iv, H.ALL_FLAGS)
        r.render_frame()
        r.render_frame()
        vis, cmds, owner = _frame_inputs(r, ms)
        kw = dict(asset_meshlet_base=ms.asset_meshlet_base)
        got = _images(r, list(SR.NAMES) + list(SS.NAMES))
        want = dict(SR.resolve(ms.spec, vis, cmds, view, iv, FW, FH, **kw))
        want.update(SS.resolve(ms.spec, vis, cmds, view, iv, FW, FH))
        _same_images(got, want, "eleven images")
        # the asset without normals gives zeros, the others do not; the asset without uvs gives uv (0, 0)
        vn = got["vertexNormal"].view(f32)[..., :3]
        assert not vn[owner == 1].any() and not got["tangent"][owner == 1].any() and vn[owner == 0].any() and vn[owner == 2].any()
        uv = got["uv"].view(f32)
        assert not uv[owner == 1].any() and uv[owner == 0].any() and uv[owner == 2].any()
        for mode in range(4):
            d = L.ResolveDesc()
            d.debugMode = mode
            g = _images(r, ["debugRGBA8"], desc=d)
            w = SR.resolve(ms.spec, vis, cmds, view, iv, FW, FH, names=("debugRGBA8",), debug_mode=mode, **kw)
            _same_images(g, w, "debug mode %d" % mode)
    finally:
        r.close()


def test_material_gbuffer_and_material_feedback(gpu):
    """chordvis_resolve_material, chordvis_resolve_gbuffer and chordvis_material_feedback: the materials of assets 1 and 2 carry texture
    and sampler ids shifted by their assets' bases; asset 1, without texture coordinates, samples its texture at (0, 0)."""
    ms, cam, view, iv = _setup()
    r = _renderer(ms, FW, FH, textures=True)
    try:
        r.set_view(view, iv, H.ALL_FLAGS)
        r.render_frame()
        r.render_frame()
        vis, cmds, owner = _frame_inputs(r, ms)
        got = _images(r, SM.NAMES)
        stats = {}
        want = SM.resolve(ms.spec, vis, cmds, view, iv, FW, FH, stats=stats)
        _same_images(got, want, "material images")
        # asset 1: one texel of its own texture under every pixel of the material that names it
        mat = SM.material_of_pixels(ms.spec, vis, cmds).reshape(FH, FW)
        named = (owner == 1) & (mat >= 0)
        named[named] = ms.materials["baseColorId"][mat[named]] == ms.texture_base[1]
        assert named.sum() > 50 and len(np.unique(got["baseColor"][named].reshape(-1, 4), axis=0)) == 1
        assert len(np.unique(got["baseColor"][owner == 2].reshape(-1, 4), axis=0)) > 50
        packed = TG._packed(r)
        want_packed, written, _ = TG._spec(ms.spec, vis, cmds, view, iv, FW, FH)
        TG._same(packed, want_packed, "packed G-buffer")
        r.reset_material_feedback()
        r.material_feedback(15, 1, (0, 0))
        taps = r.read_material_feedback()
        want_taps = SF.feedback_of(stats, ms.spec, FW)
        assert taps.shape == want_taps.shape == (len(ms.texture_images), SF.LEVELS)
        assert np.array_equal(taps, want_taps), "material feedback\ngot\n%s\nwant\n%s" % (taps, want_taps)
        per_texture = taps.sum(axis=1)
        assert per_texture[ms.texture_base[1]] > 0 and (per_texture[ms.texture_base[2]:] > 0).sum() >= 3 and per_texture[0] > 0
    finally:
        r.close()


# ---- 3. geometry feedback and the visible clusters -------------------------------------------------------------------------------

def test_geometry_feedback_and_visible_clusters(gpu):
    """The per-object and per-(primitive, LOD) counts against tests/spec_geometry_feedback_np.py on the twin.

    chordvis_visible_clusters writes "records verbatim" into DEVICE memory: the records of the device list (kernels_geometry.hip copies
    a.cmds[i]), which the library's device lists keep in the CONCATENATED numbering -- the output is a list for the calls that take
    device lists, not a read-back, so no base is subtracted.  Held here: the visible records equal the twin's, untranslated, and
    differ from what chordvis_readback_cmds returns for the same slots on assets 1 and 2."""
    ms, cam, view, iv = _setup()
    r = _renderer(ms, FW, FH)
    try:
        r.set_view(view, iv, H.ALL_FLAGS)
        r.render_frame()
        r.render_frame()
        vis, cmds, owner = _frame_inputs(r, ms)
        handle = r.last_frame_cmds()
        for stride, offset in ((1, (0, 0)), (2, (1, 0))):
            r.reset_geometry_feedback()
            r.geometry_feedback(stride, offset, handle)
            want = SGF.geometry_feedback(ms.spec, vis, cmds, len(cmds), FW, FH, handle.capacity, stride, offset)
            assert SGF.identities(want) == []
            got = r.read_geometry_feedback()
            for k in SGF.ARRAYS:
                assert np.array_equal(got[k], want[k]), "stride %d: %s\ngot  %s\nwant %s" % (stride, k, got[k], want[k])
            assert np.array_equal(r.read_geometry_feedback_seen(), want["seen"]), "stride %d: the seen bitmap" % stride
            visible, total = r.visible_clusters(drawed_meshlet_cmd=handle)
            assert total == len(want["visible"]) and np.array_equal(visible, want["visible"]), "stride %d: the visible list (concatenated ids)" % stride
        for a in range(3):
            assert want["objectPixels"][ms.asset_of_object == a].sum() > 100 and want["lodPixels"][ms.asset_of_primitive == a].sum() > 100
        rel = ms.to_asset_relative(visible)
        own = ms.asset_of_object[visible["objectId"]]
        assert (own > 0).sum() > 20 and (rel["meshletId"][own > 0] != visible["meshletId"][own > 0]).all()
    finally:
        r.close()


# ---- 4. a depth view -------------------------------------------------------------------------------------------------------------

def test_one_cascade_depth_pass_equals_the_oracle(gpu):
    """tests/test_depth_views.py's cascade loop for one cascade at 256 x 256: the child context shares the re-based scene, its culled
    list reads back asset-relative through the parent's tables, and its depth image is the oracle's on the twin."""
    ms, cam, view, iv = _setup()
    dim, k = 256, 1
    cfg = R.default_cascade_config(cascadeCount=3, realtimeCascadeCount=2, cascadeDim=dim, cascadeEndDistance=14.0, farCascadeEndDistance=40.0)
    views = L.cascade_setup(cfg, view, iv, LIGHT)
    r = _renderer(ms, FW, FH)
    try:
        r.set_view(view, iv, H.ALL_FLAGS)
        r.allocate_depth_views(dim, len(views))
        r.set_instance_views(views)
        vk = views[k:k + 1]
        got_list = r.instance_culling_view(k)
        want_cmds = orc.instance_culling(ms.spec, view, vk, H.ALL_FLAGS)
        got = r.read_cmds(got_list)
        assert np.array_equal(got, ms.to_asset_relative(want_cmds)), "the cascade's culled list"
        _list_is_telling(ms, got, want_cmds)
        target = r.render_mesh_depth(k, got_list, True, 0.0, 0.0)
        want_depth, _ = orc.raster_depth(ms.spec, vk, want_cmds, dim, dim, True, 0.0, 0.0)
        got_depth = r.read_depth(target)
        bad = np.flatnonzero(got_depth.view(u32) != want_depth.view(u32))
        assert len(bad) == 0, "%d texels differ, first %d: %r vs %r" % (len(bad), bad[0], got_depth[bad[0]], want_depth[bad[0]])
        assert (want_depth > 0).sum() > dim * dim // 20 and r.depth_view_stats()["overflow"] == 0
        r.render_frame()
        _check_frame(r, ms, orc.frame(ms.spec, view, iv, H.ALL_FLAGS), "the main view after the depth pass", with_stats=False)
    finally:
        r.close()


# ---- 5. object lists and device-built records --------------------------------------------------------------------------------------

def test_object_list_without_asset_0_then_records_built_on_the_device(gpu):
    """chordvis_set_object_list to a list that drops every object of asset 0 and names four objects of asset 2 twice; then
    chordvis_upload_world_transforms and chordvis_build_objects under a moved camera.  Two frames after that equal the oracle's on the
    twin under the records the device built, and the frames of a context that uploaded that list afresh."""
    ms, cam, view, iv = _setup()
    a1, a2 = np.flatnonzero(ms.asset_of_object == 1), np.flatnonzero(ms.asset_of_object == 2)
    order = np.concatenate([a2[::-1], a1, a2[:4]])
    l2w = ms.local_to_world[order].copy()
    l2w[-4:, 12:15] += np.array((0.7, 1.5, -0.9))                      # (the second copies stand elsewhere)
    lst = ms.with_object_list(ms.objects[order].copy(), l2w)
    L.fill_objects(lst, cam)
    cam2 = cam.moved((0.3, 0.2, -0.4))
    view2, iv2 = L.make_views(cam2)
    r = _renderer(ms, FW, FH)
    try:
        r.set_view(view, iv, H.ALL_FLAGS)
        r.render_frame()                                               # (the full list has rendered: there is a history to reset)
        r.set_object_list(lst)
        r.upload_world_transforms(lst.local_to_world)
        r.build_objects(cam2.position, cam2.position)
        assert r.build_objects_status()[0] == 0
        built = r.read_objects()
        assert len(built) == len(order) and np.array_equal(built["GLTFPrimitiveDetail"], lst.objects["GLTFPrimitiveDetail"])
        assert np.array_equal(built["GLTFMaterialData"], lst.objects["GLTFMaterialData"])
        assert not (ms.asset_of_primitive[built["GLTFPrimitiveDetail"]] == 0).any()
        twin = ms.with_object_list(built, l2w)
        r.history_hzb()
        r.reset_history()
        r.set_view(view2, iv2, H.ALL_FLAGS)
        fresh = _renderer(ms.relisted(built), FW, FH)
        try:
            fresh.set_view(view2, iv2, H.ALL_FLAGS)
            prev = None
            for frame in range(2):
                want = orc.frame(twin, view2, iv2, H.ALL_FLAGS, prev_hzb_min=prev)
                assert want["vis"].any()
                r.render_frame()
                fresh.render_frame()
                got = _check_frame(r, ms, want, "new list, frame %d" % frame, with_stats=frame > 0, objects=built)
                _check_frame(fresh, ms, want, "fresh upload, frame %d" % frame, with_stats=frame > 0, objects=built)
                _list_is_telling(ms, got, want["cmds"], built)
                prev = want["hzb_min"]
        finally:
            fresh.close()
    finally:
        r.close()


# ---- 6. rays ---------------------------------------------------------------------------------------------------------------------

def _hits(r, rays, any_hit=False):
    out = r.trace_rays(np.asarray(rays), any_hit=any_hit)
    r.sync()
    return out.cpu().numpy().view(R.RAY_HIT).reshape(-1)


def _same_hits(got, want, rays, what):
    if got.tobytes() == want.tobytes():
        return
    g, w = got.view(u32).reshape(-1, 8), want.view(u32).reshape(-1, 8)
    bad = np.flatnonzero((g != w).any(axis=1))
    k = int(bad[0])
    raise AssertionError("%s: %d of %d rays differ from the specification; first: ray %d %r\n got  %r\n want %r"
                         % (what, len(bad), len(got), k, rays[k], got[k], want[k]))


def _same_surfaces(got, want, hits, what):
    w = np.ascontiguousarray(want).view(u32).reshape(-1, 16)
    assert got.shape == w.shape, (what, got.shape, w.shape)
    if not np.array_equal(got, w):
        bad = np.flatnonzero((got != w).any(axis=1))
        k = int(bad[0])
        raise AssertionError("%s: %d of %d hits differ from the specification; first: hit %d %r\n got  %r\n want %r"
                             % (what, len(bad), len(w), k, hits[k], got[k].view(RS.RAY_HIT_SURFACE), np.asarray(want)[k]))


def test_build_trace_and_refit(gpu):
    """chordvis_build_ray_scene (a BLAS per primitive of every asset), closest-hit and any-hit against tests/spec_rays_np.py on the twin
    with the meshlets asset-relative, and a refit after moved objects."""
    ms, cam, view, iv = _setup()
    rays, origin = MA.ray_set(ms)
    tris = S.lod0_triangles(ms.spec, ms.asset_meshlet_base)
    want = S.trace(ms.spec, ms.objects, rays, triangles=tris, meshlet_cull=True)
    hit = (want["status"] & 1) != 0
    assert want["meshlet"][hit].max() < max(s["meshlets"] for s in ms.sizes)
    r = _renderer(ms)
    try:
        info = r.build_ray_scene()
        assert info.blasBuilt == info.blasCount == len(ms.primitives) == sum(len(a.primitives) for a in ms.assets)
        assert info.blasTriangles == sum(len(t[0]) for t in tris)
        _same_hits(_hits(r, rays), want, rays, "closest")
        want_any = np.zeros(len(rays), dtype=R.RAY_HIT)
        want_any["status"] = want["status"] & 1
        _same_hits(_hits(r, rays, any_hit=True), want_any, rays, "any-hit")
        moved = ms.local_to_world.copy()
        moved[::3, 12:15] += np.array((0.9, 0.4, -1.3))
        old = ms.local_to_world
        ms.local_to_world = moved
        L.fill_objects(ms, cam)
        ms.local_to_world = old
        r.update_objects(ms.objects)
        _refused(lambda: r.trace_rays(rays), "objects changed.*chordvis_refit_ray_scene")
        r.refit_ray_scene()
        want_moved = S.trace(ms.spec, ms.objects, rays, triangles=tris, meshlet_cull=True)
        assert want_moved.tobytes() != want.tobytes()
        _same_hits(_hits(r, rays), want_moved, rays, "after update_objects + refit")
    finally:
        r.close()


# Nothing on the device outlives these helpers: a tensor that a failed assertion's traceback kept alive past r.close() -- which destroys
# the stream the tensor was recorded on -- ends the interpreter when it is collected.

def _trace_and_shade(r, rays, lods):
    """trace, then two shades of the hits where they lie: (hits, surfaces at lod 1, surfaces at the per-hit lods) on the host"""
    dhits = r.trace_rays(rays)
    a = r.shade_ray_hits(dhits, lod=1.0)
    b = r.shade_ray_hits(dhits, lods=lods)
    r.sync()
    return (dhits.cpu().numpy().view(R.RAY_HIT).reshape(-1), a.cpu().numpy().view(u32).reshape(-1, 16), b.cpu().numpy().view(u32).reshape(-1, 16))


def _shade(r, hits, lod):
    out = r.shade_ray_hits(np.asarray(hits), lod=lod)
    r.sync()
    return out.cpu().numpy().view(u32).reshape(-1, 16)


def _frame_images_and_pixel_rays(r, z_of, runs):
    """resolve positionRS and vertexNormal of the frame, then one chordvis_pixel_rays call with hit records per run (its keyword
    arguments; "table" a numpy array): (position, normal, [(image, hits)]) on the host.  z_of(): the depth image, read after the resolve."""
    res = r.resolve_attributes(names=["positionRS", "vertexNormal"])
    r.sync()
    dz = _device(z_of())
    got = []
    for args in runs:
        args = dict(args, depth=dz, depth_stride=1)
        if "table" in args:
            args["table"] = _device(args["table"])
        out, dhits = r.pixel_rays(res["positionRS"], res["vertexNormal"], hits=True, **args)
        r.sync()
        got.append((out.cpu().numpy().view(u32), dhits.cpu().numpy().view(R.RAY_HIT).reshape(-1)))
    return res["positionRS"].cpu().numpy().view(u32), res["vertexNormal"].cpu().numpy().view(u32), got


def _device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(torch.device("cuda", 0))


@pytest.mark.parametrize("store", ["texels", "blocks"])
def test_trace_then_shade_on_the_device(gpu, store):
    """chordvis_shade_ray_hits of the very hits chordvis_trace_rays wrote, with no host round trip, against tests/spec_ray_shade_np.py:
    the hit's meshlet is asset-relative, read at the asset's base.  Then host-made hits at the edges of that numbering.  Under the
    texel store, and under the block store with asset 2's textures block-compressed (the decoded twin is the specification's scene)."""
    if store == "blocks":
        ms, twin, cam = MA.three_assets_blocks()
        MA.filled(ms, cam)
        MA.filled(twin, cam)
    else:
        ms, cam = MA.three_assets()
        MA.filled(ms, cam)
        twin = ms
    kw = dict(asset_meshlet_base=ms.asset_meshlet_base, asset_meshlet_count=ms.asset_meshlet_count)
    rays, origin = MA.ray_set(ms)
    want_hits = S.trace(twin.spec, twin.objects, rays, meshlet_cull=True, asset_meshlet_base=ms.asset_meshlet_base)
    lods = np.log2(np.maximum(want_hits["t"].astype(np.float64), 1e-3)).astype(f32)
    r = _renderer(ms, textures=True, store=L.TEXSTORE_BLOCKS if store == "blocks" else L.TEXSTORE_EXPANDED)
    try:
        texel_bytes, block_bytes = r.material_texture_memory()[:2]
        assert (block_bytes > 0) == (store == "blocks")
        r.build_ray_scene()
        got_hits, a, b = _trace_and_shade(r, rays, lods)
        _same_hits(got_hits, want_hits, rays, "the traced hits")
        for label, got, lod_kw in (("lod 1", a, dict(lod=1.0)), ("per-hit lod", b, dict(lods=lods))):
            want = RS.shade(twin.spec, twin.objects, want_hits, **lod_kw, **kw)
            valid = (want["flags"] & RS.RAYSURF_VALID) != 0
            on = twin.asset_of_object[np.where(valid, want_hits["object"], 0)]
            assert all((valid & (on == k)).sum() >= 50 for k in range(3))
            _same_surfaces(got, want, want_hits, "%s store, %s" % (store, label))
        edges = ms.edge_hits()
        hits = np.concatenate([h for _, h, _ in edges])
        want = RS.shade(twin.spec, twin.objects, hits, lod=0.5, **kw)
        assert [bool(f & RS.RAYSURF_VALID) for f in want["flags"]] == [v for _, _, v in edges]
        _same_surfaces(_shade(r, hits, 0.5), want, hits, "%s store, the edges of the numbering" % store)
    finally:
        r.close()


def test_pixel_rays_from_the_frames_own_images(gpu):
    """A frame, chordvis_resolve_surface's positionRS and vertexNormal, then chordvis_pixel_rays with hit records in the hemisphere mode
    (starting from the image's depth) and in the direction mode: images and hits against tests/spec_pixel_rays_np.py on the twin, the
    hits' meshlets asset-relative."""
    w, h = 80, 64                                                      # (a G-buffer is at least 64 pixels a side; a ray per pixel)
    ms, _ = MA.three_assets()
    cam = MA.camera(w, h)
    view, iv = MA.filled(ms, cam)
    tris = S.lod0_triangles(ms.spec, ms.asset_meshlet_base)
    tab = PC.table(16, 16)
    r = _renderer(ms, w, h)
    try:
        r.build_ray_scene()
        r.set_view(view, iv, H.ALL_FLAGS)
        r.render_frame()
        sun = (-0.35, 1.0, -0.25)
        runs = [("hemisphere", dict(mode=L.PIXEL_RAYS_HEMISPHERE, table=tab, ray_length=2.0, z_near=cam.z_near, start_from_depth=True),
                 PR.Desc(w, h, PR.HEMISPHERE, PR.START_FROM_DEPTH, 16, 16, rayLength=2.0, tMin=0.0, zNear=cam.z_near), tab),
                ("direction", dict(mode=L.PIXEL_RAYS_DIRECTION, direction=sun, ray_length=30.0, t_min=0.02),
                 PR.Desc(w, h, PR.DIRECTION, 0, direction=sun, rayLength=30.0, tMin=0.02), None)]
        depth_of = lambda: (r.read_visibility() >> np.uint64(32)).astype(u32).view(f32).reshape(h, w)
        got_pos, got_nrm, got = _frame_images_and_pixel_rays(r, depth_of, [args for _, args, _, _ in runs])
        vis, cmds, owner = _frame_inputs(r, ms, w, h)
        pos = SR.resolve(ms.spec, vis, cmds, view, iv, w, h, names=("positionRS",))["positionRS"]
        nrm = SS.resolve(ms.spec, vis, cmds, view, iv, w, h, names=("vertexNormal",))["vertexNormal"]
        assert np.array_equal(got_pos, pos.view(u32)) and np.array_equal(got_nrm, nrm.view(u32))
        z = depth_of()
        for (name, args, desc, table), (out, hits) in zip(runs, got):
            want_out, want_hits = PR.pixel_rays(ms.spec, ms.objects, pos, nrm, z, table, desc, triangles=tris, meshlet_cull=True)
            hit = (want_hits["status"] & 1) != 0
            on = np.where(hit, ms.asset_of_object[np.where(hit, want_hits["object"], 0)], -1)
            print(name, "hits per asset", [int((on == a).sum()) for a in range(3)], "misses", int((~hit & (z.reshape(-1) > 0)).sum()))
            assert (on == 2).sum() > 50 and (on == 0).sum() + (on == 1).sum() > 50 and (~hit & (z.reshape(-1) > 0)).sum() > 100, name
            assert np.array_equal(out, want_out.view(u32).reshape(h, w)), name + ": the image"
            _same_hits(hits, want_hits, np.arange(w * h), name + ": the hit records")
    finally:
        r.close()


# ---- 7. upload refusals only several assets can reach ----------------------------------------------------------------------------

def test_upload_refusals_between_the_assets(gpu):
    """A primitive of asset 1 -- the middle asset: one past its own streams is still inside the concatenation -- whose asset id, group
    range, group-index range, meshlet range or vertex range leaves its OWN asset is refused by its message before anything is copied to
    the device; the untouched scene uploads and renders afterwards."""
    from chord_amd.renderer import VisibilityRenderer
    ms, cam, view, iv = _setup()
    p = int(np.flatnonzero(ms.asset_of_primitive == 1)[1])
    size = ms.sizes[1]
    row = ms.primitives[p].copy()
    groups = ms.assets[1].groups[int(row["meshletGroupOffset"]): int(row["meshletGroupOffset"]) + int(row["meshletGroupCount"])]
    assert int(row["meshletGroupCount"]) >= 2 and int(groups["meshletCount"].sum()) >= 2
    cases = [("primitiveDatasBufferId", len(ms.assets), "primitiveDatasBufferId out of range"),
             ("meshletGroupOffset", size["groups"] - int(row["meshletGroupCount"]) + 1, "primitive group range out of bounds"),
             ("meshletGroupIndicesOffset", size["group_indices"] - 1, "group index out of bounds"),
             ("meshletOffset", size["meshlets"] - 1, "meshlet index out of bounds"),
             ("vertexOffset", size["vertices"] - 1, "meshlet vertex id out of the asset's position stream")]
    r = VisibilityRenderer(0)
    try:
        for field, value, message in cases:
            # every one of them would be in range in the twin: inside the concatenation
            ms.primitives[field][p] = value
            rc = L.lib.chordvis_upload_scene(r._ctx, C.byref(ms.desc))
            ms.primitives[p] = row
            assert rc == L.E_INVALID and message.encode() in L.lib.chordvis_last_error(r._ctx), (field, rc, L.lib.chordvis_last_error(r._ctx))
            _refused(r.build_ray_scene, "no scene")                       # (a refused upload leaves no scene behind)
        r.upload_scene(ms)
        r.allocate_gbuffer(FW, FH)
        r.set_view(view, iv, H.ALL_FLAGS)
        r.render_frame()
        _check_frame(r, ms, orc.frame(ms.spec, view, iv, H.ALL_FLAGS), "after the refusals", with_stats=False)
    finally:
        r.close()
