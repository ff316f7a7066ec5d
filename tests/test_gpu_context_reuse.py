"""One long-lived context across scene, size and mode changes, every frame against the oracle.

Nearly every other GPU test makes a fresh VisibilityRenderer, renders a few frames of one scene at one size and closes it.  This
module is about the host state machine that decides which kernels run, on which buffers and under which hints: what a context
carries from call to call, and which call has to drop, re-make or keep it.  A frame of the live context is always compared with
orc.frame (or the oracle call of its entry point: orc.visibility_mark, orc.shading_tiles, orc.raster_depth, the renderShadow
replay of test_depth_views.py, spec_bounds_tiles_np), never only with a second HIP context.

Carried state, read from the source before anything was run.  abi = the host layer, chord_amd/csrc/abi_*.cpp and chordvis_abi.cpp (the scene), dv = csrc/depth_views.cpp,
lr = launch_raster in csrc/raster_launch.cpp, ct = configure_targets (abi_context.cpp), the shared tail of allocate_gbuffer and set_shard.
Tests: T1 resizing, T2a templates_and_forms, T2b block_kernel_leftovers, T2c refused_upload, T2d hot_tiles, T3 mode_switches,
T4 bind_objects, T5 sharded_and_unsharded, T6 cascade_cache.

  state                              dropped / re-made by                                 kept by                          where                                     test
  ---------------------------------  ---------------------------------------------------  -------------------------------  ----------------------------------------  --------
  kept schedules (dTileOrderKeep*,   upload_scene, allocate_gbuffer, set_shard,           set_cull_mode, reset_history,    abi: upload_scene_impl, ct,               T1 T2a
  orderAge*, orderFlip)              set_tile_owners, set_tile_schedule_keep, set_debug,  set_view, update / bind_objects  install_tile_owners, the setters;         T3 T5
                                     set_limits; a direct later pass (lr)                 (a schedule lists tiles only)    aged in lr
  hBinHint[0..1] longest bin,        allocate_gbuffer, set_shard (ct)                     upload_scene and everything      ct; read in lr.  Stale after an upload    T1 T2a
  [2..3] clusters per pass,                                                               else: a stale report picks a     BY DESIGN: every form renders the same    T2b T2d
  [4..7] heavy / light serials                                                            form, never a pixel (lr)         image (asserted: T2a, T2d)
  dHotTiles                          zeroed by ct (tile ids of another target size)       upload_scene (ids stay tiles of  ct; written by the schedule kernel        T1 T2d
                                                                                          the target; T2d: image exact)
  history slot, hzb[1..2]            upload_scene, allocate_gbuffer, set_shard,           set_cull_mode, set_debug, keep,  abi: upload_scene_impl, ct,               all
                                     reset_history; replaced by upload_history_hzb        set_view, flags without HZB      chordvis_reset_history
  pendingTailSlot                    the same calls (dropped unflushed); flushed by       rides on the next frame's first  abi: flush_pending_tail and its callers   T1 T2a
                                     stats, history_hzb, read_hzb, sync, build_hzb        kernel                                                                     T3
  fullListStale, mineValid,          upload_scene; set_shard / install_tile_owners        --                               abi: upload_scene_impl, set_shard,        T5
  listMine[], cullPhaseDone          (mineValid, listMine); every cull (fullListStale)                                     install_tile_owners; kernels_cull.hip
  fusedCullDone                      start and end of every render_frame                  --                               abi: render_frame_impl                    T2a T3
  resolveFrame / resolveStale        upload_scene, allocate_gbuffer (no frame);           --                               abi: do_raster, the four calls,           T4
                                     update_objects, bind_objects, set_view (stale)                                        resolve_checks
  dLeftCmds, dRankCmds, dMineCmds,   upload_scene frees them, first use re-makes them     allocate_gbuffer                 abi: upload_scene_impl; lr,               T2b T5
  dCullExchange (by cmdCapacity /    at the new size                                                                       launch_group_cull, ensure_cull_exchange
  count blocks)
  dTileBins, dBinChunkTab,           allocate_gbuffer, set_shard (dalloc frees and        upload_scene                     ct                                        T1 T5
  dTileSlabs, dTileOrder*,           re-makes: ct)
  dRangePartials, hzb[0..2]
  dTileMarker, dShadingTiles         allocate_gbuffer frees, visibility_mark re-makes;    upload_scene, set_shard (same    abi: allocate_gbuffer, visibility_mark,   T1
                                     a marker handle of another size is refused           size)                            prepare_shading_tile_param
  dBoundsTilesScratch                grown on demand by its word count (never shrunk)     everything                       abi: chordvis_bin_bounds                  T1
  the view (hView, viewSet)          after allocate_gbuffer at another size it no longer  upload_scene, set_shard,         abi: ready, set_view; dv: render_shadow,  T1 T6
                                     fits: passes are refused until set_view has come     allocate_gbuffer of the same     instance_culling_view (view_fits_target,
                                     again; one of any other size is refused and changes  size                             device_layer.h)
                                     nothing
  anyMasked                          upload_scene                                         everything else                  abi: upload_scene_impl; read in lr        T2a
  cullMode                           set_cull_mode; upload_scene refuses a scene without  upload_scene                     abi: set_cull_mode, upload_scene_impl     T2c T3
                                     BVHs under mode 1 and then leaves NO scene
  the scene itself                   upload_scene; a REFUSED upload leaves no scene       everything else                  abi: chordvis_upload_scene                T2c
  dObjects (owned copy or bound)     update_objects, upload_scene (owned copy again);     allocate_gbuffer, set_shard;     abi: the three calls; dv:                 T4
                                     bind_objects                                         the depth child re-reads it      instance_culling_view
  depth child, dDepthImages          upload_scene (child), allocate_depth_views,          allocate_gbuffer of the parent   abi: upload_scene_impl; dv                T6
                                     render_shadow with another dim / count
  shadowHistoryValid / Config / Dir  allocate_depth_views, a refused upload; invalid      allocate_gbuffer + set_view of   dv: allocate_depth_views, render_shadow   T6
                                     without a child (upload_scene), with another         the parent (the cascades depend
                                     config, dim, count or light                          on the view, not on the size)
  instanceViews                      set_instance_views, render_shadow                    read as history only under a     dv: render_shadow                         T6
                                                                                          valid cache
  shard tables, tileOwners(Explicit) set_shard to another rank count (explicit map        allocate_gbuffer of the same     abi: set_shard, ct, set_tile_owners       T5
                                     gone), allocate_gbuffer to another tile count        tile count keeps an explicit map
  dVisResolved, exchange buffers     set_shard(1, 0) frees them, set_shard(n > 1) makes   --                               ct                                        T5
                                     them
  debugFlags, timers, limits         their setters only                                   everything                       abi                                       T2b T3

Findings (each fixed where the state is owned, and pinned below):
  1. chordvis_allocate_depth_views kept shadowHistoryValid: the same config and light after it skipped the far cascades over new,
     empty images and culled the first one against an empty HZB (T6 "reallocated").  Cleared in allocate_depth_views.
  2. chordvis_bind_objects did not set resolveStale where chordvis_update_objects does.  It does now; the header says what the
     caller guarantees for writes into the bound array, which the library cannot see (T4).
  3. A refused chordvis_upload_scene left sceneLoaded set over half-replaced tables -- under set_cull_mode(1) a scene without
     trees, whose next frame would have walked a null BVH.  A refused upload now leaves no scene (T2c).
  4. chordvis_allocate_gbuffer kept a view of the old size, and a refused chordvis_set_view had already overwritten the view
     it refused to replace: render_frame then ran the old renderDimension on the new target.  Every pass now refuses a view that
     does not fit the target (ready), and set_view checks before it takes anything over (T1).
  5. chordvis_prepare_shading_tile_param told a stale marker handle by its address alone; the allocator may hand the same address
     to the new marker, and the old dims place the count words past the new list.  The dims are checked now (T1)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import bounds_scenes as B
import helpers as H
import orc
import spec_bounds_query_np as Q
import spec_bounds_tiles_np as S
from chord_amd import lib as L, records as R, scenes
from test_depth_views import LIGHT, _replay_shadow
from test_gpu_cull_paths import MOVES, _check_frame

pytestmark = pytest.mark.gpu

FORCE_BLOCKS, FORCE_HOT = 65536, 262144                 # chordvis_set_debug switches that change no result (tests/test_gpu_parity.py)
TILE_DIRECT_MAX_CLUSTERS = 1024                         # raster_params.h: a later pass that set up more reports heavy
NEAR_FAR = R.BOUNDS_TILES_NEAR | R.BOUNDS_TILES_FAR
NO_HZB_FLAGS = R.FLAG_FRUSTUM_CULL | R.FLAG_CONE_CULL


# ---- scenes (built once; the object records of a scene are rewritten by every frame) -----------------------------------------

@functools.lru_cache(maxsize=None)
def _small():
    return scenes.small_test_scene(320, 200)


@functools.lru_cache(maxsize=None)
def _masked():
    return scenes.masked_test_scene(320, 200)


@functools.lru_cache(maxsize=None)
def _street():
    """Config 3 at 320 x 200: with every object 500 m further down the view in the frame before, its second pass holds ~2 800
    clusters (what test_gpu_setup_wide.py / test_gpu_touched_tiles.py cross TILE_DIRECT_MAX_CLUSTERS with); 38 k commands of capacity."""
    return scenes.config3_street(320, 200)


@functools.lru_cache(maxsize=None)
def _groups65():
    return scenes.group_count_scene(65, 320, 200)


def _cam_at(cam, w, h):
    return scenes.Camera(cam.position, cam.front, w, h, cam.fovy, cam.z_near, cam.z_far, cam.world_up, cam.jitter)


def _turned(cam, angle):
    """The camera turned about +y."""
    c, s = math.cos(angle), math.sin(angle)
    x, y, z = cam.front
    return scenes.Camera(cam.position, (c * x + s * z, y, c * z - s * x), cam.width, cam.height, cam.fovy, cam.z_near, cam.z_far,
                         cam.world_up, cam.jitter)


def _path(cam, n, turn=0.3):
    """n cameras from `cam`: a step of test_gpu_cull_paths.MOVES between consecutive ones, and a turn to and fro on every second step
    (clusters that enter the view have no last-frame depth to hide behind: they go through the second pass)."""
    out = [cam]
    for k in range(1, n):
        nxt = out[-1].moved(MOVES[(k - 1) % 2])
        out.append(_turned(nxt, turn if k % 4 == 2 else -turn) if k % 2 == 0 else nxt)
    return out


def _far_last_frame(scene, cam):
    """local_to_world of a frame before in which every object was 500 m further down the view: phase 0 rejects what the history
    covers and the second pass draws the scene (test_frame_whose_second_pass_holds_the_scene_matches_oracle)."""
    f = np.array(cam.front, dtype=np.float64)
    f /= np.linalg.norm(f)
    last = scene.local_to_world.copy()
    last[:, 12:15] += 500.0 * f                           # glm column-major: the translation column
    return last


# ---- one frame on the live context(s) against the oracle ---------------------------------------------------------------------

class _Track:
    """The oracle's side of a context's life: the last frame's view, camera and chain.  A new one wherever the library must have
    dropped its history."""

    def __init__(self):
        self.view = self.cam = self.hzb = None


def _frame(rs, tr, scene, cam, what, flags=H.ALL_FLAGS, with_stats=True, last=None, supply=None, render=None, check=_check_frame):
    """The next frame of a sequence on every context of rs (one call sequence each), each against orc.frame with the oracle's own
    previous chain.  supply(r): how the objects reach the context (default: update_objects); render(rs): default render_frame each.
    Returns (oracle frame, view, iv, [what check returned per context])."""
    L.fill_objects(scene, cam, tr.cam, last)
    view, iv = L.make_views(cam, tr.view)
    want = orc.frame(scene, view, iv, flags, prev_hzb_min=tr.hzb)
    for r in rs:
        if supply is None:
            r.update_objects(scene.objects)
        else:
            supply(r)
        r.set_view(view, iv, flags)
    if render is None:
        for r in rs:
            r.render_frame()
    else:
        render(rs)
    got = [check(r, scene, want, cam.width, cam.height, "%s, context %d" % (what, i), with_stats) for i, r in enumerate(rs)]
    tr.view, tr.cam, tr.hzb = view, cam, want["hzb_min"]
    return want, view, iv, got


def _wide(r):
    """Per raster pass whether its latest launch was set up by raster_setup_wide_kernel."""
    k = (C.c_uint32 * 2)()
    assert L.lib.chordvis_debug_setup_kernels(r._ctx, k) == 0
    return [int(k[0]), int(k[1])]


def _leg(r, scene, cam0, n, what, heavy=False, flags=H.ALL_FLAGS):
    """n frames of one scene along _path on a context that has just lost its history: frame 0 without it, frame 1 carrying frame 0's
    pending tail, the last frame leaving its own tail pending (no stats, no chain read).  heavy: from frame 1 on the second pass holds
    the scene.  Returns ([oracle frame], [_wide per frame])."""
    tr = _Track()
    wants, wides = [], []
    for k, cam in enumerate(_path(cam0, n)):
        last = _far_last_frame(scene, cam) if heavy and k else None
        want = _frame([r], tr, scene, cam, "%s, frame %d" % (what, k), flags, with_stats=0 < k < n - 1, last=last)[0]
        wants.append(want)
        wides.append(_wide(r))
    return wants, wides


def _refused(call, *args):
    with pytest.raises(L.ChordvisError):
        call(*args)


# ---- 1. resizing a live context -----------------------------------------------------------------------------------------------

SIZES = [(320, 200), (129, 67), (704, 384), (64, 64), (320, 200)]
CALLER_OWNED_LEG = 2                                     # the 704 x 384 leg renders into a torch tensor, the next one into the library's again


def _check_consumers(r, scene, want, view, iv, cam, cam_last, what):
    """The three consumers of the image at the current size, each against its own spec: the tile marker, the shading-tile lists of two
    shading types, and chordvis_bin_bounds over a handful of generated boxes.  Returns the marker handle."""
    w, h = cam.width, cam.height
    marker = r.visibility_mark()
    assert list(marker.markerDim) == [(w + 7) // 8, (h + 7) // 8] and list(marker.visibilityDim) == [w, h], what
    ref = orc.visibility_mark(scene, want["vis"], w, h, want["cmds"])
    assert np.array_equal(r.read_tile_marker(marker), ref), what + ": tile marker"
    for t in (1, 37):
        tiles, args = r.read_shading_tiles(r.prepare_shading_tile_param(t, marker))
        ref_tiles, ref_args = orc.shading_tiles(ref, t)
        assert sorted(map(tuple, tiles.tolist())) == sorted(map(tuple, ref_tiles.tolist())), "%s: shading tiles of type %d" % (what, t)
        assert args.tolist() == ref_args.tolist(), "%s: dispatch arguments of type %d" % (what, t)
    queries, _ = B.make_boxes(cam, cam_last, 24, seed=w * 4099 + h)
    results = Q.query_bounds(view, iv, queries, 1)[0]      # (no chain: reading the library's would flush the tail)
    farz = S.far_z(view, iv, queries, 1, results["status"])
    for T, cap in ((16, 6), (64, 24)):
        spec = S.bin_bounds(want["vis"], w, h, results, T, cap, NEAR_FAR, farz)
        got = r.bin_bounds(results, queries, T, cap, 1, NEAR_FAR)
        assert got["tiles"] == S.tile_count(w, h, T)[1:], what
        for k in ("counts", "items", "depth", "totals"):
            assert got[k].shape == spec[k].shape and np.array_equal(got[k], spec[k]), "%s: bin_bounds T %d: %s" % (what, T, k)
    return marker


@pytest.mark.parametrize("second_pass", ["light", "heavy"])
def test_resizing_a_live_context(gpu, second_pass):
    """One scene, one context, five target sizes (fewer tiles with odd edges, more tiles than ever before, one tile, the first size
    again), three frames with a moving camera at each.  Before every resize the context is dirty: a pending HZB tail, schedules one
    frame old, a second pass that has reported light / heavy, a tile marker, shading tiles and bin_bounds scratch of the old size."""
    from chord_amd.renderer import VisibilityRenderer
    heavy = second_pass == "heavy"
    base, cam0 = _street() if heavy else _small()
    scene = H.with_shading_types(base)
    scene.local_to_world = base.local_to_world
    r = VisibilityRenderer(0)
    r.upload_scene(scene)
    old_view, old_marker, caller = None, None, None
    try:
        for leg, (w, h) in enumerate(SIZES):
            what = "%s leg %d (%d x %d)" % (second_pass, leg, w, h)
            if leg == CALLER_OWNED_LEG:
                caller = H.CallerVisibility(r, w, h)       # (allocate_gbuffer with deviceVisibility)
            else:
                r.allocate_gbuffer(w, h)
            _refused(r.history_hzb)                         # no history until a frame has run at this size
            if old_view is not None:
                _refused(r.render_frame)                    # the view of the old size does not fit the new target ...
                _refused(r.set_view, old_view[0], old_view[1], H.ALL_FLAGS)      # ... and cannot come back
                _refused(r.render_frame)                    # (the refused set_view left nothing behind)
            tr = _Track()
            cams = _path(_cam_at(cam0, w, h), 3)
            for k, cam in enumerate(cams):
                last = _far_last_frame(scene, cam) if heavy and k else None
                # frame 0: no stats (frame 1 carries its tail); frame 2: none either (the resize meets a pending tail)
                want, view, iv, _ = _frame([r], tr, scene, cam, "%s, frame %d" % (what, k), with_stats=k == 1, last=last)
                if leg == CALLER_OWNED_LEG:
                    # (the frame's read-back has waited for the context's stream; caller.read() would flush the tail through chordvis_sync)
                    assert np.array_equal(caller.tensor.cpu().numpy().view(np.uint64), want["vis"]), what + ": the caller's tensor"
                if k == 1:
                    marker = _check_consumers(r, scene, want, view, iv, cam, cams[0], what)
                    if old_marker is not None:              # a handle from before the resize, now that a new marker exists
                        _refused(r.prepare_shading_tile_param, 1, old_marker)
                if heavy and k and max(w, h) >= 320:
                    assert want["counts"][3] > TILE_DIRECT_MAX_CLUSTERS, (what, k, list(want["counts"]))
            if not heavy:
                assert want["counts"][3] <= TILE_DIRECT_MAX_CLUSTERS
            old_view, old_marker = (view, iv), marker
    finally:
        r.close()


# ---- 2. swapping scenes on a live context -------------------------------------------------------------------------------------

def test_scene_swaps_flip_the_kernel_template_and_the_set_up_form(gpu):
    """Opaque -> masked -> opaque (anyMasked picks the template of every set-up and tile kernel), then -> a scene whose second pass is
    heavy -> a light one again, on one context at 320 x 200 with the default schedule keep.  upload_scene keeps the passes' reports:
    the first frame with a second pass after a swap may run the form the OLD scene's report asks for, and must render the same
    image; once the new scene's own report has reached the host (every frame's image is read back) the form follows it."""
    from chord_amd.renderer import VisibilityRenderer
    small, cam_s = _small()
    masked, cam_m = _masked()
    street, cam_h = _street()
    r = VisibilityRenderer(0)
    r.allocate_gbuffer(320, 200)
    assert r.tile_schedule_keep() == 1
    try:
        for name, scene, cam0, n, heavy in (("small", small, cam_s, 4, False), ("masked", masked, cam_m, 4, False),
                                            ("small again", small, cam_s, 4, False), ("street, heavy", street, cam_h, 4, True),
                                            ("small after heavy", small, cam_s, 4, False)):
            L.fill_objects(scene, cam0)
            r.upload_scene(scene)
            _refused(r.history_hzb)                         # the history went with the old scene
            wants, wides = _leg(r, scene, cam0, n, name, heavy)
            stage1 = [int(x["counts"][3]) for x in wants]
            assert all(x[0] == 0 for x in wides), (name, wides)               # a first pass is never set up wide
            if heavy:
                # frame 1 may still be announced light (asserted: its image, in _leg); from frame 2 on the report is the scene's own
                assert all(s > TILE_DIRECT_MAX_CLUSTERS for s in stage1[1:]), (name, stage1)
                assert all(x[1] == 0 for x in wides[2:]), (name, wides)
            else:
                assert max(stage1) > 0 and all(s <= TILE_DIRECT_MAX_CLUSTERS for s in stage1), (name, stage1)
                assert all(x[1] == 1 for x in wides[2:]), (name, wides)       # raster_setup_wide_kernel and the direct launch
    finally:
        r.close()


def test_scene_swaps_remake_the_block_kernel_leftover_list(gpu):
    """A scene of 260 commands, one of 38 k, the first again, with the block kernel forced on all three: dLeftCmds (sized by the scene's
    cmdCapacity, made by the first dense launch) must be re-made for the larger scene."""
    from chord_amd.renderer import VisibilityRenderer
    few, cam_f = _groups65()
    many, cam_m = _street()
    assert many.lod0_meshlet_instances > 64 * few.lod0_meshlet_instances
    r = VisibilityRenderer(0)
    r.allocate_gbuffer(320, 200)
    r.set_debug(FORCE_BLOCKS)
    try:
        for name, scene, cam0 in (("few", few, cam_f), ("many", many, cam_m), ("few again", few, cam_f)):
            L.fill_objects(scene, cam0)
            r.upload_scene(scene)
            wants, _ = _leg(r, scene, cam0, 3, "blocks forced, " + name)
            assert all(x["stats"].trianglesSubmitted > 0 for x in wants)
            if scene is many:                               # (its clusters are a few pixels wide: the forced block form takes them)
                assert r.stats()["pixelBlockBytes"] > 0, name
    finally:
        r.close()


def test_refused_upload_leaves_no_scene(gpu):
    """A scene with BVHs under set_cull_mode(1), then one without: the upload is refused with hierarchical mode still selected, and
    the context then holds NO scene (include/chordvis.h) -- what needs one is refused cleanly -- until, after set_cull_mode(0), the
    upload succeeds and renders exactly from a frame without history."""
    from chord_amd.renderer import VisibilityRenderer
    scene, cam0 = _small()
    bare = R.Scene(scene.objects.copy(), scene.primitives, scene.materials, scene.meshlets, scene.groups, scene.group_indices,
                   scene.meshlet_data, scene.positions, name="small without trees")
    bare.local_to_world = scene.local_to_world
    assert scene.bvh_nodes is not None and bare.bvh_nodes is None
    r = VisibilityRenderer(0)
    r.set_cull_mode(1)
    r.allocate_gbuffer(320, 200)
    try:
        L.fill_objects(scene, cam0)
        r.upload_scene(scene)
        _leg(r, scene, cam0, 3, "hierarchical, with trees")
        L.fill_objects(bare, cam0)
        _refused(r.upload_scene, bare)
        assert "BVH" in r.last_error()
        for call, args in ((r.render_frame, ()), (r.instance_culling, ()), (r.last_frame_cmds, ()), (r.update_objects, (bare.objects,)),
                           (r.history_hzb, ()), (r.allocate_depth_views, (128, 2)), (r.visibility_mark, (L.CountAndCmd(),))):
            _refused(call, *args)
        r.set_cull_mode(0)
        r.upload_scene(bare)
        _leg(r, bare, cam0, 3, "flat, without trees")
        _refused(r.set_cull_mode, 1)                        # (the scene on the context has no trees)
        r.reset_history()                                   # the refused switch changed nothing: the next frames are exact too
        _leg(r, bare, cam0, 2, "flat, after the refused switch")
        r.upload_scene(scene)
        r.set_cull_mode(1)
        _leg(r, scene, cam0, 3, "hierarchical again")
    finally:
        r.close()


def test_scene_swap_out_of_a_hot_tile_scene(gpu):
    """The hotspot form of config 5 (reduced, 960 x 540, the limits test_gpu_parity.py gives it) in the block form with tiles hot from 64
    entries, so that the schedule kernel fills dHotTiles and reports long bins; then, on the same context and under the same
    switches, a scene with no long bin: raster_setup_blocks_kernel<true> runs over the hot-tile list and the report the OLD scene
    left (upload_scene keeps both), and the image is still the oracle's.  Then the switch goes and the default variant runs."""
    from chord_amd.renderer import VisibilityRenderer
    w, h = 960, 540
    hot, cam_h = scenes.config5_subpixel(w, h, prims=16, patches_per_prim=256, instances=4, hotspot_sigma_px=64.0)
    calm, cam_c = scenes.small_test_scene(w, h)
    r = VisibilityRenderer(0)
    r.set_limits(max_triangle_records=8 << 20, bin_pool_chunks=16384, bin_max_chunks_per_tile=2048)
    L.fill_objects(hot, cam_h)
    r.upload_scene(hot)
    r.allocate_gbuffer(w, h)
    r.set_debug(FORCE_BLOCKS | FORCE_HOT)
    try:
        tr = _Track()
        for k in range(3):                                  # (static, one pass: the flags test_config5_hotspot_reduced_matches_oracle uses)
            want = _frame([r], tr, hot, cam_h, "hotspot, frame %d" % k, NO_HZB_FLAGS, with_stats=False)[0]
        st = r.stats()
        assert st["trianglesSubmitted"] == want["stats"].trianglesSubmitted
        tiles = ((w + 63) // 64) * ((h + 63) // 64)
        assert st["overflow"] == 0 and st["tilesTouched"][0] < 0.5 * tiles and st["binEntries"] / max(1, st["tilesTouched"][0]) > 300
        L.fill_objects(calm, cam_c)
        r.upload_scene(calm)
        _leg(r, calm, cam_c, 3, "no long bin, hot-tile variant on the old scene's report")
        r.set_debug(FORCE_BLOCKS)
        tr = _Track()
        r.reset_history()
        for k, cam in enumerate(_path(cam_c, 2)):
            _frame([r], tr, calm, cam, "no long bin, default variant, frame %d" % k)
    finally:
        r.close()


# ---- 3. mode switches between frames, history retained ------------------------------------------------------------------------

def test_mode_switches_between_frames(gpu):
    """Eleven frames of one moving sequence on one context; between every two frames one thing changes.  The history survives every
    switch but reset_history, whose next frame is a frame without history (the pending tail of the frame before is dropped with it)."""
    from chord_amd.renderer import VisibilityRenderer
    scene, cam0 = _small()
    r = VisibilityRenderer(0)
    L.fill_objects(scene, cam0)
    r.upload_scene(scene)
    r.allocate_gbuffer(320, 200)
    # (frame, what happens before it, flags, read stats and the chain afterwards -- False: the frame's tail stays pending)
    steps = [(0, None, H.ALL_FLAGS, False),
             (1, lambda: r.set_cull_mode(1), H.ALL_FLAGS, True),
             (2, lambda: r.set_tile_schedule_keep(0), H.ALL_FLAGS, False),
             (3, None, NO_HZB_FLAGS, False),                                    # no HZB cull: one pass; the history is still built
             (4, lambda: r.set_cull_mode(0), H.ALL_FLAGS, True),                # ... and this frame culls against it
             (5, lambda: r.set_tile_schedule_keep(7), H.ALL_FLAGS, False),
             (6, lambda: r.reset_history(), H.ALL_FLAGS, False),                # frame 5's tail is pending here
             (7, lambda: r.enable_timers(1), H.ALL_FLAGS, True),
             (8, lambda: (r.enable_timers(0), r.set_tile_schedule_keep(1)), H.ALL_FLAGS, False),
             (9, lambda: r.read_visibility(), H.ALL_FLAGS, False),              # (a read-back in the middle of a kept-schedule run)
             (10, lambda: r.set_cull_mode(1), H.ALL_FLAGS, True)]
    try:
        tr = _Track()
        second = 0
        for (k, before, flags, with_stats), cam in zip(steps, _path(cam0, len(steps))):
            if before is not None:
                before()
            if k == 6:
                _refused(r.history_hzb)
                tr.hzb = None
            want = _frame([r], tr, scene, cam, "mode switches, frame %d" % k, flags, with_stats)[0]
            if k in (0, 3, 6):
                assert want["counts"][2] == 0 and want["counts"][3] == 0, (k, list(want["counts"]))   # one pass
            second = max(second, int(want["counts"][3]))
        assert second > 0
        assert r.tile_schedule_keep() == 1
    finally:
        r.close()


# ---- 4. chordvis_bind_objects ---------------------------------------------------------------------------------------------------

def test_bind_objects(gpu):
    """The object records in a caller-owned device tensor: between frames the test overwrites the tensor (ordered behind the
    context's stream by the frame's read-back, and in front of the next frame by a device-wide synchronise) and makes no library call
    about objects."""
    import torch
    from chord_amd.renderer import VisibilityRenderer
    w, h = 320, 180
    scene, cam, _ = scenes.general_transform_scene(w, h)
    cams = scenes.general_cameras(cam, steps=8)
    n = len(scene.objects)
    dev = torch.device("cuda", 0)
    bound = torch.zeros(n * R.OBJECT.itemsize, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def write(objs):
        bound.copy_(torch.from_numpy(np.ascontiguousarray(objs, dtype=R.OBJECT).view(np.uint8).copy()))
        torch.cuda.synchronize()

    def scribble():
        bound.fill_(0x7F)
        torch.cuda.synchronize()

    r = VisibilityRenderer(0)
    try:
        _refused(r.bind_objects, bound.data_ptr(), n)       # before upload_scene
        H.moving_frame(scene, cams, 0)
        r.upload_scene(scene)
        r.allocate_gbuffer(w, h)
        for bad in (n - 1, n + 1, 0):
            _refused(r.bind_objects, bound.data_ptr(), bad)
        _refused(r.bind_objects, None, n)
        # depth views made while the library's own copy is current: the child must pick the bound array up by itself
        cfg = R.default_cascade_config(cascadeCount=3, realtimeCascadeCount=2, cascadeDim=128, cascadeEndDistance=14.0,
                                       farCascadeEndDistance=40.0)
        r.allocate_depth_views(128, 3)
        r.bind_objects(bound.data_ptr(), n)
        seq = H.moving_sequence(scene, cams)
        for k, view, iv, want in seq:
            what = "bound objects, frame %d" % k
            if k == 4:
                # back to the library's copy: what happens to the tensor afterwards changes nothing
                r.update_objects(scene.objects)
                scribble()
            elif k == 5:
                r.bind_objects(bound.data_ptr(), n)
                write(scene.objects)
            elif k < 4 or k == 6:
                write(scene.objects)                        # no library call about objects
            r.set_view(view, iv, H.ALL_FLAGS)
            r.render_frame()
            _check_frame(r, scene, want, w, h, what, with_stats=k > 0)
            if k == 2:
                # a depth view of this frame: the child re-reads the parent's object pointer (the moved objects, not the uploaded ones)
                views = L.cascade_setup(cfg, view, iv, LIGHT)
                r.set_instance_views(views)
                lst = r.instance_culling_view(1)
                want_cmds = orc.instance_culling(scene, view, views[1:2], H.ALL_FLAGS)
                assert len(want_cmds) > 0 and np.array_equal(r.read_cmds(lst), want_cmds), what + ": the cascade's list"
                depth = r.read_depth(r.render_mesh_depth(1, lst))
                want_depth, _ = orc.raster_depth(scene, views[1:2], want_cmds, 128, 128)
                assert (want_depth > 0).any() and np.array_equal(depth.view(np.uint32), want_depth.view(np.uint32)), what + ": the cascade's depth"
            if k == 3:
                # the rule of include/chordvis.h: bind_objects counts as a change of the objects, like update_objects
                r.resolve_attributes(names=["barycentrics"])
                r.bind_objects(bound.data_ptr(), n)
                with pytest.raises(L.ChordvisError, match="came after the frame"):
                    r.resolve_attributes(names=["barycentrics"])
            if k == 6:
                break
        # upload_scene returns to the owned copy (and drops the history): the frame equals the oracle's frame without one
        view, iv = H.moving_frame(scene, cams, 7)
        r.upload_scene(scene)
        scribble()
        r.set_view(view, iv, H.ALL_FLAGS)
        r.render_frame()
        _check_frame(r, scene, orc.frame(scene, view, iv, H.ALL_FLAGS), w, h, "after upload_scene over bound objects")
        r.sync()
    finally:
        r.close()
        del bound


# ---- 5. sharded <-> unsharded on the same contexts ------------------------------------------------------------------------------

def _check_rank(r, scene, want, w, h, what, with_stats):
    """A rank of a sharded frame against the oracle's whole frame: the resolved image, list 0 (made on request from the cull's masks),
    the history chain; returns its stats (the counts of a rank are held to the frame's by H.assert_rank_counts)."""
    H.assert_vis_equal(r.read_visibility(), want["vis"], w, h, what)
    got = r.read_cmds(r.last_frame_cmds())
    assert np.array_equal(got, want["cmds"]), "%s: list 0 (%d vs %d commands)" % (what, len(got), len(want["cmds"]))
    st = r.stats()
    assert st["overflow"] == 0, what
    mn, mx, rng = r.read_hzb(r.history_hzb())
    assert np.array_equal(mn, want["hzb_min"]) and np.array_equal(mx, want["hzb_max"]) and np.array_equal(rng, want["valid_range"]), what + ": history chain"
    return st


def _sharded_frames(ctxs, tr, scene, cams, what):
    for k, cam in enumerate(cams):
        # (a frame without history starts at phase a, the replicated cull; the others with the sharded cull -- tr is the frame before's here)
        want, _, _, sts = _frame(ctxs, tr, scene, cam, "%s, frame %d" % (what, k), check=_check_rank,
                                 render=lambda rs: H.sharded_frame(rs, sharded_cull=tr.hzb is not None))
        single = dict(zip(("countInstanceCulled", "countStage0Visible", "countStage0Rejected", "countStage1Visible"), map(int, want["counts"])))
        H.assert_rank_counts(sts, single)


def test_sharded_and_unsharded_on_the_same_contexts(gpu):
    """Two contexts render unsharded at 129 x 67, are resized to 320 x 200 and sharded over two ranks (host-staged gathers, both on
    device 0), take an explicit tile map, are re-sharded over three ranks with a third, new context -- the explicit map must be gone --
    and end unsharded again.  Every change of ownership or size drops the history: its first frame is a frame without one."""
    from chord_amd.renderer import VisibilityRenderer
    from chord_amd.sharding import tile_layout
    scene, cam0 = _small()
    cam_small, cam_big = _cam_at(cam0, 129, 67), _cam_at(cam0, 320, 200)
    ctxs = [VisibilityRenderer(0) for _ in range(2)]
    try:
        L.fill_objects(scene, cam_small)
        for r in ctxs:
            r.upload_scene(scene)
            r.allocate_gbuffer(129, 67)
        tr = _Track()
        for k, cam in enumerate(_path(cam_small, 2)):
            _frame(ctxs, tr, scene, cam, "unsharded 129 x 67, frame %d" % k, with_stats=k > 0)
        # resized and sharded over two ranks
        for rk, r in enumerate(ctxs):
            r.allocate_gbuffer(320, 200)
            r.set_shard(2, rk)
            assert np.array_equal(r.tile_owners(), tile_layout(320, 200, 2))
            _refused(r.history_hzb)
            _refused(r.render_frame)                        # (a sharded context renders through its phases)
        tr = _Track()
        cams = _path(cam_big, 5)
        _sharded_frames(ctxs, tr, scene, cams[:3], "two ranks")
        # an explicit map: every tile border a rank border; the history carries over (it is not sharded)
        tiles_x, tiles = 5, 20
        checker = np.array([(t % tiles_x + t // tiles_x) % 2 for t in range(tiles)], dtype=np.uint8)
        for r in ctxs:
            r.set_tile_owners(checker)
            assert np.array_equal(r.tile_owners(), checker)
        _sharded_frames(ctxs, tr, scene, cams[3:], "two ranks, checker map")
        # three ranks, one context new: the explicit map is gone
        ctxs.append(VisibilityRenderer(0))
        ctxs[2].upload_scene(scene)
        ctxs[2].allocate_gbuffer(320, 200)
        for rk, r in enumerate(ctxs):
            r.set_shard(3, rk)
            assert np.array_equal(r.tile_owners(), tile_layout(320, 200, 3)), "rank %d: the tile map after set_shard(3, .)" % rk
            _refused(r.history_hzb)
        _sharded_frames(ctxs, _Track(), scene, _path(cam_big, 2), "three ranks")
        ctxs.pop().close()
        # unsharded again
        for r in ctxs:
            r.set_shard(1, 0)
            assert r.resolved_visibility_ptr() == r.visibility_ptr() and not r.hzb_exchange()[0] and not r.hzb_final_exchange()[0]
            _refused(r.history_hzb)
            _refused(r.frame_phase_a)
        tr = _Track()
        for k, cam in enumerate(_path(cam_big, 3)):
            _frame(ctxs, tr, scene, cam, "unsharded again, frame %d" % k, with_stats=k != 1)
    finally:
        for r in ctxs:
            r.close()


# ---- 6. depth views and the cascade cache across re-allocation -------------------------------------------------------------------

def _shadow_tick(r, scene, cam, cfg, tick, hist, what, mask_want=None):
    """One chordvis_render_shadow against the replay with the cache `hist` (None: none).  Returns the new cache."""
    objs = L.fill_objects(scene, cam).copy()
    view, iv = L.make_views(cam)
    r.update_objects(objs)
    r.set_view(view, iv, H.ALL_FLAGS)
    depths, views, mask = r.render_shadow(cfg, LIGHT, tick)
    hist, replay_mask = _replay_shadow(scene.with_objects(objs), view, iv, cfg, tick, hist, H.ALL_FLAGS)
    n, dim = int(cfg["cascadeCount"][0]), int(cfg["cascadeDim"][0])
    assert mask == replay_mask, "%s: rendered cascades %s, replay %s" % (what, bin(mask), bin(replay_mask))
    if mask_want is not None:
        assert mask == mask_want, "%s: rendered cascades %s, expected %s" % (what, bin(mask), bin(mask_want))
    assert np.array_equal(views.view(np.uint8), hist["views"].view(np.uint8)), what + ": cascade views"
    for k in range(n):
        assert (depths[k].width, depths[k].height) == (dim, dim), what
        got = r.read_depth(depths[k])
        assert np.array_equal(got.view(np.uint32), hist["depths"][k].view(np.uint32)), "%s: cascade %d" % (what, k)
    return hist


@pytest.mark.parametrize("event", ["reallocated", "new_scene", "new_dim", "parent_resized"])
def test_cascade_cache_across_reallocation(gpu, event):
    """Three ticks of chordvis_render_shadow (five cascades of 128 x 128, two realtime), an event, one more tick with the same config
    and light.  Whatever makes new depth images must drop the cache -- every cascade is rendered, from a replay without history --;
    a new size of the PARENT's target leaves it alone (the cascades depend on the main view, not on its size): the replay with the
    history says which cascades are rendered, and from what."""
    from chord_amd.renderer import VisibilityRenderer
    scene, cam0 = _masked()
    cfg = R.default_cascade_config(cascadeCount=5, realtimeCascadeCount=2, cascadeDim=128, cascadeEndDistance=12.0,
                                   farCascadeEndDistance=60.0, shadowBiasConst=-8.0, shadowBiasSlope=-0.5)
    r = VisibilityRenderer(0)
    L.fill_objects(scene, cam0)
    r.upload_scene(scene)
    r.allocate_gbuffer(320, 200)
    try:
        hist = None
        for tick in range(3):
            hist = _shadow_tick(r, scene, cam0, cfg, tick, hist, "tick %d" % tick, 0b11111 if tick == 0 else 0b00011 | 1 << (2 + tick % 3))
        if event == "reallocated":
            r.allocate_depth_views(128, 5)
            _shadow_tick(r, scene, cam0, cfg, 3, None, "after allocate_depth_views", 0b11111)
        elif event == "new_scene":
            other, _ = _small()
            L.fill_objects(other, cam0)
            r.upload_scene(other)
            _shadow_tick(r, other, cam0, cfg, 3, None, "after upload_scene", 0b11111)
        elif event == "new_dim":
            cfg2 = R.default_cascade_config(cascadeCount=5, realtimeCascadeCount=2, cascadeDim=192, cascadeEndDistance=12.0,
                                            farCascadeEndDistance=60.0, shadowBiasConst=-8.0, shadowBiasSlope=-0.5)
            _shadow_tick(r, scene, cam0, cfg2, 3, None, "another cascadeDim", 0b11111)
        else:
            r.allocate_gbuffer(129, 67)
            _refused(r.render_shadow, cfg, LIGHT, 3)        # (the main view does not fit the new target: set_view comes first)
            hist = _shadow_tick(r, scene, _cam_at(cam0, 129, 67), cfg, 3, hist, "after the parent's allocate_gbuffer", 0b00011 | 1 << 2)
            _shadow_tick(r, scene, _cam_at(cam0, 129, 67), cfg, 4, hist, "the tick after", 0b00011 | 1 << 3)
        # the main view renders exactly after all of it
        cam = cam0 if event != "parent_resized" else _cam_at(cam0, 129, 67)
        shown = scene if event != "new_scene" else _small()[0]
        r.reset_history()
        _frame([r], _Track(), shown, cam, "main view after the shadow passes (%s)" % event)
    finally:
        r.close()
