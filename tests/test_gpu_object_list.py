"""chordvis_set_object_list on the GPU: another object list for a resident scene, held to what include/chordvis.h promises (OBJECTS COME
AND GO) -- the tables byte for byte (tests/spec_object_list_np.py), every frame against orc.frame and against a fresh context that
uploaded the same list, the history HZB kept, what is kept and what is dropped, and refusals that change nothing.

The lists are picked from a POOL scene with spec_object_list_np.relist: the same assets, primitives and materials, other objects.  A
frame's object records (basicData) travel with the list, so every list is filled for its frame's camera before it is handed over."""
import functools

import numpy as np
import pytest

import helpers as H
import inflight as IF
import orc
import spec_object_list_np as S
from chord_amd import lib as L, records as R, scenes
from test_depth_views import LIGHT
from test_gpu_cull_paths import MOVES, _check_frame, cull_blocks

pytestmark = pytest.mark.gpu


# ---- scenes and lists ---------------------------------------------------------------------------------------------------------

def _with_two_sided(scene):
    """The scene with one more material, two-sided, that no object names (group_count_scene has the one-sided default alone)."""
    two = scenes.SceneBuilder._material(1)
    out = scene.with_objects(materials=np.concatenate([scene.materials, two]))
    out.local_to_world = scene.local_to_world
    return out


@functools.lru_cache(maxsize=None)
def _pool(which):
    """(pool scene, camera, width, height): 'small' = small_test_scene(160, 96), 'groups257' = group_count_scene(257) -- four 64-group
    panels and a one-group tile, two count blocks."""
    if which == "small":
        scene, cam = scenes.small_test_scene(160, 96)
        return scene, cam, 160, 96
    scene, cam = scenes.group_count_scene(257)
    return _with_two_sided(scene), cam, cam.width, cam.height


def _orders(scene):
    """{name: (order into the pool's objects, material ids or None)}"""
    n = len(scene.objects)
    mats = scene.objects["GLTFMaterialData"].copy()
    one_sided = int(np.flatnonzero(scene.materials["bTwoSided"][mats] == 0)[0])
    two_sided = int(np.flatnonzero(scene.materials["bTwoSided"] != 0)[0])
    mats[one_sided] = two_sided
    return {"reversed": (list(range(n))[::-1], None),
            "subset": ([k for k in range(n) if k % 3 != 1], None),
            "repeated": ([0, 2, 2, 1, 2] + list(range(3, n)), None),       # (one primitive three times)
            "unnamed": (list(range(n)), None),                             # (the whole pool: names the primitive the upload left out)
            "material": (list(range(n)), mats)}                            # (an object goes from one-sided to two-sided)


def _uploaded(scene):
    """The list the context under test uploads: the pool without the objects of its LAST object's primitive, which every list that
    names that object then names for the first time."""
    prim = scene.objects["GLTFPrimitiveDetail"]
    keep = [k for k in range(len(prim)) if prim[k] != prim[-1]]
    assert 0 < len(keep) < len(prim)
    return S.relist(scene, keep)


def _renderer(scene, w=0, h=0, cull_mode=0):
    from chord_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(0)
    r.upload_scene(scene)
    if w:
        r.allocate_gbuffer(w, h)
    if cull_mode:
        r.set_cull_mode(cull_mode)
    return r


def _tables(r, scene):
    """(group-ref table, static table) of the context as bytes, at the sizes the spec gives for `scene` (chordvis_debug_read 8 / 9)."""
    refs = np.zeros(scene.group_instances * 24, dtype=np.uint8)
    stat = np.zeros(len(scene.objects) * 48, dtype=np.uint8)
    for which, out in ((8, refs), (9, stat)):
        if len(out):
            r._check(L.lib.chordvis_debug_read(r._ctx, which, 0, out.nbytes, out.ctypes.data), "debug_read %d" % which)
        # one byte past the table is past the current list
        one = np.zeros(1, dtype=np.uint8)
        assert L.lib.chordvis_debug_read(r._ctx, which, out.nbytes, 1, one.ctypes.data) == L.E_INVALID
    return refs.tobytes(), stat.tobytes()


def _refused(call, *args, match=None):
    with pytest.raises(L.ChordvisError, match=match):
        call(*args)


class _Track:
    """The oracle's side of a context's life: the last frame's view, camera and chain."""

    def __init__(self):
        self.view = self.cam = self.hzb = None


def _frame(rs, tr, scene, cam, what, new_list=False, with_stats=True, flags=H.ALL_FLAGS, render=None, check=_check_frame):
    """The next frame on every context of rs against orc.frame with the oracle's own previous chain.  new_list: `scene` reaches the
    contexts through set_object_list (records filled for this frame), else its records through update_objects.  render(rs): default
    render_frame each.  Returns (oracle frame, view, iv, [what check returned per context])."""
    L.fill_objects(scene, cam, tr.cam)
    view, iv = L.make_views(cam, tr.view)
    want = orc.frame(scene, view, iv, flags, prev_hzb_min=tr.hzb)
    for r in rs:
        if new_list:
            r.set_object_list(scene)
        else:
            r.update_objects(scene.objects)
        r.set_view(view, iv, flags)
    if render is None:
        for r in rs:
            r.render_frame()
    else:
        render(rs)
    got = [check(r, scene, want, cam.width, cam.height, "%s, context %d" % (what, i), with_stats) for i, r in enumerate(rs)]
    tr.view, tr.cam, tr.hzb = view, cam, want["hzb_min"]
    return want, view, iv, got


def _check_rank(r, scene, want, w, h, what, with_stats):
    """A rank of a sharded frame against the oracle's whole frame: the resolved image, list 0 (made on request from the cull's masks)
    and -- with_stats -- the history chain; returns its stats (a rank's counts are held to the frame's by H.assert_rank_counts)."""
    H.assert_vis_equal(r.read_visibility(), want["vis"], w, h, what)
    got = r.read_cmds(r.last_frame_cmds())
    assert np.array_equal(got, want["cmds"]), "%s: list 0 (%d vs %d commands)" % (what, len(got), len(want["cmds"]))
    if not with_stats:
        return None
    st = r.stats()
    assert st["overflow"] == 0, what
    mn, mx, rng = r.read_hzb(r.history_hzb())
    assert np.array_equal(mn, want["hzb_min"]) and np.array_equal(mx, want["hzb_max"]) and np.array_equal(rng, want["valid_range"]), what + ": history chain"
    return st


COUNTS = ("countInstanceCulled", "countStage0Visible", "countStage0Rejected", "countStage1Visible", "trianglesSubmitted", "overflow")


# ---- 1. table bytes -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["small", "groups257"])
def test_tables_equal_the_spec_and_a_fresh_upload(gpu, which):
    pool = _pool(which)[0]
    r = _renderer(_uploaded(pool))
    try:
        for name, (order, mats) in _orders(pool).items():
            new = S.relist(pool, order, mats)
            r.set_object_list(new)
            want = (S.group_refs(new).tobytes(), S.obj_static(new).tobytes())
            assert _tables(r, new) == want, "%s %s: the context's tables against the spec" % (which, name)
            fresh = _renderer(new)
            try:
                assert _tables(fresh, new) == want, "%s %s: a fresh upload's tables against the spec" % (which, name)
            finally:
                fresh.close()
    finally:
        r.close()


# ---- 2. fresh-upload equivalence ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which,cull_mode", [("small", 0), ("small", 1), ("groups257", 0)], ids=["small", "small_hierarchical", "groups257"])
def test_frame_equals_the_oracle_and_a_fresh_upload(gpu, which, cull_mode):
    """One context, the five lists one after another (longer, shorter, longer again: the buffers grow and then hold more than the
    list); after reset_history one frame of each equals the oracle's frame of the scene with that list, and the frame of a context
    that uploaded it: image, list 0, the chains, the counts of chordvis_stats, the handle's capacity."""
    pool, cam, w, h = _pool(which)
    L.fill_objects(pool, cam)
    view, iv = L.make_views(cam)
    r = _renderer(_uploaded(pool), w, h, cull_mode)
    try:
        r.set_view(view, iv, H.ALL_FLAGS)
        r.render_frame()                                     # (the list before has rendered: there is a history to reset, and reports)
        for name, (order, mats) in _orders(pool).items():
            what = "%s mode %d, list %s" % (which, cull_mode, name)
            new = S.relist(pool, order, mats)
            want = orc.frame(new, view, iv, H.ALL_FLAGS)
            assert want["counts"][0] > 0 and want["vis"].any(), what
            r.set_object_list(new)
            r.history_hzb()                                  # (the history is kept -- test 4 --, so it is reset by hand here)
            r.reset_history()
            r.render_frame()
            st = _check_frame(r, new, want, w, h, what)
            fresh = _renderer(new, w, h, cull_mode)
            try:
                fresh.set_view(view, iv, H.ALL_FLAGS)
                fresh.render_frame()
                fst = _check_frame(fresh, new, want, w, h, what + " (fresh upload)")
                assert {k: st[k] for k in COUNTS} == {k: fst[k] for k in COUNTS}, what
                a, b = r.last_frame_cmds(), fresh.last_frame_cmds()
                assert a.capacity == b.capacity == max(1, new.lod0_meshlet_instances), what
            finally:
                fresh.close()
    finally:
        r.close()


# ---- 3. count edges, going up and coming down -----------------------------------------------------------------------------------

def _edge_walk(pool, cam, sizes, what):
    """One context: the pool's first sizes[0] objects uploaded, then the other prefixes in turn through set_object_list, a frame
    with the running history after each; returns the group-instance counts visited."""
    r = _renderer(S.relist(pool, range(sizes[0])), cam.width, cam.height)
    tr, visited = _Track(), []
    try:
        for k, n in enumerate(sizes):
            sub = S.relist(pool, range(n))
            c = cam if k == 0 else tr.cam.moved(MOVES[k % 2])
            _frame([r], tr, sub, c, "%s, %d objects (%d group instances)" % (what, n, sub.group_instances), new_list=k > 0, with_stats=k % 2 == 1)
            visited.append(sub.group_instances)
        return visited
    finally:
        r.close()


def test_one_count_block_against_two(gpu):
    """255, 256 and 257 group instances (objects of one group each) on one context: up across the block edge -- the tables, masks and
    block counts grow -- and down again under what is allocated."""
    pool, cam = scenes.group_count_scene(257, panels=False)
    visited = _edge_walk(pool, cam, [255, 256, 257, 256, 255, 257], "count block edge")
    assert visited == [255, 256, 257, 256, 255, 257] and [cull_blocks(g) for g in visited] == [1, 1, 2, 1, 1, 2]


def test_either_side_of_the_quad_count_limit_on_one_context(gpu):
    """512 count blocks (the quad count kernel) and 513 (object_cull_kernel + count + self-summing scatter: launch_group_cull's
    boundary) from a pool of 512 * 256 + 70 group instances: up, and down again."""
    pool, cam = scenes.group_count_scene(512 * 256 + 70)
    assert pool.group_instances == 512 * 256 + 70 and len(pool.objects) == 2049 + 6
    visited = _edge_walk(pool, cam, [2048, 2049, 2048], "quad count limit")
    assert [cull_blocks(g) for g in visited] == [512, 513, 512]


# ---- 4. the history is kept -----------------------------------------------------------------------------------------------------

def _history_case():
    """(scene A, scene B, camera 1, camera 2): group_count_scene(320) as objects of one group each -- 48 shown in staggered walls, the
    front wall hiding most of the one behind -- and the list without the front wall's objects, with two objects of the 64-group panel
    primitive (which A names nowhere) at either end of it."""
    a, cam = scenes.group_count_scene(320, panels=False)
    n = len(a.objects)
    shown = sorted(set(np.linspace(0, n - 1, 48).round().astype(np.int64).tolist()))
    front = set(shown[:32])                                  # (group_count_scene: the first 32 shown objects are the front layer)
    keep = [k for k in range(n) if k not in front]
    objs = np.concatenate([a.objects[:1], a.objects[keep], a.objects[:1]]).copy()
    objs["GLTFPrimitiveDetail"][0] = objs["GLTFPrimitiveDetail"][-1] = 0            # the panel
    b = a.with_objects(objs)
    l2w = lambda m: np.asarray(m, dtype=np.float64).T.reshape(1, 16)
    b.local_to_world = np.ascontiguousarray(np.concatenate([l2w(scenes.translate(-1.0, 0.2, 1.0)), a.local_to_world[keep],
                                                            l2w(scenes.translate(1.5, -0.5, -2.0))]))
    assert b.group_instances == 288 + 128 and set(a.objects["GLTFPrimitiveDetail"].tolist()) == {1}
    return a, b, cam, cam.moved(MOVES[0])


def _list_handles(r):
    """Handles of lists 1 and 2 (the occlusion cull's visible and rejected lists), from a throw-away pass sequence: their addresses
    stay while nothing grows; `capacity` is the current list's."""
    r.clear_gbuffer()
    post = r.instance_culling()
    tmp = r.build_hzb(True, False, False, slot=0)
    vis, rej = r.hzb_culling(tmp, True, post)
    r.reset_history()
    return vis, rej


def test_history_is_kept(gpu):
    """Frame 1 renders A; set_object_list(B); frame 2, without reset_history, equals the oracle's frame of B against frame 1's chain --
    image, the three lists, the chains -- and the inputs can tell: the oracle's frame 2 rejects clusters in phase 0 (what the removed wall
    hid) and differs from the same frame without a history."""
    a, b, cam1, cam2 = _history_case()
    w, h = cam1.width, cam1.height
    L.fill_objects(a, cam1)
    view1, iv1 = L.make_views(cam1)
    want1 = orc.frame(a, view1, iv1, H.ALL_FLAGS)
    L.fill_objects(b, cam2, cam1)
    view2, iv2 = L.make_views(cam2, view1)
    want2 = orc.frame(b, view2, iv2, H.ALL_FLAGS, prev_hzb_min=want1["hzb_min"])
    without = orc.frame(b, view2, iv2, H.ALL_FLAGS)
    vis0, rej0 = orc.hzb_culling(b, view2, H.ALL_FLAGS, 0, want2["desc"], want1["hzb_min"], want2["cmds"])
    vis1, _ = orc.hzb_culling(b, view2, H.ALL_FLAGS, 1, want2["desc"], orc.hzb_build(orc.raster(b, iv2, vis0, w, h)[0], w, h)[1], rej0)
    assert len(rej0) > 0 and len(rej0) == want2["counts"][2] and len(vis1) == want2["counts"][3] > 0
    assert without["counts"][1] != want2["counts"][1] and without["counts"][2] == 0        # (the stage-0 list differs without the history)

    r = _renderer(a, w, h)
    try:
        # the longest list once, up front: from here on nothing grows and the lists' addresses stand
        r.set_object_list(b)
        r.set_object_list(a)
        r.set_view(view1, iv1, H.ALL_FLAGS)
        h1, h2 = _list_handles(r)
        r.render_frame()
        _check_frame(r, a, want1, w, h, "frame 1 (A)", with_stats=False)     # (its HZB tail stays pending: frame 2's cull carries it)
        r.set_object_list(b)
        r.set_view(view2, iv2, H.ALL_FLAGS)
        r.render_frame()
        st = _check_frame(r, b, want2, w, h, "frame 2 (B, history kept)")
        assert st["countStage0Rejected"] == len(rej0) and st["countStage1Visible"] == len(vis1)
        cap = r.last_frame_cmds().capacity
        assert cap == b.lod0_meshlet_instances
        # (stage 1 writes its visible clusters over list 1's records and counts them in the fourth of the context's list counts, two
        # words past list 1's own: chordvis_hzb_culling, second stage)
        for handle, at, ref, name in ((h1, 8, vis1, "list 1 (visible in stage 1)"), (h2, 0, rej0, "list 2 (rejected in stage 0)")):
            got = r.read_cmds(L.CountAndCmd(handle.count + at, handle.cmds, cap))
            assert np.array_equal(H.sort_cmds(got), H.sort_cmds(ref)), name
    finally:
        r.close()


# ---- 5. frames in flight --------------------------------------------------------------------------------------------------------

def test_lists_change_between_frames_in_flight(gpu):
    """Frame A, set B, frame B, set A, frame A behind a closed gate on a caller-owned stream (tests/inflight.py): no call waits for
    the device -- B is shorter than A, nothing grows -- and the last frame's image, list and chains are the oracle's third frame."""
    pool, cam, w, h = _pool("small")
    L.fill_objects(pool, cam)
    view, iv = L.make_views(cam)
    sub = S.relist(pool, _orders(pool)["subset"][0])
    f1 = orc.frame(pool, view, iv, H.ALL_FLAGS)
    f2 = orc.frame(sub, view, iv, H.ALL_FLAGS, prev_hzb_min=f1["hzb_min"])
    f3 = orc.frame(pool, view, iv, H.ALL_FLAGS, prev_hzb_min=f2["hzb_min"])
    assert not np.array_equal(f2["vis"], f1["vis"]) and f2["counts"][0] < f1["counts"][0]
    sc = IF.Scenario("object_lists", pool, w, h, H.ALL_FLAGS, [])

    def prepare():
        ctx = IF.Context(sc)
        ctx.r.set_view(view, iv, H.ALL_FLAGS)
        ctx.synchronize()
        return ctx

    def script(ctx):
        return [("render_frame[0]", ctx.render_frame, False),
                ("set_object_list[1]", lambda: ctx.r.set_object_list(sub.objects), False),
                ("render_frame[1]", ctx.render_frame, False),
                ("snapshot[1]", lambda: ctx.snaps.__setitem__(1, ctx.snapshot(hzb=False)), False),
                ("set_object_list[2]", lambda: ctx.r.set_object_list(pool.objects), False),
                ("render_frame[2]", ctx.render_frame, False),
                ("snapshot[2]", lambda: ctx.snaps.__setitem__(2, ctx.snapshot(hzb=True)), False)]

    what = "A, set B, B, set A, A in flight"
    ctx, log, _ = IF.run_behind_gate(prepare, script, what)
    try:
        assert IF.waits(log) == {"render_frame": False, "set_object_list": False, "snapshot": False}
        IF.check_frame(ctx.snaps[1], f2, what + ", frame B", hzb=False, counts=True)
        IF.check_frame(ctx.snaps[2], f3, what + ", the last frame", hzb=True, counts=True)
        IF.check_stats(ctx, f3, what)
        ctx.snaps.clear()
    finally:
        ctx.close()


# ---- 6. the material textures are kept ------------------------------------------------------------------------------------------

def test_material_textures_are_kept(gpu):
    from test_gpu_material import _check as check_material
    scene, cam, view, iv = H.setup_scene(scenes.material_test_scene, 320, 200)
    w, h = cam.width, cam.height
    n = len(scene.objects)
    order = list(range(n))[::-1]
    mats = scene.objects["GLTFMaterialData"][order].copy()
    mats[0] = (mats[0] + 1) % len(scene.materials)           # one object under another material
    new = S.relist(scene, order, mats)
    r = _renderer(scene, w, h)
    try:
        r.upload_material_textures()
        r.set_view(view, iv, H.ALL_FLAGS)
        r.render_frame()
        check_material(r, scene, view, iv, "the uploaded list")
        memory = r.material_texture_memory()
        assert sum(memory) > 0
        r.set_object_list(new)
        assert r.material_texture_memory() == memory
        r.render_frame()
        want = orc.frame(new, view, iv, H.ALL_FLAGS, prev_hzb_min=orc.frame(scene, view, iv, H.ALL_FLAGS)["hzb_min"])
        _check_frame(r, new, want, w, h, "the new list", with_stats=False)
        got = check_material(r, new, view, iv, "the new list")
        assert np.any(got["baseColor"])
        assert r.material_texture_memory() == memory
    finally:
        r.close()


# ---- 7. what is dropped ---------------------------------------------------------------------------------------------------------

def test_what_the_call_drops(gpu):
    import torch
    pool, cam, w, h = _pool("small")
    L.fill_objects(pool, cam)
    view, iv = L.make_views(cam)
    sub = S.relist(pool, _orders(pool)["subset"][0])
    # two far cascades: under a valid cache a tick renders one of them (isCascadeCacheValid), without one both
    cfg = R.default_cascade_config(cascadeCount=2, realtimeCascadeCount=0, cascadeDim=64, cascadeEndDistance=12.0, farCascadeEndDistance=60.0)
    r = _renderer(pool, w, h)
    fresh = _renderer(sub, w, h)
    try:
        r.set_view(view, iv, H.ALL_FLAGS)
        fresh.set_view(view, iv, H.ALL_FLAGS)
        r.reset_geometry_feedback()
        r.upload_world_transforms(pool.local_to_world)
        r.build_objects(cam.position)
        r.render_frame()
        r.geometry_feedback()
        r.resolve_attributes(names=["barycentrics"])
        assert r.render_shadow(cfg, LIGHT, 0)[2] == 0b11
        assert r.render_shadow(cfg, LIGHT, 1)[2] == 0b10     # (the cache holds: tick 1 renders cascade 1 alone; tick 2 would render cascade 0)
        # a bound array of other records (all zero: nothing would be drawn from it)
        bound = torch.zeros(len(sub.objects) * R.OBJECT.itemsize, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()

        r.set_object_list(sub)
        r.bind_objects(bound.data_ptr(), len(sub.objects))
        r.set_object_list(sub)                               # ... returns the context to its own array, which receives the records
        assert r.read_objects(len(sub.objects)).tobytes() == sub.objects.tobytes()
        _refused(r.resolve_attributes, ["barycentrics"], match="no frame rendered yet")
        _refused(r.geometry_feedback, match="no frame rendered yet")
        _refused(r.build_objects, cam.position, match="upload_world_transforms")
        _refused(r.update_objects, pool.objects)             # (the count is the new list's)
        depths, views, mask = r.render_shadow(cfg, LIGHT, 2)
        fdepths, fviews, fmask = fresh.render_shadow(cfg, LIGHT, 2)
        assert mask == fmask == 0b11
        assert np.array_equal(views.view(np.uint8), fviews.view(np.uint8))
        drawn = 0
        for k in range(2):
            a, b = r.read_depth(depths[k]), fresh.read_depth(fdepths[k])
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "cascade %d" % k
            drawn += int(np.count_nonzero(a))
        assert drawn > 0
        r.render_frame()
        want = orc.frame(sub, view, iv, H.ALL_FLAGS, prev_hzb_min=orc.frame(pool, view, iv, H.ALL_FLAGS)["hzb_min"])
        _check_frame(r, sub, want, w, h, "the frame after the call", with_stats=False)
        r.resolve_attributes(names=["barycentrics"])
        _refused(r.geometry_feedback, match="geometry_feedback_reset")       # a frame has run, the counts are still gone
        r.reset_geometry_feedback()
        r.geometry_feedback()
        got = r.read_geometry_feedback(("objectSubmitted",))["objectSubmitted"]
        assert len(got) == len(sub.objects) and got.sum() == len(want["cmds"])      # (+1 per command of the frame's list 0)
        r.upload_world_transforms(sub.local_to_world)
        r.build_objects(cam.position)
        assert r.read_objects(len(sub.objects))["localToTranslatedWorld"].tobytes() == sub.objects["localToTranslatedWorld"].tobytes()
    finally:
        r.close()
        fresh.close()


# ---- 8. refusals leave the context intact ---------------------------------------------------------------------------------------

def test_refusals_change_nothing(gpu):
    pool, cam = scenes.group_count_scene(257)
    w, h = cam.width, cam.height
    r = _renderer(pool, w, h)
    tr = _Track()
    try:
        _frame([r], tr, pool, cam, "before the refusals", with_stats=False)
        objs = pool.objects.copy()
        bad_prim, bad_mat = objs.copy(), objs.copy()
        bad_prim["GLTFPrimitiveDetail"][2] = len(pool.primitives)
        bad_mat["GLTFMaterialData"][-1] = len(pool.materials)
        panels = np.zeros(65536, dtype=R.OBJECT)             # 65 536 x 256 meshlets = 2^24 cluster instances
        panels[:] = objs[0]
        assert int(objs["GLTFPrimitiveDetail"][0]) == 0 and S.totals(S.relist(pool, [0]))[1] == 256
        cases = [("count == 0", objs, 0, L.E_INVALID, "count must be at least 1"),
                 ("primitive id == primitiveCount", bad_prim, len(objs), L.E_INVALID, "primitive/material id out of range"),
                 ("material id == materialCount", bad_mat, len(objs), L.E_INVALID, "primitive/material id out of range"),
                 ("2^24 cluster instances", panels, len(panels), L.E_CAPACITY, "2^24-2 cluster instances")]
        before = _tables(r, pool)
        for name, arr, count, code, rule in cases:
            assert L.lib.chordvis_set_object_list(r._ctx, arr.ctypes.data, count) == code, name
            assert rule in r.last_error() and r.last_error().startswith("set_object_list:"), (name, r.last_error())
        assert _tables(r, pool) == before
        assert r.last_frame_cmds().capacity == pool.lod0_meshlet_instances
        # the old list still renders, with its history
        _frame([r], tr, pool, cam.moved(MOVES[0]), "after the refusals")
        # a context without a scene refuses too
        from chord_amd.renderer import VisibilityRenderer
        empty = VisibilityRenderer(0)
        try:
            assert L.lib.chordvis_set_object_list(empty._ctx, objs.ctypes.data, len(objs)) == L.E_INVALID
            assert "no scene" in empty.last_error()
        finally:
            empty.close()
    finally:
        r.close()


# ---- 9. sharded (last: the contexts of the emulated ranks and the group's workers) ----------------------------------------------

def test_sharded_ranks_and_group(gpu):
    from chord_amd.renderer import VisibilityGroup
    pool, cam, w, h = _pool("small")
    w, h = 320, 200                                          # (15 tiles: both ranks own some)
    cam = scenes.Camera(cam.position, cam.front, w, h, cam.fovy, cam.z_near, cam.z_far, cam.world_up, cam.jitter)
    L.fill_objects(pool, cam)
    view, iv = L.make_views(cam)
    uploaded = _uploaded(pool)
    L.fill_objects(uploaded, cam)
    ctxs = H.sharded_contexts(uploaded, view, iv, w, h, H.ALL_FLAGS, 2)
    g = VisibilityGroup([0, 0])
    try:
        tr = _Track()
        _frame(ctxs, tr, uploaded, cam, "two ranks, the uploaded list", render=lambda rs: H.sharded_frame(rs, sharded_cull=False), with_stats=False,
               check=_check_rank)
        c = cam
        for k, name in enumerate(("repeated", "subset", "unnamed")):
            order, mats = _orders(pool)[name]
            new = S.relist(pool, order, mats)
            for form in (True, False):                       # the sharded cull, then the replicated one
                c = c.moved(MOVES[k % 2])
                want, _, _, sts = _frame(ctxs, tr, new, c, "two ranks, list %s, sharded cull %s" % (name, form), new_list=form,
                                         render=lambda rs: H.sharded_frame(rs, sharded_cull=form), check=_check_rank)
                single = dict(zip(("countInstanceCulled", "countStage0Visible", "countStage0Rejected", "countStage1Visible"), map(int, want["counts"])))
                H.assert_rank_counts(sts, single)
        assert all(x.cull_exchange()[1] == ctxs[0].cull_exchange()[1] > 0 for x in ctxs)

        # the group: replicated over its ranks, a refusal on every rank alike
        g.upload_scene(uploaded)
        g.allocate_gbuffer(w, h)
        gt = _Track()
        for k, name in enumerate(("unnamed", "subset")):
            order, mats = _orders(pool)[name]
            new = S.relist(pool, order, mats)
            cg = cam if k == 0 else gt.cam.moved(MOVES[0])
            L.fill_objects(new, cg, gt.cam)
            gview, giv = L.make_views(cg, gt.view)
            want = orc.frame(new, gview, giv, H.ALL_FLAGS, prev_hzb_min=gt.hzb)
            g.set_object_list(new)
            g.set_view(gview, giv, H.ALL_FLAGS)
            g.render_frame()
            g.sync()
            for rk, x in enumerate(g.ranks):
                H.assert_vis_equal(x.read_visibility(), want["vis"], w, h, "group rank %d, list %s" % (rk, name))
                assert x.read_objects().tobytes() == new.objects.tobytes()
            gt.view, gt.cam, gt.hzb = gview, cg, want["hzb_min"]
        bad = new.objects.copy()
        bad["GLTFPrimitiveDetail"][0] = len(pool.primitives)
        _refused(g.set_object_list, bad, match="out of range")
        g.render_frame()
        g.sync()
        want = orc.frame(new, gview, giv, H.ALL_FLAGS, prev_hzb_min=gt.hzb)
        for rk, x in enumerate(g.ranks):
            H.assert_vis_equal(x.read_visibility(), want["vis"], w, h, "group rank %d after the refusal" % rk)
    finally:
        g.close()
        for x in ctxs:
            x.close()
