"""Object records built on the device from resident f64 world transforms (chordvis_upload_world_transforms,
chordvis_scatter_world_transforms, chordvis_build_objects) against the host function chordvis_object_basic_data, byte for byte: the
records themselves on the input set of tests/spec_object_build_np.py, the library's own copy of the previous transforms across
builds and scatters, whole frames of the moving sequence against the oracle, the state rules of the header, a depth view, frames
enqueued ahead of the device, and the group forms.  tests/test_object_build_spec.py holds the input set and the numpy spec to the host
function.  No tolerances anywhere."""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers as H
import inflight as IF
import orc
import spec_object_build_np as SOB
from chord_amd import records as R, scenes

pytestmark = pytest.mark.gpu

COUNTS = [1, 63, 64, 65, 256, 257, 1000]      # around the kernel's 64 objects per workgroup, and several workgroups with a ragged end


@functools.lru_cache(maxsize=None)
def _one_primitive():
    """One small primitive (a coarse bumpy sphere through the builder) under a single object: the geometry every scene here shares"""
    return scenes.scene_from_meshes([scenes.bumpy_sphere_mesh(10)], [np.eye(4)], name="object_build")


def _scene_of(n):
    """n objects of the one primitive; the 16 bytes behind basicData differ from object to object (material 0 / 1, the pads)"""
    objs = np.zeros(n, dtype=R.OBJECT)
    objs["GLTFMaterialData"] = np.arange(n) % 2
    objs["pad1"] = np.arange(n) + 7
    objs["pad2"] = 0xABCD0000 + np.arange(n)
    return _one_primitive().with_objects(objs)


@functools.lru_cache(maxsize=None)
def _host(case_index):
    """chordvis_object_basic_data on a case of the input set, object by object, once per process: ((n, 208) uint8, singular)"""
    case = SOB.input_set()[case_index]
    return SOB.host_records(case["cur"], case["prev"], case["cam"], case["cam_last"])


def _renderer(scene, w=0, h=0):
    from chord_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(0)
    r.upload_scene(scene)
    if w:
        r.allocate_gbuffer(w, h)
    return r


def _assert_records(got, want_basic, want_tail, what):
    bad = np.flatnonzero((SOB.basic_bytes(got) != want_basic).any(axis=1))
    assert len(bad) == 0, "%s: basicData of %d objects differs from chordvis_object_basic_data, first %s" % (what, len(bad), bad[:8])
    assert np.array_equal(SOB.tail_bytes(got), want_tail), what + ": the 16 bytes behind basicData changed"


def _device(indices, matrices):
    """(int32 tensor, float64 tensor) on device 0, there before anything of a context's stream reads them"""
    import torch
    idx = torch.from_numpy(np.ascontiguousarray(indices, dtype=np.uint32).view(np.int32).copy()).cuda()
    mats = torch.from_numpy(np.ascontiguousarray(matrices, dtype=np.float64).reshape(-1, 16).copy()).cuda()
    torch.cuda.synchronize()
    return idx, mats


# ---- 1. records ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", COUNTS)
def test_built_records_equal_the_host_function(gpu, n):
    scene = _scene_of(n)
    r = _renderer(scene)
    try:
        assert r.build_objects_status() == (0, 0xFFFFFFFF)                   # no build yet
        for ci, case in enumerate(SOB.input_set()):
            cur, prev = SOB.cycled(case, n)
            idx = np.arange(n) % len(case["cur"])
            want, singular = _host(ci)
            r.upload_world_transforms(cur, prev)
            r.build_objects(case["cam"], case["cam_last"])
            what = "%d objects, %s" % (n, case["name"])
            _assert_records(r.read_objects(), want[idx], SOB.tail_bytes(scene.objects), what)
            at = np.flatnonzero(singular[idx])
            assert r.build_objects_status() == (len(at), int(at[0]) if len(at) else 0xFFFFFFFF), what
            got_cur, got_prev = r.read_world_transforms()
            assert np.array_equal(got_cur, cur) and np.array_equal(got_prev, cur), what + ": prev = cur after the build"
        # the defaults: no previous transforms, no last camera
        case = SOB.input_set()[2]
        cur, _ = SOB.cycled(case, n)
        want, _ = SOB.host_records(case["cur"], None, case["cam"], None)
        r.upload_world_transforms(cur)
        r.build_objects(case["cam"])
        _assert_records(r.read_objects(), want[np.arange(n) % len(case["cur"])], SOB.tail_bytes(scene.objects), "%d objects, defaults" % n)
    finally:
        r.close()


# ---- 2. history and scatter ---------------------------------------------------------------------------------------------------------

def _batch(cur, prev, cam, cam_last, tail_of):
    """chordvis_object_basic_data_batch with explicit prev arrays (no singular matrix among them) -> records.OBJECT array"""
    from chord_amd import lib as L
    objs = tail_of.copy()
    cam_c, last_c = (C.c_double * 3)(*cam), (C.c_double * 3)(*cam_last)
    cur, prev = np.ascontiguousarray(cur), np.ascontiguousarray(prev)
    assert L.lib.chordvis_object_basic_data_batch(len(objs), cur.ctypes.data, prev.ctypes.data, cam_c, last_c, objs.ctypes.data) == L.OK
    return objs


def _fill_static(scene, cur, cam, cam_last):
    """lib.fill_objects(scene, cam, cam_last, None) for the given transforms: what a static object under a moving camera gets"""
    from chord_amd import lib as L
    sc = scene.with_objects(scene.objects.copy())
    sc.local_to_world = np.ascontiguousarray(cur)
    return L.fill_objects(sc, scenes.Camera(tuple(cam), (0.0, 0.0, -1.0), 64, 64), scenes.Camera(tuple(cam_last), (0.0, 0.0, -1.0), 64, 64), None)


@pytest.mark.parametrize("k", [0, 1, 65])
def test_history_and_scatter(gpu, k):
    n = 257
    case = SOB.input_set()[3]
    regular = np.array([i for i in range(len(case["cur"])) if i not in case["singular"]])
    idx = regular[np.arange(n) % len(regular)]
    cur0, prev0 = case["cur"][idx].copy(), case["prev"][idx].copy()
    cams = [case["cam"], case["cam"] + np.array([0.5, 0.125, -0.25]), case["cam"] + np.array([0.75, 0.5, 0.25])]
    scene = _scene_of(n)
    r = _renderer(scene)
    try:
        r.upload_world_transforms(cur0, prev0)
        r.build_objects(cams[0], case["cam_last"])
        # a second build without a scatter: static last-frame matrices under a moved camera
        r.build_objects(cams[1], cams[0])
        want = _batch(cur0, cur0, cams[1], cams[0], scene.objects)
        assert r.read_objects().tobytes() == want.tobytes(), "second build, nothing scattered"
        assert want.tobytes() == _fill_static(scene, cur0, cams[1], cams[0]).tobytes()
        # a scatter of k objects (spread over the workgroups, not in order), one index out of range in the list
        moved = (np.arange(k) * 97 + 5) % n
        assert len(set(moved.tolist())) == k
        new = cur0.copy()
        new[moved, 0:3] *= 1.5                             # (column 0 longer, the object somewhere else: regular like before)
        new[moved, 12:15] += np.array([0.25, -0.5, 0.125])
        lst = np.concatenate([moved[:k // 2], [n + 3], moved[k // 2:]]).astype(np.uint32) if k else np.zeros(0, dtype=np.uint32)
        mats = np.concatenate([new[moved[:k // 2]], case["cur"][:1] * 3.0, new[moved[k // 2:]]]) if k else np.zeros((0, 16))
        ti, tm = _device(lst, mats) if k else _device([0], np.zeros((1, 16)))
        r.scatter_world_transforms(ti, tm, n=len(lst))
        r.build_objects(cams[2], cams[1])
        want = _batch(new, cur0, cams[2], cams[1], scene.objects)
        got = r.read_objects()
        assert got.tobytes() == want.tobytes(), "scatter of %d objects, then a build" % k
        got_cur, got_prev = r.read_world_transforms()
        assert np.array_equal(got_cur, new) and np.array_equal(got_prev, new)
        assert r.build_objects_status() == (0, 0xFFFFFFFF)
        if k == 1:
            # two scatter calls to one index: the later one wins
            a, b = cur0[moved[:1]] * 2.0, cur0[moved[:1]] * 0.5
            t1, t2 = _device(moved[:1], a), _device(moved[:1], b)
            r.scatter_world_transforms(*t1)
            r.scatter_world_transforms(*t2)
            r.build_objects(cams[0], cams[2])
            newer = new.copy()
            newer[moved[0]] = b[0]
            assert r.read_objects().tobytes() == _batch(newer, new, cams[0], cams[2], scene.objects).tobytes(), "two scatters to one index"
            del t1, t2
        del ti, tm
    finally:
        r.close()


# ---- 3. frames ----------------------------------------------------------------------------------------------------------------------

def test_moving_frames_fed_by_scatter_and_build_match_oracle(gpu):
    from test_gpu_general_transforms import _check_frame, _resolved, _scene
    w, h = 333, 201                                        # the smallest size tests/test_gpu_general_transforms.py uses
    scene, cams = _scene(w, h)
    r, fed = _renderer(scene, w, h), _renderer(scene, w, h)
    try:
        scattered = 0
        for k, view, iv, want in H.moving_sequence(scene, cams):
            what = "frame %d" % k
            if k == 0:
                r.upload_world_transforms(scene.local_to_world_at(0))
                r.build_objects(cams[0].position)
            else:
                now, before = scene.local_to_world_at(k), scene.local_to_world_at(k - 1)
                changed = np.flatnonzero((now != before).any(axis=1))
                assert 0 < len(changed) < len(now), "some objects move and some stand"
                scattered += len(changed)
                ti, tm = _device(changed, now[changed])
                r.scatter_world_transforms(ti, tm)
                r.build_objects(cams[k].position, cams[k - 1].position)
            assert r.read_objects().tobytes() == scene.objects.tobytes(), what + ": the built records are the helper's"
            if k:
                del ti, tm
            assert r.build_objects_status() == (0, 0xFFFFFFFF)
            r.set_view(view, iv, H.ALL_FLAGS)
            r.render_frame()
            _check_frame(r, want, w, h, what, with_stats=k > 0)
            fed.update_objects(scene.objects)
            fed.set_view(view, iv, H.ALL_FLAGS)
            fed.render_frame()
        assert scattered > 0
        mv, mv_fed = _resolved(r, ["motionVector"])["motionVector"], _resolved(fed, ["motionVector"])["motionVector"]
        assert np.any(mv) and np.array_equal(mv, mv_fed), "motion vectors of the last frame"
    finally:
        r.close()
        fed.close()


# ---- 4. state rules -----------------------------------------------------------------------------------------------------------------

def test_state_rules(gpu):
    import torch
    from chord_amd import lib as L
    from test_gpu_general_transforms import _resolved
    scene, cam = scenes.small_test_scene(160, 96)
    w, h = cam.width, cam.height
    cam_b = cam.moved((0.3, 0.1, -0.2))
    l2w = scene.local_to_world.copy()
    n = len(scene.objects)
    objs_a = L.fill_objects(scene, cam).copy()
    objs_b = L.fill_objects(scene, cam_b).copy()
    view, iv = L.make_views(cam)
    r = _renderer(scene, w, h)
    try:
        def refused(call, *args, word=None):
            with pytest.raises(L.ChordvisError) as e:
                call(*args)
            assert "(%d)" % L.E_INVALID in str(e.value) and (word is None or word in str(e.value)), str(e.value)

        refused(r.build_objects, cam.position, word="chordvis_upload_world_transforms")        # before any transform upload
        refused(r.upload_world_transforms, l2w[:-1], word="objectCount")                       # a wrong count
        refused(r.upload_world_transforms, np.concatenate([l2w, l2w[:1]]), word="objectCount")
        refused(r.build_objects, cam.position)                                                 # (a refused upload kept nothing)
        r.upload_world_transforms(l2w)
        refused(lambda: r.read_world_transforms(n + 1))
        refused(lambda: r.read_objects(n - 1))
        r.build_objects(cam.position)
        assert r.read_objects().tobytes() == objs_a.tobytes()
        r.upload_scene(scene)                                                                   # a new scene upload drops the transforms
        refused(r.build_objects, cam.position, word="chordvis_upload_world_transforms")
        refused(lambda: r.scatter_world_transforms(*_device([0], l2w[:1])))
        r.upload_world_transforms(l2w)

        # a resolve straight after a build is refused, and works again after a frame
        r.build_objects(cam.position)
        r.set_view(view, iv, H.ALL_FLAGS)
        r.render_frame()
        first = _resolved(r, ["motionVector"])["motionVector"]
        r.build_objects(cam.position)
        refused(lambda: r.resolve_attributes(names=["motionVector"]))
        r.render_frame()
        assert np.array_equal(_resolved(r, ["motionVector"])["motionVector"], first)

        # bind_objects after a build reads the bound array; the next build returns to the library's own
        bound = torch.from_numpy(objs_b.view(np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        r.bind_objects(bound.data_ptr(), n)
        assert r.read_objects().tobytes() == objs_b.tobytes()
        assert np.array_equal(r.read_cmds(r.instance_culling()), orc.instance_culling(scene.with_objects(objs_b), view, iv, H.ALL_FLAGS))
        r.build_objects(cam.position)
        assert r.read_objects().tobytes() == objs_a.tobytes()
        assert np.array_equal(r.read_cmds(r.instance_culling()), orc.instance_culling(scene.with_objects(objs_a), view, iv, H.ALL_FLAGS))
        del bound

        # update_objects followed by a build: the built records, with the ids and pads the update brought
        marked = objs_b.copy()
        marked["pad1"] = 5
        r.update_objects(marked)
        r.build_objects(cam.position)
        got = r.read_objects()
        assert np.array_equal(SOB.basic_bytes(got), SOB.basic_bytes(objs_a)) and np.array_equal(SOB.tail_bytes(got), SOB.tail_bytes(marked))

        # a misaligned matrix array is refused; an empty scatter is not, and launches nothing
        ti, tm = _device([0, 1], np.zeros((3, 16)))
        refused(lambda: r.scatter_world_transforms(ti.data_ptr(), tm.data_ptr() + 8, 2), word="16-byte")
        r.scatter_world_transforms(ti.data_ptr(), tm.data_ptr() + 8, 0)
        r.scatter_world_transforms(0, 0, 0)
        cur, _ = r.read_world_transforms()
        assert np.array_equal(cur, l2w)
        del ti, tm
    finally:
        r.close()


# ---- 5. depth view ------------------------------------------------------------------------------------------------------------------

def test_depth_view_cull_reads_the_built_records(gpu):
    from chord_amd import lib as L
    scene, cam = scenes.small_test_scene(160, 96)
    objs = L.fill_objects(scene, cam).copy()
    view, iv = L.make_views(cam)
    cfg = R.default_cascade_config(cascadeCount=3, realtimeCascadeCount=2, cascadeDim=128, cascadeEndDistance=14.0, farCascadeEndDistance=40.0)
    views = L.cascade_setup(cfg, view, iv, (0.35, -1.0, 0.25))          # orthographic views; the first one is culled
    r = _renderer(scene, cam.width, cam.height)
    try:
        r.set_view(view, iv, H.ALL_FLAGS)
        r.allocate_depth_views(128, 3)
        r.set_instance_views(views)
        r.upload_world_transforms(scene.local_to_world)
        r.build_objects(cam.position)
        built = r.read_cmds(r.instance_culling_view(0))
        r.update_objects(objs)
        fed = r.read_cmds(r.instance_culling_view(0))
        assert len(built) > 0 and np.array_equal(built, fed)
        assert np.array_equal(built, orc.instance_culling(scene.with_objects(objs), view, views[0:1], H.ALL_FLAGS))
    finally:
        r.close()


# ---- 6. in flight -------------------------------------------------------------------------------------------------------------------

def _camera_of(frame):
    """The camera position a frame's view was made for (ChordInstanceCullingView::cameraWorldPos holds the doubles)"""
    return np.frombuffer(frame.iv["cameraWorldPos"][0].tobytes(), dtype=np.float64)[:3].copy()


def test_scatter_and_build_are_enqueued_ahead_of_the_device(gpu):
    """Frames 1..3 of the moving small scene as (scatter, build, set_view, render_frame, snapshot) behind a closed gate on a
    caller-owned stream: every call returns with the gate closed, the two camera arrays are overwritten as soon as a build call
    has returned, and the images are the oracle's -- and those of the same frames run one by one."""
    from chord_amd import lib as L
    sc = IF.moving("small")
    l2w = sc.scene.local_to_world_at(0)
    camera = [_camera_of(f) for f in sc.frames]
    some = np.arange(0, len(l2w), 3)

    def prepare():
        ctx = IF.Context(sc)
        ctx.tensors = _device(some, l2w[some])
        ctx.r.upload_world_transforms(l2w)
        ctx.r.build_objects(camera[0])
        ctx.r.set_view(sc.frames[0].view, sc.frames[0].iv, sc.flags)
        ctx.render_frame()
        ctx.synchronize()
        return ctx

    def script(ctx):
        cam, last = (C.c_double * 3)(), (C.c_double * 3)()
        ti, tm = ctx.tensors

        def build(k):
            cam[:], last[:] = camera[k].tolist(), camera[k - 1].tolist()
            ctx.r._check(L.lib.chordvis_build_objects(ctx.r._ctx, cam, last), "build_objects")
            cam[:], last[:] = [1e30, -1e30, 3.0], [7.0, 1e-30, -2.0]           # the caller's arrays are free on return

        calls = []
        for k in (1, 2, 3):
            f = sc.frames[k]
            calls += [("scatter_world_transforms[%d]" % k, lambda: ctx.r.scatter_world_transforms(ti.data_ptr(), tm.data_ptr(), len(some)), False),
                      ("build_objects[%d]" % k, lambda k=k: build(k), False),
                      ("set_view[%d]" % k, lambda f=f: ctx.r.set_view(f.view, f.iv, sc.flags), False),
                      ("render_frame[%d]" % k, ctx.render_frame, False),
                      ("snapshot[%d]" % k, lambda k=k: ctx.snaps.__setitem__(k, ctx.snapshot(hzb=False)), False)]
        return calls

    what = "scatter + build, three frames in flight"
    ctx, log, _ = IF.run_behind_gate(prepare, script, what)
    try:
        assert IF.waits(log) == {"scatter_world_transforms": False, "build_objects": False, "set_view": False, "render_frame": False,
                                 "snapshot": False}
        for k in (1, 2, 3):
            IF.check_frame(ctx.snaps[k], sc.frames[k].want, "%s, frame %d" % (what, k), hzb=False, counts=True)
        images = {k: IF.host(ctx.snaps[k]["vis"], np.uint64).copy() for k in (1, 2, 3)}
        ctx.snaps.clear()
        ctx.tensors = None
    finally:
        ctx.close()
    r = _renderer(sc.scene, sc.w, sc.h)                    # the same frames one by one
    try:
        r.upload_world_transforms(l2w)
        for k in range(4):
            r.build_objects(camera[k], camera[k - 1] if k else None)
            r.set_view(sc.frames[k].view, sc.frames[k].iv, sc.flags)
            r.render_frame()
            r.sync()
            if k:
                H.assert_vis_equal(images[k], r.read_visibility(), sc.w, sc.h, "in flight vs one by one, frame %d" % k)
    finally:
        r.close()


# ---- 7. group -----------------------------------------------------------------------------------------------------------------------

def test_group_upload_and_build_give_the_single_context_image(gpu):
    from chord_amd import lib as L
    from chord_amd.renderer import VisibilityGroup
    scene, cam = scenes.small_test_scene(320, 200, seed=17)
    w, h = cam.width, cam.height
    cam1 = cam.moved((0.2, 0.05, -0.1))
    view0, iv0 = L.make_views(cam)
    view1, iv1 = L.make_views(cam1, view0)
    ref = _renderer(scene, w, h)
    g = VisibilityGroup([0, 0])
    try:
        g.upload_scene(scene)
        with pytest.raises(L.ChordvisError):
            g.build_objects(cam.position)                                         # no transforms on the ranks yet
        g.allocate_gbuffer(w, h)
        with pytest.raises(L.ChordvisError):
            g.upload_world_transforms(scene.local_to_world[:-1])
        g.upload_world_transforms(scene.local_to_world)
        for c, last, view, iv in ((cam, None, view0, iv0), (cam1, cam, view1, iv1)):
            ref.update_objects(L.fill_objects(scene, c, last).copy())
            ref.set_view(view, iv, H.ALL_FLAGS)
            ref.render_frame()
            g.build_objects(c.position, last.position if last else None)
            g.set_view(view, iv, H.ALL_FLAGS)
            g.render_frame()
        g.sync()
        want = ref.read_visibility()
        assert np.any(want)
        for rk, r in enumerate(g.ranks):
            assert r.read_objects(len(scene.objects)).tobytes() == scene.objects.tobytes(), "rank %d records" % rk
            H.assert_vis_equal(r.read_visibility(), want, w, h, "rank %d" % rk)
    finally:
        g.close()
        ref.close()
