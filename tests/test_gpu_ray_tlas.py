"""chordvis_rebuild_ray_tlas / chordvis_readback_ray_tlas on the GPU, held to what include/chordvis.h promises (RAY QUERIES, "rebuilding
the TLAS"): the tree read back equals tests/spec_ray_tlas_np.py byte for byte -- node words, every box, leaf references -- on both
sides of CHORD_RAY_TLAS_GROUP_MAX; every hit word on the rebuilt tree equals the brute-force specification (tests/spec_rays_np.py); the
rebuild follows moved objects through every way objects change; build and rebuild answer alike; the refusals and their messages;
frames are untouched; and the calls do not wait for the device.

Two rules are not reachable from here: a depth-view child context has no handle in the ABI, and a refusal that finds a TLAS (more
than 4^12 objects) is beyond a test's size -- both read from the code (abi_raytlas.cpp refuses before it touches anything)."""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers as H
import inflight as IF
import ray_tlas_cases as TC
import spec_ray_tlas_np as T
import spec_rays_np as S
from chord_amd import lib as L, records as R, scenes

pytestmark = pytest.mark.gpu
F = np.float32
G = L.RAY_TLAS_GROUP_MAX


@functools.lru_cache(maxsize=None)
def _base():
    scene, cam = scenes.config1_single_meshlet()
    L.fill_objects(scene, cam)
    return scene, cam, S.lod0_triangles(scene)


@functools.lru_cache(maxsize=None)
def _list(kind, n):
    scene, cam, _ = _base()
    if kind == "grid":
        return TC.instances(scene, cam, n, 100 + n)
    if kind == "equal":
        return TC.equal_instances(scene, cam, n)
    return TC.plane_instances(scene, cam, n, 300 + n)


def _rays(cur, cam, seed):
    lo, hi = S.object_boxes(cur.objects, cur.primitives)
    lo, hi = lo.min(axis=0).astype(np.float64), hi.max(axis=0).astype(np.float64)
    n = 200
    r = scenes.rand01(seed, np.arange(7 * n)).reshape(n, 7)
    rays = S.make_rays(lo + r[:, :3] * (hi - lo), r[:, 3:6] * 2.0 - 1.0, 1e-2, 1e9)
    rays["tMax"][::5] = (r[::5, 6] * np.linalg.norm(hi - lo)).astype(F)
    return np.concatenate([rays, S.pixel_rays(L.make_views(cam)[0], 16, 16)])


@functools.lru_cache(maxsize=None)
def _hit_case(kind, n):
    """(list, rays, closest hits, any-hit) of the specification, once."""
    scene, cam, tris = _base()
    cur = _list(kind, n)
    rays = _rays(cur, cam, 11 + n)
    want = S.trace(cur, cur.objects, rays, triangles=tris, meshlet_cull=True)
    any_ = np.zeros(len(rays), dtype=R.RAY_HIT)
    any_["status"] = want["status"] & 1
    for a in (rays, want, any_):
        a.setflags(write=False)
    return cur, rays, want, any_


def _renderer(w=0, h=0):
    from chord_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(0)
    r.upload_scene(_base()[0])
    if w:
        r.allocate_gbuffer(w, h)
    return r


def _hits(r, rays, any_hit=False):
    out = r.trace_rays(np.asarray(rays), any_hit=any_hit)
    r.sync()
    return out.cpu().numpy().view(R.RAY_HIT).reshape(-1)


def _same(got, want, what):
    if got.tobytes() == want.tobytes():
        return
    g, w = got.view(np.uint32).reshape(-1, 8), want.view(np.uint32).reshape(-1, 8)
    bad = np.flatnonzero((g != w).any(axis=1))
    k = int(bad[0])
    raise AssertionError("%s: %d of %d rays differ from the specification; first: ray %d\n got  %r\n want %r" % (what, len(bad), len(got), k, got[k], want[k]))


def _refused(call, match):
    with pytest.raises(L.ChordvisError, match=match):
        call()


def _tree_is_the_specification(r, objects, primitives, what):
    want, want_ref, s = T.tree_of_objects(objects, primitives)
    nodes, leaf_ref = r.read_ray_tlas(len(objects))
    info = r.ray_scene_info()
    assert (info.tlasNodes, info.tlasDepth) == (s.nodes, s.depth), what
    assert np.array_equal(leaf_ref, want_ref), (what, "leafRef", np.flatnonzero(leaf_ref != want_ref)[:8])
    for f in ("child", "parentRef", "childCount", "pad"):
        assert np.array_equal(nodes[f], want[f]), (what, f, np.flatnonzero((nodes[f] != want[f]).reshape(len(nodes), -1).any(axis=1))[:8])
    assert nodes.tobytes() == want.tobytes(), (what, "boxes")
    lo, hi = T.root_box(want)
    assert np.array(info.rootMin, dtype=F).tobytes() == lo.tobytes() and np.array(info.rootMax, dtype=F).tobytes() == hi.tobytes(), what
    return s


# ---- 1. tree words ----------------------------------------------------------------------------------------------------------------

TREE_LISTS = [("grid", n) for n in (1, 2, 4, 5, 16, 17, 64, 65, 257, G, G + 1, 16385)] + [("equal", 37), ("plane", 41)]


@pytest.mark.parametrize("kind,n", TREE_LISTS, ids=["%s-%d" % kn for kn in TREE_LISTS])
def test_tree_words_equal_the_specification(gpu, kind, n):
    cur = _list(kind, n)
    r = _renderer()
    try:
        r.build_ray_scene()
        r.set_object_list(cur)
        r.rebuild_ray_tlas()
        s = _tree_is_the_specification(r, cur.objects, cur.primitives, "%s, %d objects" % (kind, n))
        if n == 16385:                 # depth 8, and the last workgroup of every pass is a partial one
            assert s.depth == 8 and n % 2048 == 1 and n % 256 == 1
        if kind == "equal":
            assert T.order(*S.object_boxes(cur.objects, cur.primitives)).tolist() == list(range(n))
        if kind == "plane":
            lo, hi = S.object_boxes(cur.objects, cur.primitives)
            c = T.centres(lo, hi)
            assert len(np.unique(c[:, 2])) == 1 and len(np.unique(T.keys(lo, hi))) > n // 2
    finally:
        r.close()


# ---- 2. hits ----------------------------------------------------------------------------------------------------------------------

HIT_LISTS = [("grid", 1), ("grid", 5), ("grid", 17), ("grid", 600), ("grid", G + 1), ("equal", 37)]


@pytest.mark.parametrize("kind,n", HIT_LISTS, ids=["%s-%d" % kn for kn in HIT_LISTS])
def test_hits_equal_the_specification(gpu, kind, n):
    cur, rays, want, want_any = _hit_case(kind, n)
    assert (want["status"] != 0).sum() >= 10 and (want["status"] == 0).sum() >= 10, "the ray set must hit and miss"
    if kind == "equal":                # n objects in one place: every hit names the lowest index
        assert (want["object"][want["status"] != 0] == 0).all()
    r = _renderer()
    try:
        r.build_ray_scene()
        r.set_object_list(cur)
        _refused(lambda: r.trace_rays(rays), "no ray scene.*chordvis_build_ray_scene")
        r.rebuild_ray_tlas()
        _same(_hits(r, rays), want, "%s %d, closest" % (kind, n))
        _same(_hits(r, rays, any_hit=True), want_any, "%s %d, any-hit" % (kind, n))
    finally:
        r.close()


# ---- 3. rebuild after moves -------------------------------------------------------------------------------------------------------

def test_rebuild_follows_moved_objects(gpu):
    import torch
    scene, cam, tris = _base()
    cur, rays, want0, _ = _hit_case("grid", 600)
    dev = torch.device("cuda", 0)
    r = _renderer()
    try:
        r.set_object_list(cur)
        r.build_ray_scene()                                                # the host's topology for the list as it stands
        host_nodes = r.read_ray_tlas()[0]
        # (a) chordvis_update_objects: every object somewhere else
        moved = TC.permuted(cur, cam)
        assert not (moved.local_to_world == cur.local_to_world).all(axis=1).any()
        r.update_objects(moved.objects)
        _refused(lambda: r.trace_rays(rays), "objects changed")
        r.rebuild_ray_tlas()
        _tree_is_the_specification(r, moved.objects, moved.primitives, "after update_objects")
        assert r.read_ray_tlas()[0]["child"].tobytes() != host_nodes["child"].tobytes()
        want = S.trace(moved, moved.objects, rays, triangles=tris, meshlet_cull=True)
        assert want.tobytes() != want0.tobytes()
        _same(_hits(r, rays), want, "after update_objects + rebuild")
        # (b) records built on the device
        r.upload_world_transforms(cur.local_to_world[::-1].copy())
        r.build_objects(cam.position, cam.position)
        _refused(lambda: r.trace_rays(rays), "objects changed")
        r.rebuild_ray_tlas()
        built = cur.with_objects(r.read_objects())
        _tree_is_the_specification(r, built.objects, built.primitives, "after build_objects")
        _same(_hits(r, rays), S.trace(built, built.objects, rays, triangles=tris, meshlet_cull=True), "after build_objects + rebuild")
        # (c) a caller's array
        mine = torch.from_numpy(cur.objects.view(np.uint8).copy()).to(dev)
        r.bind_objects(mine.data_ptr(), len(cur.objects))
        _refused(lambda: r.trace_rays(rays), "objects changed")
        r.rebuild_ray_tlas()
        _tree_is_the_specification(r, cur.objects, cur.primitives, "after bind_objects")
        _same(_hits(r, rays), want0, "after bind_objects + rebuild")
        # a further change: refused until a refit OR a rebuild
        r.update_objects(moved.objects)
        _refused(lambda: r.trace_rays(rays), "objects changed.*chordvis_refit_ray_scene")
        r.refit_ray_scene()
        _same(_hits(r, rays), want, "update_objects + refit on the rebuilt tree")
        r.update_objects(cur.objects)
        _refused(lambda: r.trace_rays(rays), "objects changed")
        r.rebuild_ray_tlas()
        _same(_hits(r, rays), want0, "update_objects + rebuild")
        r.sync()
    finally:
        r.close()


# ---- 4. build and rebuild agree ---------------------------------------------------------------------------------------------------

def test_build_and_rebuild_answer_alike(gpu):
    cur, rays, want, want_any = _hit_case("grid", 600)
    r = _renderer()
    try:
        r.set_object_list(cur)
        built = r.build_ray_scene()
        a, a_any = _hits(r, rays), _hits(r, rays, any_hit=True)
        host_nodes, host_ref = r.read_ray_tlas()                          # the read-back serves a host-built tree too
        assert len(host_nodes) == built.tlasNodes and len(np.unique(host_ref)) == len(cur.objects)
        r.rebuild_ray_tlas()
        b, b_any = _hits(r, rays), _hits(r, rays, any_hit=True)
        assert a.tobytes() == b.tobytes() == want.tobytes() and a_any.tobytes() == b_any.tobytes() == want_any.tobytes()
        again = r.build_ray_scene()                                        # ... and back: the host builder's tree as before
        assert (again.tlasNodes, again.tlasDepth, again.blasBuilt) == (built.tlasNodes, built.tlasDepth, 0)
        assert r.read_ray_tlas()[0].tobytes() == host_nodes.tobytes()
        assert _hits(r, rays).tobytes() == want.tobytes()
    finally:
        r.close()


# ---- 5. refusals, lifecycle, frames untouched -------------------------------------------------------------------------------------

def test_refusals_and_lifecycle(gpu):
    from chord_amd.renderer import VisibilityRenderer
    scene, cam, tris = _base()
    cur, rays, want, _ = _hit_case("grid", 17)
    assert L.lib.chordvis_rebuild_ray_tlas(None) == L.E_INVALID and L.lib.chordvis_readback_ray_tlas(None, None, 0, None, 0) == L.E_INVALID
    r = VisibilityRenderer(0)
    try:
        _refused(r.rebuild_ray_tlas, "rebuild_ray_tlas: no scene.*chordvis_upload_scene")
        r.upload_scene(scene)
        _refused(r.rebuild_ray_tlas, "rebuild_ray_tlas: no BLASes.*chordvis_build_ray_scene")
        _refused(lambda: r._check(L.lib.chordvis_readback_ray_tlas(r._ctx, None, 0, None, 0), "readback_ray_tlas"), "no ray scene")
        r.build_ray_scene()
        r.rebuild_ray_tlas()                                               # a TLAS exists: re-shaped
        _tree_is_the_specification(r, scene.objects, scene.primitives, "the uploaded list")
        r.set_object_list(cur)
        for call in (lambda: r.trace_rays(rays), r.refit_ray_scene, r.ray_scene_info):
            _refused(call, "no ray scene.*chordvis_build_ray_scene")
        _refused(lambda: r.read_ray_tlas(len(cur.objects)), "no ray scene")
        r.rebuild_ray_tlas()                                               # a TLAS was dropped: made
        _same(_hits(r, rays), want, "after set_object_list + rebuild")
        nodes = np.zeros(1, dtype=R.RAY_NODE)
        _refused(lambda: r._check(L.lib.chordvis_readback_ray_tlas(r._ctx, nodes.ctypes.data, 1, None, 0), "readback_ray_tlas"), "nodeCapacity")
        ref = np.zeros(16, dtype=np.uint32)
        _refused(lambda: r._check(L.lib.chordvis_readback_ray_tlas(r._ctx, None, 0, ref.ctypes.data, 16), "readback_ray_tlas"), "objectCapacity")
        assert L.lib.chordvis_readback_ray_tlas(r._ctx, None, 0, None, 0) == L.OK
        _same(_hits(r, rays), want, "after refused read-backs")
        # an upload drops everything: a rebuild is refused until a build
        r.upload_scene(scene)
        _refused(r.rebuild_ray_tlas, "no BLASes")
        _refused(lambda: r.trace_rays(rays), "no ray scene")
        assert r.build_ray_scene().blasBuilt == 1
        r.set_object_list(cur)
        r.rebuild_ray_tlas()
        _same(_hits(r, rays), want, "after upload, build, set_object_list, rebuild")
    finally:
        r.close()


def test_frames_are_untouched(gpu):
    """Frames before and after a rebuild are bit for bit those of a context without a ray scene: image, list, HZB and launches."""
    scene, cam = scenes.small_test_scene(64, 40, lods=3)
    L.fill_objects(scene, cam)
    fw, fh = 160, 96
    fview, fiv = L.make_views(scenes.Camera(cam.position, cam.front, fw, fh))
    tris = S.lod0_triangles(scene)
    rays = S.pixel_rays(L.make_views(cam)[0], 32, 20)
    want = S.trace(scene, scene.objects, rays, triangles=tris, meshlet_cull=True)
    assert (want["status"] != 0).sum() >= 10

    def frames(with_rays):
        from chord_amd.renderer import VisibilityRenderer
        r = VisibilityRenderer(0)
        out = []
        try:
            r.upload_scene(scene)
            r.allocate_gbuffer(fw, fh)
            r.set_view(fview, fiv, H.ALL_FLAGS)
            for k in range(3):
                if with_rays and k == 1:
                    r.build_ray_scene()
                if with_rays and k >= 1:
                    r.rebuild_ray_tlas()
                    _same(_hits(r, rays), want, "between frames")
                r.render_frame()
                r.sync()
                out.append((r.read_visibility().tobytes(), r.read_cmds(r.last_frame_cmds()).tobytes(),
                            [None if a is None else a.tobytes() for a in r.read_hzb(r.history_hzb())], r.stats()))
        finally:
            r.close()
        return out
    a, b = frames(False), frames(True)
    for k in range(3):
        assert a[k][0] == b[k][0], "frame %d: image" % k
        assert a[k][1] == b[k][1], "frame %d: list" % k
        assert a[k][2] == b[k][2], "frame %d: HZB" % k
        for key in ("countInstanceCulled", "countStage0Visible", "countStage0Rejected", "countStage1Visible", "kernelLaunches"):
            assert a[k][3][key] == b[k][3][key], (k, key)
    assert any(np.frombuffer(f[0], dtype=np.uint64).any() for f in a)


# ---- 6. stream order --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (600, G + 1))
def test_rebuild_does_not_wait(gpu, n):
    """set_object_list (same count), rebuild, trace, update_objects, rebuild, trace behind a closed gate on a caller-owned stream
    (tests/inflight.py): every call returns while the device is held, and both traces are the specification's once it opens."""
    import torch
    scene, cam, tris = _base()
    first = _list("grid", n)
    second = TC.instances(scene, cam, n, 900 + n)
    third = TC.permuted(second, cam)
    rays = _rays(second, cam, 5)[:256]
    want = [S.trace(x, x.objects, rays, triangles=tris, meshlet_cull=True) for x in (second, third)]
    assert all((w["status"] != 0).sum() >= 10 for w in want) and want[0].tobytes() != want[1].tobytes()
    sc = IF.Scenario("ray_tlas", first, 160, 96, H.ALL_FLAGS, [])

    def prepare():
        ctx = IF.Context(sc)
        ctx.r.build_ray_scene()
        ctx.r.rebuild_ray_tlas()                                           # (the rebuild's buffers exist from here on)
        with torch.cuda.stream(ctx.stream):
            ctx.rays = torch.from_numpy(np.asarray(rays).view(np.uint8).copy()).to(torch.device("cuda", 0))
            ctx.hits = [torch.zeros((len(rays), 8), dtype=torch.int32, device=ctx.rays.device) for _ in range(2)]
        ctx.synchronize()
        return ctx

    def script(ctx):
        def trace(out):
            with torch.cuda.stream(ctx.stream):
                ctx.r.trace_rays(ctx.rays, out=out)
        return [("set_object_list[0]", lambda: ctx.r.set_object_list(second), False),
                ("rebuild_ray_tlas[0]", ctx.r.rebuild_ray_tlas, False),
                ("trace_rays[0]", lambda: trace(ctx.hits[0]), False),
                ("update_objects[0]", lambda: ctx.r.update_objects(third.objects), False),
                ("rebuild_ray_tlas[1]", ctx.r.rebuild_ray_tlas, False),
                ("trace_rays[1]", lambda: trace(ctx.hits[1]), False)]

    ctx, log, _ = IF.run_behind_gate(prepare, script, "set_object_list, rebuild, trace in flight")
    try:
        assert IF.waits(log) == {"set_object_list": False, "rebuild_ray_tlas": False, "trace_rays": False, "update_objects": False}
        for k in range(2):
            _same(ctx.hits[k].cpu().numpy().view(R.RAY_HIT).reshape(-1), want[k], "in flight, trace %d" % k)
        _tree_is_the_specification(ctx.r, third.objects, third.primitives, "in flight")
    finally:
        ctx.close()
