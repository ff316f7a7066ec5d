"""chordvis_build_ray_scene / chordvis_refit_ray_scene / chordvis_trace_rays on the GPU, held to what include/chordvis.h promises (RAY
QUERIES): every word of every hit equals the brute-force specification (tests/spec_rays_np.py) -- no tolerance, no ray left out --
in closest-hit and any-hit mode; the TLAS follows object lists and moved objects; the refusals and their messages; frames are
untouched; the calls do not wait for the device; and the ids a hit names are the ids the raster writes.

The specification is evaluated once per (scene, ray set) with its meshlet_cull path (tests/test_rays_spec.py holds that path to the
plain one).  One rule of the header is not reachable from here: a depth-view child context has no handle in the ABI."""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers as H
import inflight as IF
import meshlet_shapes as MS
import spec_rays_np as S
from ray_deep_cases import meshlet_primitive as _meshlet_primitive
from chord_amd import lib as L, records as R, scenes

pytestmark = pytest.mark.gpu
F = np.float32
PW, PH = 64, 40


# ---- scenes ---------------------------------------------------------------------------------------------------------------------

def _quads(quads):
    """positions and triangles of axis-aligned quads given by four corners each, corners shared exactly between neighbours."""
    verts, index, tris = [], {}, []
    for q in quads:
        ids = []
        for c in q:
            key = tuple(float(x) for x in c)
            if key not in index:
                index[key] = len(verts)
                verts.append(key)
            ids.append(index[key])
        tris += [(ids[0], ids[1], ids[2]), (ids[0], ids[2], ids[3])]
    return np.array(verts, dtype=np.float32), np.array(tris, dtype=np.int64)


def quad_scene():
    """Axis-aligned unit quads: a 3 x 3 floor of quads sharing edges and vertices (y = 0), a wall (x = 3) on the floor's edge and a
    unit cube, as two primitives; the floor twice under one matrix (a tie between objects), the cube moved and mirrored."""
    floor = [[(x, 0, z), (x + 1, 0, z), (x + 1, 0, z + 1), (x, 0, z + 1)] for z in range(3) for x in range(3)]
    wall = [[(3, y, z), (3, y, z + 1), (3, y + 1, z + 1), (3, y + 1, z)] for y in range(2) for z in range(3)]
    cube = [[(0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0)], [(0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)],
            [(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)], [(0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 1, 0)],
            [(0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0)], [(1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1)]]
    sb = scenes.SceneBuilder("ray_quads")
    p, t = _quads(floor + wall)
    sb.prims.append(_meshlet_primitive(p, [t[:18], t[18:]], (2,)))
    p, t = _quads(cube)
    sb.prims.append(_meshlet_primitive(p, [t], (1,)))
    sb.add_object(0)
    sb.add_object(1, scenes.translate(1.0, 0.0, 1.0))
    sb.add_object(0)                                                       # the same primitive under the same matrix: ties go to object 0
    sb.add_object(1, scenes.translate(0.5, 1.0, 2.5) @ scenes.scale(-1.0, 0.5, 1.0))
    return sb.build(), scenes.Camera((-2.5, 2.2, 5.5), (0.75, -0.35, -0.6), PW, PH)


def tie_scene():
    """A meshlet with a duplicated triangle, and 1 024 coincident triangles (8 meshlets of 128, two groups)."""
    sb = scenes.SceneBuilder("ray_ties")
    pos = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)], dtype=np.float32)
    sb.prims.append(_meshlet_primitive(pos, [[(0, 1, 2), (0, 2, 3), (0, 1, 2)]], (1,)))
    pos = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], dtype=np.float32)
    sb.prims.append(_meshlet_primitive(pos, [[(0, 1, 2)] * 128] * 8, (4, 4)))
    sb.add_object(0)
    sb.add_object(1, scenes.translate(2.0, 0.0, 0.0))
    return sb.build(), scenes.Camera((1.5, 0.5, 4.0), (0.0, 0.0, -1.0), PW, PH)


def _small():
    return scenes.small_test_scene(PW, PH, lods=3)


def _general():
    scene, cam, _ = scenes.general_transform_scene(PW, PH)
    return scene, cam


def _shapes():
    scene, cam = MS.scene("plain")
    return scene, scenes.Camera(cam.position, cam.front, PW, PH)


SCENES = {"small": _small, "general": _general, "shapes": _shapes, "quads": quad_scene}


# ---- rays -----------------------------------------------------------------------------------------------------------------------

def _random_rays(scene, n, seed):
    lo, hi = S.object_boxes(scene.objects, scene.primitives)
    lo, hi = lo.min(axis=0).astype(np.float64), hi.max(axis=0).astype(np.float64)
    r = scenes.rand01(seed, np.arange(7 * n)).reshape(n, 7)
    d = r[:, 3:6] * 2.0 - 1.0
    rays = S.make_rays(lo + r[:, :3] * (hi - lo), d, 1e-2, 1e9)
    rays["tMax"][::5] = (r[::5, 6] * np.linalg.norm(hi - lo)).astype(F)    # some short rays
    return rays


def _adversarial(base_rays, base_hits):
    """The generic adversarial set, made from rays that hit: origin on the surface, tMin == tMax on the hit, tMin > tMax, NaN and inf
    words, and directions with one, two and three zero components and a subnormal one."""
    hit = np.flatnonzero(base_hits["status"] & 1)[:24]
    out = []
    src = base_rays[hit].copy()
    point = src["origin"].astype(np.float64) + src["direction"].astype(np.float64) * base_hits["t"][hit][:, None].astype(np.float64)
    a = src.copy(); a["origin"] = point.astype(F); a["tMin"] = 0.0; out.append(a)                      # origin on a surface
    a = src.copy(); a["tMin"] = a["tMax"] = base_hits["t"][hit]; out.append(a)                         # tMin == tMax on a hit
    a = src.copy(); a["tMin"], a["tMax"] = 2.0, 1.0; out.append(a)                                     # tMin > tMax
    for word, value in ((0, np.nan), (2, np.inf), (3, np.nan), (4, np.nan), (5, -np.inf), (7, np.inf), (7, np.nan), (3, -np.inf)):
        a = src[:3].copy()
        a.view(F).reshape(-1, 8)[:, word] = value
        out.append(a)
    for zero in ((0,), (1,), (2,), (0, 1), (1, 2), (0, 2), (0, 1, 2)):
        a = src.copy()
        for k in zero:
            a["direction"][:, k] = 0.0 if len(zero) != 2 else -0.0
        out.append(a)
        a = a.copy(); a["origin"] = point.astype(F); a["tMin"] = -1.0; out.append(a)                   # ... from the surface itself
    a = src.copy(); a["direction"][:, 1] = 1e-42; out.append(a)                                        # a subnormal component
    a = src.copy(); a["direction"][:, 0] = -1e-45; a["direction"][:, 2] = 0.0; out.append(a)
    return np.concatenate(out)


def _quad_rays():
    """Rays of the quad scene: in the floor's plane, through shared edges and shared vertices (from above and along the axes), along
    the wall, and from points on the surfaces."""
    o, d = [], []
    for x in (0.0, 0.5, 1.0, 2.0, 3.0):
        for z in (0.0, 0.25, 1.0, 2.0, 3.0):
            o.append((x, 2.0, z)); d.append((0.0, -1.0, 0.0))          # straight down: interiors, edges (x or z whole), vertices (both)
            o.append((x, 0.0, z)); d.append((0.0, -1.0, 0.0))          # ... from the surface
            o.append((x, 2.0, z)); d.append((0.0, -2.0, 0.0))
    for z in (0.0, 0.5, 1.0, 1.5, 3.0):
        o.append((-1.0, 0.0, z)); d.append((1.0, 0.0, 0.0))            # in the floor's plane, along quad edges and through interiors
        o.append((-1.0, 0.0, z)); d.append((1.0, 0.0, 0.25))
        o.append((4.0, 0.5, z)); d.append((-1.0, 0.0, 0.0))            # at the wall, through its edges and vertices
        o.append((3.0, 3.0, z)); d.append((0.0, -1.0, 0.0))            # in the wall's plane
    for k in range(12):
        o.append((1.0 + 0.1 * k, 3.0, 1.0 + 0.1 * k)); d.append((0.0, -1.0, 0.0))      # the cube's top along its diagonal (a shared edge)
        o.append((-1.0, 0.1 * k, 1.5)); d.append((1.0, 0.0, 0.0))                      # the cube's side, its bottom edge on the floor
    return S.make_rays(np.array(o, dtype=F), np.array(d, dtype=F), 0.0, 1e9)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(scene with records filled, camera, view, iv, lod0 triangles, rays, expected closest hits, expected any-hit) -- computed once."""
    scene, cam = SCENES[name]()
    L.fill_objects(scene, cam)
    view, iv = L.make_views(cam)
    tris = S.lod0_triangles(scene)
    pix = S.pixel_rays(view, PW, PH)
    pix_hits = S.trace(scene, scene.objects, pix, triangles=tris, meshlet_cull=True)
    sets = [pix, _random_rays(scene, 300, 17), _adversarial(pix, pix_hits)]
    if name == "quads":
        sets.append(_quad_rays())
    rays = np.concatenate(sets)
    rest = S.trace(scene, scene.objects, rays[len(pix):], triangles=tris, meshlet_cull=True)
    want = np.concatenate([pix_hits, rest])
    want_any = np.zeros(len(rays), dtype=R.RAY_HIT)
    want_any["status"] = want["status"] & 1
    for a in (rays, want, want_any):
        a.setflags(write=False)
    return scene, cam, view, iv, tris, rays, want, want_any


def _renderer(scene, w=0, h=0):
    from chord_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(0)
    r.upload_scene(scene)
    if w:
        r.allocate_gbuffer(w, h)
    return r


def _hits(r, rays, any_hit=False):
    out = r.trace_rays(np.asarray(rays), any_hit=any_hit)
    r.sync()
    return out.cpu().numpy().view(R.RAY_HIT).reshape(-1)


def _same(got, want, rays, what):
    if got.tobytes() == want.tobytes():
        return
    g, w = got.view(np.uint32).reshape(-1, 8), want.view(np.uint32).reshape(-1, 8)
    bad = np.flatnonzero((g != w).any(axis=1))
    k = int(bad[0])
    raise AssertionError("%s: %d of %d rays differ from the specification; first: ray %d %r\n got  %r\n want %r"
                         % (what, len(bad), len(got), k, rays[k], got[k], want[k]))


def _refused(call, match):
    with pytest.raises(L.ChordvisError, match=match):
        call()


# ---- 1. every hit word, every scene, both modes ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(SCENES))
def test_hits_equal_the_specification(gpu, name):
    scene, cam, view, iv, tris, rays, want, want_any = _case(name)
    assert (want["status"] & 1).sum() > len(rays) // 8 and (want["status"] == 0).sum() > 30, "the ray set must hit and miss"
    if name == "small":          # a hit names LOD-0 meshlets only
        assert (scene.meshlets["lod"] > 0).any() and (scene.meshlets["lod"][want["meshlet"][want["status"] != 0]] == 0).all()
    if name == "shapes":         # the 255-vertex meshlets are hit; the T = 0 meshlet is there
        vt = scene.meshlets["vertexTriangleCount"]
        assert ((vt[want["meshlet"][want["status"] != 0]] & 0xFF) == 255).any() and ((vt >> 8) == 0).any()
    if name == "general":        # mirrored objects: both faces are met
        assert (want["status"] == 3).any() and (want["status"] == 1).any()
    r = _renderer(scene)
    try:
        info = r.build_ray_scene()
        assert info.blasBuilt == info.blasCount == len(scene.primitives) and info.blasTriangles == sum(len(t[0]) for t in tris)
        assert 1 <= info.blasMaxDepth <= L.RAY_MAX_DEPTH and 1 <= info.tlasDepth <= L.RAY_MAX_DEPTH
        _same(_hits(r, rays), want, rays, name + ", closest")
        _same(_hits(r, rays, any_hit=True), want_any, rays, name + ", any-hit")
    finally:
        r.close()


def test_ray_counts(gpu):
    """0, 1, 63, 64, 65 and 4 097 rays: the wave's edges, and a last workgroup of one lane; a count of 0 launches nothing."""
    scene, cam, view, iv, tris, rays, want, want_any = _case("quads")
    r = _renderer(scene)
    try:
        r.build_ray_scene()
        assert len(_hits(r, rays[:0])) == 0
        assert L.lib.chordvis_trace_rays(r._ctx, None, 0, 0, None) == L.OK
        for n in (1, 63, 64, 65, 4097):
            idx = np.arange(n) % len(rays)
            _same(_hits(r, rays[idx]), want[idx], rays[idx], "%d rays" % n)
            _same(_hits(r, rays[idx], any_hit=True), want_any[idx], rays[idx], "%d rays, any-hit" % n)
    finally:
        r.close()


# ---- 2. ties ----------------------------------------------------------------------------------------------------------------------

def test_ties_go_to_the_lowest_ids(gpu):
    scene, cam, view, iv, tris, rays, want, _ = _case("quads")
    # two objects with one primitive and one matrix: every hit on them names the lower index
    on_floor = (want["status"] != 0) & (want["primitive"] == 0)
    assert on_floor.sum() > 100 and (want["object"][on_floor] == 0).all()
    scene, cam = tie_scene()
    L.fill_objects(scene, cam)
    tris = S.lod0_triangles(scene)
    o = [(0.7, 0.3, 3.0), (0.6, 0.2, -2.0), (2.2, 0.3, 3.0), (2.5, 0.25, 1.0), (2.1, 0.1, -1.0), (2.3, 0.6, 2.0)]
    d = [(0, 0, -1), (0, 0, 1), (0, 0, -1), (0, 0, -1), (0, 0, 1), (0.01, 0.0, -1.0)]
    rays = S.make_rays(np.array(o, dtype=F) - np.array(cam.position, dtype=F), np.array(d, dtype=F), 0.0, 1e9)
    want = S.trace(scene, scene.objects, rays, triangles=tris)
    assert (want["status"] != 0).all()
    assert (want["triangle"][:2] == 0).all()                                   # the duplicated triangle: index 0, not 2
    first = int(scene.primitives[1]["meshletOffset"])
    assert (want["meshlet"][2:] == first).all() and (want["triangle"][2:] == 0).all()      # 1 024 coincident: the lowest ids
    r = _renderer(scene)
    try:
        info = r.build_ray_scene()
        assert info.blasTriangles == 3 + 1024
        _same(_hits(r, rays), want, rays, "ties")
    finally:
        r.close()


# ---- 3. TLAS shapes and object lists ---------------------------------------------------------------------------------------------

def _instances(scene, cam, n, seed):
    """n instances of the scene's first primitive on a jittered grid, records filled."""
    side = int(np.ceil(np.sqrt(n)))
    rnd = scenes.rand01(seed, np.arange(3 * n)).reshape(n, 3)
    objs = np.zeros(n, dtype=R.OBJECT)
    out = scene.with_objects(objs)
    out.local_to_world = np.ascontiguousarray(np.stack([
        (scenes.translate(2.5 * (k % side) - 1.25 * side + rnd[k, 0], 2.5 * (k // side) - 1.25 * side + rnd[k, 1], -3.0 * rnd[k, 2]) @
         scenes.rotate_y(rnd[k, 0] * 2.0)).T.reshape(16) for k in range(n)]), dtype=np.float64)
    L.fill_objects(out, cam)
    return out


def test_tlas_follows_the_object_list(gpu):
    scene, cam = scenes.config1_single_meshlet()
    L.fill_objects(scene, cam)
    tris = S.lod0_triangles(scene)
    r = _renderer(scene)
    try:
        assert r.build_ray_scene().blasBuilt == 1
        for n in (1, 2, 9, 600):
            cur = _instances(scene, cam, n, 100 + n)
            r.set_object_list(cur)
            rays = np.concatenate([_random_rays(cur, 200, n), S.pixel_rays(L.make_views(cam)[0], 16, 16)])
            _refused(lambda: r.trace_rays(rays), "no ray scene.*chordvis_build_ray_scene")
            _refused(r.refit_ray_scene, "no ray scene")
            _refused(r.ray_scene_info, "no ray scene")
            info = r.build_ray_scene()
            assert info.blasBuilt == 0 and info.blasCount == 1 and info.blasTriangles == 128
            assert info.tlasNodes >= 1 and 1 <= info.tlasDepth <= L.RAY_MAX_DEPTH and (n > 4 or (info.tlasNodes, info.tlasDepth) == (1, 1))
            lo, hi = S.object_boxes(cur.objects, cur.primitives)
            assert np.array_equal(np.array(info.rootMin, dtype=F), lo.min(axis=0)) and np.array_equal(np.array(info.rootMax, dtype=F), hi.max(axis=0))
            again = r.ray_scene_info()
            assert list(again.rootMin) == list(info.rootMin) and list(again.rootMax) == list(info.rootMax) and again.blasBuilt == 0
            want = S.trace(cur, cur.objects, rays, triangles=tris, meshlet_cull=True)
            assert (want["status"] != 0).sum() >= 10
            _same(_hits(r, rays), want, rays, "%d instances" % n)
    finally:
        r.close()


# ---- 4. refit ---------------------------------------------------------------------------------------------------------------------

def _moved(scene, every=3, by=(0.9, 0.4, -1.3)):
    l2w = scene.local_to_world.copy()
    l2w[::every, 12:15] += np.array(by)
    return l2w


def test_refit_follows_moved_objects(gpu):
    import torch
    scene0, cam, view, iv, tris, rays, want0, _ = _case("small")
    scene = scene0.with_objects(scene0.objects.copy())
    rays = rays[: PW * PH + 300]
    r = _renderer(scene)
    try:
        r.build_ray_scene()
        # (a) chordvis_update_objects
        moved = scene.with_objects(scene.objects.copy())
        moved.local_to_world = _moved(scene)
        L.fill_objects(moved, cam)
        r.update_objects(moved.objects)
        _refused(lambda: r.trace_rays(rays), "objects changed.*chordvis_refit_ray_scene")
        r.refit_ray_scene()
        want = S.trace(moved, moved.objects, rays, triangles=tris, meshlet_cull=True)
        assert want.tobytes() != want0[: len(rays)].tobytes()
        _same(_hits(r, rays), want, rays, "after update_objects + refit")
        lo, hi = S.object_boxes(moved.objects, moved.primitives)
        info = r.ray_scene_info()
        assert np.array_equal(np.array(info.rootMin, dtype=F), lo.min(axis=0)) and np.array_equal(np.array(info.rootMax, dtype=F), hi.max(axis=0))
        # (b) scatter + build on the device, under a moved camera: the rays' space moves with the records
        cam2 = cam.moved((0.4, 0.1, -0.3))
        r.upload_world_transforms(scene.local_to_world)
        idx = np.arange(0, len(scene.objects), 3, dtype=np.int32)
        dev = torch.device("cuda", 0)
        r.scatter_world_transforms(torch.from_numpy(idx).to(dev), torch.from_numpy(np.ascontiguousarray(_moved(scene, by=(-0.5, 0.2, 0.8))[idx])).to(dev))
        r.build_objects(cam2.position, cam.position)
        _refused(lambda: r.trace_rays(rays), "objects changed")
        r.refit_ray_scene()
        built = scene.with_objects(r.read_objects())
        rays2 = S.pixel_rays(L.make_views(cam2)[0], PW, PH)
        want = S.trace(built, built.objects, rays2, triangles=tris, meshlet_cull=True)
        _same(_hits(r, rays2), want, rays2, "after build_objects + refit")
        # (c) a caller's array
        mine = torch.from_numpy(moved.objects.view(np.uint8).copy()).to(dev)
        r.bind_objects(mine.data_ptr(), len(moved.objects))
        _refused(lambda: r.trace_rays(rays), "objects changed")
        r.refit_ray_scene()
        want = S.trace(moved, moved.objects, rays, triangles=tris, meshlet_cull=True)
        _same(_hits(r, rays), want, rays, "after bind_objects + refit")
        r.sync()
    finally:
        r.close()


# ---- 5. lifecycle, refusals, frames untouched ------------------------------------------------------------------------------------

def test_refusals_and_lifecycle(gpu):
    import torch
    from chord_amd.renderer import VisibilityRenderer
    scene, cam, view, iv, tris, rays, want, _ = _case("quads")
    dev = torch.device("cuda", 0)
    drays = torch.from_numpy(np.asarray(rays).view(np.uint8).copy()).to(dev)
    dhits = torch.zeros((len(rays), 8), dtype=torch.int32, device=dev)
    r = VisibilityRenderer(0)
    try:
        trace = lambda flags=0, rp=drays.data_ptr(), hp=dhits.data_ptr(), n=len(rays): r._check(L.lib.chordvis_trace_rays(r._ctx, rp, n, flags, hp), "trace_rays")
        for call in (r.build_ray_scene, r.refit_ray_scene, r.ray_scene_info, trace):
            _refused(call, "no scene")
        r.upload_scene(scene)
        for call in (r.refit_ray_scene, r.ray_scene_info, trace):
            _refused(call, "no ray scene")
        r.build_ray_scene()
        trace()                                                    # valid without a view or a G-buffer
        _refused(lambda: trace(flags=2), "unknown flag bits")
        _refused(lambda: trace(flags=1 | 4), "unknown flag bits")
        _refused(lambda: trace(rp=None), "16-byte aligned")
        _refused(lambda: trace(hp=None), "16-byte aligned")
        _refused(lambda: trace(rp=drays.data_ptr() + 4), "16-byte aligned")
        _refused(lambda: trace(hp=dhits.data_ptr() + 8), "16-byte aligned")
        assert L.lib.chordvis_trace_rays(r._ctx, None, 0, 0, None) == L.OK
        assert L.lib.chordvis_ray_scene_info(r._ctx, None) == L.E_INVALID
        r.sync()
        _same(dhits.cpu().numpy().view(R.RAY_HIT).reshape(-1), want, rays, "raw call")
        # an upload drops everything, a refused one too
        r.upload_scene(scene)
        _refused(trace, "no ray scene")
        assert r.build_ray_scene().blasBuilt == len(scene.primitives)
        empty = R.SceneDesc()
        assert L.lib.chordvis_upload_scene(r._ctx, C.byref(empty)) != L.OK
        _refused(trace, "no scene")
        r.upload_scene(scene)
        _refused(trace, "no ray scene")
        # a non-finite LOD-0 position: the build refuses, and leaves no ray scene
        pos = scene.positions.copy()
        pos[3, 1] = np.nan
        bad = R.Scene(scene.objects, scene.primitives, scene.materials, scene.meshlets, scene.groups, scene.group_indices, scene.meshlet_data, pos,
                      bvh_nodes=scene.bvh_nodes)
        r.upload_scene(bad)
        _refused(r.build_ray_scene, "non-finite position")
        _refused(trace, "no ray scene")
    finally:
        r.close()


def test_frames_are_untouched(gpu):
    """A frame before and after a build, a refit and a trace is bit for bit the frame of a context that never built a ray scene: image,
    lists and HZB."""
    scene, cam, view, iv, tris, rays, want, _ = _case("small")
    fw, fh = 160, 96                                                       # (the frames' own size: a target is at least 64 pixels a side)
    fview, fiv = L.make_views(scenes.Camera(cam.position, cam.front, fw, fh))

    def frames(with_rays):
        r = _renderer(scene, fw, fh)
        out = []
        try:
            r.set_view(fview, fiv, H.ALL_FLAGS)
            for k in range(3):
                if with_rays and k == 1:
                    r.build_ray_scene()
                if with_rays and k >= 1:
                    r.refit_ray_scene()
                    _same(_hits(r, rays[:500]), want[:500], rays[:500], "between frames")
                r.render_frame()
                r.sync()
                cmds = [r.read_cmds(r.last_frame_cmds())]
                out.append((r.read_visibility().tobytes(), [c.tobytes() for c in cmds], [None if a is None else a.tobytes() for a in r.read_hzb(r.history_hzb())],
                            r.stats()))
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


# ---- 6. stream order ---------------------------------------------------------------------------------------------------------------

def test_refit_and_trace_do_not_wait(gpu):
    """update_objects, refit, trace (closest and any-hit) behind a closed gate on a caller-owned stream (tests/inflight.py): every call
    returns while the device is held, and the results are the specification's once it is released."""
    import torch
    scene0, cam, view, iv, tris, rays, want0, _ = _case("small")
    scene = scene0.with_objects(scene0.objects.copy())
    rays = rays[: PW * PH + 300]
    moved = scene.with_objects(scene.objects.copy())
    moved.local_to_world = _moved(scene, every=2, by=(0.3, 0.0, 0.7))
    L.fill_objects(moved, cam)
    want = S.trace(moved, moved.objects, rays, triangles=tris, meshlet_cull=True)
    sc = IF.Scenario("rays", scene, 160, 96, H.ALL_FLAGS, [])

    def prepare():
        ctx = IF.Context(sc)
        ctx.r.build_ray_scene()
        with torch.cuda.stream(ctx.stream):
            ctx.rays = torch.from_numpy(np.asarray(rays).view(np.uint8).copy()).to(torch.device("cuda", 0))
            ctx.hits = torch.zeros((len(rays), 8), dtype=torch.int32, device=ctx.rays.device)
            ctx.any = torch.zeros((len(rays), 8), dtype=torch.int32, device=ctx.rays.device)
        ctx.synchronize()
        return ctx

    def script(ctx):
        def trace(any_hit, out):
            with torch.cuda.stream(ctx.stream):
                ctx.r.trace_rays(ctx.rays, any_hit=any_hit, out=out)
        return [("update_objects[0]", lambda: ctx.r.update_objects(moved.objects), False),
                ("refit_ray_scene[0]", ctx.r.refit_ray_scene, False),
                ("trace_rays[0]", lambda: trace(False, ctx.hits), False),
                ("trace_rays[1]", lambda: trace(True, ctx.any), False)]

    ctx, log, _ = IF.run_behind_gate(prepare, script, "update, refit, trace in flight")
    try:
        assert IF.waits(log) == {"update_objects": False, "refit_ray_scene": False, "trace_rays": False}
        _same(ctx.hits.cpu().numpy().view(R.RAY_HIT).reshape(-1), want, rays, "in flight, closest")
        assert np.array_equal(ctx.any.cpu().numpy().view(R.RAY_HIT).reshape(-1)["status"], want["status"] & 1)
    finally:
        ctx.close()


# ---- 7. agreement with the raster -----------------------------------------------------------------------------------------------

def agreement_scene(width=160, height=100):
    """LOD-0 only, triangles several pixels across, no coplanar overlaps: a bumpy floor of one 128-triangle patch, three patches
    standing on it under general transforms, and a cylinder."""
    sb = scenes.SceneBuilder("ray_agreement")
    two = sb.add_material(1)
    pb = scenes.PrimitiveBuilder()
    pb.add_surface(scenes.plane_surface((-4, 0, 4), (8, 0, 0), (0, 0, -8), 3, 0.15, 0.8), 1, 1, 1)
    sb.add_object(sb.add_primitive(pb))
    pb = scenes.PrimitiveBuilder()
    pb.add_surface(scenes.plane_surface((-1, 0, 0), (2, 0, 0), (0, 2, 0), 5, 0.1, 1.0), 1, 1, 1)
    wall = sb.add_primitive(pb)
    sb.add_object(wall, scenes.translate(-1.5, 0.3, -1.0) @ scenes.rotate_y(0.5), material=two)
    sb.add_object(wall, scenes.translate(1.8, 0.2, -0.5) @ scenes.rotate_y(-0.7) @ scenes.scale(0.8, 1.4, 1.0), material=two)
    sb.add_object(wall, scenes.translate(0.2, 0.4, -2.5) @ scenes.rotate_x(-0.3) @ scenes.scale(-1.5, 1.0, 1.0), material=two)
    pb = scenes.PrimitiveBuilder()
    pb.add_surface(scenes.cylinder_surface((0, 0, 0), 0.5, 1.5, 9, 0.02), 1, 1, 1)
    sb.add_object(sb.add_primitive(pb), scenes.translate(0.3, 0.2, 0.8), material=two)
    return sb.build(), scenes.Camera((-0.5, 2.0, 4.5), (0.1, -0.35, -1.0), width, height)


def raster_agreement(scene, view, vis, cmds, hits, w, h):
    """(covered pixels, interior pixels, interior pixels whose hit names another object / meshlet / triangle than the image).  A pixel
    is interior when its 3 x 3 neighbourhood in the image names one (cluster, triangle)."""
    low = (np.asarray(vis, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64).reshape(h, w)
    covered = low != 0
    pad = np.pad(low, 1, constant_values=-1)
    interior = covered.copy()
    for dy in range(3):
        for dx in range(3):
            interior &= pad[dy:dy + h, dx:dx + w] == low
    slot = np.where(covered, ((low >> 8) & 0xFFFFFF) - 1, 0)
    hits = hits.reshape(h, w)
    same = ((hits["status"] & 1) != 0) & (hits["object"] == cmds["objectId"][slot]) & (hits["meshlet"] == cmds["meshletId"][slot]) & \
           (hits["triangle"] == (low & 0xFF))
    return int(covered.sum()), int(interior.sum()), int((interior & ~same).sum())


def test_hits_name_what_the_raster_names(gpu):
    scene, cam, view, iv = H.setup_scene(agreement_scene)
    w, h = cam.width, cam.height
    assert view["translatedWorldToClip"].tobytes() == L.make_views(cam)[0]["translatedWorldToClip"].tobytes() and tuple(cam.jitter) == (0.0, 0.0)
    rays = S.pixel_rays(view, w, h)
    r = _renderer(scene, w, h)
    try:
        r.set_view(view, iv, H.ALL_FLAGS)
        r.render_frame()
        r.sync()
        vis, cmds = r.read_visibility(), r.read_cmds(r.last_frame_cmds())
        r.build_ray_scene()
        hits = _hits(r, rays)
        covered, interior, wrong = raster_agreement(scene, view, vis, cmds, hits, w, h)
        print("covered %d interior %d wrong %d" % (covered, interior, wrong))
        assert covered > w * h // 2 and 4 * interior >= covered, (covered, interior)
        assert wrong == 0
    finally:
        r.close()
