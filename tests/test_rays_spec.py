"""tests/spec_rays_np.py -- the specification of chordvis_trace_rays -- held to itself on the CPU: the claim that makes the tree
invisible (the slab interval of a union box contains the interval of every box in it, in floating point), the tie rule, miss
records, the clamp on a flat triangle, and the quicker evaluation path against the plain one."""
import numpy as np

import spec_rays_np as S
from chord_amd import lib as L, records as R, scenes

F = np.float32


def _scene_of(positions, triangles, transforms, cam_pos=(0.0, 0.0, 0.0)):
    """One primitive of one LOD-0 meshlet (positions (n, 3), triangles (T, 3) local indices) under each of `transforms`."""
    positions = np.asarray(positions, dtype=np.float32)
    triangles = np.asarray(triangles, dtype=np.int64)
    m = np.zeros(1, dtype=R.MESHLET)
    m["posMin"], m["posMax"], m["coneCutOff"] = positions.min(axis=0), positions.max(axis=0), 1.0
    m["vertexTriangleCount"] = len(positions) | (len(triangles) << 8)
    data = np.concatenate([np.arange(len(positions)), triangles[:, 0] | (triangles[:, 1] << 8) | (triangles[:, 2] << 16)]).astype(np.uint32)
    groups = np.zeros(1, dtype=R.MESHLET_GROUP)
    groups["error"], groups["parentError"], groups["meshletCount"] = -1.0, scenes.FLT_MAX, 1
    groups, nodes = scenes.build_bvh(groups)
    sb = scenes.SceneBuilder("ray_spec")
    sb.prims.append(dict(bvh_nodes=nodes, positions=positions, texcoords=np.zeros((len(positions), 2), np.float32), normals=None, tangents=None,
                         meshlets=m, meshlet_data=data, groups=groups, group_indices=np.zeros(1, dtype=np.uint32)))
    for t in transforms:
        sb.add_object(0, t)
    scene = sb.build()
    L.fill_objects(scene, scenes.Camera(cam_pos, (0.0, 0.0, -1.0), 64, 64))
    return scene


def test_union_interval_contains_every_child_interval():
    """Random boxes in groups of four and random rays, zero, negative-zero and subnormal direction components and origins on box
    faces included: whenever a child's interval is non-empty, the union's is non-empty, starts no later and ends no earlier."""
    rng = np.random.default_rng(5)
    n, rays = 4000, 60
    c = rng.uniform(-10, 10, (n, 4, 3)).astype(F)
    e = (rng.uniform(0, 3, (n, 4, 3)) * (rng.uniform(0, 1, (n, 4, 3)) > 0.15)).astype(F)          # (some boxes flat in an axis)
    lo, hi = c - e, c + e
    ulo, uhi = lo[:, 0], hi[:, 0]
    for k in range(1, 4):
        ulo, uhi = S.rmin(ulo, lo[:, k]), S.rmax(uhi, hi[:, k])
    o = rng.uniform(-12, 12, (rays, 3)).astype(F)
    d = rng.uniform(-1, 1, (rays, 3)).astype(F)
    special = np.array([0.0, -0.0, 1e-42, -1e-45, 1e-38, 3e38, -3e38], dtype=F)
    for r in range(rays):
        for a in range(3):
            if rng.uniform() < 0.35:
                d[r, a] = special[rng.integers(len(special))]
        if r % 7 == 0:
            o[r] = lo[r, r % 4]                                                                   # an origin on a corner of a box
    checked = 0
    for r in range(rays):
        un, uf = S.slab(o[r], d[r], ulo, uhi)
        for k in range(4):
            cn, cf = S.slab(o[r], d[r], lo[:, k], hi[:, k])
            live = ~(cn > cf)
            assert not (un[live] > uf[live]).any()
            assert (un[live] <= cn[live]).all() and (uf[live] >= cf[live]).all()
            checked += int(live.sum())
    assert checked > 10000


def test_ties_go_to_the_smallest_ids():
    # triangle 2 repeats triangle 0; two objects under one matrix
    scene = _scene_of([(0, 0, -2), (1, 0, -2), (1, 1, -2), (0, 1, -2)], [(0, 1, 2), (0, 2, 3), (0, 1, 2)], [np.eye(4), np.eye(4)])
    rays = S.make_rays([(0.7, 0.3, 0.0), (0.3, 0.7, 0.0), (0.7, 0.3, -4.0)], [(0, 0, -1), (0, 0, -1), (0, 0, 1)], 0.0, 1e9)
    for cull in (False, True):
        h = S.trace(scene, scene.objects, rays, meshlet_cull=cull)
        assert list(h["status"]) == [1, 1, 3] and list(h["object"]) == [0, 0, 0] and list(h["triangle"]) == [0, 1, 0]
        assert list(h["t"]) == [2.0, 2.0, 2.0] and list(h["primitive"]) == [0, 0, 0]
    # the later object wins when it is strictly nearer
    scene = _scene_of([(0, 0, -2), (1, 0, -2), (1, 1, -2), (0, 1, -2)], [(0, 1, 2), (0, 2, 3)], [np.eye(4), scenes.translate(0, 0, 0.5)])
    h = S.trace(scene, scene.objects, rays[:1])
    assert h["object"][0] == 1 and h["t"][0] == 1.5


def test_miss_records():
    scene = _scene_of([(0, 0, -2), (1, 0, -2), (1, 1, -2), (0, 1, -2)], [(0, 1, 2), (0, 2, 3)], [np.eye(4)])
    good = S.make_rays([(0.7, 0.3, 0.0)], [(0, 0, -1)], 0.0, 1e9)
    assert S.trace(scene, scene.objects, good)["status"][0] == 1
    bad = []
    for word, value in ((0, np.nan), (1, np.inf), (3, np.nan), (3, -np.inf), (4, np.nan), (6, np.inf), (7, np.nan), (7, np.inf)):
        a = good.copy()
        a.view(F).reshape(-1, 8)[:, word] = value
        bad.append(a)
    a = good.copy(); a["direction"] = (0.0, -0.0, 1e-45); bad.append(a)            # no finite reciprocal
    a = good.copy(); a["tMin"], a["tMax"] = 3.0, 2.5; bad.append(a)                # tMin > tMax
    a = good.copy(); a["tMax"] = 1.5; bad.append(a)                                # too short
    a = good.copy(); a["tMin"] = 2.5; bad.append(a)                                # starts behind it
    a = good.copy(); a["origin"] = (1.7, 0.3, 0.0); bad.append(a)                  # beside it
    bad = np.concatenate(bad)
    for any_hit in (False, True):
        for cull in (False, True):
            h = S.trace(scene, scene.objects, bad, any_hit=any_hit, meshlet_cull=cull)
            assert not h.view(np.uint32).any(), "a miss is eight zero words"
    assert S.trace(scene, scene.objects, good, any_hit=True).view(np.uint32).tolist() == [0, 0, 0, 0, 0, 0, 0, 1]
    edge = good.copy(); edge["tMin"] = edge["tMax"] = 2.0                          # tMin == tMax on the hit
    assert S.trace(scene, scene.objects, edge)["status"][0] == 1


def test_t_is_clamped_into_the_box_intervals():
    """A flat triangle in an axis plane (its box is degenerate in z; its edges are not powers of two, so Moller-Trumbore rounds) met by a slanted ray: the triangle box's interval is one point up to
    rounding, and t is clamped into it, then into the object's interval -- so t lies in both whatever Moller-Trumbore rounded to."""
    m = scenes.translate(0.1, 0.2, 0.3) @ scenes.rotate_y(0.3)
    scene = _scene_of([(0, 0, -2), (3, 0, -2), (1, 5, -2)], [(0, 1, 2)], [m])
    rng = np.random.default_rng(2)
    o = rng.uniform(-0.5, 0.5, (400, 3))
    ba, bb = rng.uniform(0.1, 0.4, 400), rng.uniform(0.1, 0.4, 400)                                # points of the triangle: v0 + a e1 + b e2
    inside = np.stack([3.0 * ba + 1.0 * bb, 5.0 * bb, np.full(400, -2.0), np.ones(400)], axis=1)
    target = (inside @ m.T)[:, :3]
    rays = S.make_rays(o, target - o, 0.0, 1e9)
    h = S.trace(scene, scene.objects, rays)
    assert (h["status"] & 1).sum() > 300
    lo, hi = S.object_boxes(scene.objects, scene.primitives)
    nO, fO = S.slab(rays["origin"], rays["direction"], lo[0], hi[0])
    w = scene.objects["translatedWorldToLocal"][0].astype(F).reshape(4, 4)
    ol = np.stack([((w[0, r] * rays["origin"][:, 0] + w[1, r] * rays["origin"][:, 1]) + w[2, r] * rays["origin"][:, 2]) + w[3, r] for r in range(3)], axis=1)
    dl = np.stack([(w[0, r] * rays["direction"][:, 0] + w[1, r] * rays["direction"][:, 1]) + w[2, r] * rays["direction"][:, 2] for r in range(3)], axis=1)
    nT, fT = S.slab(ol, dl, np.array((0, 0, -2), dtype=F), np.array((3, 5, -2), dtype=F))
    hit = (h["status"] & 1) != 0
    assert (h["t"][hit] >= nO[hit]).all() and (h["t"][hit] <= fO[hit]).all()
    inner = hit & (nT >= nO) & (fT <= fO)                       # (the triangle interval lies inside the object's: the second clamp is idle)
    assert inner.sum() > 100 and (h["t"][inner] >= nT[inner]).all() and (h["t"][inner] <= fT[inner]).all()
    # the clamp acts: for some rays the unclamped Moller-Trumbore t is outside the triangle box's interval
    ok, t, u, v, det = S.pair_candidates(ol, dl, *(np.broadcast_to(np.array(p, dtype=F), ol.shape) for p in ((0, 0, -2), (3, 0, -2), (1, 5, -2))),
                                         np.full(len(ol), -np.inf, dtype=F), np.full(len(ol), np.inf, dtype=F), np.full(len(ol), 0, dtype=F), np.full(len(ol), np.inf, dtype=F))
    assert ok[hit].all() and (t[hit] >= nT[hit]).all() and (t[hit] <= fT[hit]).all()
    with np.errstate(all="ignore"):
        v0, v1, v2 = (np.broadcast_to(np.array(p, dtype=F), ol.shape) for p in ((0, 0, -2), (3, 0, -2), (1, 5, -2)))
        e1, e2, s = v1 - v0, v2 - v0, ol - v0
        raw = S._dot(e2, S._cross(s, e1)) * (F(1.0) / S._dot(e1, S._cross(dl, e2)))           # tMT, before any clamp
    outside = hit & ((raw < nT) | (raw > fT))
    print("rays whose unclamped t lies outside the triangle box's interval: %d of %d" % (outside.sum(), hit.sum()))
    assert outside.sum() >= 1 and (t[outside] != raw[outside]).all()


def test_the_quicker_path_is_the_plain_one():
    """meshlet_cull skips the triangles of meshlets whose box interval is empty (the claim of the first test); the records are the
    plain path's, byte for byte, on a scene with LODs, instances and transforms."""
    scene, cam = scenes.small_test_scene(64, 40, lods=2)
    L.fill_objects(scene, cam)
    tris = S.lod0_triangles(scene)
    assert sum(len(t[0]) for t in tris) == sum(int((m["vertexTriangleCount"] >> 8) & 0xFF) for m in scene.meshlets if m["lod"] == 0)
    rays = S.pixel_rays(L.make_views(cam)[0], 64, 40)[::23]
    a = S.trace(scene, scene.objects, rays, triangles=tris)
    b = S.trace(scene, scene.objects, rays, triangles=tris, meshlet_cull=True)
    assert (a["status"] & 1).sum() > len(rays) // 2 and a.tobytes() == b.tobytes()
    assert S.trace(scene, scene.objects, rays, any_hit=True, triangles=tris)["status"].tolist() == (a["status"] & 1).tolist()
