"""Ray scenes whose trees are as deep as the ray scene allows (ray::kMaxDepth = CHORD_RAY_MAX_DEPTH = 12 interior levels in the BLAS
and in the TLAS), small enough to brute-force, with rays that fill the traversal stack to within two words of its theoretical
high-water mark, 3 * (12 + 12) + 1 = 73 of ray::kStackEntries = 76.  Shared by tests/test_ray_walk_host.py (CPU: the
host build of the walk, which also reports the depths and the stack use) and tests/test_gpu_rays_deep.py.

How a tree gets that deep: the builder's surface-area split peels ONE item off a set whose items are exponentially spaced, until the
depth bound makes it finish by equal counts.  Peeling needs about 2^96 of coordinate range per tree, so the two trees share the x axis
and split the float exponent range between them:

    primitive `chain`   triangle j of 128: x = 2^(j - 125), vertices (x, 0, 0), (x, 1, 0), (x (1 + 2^-7), 0, 1).  Disjoint triangles
                        (384 vertices), so two meshlets of 64.
    objects             instance k of 120: moved along x by T_k = 2^(k + 2) (T_0 = 0), exact in float32 and so is the inverse; the camera
                        at the origin.  World x runs from 2^-125 to 2^121 + 4: every coordinate finite and normal.

Instance 0 is the primitive itself, and it is the DEEPEST leaf of the TLAS (the far, wide-apart boxes are the ones peeled off).  A ray
from the origin along +x at y = z = 1/4 meets the nearest box of every level first -- every entry distance on its way is distinct, so
no tie decides the order -- and every level leaves up to three farther children on the stack beneath the one being walked: twelve
levels of the TLAS, and on top of them twelve levels of instance 0's BLAS.  (Scaled instances, diag(2^k, 1, 1), give the same TLAS
shape but not the stack: an object's box is formed from centre and extent, which rounds the near face 2^(k - 125) of every such box
to 0, every entry distance ties, and the walk starts with the shallow far end.)  Farther instances lie beyond 2^26, where their
world-space boxes are flat and the hit distances of all their triangles tie: the answer is still the specification's, by its tie rule."""
import functools

import numpy as np

import spec_rays_np as S
from chord_amd import lib as L, records as R, scenes

F = np.float32
CHAIN_TRIANGLES, CHAIN_INSTANCES = 128, 120
MAX_DEPTH = 12                               # ray::kMaxDepth
STACK_ENTRIES = 76                           # ray::kStackEntries
STACK_BOUND = 3 * (MAX_DEPTH + MAX_DEPTH) + 1
STACK_REACHED = STACK_BOUND - 2              # what the stack-filling ray must reach
MIRRORED = 37                                # the instance of `deep` that is mirrored in z (about z = 1/2)


def meshlet_primitive(positions, tris_per_meshlet, group_sizes):
    """A finished-primitive dictionary (scenes.PrimitiveBuilder.finish) of LOD-0 meshlets written directly: positions (n, 3), and per
    meshlet an int array (T, 3) of indices into them (none: a meshlet of every vertex and no triangle)."""
    positions = np.asarray(positions, dtype=np.float32)
    meshlets, data, nd = np.zeros(len(tris_per_meshlet), dtype=R.MESHLET), [], 0
    for k, tris in enumerate(tris_per_meshlet):
        tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
        gid = np.unique(tris) if len(tris) else np.arange(len(positions))
        local = np.searchsorted(gid, tris)
        m = meshlets[k]
        m["posMin"], m["posMax"] = positions[gid].min(axis=0), positions[gid].max(axis=0)
        m["coneCutOff"] = 1.0                                              # (a cone that never culls)
        m["vertexTriangleCount"] = len(gid) | (len(tris) << 8)
        m["dataOffset"] = nd
        data.append(np.concatenate([gid, local[:, 0] | (local[:, 1] << 8) | (local[:, 2] << 16)]).astype(np.uint32))
        nd += len(gid) + len(tris)
    groups = np.zeros(len(group_sizes), dtype=R.MESHLET_GROUP)
    groups["error"], groups["parentError"] = -1.0, scenes.FLT_MAX
    groups["meshletCount"] = group_sizes
    groups["meshletOffset"] = np.concatenate([[0], np.cumsum(group_sizes)[:-1]])
    groups, nodes = scenes.build_bvh(groups)
    return dict(bvh_nodes=nodes, positions=positions, texcoords=np.zeros((len(positions), 2), np.float32), normals=None, tangents=None,
                meshlets=meshlets, meshlet_data=np.concatenate(data), groups=groups,
                group_indices=np.arange(len(tris_per_meshlet), dtype=np.uint32))


def chain_positions(n=CHAIN_TRIANGLES, first=-125):
    """(3 n, 3) float64: the vertices of n exponentially spaced triangles across the unit cross-section, every value exact in float32."""
    x = 2.0 ** (np.arange(n) + first)
    p = np.zeros((n, 3, 3))
    p[:, 0] = np.stack([x, np.zeros(n), np.zeros(n)], axis=1)
    p[:, 1] = np.stack([x, np.ones(n), np.zeros(n)], axis=1)
    p[:, 2] = np.stack([x * (1.0 + 2.0 ** -7), np.zeros(n), np.ones(n)], axis=1)
    assert np.array_equal(p.astype(F).astype(np.float64), p)
    return p.reshape(-1, 3)


def chain_primitive(n=CHAIN_TRIANGLES, first=-125):
    tris = np.arange(3 * n).reshape(n, 3)
    return meshlet_primitive(chain_positions(n, first), [tris[k:k + 64] for k in range(0, n, 64)], ((n + 63) // 64,))


def chain_boxes(n=CHAIN_TRIANGLES):
    """(lo, hi) float32 (n, 3): the triangle boxes of the chain primitive (what tests/ray_build_main.cpp builds its case from)."""
    p = chain_positions(n).astype(F).reshape(n, 3, 3)
    return p.min(axis=1), p.max(axis=1)


def offsets(n=CHAIN_INSTANCES):
    """T_k: 0, 8, 16, 32, ... 2^(n + 1)."""
    return np.concatenate([[0.0], 2.0 ** (np.arange(1, n) + 2.0)])


def deep_scene():
    """BLAS and TLAS both 12 levels: 120 instances of the chain, one of them mirrored in z about z = 1/2."""
    sb = scenes.SceneBuilder("ray_deep")
    sb.prims.append(chain_primitive())
    for k, t in enumerate(offsets()):
        sb.add_object(0, scenes.translate(t, 0.0, 1.0) @ scenes.scale(1.0, 1.0, -1.0) if k == MIRRORED else scenes.translate(t, 0.0, 0.0))
    return sb.build()


def deep_blas_only_scene():
    """The 12-level BLAS under a TLAS of one node: four plain instances."""
    sb = scenes.SceneBuilder("ray_deep_blas_only")
    sb.prims.append(chain_primitive())
    for t in (0.0, 8.0, 64.0, 4096.0):
        sb.add_object(0, scenes.translate(t, 0.0, 0.0))
    return sb.build()


def deep_tlas_only_scene():
    """The 12-level TLAS over BLASes of one node: 120 instances of a 4-triangle chain that starts at x = 2^-125 -- and, in the
    middle of the list, one instance of a primitive with NO LOD-0 triangle (no BLAS: blasRoot is `no child`), whose box spans the
    whole chain: every ray through it must fall through to what lies behind."""
    sb = scenes.SceneBuilder("ray_deep_tlas_only")
    sb.prims.append(chain_primitive(4))
    sb.prims.append(meshlet_primitive(np.array([(2.0 ** -100, 0, 0), (2.0 ** 100, 1, 0), (1.0, 0, 1)]), [np.zeros((0, 3), dtype=np.int64)], (1,)))
    for k, t in enumerate(offsets()):
        if k == 60:
            sb.add_object(1)
        sb.add_object(0, scenes.translate(t, 0.0, 0.0))
    return sb.build()


SCENES = {"deep": deep_scene, "deep_blas_only": deep_blas_only_scene, "deep_tlas_only": deep_tlas_only_scene}
CAMERA = scenes.Camera((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), 64, 64)
FILL, WALK = 0, 1                            # indices into deep_rays(): the stack-filling hit, and the complete walk that misses


def deep_rays():
    """A few hundred rays along and near the x axis (the module's docstring says why); rays 0 and 1 are FILL and WALK."""
    o, d, lo, hi = [], [], [], []

    def add(origin, direction, t_min=0.0, t_max=3.0e38):
        o.append(origin); d.append(direction); lo.append(t_min); hi.append(t_max)

    add((0.0, 0.25, 0.25), (1.0, 0.0, 0.0))                                 # FILL: the nearest child first on every level of both trees
    add((0.0, 0.9, 0.5), (1.0, 0.0, 0.0))                                   # WALK: through every box, u + v > 1 on every triangle
    far = 2.0 ** 123
    for y, z in ((0.25, 0.25), (0.5, 0.125), (0.9, 0.5), (0.0625, 0.75)):   # back along -x from beyond the far end: closest-hit pruning
        add((far, y, z), (-1.0, 0.0, 0.0))
        add((far, y, z), (-2.0 ** 60, 0.0, 0.0))
    r = scenes.rand01(71, np.arange(6 * 160)).reshape(160, 6)
    for k in range(160):                                                    # origins log-uniform in x, between and inside instances
        e = -126.0 + 248.0 * r[k, 0]
        x = 2.0 ** e if k % 4 else 2.0 ** round(e)                          # (every fourth exactly on a triangle's plane x = 2^n)
        y, z = (0.05 + 0.9 * r[k, 1]) * 0.5, (0.05 + 0.9 * r[k, 2]) * 0.5   # u + v < 1: these meet triangles
        sign = 1.0 if k % 2 else -1.0
        if k % 5 == 0:                                                      # a window that opens and closes in the middle of the chain
            add((0.0, y, z), (1.0, 0.0, 0.0), 2.0 ** (e - 3.0 * r[k, 3]), 2.0 ** (e + 6.0 * r[k, 4]))
        elif k % 5 == 1:
            add((x, y, z), (sign, 0.0, 0.0), x * 2.0 ** (-8.0 * r[k, 3]), x * 2.0 ** (8.0 * r[k, 4] - 2.0))
        else:
            add((x, y, z), (sign * 2.0 ** round(20.0 * r[k, 5] - 10.0), 0.0, 0.0))
    r = scenes.rand01(72, np.arange(5 * 60)).reshape(60, 5)
    for k in range(60):                                                     # small slopes: the ray leaves the cross-section part-way
        e = -120.0 + 230.0 * r[k, 0]
        reach = 2.0 ** (e + 12.0 * r[k, 1])
        y, z = r[k, 2] * 0.6, r[k, 3] * 0.4
        dy, dz = (1.0 - y) / reach * (1.0 if k % 3 else -y / (1.0 - y)), (0.5 - z) / reach * (r[k, 4] * 2.0 - 1.0)
        add((0.0 if k % 2 else 2.0 ** e, y, z), (1.0, dy, dz))
    for y, z in ((0.0, 0.25), (1.0, 0.0), (0.5, 0.0), (0.0, 0.0), (0.0, 1.0), (0.25, 0.75), (0.5, 0.5), (0.75, 0.25), (1.0, 0.5), (0.5, 1.0)):
        add((0.0, y, z), (1.0, 0.0, 0.0))                                   # on the faces y = 0, y = 1, z = 0 and the diagonal u + v = 1
        add((2.0 ** 122, y, z), (-1.0, 0.0, 0.0))
        add((2.0 ** -30, y, z), (1.0, 0.0, 0.0), 0.0, 2.0 ** 20)
    rays = np.zeros(len(o), dtype=R.RAY)
    rays["origin"], rays["direction"] = np.array(o, dtype=F), np.array(d, dtype=F)
    rays["tMin"], rays["tMax"] = np.array(lo, dtype=F), np.array(hi, dtype=F)
    extra = []
    a = rays[:40].copy(); a["tMin"], a["tMax"] = 2.0, 1.0; extra.append(a)                  # tMin > tMax
    a = rays[:40].copy(); a["direction"][:, 1] = 1e-42; extra.append(a)                     # a subnormal direction component
    a = rays[10:50].copy(); a["direction"][:, 2] = -1e-45; extra.append(a)
    rays = np.concatenate([rays] + extra)
    assert np.isfinite(rays.view(F)).all()
    return rays


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene with records filled, lod0 triangles, rays, expected closest hits, expected any-hit) -- computed once, read-only."""
    scene = SCENES[name]()
    L.fill_objects(scene, CAMERA)
    tris = S.lod0_triangles(scene)
    rays = deep_rays()
    want = S.trace(scene, scene.objects, rays, triangles=tris, meshlet_cull=True)
    want_any = np.zeros(len(rays), dtype=R.RAY_HIT)
    want_any["status"] = want["status"] & 1
    for a in (rays, want, want_any):
        a.setflags(write=False)
    return scene, tris, rays, want, want_any


def conditions(want):
    """What the ray set must do on scene `deep`, from the specification alone: [] when it does."""
    hit = (want["status"] & 1) != 0
    bad = []
    if hit.sum() < 100 or (~hit).sum() < 50:
        bad.append("hits %d (>= 100), misses %d (>= 50)" % (hit.sum(), (~hit).sum()))
    if len(np.unique(want["object"][hit])) < 30:
        bad.append("hits land in %d distinct objects (>= 30)" % len(np.unique(want["object"][hit])))
    pairs = np.unique(np.stack([want["meshlet"][hit], want["triangle"][hit]], axis=1), axis=0)
    if len(pairs) < 30:
        bad.append("hits land on %d distinct triangles (>= 30)" % len(pairs))
    if not ((want["status"] == 1).any() and (want["status"] == 3).any()):
        bad.append("front and back faces must both be met")
    return bad
