"""Scenes of meshlets chosen for their shape -- (vertex count V, triangle count T) -- up to the contract's 255 / 128.  TEST INFRASTRUCTURE.

The procedural generators emit 81 / 128 patches and chordvis_nanite_build grows meshlets along shared edges (V <= T + 2), so nothing
else in the suite sends a cluster of more than 130 vertices through the set-up kernels.  The meshlets here are written directly in
the importer's output format: records.MESHLET, records.MESHLET_GROUP and the [V vertex ids][T words i0 | i1 << 8 | i2 << 16] stream.

One shape is a unit patch of T triangles laid along a serpentine of cells, front-facing (counter-clockwise in x, y; the camera
looks down -z), z rising with the vertex's creation order (a depth of its own per triangle).  Triangle k brings n_k new vertices
(n_0 = 3, the rest of V - 3 spread evenly over the T - 1 others, each 0..3) and takes its other corners from the six newest
vertices before it, never the same three twice.  Every local index is used.  A `permuted` shape numbers its local indices by a
seeded permutation of the creation order -- its vertex-id table is then not ascending -- and, where it is not the first meshlet of its
primitive, its first two vertices are global vertices of the meshlet before it.  Every global vertex has a texture coordinate of its
own, made from the local index it has in the meshlet that created it.

Three primitives, laid on one 6 x 4 grid of cells (pitch 1.2) in a common space:
  0: the shapes up to 65 vertices and, in the middle of its stream, the meshlet of 6 vertices and no triangle (groups of 4, 3, 1);
  1: 81..128 vertices (groups of 2, 3);
  2: every shape of more than 128 vertices (groups of 1, 2, 4, 2).
Variants (scene(variant) -> (records.Scene, camera)):
  plain   one object per primitive, a patch ~36 pixels across at 320 x 200;
  masked  the same under the alpha-tested materials, textures and samplers of scenes.masked_test_scene;
  tiny    60 scaled copies of the three objects, a patch 2..6 pixels across;
  near    plain plus 27 copies of primitive 2 laid as floors 3..14 cm under the camera, three (NEAR_SHIFTS) with the patch of each
          shape of more than 128 vertices under the camera's foot: their triangles straddle the camera plane (w = 0), which is
          what sends a triangle to the clipper (the near plane and the guard band).
cut_last gives the transforms of a frame before that send a whole frame through the second raster pass."""
import itertools
import math

import numpy as np

from chord_amd import records as R
from chord_amd import scenes

SHAPES = [(3, 1), (4, 2), (33, 32), (34, 33), (64, 62), (65, 64), (65, 63), (98, 96), (99, 97), (81, 128), (127, 65), (128, 128),
          (129, 43), (129, 128), (130, 128), (191, 127), (192, 64), (193, 65), (254, 128), (255, 85), (255, 128)]
EMPTY = (6, 0)
# the meshlets of each primitive in stream order, and its groups' sizes
PRIMS = [([(3, 1), (4, 2), (33, 32), (34, 33), EMPTY, (64, 62), (65, 64), (65, 63)], (4, 3, 1)),
         ([(98, 96), (99, 97), (81, 128), (127, 65), (128, 128)], (2, 3)),
         ([(129, 43), (129, 128), (130, 128), (191, 127), (192, 64), (193, 65), (254, 128), (255, 85), (255, 128)], (1, 2, 4, 2))]
# grid cell (column, row) of the k-th meshlet of each primitive
CELLS = [[(c, r) for r in range(3) for c in range(3)][:8], [(c, 3) for c in range(5)], [(3 + c, r) for r in range(3) for c in range(3)]]
PITCH = 1.2
CENTRE = (3.5, 2.3, 0.0)
BANDS = ((0, 64), (64, 128), (128, 192), (192, 255))
W, H = 320, 200
NEAR_SHIFTS = ((0.0, 0.0), (0.17, -0.11), (-0.13, 0.19))     # where in its patch (patch units from the centre) a floor copy has the camera's foot


def bands_of(V):
    return [b for b, (lo, _) in enumerate(BANDS) if V > lo]


def shape_topology(V, T, seed, given=None):
    """(xy float64[V, 2] in the unit square, z float64[V], tris int[T, 3]) in creation order.  given: xy of the first len(given)
    vertices (vertices that another meshlet owns), or None."""
    rnd = scenes.rand01(seed, np.arange(4 * V + 8))
    xy, z = np.zeros((V, 2)), np.zeros(V)
    if T == 0:
        for c in range(V):
            xy[c] = (0.2 + 0.6 * rnd[2 * c], 0.2 + 0.6 * rnd[2 * c + 1])
        return xy, z, np.zeros((0, 3), np.int64)
    cols = int(math.ceil(math.sqrt(T)))
    cell = 1.0 / cols
    up = [-((-k * (V - 3)) // (T - 1)) for k in range(T)] if T > 1 else [0]          # ceil(k (V - 3) / (T - 1)): a triangle without a new vertex comes late
    news = [3] + [up[k] - up[k - 1] for k in range(1, T)]
    assert sum(news) == V and all(0 <= n <= 3 for n in news)
    made, used, tris = 0, set(), []

    def area(t):
        a, b, c = xy[t[0]], xy[t[1]], xy[t[2]]
        return 0.5 * ((b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]))

    for k, n in enumerate(news):
        row, col = k // cols, k % cols
        if row % 2:
            col = cols - 1 - col
        cx, cy = (col + 0.5) * cell, (row + 0.5) * cell
        first = made
        for j in range(n):
            c = made
            if given is not None and c < len(given):
                xy[c] = given[c]
            else:
                ang = 2.0 * math.pi * (j / 3.0 + 0.25 * rnd[4 * c]) + k
                rad = cell * (0.42 if n > 1 else 0.25) * (0.8 + 0.2 * rnd[4 * c + 1])
                xy[c] = (cx + rad * math.cos(ang), cy + rad * math.sin(ang))
            z[c] = 0.15 * (c + rnd[4 * c + 2]) / V
            made += 1
        mine = list(range(first, made))
        recent = list(range(first - 1, max(first - 7, -1), -1))
        pick = None
        for least in (0.04 * cell * cell, 1e-4 * cell * cell):
            for old in itertools.combinations(recent, 3 - n):
                t = tuple(sorted(mine + list(old)))
                if t not in used and abs(area(t)) >= least:
                    pick = t
                    break
            if pick:
                break
        assert pick is not None, (V, T, k)
        used.add(pick)
        tris.append(pick if area(pick) > 0 else (pick[0], pick[2], pick[1]))
    assert made == V
    return xy, z, np.array(tris, dtype=np.int64)


def meshlet_bounds(pos, tris):
    """AABB and meshopt-style normal cone of one meshlet (scenes._meshlet_bounds for any topology); no triangles: a cone that never culls."""
    pmin, pmax = pos.min(axis=0), pos.max(axis=0)
    never = (pmin, pmax, np.zeros(3, np.float32), np.float32(1.0), np.zeros(3, np.float32))
    if len(tris) == 0:
        return never
    p = pos.astype(np.float64)
    a, b, c = p[tris[:, 0]], p[tris[:, 1]], p[tris[:, 2]]
    n = np.cross(b - a, c - a)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    assert (ln > 0).all()
    n = n / ln
    axis = n.sum(axis=0)
    axis = axis / np.linalg.norm(axis)
    dp = n @ axis
    mindp = dp.min()
    if mindp <= 0.1:
        return never
    centre = 0.5 * (pmin.astype(np.float64) + pmax.astype(np.float64))
    t = ((centre[None, :] - a) * n).sum(axis=1) / dp
    apex = centre - axis * max(t.max(), 0.0)
    return pmin, pmax, axis.astype(np.float32), np.float32(math.sqrt(max(0.0, 1.0 - mindp * mindp))), apex.astype(np.float32)


def is_permuted(p, k):
    """Whether the k-th meshlet of primitive p numbers its local indices by a permutation (two of three do)."""
    return (p + k) % 3 != 0


def _primitive(p):
    """The finished-primitive dictionary of scenes.PrimitiveBuilder.finish for primitive p."""
    shapes, group_sizes = PRIMS[p]
    positions, uvs, meshlets, data = [], [], np.zeros(len(shapes), dtype=R.MESHLET), []
    nverts = ndata = 0
    last_ids = None                                    # global ids of the meshlet before, in its creation order
    for k, (V, T) in enumerate(shapes):
        gx, gy = CELLS[p][k]
        origin = np.array([gx * PITCH, gy * PITCH])
        seed = 7000 + 100 * p + k
        borrow = 2 if (is_permuted(p, k) and last_ids is not None and T > 0 and len(last_ids) >= 4) else 0
        given = None
        if borrow:
            ids = [last_ids[-2], last_ids[-4]]
            given = [(np.asarray(positions[i][:2], dtype=np.float64) - origin) for i in ids]
        xy, z, tris = shape_topology(V, T, seed, given)
        perm = np.arange(V)
        if is_permuted(p, k):
            perm = np.argsort(scenes.rand01(seed + 50, np.arange(V)), kind="stable")      # local index l holds created vertex perm[l]
            assert not np.array_equal(perm, np.arange(V)) or V < 2
        local_of = np.argsort(perm)                                                       # created vertex c has local index local_of[c]
        gid = np.zeros(V, dtype=np.int64)
        for c in range(V):
            if c < borrow:
                gid[c] = ids[c]
                continue
            gid[c] = nverts
            positions.append(np.array([origin[0] + xy[c, 0], origin[1] + xy[c, 1], z[c] + 0.01 * k], dtype=np.float32))
            l = int(local_of[c])
            uvs.append(np.array([3.0 * (l + 0.5) / V + 0.0137 * k + 0.0031 * p, 2.0 * ((l * 0.6180339887 + 0.077 * k) % 1.0)], dtype=np.float32))
            nverts += 1
        pos = np.stack([positions[i] for i in gid])
        pmin, pmax, axis, cutoff, apex = meshlet_bounds(pos, tris)
        m = meshlets[k]
        m["posMin"], m["posMax"], m["coneAxis"], m["coneCutOff"], m["coneApex"] = pmin, pmax, axis, cutoff, apex
        m["lod"] = 0
        m["vertexTriangleCount"] = V | (T << 8)
        m["dataOffset"] = ndata
        words = local_of[tris[:, 0]] | (local_of[tris[:, 1]] << 8) | (local_of[tris[:, 2]] << 16) if T else np.zeros(0, np.int64)
        data.append(np.concatenate([gid[perm], words]).astype(np.uint32))
        ndata += V + T
        last_ids = gid
    assert sum(group_sizes) == len(shapes)
    groups = np.zeros(len(group_sizes), dtype=R.MESHLET_GROUP)
    groups["error"], groups["parentError"] = -1.0, scenes.FLT_MAX           # un-parented LOD-0 groups
    groups["meshletCount"] = group_sizes
    groups["meshletOffset"] = np.concatenate([[0], np.cumsum(group_sizes)[:-1]])
    groups, nodes = scenes.build_bvh(groups)
    return dict(bvh_nodes=nodes, positions=np.stack(positions), texcoords=np.stack(uvs), normals=None, tangents=None, meshlets=meshlets,
                meshlet_data=np.concatenate(data), groups=groups, group_indices=np.arange(len(shapes), dtype=np.uint32))


def _builder(name, masked):
    """A SceneBuilder holding the three primitives and masked_test_scene's textures, samplers and first three materials (the
    materials without their alpha test unless masked: the same sidedness either way)."""
    sb = scenes.SceneBuilder(name)
    tex = [sb.add_texture(t) for t in scenes._alpha_textures(3)]
    smp = [sb.add_sampler(R.FILTER_LINEAR_MIPMAP_LINEAR, R.FILTER_LINEAR, R.WRAP_REPEAT, R.WRAP_REPEAT),
           sb.add_sampler(R.FILTER_NEAREST, R.FILTER_NEAREST, R.WRAP_CLAMP_TO_EDGE, R.WRAP_MIRRORED_REPEAT),
           sb.add_sampler(R.FILTER_LINEAR_MIPMAP_NEAREST, R.FILTER_NEAREST, R.WRAP_MIRRORED_REPEAT, R.WRAP_CLAMP_TO_EDGE)]
    mode = R.ALPHA_MASK if masked else 0
    mats = [sb.add_material(0, mode, tex[0], smp[0], 0.5, 1.0),
            sb.add_material(1, mode, tex[1], smp[1], 0.4, 0.9),
            sb.add_material(1, mode, tex[2], smp[2], 0.35, 1.0)]
    for p in range(len(PRIMS)):
        sb.prims.append(_primitive(p))
    return sb, mats


def _about_centre(m):
    return scenes.translate(*CENTRE) @ m @ scenes.translate(*(-c for c in CENTRE))


def scene(variant="plain"):
    """(records.Scene, camera) of a variant; the scene has local_to_world, like every scenes.* scene."""
    assert variant in ("plain", "masked", "tiny", "near")
    sb, mats = _builder("meshlet_shapes_" + variant, variant == "masked")
    cam = scenes.Camera((3.5, 2.3, 6.6), (0.03, -0.02, -1.0), W, H)
    tilt = _about_centre(scenes.rotate_y(0.12) @ scenes.rotate_x(-0.08))
    if variant == "tiny":
        for i in range(60):
            r = scenes.rand01(7700, np.arange(6 * i, 6 * i + 6))
            spot = scenes.translate(0.45 + 0.68 * (i % 10) + 0.2 * r[0] - CENTRE[0], 0.4 + 0.75 * (i // 10) + 0.2 * r[1] - CENTRE[1], -0.8 + 1.6 * r[2])
            m = spot @ _about_centre(scenes.rotate_y(0.5 * (r[3] - 0.5)) @ scenes.scale(0.06 + 0.1 * r[4]))
            for p in range(len(PRIMS)):
                sb.add_object(p, m, material=0 if (i + p) % 2 else mats[2])       # one-sided / two-sided
    else:
        for p in range(len(PRIMS)):
            sb.add_object(p, tilt, material=mats[p] if variant == "masked" else (0, mats[1], 0)[p])
    if variant == "near":
        for i, (gx, gy) in enumerate(CELLS[2]):
            for j, (dx, dy) in enumerate(NEAR_SHIFTS):
                # the patch's plane becomes a floor under the camera (patch +y -> forward, patch +z -> up), a little tilted
                floor = scenes.rotate_x(-1.47) @ scenes.rotate_z(0.3 * i + 1.1 * j)
                under = scenes.translate(cam.position[0], cam.position[1] - 0.03 - 0.004 * (3 * i + j), cam.position[2] - 0.02)
                sb.add_object(2, under @ floor @ scenes.translate(-(gx * PITCH + 0.5 + dx), -(gy * PITCH + 0.5 + dy), -0.1),
                              material=0 if (i + j) % 2 else mats[1])
    return sb.build(), cam


def meshlet_table(sc):
    """[(primitive, meshlet id in the scene, V, T, dataOffset)] read back from the scene's records."""
    out = []
    for p, prim in enumerate(sc.primitives):
        end = int(sc.primitives[p + 1]["meshletOffset"]) if p + 1 < len(sc.primitives) else len(sc.meshlets)
        for m in range(int(prim["meshletOffset"]), end):
            vt = int(sc.meshlets[m]["vertexTriangleCount"])
            out.append((p, m, vt & 0xFF, (vt >> 8) & 0xFF, int(sc.meshlets[m]["dataOffset"])))
    return out


def triangle_locals(sc, m):
    """int[T, 3] local indices of meshlet m's triangles, decoded from the stream."""
    vt = int(sc.meshlets[m]["vertexTriangleCount"])
    V, T, off = vt & 0xFF, (vt >> 8) & 0xFF, int(sc.meshlets[m]["dataOffset"])
    w = sc.meshlet_data[off + V: off + V + T].astype(np.int64)
    return np.stack([w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFF], axis=1)


def project(sc, iv, obj, m):
    """(pixel x, pixel y, clip w), float64[V] each in local-index order, of meshlet m under object obj (records filled) and the
    instance view iv -- in double precision: for choosing and describing scenes, not for comparing images."""
    vt = int(sc.meshlets[m]["vertexTriangleCount"])
    V, off = vt & 0xFF, int(sc.meshlets[m]["dataOffset"])
    base = int(sc.primitives[int(sc.objects[obj]["GLTFPrimitiveDetail"])]["vertexOffset"])
    p = sc.positions[base + sc.meshlet_data[off: off + V].astype(np.int64)].astype(np.float64)
    l2t = sc.objects[obj]["localToTranslatedWorld"].reshape(4, 4).T.astype(np.float64)           # glm column-major
    vp = iv["translatedWorldToClip"][0].reshape(4, 4).T.astype(np.float64)
    h = np.concatenate([p, np.ones((V, 1))], axis=1) @ (vp @ l2t).T
    aw = np.maximum(np.abs(h[:, 3]), 1e-30)
    return (h[:, 0] / aw * 0.5 + 0.5) * float(iv["renderDimension"][0][0]), (h[:, 1] / aw * -0.5 + 0.5) * float(iv["renderDimension"][0][1]), h[:, 3]


def displaced(sc, band, by, min_vertices=129):
    """A copy of the scene in which the vertices that the meshlets of at least min_vertices vertices hold at the local indices of
    `band` are moved by `by` (x, y in the primitives' space)."""
    pos = sc.positions.copy()
    lo, hi = BANDS[band]
    moved = set()
    for p, m, V, T, off in meshlet_table(sc):
        if V >= min_vertices and V > lo:
            base = int(sc.primitives[p]["vertexOffset"])
            moved.update((base + sc.meshlet_data[off + lo: off + min(V, hi)].astype(np.int64)).tolist())
    idx = np.array(sorted(moved), dtype=np.int64)
    pos[idx, 0] += by[0]
    pos[idx, 1] += by[1]
    out = R.Scene(sc.objects, sc.primitives, sc.materials, sc.meshlets, sc.groups, sc.group_indices, sc.meshlet_data, pos, name=sc.name,
                  texcoord0=sc.texcoord0, textures=sc.texture_images, samplers=sc.samplers, bvh_nodes=sc.bvh_nodes)
    out.local_to_world = sc.local_to_world
    return out, len(idx)


def only_objects(sc, keep):
    """The scene with the objects `keep` (indices) alone; local_to_world follows."""
    keep = np.asarray(keep, dtype=np.int64)
    out = sc.with_objects(sc.objects[keep].copy())
    out.local_to_world = np.ascontiguousarray(sc.local_to_world[keep])
    return out


def cut_last(sc, cam, distance=500.0):
    """local_to_world of a frame before in which every object 'was' `distance` to the camera's right and a fifth of that further
    down the view: in front of the camera and beside its screen, so this frame's first pass rejects every cluster and all of them
    go through the second pass.  (The scenes here have no backdrop: an object that 'was' straight down the view would be tested
    against the empty texels between the patches and stay in the first pass; one whose box reaches behind the camera plane is
    never rejected.)"""
    f = np.asarray(cam.front, dtype=np.float64)
    f /= np.linalg.norm(f)
    right = np.cross(f, np.asarray(cam.world_up, dtype=np.float64))
    right /= np.linalg.norm(right)
    last = sc.local_to_world.copy()
    last[:, 12:15] += distance * right + 0.2 * distance * f     # glm column-major: the translation column
    return last
