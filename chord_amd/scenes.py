"""Deterministic procedural meshlet scenes for BASELINE.json's configs.

The reference ships no Sponza/Bistro assets (install/resource/mesh holds only
low_sphere.glb) and its importer needs METIS (nanite_builder.cpp:692-716), so
the inputs are synthesized here in the *output format* of the reference's
importer: meshlets of <=255 vertices / <=128 triangles with AABB + normal cone
(nanite_builder.cpp:1024-1044, meshopt_clusterizer.cpp:760-860), meshlet groups
that share one (error sphere, parent error sphere) (nanite_builder.cpp:313-395),
and the packed meshletData stream [V vertex ids][T tris i0|i1<<8|i2<<16]
(asset_gltf_helper.cpp:522-548).

Every surface is a grid of 9x9-vertex patches (81 vertices / 128 triangles per
meshlet).  LOD levels follow a patch quadtree: the 4 LOD0 patches of a 2x2
block are replaced by 2 LOD1 meshlets (half the triangles), the 8 LOD1 meshlets
of a 4x4 block by 4 LOD2 meshlets.
"""
import ctypes as C
import math

import numpy as np

from . import records as T

FLT_MAX = np.float32(3.4028234663852886e38)


def pcg_hash(v):
    """Counter-based PCG (Jarzynski & Olano 2020) on uint32 arrays."""
    v = np.asarray(v, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    state = (v * np.uint64(747796405) + np.uint64(2891336453)) & np.uint64(0xFFFFFFFF)
    sh = ((state >> np.uint64(28)) + np.uint64(4))
    word = (((state >> sh) ^ state) * np.uint64(277803737)) & np.uint64(0xFFFFFFFF)
    return (((word >> np.uint64(22)) ^ word) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def pcg32(seed, i):
    """i-th 32-bit value of stream `seed`."""
    return pcg_hash((np.uint64(seed) * np.uint64(0x9E3779B9) + np.asarray(i, dtype=np.uint64)) & np.uint64(0xFFFFFFFF))


def rand01(seed, i):
    return (pcg32(seed, i).astype(np.float64) / 4294967295.0)


# ---------------------------------------------------------------------------------------------
# 9x9 patch topology: vertex (i, j) -> j*9+i ; cell -> (v00, v10, v11), (v00, v11, v01): CCW
# when the parameter plane is seen with u to the right and v up (normal = dS/du x dS/dv).

def _patch_tri_table():
    tris = []
    for j in range(8):
        for i in range(8):
            v00 = j * 9 + i
            v10 = v00 + 1
            v01 = v00 + 9
            v11 = v01 + 1
            tris.append(v00 | (v10 << 8) | (v11 << 16))
            tris.append(v00 | (v11 << 8) | (v01 << 16))
    return np.array(tris, dtype=np.uint32)


PATCH_TRIS = _patch_tri_table()
PATCH_V, PATCH_T = 81, 128
_TI = np.stack([PATCH_TRIS & 0xFF, (PATCH_TRIS >> 8) & 0xFF, (PATCH_TRIS >> 16) & 0xFF], axis=1).astype(np.int64)


def _meshlet_bounds(pos):
    """pos: (M, 81, 3) float32 -> AABB + meshopt-style normal cone per meshlet."""
    pos64 = pos.astype(np.float64)
    pmin = pos.min(axis=1)
    pmax = pos.max(axis=1)
    a, b, c = pos64[:, _TI[:, 0]], pos64[:, _TI[:, 1]], pos64[:, _TI[:, 2]]
    n = np.cross(b - a, c - a)                                # (M, 128, 3)
    ln = np.linalg.norm(n, axis=2, keepdims=True)
    valid = ln[..., 0] > 0
    n = np.where(ln > 0, n / np.maximum(ln, 1e-300), 0.0)
    axis = n.sum(axis=1)
    la = np.linalg.norm(axis, axis=1, keepdims=True)
    axis = np.where(la > 0, axis / np.maximum(la, 1e-300), 0.0)
    dp = (n * axis[:, None, :]).sum(axis=2)
    dp = np.where(valid, dp, 1.0)
    mindp = dp.min(axis=1)
    center = 0.5 * (pmin.astype(np.float64) + pmax.astype(np.float64))
    # apex = center - axis * maxt, t = dot(center - corner, n) / dot(axis, n)
    dc = ((center[:, None, :] - a) * n).sum(axis=2)
    dn = np.where(dp > 1e-6, dp, 1.0)
    t = np.where(valid, dc / dn, 0.0)
    maxt = np.maximum(t.max(axis=1), 0.0)
    apex = center - axis * maxt[:, None]
    cutoff = np.sqrt(np.maximum(0.0, 1.0 - mindp * mindp))
    degenerate = mindp <= 0.1                                  # meshopt: cone wider than ~168 deg => never culls
    axis = np.where(degenerate[:, None], 0.0, axis)
    apex = np.where(degenerate[:, None], 0.0, apex)
    cutoff = np.where(degenerate, 1.0, cutoff)
    return pmin, pmax, axis.astype(np.float32), cutoff.astype(np.float32), apex.astype(np.float32)


class PrimitiveBuilder:
    """Accumulates parametric surfaces into one primitive (one GLTFPrimitiveBuffer).

    attributes=True also makes per-vertex normals and tangents (surface_frames): smooth, unit length in float32, the tangent along
    +u, its handedness w alternating +1 / -1 from one add_surface to the next."""

    def __init__(self, attributes=False):
        self.attributes = attributes
        self.normals = []          # list of (n,3) float32 (attributes only)
        self.tangents = []         # list of (n,4) float32 (attributes only)
        self.nsurfaces = 0
        self.positions = []        # list of (n,3) float32
        self.texcoords = []        # list of (n,2) float32: the surface parameters (u, v) times uv_scale
        self.uv_scale = (1.0, 1.0)
        self.nverts = 0
        self.meshlets = []         # list of structured arrays (dataOffset relative to primitive)
        self.meshlet_data = []     # list of uint32 arrays
        self.ndata = 0
        self.nmeshlets = 0
        self.groups = []
        self.group_indices = []
        self.nindices = 0

    def _add_meshlets(self, pos, lod, uv=None):
        """pos (M,81,3) float32, uv (M,81,2). Returns meshlet ids (relative to this primitive)."""
        M = pos.shape[0]
        self.texcoords.append(np.zeros((M * PATCH_V, 2), np.float32) if uv is None else uv.reshape(-1, 2).astype(np.float32))
        if self.attributes:
            self.normals.append(self._last_frame[0].reshape(-1, 3))
            self.tangents.append(self._last_frame[1].reshape(-1, 4))
        pmin, pmax, axis, cutoff, apex = _meshlet_bounds(pos)
        ml = np.zeros(M, dtype=T.MESHLET)
        ml["posMin"], ml["posMax"] = pmin, pmax
        ml["coneAxis"], ml["coneCutOff"], ml["coneApex"] = axis, cutoff, apex
        ml["lod"] = lod
        ml["vertexTriangleCount"] = PATCH_V | (PATCH_T << 8)
        stride = PATCH_V + PATCH_T
        ml["dataOffset"] = self.ndata + np.arange(M, dtype=np.uint32) * stride
        data = np.empty((M, stride), dtype=np.uint32)
        data[:, :PATCH_V] = self.nverts + np.arange(M, dtype=np.uint32)[:, None] * PATCH_V + np.arange(PATCH_V, dtype=np.uint32)[None, :]
        data[:, PATCH_V:] = PATCH_TRIS[None, :]
        ids = self.nmeshlets + np.arange(M, dtype=np.uint32)
        self.positions.append(pos.reshape(-1, 3))
        self.nverts += M * PATCH_V
        self.meshlets.append(ml)
        self.meshlet_data.append(data.reshape(-1))
        self.ndata += M * stride
        self.nmeshlets += M
        return ids

    def _add_groups(self, member_ids, center, error, parent_center, parent_error):
        """member_ids (G, k) meshlet ids; one group per row."""
        G, k = member_ids.shape
        g = np.zeros(G, dtype=T.MESHLET_GROUP)
        g["clusterPosCenter"] = center
        g["error"] = error
        g["parentPosCenter"] = parent_center
        g["parentError"] = parent_error
        g["meshletOffset"] = self.nindices + np.arange(G, dtype=np.uint32) * k
        g["meshletCount"] = k
        self.groups.append(g)
        self.group_indices.append(member_ids.reshape(-1).astype(np.uint32))
        self.nindices += G * k

    def add_surface(self, S, P, Q, lods=1, error_scale=0.06):
        """S(u, v) -> (..., 3) float64 over [0,1]^2; P x Q LOD0 patches; lods in {1, 2, 3}."""
        if lods > 1:
            assert P % 4 == 0 and Q % 4 == 0, "LOD quadtree needs patch grids in multiples of 4"
        k = np.arange(9) / 8.0
        handedness = 1.0 if self.nsurfaces % 2 == 0 else -1.0
        self.nsurfaces += 1

        def sample(u0, v0, du, dv):
            # u0,v0: (M,) patch origins; du,dv patch extents -> (M,81,3) float32 (row j = v, col i = u)
            U = u0[:, None, None] + du * k[None, None, :]
            V = v0[:, None, None] + dv * k[None, :, None]
            U, V = np.broadcast_arrays(U, V)
            self._last_uv = np.stack([U * self.uv_scale[0], V * self.uv_scale[1]], axis=-1).astype(np.float32).reshape(len(u0), 81, 2)
            if self.attributes:
                self._last_frame = surface_frames(S, U, V, handedness)
            return S(U, V).astype(np.float32).reshape(len(u0), 81, 3)

        pi, pj = np.meshgrid(np.arange(P), np.arange(Q), indexing="xy")     # (Q,P)
        pos0 = sample((pi / P).reshape(-1), (pj / Q).reshape(-1), 1.0 / P, 1.0 / Q)
        ids0 = self._add_meshlets(pos0, 0, self._last_uv).reshape(Q, P)
        edge = float(np.mean(np.linalg.norm(pos0[:, 8].astype(np.float64) - pos0[:, 0].astype(np.float64), axis=1)))
        e1, e2 = error_scale * edge, 2.0 * error_scale * edge

        def block_centers(step):
            # AABB centre of each step x step block of LOD0 patches -> (Q/step, P/step, 3)
            bq, bp = Q // step, P // step
            pm = pos0.reshape(Q, P, 81, 3)
            pm = pm.reshape(bq, step, bp, step, 81, 3)
            mn = pm.min(axis=(1, 3, 4))
            mx = pm.max(axis=(1, 3, 4))
            return (0.5 * (mn.astype(np.float64) + mx.astype(np.float64))).astype(np.float32)

        if lods == 1:
            # un-parented LOD0 groups: runs of up to 4 meshlets in id order (rootSphereGroupMap, nanite_builder.cpp:373-390)
            flat = ids0.reshape(-1)
            n4 = (len(flat) // 4) * 4
            if n4:
                self._add_groups(flat[:n4].reshape(-1, 4), 0.0, -1.0, 0.0, FLT_MAX)
            if len(flat) - n4:
                self._add_groups(flat[n4:].reshape(1, -1), 0.0, -1.0, 0.0, FLT_MAX)
            return

        c1 = block_centers(2)                                                 # (Q/2, P/2, 3)
        blk0 = ids0.reshape(Q // 2, 2, P // 2, 2).transpose(0, 2, 1, 3).reshape(-1, 4)
        self._add_groups(blk0, 0.0, -1.0, c1.reshape(-1, 3), e1)

        # LOD1: two meshlets per 2x2 block, each spanning half the block in u
        bi, bj = np.meshgrid(np.arange(P // 2), np.arange(Q // 2), indexing="xy")
        u0 = np.stack([bi * 2 / P, bi * 2 / P + 1.0 / P], axis=-1).reshape(-1)
        v0 = np.repeat((bj * 2 / Q).reshape(-1), 2)
        pos1 = sample(u0, v0, 1.0 / P, 2.0 / Q)
        ids1 = self._add_meshlets(pos1, 1, self._last_uv).reshape(Q // 2, P // 2, 2)
        if lods == 2:
            self._add_groups(ids1.reshape(-1, 2), c1.reshape(-1, 3), e1, 0.0, FLT_MAX)
            return
        c2 = block_centers(4)                                                 # (Q/4, P/4, 3)
        c2_for_b1 = np.repeat(np.repeat(c2, 2, axis=0), 2, axis=1)
        self._add_groups(ids1.reshape(-1, 2), c1.reshape(-1, 3), e1, c2_for_b1.reshape(-1, 3), e2)

        # LOD2: four meshlets per 4x4 block, each spanning a 2x2-patch quadrant
        qi, qj = np.meshgrid(np.arange(P // 2), np.arange(Q // 2), indexing="xy")
        pos2 = sample((qi * 2 / P).reshape(-1), (qj * 2 / Q).reshape(-1), 2.0 / P, 2.0 / Q)
        ids2 = self._add_meshlets(pos2, 2, self._last_uv).reshape(Q // 2, P // 2)
        blk2 = ids2.reshape(Q // 4, 2, P // 4, 2).transpose(0, 2, 1, 3).reshape(-1, 4)
        self._add_groups(blk2, c2.reshape(-1, 3), e2, 0.0, FLT_MAX)

    def finish(self):
        pos = np.concatenate(self.positions) if self.positions else np.zeros((0, 3), np.float32)
        groups, nodes = build_bvh(np.concatenate(self.groups))
        self.groups = [groups]
        return dict(
            bvh_nodes=nodes,
            positions=pos,
            texcoords=np.concatenate(self.texcoords) if self.texcoords else np.zeros((0, 2), np.float32),
            normals=np.concatenate(self.normals) if self.attributes else None,
            tangents=np.concatenate(self.tangents) if self.attributes else None,
            meshlets=np.concatenate(self.meshlets),
            meshlet_data=np.concatenate(self.meshlet_data),
            groups=np.concatenate(self.groups),
            group_indices=np.concatenate(self.group_indices),
        )


def surface_frames(S, U, V, handedness=1.0, h=1e-5):
    """Normals and tangents of the surface S at the parameters (U, V): the partials dS/du and dS/dv by float64 central differences
    of the surface function, n = normalize(dS/du x dS/dv), t = (normalize(dS/du), handedness).  Returns float32 (..., 3) and
    (..., 4)."""
    su = (S(U + h, V) - S(U - h, V)) / (2.0 * h)
    sv = (S(U, V + h) - S(U, V - h)) / (2.0 * h)
    n = np.cross(su, sv)
    n = n / np.linalg.norm(n, axis=-1, keepdims=True)
    t = su / np.linalg.norm(su, axis=-1, keepdims=True)
    return _unit32(n), np.concatenate([_unit32(t), np.full(t.shape[:-1] + (1,), handedness, np.float32)], axis=-1)


def _unit32(v):
    """float64 unit vectors -> float32: divided by the length of their float32 rounding, then rounded (|v| = 1 to float32 rounding)"""
    v = np.asarray(v, dtype=np.float64)
    v32 = v.astype(np.float32)
    l = np.sqrt((v32.astype(np.float64) ** 2).sum(axis=-1, keepdims=True))
    return (v / l).astype(np.float32)


def mesh_attributes(positions, indices, texcoord0=None):
    """Smooth normals and tangents of an indexed triangle mesh, in float64: normals = normalized area-weighted face normals; tangents
    = the area-weighted dP/du of the texture coordinates (u along +x of the mesh when there are none), made orthogonal to the normal
    and normalised, w = the sign of dot(cross(n, t), dP/dv).  A vertex with no usable direction gets a tangent perpendicular to n."""
    p = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    tri = np.asarray(indices, dtype=np.int64).reshape(-1, 3)
    e1, e2 = p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]]
    fn = np.cross(e1, e2)                                       # |fn| = 2 x area: the area weight
    n = np.zeros_like(p)
    for k in range(3):
        np.add.at(n, tri[:, k], fn)
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)
    tu, tv = np.zeros_like(p), np.zeros_like(p)
    if texcoord0 is not None:
        uv = np.asarray(texcoord0, dtype=np.float64).reshape(-1, 2)
        d1, d2 = uv[tri[:, 1]] - uv[tri[:, 0]], uv[tri[:, 2]] - uv[tri[:, 0]]
        d1 = d1 - np.round(d1); d2 = d2 - np.round(d2)            # (wrapped coordinates: the seam of a closed surface)
        det = d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1]
        ok = np.abs(det) > 1e-12
        r = np.where(ok, 1.0 / np.where(ok, det, 1.0), 0.0)[:, None]
        area = 0.5 * np.linalg.norm(fn, axis=1)[:, None]
        fu = (e1 * d2[:, 1:2] - e2 * d1[:, 1:2]) * r
        fv = (e2 * d1[:, 0:1] - e1 * d2[:, 0:1]) * r
        fu *= area / np.maximum(np.linalg.norm(fu, axis=1, keepdims=True), 1e-300)
        fv *= area / np.maximum(np.linalg.norm(fv, axis=1, keepdims=True), 1e-300)
        for k in range(3):
            np.add.at(tu, tri[:, k], fu)
            np.add.at(tv, tri[:, k], fv)
    else:
        tu[:] = (1.0, 0.0, 0.0)
    t = tu - (tu * n).sum(axis=1, keepdims=True) * n
    bad = np.linalg.norm(t, axis=1) < 1e-9
    alt = np.cross(n, np.where(np.abs(n[:, 1:2]) < 0.9, (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)))
    t = np.where(bad[:, None], alt, t)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    w = np.where((np.cross(n, t) * tv).sum(axis=1) < 0.0, -1.0, 1.0)
    return _unit32(n), np.concatenate([_unit32(t), w[:, None].astype(np.float32)], axis=1)


def build_bvh(groups):
    """The 8-wide tree over the parented cluster groups of one primitive, shaped like the reference's buildBVHTree /
    buildBVH / flattenBVH (nanite_builder.cpp:77-416): un-parented groups are the root's leaves; the others are split
    2 x 2 x 2 by sorting on the longest axis of the union of their parent-error boxes until fewer than 8 remain; nodes are
    flattened breadth first and the groups re-ordered as the nodes list them.  Returns (groups in tree order, nodes)."""
    groups = np.asarray(groups, dtype=T.MESHLET_GROUP)
    parented = np.nonzero(groups["parentError"] < 3.0e38)[0]
    roots = np.nonzero(groups["parentError"] >= 3.0e38)[0]
    pc = groups["parentPosCenter"].astype(np.float32)
    pe = groups["parentError"].astype(np.float32)

    def bounds(ids):
        if len(ids) == 0:
            return np.zeros(3, np.float32), np.zeros(3, np.float32)
        return (pc[ids] - pe[ids, None]).min(axis=0), (pc[ids] + pe[ids, None]).max(axis=0)

    def longest(mn, mx):
        d = mx - mn
        a = 0
        if d[1] >= d[0] and d[1] >= d[2]:
            a = 1
        if d[2] >= d[0] and d[2] >= d[1]:
            a = 2
        return a

    def halves(ids, mn, mx):
        order = ids[np.argsort(pc[ids, longest(mn, mx)], kind="stable")]
        n = len(order)
        return [order[i * n // 2:(i + 1) * n // 2] for i in range(2)]

    class Node:
        pass
    root = Node()
    root.mn, root.mx = bounds(parented)
    root.leaves, root.children, root.depth, root.todo = list(roots), [None] * 8, 0, parented
    queue, order = [root], []
    while queue:
        nd = queue.pop(0)
        order.append(nd)
        ids = nd.todo
        if len(ids) == 0:
            continue
        if len(ids) < 8 or nd.depth == 13:                       # kNaniteBVHLevelNodeCount / kNaniteMaxBVHLevelCount - 1
            nd.leaves = nd.leaves + list(ids)
            continue
        for i, h0 in enumerate(halves(ids, nd.mn, nd.mx)):
            for j, h1 in enumerate(halves(h0, *bounds(h0))):
                for k, h2 in enumerate(halves(h1, *bounds(h1))):
                    ch = Node()
                    ch.mn, ch.mx = bounds(h2)
                    ch.leaves, ch.children, ch.depth, ch.todo = [], [None] * 8, nd.depth + 1, h2
                    nd.children[(i * 2 + j) * 2 + k] = ch
                    queue.append(ch)
    # breadth-first flatten (the queue above already visits in that order)
    for i, nd in enumerate(order):
        nd.index = i
    nodes = np.zeros(len(order), dtype=T.BVH_NODE)
    new_order = []
    for nd in order:
        n = nodes[nd.index]
        n["sphere"][:3] = 0.5 * (nd.mx + nd.mn)
        n["sphere"][3] = 0.5 * np.float32(np.linalg.norm((nd.mx - nd.mn).astype(np.float32)))
        n["children"] = [c.index if c is not None else 0xFFFFFFFF for c in nd.children]
        n["leafMeshletGroupOffset"], n["leafMeshletGroupCount"] = len(new_order), len(nd.leaves)
        new_order += nd.leaves
    for nd in reversed(order):
        nodes[nd.index]["bvhNodeCount"] = 1 + sum(int(nodes[c.index]["bvhNodeCount"]) for c in nd.children if c is not None)
    assert sorted(new_order) == list(range(len(groups))) and nodes[0]["bvhNodeCount"] == len(nodes)
    return groups[np.array(new_order, dtype=np.int64)], nodes


class SceneBuilder:
    def __init__(self, name, attributes=False):
        self.name = name
        self.attributes = attributes      # normals and tangents in the scene (every primitive's PrimitiveBuilder makes them)
        self.prims = []
        self.materials = [self._material(0)]
        self.obj_prim = []
        self.obj_mat = []
        self.obj_l2w = []
        self.textures = []
        self.samplers = []

    @staticmethod
    def _material(two_sided, alpha_mode=0, texture=0xFFFFFFFF, sampler=0, cutoff=0.5, alpha_factor=1.0):
        m = np.zeros(1, dtype=T.MATERIAL)
        m["bTwoSided"] = two_sided
        m["baseColorFactor"] = 1.0
        m["baseColorFactor"][0, 3] = alpha_factor
        m["alphaMode"], m["alphaCutOff"] = alpha_mode, cutoff
        m["baseColorId"], m["baseColorSampler"] = texture, sampler
        m["materialType"] = 1
        return m

    def add_material(self, two_sided, alpha_mode=0, texture=0xFFFFFFFF, sampler=0, cutoff=0.5, alpha_factor=1.0, *, pbr=False,
                     base_color_factor=None, emissive=None, emissive_factor=None, normal=None, normal_scale=None,
                     metallic_roughness=None, metallic_factor=None, roughness_factor=None, occlusion_strength=None, material_type=None):
        """The keyword-only arguments fill the further slots of loadGLTFMetallicRoughnessPBRMaterial (material.hlsli:66-153):
        emissive / normal / metallic_roughness = (texture, sampler); occlusion_strength not None sets bExistOcclusion.  pbr=True
        makes the slots that are not given name NO texture (0xFFFFFFFF); without it they keep the 0 this builder has always
        written (texture 0 of a scene that has textures)."""
        m = self._material(two_sided, alpha_mode, texture, sampler, cutoff, alpha_factor)
        for field, smp, pair in (("emissiveTexture", "emissiveSampler", emissive), ("normalTexture", "normalSampler", normal),
                                 ("metallicRoughnessTexture", "metallicRoughnessSampler", metallic_roughness)):
            if pair is not None:
                m[field], m[smp] = pair
            elif pbr:
                m[field] = 0xFFFFFFFF
        if base_color_factor is not None:
            m["baseColorFactor"][0, :3] = base_color_factor
        for field, val in (("emissiveFactor", emissive_factor), ("normalFactorScale", normal_scale), ("metallicFactor", metallic_factor),
                           ("roughnessFactor", roughness_factor), ("materialType", material_type)):
            if val is not None:
                m[field] = val
        if occlusion_strength is not None:
            m["bExistOcclusion"], m["occlusionTextureStrength"] = 1, occlusion_strength
        self.materials.append(m)
        return len(self.materials) - 1

    def add_texture(self, rgba8):
        self.textures.append(np.ascontiguousarray(rgba8, dtype=np.uint8))
        return len(self.textures) - 1

    def add_sampler(self, min_filter=T.FILTER_LINEAR_MIPMAP_LINEAR, mag_filter=T.FILTER_LINEAR, wrap_s=T.WRAP_REPEAT, wrap_t=T.WRAP_REPEAT):
        self.samplers.append((min_filter, mag_filter, wrap_s, wrap_t))
        return len(self.samplers) - 1

    def add_primitive(self, builder):
        self.prims.append(builder.finish())
        return len(self.prims) - 1

    def add_object(self, prim, l2w=None, material=0):
        self.obj_prim.append(prim)
        self.obj_mat.append(material)
        self.obj_l2w.append(np.eye(4) if l2w is None else np.asarray(l2w, dtype=np.float64))
        return len(self.obj_prim) - 1

    def build(self):
        prims = np.zeros(len(self.prims), dtype=T.PRIMITIVE)
        pos, ml, md, gr, gi, uv, bv, nrm, tng = [], [], [], [], [], [], [], [], []
        nv = nm = nd = ng = ni = nb = 0
        for i, p in enumerate(self.prims):
            prims[i]["posMin"] = p["positions"].min(axis=0)
            prims[i]["posMax"] = p["positions"].max(axis=0)
            prims[i]["posAverage"] = p["positions"].mean(axis=0)
            prims[i]["vertexOffset"], prims[i]["vertexCount"] = nv, len(p["positions"])
            prims[i]["meshletOffset"] = nm
            prims[i]["meshletGroupOffset"], prims[i]["meshletGroupCount"] = ng, len(p["groups"])
            prims[i]["meshletGroupIndicesOffset"] = ni
            prims[i]["bvhNodeOffset"] = nb
            bv.append(p["bvh_nodes"]); nb += len(p["bvh_nodes"])
            m = p["meshlets"].copy()
            m["dataOffset"] += nd
            uv.append(p["texcoords"]); pos.append(p["positions"]); ml.append(m); md.append(p["meshlet_data"]); gr.append(p["groups"]); gi.append(p["group_indices"])
            if self.attributes:
                assert p["normals"] is not None, "SceneBuilder(attributes=True): every primitive needs PrimitiveBuilder(attributes=True)"
                nrm.append(p["normals"]); tng.append(p["tangents"])
            nv += len(p["positions"]); nm += len(m); nd += len(p["meshlet_data"]); ng += len(p["groups"]); ni += len(p["group_indices"])
        objects = np.zeros(len(self.obj_prim), dtype=T.OBJECT)
        objects["GLTFPrimitiveDetail"] = np.array(self.obj_prim, dtype=np.uint32)
        objects["GLTFMaterialData"] = np.array(self.obj_mat, dtype=np.uint32)
        scene = T.Scene(objects, prims, np.concatenate(self.materials), np.concatenate(ml), np.concatenate(gr),
                        np.concatenate(gi), np.concatenate(md), np.concatenate(pos), name=self.name,
                        texcoord0=np.concatenate(uv) if (self.textures and uv) else None, textures=self.textures,
                        samplers=np.array(self.samplers, dtype=T.SAMPLER) if self.samplers else None,
                        bvh_nodes=np.concatenate(bv) if bv else None,
                        normals=np.concatenate(nrm) if self.attributes else None, tangents=np.concatenate(tng) if self.attributes else None)
        # glm column-major doubles
        scene.local_to_world = np.ascontiguousarray(np.stack([m.T.reshape(16) for m in self.obj_l2w]), dtype=np.float64)
        return scene


def translate(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def rotate_y(a):
    c, s = math.cos(a), math.sin(a)
    m = np.eye(4)
    m[0, 0], m[0, 2], m[2, 0], m[2, 2] = c, s, -s, c
    return m


def scale(sx, sy=None, sz=None):
    sy = sx if sy is None else sy
    sz = sx if sz is None else sz
    return np.diag([sx, sy, sz, 1.0])


# --------------------------------------------------------------------------------- surfaces ---

def _bumps(seed, amp, freq):
    """Smooth deterministic displacement field d(a, b) (sum of 4 sinusoids)."""
    ph = rand01(seed, np.arange(12))
    ths = ph[0:4] * 2 * math.pi
    fs = freq * (0.6 + 1.4 * ph[4:8])
    ps = ph[8:12] * 2 * math.pi

    def d(a, b):
        r = 0.0
        for k in range(4):
            r = r + np.sin(fs[k] * (a * math.cos(ths[k]) + b * math.sin(ths[k])) + ps[k])
        return amp * 0.25 * r
    return d


def plane_surface(origin, du, dv, seed=0, amp=0.0, freq=1.0):
    """S(u,v) = origin + u*du + v*dv + n*d(u,v); normal n = normalize(du x dv)."""
    origin, du, dv = (np.asarray(x, dtype=np.float64) for x in (origin, du, dv))
    n = np.cross(du, dv)
    n = n / np.linalg.norm(n)
    lu, lv = np.linalg.norm(du), np.linalg.norm(dv)
    d = _bumps(seed, amp, freq)

    def S(U, V):
        h = d(U * lu, V * lv) if amp else 0.0
        return origin + U[..., None] * du + V[..., None] * dv + (np.zeros_like(U) + h)[..., None] * n
    return S


def cylinder_surface(base, radius, height, seed=0, amp=0.0):
    """Outward-facing cylinder wall around +y; u = angle, v = height."""
    base = np.asarray(base, dtype=np.float64)
    d = _bumps(seed, amp, 3.0)

    def S(U, V):
        ang = -U * 2 * math.pi                    # dS/du x dS/dv points outward
        r = radius + (d(U * 2 * math.pi * radius, V * height) if amp else 0.0)
        return base + np.stack([r * np.cos(ang), V * height, r * np.sin(ang)], axis=-1)
    return S


# ------------------------------------------------------------------------------------ camera ---

class Camera:
    def __init__(self, position, front, width, height, fovy=math.radians(45.0), z_near=0.001, z_far=20000.0,
                 world_up=(0.0, 1.0, 0.0), jitter=(0.0, 0.0)):
        self.position = tuple(float(x) for x in position)
        self.front = tuple(float(x) for x in front)
        self.world_up = world_up
        self.width, self.height = int(width), int(height)
        self.fovy, self.z_near, self.z_far = float(fovy), float(z_near), float(z_far)
        self.jitter = jitter

    def moved(self, delta):
        c = Camera(tuple(p + d for p, d in zip(self.position, delta)), self.front, self.width, self.height,
                   self.fovy, self.z_near, self.z_far, self.world_up, self.jitter)
        return c


# ------------------------------------------------------------------------------------ configs ---

def config1_single_meshlet():
    """BASELINE config 1: one 128-triangle meshlet, 256x256, fixed camera."""
    i = np.arange(81)
    z = ((pcg32(1, i) & 0xFFFF).astype(np.float64) / 65535.0 - 0.5) * 0.2

    def S(U, V):
        # exact lattice: look the height up by vertex index
        ii = np.rint(U * 8).astype(np.int64)
        jj = np.rint(V * 8).astype(np.int64)
        return np.stack([U * 2 - 1, V * 2 - 1, z[jj * 9 + ii]], axis=-1)

    pb = PrimitiveBuilder()
    pb.add_surface(S, 1, 1, lods=1)
    sb = SceneBuilder("config1_single_meshlet")
    sb.add_object(sb.add_primitive(pb))
    cam = Camera((0.0, 0.0, 3.0), (0.0, 0.0, -1.0), 256, 256)
    return sb.build(), cam


def config2_atrium(width=1920, height=1080):
    """BASELINE config 2 (Sponza-class): 2048 patches = 262 144 triangles, 22 objects, single LOD."""
    sb = SceneBuilder("config2_atrium")
    L, Wd, Hh = 32.0, 16.0, 8.0
    seed = 2000

    def obj(S, P, Q):
        nonlocal seed
        pb = PrimitiveBuilder()
        pb.add_surface(S, P, Q, lods=1)
        sb.add_object(sb.add_primitive(pb))
        seed += 1

    # floor (normal +y), ceiling (normal -y)
    obj(plane_surface((-L / 2, 0, Wd / 2), (L, 0, 0), (0, 0, -Wd), seed, 0.03, 2.0), 32, 16)
    obj(plane_surface((-L / 2, Hh, -Wd / 2), (L, 0, 0), (0, 0, Wd), seed, 0.05, 1.0), 32, 8)
    # long walls (normals facing inward)
    obj(plane_surface((-L / 2, 0, -Wd / 2), (L, 0, 0), (0, Hh, 0), seed, 0.04, 1.5), 32, 8)
    obj(plane_surface((L / 2, 0, Wd / 2), (-L, 0, 0), (0, Hh, 0), seed, 0.04, 1.5), 32, 8)
    # end walls
    obj(plane_surface((-L / 2, 0, Wd / 2), (0, 0, -Wd), (0, Hh, 0), seed, 0.04, 1.5), 16, 8)
    obj(plane_surface((L / 2, 0, -Wd / 2), (0, 0, Wd), (0, Hh, 0), seed, 0.04, 1.5), 16, 8)
    # two colonnades of 8 columns
    for side in (-1, 1):
        for k in range(8):
            x = -L / 2 + 2.0 + k * 4.0
            obj(cylinder_surface((x, 0.0, side * 4.0), 0.45, Hh, seed, 0.02), 4, 8)
    cam = Camera((-L / 2 + 1.0, 1.7, 0.3), (1.0, -0.02, -0.01), width, height)
    return sb.build(), cam


def _building(pb, w, d, h, seed, lods):
    # 4 sides + roof, each 8x8 patches, normals outward
    pb.add_surface(plane_surface((-w / 2, 0, d / 2), (w, 0, 0), (0, h, 0), seed + 0, 0.15, 0.8), 8, 8, lods)      # +z face
    pb.add_surface(plane_surface((w / 2, 0, d / 2), (0, 0, -d), (0, h, 0), seed + 1, 0.15, 0.8), 8, 8, lods)     # +x face
    pb.add_surface(plane_surface((w / 2, 0, -d / 2), (-w, 0, 0), (0, h, 0), seed + 2, 0.15, 0.8), 8, 8, lods)    # -z face
    pb.add_surface(plane_surface((-w / 2, 0, -d / 2), (0, 0, d), (0, h, 0), seed + 3, 0.15, 0.8), 8, 8, lods)    # -x face
    pb.add_surface(plane_surface((-w / 2, h, d / 2), (w, 0, 0), (0, 0, -d), seed + 4, 0.10, 0.5), 8, 8, lods)    # roof


def _street_primitives(sb, lods=3, uv_tiles=None):
    """Unique geometry of one 'street' block: ground + 40 buildings + 311 props. Returns [(prim, l2w)].
    uv_tiles: (buildings, props) texture repeats per surface for the masked variant (texture coordinates are generated either way)."""
    out = []
    pb = PrimitiveBuilder(sb.attributes)
    pb.add_surface(plane_surface((-64, 0, 64), (128, 0, 0), (0, 0, -128), 3000, 0.08, 0.9), 64, 64, lods)
    out.append((sb.add_primitive(pb), np.eye(4)))
    # 4 rows x 10 buildings along x; rows at z = -34, -14 | +14, +34 (street down the middle)
    b = 0
    for row, z in enumerate((-36.0, -15.0, 15.0, 36.0)):
        for k in range(10):
            r = rand01(3100, np.arange(b * 4, b * 4 + 4))
            w, d, h = 9.0 + 2.0 * r[0], 9.0 + 2.0 * r[1], 10.0 + 14.0 * r[2]
            pb = PrimitiveBuilder(sb.attributes)
            if uv_tiles:
                pb.uv_scale = (uv_tiles[0], uv_tiles[0])
            _building(pb, w, d, h, 3200 + b * 8, lods)
            x = -58.0 + k * 12.8 + (r[3] - 0.5)
            out.append((sb.add_primitive(pb), translate(x, 0.0, z) @ rotate_y((r[3] - 0.5) * 0.2)))
            b += 1
    # 311 props (lamp posts / bollards / planters): 4x4-patch cylinders scattered over the street and sidewalks
    for p in range(311):
        r = rand01(3900, np.arange(p * 5, p * 5 + 5))
        rad, hgt = 0.15 + 0.5 * r[0], 0.8 + 3.5 * r[1]
        pb = PrimitiveBuilder(sb.attributes)
        if uv_tiles:
            pb.uv_scale = (uv_tiles[1], uv_tiles[1])
        pb.add_surface(cylinder_surface((0, 0, 0), rad, hgt, 4000 + p, 0.02), 4, 4, lods)
        x, z = -60.0 + 120.0 * r[2], -8.0 + 16.0 * r[3]
        out.append((sb.add_primitive(pb), translate(x, 0.0, z)))
    return out


def config3_street(width=3840, height=2160, lods=3, masked=False, attributes=False, materials=False):
    """BASELINE config 3 (Bistro-class): 21 872 LOD0 patches = 2 799 616 triangles, 352 objects, 3 LOD levels.
    masked: the SAME geometry with alpha-tested materials (mesh_raster.hlsl:34-38,107-112,198-204) on every prop and every other
    building -- two-sided foliage-style cut-outs (a noise and a disc texture, trilinear / nearest samplers): the workload of
    bench.py --workload street_4k_masked, triangle for triangle the opaque scene.
    attributes: with per-vertex normals and tangents (PrimitiveBuilder); the geometry is the same.
    materials: the opaque geometry under the textured materials of the material resolve (_pbr_materials, cycled over the objects),
    with normals, tangents and the masked variant's texture tiling: the workload of tools/resolve_time.py's material sets."""
    assert not (masked and materials)
    sb = SceneBuilder("config3_street" + ("_masked" if masked else "_materials" if materials else ""), attributes or materials)
    mats = [0]
    if materials:
        pm = _pbr_materials(sb, 11)
        for k, (prim, l2w) in enumerate(_street_primitives(sb, lods, uv_tiles=(6.0, 3.0))):
            sb.add_object(prim, l2w, material=pm[k % len(pm)])
        return sb.build(), Camera((-62.0, 12.0, 3.0), (1.0, -0.18, -0.04), width, height)
    if masked:
        tex = [sb.add_texture(t) for t in _alpha_textures(11)]
        smp = [sb.add_sampler(T.FILTER_LINEAR_MIPMAP_LINEAR, T.FILTER_LINEAR, T.WRAP_REPEAT, T.WRAP_REPEAT),
               sb.add_sampler(T.FILTER_NEAREST, T.FILTER_NEAREST, T.WRAP_REPEAT, T.WRAP_MIRRORED_REPEAT)]
        # masked == "twin": the same two-sided materials WITHOUT the alpha test -- the opaque frame of equal triangle count the
        # masked frame is measured against (two-sided materials skip the cone cull, so the plain scene submits fewer clusters)
        mode = T.ALPHA_MASK if masked != "twin" else 0
        mats = [sb.add_material(1, mode, tex[1], smp[0], 0.35, 1.0),    # noise: ~2/3 of the surface survives
                sb.add_material(1, mode, tex[2], smp[1], 0.30, 1.0),    # discs
                sb.add_material(1, mode, tex[0], smp[0], 0.5, 1.0)]     # checker
    for k, (prim, l2w) in enumerate(_street_primitives(sb, lods, uv_tiles=(6.0, 3.0) if masked else None)):
        # object 0: the ground (opaque); 1..40: buildings (every other one masked); 41..: props (all masked)
        m = 0 if (not masked or k == 0 or (k <= 40 and k % 2 == 0)) else mats[k % len(mats)]
        sb.add_object(prim, l2w, material=m)
    # second-floor view down the street: ~8.9k clusters pass LOD/frustum/cone culling, ~3.8k survive the
    # two-pass HZB test (~0.49 M triangles submitted, ~11.7 M fragments at 4K)
    cam = Camera((-62.0, 12.0, 3.0), (1.0, -0.18, -0.04), width, height)
    return sb.build(), cam


def config4_street_x64(width=3840, height=2160, grid=8, lods=3):
    """BASELINE config 4: config 3 instanced on a grid x grid lattice (shared geometry), ~179 M triangles at 8x8."""
    sb = SceneBuilder("config4_street_x%d" % (grid * grid))
    prims = _street_primitives(sb, lods)
    pitch = 132.0
    for gz in range(grid):
        for gx in range(grid):
            off = translate((gx - (grid - 1) / 2) * pitch, 0.0, (gz - (grid - 1) / 2) * pitch)
            for prim, l2w in prims:
                sb.add_object(prim, off @ l2w)
    half = (grid - 1) / 2 * pitch
    cam = Camera((-half - 60.0, 45.0, -half - 20.0), (1.0, -0.28, 0.75), width, height)
    return sb.build(), cam


def small_test_scene(width=160, height=96, lods=3, seed=7, two_sided_every=3, attributes=False):
    """A small multi-object scene with LODs for parity tests (a few hundred meshlets).  attributes: with normals and tangents."""
    sb = SceneBuilder("small_test_scene", attributes)
    two = sb.add_material(1)
    pb = PrimitiveBuilder(sb.attributes)
    pb.add_surface(plane_surface((-8, 0, 8), (16, 0, 0), (0, 0, -16), seed, 0.2, 0.7), 8, 8, lods)
    sb.add_object(sb.add_primitive(pb))
    for k in range(6):
        r = rand01(seed + 1, np.arange(k * 4, k * 4 + 4))
        pb = PrimitiveBuilder(sb.attributes)
        if k % 2 == 0:
            _building(pb, 1.5 + r[0], 1.5 + r[1], 1.0 + 2.5 * r[2], seed * 100 + k * 8, min(lods, 3))
        else:
            pb.add_surface(cylinder_surface((0, 0, 0), 0.3 + 0.4 * r[0], 1.0 + 2.0 * r[1], seed * 100 + k, 0.03), 4, 4, lods)
        prim = sb.add_primitive(pb)
        m = translate(-5.0 + 10.0 * r[2], 0.0, -5.0 + 10.0 * r[3]) @ rotate_y(r[0] * 3.0) @ scale(1.0 + 0.5 * r[1])
        sb.add_object(prim, m, material=two if (k % two_sided_every == 1) else 0)
        if k == 2:      # an instanced copy
            sb.add_object(prim, translate(3.0, 0.0, 4.0) @ m)
    cam = Camera((-7.0, 1.6, 6.5), (0.8, -0.12, -0.6), width, height)
    return sb.build(), cam


def group_count_scene(groups, width=320, height=180, shown=48, seed=1, panels=True):
    """Exactly `groups` group instances (Scene.group_instances), for the cull paths chosen by the group-instance count: objects of a
    one-group tile (2 x 2 patches, four meshlets: every lane of a quad) and, past 256 groups and unless `panels` is False, of a
    64-group panel (16 x 16 patches) ahead of them.  At most `shown` objects, spread over the whole object order (first and last included), stand in three
    staggered layers of 8 x 4 unit squares in front of the camera, each layer a wall that hides most of the next; the others are
    behind the camera (culled by the object test)."""
    sb = SceneBuilder("group_count_%d" % groups)
    pb = PrimitiveBuilder()
    pb.add_surface(plane_surface((-0.5, -0.5, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), seed, 0.05, 2.0), 16, 16, 1)
    panel = sb.add_primitive(pb)
    pb = PrimitiveBuilder()
    pb.add_surface(plane_surface((-0.5, -0.5, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), seed + 1, 0.08, 1.5), 2, 2, 1)
    tile = sb.add_primitive(pb)
    prims = [panel] * (groups // 64) + [tile] * (groups % 64) if groups > 256 and panels else [tile] * groups
    n = len(prims)
    picked = set(np.linspace(0, n - 1, min(n, shown)).round().astype(np.int64).tolist()) if n else set()
    j = 0
    for k, prim in enumerate(prims):
        if k in picked:
            col, row, layer = j % 8, (j // 8) % 4, (j // 32) % 3
            r = rand01(seed + 7, np.arange(3 * j, 3 * j + 3))
            m = translate(col - 3.5 + 0.5 * layer, row - 1.5 + 0.3 * layer, -1.2 * layer - 0.2 * r[0]) @ rotate_y((r[1] - 0.5) * 0.4)
            j += 1
        else:
            m = translate((k % 37) * 0.5, (k % 11) * 0.5, 40.0 + (k % 5))
        sb.add_object(prim, m)
    scene = sb.build()
    assert scene.group_instances == groups
    return scene, Camera((0.0, 0.0, 6.0), (0.0, 0.0, -1.0), width, height)


def _alpha_textures(seed):
    """Three procedural RGBA8 textures whose alpha the masked materials test: a checker, an odd-sized noise, a disc."""
    yy, xx = np.mgrid[0:64, 0:64]
    checker = np.where(((xx // 8) + (yy // 8)) % 2 == 0, 255, 0).astype(np.uint8)
    noise = (pcg_hash(np.arange(37 * 21, dtype=np.uint32) + np.uint32(seed * 7919)) & 0xFF).astype(np.uint8).reshape(21, 37)
    yy, xx = np.mgrid[0:16, 0:16]
    disc = np.clip(255.0 - 40.0 * np.hypot(xx - 7.5, yy - 7.5), 0, 255).astype(np.uint8)
    out = []
    for a in (checker, noise, disc):
        img = np.zeros(a.shape + (4,), np.uint8)
        img[..., 0:3] = 200
        img[..., 3] = a
        out.append(img)
    return out


def _masked_layout(sb, mats, lods, seed, position, front, width, height, ground=0, screen=None, behind=0, ground_uv=None, screen_scale=1.0):
    """The geometry of masked_test_scene: a ground, eight buildings / cylinders with tiled (also negative) texture coordinates and
    material mats[k % len(mats)], two copies behind masked ones, a screen right in front of the camera.  ground / screen / behind:
    the materials of those objects (screen None: mats[1])."""
    pb = PrimitiveBuilder(sb.attributes)
    if ground_uv:
        pb.uv_scale = ground_uv
    pb.add_surface(plane_surface((-8, 0, 8), (16, 0, 0), (0, 0, -16), seed, 0.2, 0.7), 8, 8, lods)
    sb.add_object(sb.add_primitive(pb), material=ground)                         # ground (opaque in masked_test_scene)
    for k in range(8):
        r = rand01(seed + 1, np.arange(k * 4, k * 4 + 4))
        pb = PrimitiveBuilder(sb.attributes)
        pb.uv_scale = (1.0 + 3.0 * r[3], 0.5 + 2.5 * r[2]) if k % 3 else (-2.0, 3.0)     # tiling, incl. negative coordinates
        if k % 2 == 0:
            _building(pb, 1.5 + r[0], 1.5 + r[1], 1.0 + 2.5 * r[2], seed * 100 + k * 8, lods)
        else:
            pb.add_surface(cylinder_surface((0, 0, 0), 0.3 + 0.4 * r[0], 1.0 + 2.0 * r[1], seed * 100 + k, 0.03), 4, 4, lods)
        prim = sb.add_primitive(pb)
        m = translate(-5.0 + 10.0 * r[2], 0.0, -5.0 + 10.0 * r[3]) @ rotate_y(r[0] * 3.0) @ scale(1.0 + 0.5 * r[1])
        sb.add_object(prim, m, material=mats[k % len(mats)])
        if k in (1, 4):                                                          # an opaque copy behind a masked one
            sb.add_object(prim, translate(0.6, 0.0, -1.2) @ m, material=behind)
    # a masked screen right in front of the camera: magnified texels, clipped by the near plane at the edges
    pb = PrimitiveBuilder(sb.attributes)
    pb.uv_scale = (3.0, 2.0)
    f = np.array(front, dtype=np.float64) / np.linalg.norm(front)
    side = np.cross(f, (0.0, 1.0, 0.0)); side /= np.linalg.norm(side)
    org = np.array(position) + 0.9 * f - (0.7 * screen_scale) * side - np.array((0.0, 0.45 * screen_scale, 0.0))
    pb.add_surface(plane_surface(tuple(org), tuple((1.4 * screen_scale) * side), (0.0, 0.9 * screen_scale, 0.0), seed + 5, 0.0, 1.0), 4, 4, 1)
    sb.add_object(sb.add_primitive(pb), material=mats[1] if screen is None else screen)
    cam = Camera(position, front, width, height)
    return sb.build(), cam


def masked_test_scene(width=320, height=200, lods=2, seed=3, position=(-6.5, 2.2, 6.0), front=(0.75, -0.22, -0.62), attributes=False):
    """small_test_scene's layout with alpha-tested, blended and white-fallback materials (mesh_raster.hlsl:34-38,107-112,
    198-204; mesh_raster.cpp:224): holes in the masked surfaces show the geometry behind them, blended objects draw
    nothing.  Three textures x three samplers (every wrap mode, nearest and linear, with and without minification).
    attributes: with normals and tangents."""
    sb = SceneBuilder("masked_test_scene", attributes)
    tex = [sb.add_texture(t) for t in _alpha_textures(seed)]
    smp = [sb.add_sampler(T.FILTER_LINEAR_MIPMAP_LINEAR, T.FILTER_LINEAR, T.WRAP_REPEAT, T.WRAP_REPEAT),
           sb.add_sampler(T.FILTER_NEAREST, T.FILTER_NEAREST, T.WRAP_CLAMP_TO_EDGE, T.WRAP_MIRRORED_REPEAT),
           sb.add_sampler(T.FILTER_LINEAR_MIPMAP_NEAREST, T.FILTER_NEAREST, T.WRAP_MIRRORED_REPEAT, T.WRAP_CLAMP_TO_EDGE)]
    mats = [sb.add_material(0, T.ALPHA_MASK, tex[0], smp[0], 0.5, 1.0),        # one-sided checker
            sb.add_material(1, T.ALPHA_MASK, tex[1], smp[1], 0.4, 0.9),        # two-sided noise, nearest, clamp / mirror
            sb.add_material(1, T.ALPHA_MASK, tex[2], smp[2], 0.35, 1.0),       # two-sided disc, mirrored / clamp
            sb.add_material(0, T.ALPHA_BLEND),                                  # blended: draws nothing
            sb.add_material(0, T.ALPHA_MASK, 0xFFFFFFFF, 99, 0.5, 1.0),        # no texture: white fallback, opaque in effect
            sb.add_material(1, T.ALPHA_MASK, tex[0], smp[0], 0.5, 0.4)]        # alpha factor below the cut-off: nothing survives
    return _masked_layout(sb, mats, lods, seed, position, front, width, height)


def _pbr_textures(seed):
    """Procedural RGBA8 textures of the material resolve: [0] a coloured brick albedo 64 x 64 with a checker in alpha, [1] an
    odd-sized (37 x 21) colour noise, [2] a tangent-space normal map 64 x 32 with visible relief (round bumps, z reconstructed by
    the consumer), [3] an occlusion (R) / roughness (G) / metallic (B) map 8 x 64 whose last levels are one texel wide, [4] an
    emissive map 16 x 16 of coloured discs."""
    yy, xx = np.mgrid[0:64, 0:64]
    brick = ((xx + 16 * ((yy // 8) % 2)) % 32 < 30) & (yy % 8 < 7)
    albedo = np.zeros((64, 64, 4), np.uint8)
    albedo[..., 0] = np.where(brick, 150 + (xx * 3 + yy) % 90, 60)
    albedo[..., 1] = np.where(brick, 60 + (yy * 2) % 50, 58)
    albedo[..., 2] = np.where(brick, 40 + (xx ^ yy) % 40, 55)
    albedo[..., 3] = np.where(((xx // 8) + (yy // 8)) % 2 == 0, 255, 90)
    h = pcg_hash(np.arange(37 * 21 * 4, dtype=np.uint32) + np.uint32(seed * 7919))
    noise = (h & 0xFF).astype(np.uint8).reshape(21, 37, 4)
    yy, xx = np.mgrid[0:32, 0:64]
    # height = a lattice of round bumps; the map stores the unit normal's xy, remapped to [0, 255]
    hx = 0.9 * np.sin(xx * (2.0 * np.pi / 16.0)) * (0.6 + 0.4 * np.cos(yy * (2.0 * np.pi / 16.0)))
    hy = 0.9 * np.sin(yy * (2.0 * np.pi / 16.0)) * (0.6 + 0.4 * np.cos(xx * (2.0 * np.pi / 16.0)))
    ln = np.sqrt(hx * hx + hy * hy + 1.0)
    nmap = np.zeros((32, 64, 4), np.uint8)
    nmap[..., 0] = np.round((hx / ln * 0.5 + 0.5) * 255.0)
    nmap[..., 1] = np.round((hy / ln * 0.5 + 0.5) * 255.0)
    nmap[..., 2] = np.round((1.0 / ln * 0.5 + 0.5) * 255.0)
    nmap[..., 3] = 255
    yy, xx = np.mgrid[0:64, 0:8]
    orm = np.zeros((64, 8, 4), np.uint8)
    orm[..., 0] = 120 + (yy * 2) % 130
    orm[..., 1] = 30 + (xx * 28 + yy * 3) % 220
    orm[..., 2] = np.where((yy // 8) % 2 == 0, 230, 20)
    orm[..., 3] = 255
    yy, xx = np.mgrid[0:16, 0:16]
    d = np.clip(1.0 - np.hypot(xx % 8 - 3.5, yy % 8 - 3.5) / 4.0, 0.0, 1.0)
    emis = np.zeros((16, 16, 4), np.uint8)
    emis[..., 0] = np.round(255.0 * d)
    emis[..., 1] = np.round(180.0 * d * ((xx // 8) % 2))
    emis[..., 2] = np.round(255.0 * d * ((yy // 8) % 2))
    emis[..., 3] = 255
    return [albedo, noise, nmap, orm, emis]


def _pbr_materials(sb, seed, masked=False):
    """Textures, samplers and materials of the material resolve's scenes: all three wrap modes and all six filter values across
    the slots, a material with no textures at all, one with metallicFactor 1, one of another shading type, normalFactorScale
    != 1, bExistOcclusion on and off.  masked: some of them alpha-tested.  Returns the material ids."""
    al, no, nm, orm, em = [sb.add_texture(t) for t in _pbr_textures(seed)]
    tri = sb.add_sampler(T.FILTER_LINEAR_MIPMAP_LINEAR, T.FILTER_LINEAR, T.WRAP_REPEAT, T.WRAP_REPEAT)
    near = sb.add_sampler(T.FILTER_NEAREST, T.FILTER_NEAREST, T.WRAP_CLAMP_TO_EDGE, T.WRAP_MIRRORED_REPEAT)
    lmn = sb.add_sampler(T.FILTER_LINEAR_MIPMAP_NEAREST, T.FILTER_NEAREST, T.WRAP_MIRRORED_REPEAT, T.WRAP_CLAMP_TO_EDGE)
    nml = sb.add_sampler(T.FILTER_NEAREST_MIPMAP_LINEAR, T.FILTER_LINEAR, T.WRAP_REPEAT, T.WRAP_MIRRORED_REPEAT)
    nmn = sb.add_sampler(T.FILTER_NEAREST_MIPMAP_NEAREST, T.FILTER_LINEAR, T.WRAP_MIRRORED_REPEAT, T.WRAP_REPEAT)
    lin = sb.add_sampler(T.FILTER_LINEAR, T.FILTER_LINEAR, T.WRAP_CLAMP_TO_EDGE, T.WRAP_REPEAT)
    mask = T.ALPHA_MASK if masked else 0
    return [
        sb.add_material(0, 0, al, tri, pbr=True, normal=(nm, tri), metallic_roughness=(orm, nml), emissive=(em, lmn),
                        emissive_factor=(1.0, 0.5, 2.0), occlusion_strength=0.75, normal_scale=1.0),                  # everything, trilinear
        sb.add_material(1, mask, no, near, 0.4, 0.9, pbr=True, normal=(nm, nmn), normal_scale=0.5,
                        base_color_factor=(0.8, 1.0, 0.6), roughness_factor=0.35, metallic_factor=1.0),              # no MR texture, metallicFactor 1
        sb.add_material(1, mask, al, lmn, 0.35, 1.0, pbr=True, metallic_roughness=(orm, lin), emissive=(em, nml),
                        emissive_factor=(0.3, 0.3, 0.3)),                                                            # no normal map, occlusion off
        sb.add_material(0, 0, pbr=True, roughness_factor=0.6, metallic_factor=0.25, base_color_factor=(0.5, 0.25, 0.125),
                        emissive_factor=(1.0, 1.0, 1.0)),                                                            # no textures at all
        sb.add_material(0, 0, al, tri, pbr=True, normal=(nm, tri), material_type=0),                                 # not a PBR material: zeros
        sb.add_material(0, 0, no, nmn, pbr=True, normal=(nm, lin), normal_scale=2.0, metallic_roughness=(orm, lmn),
                        occlusion_strength=1.0, emissive=(em, near), emissive_factor=(2.0, 2.0, 0.0)),               # nearest mips, scale 2
    ]


def material_test_scene(width=320, height=200, lods=2, seed=3, position=(-6.5, 2.2, 6.0), front=(0.75, -0.22, -0.62), masked=True):
    """masked_test_scene's layout under materials with all four texture slots (_pbr_materials), with normals and tangents: a
    magnified screen near the camera (alpha-tested unless masked is False: the scene shows through its holes), far minified
    buildings, tiled and negative texture coordinates, a ground under the trilinear material."""
    sb = SceneBuilder("material_test_scene", True)
    mats = _pbr_materials(sb, seed, masked)
    order = [mats[3], mats[1], mats[2], mats[0], mats[4], mats[5], mats[3], mats[1]]
    return _masked_layout(sb, order, lods, seed, position, front, width, height, ground=mats[0], behind=mats[3],
                          ground_uv=(96.0, 96.0), screen_scale=0.55)


def with_textures(scene, textures):
    """`scene` under other texture entries, one per texture of the scene: (H, W, 4) images or records.TextureChain (a finished
    chain, e.g. records.bc_chain(image, T.TEXFMT_BC3): the texture block-compressed as the reference's material import stores
    it).  Everything else is shared with `scene`."""
    textures = list(textures)
    assert len(textures) == len(scene.texture_images)
    out = T.Scene(scene.objects, scene.primitives, scene.materials, scene.meshlets, scene.groups, scene.group_indices,
                  scene.meshlet_data, scene.positions, name=scene.name, texcoord0=scene.texcoord0, textures=textures,
                  samplers=scene.samplers, bvh_nodes=scene.bvh_nodes, normals=scene.normals, tangents=scene.tangents)
    if hasattr(scene, "local_to_world"):
        out.local_to_world = scene.local_to_world
    return out


def floor_under_camera(position=(0.3, 0.25, 0.2), front=(0.1, -0.6, -1.0), width=128, height=96):
    """One coarse 16 m floor patch (2 m cells) with the camera just above it: its triangles straddle
    the w = 0 plane and exercise the homogeneous clipper."""
    pb = PrimitiveBuilder()
    pb.add_surface(plane_surface((-8, 0, 8), (16, 0, 0), (0, 0, -16)), 1, 1)
    sb = SceneBuilder("floor_under_camera")
    sb.add_object(sb.add_primitive(pb))
    return sb.build(), Camera(position, front, width, height)


def masked_floor_under_camera(position=(0.3, 0.25, 0.2), front=(0.1, -0.6, -1.0), width=160, height=120, seed=4):
    """floor_under_camera with an alpha-tested checker on the (two-sided) floor and an opaque floor 1 m below it: the
    triangles that straddle the w = 0 plane go through the clipper WITH their texture coordinates."""
    sb = SceneBuilder("masked_floor_under_camera")
    tex = sb.add_texture(_alpha_textures(seed)[0])
    smp = sb.add_sampler(T.FILTER_LINEAR_MIPMAP_LINEAR, T.FILTER_LINEAR, T.WRAP_REPEAT, T.WRAP_MIRRORED_REPEAT)
    mat = sb.add_material(1, T.ALPHA_MASK, tex, smp, 0.5, 1.0)
    pb = PrimitiveBuilder()
    pb.uv_scale = (6.0, 6.0)
    pb.add_surface(plane_surface((-8, 0, 8), (16, 0, 0), (0, 0, -16)), 1, 1)
    sb.add_object(sb.add_primitive(pb), material=mat)
    pb = PrimitiveBuilder()
    pb.add_surface(plane_surface((-8, -1, 8), (16, 0, 0), (0, 0, -16)), 2, 2)
    sb.add_object(sb.add_primitive(pb))
    return sb.build(), Camera(position, front, width, height)


def bumpy_sphere_mesh(n=96, seed=1):
    """An indexed triangle mesh (not grid patches): a sphere with low-frequency bumps, open at the poles."""
    u, v = np.meshgrid(np.linspace(0, 2 * np.pi, n, endpoint=False), np.linspace(0.05, np.pi - 0.05, n))
    r = 1.0 + 0.05 * np.sin((4 + seed) * u) * np.sin(7 * v)
    pos = np.stack([r * np.sin(v) * np.cos(u), r * np.cos(v), r * np.sin(v) * np.sin(u)], -1).reshape(-1, 3).astype(np.float32)
    j, i = np.meshgrid(np.arange(n - 1), np.arange(n), indexing="ij")
    a, b, c, d = j * n + i, j * n + (i + 1) % n, (j + 1) * n + i, (j + 1) * n + (i + 1) % n
    idx = np.stack([a, c, b, b, c, d], -1).reshape(-1).astype(np.uint32)
    uv = np.stack([u / (2 * np.pi), v / np.pi], -1).reshape(-1, 2).astype(np.float32)
    return pos, idx, uv


def scene_from_meshes(meshes, local_to_world, prim_of_object=None, two_sided_of_object=None, name="mesh_scene", attributes=False):
    """A scene of triangle meshes that go through chordvis_nanite_build (own clusterizer / partition / simplifier, SURVEY
    8f-4): `meshes` = [(positions, indices, texcoord0 or None), ...], one primitive each; `local_to_world` = 4x4 matrices, one
    object each (object k instantiates primitive prim_of_object[k], default k mod len(meshes)).  attributes: normals and tangents of
    mesh_attributes built along (chordvis_nanite_build_attributes)."""
    from . import lib as L
    if attributes:
        prims = []
        for pos, idx, uv in meshes:
            nrm, tng = mesh_attributes(pos, idx, uv)
            prims.append(L.nanite_build(pos, idx, uv, normals=nrm, tangents=tng))
    else:
        prims = [L.nanite_build(pos, idx, uv) for pos, idx, uv in meshes]
    pr = np.zeros(len(prims), dtype=T.PRIMITIVE)
    ml, md, gr, gi, ps, bv, uvs = [], [], [], [], [], [], []
    nv = nm = nd = ng = ni = nb = 0
    for k, a in enumerate(prims):
        pr[k] = a.primitive[0]
        pr[k]["vertexOffset"], pr[k]["meshletOffset"], pr[k]["meshletGroupOffset"] = nv, nm, ng
        pr[k]["meshletGroupIndicesOffset"], pr[k]["bvhNodeOffset"] = ni, nb
        m = a.meshlets.copy(); m["dataOffset"] += nd
        ml.append(m); md.append(a.meshlet_data); gr.append(a.groups); gi.append(a.group_indices); ps.append(a.positions); bv.append(a.bvh_nodes)
        uvs.append(a.texcoord0 if a.texcoord0 is not None else np.zeros((len(a.positions), 2), np.float32))
        nv += len(a.positions); nm += len(m); nd += len(a.meshlet_data); ng += len(a.groups); ni += len(a.group_indices); nb += len(a.bvh_nodes)
    mats = np.concatenate([SceneBuilder._material(0), SceneBuilder._material(1)])
    objects = np.zeros(len(local_to_world), dtype=T.OBJECT)
    objects["GLTFPrimitiveDetail"] = (np.arange(len(local_to_world)) % len(prims)) if prim_of_object is None else np.asarray(prim_of_object)
    objects["GLTFMaterialData"] = 0 if two_sided_of_object is None else np.asarray(two_sided_of_object)
    scene = T.Scene(objects, pr, mats, np.concatenate(ml), np.concatenate(gr), np.concatenate(gi), np.concatenate(md), np.concatenate(ps),
                    name=name, texcoord0=np.concatenate(uvs), bvh_nodes=np.concatenate(bv),
                    normals=np.concatenate([a.normals for a in prims]) if attributes else None,
                    tangents=np.concatenate([a.tangents for a in prims]) if attributes else None)
    scene.local_to_world = np.ascontiguousarray(np.stack([np.asarray(m).T.reshape(16) for m in local_to_world]), dtype=np.float64)
    scene.built = prims
    return scene


def built_mesh_scene(width=640, height=360, n=96, attributes=False):
    """Meshes that went through chordvis_nanite_build instead of the grid-patch generator: instances of a bumpy sphere from
    3 m to 400 m so that every LOD level of the DAG is in use.  attributes: with normals and tangents (mesh_attributes)."""
    dists = [3.0, 6.0, 14.0, 30.0, 70.0, 160.0, 400.0]
    l2w = [translate(((k % 3) - 1) * 0.3 * dist, 0.08 * dist * ((k // 3) - 1), -dist) @ rotate_y(0.7 * k) @ scale(1.0 + 0.15 * k) for k, dist in enumerate(dists)]
    scene = scene_from_meshes([bumpy_sphere_mesh(n, seed) for seed in (1, 2)], l2w, two_sided_of_object=(np.arange(len(l2w)) // 2) % 2, name="built_mesh_scene",
                              attributes=attributes)
    return scene, Camera((0.0, 0.4, 1.0), (0.0, -0.05, -1.0), width, height)


def big_built_mesh_scene(width=1280, height=720, n=360):
    """One 258 k-triangle mesh through the builder (7 575 LOD-0 meshlets, 10+ LOD levels), seen close, at mid range and far."""
    l2w = [translate(-0.9, 0.0, -2.4) @ rotate_y(0.3), translate(1.5, 0.2, -7.0) @ rotate_y(1.1), translate(0.0, 3.0, -60.0)]
    scene = scene_from_meshes([bumpy_sphere_mesh(n, 3)], l2w, name="big_built_mesh_scene")
    return scene, Camera((0.0, 0.2, 1.0), (0.0, -0.02, -1.0), width, height)


def config5_subpixel(width=3840, height=2160, prims=1024, patches_per_prim=1024, instances=8, patch_px=8.0, seed=5, hotspot_sigma_px=None):
    """BASELINE config 5: `prims * patches_per_prim` unique camera-facing patches, each ~patch_px x patch_px
    pixels (128 triangles of ~0.5 px^2 at patch_px = 8), centres uniform over the screen, view depth uniform in
    [5, 50], instanced `instances` times with slightly shifted transforms; LOD0 only.  The defaults give
    1 048 576 patches = 134 M unique triangles (1.0 GB of positions + 0.84 GB of meshlet data), x 8 = 1.07 G triangles.
    Camera at the origin looking down -z (so world space = view space).
    hotspot_sigma_px: SURVEY 8d's variant "hotspot" -- the centres are Gaussian around the screen centre with that sigma in
    pixels (Box-Muller on the same counter-based random numbers) instead of uniform: every cluster of the frame lands in a
    few dozen screen tiles, which is the atomic-contention case the configuration is named for."""
    assert patches_per_prim % 4 == 0
    cam = Camera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), width, height)
    th = math.tan(0.5 * cam.fovy) if hasattr(cam, "fovy") else math.tan(0.5 * math.radians(45.0))
    aspect = width / height
    sb = SceneBuilder("config5_subpixel")
    k = (np.arange(9) / 8.0 - 0.5)
    M = patches_per_prim
    for p in range(prims):
        idx = (np.arange(M, dtype=np.uint64) + np.uint64(p) * np.uint64(M)) * np.uint64(4)
        if hotspot_sigma_px is None:
            sx = rand01(seed, idx + np.uint64(0)) * width
            sy = rand01(seed, idx + np.uint64(1)) * height
        else:
            u1 = np.maximum(rand01(seed, idx + np.uint64(0)), 1.0e-12)
            u2 = rand01(seed, idx + np.uint64(1))
            rad = np.sqrt(-2.0 * np.log(u1)) * float(hotspot_sigma_px)
            sx = np.clip(0.5 * width + rad * np.cos(2.0 * np.pi * u2), 0.0, width - 1.0)
            sy = np.clip(0.5 * height + rad * np.sin(2.0 * np.pi * u2), 0.0, height - 1.0)
        zv = 5.0 + 45.0 * rand01(seed, idx + np.uint64(2))
        size = patch_px * 2.0 * zv * th / height
        cx = (sx / width * 2.0 - 1.0) * zv * th * aspect
        cy = -(sy / height * 2.0 - 1.0) * zv * th
        X = cx[:, None, None] + size[:, None, None] * k[None, None, :]
        Y = cy[:, None, None] + size[:, None, None] * k[None, :, None]
        X, Y = np.broadcast_arrays(X, Y)
        nz = rand01(seed + 1, (np.arange(M * 81, dtype=np.uint64) + np.uint64(p) * np.uint64(M * 81))).reshape(M, 9, 9)
        Z = -zv[:, None, None] + (nz - 0.5) * 0.2 * size[:, None, None]
        pos = np.stack([X, Y, Z], axis=-1).astype(np.float32).reshape(M, 81, 3)
        pb = PrimitiveBuilder()
        ids = pb._add_meshlets(pos, 0)
        pb._add_groups(ids.reshape(-1, 4), 0.0, -1.0, 0.0, FLT_MAX)     # un-parented LOD0 groups of 4 (nanite_builder.cpp:373-390)
        prim = sb.add_primitive(pb)
        for i in range(instances):
            sb.add_object(prim, translate(0.013 * i, 0.007 * i, -0.05 * i))
    return sb.build(), cam


def stacked_layers(variant="large", width=320, height=192, layers=None, per_object=16):
    """Layers of one two-sided meshlet each (81 vertices / 128 triangles), stacked so that one binner of the set-up kernels
    fills a few tiles' bins far past their fixed part; groups of per_object layers are objects of their own (so that
    update_objects can take some of them out of view).
      * "large": camera-facing layers at distinct view depths 4 .. 20 m, camera at the origin looking down -z.  Every triangle
        of a layer is a sliver of a wedge through the screen centre (rows of vertices alternate between two opposite rays
        1 200 px out), so its bbox spans the whole screen -- a large record -- and every triangle touches the centre tile
        (2, 1): that bin holds 128 entries per layer.  Nothing crosses the near plane or the guard band.  An opaque backdrop
        at 40 m covers the screen behind them (its cells are small: not large records), so a history HZB occludes anything
        moved further down the view.
      * "near": horizontal layers 2 mm apart, 0 .. 0.64 m under a camera looking down and forward; rows of vertices alternate
        between 3 m in front of the camera and 2 m behind it, so every triangle straddles the near plane and nearly all the
        bin entries of the frame come from clipped pieces."""
    sb = SceneBuilder("stacked_layers_" + variant)
    mat = sb.add_material(1)
    i = np.arange(9, dtype=np.float64)[None, :]
    j = np.arange(9, dtype=np.float64)[:, None]
    if variant == "large":
        layers = 192 if layers is None else layers
        cam = Camera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), width, height)
        th, aspect = math.tan(0.5 * cam.fovy), width / height
        R, delta = 1200.0, 4.0 / 1200.0
        golden = math.pi * (3.0 - math.sqrt(5.0))

        def world(sx, sy, zv):
            return np.stack([(sx / width * 2.0 - 1.0) * zv * th * aspect, -(sy / height * 2.0 - 1.0) * zv * th,
                             np.broadcast_to(-zv, np.shape(sx))], axis=-1)

        def layer(l):
            ang = (l * golden) % math.pi + i * delta + j * math.pi
            rad = R * (1.0 + 0.03 * j)
            zv = 4.0 + 16.0 * l / layers
            return world(0.5 * width + rad * np.cos(ang), 0.5 * height + rad * np.sin(ang), zv)
    elif variant == "near":
        layers = 320 if layers is None else layers
        cam = Camera((0.3, 0.25, 0.2), (0.1, -0.6, -1.0), width, height)
        cx, cz = cam.position[0], cam.position[2]

        def layer(l):
            x = np.broadcast_to(cx - 0.6 + 1.2 * i / 8.0, (9, 9))
            z = np.broadcast_to(cz + np.where(j % 2 == 0, -3.0, 2.0) - 0.05 * j, (9, 9))
            return np.stack([x, np.full((9, 9), -0.002 * l), z], axis=-1)
    else:
        raise ValueError(variant)
    assert layers % per_object == 0 and per_object % 4 == 0
    for o in range(layers // per_object):
        pos = np.stack([layer(o * per_object + k) for k in range(per_object)]).astype(np.float32).reshape(per_object, 81, 3)
        pb = PrimitiveBuilder()
        ids = pb._add_meshlets(pos, 0)
        pb._add_groups(ids.reshape(-1, 4), 0.0, -1.0, 0.0, FLT_MAX)     # un-parented LOD0 groups of 4
        sb.add_object(sb.add_primitive(pb), material=mat)
    if variant == "large":
        pb = PrimitiveBuilder()
        zb = 40.0
        x0, y0 = -1.1 * zb * th * aspect, -1.1 * zb * th
        pb.add_surface(plane_surface((x0, y0, -zb), (-2.0 * x0, 0.0, 0.0), (0.0, -2.0 * y0, 0.0)), 1, 1)
        sb.add_object(sb.add_primitive(pb), material=mat)
    return sb.build(), cam


# ------------------------------------------------------------------ general transforms and motion ---

def rotate_x(a):
    c, s = math.cos(a), math.sin(a)
    m = np.eye(4)
    m[1, 1], m[1, 2], m[2, 1], m[2, 2] = c, -s, s, c
    return m


def rotate_z(a):
    c, s = math.cos(a), math.sin(a)
    m = np.eye(4)
    m[0, 0], m[0, 1], m[1, 0], m[1, 1] = c, -s, s, c
    return m


def rotate_axis(axis, a):
    """Rotation by `a` about an arbitrary axis (Rodrigues)."""
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + math.sin(a) * K + (1.0 - math.cos(a)) * (K @ K)
    return m


# classes of general_transform_scene's objects (Scene.transform_class)
TILTED, STRETCHED, MIRRORED, SIZED = 0, 1, 2, 3


def _moving(scene, at):
    """Gives a built scene its motion: at(t) -> list of 4x4 local-to-world matrices; t = 1 is the scene's own frame, t = 0 the one
    before it.  Scene.local_to_world_at(t) has Scene.local_to_world's layout (glm column-major doubles)."""
    scene.local_to_world_at = lambda t: np.ascontiguousarray(np.stack([np.asarray(m).T.reshape(16) for m in at(float(t))]), dtype=np.float64)
    scene.local_to_world = scene.local_to_world_at(1.0)
    return scene.local_to_world_at(0.0)


def _camera_basis(position, front, world_up=(0.0, 1.0, 0.0)):
    f = np.asarray(front, dtype=np.float64); f = f / np.linalg.norm(f)
    r = np.cross(f, np.asarray(world_up, dtype=np.float64)); r = r / np.linalg.norm(r)
    return np.asarray(position, dtype=np.float64), f, r, np.cross(r, f)


def general_transform_scene(width=640, height=360, seed=11, masked=False, attributes=False, lods=3,
                            position=(-7.0, 1.6, 6.5), front=(0.8, -0.12, -0.6), world_up=(0.22, 1.0, 0.13), materials=False):
    """The primitives of small_test_scene / masked_test_scene under general object transforms, in motion.  Returns (scene, camera,
    local_to_world_last); the scene also carries transform_class (one of TILTED, STRETCHED, MIRRORED, SIZED per object), motion (a
    word per object) and local_to_world_at(t) (t = 1: the scene's frame, 0: the frame before, 2, 3 ..: the motion continued).

    Classes cycle over the objects so that each occurs several times with single- and two-sided materials:
      TILTED     rotations about x, y and z composed, uniform scale;
      STRETCHED  R1 @ scale(sx, sy, sz) @ R2 with one factor below 1 and one above 2: sheared relative to the mesh axes;
      MIRRORED   one of the two above with one axis negated (determinant < 0);
      SIZED      instances of one building from large and near to small and far (the LOD cut picks different levels).
    Motion: "spin" rotates in place, "slide" translates across the view, "rescale" changes scale, "reveal" starts behind the wall (a
    large occluder in front of the camera) and ends beside it, "hide" does the reverse, "enter" comes into the frustum from outside,
    "still" does not move.  masked: alpha-tested materials on every class and a masked quad that crosses the near plane.
    materials: the opaque scene under the textured materials of the material resolve (_pbr_materials), with normals and tangents
    and masked's texture coordinates: mirrored and stretched objects carry the bitangent's sign through the TBN."""
    assert not (masked and materials)
    sb = SceneBuilder("general_transform_scene" + ("_masked" if masked else "_materials" if materials else ""), attributes or materials)
    P, f, r, u = _camera_basis(position, front, world_up)
    if materials:
        pm = _pbr_materials(sb, seed)
        one, two = [pm[0], pm[5]], [pm[1], pm[2]]
        masked = "uv"                               # (the tiled texture coordinates of the masked variant; no alpha test)
    elif masked:
        tex = [sb.add_texture(t) for t in _alpha_textures(seed)]
        smp = [sb.add_sampler(T.FILTER_LINEAR_MIPMAP_LINEAR, T.FILTER_LINEAR, T.WRAP_REPEAT, T.WRAP_REPEAT),
               sb.add_sampler(T.FILTER_NEAREST, T.FILTER_NEAREST, T.WRAP_CLAMP_TO_EDGE, T.WRAP_MIRRORED_REPEAT)]
        one = [sb.add_material(0, T.ALPHA_MASK, tex[0], smp[0], 0.5, 1.0), 0]
        two = [sb.add_material(1, T.ALPHA_MASK, tex[1], smp[1], 0.4, 0.9), sb.add_material(1, T.ALPHA_MASK, tex[2], smp[0], 0.35, 1.0)]
    else:
        one, two = [0], [sb.add_material(1)]
    objs = []                                   # (prim, material, class, motion word, at(t) -> 4x4)

    def rnd(k, n=12):
        return rand01(seed + 1, np.arange(k * n, k * n + n))

    def tilt(q, t=0.0):
        return rotate_y(q[0] * 6.0 + t) @ rotate_x((q[1] - 0.5) * 1.2 + 0.35) @ rotate_z((q[2] - 0.5) * 1.2 + 0.3)

    def general(cls, q, mirror_axis=0):
        """t -> the 4x4 without its translation, for a class and 12 random numbers"""
        if cls == TILTED:
            return lambda t, spin=0.0, grow=0.0: tilt(q, spin * t) @ scale((0.8 + 0.6 * q[3]) * (1.0 + grow * t))
        s3 = (0.4 + 0.25 * q[3], 2.1 + 0.4 * q[4], 1.0 + 0.3 * q[5])
        s3 = tuple(np.roll(s3, int(q[6] * 3)))
        R2 = rotate_z(0.4 + q[7]) @ rotate_x(0.3 + q[8])
        if cls == STRETCHED:
            return lambda t, spin=0.0, grow=0.0: tilt(q, spin * t) @ scale(*s3) @ scale(1.0 + grow * t) @ R2
        flip = np.ones(3); flip[mirror_axis] = -1.0
        base = general(TILTED if q[9] < 0.5 else STRETCHED, q)
        return lambda t, spin=0.0, grow=0.0: base(t, spin, grow) @ scale(*flip)

    # the ground, tilted a little (class TILTED, still)
    pb = PrimitiveBuilder(sb.attributes)
    pb.add_surface(plane_surface((-8, 0, 8), (16, 0, 0), (0, 0, -16), seed, 0.2, 0.7), 8, 8, min(lods, 3))
    g = translate(0.0, -0.4, 0.0) @ rotate_y(0.5) @ rotate_x(0.06) @ rotate_z(-0.05)
    objs.append((sb.add_primitive(pb), 0, TILTED, "still", lambda t, g=g: g))
    # one building shared by the SIZED objects
    pb = PrimitiveBuilder(sb.attributes)
    if masked:
        pb.uv_scale = (2.0, 3.0)
    _building(pb, 2.0, 1.6, 2.4, seed * 100 + 900, min(lods, 3))
    sized_prim = sb.add_primitive(pb)
    motions = ["spin", "slide", "rescale", "still"]
    n_cycle = 16
    for k in range(n_cycle):
        q = rnd(k)
        cls = k % 4
        two_sided = (k // 4) % 2 == 1
        mat = (two if two_sided else one)[(k // 8) % len(two if two_sided else one)]
        if cls == SIZED:
            prim = sized_prim
            j = k // 4                                               # 0 .. 3: near and large -> far and small
            dist, size = (4.5, 8.0, 16.0, 34.0)[j], (0.45, 0.6, 0.45, 0.25)[j]
            centre = P + dist * f + ((j % 2) * 2 - 1) * 0.25 * dist * r - 0.2 * dist * u
            base = lambda t, spin=0.0, grow=0.0, q=q, size=size: tilt(q, spin * t) @ scale(size * (1.0 + grow * t))
        else:
            pb = PrimitiveBuilder(sb.attributes)
            if masked:
                pb.uv_scale = (1.0 + 3.0 * q[10], 0.5 + 2.5 * q[11]) if k % 3 else (-2.0, 3.0)
            if (k + k // 4) % 2 == 0:
                _building(pb, 1.5 + q[3], 1.5 + q[4], 1.0 + 2.5 * q[5], seed * 100 + k * 8, min(lods, 3))
            else:
                pb.add_surface(cylinder_surface((0, 0, 0), 0.3 + 0.4 * q[3], 1.0 + 2.0 * q[4], seed * 100 + k, 0.03), 4, 4, lods)
            prim = sb.add_primitive(pb)
            centre = P + (5.0 + 9.0 * q[10]) * f + (q[11] - 0.5) * 7.0 * r - (0.6 + 0.8 * q[9]) * u
            base = general(cls, q, mirror_axis=k % 3)
        word = motions[(k // 4 + k) % 4]
        d = {"spin": dict(spin=0.35), "rescale": dict(grow=0.3)}.get(word, {})
        v = (1.2 * r + 0.3 * f) if word == "slide" else np.zeros(3)
        objs.append((prim, mat, cls, word, lambda t, c=centre, v=v, base=base, d=d: translate(*(c + (t - 1.0) * v)) @ base(t, **d)))
    # the wall: a large occluder 4 m in front of the camera, right of the view's centre (single-sided, facing the camera; TILTED by
    # construction: its plane follows the rolled camera)
    pb = PrimitiveBuilder(sb.attributes)
    pb.add_surface(plane_surface((0, 0, 0), (1, 0, 0), (0, 1, 0), seed + 3, 0.0, 1.0), 4, 4, 1)
    wall = np.eye(4)
    wall[:3, 0], wall[:3, 1], wall[:3, 2] = 2.2 * r, 1.7 * u, -f
    wall[:3, 3] = P + 4.0 * f + 0.5 * r - 0.6 * u
    objs.append((sb.add_primitive(pb), 0, TILTED, "still", lambda t, w=wall: w))
    # behind it, 7 .. 8 m out: one object of each general class comes out from behind the wall, one of each goes in, one of each
    # enters the frustum from the left
    for j, (word, cls) in enumerate([(w_, c_) for w_ in ("reveal", "hide", "enter") for c_ in (TILTED, STRETCHED, MIRRORED)]):
        q = rnd(100 + j)
        pb = PrimitiveBuilder(sb.attributes)
        if masked:
            pb.uv_scale = (2.0, 2.0)
        pb.add_surface(cylinder_surface((0, -0.5, 0), 0.35, 1.0, seed * 100 + 500 + j, 0.03), 4, 4, lods)
        prim = sb.add_primitive(pb)
        base = general(cls, q, mirror_axis=j % 3)
        dist = 7.0 + 0.35 * (j % 3)
        row = (((j % 3) - 1) * 0.7 + 0.4) * u
        half = dist * math.tan(math.radians(22.5)) * width / height
        if word == "reveal":
            c0, c1 = P + dist * f + 2.8 * r + row, P + dist * f - 1.6 * r + row
        elif word == "hide":
            c0, c1 = P + (dist + 1.0) * f - 2.4 * r + row, P + (dist + 1.0) * f + 3.0 * r + row
        else:                                                        # (the mirrored one is a frame late: still outside at t = 1)
            c0 = P + dist * f - (half + (4.5 if cls == MIRRORED else 2.5)) * r + row
            c1 = c0 + (2.6 if cls == MIRRORED else 3.7) * r
        mat = (two if j % 2 else one)[0]
        objs.append((prim, mat, cls, word, lambda t, c0=c0, c1=c1, base=base: translate(*(c0 + t * (c1 - c0))) @ base(t, spin=0.2)))
    # two single-sided panels whose surface normal points at the camera, one stretched, one stretched and mirrored: the mirrored
    # one has every triangle wound the other way on screen and loses them all to the back-face rule (mesh_raster.cpp:235)
    pb = PrimitiveBuilder(sb.attributes)
    if masked:
        pb.uv_scale = (2.0, 1.0)
    pb.add_surface(plane_surface((-0.5, -0.5, 0), (1, 0, 0), (0, 1, 0), seed + 4, 0.03, 5.0), 2, 2, 1)
    panel = sb.add_primitive(pb)
    for sign, cls, c in ((1.0, STRETCHED, P + 5.0 * f - 2.6 * r + 1.25 * u), (-1.0, MIRRORED, P + 5.2 * f - 0.3 * r + 1.3 * u)):
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = sign * 2.1 * r, 0.55 * u, -f, c
        objs.append((panel, one[0], cls, "spin", lambda t, m=m: m @ rotate_z(0.25 * (t - 1.0))))
    # a two-sided strip that passes left of and below the camera, from 2 m behind it to 2 m ahead, stretched, sheared and mirrored: its
    # triangles cross the near plane and (masked: with their texture coordinates) go through the clipper under a general matrix
    pb = PrimitiveBuilder(sb.attributes)
    pb.uv_scale = (3.0, 2.0)
    pb.add_surface(plane_surface((-0.5, -0.5, 0), (1, 0, 0), (0, 1, 0), seed + 5, 0.0, 1.0), 1, 1, 1)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2] = 4.0 * (f + 0.05 * u + 0.03 * r), 0.3 * (r + 0.2 * f + 0.1 * u), u + 0.1 * r - 0.15 * f
    m[:3, 3] = P + 0.3 * f - 0.05 * r - 0.12 * u
    objs.append((sb.add_primitive(pb), two[0], MIRRORED, "still", lambda t, m=m: m))
    for prim, mat, cls, word, at in objs:
        sb.add_object(prim, at(1.0), material=mat)
    scene = sb.build()
    scene.transform_class = np.array([o[2] for o in objs])
    scene.motion = [o[3] for o in objs]
    last = _moving(scene, lambda t: [o[4](t) for o in objs])
    return scene, Camera(position, front, width, height, world_up=world_up, jitter=(0.3, -0.2)), last


def general_cameras(cam, steps=4):
    """Views of a sequence that starts at `cam`: the camera turns (front changes) and moves between consecutive views, its world_up
    is rolled out of the plane of front and +y, and fovy (45, 52, 100, 20 degrees), z_near and jitter change from view to view."""
    P, f, r, u = _camera_basis(cam.position, cam.front, cam.world_up)
    out = [cam]
    spec = [(52.0, 0.05, (-0.25, 0.4), 0.06, (0.1, 0.02, -0.05), (0.3, 1.0, -0.1)),
            (100.0, 0.01, (0.45, 0.1), -0.05, (0.05, 0.05, 0.1), (-0.25, 1.0, -0.15)),
            (20.0, 0.2, (-0.4, -0.35), 0.04, (-0.1, 0.0, 0.05), (0.15, 1.0, 0.3))]
    for k in range(1, steps):
        fov, zn, jit, turn, move, up = spec[(k - 1) % len(spec)]
        f = f + turn * r + 0.3 * turn * u
        f = f / np.linalg.norm(f)
        P = P + np.asarray(move)
        out.append(Camera(tuple(P), tuple(f), cam.width, cam.height, math.radians(fov), zn, cam.z_far, up, jit))
    return out


def config3_street_general(width=3840, height=2160, lods=3, share_mirrored=4):
    """config3_street's geometry (_street_primitives) with every building tilted by a few degrees and stretched non-uniformly, every
    share_mirrored-th building and prop mirrored, and every seventh prop moving along the street.  Returns (scene, camera,
    local_to_world_last) like general_transform_scene; the camera is config3_street's, rolled."""
    sb = SceneBuilder("config3_street_general")
    ats = []
    for k, (prim, l2w) in enumerate(_street_primitives(sb, lods)):
        q = rand01(3777, np.arange(k * 8, k * 8 + 8))
        if k == 0:
            m = l2w @ rotate_y(0.02) @ rotate_x(0.004) @ rotate_z(-0.003)
        else:
            tilt = rotate_x((q[0] - 0.5) * 0.14 + 0.03) @ rotate_z((q[1] - 0.5) * 0.14 - 0.03) @ rotate_y(0.1 + q[2])
            s3 = np.roll((0.75 + 0.2 * q[3], 1.0 + 0.2 * q[4], 1.25 + 0.25 * q[5]), k % 3)
            if k % share_mirrored == 0:
                s3[k % 2 * 2] *= -1.0
            m = l2w @ tilt @ scale(*s3) @ rotate_y(-(0.1 + q[2]))
        v = np.array([2.5 * (q[6] - 0.3), 0.0, 0.4 * (q[7] - 0.5)]) if (k > 40 and k % 7 == 0) else None
        sb.add_object(prim, m)
        ats.append((lambda t, m=m: m) if v is None else (lambda t, m=m, v=v: translate(*((t - 1.0) * v)) @ m @ rotate_y(0.3 * (t - 1.0))))
    scene = sb.build()
    last = _moving(scene, lambda t: [a(t) for a in ats])
    return scene, Camera((-62.0, 12.0, 3.0), (1.0, -0.18, -0.04), width, height, world_up=(0.1, 1.0, -0.06)), last


def general_long_scene(groups=512 * 256 + 64 * 5 + 7, width=640, height=360, shown=64, seed=2):
    """group_count_scene's construction (more than 65 536 group instances and more than 512 count blocks of 256 at the default) under
    general transforms: the shown objects are tilted, stretched or mirrored in turn and move between the frames; the others are
    behind the camera, general as well.  Returns (scene, camera, local_to_world_last)."""
    sb = SceneBuilder("general_long_%d" % groups)
    pb = PrimitiveBuilder()
    pb.add_surface(plane_surface((-0.5, -0.5, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), seed, 0.05, 2.0), 16, 16, 1)
    panel = sb.add_primitive(pb)
    pb = PrimitiveBuilder()
    pb.add_surface(plane_surface((-0.5, -0.5, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), seed + 1, 0.08, 1.5), 2, 2, 1)
    tile = sb.add_primitive(pb)
    two = sb.add_material(1)
    prims = [panel] * (groups // 64) + [tile] * (groups % 64)
    n = len(prims)
    picked = set(np.linspace(0, n - 1, min(n, shown)).round().astype(np.int64).tolist())
    hidden = rotate_x(0.3) @ rotate_y(0.4) @ rotate_z(0.2) @ scale(0.8, 1.1, 0.9)
    ats, j = [], 0
    for k, prim in enumerate(prims):
        if k in picked:
            col, row, layer = j % 8, (j // 8) % 4, (j // 32) % 3
            q = rand01(seed + 7, np.arange(6 * j, 6 * j + 6))
            c = np.array([col - 3.5 + 0.5 * layer, row - 1.5 + 0.3 * layer, -1.2 * layer - 0.2 * q[0]])
            s3 = np.roll((0.6, 1.0, 1.3), j % 3) * (1.0, 1.0, 1.0)
            if j % 3 == 2:
                s3[j % 2] *= -1.0
            R = rotate_y((q[1] - 0.5) * 0.8 + 0.15) @ rotate_x((q[2] - 0.5) * 0.6 + 0.1) @ rotate_z((q[3] - 0.5) * 0.6 - 0.1)
            R2 = rotate_z(0.2 + 0.3 * q[4])
            v = np.array([0.6 * (q[5] - 0.5), 0.2 * (q[4] - 0.5), 0.5 * (q[3] - 0.5)]) if j % 2 else np.zeros(3)
            ats.append(lambda t, c=c, v=v, R=R, s3=s3, R2=R2, sp=0.2 * (j % 4): translate(*(c + (t - 1.0) * v)) @ rotate_y(sp * (t - 1.0)) @ R @ scale(*s3) @ R2)
            mat = two if j % 4 == 1 else 0
            j += 1
        else:
            m = translate((k % 37) * 0.5, (k % 11) * 0.5, 40.0 + (k % 5)) @ hidden @ scale(-1.0 if k % 3 == 0 else 1.0, 1.0, 1.0)
            ats.append(lambda t, m=m: m)
            mat = 0
        sb.add_object(prim, ats[-1](1.0), material=mat)
    scene = sb.build()
    assert scene.group_instances == groups
    last = _moving(scene, lambda t: [a(t) for a in ats])
    return scene, Camera((0.0, 0.0, 6.0), (0.02, -0.01, -1.0), width, height, world_up=(0.2, 1.0, 0.0)), last


def unit_depth_scene(width=320, height=180):
    """A perspective camera at the origin looking down -z and objects whose origin lies at view depth exactly 1: the float32 product
    translatedWorldToClip * localToTranslatedWorld has [3][3] == 1.0f.  isOrthoProjection (base.hlsli:243-246) is asked about that
    PRODUCT (instance_culling.hlsl:71-89: isOrthoProjection(localToClip)), so the shader takes orthoFrustumCulling for these
    objects, for their meshlets and in the LOD cut -- the branch the text implies, and the one oracle, spec and kernels must share."""
    sb = SceneBuilder("unit_depth")
    two = sb.add_material(1)
    for k in range(6):
        pb = PrimitiveBuilder()
        pb.add_surface(cylinder_surface((0, -0.4, 0), 0.25, 0.8, 40 + k, 0.03), 4, 4, 2)
        R3 = rotate_y(0.4 + k) @ rotate_x(0.3 + 0.2 * k) @ rotate_z(0.2 - 0.3 * k) @ scale(0.5, 1.3, 0.8 if k % 2 else -0.8)
        x = (-0.9, -0.3, 0.3, 0.9, -4.5, 1.3)[k]
        if k == 4:      # large, left of the view, reaching behind the camera: every corner is behind the left plane, but the corners
            R3 = R3 @ scale(4.0)   # with w < 0 project across the screen -- the plane test culls it, the projected rectangle does not
        sb.add_object(sb.add_primitive(pb), translate(x, 0.1 * (k % 3) - 0.1, -1.0) @ R3, material=two if k % 3 == 0 else 0)
    pb = PrimitiveBuilder()
    pb.add_surface(plane_surface((-3, -2, -4), (6, 0, 0), (0, 4, 0), 50, 0.1, 1.0), 4, 4, 1)
    sb.add_object(sb.add_primitive(pb))
    return sb.build(), Camera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), width, height)
