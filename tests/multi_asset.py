"""Scenes of SEVERAL assets for the tests that hold every consumer of chordvis_upload_scene's concatenation to its specification
(tests/test_multi_asset_spec.py on the CPU, tests/test_gpu_multi_asset.py on the device).  TEST INFRASTRUCTURE: never imported by
chord_amd/.

chordvis_upload_scene lays the assets' meshlets, groups, group indices, meshlet data, vertices and BVH nodes down one asset after
the other and re-bases every primitive through primitiveDatasBufferId.  After that a meshlet has two numbers:
  concatenated    its index in the device's meshlet array: device command lists, the cull and the raster use it;
  asset-relative  its index in its own asset's meshlets: ChordDrawCmd::meshletId as chordvis_readback_cmds returns it, the meshlet
                  debug colour's hash id, and ChordRayHit::meshlet as chordvis_trace_rays / chordvis_pixel_rays write it and
                  chordvis_shade_ray_hits reads it.
With one asset every base is 0 and the two are one number; here no base but the first asset's is 0.

MultiAssetScene(assets) takes a list of records.Scene (each with .local_to_world) and gives
  .desc       the ChordSceneDesc the library gets: N ChordAssetDesc over the assets' own arrays; objects and primitives INTERLEAVED
              across the assets (A, B, C, A, ...: a primitive's row says nothing about its asset), GLTFPrimitiveDetail and
              GLTFMaterialData re-indexed, primitiveDatasBufferId set, every primitive's offsets still relative to its own asset;
              materials, textures and samplers concatenated asset by asset, a material's texture / sampler id shifted by its asset's
              first texture / sampler (an id its own asset does not have stays "none": 0xFFFFFFFF)
  .spec       the one-asset twin the specifications and the oracle read: a records.Scene over the SAME object, material, texture and
              sampler arrays with the assets' streams concatenated in the upload's order and the primitives' vertexOffset,
              meshletOffset, meshletGroupOffset, meshletGroupIndicesOffset, bvhNodeOffset and the meshlets' dataOffset re-based.
              An asset without texcoord0 / normals / tangents contributes zeros; a stream no asset has is absent.  Its command lists
              and hits are in the concatenated numbering.
  .asset_meshlet_base / .asset_meshlet_count   per primitive: its asset's first meshlet in .spec.meshlets and its meshlet count
  .to_asset_relative(records) / .to_concatenated(records)   copies of records.DRAW_CMD or records.RAY_HIT arrays in the other
              numbering, through the object's primitive; a record that names no object of the list (and a hit without status bit 0)
              is left alone.
"""
import functools

import numpy as np

from chord_amd import lib as L, records as R, scenes

import spec_rays_np as S

NONE = 0xFFFFFFFF
STREAMS = ("meshlets", "groups", "group_indices", "meshlet_data", "vertices", "bvh_nodes")
FW, FH = 200, 120                                     # the frames of the tests
PW, PH = 64, 40                                       # their pixel rays
_TEX_FIELDS = (("baseColorId", "baseColorSampler"), ("emissiveTexture", "emissiveSampler"), ("normalTexture", "normalSampler"),
               ("metallicRoughnessTexture", "metallicRoughnessSampler"))


def _interleave(counts):
    """[(asset, index in asset)] round robin: asset 0's first, asset 1's first, ..., asset 0's second, ... until all are placed."""
    out = []
    for k in range(max(counts)):
        out += [(a, k) for a, n in enumerate(counts) if k < n]
    return out


def _sizes(a):
    return dict(meshlets=len(a.meshlets), groups=len(a.groups), group_indices=len(a.group_indices), meshlet_data=len(a.meshlet_data),
                vertices=len(a.positions), bvh_nodes=0 if a.bvh_nodes is None else len(a.bvh_nodes))


class MultiAssetScene:
    def __init__(self, assets, name="multi_asset"):
        assets = list(assets)
        n = len(assets)
        self.name, self.assets = name, assets
        self.sizes = [_sizes(a) for a in assets]
        # the running bases of the upload (chordvis_abi.cpp "asset bases")
        self.bases = [{k: sum(self.sizes[b][k] for b in range(a)) for k in STREAMS} for a in range(n)]
        mat_base = np.cumsum([0] + [len(a.materials) for a in assets])
        tex_base = np.cumsum([0] + [len(a.texture_images) for a in assets])
        smp_base = np.cumsum([0] + [len(a.samplers) for a in assets])

        # primitives and objects, interleaved
        prim_at = _interleave([len(a.primitives) for a in assets])
        new_prim = {key: i for i, key in enumerate(prim_at)}
        prims = np.zeros(len(prim_at), dtype=R.PRIMITIVE)
        for i, (a, k) in enumerate(prim_at):
            prims[i] = assets[a].primitives[k]
            prims[i]["primitiveDatasBufferId"] = a
        self.asset_of_primitive = np.array([a for a, _ in prim_at], dtype=np.int64)
        obj_at = _interleave([len(a.objects) for a in assets])
        objs = np.zeros(len(obj_at), dtype=R.OBJECT)
        l2w = np.zeros((len(obj_at), 16), dtype=np.float64)
        for i, (a, k) in enumerate(obj_at):
            objs[i] = assets[a].objects[k]
            objs[i]["GLTFPrimitiveDetail"] = new_prim[(a, int(assets[a].objects[k]["GLTFPrimitiveDetail"]))]
            objs[i]["GLTFMaterialData"] = int(assets[a].objects[k]["GLTFMaterialData"]) + mat_base[a]
            l2w[i] = assets[a].local_to_world[k]
        self.asset_of_object = np.array([a for a, _ in obj_at], dtype=np.int64)
        self.index_in_asset_of_object = np.array([k for _, k in obj_at], dtype=np.int64)
        self.objects, self.primitives, self.local_to_world = objs, prims, l2w

        # materials, textures, samplers: asset by asset
        mats = []
        for a, s in enumerate(assets):
            m = s.materials.copy()
            for tex, smp in _TEX_FIELDS:
                m[tex] = np.where(m[tex] < len(s.texture_images), m[tex] + np.uint32(tex_base[a]), np.uint32(NONE))
                m[smp] = np.where(m[smp] < len(s.samplers), m[smp] + np.uint32(smp_base[a]), np.uint32(NONE))
            mats.append(m)
        self.materials = np.concatenate(mats)
        self.asset_of_material = np.concatenate([np.full(len(s.materials), a, dtype=np.int64) for a, s in enumerate(assets)])
        self.texture_images = [t for s in assets for t in s.texture_images]
        self.texture_base, self.sampler_base = [int(x) for x in tex_base[:-1]], [int(x) for x in smp_base[:-1]]
        self.samplers = np.concatenate([s.samplers for s in assets]) if smp_base[-1] else np.zeros(0, dtype=R.SAMPLER)
        self._textures = (R.Texture * max(1, len(self.texture_images)))()
        i = 0
        for s in assets:
            for k in range(len(s.texture_images)):
                t = s._textures[k]
                self._textures[i] = R.Texture(t.rgba8, t.width, t.height, t.mipCount, t.format)
                i += 1
        self._assets = (R.AssetDesc * n)(*[s._asset for s in assets])
        import ctypes as C
        self.desc = R.SceneDesc(objs.ctypes.data, len(objs), prims.ctypes.data, len(prims), self.materials.ctypes.data, len(self.materials),
                                self._assets, n, C.cast(self._textures, C.c_void_p) if self.texture_images else None, len(self.texture_images),
                                self.samplers.ctypes.data if len(self.samplers) else None, len(self.samplers))

        # the one-asset twin
        sp = prims.copy()
        sp["primitiveDatasBufferId"] = 0
        for i, (a, _) in enumerate(prim_at):
            b = self.bases[a]
            sp[i]["vertexOffset"] += b["vertices"]; sp[i]["meshletOffset"] += b["meshlets"]
            sp[i]["meshletGroupOffset"] += b["groups"]; sp[i]["meshletGroupIndicesOffset"] += b["group_indices"]
            sp[i]["bvhNodeOffset"] += b["bvh_nodes"]
        ml = []
        for a, s in enumerate(assets):
            m = s.meshlets.copy()
            m["dataOffset"] += self.bases[a]["meshlet_data"]
            ml.append(m)

        def stream(field, width):
            if all(getattr(s, field) is None for s in assets):
                return None
            return np.concatenate([getattr(s, field) if getattr(s, field) is not None else np.zeros((len(s.positions), width), np.float32)
                                   for s in assets])
        self.bvh_complete = all(s.bvh_nodes is not None for s in assets)
        self.spec = R.Scene(objs, sp, self.materials, np.concatenate(ml), np.concatenate([s.groups for s in assets]),
                            np.concatenate([s.group_indices for s in assets]), np.concatenate([s.meshlet_data for s in assets]),
                            np.concatenate([s.positions for s in assets]), name=name + "+twin", texcoord0=stream("texcoord0", 2),
                            textures=self.texture_images, samplers=self.samplers if len(self.samplers) else None,
                            bvh_nodes=np.concatenate([s.bvh_nodes for s in assets]) if self.bvh_complete else None,
                            normals=stream("normals", 3), tangents=stream("tangents", 4))
        assert self.spec.objects is objs and self.spec.materials is self.materials, "the twin reads the very records the library gets"
        self.spec.local_to_world = l2w

        # the numbering contract as data
        self.asset_meshlet_base = np.array([self.bases[a]["meshlets"] for a in self.asset_of_primitive], dtype=np.int64)
        self.asset_meshlet_count = np.array([self.sizes[a]["meshlets"] for a in self.asset_of_primitive], dtype=np.int64)

    # -- what the renderer's helpers and the scene helpers read of a scene ---------------------------------------------------------
    def with_object_list(self, objects, local_to_world=None):
        """The twin under another object list (records of THIS scene's primitives and materials), for chordvis_set_object_list."""
        out = self.spec.with_objects(np.ascontiguousarray(objects, dtype=R.OBJECT))
        if local_to_world is not None:
            out.local_to_world = np.ascontiguousarray(local_to_world, dtype=np.float64)
        return out

    def relisted(self, objects):
        """This scene under another object list, as a scene of several assets to upload afresh: .desc (the same assets, primitives,
        materials and textures), .objects, .primitives, .texture_images."""
        import copy
        out = copy.copy(self)
        out.objects = np.ascontiguousarray(objects, dtype=R.OBJECT).copy()
        d = self.desc
        out.desc = R.SceneDesc(out.objects.ctypes.data, len(out.objects), d.primitives, d.primitiveCount, d.materials, d.materialCount,
                               d.assets, d.assetCount, d.textures, d.textureCount, d.samplers, d.samplerCount)
        out._base = self                                    # (the arrays the descriptor points into)
        return out

    def alone(self, a):
        """Asset a as a records.Scene of its own under the records its objects have in this scene NOW (filled for a camera), with its
        own primitive, material, texture and sampler numbering: what the asset looks like without the others."""
        at = np.flatnonzero(self.asset_of_object == a)
        objs = self.objects[at].copy()
        objs["GLTFPrimitiveDetail"] = self.assets[a].objects["GLTFPrimitiveDetail"][self.index_in_asset_of_object[at]]
        objs["GLTFMaterialData"] = self.assets[a].objects["GLTFMaterialData"][self.index_in_asset_of_object[at]]
        return self.assets[a].with_objects(objs)

    def edge_hits(self):
        """[(what, records.RAY_HIT of one hit, valid?)] at the edges of the asset-relative numbering, for chordvis_shade_ray_hits:
        the last meshlet of asset 1 on an object of the primitive that owns it; a relative id equal to asset 1's meshlet count --
        invalid, though base + id is a meshlet of asset 2 and the id is below the scene's total --; an object of asset 2 with a
        meshlet of another primitive of asset 2 (the vertex ids take the OBJECT's primitive's vertexOffset)."""
        def hit(obj, meshlet, tri=0, u=0.25, v=0.5, status=1):
            h = np.zeros(1, dtype=R.RAY_HIT)
            h["t"], h["u"], h["v"], h["object"], h["meshlet"], h["triangle"], h["status"] = 1.0, u, v, obj, meshlet, tri, status
            h["primitive"] = self.objects["GLTFPrimitiveDetail"][obj]
            return h
        prim_of = self.objects["GLTFPrimitiveDetail"].astype(np.int64)
        n1 = self.sizes[1]["meshlets"]
        # asset 1's last meshlet belongs to its last primitive (meshlets lie primitive after primitive)
        own1 = [p for p in np.flatnonzero(self.asset_of_primitive == 1)]
        last1 = max(own1, key=lambda p: int(self.primitives["meshletOffset"][p]))
        obj1 = int(np.flatnonzero(prim_of == last1)[0])
        # asset 2: an object, and the first meshlet of another of its primitives whose vertex ids fit the object's primitive
        own2 = [int(p) for p in np.flatnonzero(self.asset_of_primitive == 2)]
        obj2 = int(np.flatnonzero(prim_of == own2[1])[0])
        other = int(self.primitives["meshletOffset"][own2[0]])
        assert n1 < len(self.spec.meshlets) and self.bases[1]["meshlets"] + n1 == self.bases[2]["meshlets"]
        return [("the last meshlet of asset 1", hit(obj1, n1 - 1), True),
                ("asset 1's meshlet count on an object of asset 1", hit(obj1, n1), False),
                ("0xFFFFFFFF on an object of asset 1", hit(obj1, 0xFFFFFFFF), False),
                ("asset 2's meshlet count on an object of asset 2", hit(obj2, self.sizes[2]["meshlets"]), False),
                ("a meshlet of another primitive of asset 2", hit(obj2, other, status=3), True)]

    # -- the two numberings ------------------------------------------------------------------------------------------------------
    def _shift(self, records, sign, objects):
        records = np.array(records, copy=True)
        objects = self.objects if objects is None else objects
        if records.dtype == R.DRAW_CMD:
            obj, field, live = records["objectId"].astype(np.int64), "meshletId", np.ones(len(records), dtype=bool)
        elif records.dtype == R.RAY_HIT:
            obj, field, live = records["object"].astype(np.int64), "meshlet", (records["status"] & 1) != 0
        else:
            raise TypeError("records.DRAW_CMD or records.RAY_HIT, not %r" % (records.dtype,))
        live &= obj < len(objects)
        prim = objects["GLTFPrimitiveDetail"][np.where(live, obj, 0)].astype(np.int64)
        live &= prim < len(self.primitives)
        base = self.asset_meshlet_base[np.where(live, prim, 0)]
        records[field] = np.where(live, (records[field].astype(np.int64) + sign * base) & 0xFFFFFFFF, records[field]).astype(np.uint32)
        return records

    def to_asset_relative(self, records, objects=None):
        return self._shift(records, -1, objects)

    def to_concatenated(self, records, objects=None):
        return self._shift(records, +1, objects)


# ---- the assets ------------------------------------------------------------------------------------------------------------------

def _offset(scene, matrix):
    """`scene` with every object's world transform behind `matrix` (4 x 4, applied after the object's own)."""
    l2w = np.stack([(np.asarray(matrix, dtype=np.float64) @ m.reshape(4, 4).T).T.reshape(16) for m in scene.local_to_world])
    scene.local_to_world = np.ascontiguousarray(l2w)
    return scene


def _rebuilt(s, materials=None, texcoord0=None, textures=(), samplers=None, bvh=True):
    out = R.Scene(s.objects, s.primitives, s.materials if materials is None else materials, s.meshlets, s.groups, s.group_indices,
                  s.meshlet_data, s.positions, name=s.name, texcoord0=texcoord0, textures=textures, samplers=samplers,
                  bvh_nodes=s.bvh_nodes if bvh else None, normals=s.normals, tangents=s.tangents)
    out.local_to_world = s.local_to_world.copy()
    return out


@functools.lru_cache(maxsize=None)
def _asset(which):
    """The three assets, of different sizes in every stream (built once; MultiAssetScene copies what it changes):
      0  scenes.small_test_scene(lods=3, attributes=True): normals, tangents, a BVH, and -- the builder makes no texture coordinates for a
         scene without textures -- a planar uv stream (x, z of the position scaled), one texture and one sampler of its own, which its
         two-sided material names as base colour
      1  small_test_scene of another seed with none of the three vertex streams, but a texture of its own that its first material
         names: every pixel of it samples at uv (0, 0)
      2  the textured "material" scene of tests/ray_shade_cases.py (scenes.material_test_scene: five textures, six samplers, masked
         materials)
      "1 without a BVH"  asset 1 with bvhNodes null."""
    rng = np.random.default_rng(41)
    if which == 0:
        s, _ = scenes.small_test_scene(FW, FH, lods=3, attributes=True)
        mats = s.materials.copy()
        mats["baseColorId"][1], mats["baseColorSampler"][1] = 0, 0
        uv = (s.positions[:, [0, 2]] * np.float32(0.37)).astype(np.float32)
        s = _rebuilt(s, mats, uv, [rng.integers(0, 256, size=(8, 16, 4), dtype=np.uint8)],
                     np.array([(R.FILTER_LINEAR_MIPMAP_LINEAR, R.FILTER_LINEAR, R.WRAP_REPEAT, R.WRAP_MIRRORED_REPEAT)], dtype=R.SAMPLER))
        return _offset(s, scenes.translate(-2.5, 2.0, 2.5) @ scenes.scale(0.35))
    if which in (1, "1 without a BVH"):
        s, _ = scenes.small_test_scene(FW, FH, lods=2, seed=9)     # (two LODs: another size in every stream)
        mats = s.materials.copy()
        mats["baseColorId"][0], mats["baseColorSampler"][0] = 0, 0
        tex = rng.integers(0, 256, size=(4, 4, 4), dtype=np.uint8)
        s = _rebuilt(s, mats, None, [tex], np.array([(R.FILTER_NEAREST, R.FILTER_NEAREST, R.WRAP_CLAMP_TO_EDGE, R.WRAP_CLAMP_TO_EDGE)], dtype=R.SAMPLER),
                     bvh=which == 1)
        return _offset(s, scenes.translate(1.0, 1.2, 5.5) @ scenes.scale(0.35))
    s, _ = scenes.material_test_scene(FW, FH)
    return s


def camera(width=FW, height=FH):
    """The material scene's camera, a little higher and further back: the three assets stand in view."""
    return scenes.Camera((-8.5, 4.0, 8.0), (0.75, -0.3, -0.62), width, height)


def three_assets():
    """(MultiAssetScene of assets 0, 1, 2 -- all with a BVH --, camera at the frames' size); object records not yet filled."""
    ms = MultiAssetScene([_asset(0), _asset(1), _asset(2)], "three_assets")
    check_bases(ms)
    return ms, camera()


def three_assets_blocks():
    """(scene, decoded twin scene, camera): three_assets with asset 2's five textures block-compressed (tests/test_gpu_ray_shade.py's
    formats) -- what the block store keeps as blocks -- and the same scene over the RGBA8 chains the blocks decode to, whose .spec the
    specifications read.  Both have records of their own to fill."""
    import spec_texture_bc_np as BC
    bc = BC.bc_scene(_asset(2), [BC.BC3, BC.BC3, BC.BC5, BC.BC1_RGB, BC.BC3])
    ms = MultiAssetScene([_asset(0), _asset(1), bc], "three_assets+blocks")
    twin = MultiAssetScene([_asset(0), _asset(1), BC.decoded_twin(bc)], "three_assets+decoded")
    return ms, twin, camera()


def two_assets_one_without_bvh():
    """(MultiAssetScene of asset 0 and asset 1 without its BVH, camera): the hierarchical cull is refused, flat frames are not."""
    ms = MultiAssetScene([_asset(0), _asset("1 without a BVH")], "two_assets_one_without_bvh")
    assert not ms.bvh_complete
    return ms, camera()


def check_bases(ms):
    """No base of assets 1 and 2 is 0, the two differ in every stream, and so do the three assets' sizes: with two assets "base of the
    last asset" and "size of the first" are one number, and with equal sizes "base of asset 2" is twice "base of asset 1"."""
    assert len(ms.assets) >= 3
    for k in STREAMS:
        b1, b2 = ms.bases[1][k], ms.bases[2][k]
        assert 0 < b1 < b2, (k, b1, b2)
        sz = [ms.sizes[a][k] for a in range(3)]
        assert len(set(sz)) == 3, (k, sz)
        assert b2 != 2 * b1, (k, b1, b2, sz)
    assert 0 < ms.texture_base[1] < ms.texture_base[2] and 0 < ms.sampler_base[1] < ms.sampler_base[2]
    # interleaved: three indirections, and a row says nothing about its asset
    assert list(ms.asset_of_primitive[:6]) == [0, 1, 2, 0, 1, 2] and list(ms.asset_of_object[:6]) == [0, 1, 2, 0, 1, 2]


def filled(ms, cam, camera_last=None, local_to_world_last=None):
    """Fills ms.objects (shared with the twin) for the camera; returns (view, iv)."""
    L.fill_objects(ms, cam, camera_last, local_to_world_last)
    assert ms.spec.objects is ms.objects
    return L.make_views(cam)


def ray_set(ms, seed=17):
    """The 64 x 40 pixel rays of camera(), then 100 seeded random rays from the box of each asset's objects (tests/test_gpu_rays.py's
    _random_rays per asset): (rays, asset of the random rays' origin box or -1 for a pixel ray).  Object records must be filled."""
    view, _ = L.make_views(camera(PW, PH))
    sets, origin = [S.pixel_rays(view, PW, PH)], [np.full(PW * PH, -1, dtype=np.int64)]
    for a in range(len(ms.assets)):
        objs = ms.objects[ms.asset_of_object == a]
        lo, hi = S.object_boxes(objs, ms.spec.primitives)
        lo, hi = lo.min(axis=0).astype(np.float64), hi.max(axis=0).astype(np.float64)
        n = 100
        r = scenes.rand01(seed + a, np.arange(7 * n)).reshape(n, 7)
        rays = S.make_rays(lo + r[:, :3] * (hi - lo), r[:, 3:6] * 2.0 - 1.0, 1e-2, 1e9)
        rays["tMax"][::5] = (r[::5, 6] * np.linalg.norm(hi - lo)).astype(np.float32)
        sets.append(rays)
        origin.append(np.full(n, a, dtype=np.int64))
    return np.concatenate(sets), np.concatenate(origin)
