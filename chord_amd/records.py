"""numpy mirrors of include/chordvis_types.h (the reference's shared C++/HLSL records).

Byte layouts follow install/resource/shader/gltf.h:16-153 and base.h:121-135,343-360
of the reference; sizes are asserted below and again against the C header in tests.
"""
import ctypes as C

import numpy as np

f32, u32 = np.float32, np.uint32

MESHLET = np.dtype([
    ("posMin", f32, 3), ("dataOffset", u32),
    ("posMax", f32, 3), ("vertexTriangleCount", u32),
    ("coneAxis", f32, 3), ("coneCutOff", f32),
    ("coneApex", f32, 3), ("lod", u32),
])
MESHLET_GROUP = np.dtype([
    ("clusterPosCenter", f32, 3), ("parentError", f32),
    ("parentPosCenter", f32, 3), ("error", f32),
    ("meshletOffset", u32), ("meshletCount", u32),
])
BVH_NODE = np.dtype([
    ("sphere", f32, 4), ("children", u32, 8), ("bvhNodeCount", u32), ("leafMeshletGroupOffset", u32), ("leafMeshletGroupCount", u32),
])
PRIMITIVE = np.dtype([
    ("posMin", f32, 3), ("primitiveDatasBufferId", u32),
    ("posMax", f32, 3), ("vertexOffset", u32),
    ("posAverage", f32, 3), ("vertexCount", u32),
    ("meshletOffset", u32), ("color0Offset", u32), ("smoothNormalOffset", u32), ("textureCoord1Offset", u32),
    ("bvhNodeOffset", u32), ("meshletGroupOffset", u32), ("meshletGroupIndicesOffset", u32), ("meshletGroupCount", u32),
    ("lod0IndicesOffset", u32), ("lod0IndicesCount", u32), ("pad0", u32), ("pad1", u32),
])
MATERIAL = np.dtype([
    ("alphaMode", u32), ("alphaCutOff", f32), ("bTwoSided", u32), ("baseColorId", u32),
    ("baseColorFactor", f32, 4),
    ("emissiveFactor", f32, 3), ("emissiveTexture", u32),
    ("metallicFactor", f32), ("roughnessFactor", f32), ("metallicRoughnessTexture", u32), ("normalTexture", u32),
    ("baseColorSampler", u32), ("emissiveSampler", u32), ("normalSampler", u32), ("metallicRoughnessSampler", u32),
    ("normalFactorScale", f32), ("bExistOcclusion", u32), ("occlusionTextureStrength", f32), ("materialType", u32),
])
OBJECT = np.dtype([
    ("localToTranslatedWorld", f32, 16),
    ("translatedWorldToLocal", f32, 16),
    ("localToTranslatedWorldLastFrame", f32, 16),
    ("scaleExtractFromMatrix", f32, 4),
    ("GLTFPrimitiveDetail", u32), ("GLTFMaterialData", u32), ("pad1", u32), ("pad2", u32),
])
INSTANCE_CULLING_VIEW = np.dtype([
    ("translatedWorldToClip", f32, 16),
    ("clipToTranslatedWorld", f32, 16),
    ("cameraWorldPos", u32, 8),
    ("orthoDepthConvertToView", f32, 4),
    ("renderDimension", f32, 4),
    ("frustumPlanesRS", f32, (6, 4)),
])
CAMERA_VIEW = np.dtype([
    ("translatedWorldToView", f32, 16),
    ("translatedWorldToClip", f32, 16),
    ("translatedWorldToClipLastFrame", f32, 16),
    ("renderDimension", f32, 4),
    ("cameraFovy", f32), ("zNear", f32), ("zFar", f32), ("lodScale", f32),
    ("clipToTranslatedWorldWithZFar_NoJitter", f32, 16),
])
CASCADE_CONFIG = np.dtype([
    ("cascadeCount", np.int32), ("realtimeCascadeCount", np.int32), ("cascadeDim", u32),
    ("cascadeStartDistance", f32), ("cascadeEndDistance", f32), ("farCascadeEndDistance", f32), ("splitLambda", f32),
    ("farCascadeSplitLambda", f32), ("shadowBiasConst", f32), ("shadowBiasSlope", f32), ("radiusScaleFixed", f32),
])


def default_cascade_config(**kw):
    """CascadeShadowMapConfig defaults (render_helper.h:467-483)."""
    c = np.zeros(1, dtype=CASCADE_CONFIG)
    c["cascadeCount"], c["realtimeCascadeCount"], c["cascadeDim"] = 8, 3, 2048
    c["cascadeStartDistance"], c["cascadeEndDistance"], c["farCascadeEndDistance"] = 0.0, 80.0, 800.0
    c["splitLambda"], c["farCascadeSplitLambda"], c["radiusScaleFixed"] = 0.8, 0.8, 10.0
    for k, v in kw.items():
        c[k] = v
    return c
DRAW_CMD = np.dtype([("objectId", u32), ("meshletId", u32), ("slot", u32)])

assert MESHLET.itemsize == 64 and MESHLET_GROUP.itemsize == 40 and PRIMITIVE.itemsize == 96 and BVH_NODE.itemsize == 60
assert MATERIAL.itemsize == 96 and OBJECT.itemsize == 224 and INSTANCE_CULLING_VIEW.itemsize == 288
assert CAMERA_VIEW.itemsize == 288 and DRAW_CMD.itemsize == 12 and CASCADE_CONFIG.itemsize == 44

FLAG_FRUSTUM_CULL = 1 << 0
FLAG_HZB_CULL = 1 << 1
FLAG_CONE_CULL = 1 << 2

# chordvis_query_bounds (ChordBoundsQuery / ChordBoundsResult)
BOUNDS_QUERY = np.dtype([
    ("localToTranslatedWorld", f32, 16),
    ("localToTranslatedWorldLastFrame", f32, 16),
    ("posMin", f32, 3), ("user", u32),
    ("posMax", f32, 3), ("pad", u32),
])
BOUNDS_RESULT = np.dtype([("status", u32), ("nearestZ", f32), ("rect", np.uint16, 4)])
assert BOUNDS_QUERY.itemsize == 160 and BOUNDS_RESULT.itemsize == 16
BOUNDS_IN_FRUSTUM, BOUNDS_UNOCCLUDED, BOUNDS_NEAR, BOUNDS_OFFSCREEN, BOUNDS_EMPTY_RECT = 1, 2, 4, 8, 16
BOUNDS_LEVEL_SHIFT, BOUNDS_LEVEL_MASK = 8, 0xF

# chordvis_bin_bounds (ChordBoundsTilesDesc / ChordBoundsTiles: four device pointers)
BOUNDS_TILES_DESC = np.dtype([("tileSize", u32), ("maxPerTile", u32), ("phase", u32), ("flags", u32)])
BOUNDS_TILES = np.dtype([("tileCounts", np.uint64), ("tileItems", np.uint64), ("tileDepth", np.uint64), ("totals", np.uint64)])
assert BOUNDS_TILES_DESC.itemsize == 16 and BOUNDS_TILES.itemsize == 32
BOUNDS_TILES_NEAR, BOUNDS_TILES_FAR = 1, 2

# chordvis_trace_rays (ChordRay / ChordRayHit)
RAY = np.dtype([("origin", f32, 3), ("tMin", f32), ("direction", f32, 3), ("tMax", f32)])
RAY_HIT = np.dtype([("t", f32), ("u", f32), ("v", f32), ("object", u32), ("meshlet", u32), ("triangle", u32), ("primitive", u32), ("status", u32)])
assert RAY.itemsize == 32 and RAY_HIT.itemsize == 32
# chordvis_readback_ray_tlas (ChordRayNode): a 4-wide TLAS node, the boxes of its children axis by axis
RAY_NODE = np.dtype([("lo", f32, (3, 4)), ("hi", f32, (3, 4)), ("child", u32, 4), ("parentRef", u32), ("childCount", u32), ("pad", u32, 2)])
assert RAY_NODE.itemsize == 128
# chordvis_shade_ray_hits (ChordRayHitSurface): sixteen words per hit, an invalid hit all zero
RAY_HIT_SURFACE = np.dtype([("baseColor", f32, 4), ("emissive", f32, 3), ("roughness", f32), ("normal", f32, 3), ("metallic", f32),
                            ("uv", f32, 2), ("material", u32), ("flags", u32)])
assert RAY_HIT_SURFACE.itemsize == 64

HZB_MAX_MIPS = 12


class AssetDesc(C.Structure):
    _fields_ = [
        ("meshlets", C.c_void_p), ("meshletCount", C.c_uint32),
        ("meshletGroups", C.c_void_p), ("meshletGroupCount", C.c_uint32),
        ("meshletGroupIndices", C.c_void_p), ("meshletGroupIndexCount", C.c_uint32),
        ("meshletData", C.c_void_p), ("meshletDataCount", C.c_uint32),
        ("positions", C.c_void_p), ("vertexCount", C.c_uint32),
        ("texcoord0", C.c_void_p), ("texcoord0Count", C.c_uint32),
        ("bvhNodes", C.c_void_p), ("bvhNodeCount", C.c_uint32),
        ("normals", C.c_void_p), ("normalCount", C.c_uint32),
        ("tangents", C.c_void_p), ("tangentCount", C.c_uint32),
    ]


class SceneDesc(C.Structure):
    _fields_ = [
        ("objects", C.c_void_p), ("objectCount", C.c_uint32),
        ("primitives", C.c_void_p), ("primitiveCount", C.c_uint32),
        ("materials", C.c_void_p), ("materialCount", C.c_uint32),
        ("assets", C.POINTER(AssetDesc)), ("assetCount", C.c_uint32),
        ("textures", C.c_void_p), ("textureCount", C.c_uint32),
        ("samplers", C.c_void_p), ("samplerCount", C.c_uint32),
    ]


class Texture(C.Structure):
    _fields_ = [("rgba8", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("mipCount", C.c_uint32), ("format", C.c_uint32)]


# ChordTexture::format (CHORD_TEXFMT_*) and the bytes of a 4 x 4 block of the block formats
TEXFMT_RGBA8, TEXFMT_BC1_RGB, TEXFMT_BC3, TEXFMT_BC4, TEXFMT_BC5 = 0, 1, 2, 3, 4
BC_BLOCK_BYTES = {TEXFMT_BC1_RGB: 8, TEXFMT_BC3: 16, TEXFMT_BC4: 8, TEXFMT_BC5: 16}


SAMPLER = np.dtype([("minFilter", u32), ("magFilter", u32), ("wrapS", u32), ("wrapT", u32)])
ALPHA_OPAQUE, ALPHA_MASK, ALPHA_BLEND = 0, 1, 2
FILTER_NEAREST, FILTER_LINEAR = 9728, 9729
FILTER_NEAREST_MIPMAP_NEAREST, FILTER_LINEAR_MIPMAP_NEAREST, FILTER_NEAREST_MIPMAP_LINEAR, FILTER_LINEAR_MIPMAP_LINEAR = 9984, 9985, 9986, 9987
WRAP_REPEAT, WRAP_CLAMP_TO_EDGE, WRAP_MIRRORED_REPEAT = 10497, 33071, 33648


def mip_chain_rgba8(level0):
    """All mip levels of an (H, W, 4) uint8 image back to back (2x2 box filter, floor division; odd sizes drop the last
    row / column like a plain downsample), as ChordTexture::rgba8 wants them.  Returns (bytes array, mipCount)."""
    img = np.ascontiguousarray(level0, dtype=np.uint8)
    levels = [img]
    while img.shape[0] > 1 or img.shape[1] > 1:
        h, w = max(1, img.shape[0] // 2), max(1, img.shape[1] // 2)
        a = img[:h * 2 if img.shape[0] > 1 else 1, :w * 2 if img.shape[1] > 1 else 1].astype(np.uint32)
        if img.shape[0] > 1:
            a = a[0::2] + a[1::2]
        else:
            a = a * 2
        if img.shape[1] > 1:
            a = a[:, 0::2] + a[:, 1::2]
        else:
            a = a * 2
        img = ((a + 2) // 4).astype(np.uint8)
        levels.append(img)
    return np.concatenate([l.reshape(-1) for l in levels]), len(levels)


class TextureChain:
    """A texture handed to Scene(textures=...) as a finished chain: `data` holds every level back to back in the layout of
    ChordTexture (RGBA8 texels for format 0, 4 x 4 blocks for the TEXFMT_BC* formats), level 0 is width x height."""

    def __init__(self, data, width, height, mips, format=TEXFMT_RGBA8):
        self.data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        self.width, self.height, self.mips, self.format = int(width), int(height), int(mips), int(format)

    @property
    def shape(self):
        return (self.height, self.width, 4)


def level_dims(width, height, mips):
    """[(w, h)] of the levels of a chain."""
    return [(max(1, width >> l), max(1, height >> l)) for l in range(mips)]


def _channel_palette(a0, a1):
    """(n, 8) values of alpha / single-channel blocks with endpoints a0, a1 (int64 arrays)."""
    pal = np.zeros((len(a0), 8), dtype=np.int64)
    pal[:, 0], pal[:, 1] = a0, a1
    for k in range(2, 8):
        six = ((6 - k) * a0 + (k - 1) * a1) // 5 if k < 6 else np.full_like(a0, 0 if k == 6 else 255)
        pal[:, k] = np.where(a0 > a1, ((8 - k) * a0 + (k - 1) * a1) // 7, six)
    return pal


def _encode_channel(v, flip):
    """v (n, 16) one channel of n blocks -> (n, 8) block bytes: a0 = the block's maximum and a1 = its minimum (the eight-value
    mode), the other way round where `flip` (the six-value mode with its 0 and 255), every texel the nearest value."""
    v = v.astype(np.int64)
    hi, lo = v.max(axis=1), v.min(axis=1)
    a0, a1 = np.where(flip, lo, hi), np.where(flip, hi, lo)
    idx = np.abs(v[:, :, None] - _channel_palette(a0, a1)[:, None, :]).argmin(axis=2).astype(np.uint64)
    bits = np.zeros(len(v), dtype=np.uint64)
    for i in range(16):
        bits |= idx[:, i] << np.uint64(3 * i)
    out = np.zeros((len(v), 8), dtype=np.uint8)
    out[:, 0], out[:, 1] = a0, a1
    for j in range(6):
        out[:, 2 + j] = (bits >> np.uint64(8 * j)) & np.uint64(0xFF)
    return out


def _encode_colour(rgb):
    """rgb (n, 16, 3) -> (n, 8) colour block bytes: c0 = the block's per-channel maximum and c1 = its minimum in 5:6:5 (always
    c0 > c1: the four-colour mode), every texel the nearest of the four colours."""
    rgb = rgb.astype(np.int64)
    q = lambda c: ((c[:, 0] >> 3) << 11) | ((c[:, 1] >> 2) << 5) | (c[:, 2] >> 3)
    c0, c1 = q(rgb.max(axis=1)), q(rgb.min(axis=1))
    same = c0 == c1
    c1 = np.where(same & (c0 > 0), c0 - 1, c1)          # (a solid block: any second endpoint below the first)
    c0 = np.where(same & (c0 == 0), 1, c0)

    def expand(c):
        r, g, b = c >> 11, (c >> 5) & 63, c & 31
        return np.stack([(r << 3) | (r >> 2), (g << 2) | (g >> 4), (b << 3) | (b >> 2)], axis=1)
    p0, p1 = expand(c0), expand(c1)
    pal = np.stack([p0, p1, (2 * p0 + p1) // 3, (p0 + 2 * p1) // 3], axis=1)
    idx = ((rgb[:, :, None, :] - pal[:, None, :, :]) ** 2).sum(axis=3).argmin(axis=2).astype(np.uint32)
    bits = np.zeros(len(rgb), dtype=np.uint32)
    for i in range(16):
        bits |= idx[:, i] << np.uint32(2 * i)
    out = np.zeros((len(rgb), 8), dtype=np.uint8)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = c0 & 0xFF, c0 >> 8, c1 & 0xFF, c1 >> 8
    for j in range(4):
        out[:, 4 + j] = (bits >> np.uint32(8 * j)) & np.uint32(0xFF)
    return out


def encode_bc(level_rgba8, format):
    """A simple encoder for tests: the blocks (uint8, row-major, ceil(w / 4) x ceil(h / 4) of them) of one (h, w, 4) uint8 level in
    a TEXFMT_BC* format.  Bounding-box endpoints, nearest index; always well-formed, never the three-colour mode; quality is not a
    goal.  Channel blocks (BC3 alpha, BC4, BC5) alternate the order of a0 and a1 from block to block, so both of their modes occur.
    Edge blocks repeat the level's last row / column."""
    img = np.ascontiguousarray(level_rgba8, dtype=np.uint8)
    h, w = img.shape[:2]
    bh, bw = (h + 3) // 4, (w + 3) // 4
    img = np.pad(img, ((0, bh * 4 - h), (0, bw * 4 - w), (0, 0)), mode="edge")
    blocks = img.reshape(bh, 4, bw, 4, 4).transpose(0, 2, 1, 3, 4).reshape(-1, 16, 4)
    flip = (np.arange(len(blocks)) & 1).astype(bool)
    if format == TEXFMT_BC1_RGB:
        out = _encode_colour(blocks[:, :, :3])
    elif format == TEXFMT_BC3:
        out = np.concatenate([_encode_channel(blocks[:, :, 3], flip), _encode_colour(blocks[:, :, :3])], axis=1)
    elif format == TEXFMT_BC4:
        out = _encode_channel(blocks[:, :, 0], flip)
    elif format == TEXFMT_BC5:
        out = np.concatenate([_encode_channel(blocks[:, :, 0], flip), _encode_channel(blocks[:, :, 1], ~flip)], axis=1)
    else:
        raise ValueError("encode_bc: format %r is not a block format" % (format,))
    return np.ascontiguousarray(out).reshape(-1)


def bc_chain(image, format):
    """TextureChain of an (H, W, 4) uint8 image in a TEXFMT_BC* format: every level of mip_chain_rgba8, encoded by encode_bc."""
    chain, mips = mip_chain_rgba8(image)
    h, w = image.shape[:2]
    out, off = [], 0
    for lw, lh in level_dims(w, h, mips):
        out.append(encode_bc(chain[off:off + lw * lh * 4].reshape(lh, lw, 4), format))
        off += lw * lh * 4
    return TextureChain(np.concatenate(out), w, h, mips, format)


class HZBDesc(C.Structure):
    _fields_ = [
        ("srcWidth", C.c_uint32), ("srcHeight", C.c_uint32),
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("mipCount", C.c_uint32),
        ("mipOffset", C.c_uint32 * HZB_MAX_MIPS),
        ("totalTexels", C.c_uint32),
    ]

    def mip_dims(self, level):
        return max(1, self.width >> level), max(1, self.height >> level)

    def valid_dims(self, level):
        w, h = self.mip_dims(level)
        return (min(w, (((self.srcWidth - 1) >> 1) >> level) + 1),
                min(h, (((self.srcHeight - 1) >> 1) >> level) + 1))


class Scene:
    """Host-side scene: the reference's per-frame collected arrays, one asset.

    Holds numpy arrays alive and exposes a ctypes SceneDesc over them.

    With ONE asset the two numberings of a meshlet are one number: the index into `meshlets` is both the asset-relative id of
    ChordDrawCmd::meshletId / ChordRayHit::meshlet (what chordvis_readback_cmds, chordvis_trace_rays and chordvis_pixel_rays return
    and chordvis_shade_ray_hits reads) and the device's concatenated id.  A ChordSceneDesc of several assets tells them apart: the
    library concatenates the assets' streams and subtracts the asset's first meshlet wherever a record leaves it as asset-relative
    ("Two numberings of a meshlet"; tests/multi_asset.py builds such scenes out of several Scene).
    """

    def __init__(self, objects, primitives, materials, meshlets, groups, group_indices, meshlet_data, positions,
                 name="scene", texcoord0=None, textures=(), samplers=None, bvh_nodes=None, normals=None, tangents=None):
        """textures: sequence of (H, W, 4) uint8 images (mip chains are built here) or TextureChain entries (finished chains, also
        block-compressed: handed over as they are); samplers: SAMPLER records; normals (n, 3) and
        tangents (n, 4, w = handedness) float32 per vertex, or None (read only by chordvis_resolve_surface)."""
        self.name = name
        self.objects = np.ascontiguousarray(objects, dtype=OBJECT)
        self.primitives = np.ascontiguousarray(primitives, dtype=PRIMITIVE)
        self.materials = np.ascontiguousarray(materials, dtype=MATERIAL)
        self.meshlets = np.ascontiguousarray(meshlets, dtype=MESHLET)
        self.groups = np.ascontiguousarray(groups, dtype=MESHLET_GROUP)
        self.group_indices = np.ascontiguousarray(group_indices, dtype=u32)
        self.meshlet_data = np.ascontiguousarray(meshlet_data, dtype=u32)
        self.positions = np.ascontiguousarray(positions, dtype=f32).reshape(-1, 3)
        self.bvh_nodes = None if bvh_nodes is None else np.ascontiguousarray(bvh_nodes, dtype=BVH_NODE)
        self.texcoord0 = None if texcoord0 is None else np.ascontiguousarray(texcoord0, dtype=f32).reshape(-1, 2)
        self.normals = None if normals is None else np.ascontiguousarray(normals, dtype=f32).reshape(-1, 3)
        self.tangents = None if tangents is None else np.ascontiguousarray(tangents, dtype=f32).reshape(-1, 4)
        self.texture_images = list(textures)
        self._tex_chains = [(t.data, t.mips) if isinstance(t, TextureChain) else mip_chain_rgba8(t) for t in self.texture_images]
        self._textures = (Texture * max(1, len(self._tex_chains)))()
        for i, (chain, mips) in enumerate(self._tex_chains):
            t = self.texture_images[i]
            self._textures[i] = Texture(chain.ctypes.data, t.shape[1], t.shape[0], mips, t.format if isinstance(t, TextureChain) else TEXFMT_RGBA8)
        self.samplers = np.zeros(0, dtype=SAMPLER) if samplers is None else np.ascontiguousarray(samplers, dtype=SAMPLER)
        self._asset = AssetDesc(
            self.meshlets.ctypes.data, len(self.meshlets),
            self.groups.ctypes.data, len(self.groups),
            self.group_indices.ctypes.data, len(self.group_indices),
            self.meshlet_data.ctypes.data, len(self.meshlet_data),
            self.positions.ctypes.data, len(self.positions),
            self.texcoord0.ctypes.data if self.texcoord0 is not None else None, len(self.texcoord0) if self.texcoord0 is not None else 0,
            self.bvh_nodes.ctypes.data if self.bvh_nodes is not None else None, len(self.bvh_nodes) if self.bvh_nodes is not None else 0,
            self.normals.ctypes.data if self.normals is not None else None, len(self.normals) if self.normals is not None else 0,
            self.tangents.ctypes.data if self.tangents is not None else None, len(self.tangents) if self.tangents is not None else 0,
        )
        self._assets = (AssetDesc * 1)(self._asset)
        self.desc = SceneDesc(
            self.objects.ctypes.data, len(self.objects),
            self.primitives.ctypes.data, len(self.primitives),
            self.materials.ctypes.data, len(self.materials),
            self._assets, 1,
            C.cast(self._textures, C.c_void_p) if self._tex_chains else None, len(self._tex_chains),
            self.samplers.ctypes.data if len(self.samplers) else None, len(self.samplers),
        )

    def with_objects(self, objects=None, materials=None):
        """The same geometry, textures and samplers under other object / material records (shallow: arrays are shared)."""
        out = Scene(self.objects if objects is None else objects, self.primitives, self.materials if materials is None else materials,
                    self.meshlets, self.groups, self.group_indices, self.meshlet_data, self.positions, name=self.name,
                    texcoord0=self.texcoord0, textures=self.texture_images, samplers=self.samplers, bvh_nodes=self.bvh_nodes,
                    normals=self.normals, tangents=self.tangents)
        if hasattr(self, "local_to_world"):
            out.local_to_world = self.local_to_world
        return out

    # --- aggregate counts the reference keeps in PerframeCollected (scene_common.h) -------------
    @property
    def object_count(self):
        return len(self.objects)

    @property
    def lod0_meshlet_instances(self):
        """Upper bound of draw commands: every meshlet instance (all LODs) of every object."""
        prim = self.primitives[self.objects["GLTFPrimitiveDetail"]]
        per_prim = np.zeros(len(self.primitives), dtype=np.int64)
        for i, p in enumerate(self.primitives):
            g = self.groups[p["meshletGroupOffset"]: p["meshletGroupOffset"] + p["meshletGroupCount"]]
            per_prim[i] = int(g["meshletCount"].sum())
        del prim
        return int(per_prim[self.objects["GLTFPrimitiveDetail"]].sum())

    @property
    def group_instances(self):
        return int(self.primitives["meshletGroupCount"][self.objects["GLTFPrimitiveDetail"]].sum())

    def triangle_count_lod0(self):
        lod0 = self.meshlets["lod"] == 0
        tri = (self.meshlets["vertexTriangleCount"] >> 8) & 0xFF
        per_meshlet = np.where(lod0, tri, 0).astype(np.int64)
        # meshlets are laid out per primitive [meshletOffset, next)
        cs = np.concatenate([[0], np.cumsum(per_meshlet)])
        offs = self.primitives["meshletOffset"].astype(np.int64)
        ends = np.concatenate([offs[1:], [len(self.meshlets)]])
        per_prim = cs[ends] - cs[offs]
        return int(per_prim[self.objects["GLTFPrimitiveDetail"]].sum())
