/*
 * chordvis_types.h — the data contract of the visibility hot path.
 *
 * Plain-C restatement of the POD records the reference shares between its C++
 * host code and its HLSL kernels.  Byte layouts are identical to the reference
 * so a maintainer can hand the reference's own arrays across the C ABI:
 *
 *   ChordMeshlet              <- GPUGLTFMeshlet            install/resource/shader/gltf.h:38-51
 *   ChordMeshletGroup         <- GPUGLTFMeshletGroup       install/resource/shader/gltf.h:26-36
 *   ChordPrimitive            <- GLTFPrimitiveBuffer       install/resource/shader/gltf.h:65-91
 *   ChordMaterial             <- GLTFMaterialGPUData       install/resource/shader/gltf.h:118-153
 *   ChordObjectBasicData      <- GPUObjectBasicData        install/resource/shader/base.h:343-351
 *   ChordObject               <- GPUObjectGLTFPrimitive    install/resource/shader/base.h:353-360
 *   ChordInstanceCullingView  <- InstanceCullingViewInfo   install/resource/shader/base.h:121-135
 *   ChordDrawCmd              <- uint3 draw command        install/resource/shader/instance_culling.hlsl:28-33
 *
 * Matrices are glm column-major in memory (element (row r, col c) at m[c*4+r]);
 * the kernels read them with the HLSL convention M[r][c] == glm m[c][r]
 * (install/resource/shader/hzb_culling_generic.hlsl:78-80).
 *
 * What changes versus the reference: bindless buffer ids
 * (GLTFPrimitiveDatasBuffer, gltf.h:94-116) become plain pointers in
 * ChordAssetDesc, and the slice of PerframeCameraView (base.h:292-340) that the
 * path reads is restated as ChordCameraView.
 */
#ifndef CHORDVIS_TYPES_H
#define CHORDVIS_TYPES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* switchFlags bits — gltf.h:10-12 */
#define CHORD_FLAG_FRUSTUM_CULL   (1u << 0) /* kFrustumCullingEnableBit  */
#define CHORD_FLAG_HZB_CULL       (1u << 1) /* kHZBCullingEnableBit      */
#define CHORD_FLAG_CONE_CULL      (1u << 2) /* kMeshletConeCullEnableBit */

/* base.h:428-436 */
#define CHORD_MESHLET_MAX_VERTICES     255u
#define CHORD_MESHLET_MAX_TRIANGLES    128u
#define CHORD_GROUP_MAX_MESHLETS       4u
#define CHORD_HZB_MAX_MIPS             12u
#define CHORD_MAX_INSTANCE_ID          0xFFFFFFu /* kMaxInstanceIdCount, base.h:412 */

/* nanite_shared.hlsli:11-12 */
#define CHORD_ERROR_PIXEL_THRESHOLD    1.0f
#define CHORD_ERROR_RADIUS_ROOT        3e38f

/* base.h:442-444: sub-pixel precision of the raster the reference assumes */
#define CHORD_SUBPIXEL_BITS            8

typedef struct ChordMat4 { float m[16]; } ChordMat4;

typedef struct ChordMeshlet {
    float    posMin[3];
    uint32_t dataOffset;           /* u32 index into meshletData           */
    float    posMax[3];
    uint32_t vertexTriangleCount;  /* V & 0xff | T << 8   (gltf.h:60-62)   */
    float    coneAxis[3];
    float    coneCutOff;
    float    coneApex[3];
    uint32_t lod;
} ChordMeshlet;

typedef struct ChordMeshletGroup {
    float    clusterPosCenter[3];
    float    parentError;          /* FLT_MAX when un-parented (root)      */
    float    parentPosCenter[3];
    float    error;                /* -1 at LOD0                           */
    uint32_t meshletOffset;        /* into meshletGroupIndices             */
    uint32_t meshletCount;         /* <= 4                                 */
} ChordMeshletGroup;

/* GPUBVHNode -- gltf.h:16-24, built by buildBVHTree / flattenBVH (nanite_builder.cpp:215-416): an 8-wide tree over the
 * PARENTED cluster groups of a primitive, keyed on their parent-error spheres; `sphere` bounds the parent spheres of
 * every group in the node's subtree (nanite_builder.cpp:53-56), the root's own leaves are the un-parented groups.
 * Indices are relative to the primitive's first node / first group; nodes are in breadth-first order and the
 * primitive's groups in the order the nodes list them.  The reference uploads the tree and never walks it
 * (instance_culling.hlsl:96-99); chordvis_set_cull_mode(ctx, 1) does. */
#define CHORD_BVH_WIDTH 8u             /* kNaniteBVHLevelNodeCount, base.h:433 */
#define CHORD_BVH_MAX_LEVELS 14u       /* kNaniteMaxBVHLevelCount,  base.h:432 */
#define CHORD_BVH_NO_CHILD 0xFFFFFFFFu
typedef struct ChordBVHNode {
    float    sphere[4];
    uint32_t children[8];
    uint32_t bvhNodeCount;             /* nodes of the subtree, this one included */
    uint32_t leafMeshletGroupOffset;
    uint32_t leafMeshletGroupCount;
} ChordBVHNode;

typedef struct ChordPrimitive {
    float    posMin[3];
    uint32_t primitiveDatasBufferId;   /* index into ChordSceneDesc.assets */
    float    posMax[3];
    uint32_t vertexOffset;
    float    posAverage[3];
    uint32_t vertexCount;
    uint32_t meshletOffset;
    uint32_t color0Offset;
    uint32_t smoothNormalOffset;
    uint32_t textureCoord1Offset;
    uint32_t bvhNodeOffset;
    uint32_t meshletGroupOffset;
    uint32_t meshletGroupIndicesOffset;
    uint32_t meshletGroupCount;
    uint32_t lod0IndicesOffset;
    uint32_t lod0IndicesCount;
    uint32_t pad0;
    uint32_t pad1;
} ChordPrimitive;

typedef struct ChordMaterial {
    uint32_t alphaMode;
    float    alphaCutOff;
    uint32_t bTwoSided;
    uint32_t baseColorId;
    float    baseColorFactor[4];
    float    emissiveFactor[3];
    uint32_t emissiveTexture;
    float    metallicFactor;
    float    roughnessFactor;
    uint32_t metallicRoughnessTexture;
    uint32_t normalTexture;
    uint32_t baseColorSampler;
    uint32_t emissiveSampler;
    uint32_t normalSampler;
    uint32_t metallicRoughnessSampler;
    float    normalFactorScale;
    uint32_t bExistOcclusion;
    float    occlusionTextureStrength;
    uint32_t materialType;
} ChordMaterial;

typedef struct ChordObjectBasicData {
    ChordMat4 localToTranslatedWorld;
    ChordMat4 translatedWorldToLocal;
    ChordMat4 localToTranslatedWorldLastFrame;
    float     scaleExtractFromMatrix[4]; /* .w = max |scale| */
} ChordObjectBasicData;

typedef struct ChordObject {
    ChordObjectBasicData basicData;
    uint32_t GLTFPrimitiveDetail;  /* index into primitives */
    uint32_t GLTFMaterialData;     /* index into materials  */
    uint32_t pad1;
    uint32_t pad2;
} ChordObject;

typedef struct ChordInstanceCullingView {
    ChordMat4 translatedWorldToClip;
    ChordMat4 clipToTranslatedWorld;
    uint32_t  cameraWorldPos[8];          /* GPUStorageDouble4 */
    float     orthoDepthConvertToView[4];
    float     renderDimension[4];         /* w, h, 1/w, 1/h */
    float     frustumPlanesRS[6][4];      /* left, down, right, top, front, back (camera.h:10-18) */
} ChordInstanceCullingView;

/* The slice of PerframeCameraView (base.h:292-340) the path reads, plus the
 * one host-precomputed scalar the canonical arithmetic needs (lodScale). */
typedef struct ChordCameraView {
    ChordMat4 translatedWorldToView;
    ChordMat4 translatedWorldToClip;
    ChordMat4 translatedWorldToClipLastFrame;
    float     renderDimension[4];         /* w, h, 1/w, 1/h */
    float     cameraFovy;
    float     zNear;
    float     zFar;
    float     lodScale;                   /* (h * 0.5f) / tanf(0.5f * fovy), base.hlsli:503-518 */
    ChordMat4 clipToTranslatedWorldWithZFar_NoJitter;   /* camera.cpp:25-31: inverse of (perspectiveRH_ZO(fovy, aspect, zFar, zNear) * view);
                                                         * read by the cascade setup only (cascade_setup.hlsl:175) */
} ChordCameraView;

/* CascadeShadowMapConfig -- render_helper.h:462-484 (the fields the cascade setup and the depth passes read) */
typedef struct ChordCascadeConfig {
    int32_t  cascadeCount;            /* 8 */
    int32_t  realtimeCascadeCount;    /* 3 */
    uint32_t cascadeDim;              /* 2048 */
    float    cascadeStartDistance;    /* 0 */
    float    cascadeEndDistance;      /* 80 */
    float    farCascadeEndDistance;   /* 800 */
    float    splitLambda;             /* 0.8 */
    float    farCascadeSplitLambda;   /* 0.8 */
    float    shadowBiasConst;         /* 0 */
    float    shadowBiasSlope;         /* 0 */
    float    radiusScaleFixed;        /* 10 */
} ChordCascadeConfig;
#define CHORD_MAX_CASCADES 32u        /* the setup shader's group size (cascade_setup.hlsl:79) */

typedef struct ChordDrawCmd {
    uint32_t objectId;
    uint32_t meshletId;    /* index into the asset's meshlet array (primitive.meshletOffset applied) */
    uint32_t slot;         /* index in the post-instanceCulling list; the visibility payload */
} ChordDrawCmd;

/* GLTFMaterialGPUData::alphaMode -- EAlphaMode (asset_gltf.h:161; asset_gltf_material.cpp:703-705).  The visibility and
 * depth passes draw the opaque and the masked bucket; blended materials are in neither (mesh_raster.cpp:178,224). */
#define CHORD_ALPHA_OPAQUE 0u
#define CHORD_ALPHA_MASK   1u
#define CHORD_ALPHA_BLEND  2u

/* GLTFSampler (asset_gltf.h:9-39), the glTF enum values as the reference keeps them. */
#define CHORD_FILTER_NEAREST                 9728u
#define CHORD_FILTER_LINEAR                  9729u
#define CHORD_FILTER_NEAREST_MIPMAP_NEAREST  9984u
#define CHORD_FILTER_LINEAR_MIPMAP_NEAREST   9985u
#define CHORD_FILTER_NEAREST_MIPMAP_LINEAR   9986u
#define CHORD_FILTER_LINEAR_MIPMAP_LINEAR    9987u
#define CHORD_WRAP_REPEAT           10497u
#define CHORD_WRAP_CLAMP_TO_EDGE    33071u
#define CHORD_WRAP_MIRRORED_REPEAT  33648u
typedef struct ChordSampler {
    uint32_t minFilter, magFilter, wrapS, wrapT;
} ChordSampler;

/* A base-colour texture as the masked buckets read it (mesh_raster.hlsl:198-204: only .w of the sample is used):
 * RGBA8, `mipCount` levels back to back starting with level 0 (level l is max(1, width >> l) x max(1, height >> l)).
 * ChordMaterial::baseColorId / baseColorSampler index ChordSceneDesc::textures / samplers (the reference's bindless ids);
 * an id >= textureCount reads as the reference's white fallback (alpha 1, asset_gltf.cpp:374). */
/* ChordTexture::format.  0 is the layout above.  1..4 are the block formats the reference's material import stores its textures in
 * (asset_gltf_material.cpp:80-110; written by mipmapCompressBC1/3/4/5, asset_texture_helper.cpp, through stb_dxt): `rgba8` then
 * points at the blocks.  Level l is stored as ceil(w / 4) x ceil(h / 4) blocks, row-major, the levels back to back from level 0;
 * texels of an edge block that fall outside the level are ignored.  The library expands the blocks on the GPU at upload into the
 * same texel stores RGBA8 textures go to, by the pinned integer decode of DESIGN.md 2 item 9(h) (a fixed-function decoder may
 * differ by one code in the interpolated values); the format says nothing about sRGB (the resolve decides that per slot). */
#define CHORD_TEXFMT_RGBA8    0u
#define CHORD_TEXFMT_BC1_RGB  1u  /*  8 bytes per block: colour; alpha always 255 (the reference uses the _RGB_ formats) */
#define CHORD_TEXFMT_BC3      2u  /* 16 bytes per block: alpha block, then a colour block (always four-colour mode)      */
#define CHORD_TEXFMT_BC4      3u  /*  8 bytes per block: one channel block -> (v, 0, 0, 255)                             */
#define CHORD_TEXFMT_BC5      4u  /* 16 bytes per block: two channel blocks -> (r, g, 0, 255)                            */
typedef struct ChordTexture {
    const uint8_t* rgba8;      /* the texels, or the blocks of a CHORD_TEXFMT_BC* chain */
    uint32_t width, height, mipCount, format;
} ChordTexture;

/* One GLTFPrimitiveDatasBuffer (gltf.h:94-116): bindless ids -> host pointers. */
typedef struct ChordAssetDesc {
    const ChordMeshlet*      meshlets;           uint32_t meshletCount;
    const ChordMeshletGroup* meshletGroups;      uint32_t meshletGroupCount;
    const uint32_t*          meshletGroupIndices;uint32_t meshletGroupIndexCount;
    const uint32_t*          meshletData;        uint32_t meshletDataCount;  /* u32 words */
    const float*             positions;          uint32_t vertexCount;       /* float3 tightly packed */
    const float*             texcoord0;          uint32_t texcoord0Count;    /* float2 per vertex (textureCoord0Buffer), or NULL / 0:
                                                                              * masked materials then sample at uv (0, 0) */
    const ChordBVHNode*      bvhNodes;           uint32_t bvhNodeCount;      /* bvhNodeBuffer, or NULL / 0 (flat culling only);
                                                                              * primitive p's tree starts at bvhNodeOffset */
    const float*             normals;            uint32_t normalCount;       /* float3 per vertex (normalBuffer), or NULL / 0 */
    const float*             tangents;           uint32_t tangentCount;      /* float4 per vertex (tangentBuffer: xyz, handedness
                                                                              * w = +-1), or NULL / 0.  Read only by
                                                                              * chordvis_resolve_surface */
} ChordAssetDesc;

typedef struct ChordSceneDesc {
    const ChordObject*    objects;    uint32_t objectCount;
    const ChordPrimitive* primitives; uint32_t primitiveCount;
    const ChordMaterial*  materials;  uint32_t materialCount;
    const ChordAssetDesc* assets;     uint32_t assetCount;
    const ChordTexture*   textures;   uint32_t textureCount;   /* may be NULL / 0 */
    const ChordSampler*   samplers;   uint32_t samplerCount;   /* may be NULL / 0: REPEAT, NEAREST */
} ChordSceneDesc;

/* Visibility texel — base.hlsli:437-447 (low 32 bits) under the depth bits
 * (high 32 bits, D32 reverse-Z of render_textures.h:25). 0 == empty. */
static inline uint32_t chord_encode_triangle_instance(uint32_t triangleId, uint32_t instanceId)
{
    return (((instanceId + 1u) & CHORD_MAX_INSTANCE_ID) << 8) | (triangleId & 0xFFu);
}
static inline void chord_decode_triangle_instance(uint32_t pack, uint32_t* triangleId, uint32_t* instanceId)
{
    *triangleId = pack & 0xFFu;
    *instanceId = ((pack >> 8) & CHORD_MAX_INSTANCE_ID) - 1u;
}

/* HZB chain geometry — hzb.cpp:49-63.  mip l has (w0 >> l, h0 >> l) texels
 * (min 1), stored as IEEE binary16, mips back to back, each row-major. */
typedef struct ChordHZBDesc {
    uint32_t srcWidth, srcHeight;
    uint32_t width, height;        /* mip 0 extent */
    uint32_t mipCount;
    uint32_t mipOffset[CHORD_HZB_MAX_MIPS]; /* in texels from the chain base */
    uint32_t totalTexels;
} ChordHZBDesc;

/* chordvis_query_bounds (chordvis.h): one host-owned box, and what the frustum and occlusion tests said about it. */
typedef struct ChordBoundsQuery {               /* 160 bytes, DEVICE memory, caller-owned, 16-byte aligned */
    ChordMat4 localToTranslatedWorld;           /* as ChordObject::basicData's (chordvis_object_basic_data makes them) */
    ChordMat4 localToTranslatedWorldLastFrame;  /* read by phase 0 only */
    float posMin[3]; uint32_t user;             /* local-space box; `user` is carried, never read */
    float posMax[3]; uint32_t pad;              /* 0 */
} ChordBoundsQuery;

#define CHORD_BOUNDS_IN_FRUSTUM  1u    /* the object-stage frustum test keeps it                                   */
#define CHORD_BOUNDS_UNOCCLUDED  2u    /* the main-view occlusion test keeps it                                    */
#define CHORD_BOUNDS_NEAR        4u    /* !(max z < 1 && min z > 0): kept untested, as the reference does          */
#define CHORD_BOUNDS_OFFSCREEN   8u    /* z in range, uv box outside [0,1]^2: rejected before any tap             */
#define CHORD_BOUNDS_EMPTY_RECT 16u    /* rz < rx || rw < ry: covers no pixel, rejected                            */
/* bits 8..11: the HZB level tapped (0 when nothing was tapped) */
#define CHORD_BOUNDS_LEVEL_SHIFT 8u
#define CHORD_BOUNDS_LEVEL_MASK  0xFu

typedef struct ChordBoundsResult {              /* 16 bytes, 16-byte aligned */
    uint32_t status;
    float    nearestZ;      /* max projected z of the 8 corners (reverse-Z: nearest); 1.0f with NEAR */
    uint16_t rect[4];       /* rx, ry, rz, rw: the inclusive pixel rectangle the test formed; (0, 0, W-1, H-1) with NEAR */
} ChordBoundsResult;

/* chordvis_bin_bounds (chordvis.h): the visible boxes of a ChordBoundsResult array binned into screen tiles. */
#define CHORD_BOUNDS_TILES_NEAR 1u   /* near-side depth test on */
#define CHORD_BOUNDS_TILES_FAR  2u   /* far-side depth test on (needs deviceQueries) */

typedef struct ChordBoundsTilesDesc {           /* 16 bytes */
    uint32_t tileSize;     /* 8, 16, 32 or 64 pixels */
    uint32_t maxPerTile;   /* stride of tileItems per tile; 0 allowed only when tileItems is NULL */
    uint32_t phase;        /* 0 or 1: the phase the results were made with (read by the far side only) */
    uint32_t flags;        /* CHORD_BOUNDS_TILES_*; other bits refused */
} ChordBoundsTilesDesc;

typedef struct ChordBoundsTiles {               /* caller-owned DEVICE memory, NULL = not wanted; at least one non-NULL */
    uint32_t* tileCounts;  /* [tiles]               */
    uint32_t* tileItems;   /* [tiles * maxPerTile]  */
    uint32_t* tileDepth;   /* [tiles * 2]: far bits, near bits */
    uint32_t* totals;      /* [4] */
} ChordBoundsTiles;

/* chordvis_trace_rays (chordvis.h RAY QUERIES): caller-owned DEVICE records, 16-byte aligned, moved as 16-byte vectors. */
typedef struct ChordRay {                       /* 32 bytes */
    float origin[3];    float tMin;             /* translated-world (camera-relative) space of the object records the frames read now */
    float direction[3]; float tMax;             /* need not be normalised; t is the parameter along it (base.h:439-440: 1e-2 .. 1e9 by default) */
} ChordRay;

#define CHORD_RAY_HIT        1u    /* ChordRayHit::status bit 0                                                   */
#define CHORD_RAY_BACK_FACE  2u    /* bit 1: det < 0 in the triangle test (the ray meets the clockwise side)      */
typedef struct ChordRayHit {                    /* 32 bytes; a miss is eight zero words */
    float    t, u, v;          /* v0 + u (v1 - v0) + v (v2 - v0) is the point; t along the ray's own direction      */
    uint32_t object;           /* index in the current object list                                                  */
    uint32_t meshlet;          /* index into the asset's meshlets (ChordDrawCmd::meshletId's numbering)              */
    uint32_t triangle;         /* index within the meshlet                                                          */
    uint32_t primitive;        /* the object's GLTFPrimitiveDetail                                                  */
    uint32_t status;           /* CHORD_RAY_HIT | CHORD_RAY_BACK_FACE                                               */
} ChordRayHit;

#define CHORD_RAY_ANY_HIT    1u    /* chordvis_trace_rays flags: only status bit 0 is written, the other seven words are zero */
#define CHORD_RAY_MAX_DEPTH  12u   /* interior levels of one tree (BLAS or TLAS) the traversal stack is sized for */

/* chordvis_rebuild_ray_tlas / chordvis_readback_ray_tlas (chordvis.h RAY QUERIES, "rebuilding the TLAS"). */
#define CHORD_RAY_TLAS_GROUP_MAX 4096u   /* object lists up to this long are rebuilt by one workgroup (two launches, the refit included) */
#define CHORD_RAY_TLAS_NODE  0u    /* bits 31..30 of a ChordRayNode child word: bits 29..0 index a TLAS node ...  */
#define CHORD_RAY_TLAS_LEAF  1u    /* ... or an object of the current list                                        */
#define CHORD_RAY_NO_CHILD   0xFFFFFFFFu
typedef struct ChordRayNode {                   /* 128 bytes: a 4-wide node holds the boxes of its children, axis by axis */
    float    lo[3][4];         /* [axis][child]; an unused slot: +inf                                               */
    float    hi[3][4];         /* an unused slot: -inf                                                              */
    uint32_t child[4];         /* tag << 30 | index; an unused slot: CHORD_RAY_NO_CHILD                             */
    uint32_t parentRef;        /* parent node * 4 + the slot this node's box lives in; CHORD_RAY_NO_CHILD: the root */
    uint32_t childCount;       /* 1..4: slots 0 .. childCount - 1 are used                                          */
    uint32_t pad[2];
} ChordRayNode;

/* chordvis_shade_ray_hits (chordvis.h RAY QUERIES, "shading a hit"): one record per ChordRayHit. */
#define CHORD_RAYSURF_VALID      1u   /* ChordRayHitSurface::flags bit 0: the record is filled (an invalid hit: sixteen zero words)  */
#define CHORD_RAYSURF_BACK_FACE  2u   /* copied from the hit's CHORD_RAY_BACK_FACE                                                */
#define CHORD_RAYSURF_TWO_SIDED  4u   /* the material's bTwoSided                                                                 */
#define CHORD_RAYSURF_PBR        8u   /* materialType == 1: the material fields are filled                                        */
typedef struct ChordRayHitSurface {             /* 64 bytes, 16-byte aligned, moved as four 16-byte vectors; an invalid hit is sixteen zero words */
    float    baseColor[4];     /* rgb through sRGB -> AP1, alpha                                                     */
    float    emissive[3];      /* NOT through sRGB -> AP1                                                            */
    float    roughness;
    float    normal[3];        /* translated-world space, unit length or zero; flipped on a back face of a two-sided material */
    float    metallic;
    float    uv[2];
    uint32_t material;         /* the object's GLTFMaterialData                                                      */
    uint32_t flags;            /* CHORD_RAYSURF_*                                                                    */
} ChordRayHitSurface;

/* chordvis_pixel_rays (chordvis.h RAY QUERIES, "pixel rays"): one ray per pixel of caller-owned position and normal images. */
#define CHORD_PIXEL_RAYS_HEMISPHERE        0u   /* ChordPixelRaysDesc::mode: a tangent-space direction per pixel from the table (gi_rt_ao.hlsl) */
#define CHORD_PIXEL_RAYS_DIRECTION         1u   /* one direction for every pixel (a sun shadow ray)                                             */
#define CHORD_PIXEL_RAYS_ANY_HIT           1u   /* ChordPixelRaysDesc::flags: out = 0 when a candidate exists, 1 otherwise; no hit records       */
#define CHORD_PIXEL_RAYS_FRONT_ONLY        2u   /* DIRECTION only: a pixel whose normal does not face the direction traces nothing, out = 0      */
#define CHORD_PIXEL_RAYS_START_FROM_DEPTH  4u   /* tMin from the pixel's device depth and zNear (getRayTraceStartOffset); needs deviceZ          */
typedef struct ChordPixelRaysDesc {             /* 64 bytes */
    uint32_t width, height;    /* of the position, normal, depth and output images, row-major, no padding between rows */
    uint32_t mode, flags;      /* CHORD_PIXEL_RAYS_*                                                                   */
    uint32_t tableW, tableH;   /* HEMISPHERE: the direction table's size, powers of two                                */
    uint32_t deviceZStride;    /* in floats: 1 a D32 image, 2 the depth halves of 64-bit visibility words              */
    uint32_t pad;
    float    direction[3];     /* DIRECTION: translated-world space, need not be normalised                            */
    float    rayLength, tMin, zNear, pad2[2];
} ChordPixelRaysDesc;

typedef struct ChordRaySceneInfo {              /* 64 bytes */
    uint32_t blasCount;        /* primitives of the uploaded scene (an empty BLAS counts)                           */
    uint32_t blasNodes;        /* 128-byte nodes of all BLASes                                                       */
    uint32_t blasTriangles;    /* 48-byte triangle records of all BLASes = the scene's LOD-0 triangles               */
    uint32_t blasBuilt;        /* BLASes the chordvis_build_ray_scene call that filled this built (0: they were kept) */
    uint32_t blasMaxDepth;     /* interior levels of the deepest BLAS                                                */
    uint32_t tlasNodes;
    uint32_t tlasDepth;
    uint32_t pad;
    uint64_t deviceBytes;      /* of the whole ray scene                                                             */
    float    rootMin[3];       /* the TLAS root's box after the latest refit the device has finished                 */
    float    rootMax[3];
} ChordRaySceneInfo;

#ifdef __cplusplus
}
static_assert(sizeof(ChordRay) == 32 && sizeof(ChordRayHit) == 32 && sizeof(ChordRaySceneInfo) == 64, "ray records");
static_assert(sizeof(ChordRayHitSurface) == 64, "ChordRayHitSurface");
static_assert(sizeof(ChordRayNode) == 128, "ChordRayNode");
static_assert(sizeof(ChordPixelRaysDesc) == 64, "ChordPixelRaysDesc");
static_assert(sizeof(ChordBoundsTilesDesc) == 16, "ChordBoundsTilesDesc");
static_assert(sizeof(ChordBoundsQuery) == 160, "ChordBoundsQuery");
static_assert(sizeof(ChordBoundsResult) == 16, "ChordBoundsResult");
static_assert(sizeof(ChordMeshlet) == 64, "GPUGLTFMeshlet");
static_assert(sizeof(ChordMeshletGroup) == 40, "GPUGLTFMeshletGroup");
static_assert(sizeof(ChordBVHNode) == 60, "GPUBVHNode");
static_assert(sizeof(ChordPrimitive) == 96, "GLTFPrimitiveBuffer");
static_assert(sizeof(ChordMaterial) == 96, "GLTFMaterialGPUData");
static_assert(sizeof(ChordObjectBasicData) == 208, "GPUObjectBasicData");
static_assert(sizeof(ChordObject) == 224, "GPUObjectGLTFPrimitive");
static_assert(sizeof(ChordInstanceCullingView) == 288, "InstanceCullingViewInfo");
static_assert(sizeof(ChordDrawCmd) == 12, "uint3 draw cmd");
#endif

#endif /* CHORDVIS_TYPES_H */
