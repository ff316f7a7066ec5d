/*
 * chordvis.h — C ABI of the MI355X-native visibility hot path (libchordvis.so).
 *
 * The reference has no plugin/FFI boundary for this path: its boundary is the
 * free-function pass surface of source/renderer (gltf_rendering.h:37-108,
 * postprocessing.h:41-54) called from DeferredRenderer::render
 * (renderer.cpp:319-345), sitting on the Vulkan device layer of
 * source/graphics.  Every entry point below names the reference interface it
 * replaces.  Signatures carry plain pointers and sizes only; device memory is
 * named by raw device pointers (the counterpart of the reference's bindless
 * uint32 ids obtained from asSRV/asUAV, render_helper.h:290-359).
 *
 * Conventions
 *  - every function returns 0 on success, a negative CHORDVIS_E_* code otherwise;
 *    chordvis_last_error(ctx) returns the message (reference: check()/
 *    checkVkResult() assert + log, utils.h:57-72, graphics/common.h:337).
 *  - one host thread per context; all passes are enqueued on the context's HIP
 *    stream in call order and never synchronize the host (reference: one
 *    graphics queue, one vkQueueSubmit per frame, command_list.cpp:107-153).
 *  - handles (ChordCountAndCmd, ChordHZB) point into context-owned device
 *    memory and stay valid until the next chordvis_instance_culling /
 *    chordvis_build_hzb into the same slot (reference: pooled buffers recycled
 *    after N frames, buffer_pool.cpp:71,122).
 */
#ifndef CHORDVIS_H
#define CHORDVIS_H

#include "chordvis_types.h"

#ifdef __cplusplus
extern "C" {
#endif
/* libchordvis.so is built with -fvisibility=hidden: the entry points declared in this header are its ONLY dynamic symbols (the
 * library's C++ internals live in a namespace `chord`, which is also the reference's -- a host must never see them). */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define CHORDVIS_OK              0
#define CHORDVIS_E_INVALID      -1   /* bad argument / call order            */
#define CHORDVIS_E_HIP          -2   /* a HIP runtime call failed            */
#define CHORDVIS_E_NO_DEVICE    -3   /* no usable gfx950 device              */
#define CHORDVIS_E_CAPACITY     -4   /* scene exceeds a documented limit     */
#define CHORDVIS_E_COMM         -5   /* RCCL missing / a collective failed   */

typedef struct ChordCtx ChordCtx;

/* CountAndCmdBuffer — postprocessing.h:48.  Device pointers. */
typedef struct ChordCountAndCmd {
    uint32_t*     count;     /* device: number of valid commands           */
    ChordDrawCmd* cmds;      /* device: uint3 commands                     */
    uint32_t      capacity;  /* commands the buffer can hold               */
} ChordCountAndCmd;

/* HZBContext — render_helper.h:411-451.  Device pointers into one f16 chain per channel. */
typedef struct ChordHZB {
    ChordHZBDesc desc;
    uint16_t*    minTexels;   /* device, desc.totalTexels halves, or NULL    */
    uint16_t*    maxTexels;   /* device or NULL                              */
    uint32_t*    validRange;  /* device uint2 {asuint(min), asuint(max)} or NULL */
} ChordHZB;

/* Work-list capacities (the counterpart of the reference's pool sizes); zero fields keep the default.  Call before
 * chordvis_upload_scene / chordvis_allocate_gbuffer.  The record lists are sized FROM THE SCENE at upload
 * (2 x its instanced triangles + 256 Ki, chordvis_abi.cpp alloc_scene_work_buffers) and capped by these limits; the default
 * caps fit BASELINE configs 1-4 and config 5 with pixel blocks; config 5 in the record form (1 G sub-pixel triangles in one
 * pass, debug only) needs ~1.1 G records and ~1.1 M pool chunks per pass. */
typedef struct ChordLimits {
    uint64_t maxTriangleRecords;   /* upper bound of the 32-byte record list (the 48-byte list gets a quarter, at least 1 Mi); default cap 64 Mi */
    uint32_t binPoolChunks;        /* 1024-entry overflow chunks per raster pass; default 32 Ki */
    uint32_t binMaxChunksPerTile;  /* default 240, at most 3072 */
} ChordLimits;

/* VisibilityTileMarkerContext — visibility_tile.h:11-19.  One uint4 (128 shading-type bits) per 8x8 pixels. */
typedef struct ChordTileMarker {
    uint32_t* marker;            /* device, 4 words per texel, markerDim[0] x markerDim[1] texels, row-major */
    uint32_t  visibilityDim[2];
    uint32_t  markerDim[2];      /* ceil(visibilityDim / 8), visibility_tile.cpp:31 */
} ChordTileMarker;

/* VisibilityTileContxt — visibility_tile.h:29-33 */
typedef struct ChordShadingTiles {
    uint32_t* tileCmd;           /* device uint2 per tile: pixel origin of an 8x8 tile; order unspecified (as in the reference) */
    uint32_t* count;             /* device: number of tiles */
    uint32_t* dispatchIndirect;  /* device uint4 {(count + 3) / 4, 1, 1, 1} */
    uint32_t  capacity;          /* markerDim[0] * markerDim[1] */
} ChordShadingTiles;

/* Camera inputs of ICamera (camera.h:22-139) + ViewportCamera::updateMatrixMisc (viewport.cpp:434-445). */
typedef struct ChordCameraDesc {
    double   position[3];
    double   front[3];
    double   worldUp[3];
    float    fovy;          /* radians */
    float    jitter[2];     /* PerframeCameraView::jitterData.xy, pixels in (-0.5, 0.5) */
    double   zNear;
    double   zFar;
    uint32_t width, height;
} ChordCameraDesc;

/* GPU timestamps — the labels DeferredRenderer::render inserts (renderer.cpp:322-344). */
typedef struct ChordStats {
    float    msClear;              /* "Clear GBuffers"                   */
    float    msInstanceCulling;    /* "GLTF Instance Culling"            */
    float    msStage0;             /* "GLTF Visibility Stage0"           */
    float    msHzbStage0;          /* "BuildHZB Post Prepass Stage0"     */
    float    msStage1;             /* "GLTF Visibility Stage1"           */
    float    msHzbFinal;           /* "BuildHZB"                         */
    float    msFrame;              /* clear .. final HZB                 */
    float    msRasterCluster;      /* sum over the frame's raster_setup_kernel launches (per-meshlet setup + binning) */
    float    msRasterClip;         /* ... raster_clip_and_bin_large_kernel + raster_tile_order_kernel                 */
    float    msRasterChunk;        /* ... raster_tile_kernel (per-tile resolve in LDS, tile-out, fused HZB mips 0-5)  */
    uint32_t framesTimed;          /* frames the ms* fields are averaged over               */
    uint32_t rasterLaunches;       /* renderMesh calls this frame (1 or 2)                  */
    uint32_t overflow;             /* non-zero: a deferred raster list overflowed (results invalid) */
    uint32_t countInstanceCulled;  /* commands after instanceCulling     */
    uint32_t countStage0Visible;
    uint32_t countStage0Rejected;
    uint32_t countStage1Visible;
    uint64_t trianglesSubmitted;   /* sum of meshlet triangle counts of rastered commands */
    uint64_t triangleRecords;      /* set-up triangles that survived the per-triangle culls (this frame)  */
    uint64_t binEntries;           /* (triangle, 64x64 tile) pairs binned (this frame, both raster passes) */
    uint32_t tilesTouched[2];      /* 64x64 tiles with at least one bin entry, per raster pass            */
    uint64_t triangleRecordsCompact; /* of triangleRecords, those in the 32-byte form (the rest take 48 bytes) */
    uint64_t pixelBlockBytes;      /* bytes of pixel blocks emitted for small clusters in place of records (this frame); their
                                      triangles are not in triangleRecords, a block counts as one bin entry per tile */
    uint64_t pixelBlocks;          /* number of those blocks (= their bin entries; on frames with hot tiles, plus the bin slots the block
                                      kernel drew ahead and left empty -- a few per wave and hot tile) */
    float    msExchangeHzb;        /* sharded frames: stream time between phase a and phase b = the all-gather of the HZB mip-0 exchange buffer */
    float    msExchangeVis;        /* ... between phase b and phase c = the all-gather of the visibility words (incl. waiting for the slowest rank) */
    float    msExchangeCull;       /* ... between phase cull and phase a = the all-gather of the group cull's rank masks (sharded cull) */
    float    msExchangeFinal;      /* ... library-run frames (chordvis_comm_*, ChordGroup): the small end-of-frame exchange, stamped apart from the image
                                      gather (msExchangeVis is then the image alone); 0 when the host drives the phases */
    uint32_t kernelLaunches;       /* kernel launches of the last finished frame (a sub-millisecond frame is bounded by launches x launch floor) */
    uint32_t largeRecords[2];      /* per raster pass: records touching more than 2 x 2 tiles (binned by the large-record binner, or tested by the tiles themselves) */
    uint32_t clipTriangles[2];     /* per raster pass: triangles that went through the homogeneous clipper */
    float    stampsPerFrame;       /* event records per stamped frame behind the ms* fields (0: no timers).  A record between two kernels keeps the
                                      second from being dispatched under the first: every stamped interval is a few microseconds longer than its
                                      kernels, a stamped frame that many x this longer than an unstamped one (bench.py: roofline.stamp_cost_us) */
} ChordStats;

/* ------------------------------------------------------------------ host-only (no device needed) */

const char* chordvis_version(void);

/* hzb.cpp:49-63 — extent / mip count / offsets of the HZB chain for a render size. */
int chordvis_hzb_desc(uint32_t srcWidth, uint32_t srcHeight, ChordHZBDesc* out);

/* ICamera::fillViewUniformParameter (camera.cpp:17-78), ICamera::computeRelativeWorldFrustum
 * (camera.cpp:80-154), infiniteInvertZPerspectiveRH_ZO (utils.cpp:186-198) and the main-view
 * InstanceCullingViewInfo fill of DeferredRenderer::render (renderer.cpp:175-263).
 * lastFrame may be NULL (first frame: last-frame matrices = current). */
int chordvis_camera_fill_view(const ChordCameraDesc* camera, const ChordCameraView* lastFrame,
                              ChordCameraView* outView, ChordInstanceCullingView* outInstanceView);

/* cascadeComputeCS (cascade_setup.hlsl:79-372, driven by renderShadow mesh_raster.cpp:417-441): the InstanceCullingViewInfo of
 * every shadow cascade -- log / uniform split of the view range (SDSM-tightened for the realtime cascades when the valid
 * depth range of the last buildHZB is given), bounding sphere, light-space lookAt + reverse-Z ortho projection snapped
 * to whole texels, frustum planes.  Host code: the reference runs it on the GPU only to read the depth range without a
 * readback; validDepthMinMax NULL takes the shader's own no-range branch (:118).  views[] is in/out: cascades whose
 * cache is still valid (isCascadeCacheValid, :8-22) are left untouched. */
int chordvis_cascade_setup(const ChordCascadeConfig* config, const ChordCameraView* view, const ChordInstanceCullingView* mainInstanceView,
                           const float lightDir[3], const uint32_t validDepthMinMax[2], uint32_t tickCount, int bCacheValid,
                           ChordInstanceCullingView* views /* [config->cascadeCount] */);

/* SceneNode::getObjectBasicData (scene_node.cpp:42-90): camera-relative f64 -> f32 transforms.
 * Matrices are glm column-major doubles. */
int chordvis_object_basic_data(const double localToWorld[16], const double prevLocalToWorld[16],
                               const double cameraPos[3], const double cameraPosLast[3],
                               ChordObjectBasicData* out);
/* Batched form: fills objects[i].basicData for i < count (ids/pads untouched).
 * prevLocalToWorld / cameraPosLast may be NULL (static object / camera). */
int chordvis_object_basic_data_batch(uint32_t count, const double* localToWorld /*count*16*/,
                                     const double* prevLocalToWorld, const double cameraPos[3],
                                     const double cameraPosLast[3], ChordObject* objects);

/* ------------------------------------------------------------------ producer of the input format (host-only, offline)
 * NaniteBuilder::build (nanite_builder.cpp:882-921): LOD-0 meshlets, up to 11 rounds of group / merge / simplify / split
 * with the simplification error handed up the DAG, cluster groups of at most 4 meshlets, the 8-wide BVH; packed like
 * asset_gltf_helper.cpp:496-548.  The clusterizer, the graph partition and the simplifier are this library's own (the
 * reference calls meshoptimizer and METIS), so the meshlets differ from the reference's for the same mesh; the format and
 * its invariants are the same (nanite_builder.cpp).  Indices: triangle list; texcoord0 may be NULL. */
typedef struct ChordBuiltAsset ChordBuiltAsset;
int chordvis_nanite_build(const float* positions, uint32_t vertexCount, const uint32_t* indices, uint32_t indexCount,
                          const float* texcoord0, ChordBuiltAsset** outAsset);
/* The same build carrying per-vertex normals (float3) and tangents (float4, w = handedness) along: the simplifier collapses onto
 * existing vertices, so every LOD's vertices are input vertex ids and the attributes ride along by id.  Meshlets, groups, BVH and
 * meshlet data are byte for byte chordvis_nanite_build's for the same mesh.  normals / tangents may be NULL. */
int chordvis_nanite_build_attributes(const float* positions, uint32_t vertexCount, const uint32_t* indices, uint32_t indexCount,
                                     const float* texcoord0, const float* normals, const float* tangents, ChordBuiltAsset** outAsset);
/* bounds + normal cone of ONE meshlet as the builder computes them (posMin/posMax, coneAxis, coneCutOff, coneApex of `out`;
 * the reference: meshopt_computeMeshletBounds, nanite_builder.cpp:476-486).  positions: the meshlet's own <= 255 vertices;
 * localTriangles: 3 indices into them per triangle (<= 128 triangles). */
int chordvis_meshlet_bounds(const float* positions, uint32_t vertexCount, const uint8_t* localTriangles, uint32_t triangleCount, ChordMeshlet* out);
/* views into the built arrays (valid until chordvis_free_built_asset): one ChordAssetDesc holding one primitive */
int chordvis_built_asset_desc(const ChordBuiltAsset* asset, ChordAssetDesc* outAsset, ChordPrimitive* outPrimitive, uint32_t* outLodCount);
void chordvis_free_built_asset(ChordBuiltAsset* asset);
/* a flat container for a built asset (the reference: cereal + LZ4 archives, serialize.h:217-320): layout CHRDAS01, or CHRDAS02
 * (two more counts and the normal / tangent streams) when the asset has normals or tangents; both are read */
int chordvis_save_asset(const ChordBuiltAsset* asset, const char* path);
int chordvis_load_asset(const char* path, ChordBuiltAsset** outAsset);
/* The reference's own container for an asset's geometry: the GLTFBinary archive (asset_gltf.h:260-300) as saveAsset / loadAsset
 * write and read it (serialize.h:217-320: cereal binary archive, LZ4 block compression when lz4 != 0).  Load yields ONE
 * primitive spanning the file (the per-primitive offsets live in the reference's GLTFAsset, another archive).  Positions,
 * normals, texcoords0, tangents and the Nanite data are read and written; the attributes this path does not use (smooth
 * normals, second uv set, colours, LOD-0 indices) are skipped on load and written empty. */
int chordvis_save_gltf_binary(const ChordBuiltAsset* asset, const char* path, int lz4);
int chordvis_load_gltf_binary(const char* path, ChordBuiltAsset** outAsset);

/* ------------------------------------------------------------------ context (graphics::Context, graphics.h:88-345) */

/* hipStream: an existing hipStream_t to enqueue on (e.g. the caller's current stream), or NULL for a context-owned
 * NON-BLOCKING stream.  NULL is "no stream given", not "the null stream": work the host enqueues on the legacy default
 * stream is NOT ordered against a context-owned stream.  A host that issues its own collectives or copies between passes
 * hands over the stream it issues them on (PyTorch: a torch.cuda.Stream made current; its default stream has handle 0,
 * which arrives here as NULL), or passes hipStreamLegacy / hipStreamPerThread ((void*)1 / (void*)2), which go through. */
int chordvis_create(int deviceOrdinal, void* hipStream, ChordCtx** outCtx);
/* STREAM CONTRACT.  A host may enqueue frame after frame without waiting for the device; what every call does with unfinished work
 * on the context's stream in front of it is one of three things.  tests/test_gpu_frames_in_flight.py holds each statement, on a
 * caller-owned stream and on hipStreamLegacy, with the device kept from starting anything until the last call has returned, and
 * keeps the list of the calls that wait as a table (WAITS) asserted both ways.
 *   ENQUEUED, RETURNS AT ONCE (never waits for the stream): chordvis_set_view, chordvis_bind_objects, chordvis_reset_history (host
 *     state only); chordvis_update_objects (see below for large arrays); chordvis_render_frame; the passes called one by one
 *     (chordvis_clear_gbuffer, chordvis_instance_culling, chordvis_visibility_stage0 / 1, chordvis_build_hzb);
 *     chordvis_render_shadow once the depth views exist (chordvis_allocate_depth_views allocates); chordvis_resolve_attributes and
 *     chordvis_resolve_gbuffer; chordvis_last_frame_cmds and chordvis_history_hzb (handles of device memory that the frames in flight
 *     have yet to write: read them ordered behind the context's stream; chordvis_history_hzb may launch the tail of the chain);
 *     chordvis_scatter_world_transforms and chordvis_build_objects (one launch each, of any size: the way to new object records
 *     for a host that must not wait); chordvis_set_object_list while the new list fits what is allocated (it MAY WAIT when a buffer
 *     has to grow: OBJECTS COME AND GO below); chordvis_refit_ray_scene, chordvis_trace_rays and chordvis_pixel_rays (one launch each: RAY QUERIES below).
 *     The kernels a frame launches are chosen from reports the device leaves when a pass finishes; the host may hold a report any
 *     number of frames old, or none: the choice costs or saves time, never a pixel, a list entry or an HZB texel.
 *   MAY WAIT for everything enqueued before it: chordvis_upload_scene, chordvis_upload_material_textures,
 *     chordvis_allocate_gbuffer, chordvis_upload_history_hzb, chordvis_sync, every chordvis_readback_* call (chordvis_readback_objects and
 *     chordvis_readback_world_transforms among them), chordvis_upload_world_transforms (a build in flight keeps its inputs),
 *     chordvis_build_objects_status, chordvis_build_ray_scene, chordvis_ray_scene_info, chordvis_stats and
 *     chordvis_destroy, which lets the stream run empty before it frees anything: frames in flight finish on memory that is still
 *     theirs.  (Read from the code, not among the tested calls: chordvis_set_shard, chordvis_set_tile_owners and
 *     chordvis_allocate_depth_views re-make buffers and wait likewise.)  chordvis_update_objects waits too when the array is
 *     large: its copy from the caller's pageable memory is the HIP runtime's hipMemcpyAsync, which was measured (HIP 7.0, MI355X) to
 *     return at once for arrays of 4 KB to 1 MB (4 681 objects) and to wait for the stream for arrays of 2 MB (9 362 objects) to
 *     16 MB; where between 1 and 2 MB it changes was not measured, and another runtime may draw the line elsewhere.  A host that
 *     must not wait binds a device array, or keeps the world transforms resident and calls chordvis_build_objects.
 *   CALLER MEMORY.  Host arrays are read before the call returns and are the caller's again on return, whether or not the frame that
 *     uses them has started.  For the records of chordvis_set_view, the chain of chordvis_upload_history_hzb and the scene of the
 *     uploads the library sees to that itself: it copies them into memory of its own or waits.  A second chordvis_set_view may
 *     follow a frame at once and the frame keeps its view, on both ways a view reaches the device: as an argument of the frame's
 *     cull kernel (chordvis_render_frame, chordvis_instance_culling), and through the asynchronous copy from the context's own host
 *     record that a pass makes when the view was set after the cull (chordvis_hzb_culling, chordvis_render_mesh and the stage
 *     calls built on them).  For hostObjects of chordvis_update_objects -- it may be overwritten or freed at once -- the library
 *     relies on the HIP runtime reading a pageable source before hipMemcpyAsync returns: held by the tests with the scenes of 352
 *     and 22 528 objects and with plain copies of 4 KB, 77 KB, 256 KB, 1, 2, 4, 4.8 and 16 MB; no other size was measured.
 *     The two camera positions of chordvis_build_objects travel as kernel arguments: the caller's arrays are free on return.
 *     Device memory the caller owns is read and written WHEN THE FRAME RUNS, in stream order: an array bound with
 *     chordvis_bind_objects may be rewritten between frames by work on the context's stream, and the image handed to
 *     chordvis_allocate_gbuffer and the targets of the resolves may be cleared, copied and read there; a write from another stream
 *     that is not ordered against the context's reaches whichever frame runs next. */
int chordvis_destroy(ChordCtx* ctx);
const char* chordvis_last_error(ChordCtx* ctx);
int chordvis_sync(ChordCtx* ctx);

/* GPUScene / asset upload (gpu_scene.h:20-165, asset_gltf.h:278): copies and flattens.  Limits of a scene (CHORDVIS_E_INVALID
 * beyond them): 0x55555555 vertices over all assets (vertex index x 3 is formed in 32 bits; the reference's ByteAddressBuffer
 * offsets are 32-bit BYTE offsets, a third of that), meshlets of at most 255 vertices / 128 triangles, groups of at most four
 * meshlets, alpha-tested textures of at most 16384 x 16384 texels and 15 levels.  A ChordMeshlet of ANY vertex count V <= 255 and
 * triangle count T <= 128 whose triangle words name local indices below V is accepted -- V need not be bounded by T (disjoint
 * triangles: V up to 3T), the vertex-id table need not ascend, meshlets may share vertices, T may be 0 -- and every such shape is
 * held to the oracle through each set-up kernel, the clipper, the depth-only pass and the resolve (tests/test_gpu_meshlet_shapes.py).
 * A context may take scene after scene.  An upload drops what belonged to the scene before: the history HZB (the next frame is a
 * frame without history), the kept tile schedules, the depth views and the cascade cache, the material textures and the geometry
 * feedback, and objects bound with chordvis_bind_objects (the library's copy of the new scene's objects is read again), and the
 * resident world transforms of chordvis_upload_world_transforms and the ray scene of chordvis_build_ray_scene (both dropped by a
 * refused upload too).  The
 * G-buffer, the view, the cull mode, the debug switches and the limits stay.
 * A REFUSED upload (any error code, the refusal of a scene without BVHs under chordvis_set_cull_mode(ctx, 1) included) leaves the
 * context with NO scene: the scene before is gone too, and every call that needs a scene returns CHORDVIS_E_INVALID until an upload
 * succeeds.  The G-buffer and every setting stay, so that upload may follow at once (after chordvis_set_cull_mode(ctx, 0), say). */
int chordvis_upload_scene(ChordCtx* ctx, const ChordSceneDesc* scene);
/* uploadBufferToGPU("GLTFObjectInfo", ...) renderer.cpp:229 — per-frame object records
 * (count must equal the current list's count -- the uploaded scene's objectCount, or that of the latest chordvis_set_object_list;
 * primitive/material ids must not change: a list of other objects goes through chordvis_set_object_list). */
int chordvis_update_objects(ChordCtx* ctx, const ChordObject* hostObjects, uint32_t count);
/* Same, for a caller-owned DEVICE array (no copy; must stay valid while bound).  The array stays bound -- the depth views read
 * it too -- until chordvis_update_objects or chordvis_upload_scene returns the context to its own copy.  The caller may rewrite
 * the array between frames without telling the library, ordered behind the context's stream; what the library cannot see it
 * cannot check, so between a frame and the chordvis_resolve_* calls on that frame's image the CALLER guarantees that the array
 * is not written.  The call itself counts as a change of the objects, exactly like chordvis_update_objects: a chordvis_resolve_*
 * after it is refused (CHORDVIS_E_INVALID) until the next frame has run -- also when the same array is bound again. */
int chordvis_bind_objects(ChordCtx* ctx, const ChordObject* deviceObjects, uint32_t count);

/* OBJECTS COME AND GO.  The reference collects its object list anew every frame (getPerframeCollected + uploadBufferToGPU("GLTFObjectInfo"),
 * renderer.cpp:217,229) over geometry that stays resident in the GPUScene pools (gpu_scene.h:20-165).  chordvis_set_object_list is
 * that for this library: it replaces the object LIST of the resident scene -- any count >= 1, any primitive and any material of the
 * uploaded scene in any order and any number of times, primitives no object named at upload included -- and copies no vertex, meshlet
 * or texture.  hostObjects are complete records (basicData for the next frame and the two ids), as in ChordSceneDesc::objects.
 *   EQUIVALENCE.  After a successful call the context behaves, for everything that depends on the objects, exactly like a context that
 *     uploaded the same scene descriptor with objects = hostObjects, objectCount = count: the image, the three command lists (order,
 *     slot fields and counts), the HZB chains, chordvis_stats' counts and the handles' `capacity` are bit for bit that context's, in
 *     every cull path (fused, three-launch, quad, hierarchical, sharded, the depth views).  The capacities the kernels see are always
 *     those of such an upload, whatever the buffers hold.
 *   KEPT: every asset, primitive and material table, the alpha plane; the material textures of chordvis_upload_material_textures with
 *     their block store, first levels and feedback counts; the G-buffer, the view, the limits, the cull mode, the debug switches, the
 *     kept tile schedules; and the HISTORY HZB -- the next frame is a two-pass frame against the previous frame's chain, with the new
 *     objects' own last-frame matrices, and a previous frame's HZB tail that still waits to ride in the next cull launch still runs.
 *   DROPPED, as chordvis_upload_scene drops them and with the same refusals afterwards, because each is sized by or names the old list:
 *     the geometry feedback buffer (chordvis_geometry_feedback is refused until chordvis_geometry_feedback_reset); the resident world
 *     transforms (chordvis_build_objects is refused until chordvis_upload_world_transforms); a chordvis_bind_objects binding (the
 *     context reads its own array again, which receives hostObjects); the depth views and the cascade cache (the next
 *     chordvis_render_shadow makes the views again and renders every cascade; the view-by-view depth calls are refused until
 *     chordvis_allocate_depth_views); the sharded lists and the cull exchange buffer
 *     (re-made on demand, as at upload); the resolve state -- chordvis_resolve_*, the feedback calls and everything else that needs a
 *     frame's image are refused until a frame has run; the TLAS of the ray scene (chordvis_refit_ray_scene, chordvis_trace_rays and
 *     chordvis_pixel_rays are refused until chordvis_build_ray_scene, which keeps the BLASes and builds none again).
 *   VALIDATE FIRST, COMMIT SECOND.  CHORDVIS_E_INVALID: count == 0 or hostObjects NULL; a primitive or material id out of range; no
 *     scene; a depth-view child context; a call between chordvis_frame_phase_cull and chordvis_frame_phase_a.  CHORDVIS_E_CAPACITY:
 *     2^24 - 2 or more cluster instances, or more than 2^31 - 1 group instances.  A refused call changes NOTHING -- unlike a refused
 *     chordvis_upload_scene: the context still renders the list it had, with its history, and chordvis_last_error names the rule.  The
 *     same holds when a buffer the longer list needs cannot be allocated (CHORDVIS_E_HIP): every new buffer is made before an old one
 *     is let go.
 *   STREAM ORDER AND MEMORY.  The device buffers sized by the list (object records and frames, the static and the group tables, group
 *     masks, block counts, the three command lists, the raster record lists and the block pool) only ever grow.  When the new list
 *     fits what is allocated the call is stream-ordered behind the frames in flight and NEVER WAITS for the device: one copy of the
 *     records, one copy of the 48-byte static records, one kernel launch that builds the flattened (object, group) table on the
 *     device (kernels_objects.hip), and what it drops is parked and freed by a later call that waits anyway (chordvis_sync,
 *     chordvis_upload_scene, a chordvis_set_object_list that grows, chordvis_destroy; with 32 allocations parked the call itself waits once).  hostObjects is read before the call
 *     returns and is the caller's again on return, under the rule of chordvis_update_objects above (a large pageable array makes the
 *     HIP runtime's copy wait).  When something must grow the call MAY WAIT: it lets the stream run empty first, because a frame in
 *     flight keeps its buffers, then swaps the buffers.  Allocations never shrink before chordvis_upload_scene or chordvis_destroy.  A
 *     host that wants no stall gives its LARGEST list once, up front -- at upload, or in one chordvis_set_object_list -- and shorter ones after it.
 *     On a sharded context the cull exchange buffer follows the list's count blocks (it is re-made, with a wait, whenever
 *     ceil(count blocks / ranks) changes).
 * tests/test_gpu_object_list.py holds every statement; DESIGN.md 4.15 has the kernel and the timings. */
int chordvis_set_object_list(ChordCtx* ctx, const ChordObject* hostObjects, uint32_t count);

/* OBJECT RECORDS BUILT ON THE DEVICE.  Every field of ChordObject::basicData is camera-relative, so a moving camera changes the record
 * of every object, static ones included.  Instead of filling the records on the host (chordvis_object_basic_data_batch) and copying
 * 224 bytes per object (chordvis_update_objects), a host may keep the objects' double-precision world matrices RESIDENT on the device
 * and have the records built there: per frame one scatter of the matrices that moved (the counterpart of the reference's sparse
 * GPUScene upload, gpu_scene.cpp:30-64) and one build call, neither of which ever waits for the stream.  Opt-in: a host that calls
 * none of these gets the launches and the bytes it got before.
 *   RESIDENT STATE.  Two device arrays of objectCount x 16 doubles (glm column-major), `cur` and `prev`, allocated by the first
 *     chordvis_upload_world_transforms after a scene upload, dropped by every chordvis_upload_scene (refused ones included), freed by
 *     chordvis_destroy.  `count` is the scene's objectCount in every call that takes one: otherwise CHORDVIS_E_INVALID, and
 *     chordvis_last_error names the rule.
 *   chordvis_upload_world_transforms sets cur and prev from host arrays (hostPrevLocalToWorld NULL: prev = cur).  MAY WAIT: it lets the
 *     stream run empty first, so that a build in flight keeps its inputs.  The host arrays are the caller's again on return.
 *   chordvis_scatter_world_transforms is ONE launch on the context's stream: cur[deviceIndices[k]] = deviceLocalToWorld[k] for k < n.
 *     Both arrays are caller-owned DEVICE memory, read when the launch runs, in stream order.  An index at or beyond objectCount is
 *     skipped: nothing is written for it.  Indices within one call are the caller's to keep distinct (with a duplicate one of the given
 *     matrices lands, unspecified which); calls are ordered by the stream, so a later call wins.  n == 0 succeeds without a launch.
 *     Never waits.  deviceLocalToWorld must be 16-byte aligned (CHORDVIS_E_INVALID otherwise).
 *   chordvis_build_objects is ONE launch on the context's stream over all objects.  For object i it writes into the context's own object
 *     array the 208 bytes of basicData that chordvis_object_basic_data(cur[i], prev[i], cameraPos, cameraPosLast) writes, then sets
 *     prev[i] = cur[i]: an object that was not scattered since the last build is a static object under a moving camera at the next one,
 *     and last-frame matrices -- motion vectors -- come from the library's own copy of the previous transforms.  The 16 bytes behind
 *     basicData (GLTFPrimitiveDetail, GLTFMaterialData, the pads) are never written and never read-modify-written: they stay what
 *     chordvis_upload_scene or chordvis_update_objects put there.  cameraPosLast NULL: = cameraPos.  Both positions travel by value as
 *     kernel arguments: the call returns at once and the caller's arrays are free on return.  Like chordvis_update_objects it returns
 *     the context to its own array after chordvis_bind_objects, and it counts as a change of the objects: chordvis_resolve_*, the
 *     feedback calls and everything else that needs the frame's matrices is refused until the next frame.  CHORDVIS_E_INVALID without
 *     a scene, or without a chordvis_upload_world_transforms since the scene upload.  The depth views read the same array.
 *   ARITHMETIC.  Bit for bit the host function's, for finite inputs: m[12..14] minus the camera in binary64, one round-to-nearest-even
 *     conversion per element to binary32, the cofactor inverse in the host function's source order (products left to right, sums left
 *     to right, 1 / det once, sixteen multiplies), the three column lengths through a correctly rounded square root, and their maximum;
 *     no contraction; binary32 subnormals are kept, not flushed.  Finite inputs can still end in a NaN of the inverse (a determinant
 *     in the subnormal range has an infinite reciprocal, and infinity times a zero of the last row is invalid): such a NaN has the
 *     bits an x86 host's function produces, 0xFFC00000 (the device's own pattern for an invalid operation).  Non-finite inputs do not fault; their bits are unspecified.
 *   SINGULAR MATRICES.  chordvis_object_basic_data returns an error for a matrix with det == 0 and leaves localToTranslatedWorld and
 *     the last-frame matrix filled, the inverse and the scale zero.  The build writes exactly those bytes for that object and goes on;
 *     it counts such objects and keeps the smallest of their indices.  chordvis_build_objects_status SYNCHRONISES and reports both for
 *     the latest build since the transforms were uploaded: 0 and 0xFFFFFFFF when there was none (either pointer may be NULL).  The two
 *     words are cleared for each build on the stream.
 *   chordvis_readback_objects (the array frames read now: the bound one after chordvis_bind_objects) and
 *     chordvis_readback_world_transforms (either array may be NULL) SYNCHRONISE and copy to the host.
 * tests/test_gpu_object_build.py holds the kernel to chordvis_object_basic_data byte by byte; DESIGN.md 4.14 has the layout and timings. */
int chordvis_upload_world_transforms(ChordCtx* ctx, const double* hostLocalToWorld /* count x 16 */,
                                     const double* hostPrevLocalToWorld /* or NULL: = current */, uint32_t count);
int chordvis_scatter_world_transforms(ChordCtx* ctx, const uint32_t* deviceIndices, const double* deviceLocalToWorld /* n x 16 */, uint32_t n);
int chordvis_build_objects(ChordCtx* ctx, const double cameraPos[3], const double cameraPosLast[3] /* NULL: = cameraPos */);
int chordvis_build_objects_status(ChordCtx* ctx, uint32_t* singularCount, uint32_t* firstSingular);
int chordvis_readback_objects(ChordCtx* ctx, ChordObject* host, uint32_t count);
int chordvis_readback_world_transforms(ChordCtx* ctx, double* hostCur, double* hostPrev, uint32_t count);

/* RAY QUERIES.  The reference builds an acceleration structure over the scene it rasters -- one BLAS per primitive over its LOD-0
 * triangles (asset_gltf.cpp:543-555), TLAS instances collected per frame (component_gltf_mesh.cpp:109-118), all FORCE_OPAQUE
 * (asset_gltf.cpp:575-577) -- and traces inline ray queries against it (TraceRayInline on topLevelAS: gi_rt_ao.hlsl,
 * ddgi_probe_trace.hlsl, gi_screen_probe_*.hlsl, gi_specular_trace.hlsl, accelerate_structure_visualize.hlsl, the editor's picking).
 * This is that for the resident scene: an opt-in ray scene built from what chordvis_upload_scene left on the device, kept current by
 * one launch and traced by one launch (the MI355X has no ray hardware: kernels_rays.hip walks the trees).  A host that calls none of
 * these gets the launches and the bytes it got before; no frame state is read or written.
 *   WHAT A RAY MEETS.  Every object of the current list, through the triangles of its primitive's meshlets with lod == 0 (reached through
 *     the primitive's groups), solid whatever its material: masked, blended, two-sided or not.  A ChordRay lives in the translated-world
 *     (camera-relative) space of the object records the frames read now.  The answer is DEFINED by a brute-force specification that
 *     knows no tree (tests/spec_rays_np.py) and the result is that specification's word for word: binary32, no
 *     contraction, correctly rounded divide, subnormals kept, min / max as the selects a < b ? a : b and a > b ? a : b.  In short: the
 *     object's box is the min / max of the eight corners of the primitive's bounds through localToTranslatedWorld (the object stage's
 *     arithmetic); the ray goes into local space through translatedWorldToLocal; a triangle is tested by Moller-Trumbore against the
 *     local ray, its t clamped into the slab interval of the triangle's own box and then into that of the object's box, and kept when
 *     the clamped t lies in [tMin, tMax]; the smallest t wins, ties go to the smallest (object, meshlet, triangle).  A ray with a
 *     non-finite word, with no finite reciprocal direction component, or with tMin > tMax is a miss; no ray faults.  The triangle test
 *     is NOT watertight: a ray through an edge or a vertex two triangles share may miss both (a watertight test is a later change).
 *     Object records must be finite, and so must the positions of the LOD-0 triangles: chordvis_build_ray_scene refuses a scene with a
 *     non-finite one (CHORDVIS_E_INVALID; a box that is a union with a NaN bounds nothing).
 *   chordvis_build_ray_scene MAY WAIT (it reads device memory back).  It builds one BLAS per primitive of the uploaded scene, named by
 *     an object or not (a primitive without LOD-0 triangles gets an empty BLAS and is never hit); BLASes are kept until the next
 *     chordvis_upload_scene, so a second call builds none (outInfo->blasBuilt == 0).  It builds the TLAS topology for the current
 *     object list from the object array the frames read now, and ends with a refit: tracing is valid straight after it.  outInfo may
 *     be NULL.  Trees are 4-wide with at most four triangles (one object) per leaf and at most CHORD_RAY_MAX_DEPTH interior levels each:
 *     the traversal stack holds 76 entries per ray, 3 x (12 + 12) + 2.  The builder bounds the depth by equal-count splits, so
 *     CHORDVIS_E_CAPACITY means more items than 4^12 leaves hold (67 M triangles in one primitive, 16 M objects), or 2^28 - 4 or more
 *     LOD-0 triangles in the scene.  VALIDATE FIRST, COMMIT SECOND: every new buffer is made before an old one is let go; a refused
 *     call leaves the ray scene it found.
 *   DROPPED: the whole ray scene by chordvis_upload_scene (refused ones included); the TLAS by chordvis_set_object_list, whether its
 *     buffers fit or grow.  Until the next chordvis_build_ray_scene the refit and the trace are refused.
 *   chordvis_refit_ray_scene is ONE launch on the context's stream and never waits: every TLAS leaf box again from the object array the
 *     frames read now (the bound one after chordvis_bind_objects), every interior box bottom-up.  After chordvis_update_objects,
 *     chordvis_build_objects or chordvis_bind_objects a trace is refused until a refit has been enqueued.  A bound array the caller
 *     rewrites itself is the caller's to follow with a refit.
 *   chordvis_trace_rays is ONE launch and never waits; count == 0 succeeds without one.  deviceRays / deviceHits: caller-owned device
 *     memory, 16-byte aligned, read and written when the launch runs -- behind the refit and behind whatever wrote the rays on the
 *     context's stream.  flags: CHORD_RAY_ANY_HIT asks only whether a candidate exists (which triangle is found first is not part of
 *     the contract).  Valid with or without a view or a G-buffer.
 *   chordvis_ray_scene_info SYNCHRONISES and fills the counts and the root's box from the device.
 *   CHORDVIS_E_INVALID, chordvis_last_error naming the rule: no scene; no ray scene, or one dropped since; a depth-view child context;
 *     count > 0 with a NULL or misaligned pointer; unknown flag bits; a trace before the refit an object change requires; a non-finite
 *     LOD-0 position at the build.
 *   Sharded and group contexts: every rank holds the whole scene, so a rank's own context may build and trace.
 * tests/test_gpu_rays.py holds every statement but one: the refusal on a depth-view child context, which no entry point hands out (read
 * from the code, like the same refusal of chordvis_set_object_list). */
int chordvis_build_ray_scene(ChordCtx* ctx, ChordRaySceneInfo* outInfo);
int chordvis_refit_ray_scene(ChordCtx* ctx);
int chordvis_trace_rays(ChordCtx* ctx, const ChordRay* deviceRays, uint32_t count, uint32_t flags, ChordRayHit* deviceHits);
int chordvis_ray_scene_info(ChordCtx* ctx, ChordRaySceneInfo* outInfo);

/* REBUILDING THE TLAS.  chordvis_rebuild_ray_tlas builds the TLAS topology for the current object list ON THE DEVICE,
 * in stream order, from the object array the frames read now (the bound one after chordvis_bind_objects), and ends with the refit:
 * tracing is valid straight after it and a pending refit is done.  It needs the BLASes -- one chordvis_build_ray_scene since the last
 * chordvis_upload_scene -- and is valid whether a TLAS exists (objects have travelled: a refit keeps the old topology, whose boxes
 * overlap more and more) or was dropped by chordvis_set_object_list (objects came and went).  It never synchronises, copies or
 * allocates, but for a list LONGER than every list rebuilt before on this scene: then new buffers are made first and the old ones
 * let go afterwards, and the call may wait, as a growing chordvis_set_object_list may.  The rebuild owns its buffers and keeps them
 * across object lists until the next chordvis_upload_scene.  Launches: two (one workgroup, then the refit) up to
 * CHORD_RAY_TLAS_GROUP_MAX objects, 15 above (centres, four radix passes of three launches, node table, refit): a function of the
 * count alone.  Not inside a captured graph.
 *   THE TREE is a pure function of the object boxes (tests/spec_ray_tlas_np.py states it in numpy; chord_amd/csrc/ray_tlas_shape.h is
 *   the code), binary32, one rounding per operation, no contraction, correctly rounded divide:
 *     box        of object i: the refit's (RAY QUERIES above)
 *     centre     c[a] = lo[a] * 0.5f + hi[a] * 0.5f
 *     bounds     Blo[a], Bhi[a]: min and max of c[a] over all objects under the total order of the float's bits made monotone
 *                (u & 0x80000000 ? ~u : u | 0x80000000): -0 sorts below +0, a NaN goes to an end
 *     quantised  extent = Bhi[a] - Blo[a]; !(extent > 0) || !(extent < 3.0e38f): q[a] = 0; otherwise scale = 1024.0f / extent,
 *                f = (c[a] - Blo[a]) * scale, q[a] = f > 0 ? (f < 1024.0f ? (uint32) f : 1023) : 0 (a NaN gives 0)
 *     key        30 bits: bit 3 k + a of m is bit k of q[a]
 *     order      ascending (m, i): the pairs are unique
 *     levels     cnt[0] = n, cnt[j] = ceil(cnt[j-1] / 4) up to the first j >= 1 with cnt[j] == 1: that j is the depth D (n == 1:
 *                D = 1).  D > CHORD_RAY_MAX_DEPTH (n > 4^12) is CHORDVIS_E_CAPACITY, nothing changed or launched
 *     numbering  base[D] = 0, base[j-1] = base[j] + cnt[j]; node (j, i) is base[j] + i, the root is node 0; tlasNodes = cnt[1] + ..
 *                + cnt[D], tlasDepth = D
 *     words      of node (j, i): childCount = min(4, cnt[j-1] - 4 i); child k is CHORD_RAY_TLAS_LEAF << 30 | order[4 i + k] for
 *                j == 1, else CHORD_RAY_TLAS_NODE << 30 | (base[j-1] + 4 i + k); an unused slot holds CHORD_RAY_NO_CHILD, lo = +inf,
 *                hi = -inf; parentRef is CHORD_RAY_NO_CHILD for the root, else (base[j+1] + (i >> 2)) * 4 + (i & 3); pad is 0
 *     leafRef    leafRef[order[p]] = (base[1] + (p >> 2)) * 4 + (p & 3)
 *     boxes      of used slots: the refit's exact unions
 *   The answer of a trace does not depend on the tree, so hits are the specification's whichever builder made the TLAS.  WHICH TO
 *   PREFER: chordvis_build_ray_scene's host builder splits by surface area and its tree is the cheaper one to walk; a host with time
 *   to spare -- a static list, a loading screen -- should build there and refit.  Measured on an MI355X (profiles/ray_tlas_time.txt;
 *   DESIGN.md 4.19): the rebuild takes 0.039 ms of device time for 352 objects and 0.146 ms for 22 528, against 0.26 ms and 9.8 ms of
 *   host wall time for the host's TLAS rebuild with its wait; a 4K pass of closest-hit pixel rays on the rebuilt tree takes 1.5 and
 *   2.06 times as long as on the host-built tree (AO: 1.43 and 1.95 times), because a Morton-order complete tree puts large boxes
 *   among small ones into the same nodes.  The rebuild is for the frame loop, where the list changes or the wait is what hurts.
 *   chordvis_set_object_list and chordvis_build_ray_scene behave as before: after a new list the refit, the trace and the info are
 *   refused until a build OR a rebuild; the build still makes the surface-area TLAS on the host.
 *   CHORDVIS_E_INVALID, chordvis_last_error naming the remedy, nothing changed or launched: a NULL context (no message); a depth-view
 *   child context; no scene; no BLASes since the last chordvis_upload_scene.  A refused rebuild leaves the TLAS it found.
 * chordvis_readback_ray_tlas SYNCHRONISES and copies the TLAS's node table (chordvis_ray_scene_info's tlasNodes records) and leaf
 * references (one per object) to the host, whichever builder made them; either pointer may be NULL; a capacity below the count is
 * CHORDVIS_E_INVALID, and so is a context without a TLAS.
 * tests/test_ray_tlas_spec.py holds the specification to a scalar evaluation, tests/test_ray_tlas_host.py runs ray_tlas_shape.h on
 * the host under the address and undefined-behaviour sanitizers, tests/test_gpu_ray_tlas.py holds the statements above on the GPU but
 * the refusal on a depth-view child context, which no entry point hands out (read from the code). */
int chordvis_rebuild_ray_tlas(ChordCtx* ctx);
int chordvis_readback_ray_tlas(ChordCtx* ctx, ChordRayNode* hostNodes, uint32_t nodeCapacity, uint32_t* hostLeafRef, uint32_t objectCapacity);

/* SHADING A HIT (RayHitMaterialInfo::init, raytrace_shared.hlsli: what ddgi_probe_trace.hlsl, gi_screen_probe_*.hlsl and
 * gi_specular_trace.hlsl do with a hit).  chordvis_shade_ray_hits writes one ChordRayHitSurface per ChordRayHit --
 * material, normal and uv at the hit point -- in ONE launch on the context's stream that never waits; count == 0 succeeds without
 * one.  deviceHits / deviceSurfaces: caller-owned device memory, 16-byte aligned; deviceLods: NULL (`lod` for every hit) or count
 * floats, 4-byte aligned; all read and written when the launch runs.  It needs chordvis_upload_scene and
 * chordvis_upload_material_textures and NO ray scene: the hits may be chordvis_trace_rays' or a host's own.  It reads the object array
 * the frames read now (the bound one after chordvis_bind_objects): a host that changes the objects between trace and shade gets the
 * new matrices and the new materials, and no refit is involved; after chordvis_set_object_list the valid object indices are the new
 * list's.  Valid with or without a view or a G-buffer; frames are untouched.
 *   The answer is DEFINED by tests/spec_ray_shade_np.py (shade) and is that specification's word for word: binary32, one rounding
 *   per operation, no contraction, correctly rounded divide and square root.  Per hit:
 *     meshlet   ChordRayHit::meshlet is ASSET-RELATIVE, as chordvis_trace_rays and chordvis_pixel_rays write it: an index into the
 *               meshlets of the asset (ChordPrimitive::primitiveDatasBufferId) of the OBJECT's primitive.  It is read at that asset's
 *               first meshlet + meshlet.  With one asset that is the index into the scene's meshlets.
 *     valid     status bit 0 set; u and v finite; object < the object count; the object's GLTFPrimitiveDetail and GLTFMaterialData
 *               below their counts; meshlet < the meshlet count of THAT ASSET (not the scene's: the id one past an asset's last
 *               meshlet is invalid although the concatenated array goes on); triangle < the meshlet's triangle count; the triangle
 *               word, the three vertex-id words and the three vertex ids inside their arrays.  An INVALID hit gives sixteen zero words;
 *               no hit faults.  The vertex ids are offset by the vertexOffset of the OBJECT's primitive, also where a host's own hit
 *               pairs the object with a meshlet of another primitive OF THE SAME ASSET (a meshlet of another asset cannot be named).
 *     b         ((1 - u) - v, u, v)
 *     uv        (uv0 * b.x + uv1 * b.y) + uv2 * b.z per component; (0, 0) for a scene uploaded without texture coordinates, and the
 *               material fields are then sampled at (0, 0)
 *     normal    per vertex normalize(mul(float4(nLS, 0), translatedWorldToLocal).xyz) -- chordvis_resolve_surface's vertex normal --
 *               interpolated like uv and THEN normalised (raytrace_shared.hlsli:92); normalize gives 0 where the squared length is not
 *               above 0; negated when the material is two-sided and the hit a back face; zero for a scene uploaded without normals
 *     level     lodq = (int32) floor(min(max(lod, 0), 15) * 256), a NaN lod counting as 0, from deviceLods[i] or `lod`; from lodq the
 *               level rule of chordvis_resolve_material's sampler unchanged: minified iff lodq > 0; *_MIPMAP_NEAREST takes level
 *               min((lodq + 128) >> 8, last); *_MIPMAP_LINEAR blends levels l0 = min(lodq >> 8, last) and min(l0 + 1, last) by
 *               (lodq & 255) / 256; otherwise level 0; the min / mag filter inside a level.  Levels count from the first level STORED
 *               (chordvis_set_texture_first_level).  There are no gradients, so chordvis_set_material_anisotropy has no effect.
 *     fields    baseColor = sample * baseColorFactor, rgb through sRGB -> AP1, white without a texture; emissive = sample.rgb *
 *               emissiveFactor, zero without one, NOT through sRGB -> AP1 (chordvis_resolve_material's row; a departure from the
 *               reference's hit shading); roughness, metallic = .g, .b of the metallic-roughness texture, or roughnessFactor and
 *               (metallicFactor >= 1 ? 0 : metallicFactor); the normal texture is not read.  A material of another materialType than 1
 *               leaves these fields zero and CHORD_RAYSURF_PBR clear; material, normal, uv and the other flags are filled all the same.
 *   Both texture stores (chordvis_set_material_texture_store) give the same words.
 *   CHORDVIS_E_INVALID, chordvis_last_error naming the remedy, and nothing is changed or launched: a NULL context (no message); a
 *   depth-view child context; no scene; no chordvis_upload_material_textures since the last chordvis_upload_scene; between
 *   chordvis_frame_phase_cull and chordvis_frame_phase_a; count > 0 with deviceHits or deviceSurfaces NULL or not 16-byte aligned; a
 *   deviceLods that is not 4-byte aligned.
 * tests/test_ray_shade_host.py runs the per-hit code on the host under the address and undefined-behaviour sanitizers;
 * tests/test_gpu_ray_shade.py holds the statements above on the GPU, but the refusal on a depth-view child context, which no entry
 * point hands out (read from the code). */
int chordvis_shade_ray_hits(ChordCtx* ctx, const ChordRayHit* deviceHits, uint32_t count, float lod, const float* deviceLods,
                            ChordRayHitSurface* deviceSurfaces);

/* PIXEL RAYS (gi_rt_ao.hlsl, the first of the reference's ray consumers and the one a frame of this library feeds by itself; a sun-
 * shadow mask likewise).  chordvis_pixel_rays generates one ray per pixel from caller-owned position and normal images
 * (ChordResolveTargets::positionRS; ChordSurfaceTargets::vertexNormal or the material resolve's pixel normal; or a host's own), traces
 * it against the ray scene and reduces the result to one float per pixel, in ONE launch on the context's stream that never waits;
 * width * height == 0 succeeds without one.  The rays never reach memory.  All pointers are caller-owned device memory, read and
 * written when the launch runs, in stream order: behind the refit and behind whatever wrote the images on the context's stream.  The
 * images need not come from this context's frame: valid with or without a view or a G-buffer, like chordvis_trace_rays; frames are
 * untouched.
 *   The answer is DEFINED by tests/spec_pixel_rays_np.py (pixel_rays), which builds a ChordRay per pixel and hands it to the brute
 *   force of tests/spec_rays_np.py, and is that specification's word for word: binary32, one rounding per operation, no contraction,
 *   correctly rounded divide and square root, no transcendental.  Per pixel (x, y), i = y * width + x:
 *     valid      with deviceZ: z = deviceZ[i * deviceZStride] > 0 (deviceZStride in floats: 1 reads a D32 image, 2 the depth halves of
 *                the library's 64-bit visibility words in place, the pointer at the first word's high half); without: position.w != 0
 *                (the resolve writes xyz, 1 and all-zero for an empty pixel).  An INVALID pixel traces nothing: out = 1, a zero hit record.
 *     origin     position.xyz, translated-world space: the space of a ChordRay
 *     n          normalize(normal.xyz) with chordvis_resolve_surface's normalize: 0 where the squared length is not above 0
 *     direction  CHORD_PIXEL_RAYS_HEMISPHERE (gi_rt_ao.hlsl:59-61): dT = deviceTable[(y & (tableH - 1)) * tableW + (x & (tableW - 1))].xyz,
 *                a tangent-space direction, z up, float4 per texel, tableW and tableH powers of two.  The host bakes
 *                uniformSampleHemisphere(STBN_float2(...)) into the table once per slice and passes the slice of the frame: the library
 *                owns no blue noise and evaluates no sin or cos.  createTBN (base.hlsli:1001-1025): |n.z| > 0: k = sqrt(n.y n.y +
 *                n.z n.z), u = (0, -n.z / k, n.y / k); otherwise k = sqrt(n.x n.x + n.y n.y), u = (n.y / k, -n.x / k, 0); b = cross(n, u);
 *                d = (dT.x u + dT.y b) + dT.z n per component.
 *                CHORD_PIXEL_RAYS_DIRECTION: d = desc->direction for every pixel (a sun shadow ray).  With CHORD_PIXEL_RAYS_FRONT_ONLY a
 *                pixel whose (n.x d.x + n.y d.y) + n.z d.z is not above 0 faces away: it traces nothing, out = 0, a zero hit record.
 *     interval   tMax = rayLength; tMin = desc->tMin, or with CHORD_PIXEL_RAYS_START_FROM_DEPTH (getRayTraceStartOffset,
 *                raytrace_shared.hlsli:10-17) lin = zNear / z, s = lin * 0.01f, w = s / (s + 1.0f), tMin = 5e-3f + w * (1e-1f - 5e-3f)
 *     out        closest hit (default): min(max(t / rayLength, 0), 1) with the selects of RAY QUERIES, 1 on a miss; deviceHits, when
 *                given, gets the ChordRayHit of chordvis_trace_rays for that ray.  CHORD_PIXEL_RAYS_ANY_HIT: 0 when a candidate exists,
 *                1 otherwise; no hit records.
 *     A ray with a non-finite word -- from a zero normal through 0 / 0, a non-finite table texel or position -- is a miss, as in RAY
 *     QUERIES: out = 1.  So is tMin > tMax.  No pixel faults.
 *   NOT HERE: the reference writes pow(out, power).  No pow is pinned on the device, so the exponent stays with the consumer, whose
 *   denoiser reads this image next.  Several rays per pixel: call once per table slice and accumulate.
 *   CHORDVIS_E_INVALID, chordvis_last_error naming the rule, everything checked before the device is touched and no device pointer
 *   dereferenced on the host: every refusal of chordvis_trace_rays, in its order (a depth-view child context; no scene; no ray scene, or
 *   one dropped since; a call before the refit an object change requires); a NULL desc; an unknown mode or flag bit; HEMISPHERE with a
 *   NULL table or a table dimension that is zero or no power of two; START_FROM_DEPTH without deviceZ; a deviceZStride of 0 with a
 *   deviceZ; ANY_HIT with deviceHits; FRONT_ONLY outside DIRECTION; width * height beyond 2^32 - 1; and, for an image that is not empty,
 *   a NULL or 16-byte-misaligned position, normal (HEMISPHERE, FRONT_ONLY), table (HEMISPHERE) or hits pointer where it is needed, a
 *   NULL or 4-byte-misaligned deviceOut, a 4-byte-misaligned deviceZ.
 * tests/test_pixel_rays_host.py runs the per-pixel code on the host under the address and undefined-behaviour sanitizers;
 * tests/test_gpu_pixel_rays.py holds the statements above on the GPU, but the refusal on a depth-view child context, which no entry
 * point hands out (read from the code). */
int chordvis_pixel_rays(ChordCtx* ctx, const ChordPixelRaysDesc* desc, const float* devicePosition /* float4 */,
                        const float* deviceNormal /* float4 */, const float* deviceZ /* or NULL */,
                        const float* deviceTable /* float4, HEMISPHERE only */, float* deviceOut /* float */,
                        ChordRayHit* deviceHits /* or NULL */);

/* uploadBufferToGPU("PerViewCamera") + ("MainViewInstanceCullingInfo") renderer.cpp:246,262
 * and the r.instanceculling.* cvars -> switchFlags (instance_culling.cpp:22-68). */
int chordvis_set_view(ChordCtx* ctx, const ChordCameraView* view, const ChordInstanceCullingView* instanceView,
                      uint32_t switchFlags);

/* How instanceCulling walks a primitive's cluster groups.  0 (default): flat, one thread per (object, group) like the
 * reference's dispatch (instance_culling.cpp:144-157; it uploads the BVH and never reads it, instance_culling.hlsl:96-99).
 * 1: hierarchical -- resident waves walk every visible object's GPUBVHNode tree (ChordAssetDesc::bvhNodes) and drop a
 * subtree when its sphere, which bounds the parent-error spheres beneath it, already projects below the LOD
 * threshold; only the groups of surviving nodes are tested.  The command list is the same array either way. */
int chordvis_set_cull_mode(ChordCtx* ctx, int hierarchical);

/* Tile schedules of a frame's raster passes (no counterpart: the reference's hardware rasterizer schedules its own tiles).  The first
 * pass writes every tile of the target, so its work items never change; only their order (heaviest bin first) and the cut of long bins
 * depend on the frame.  With `frames` != 0 (default 1) a pass runs under the schedule the SAME pass of the frame before left behind:
 * one workgroup of that frame's tile kernel orders its bin counts for the next frame while the others raster, so no frame launches a
 * schedule kernel and every schedule is exactly one frame old (frames inside chordvis_render_frame / the frame phases; a heavy second
 * pass the same way -- its schedule lists every tile, touched or not).  The first frame after a new target, scene, tile map or switch
 * makes its schedules with the schedule kernel.  0: a fresh schedule from the schedule kernel in every pass.  Order and cut are choices
 * of speed -- the image is the same with any; a host may ignore camera cuts: a stale order costs balance for one frame, never a pixel.
 * (Measured: along a moving camera path a one-frame-old schedule is as good as a fresh one; one reused for 3 / 7 frames -- what a
 * value > 1 meant until round 6 and still means under CHORDVIS_TILE_NEXT=0 -- costs a 30 k-cluster frame 3 / 7 %.) */
int chordvis_set_tile_schedule_keep(ChordCtx* ctx, uint32_t frames);
uint32_t chordvis_tile_schedule_keep(ChordCtx* ctx);

/* allocateGBufferTextures (render_textures.cpp:20-45): size the visibility target.  deviceVisibility
 * may be a caller-owned device buffer of chordvis_visibility_words(ctx) uint64 (used for the
 * multi-GPU all-gather), or NULL for a context-owned one.
 * May be called again on a live context, with any size and either kind of buffer.  Everything sized by the target or made for
 * it goes: the history HZB (chordvis_history_hzb is refused until a frame has run; that frame is one without history), the kept
 * tile schedules and the passes' reports, handles of tile markers and shading-tile lists (chordvis_prepare_shading_tile_param
 * refuses a marker made for another size).  A view of another renderDimension no longer fits: until chordvis_set_view has come
 * with the new size, the passes, chordvis_render_frame, the frame phases, chordvis_instance_culling_view and
 * chordvis_render_shadow are refused (CHORDVIS_E_INVALID), and a chordvis_set_view with any other size is refused and changes
 * nothing.  The scene, bound objects, the depth views and the cascade cache (which depend on the view, not on the size) stay. */
int chordvis_allocate_gbuffer(ChordCtx* ctx, uint32_t width, uint32_t height, uint64_t* deviceVisibility);

int chordvis_set_limits(ChordCtx* ctx, const ChordLimits* limits);
/* Multi-GPU screen ownership (the reference is single-device): the screen is cut into the rasterizer's 64 x 64-pixel
 * tiles and every tile belongs to one rank -- a table tile -> owner, row-major over the tile grid (ceil(W / 64) columns), the
 * same on every rank of a frame.  The visibility buffer of a sharded context is stored rank-major and tile-linear: a rank's
 * tiles sit in consecutive slots of 64 x 64 words (64 rows of 64) of the rank's chunk, chunk = the largest tile count of the
 * current map in slots (ceil(tiles / ranks) under the default map, up to chordvis_tile_slot_capacity under a weighted one), so one
 * in-place all-gather reassembles the frame and a de-tile kernel restores row-major.  ranks == 1: plain row-major.
 * chordvis_set_shard installs the default map, chordvis_tile_layout(width, height, ranks, NULL, ...): the tile grid is walked
 * along a generalised Hilbert curve and cut into `ranks` runs of equal length -- compact regions, so that few clusters touch
 * two ranks' tiles (such a cluster is set up by both). */
int chordvis_set_shard(ChordCtx* ctx, uint32_t ranks, uint32_t rank);
uint32_t chordvis_tile_count(uint32_t width, uint32_t height);
uint32_t chordvis_tile_slots_per_rank(uint32_t width, uint32_t height, uint32_t ranks);   /* ceil(tiles / ranks): a rank's tiles under the default map */
/* Tile slots a sharded context ALLOCATES per rank: a quarter more than that, room for a load-balanced map to give a rank of
 * light tiles more of them.  What the all-gathers move is ranks x (the largest tile count of the current map) slots
 * (chordvis_visibility_chunk_words and the exchange chunk sizes follow the map). */
uint32_t chordvis_tile_slot_capacity(uint32_t width, uint32_t height, uint32_t ranks);
/* The map as a function (host only, deterministic: every rank computes the same table from the same inputs).  loads NULL:
 * the default above.  loads = bin entries per tile of a rendered frame (chordvis_read_tile_loads): regions of equal LOAD along
 * the same curve; tiles heavier than a quarter of a rank's share are placed one by one (heaviest first, least loaded rank),
 * near-empty tiles fill every rank up to its tile count, each joining the region next to it on the curve while that region has
 * room.  Never more than maxTilesPerRank tiles per rank (0: ceil(tiles / ranks);
 * chordvis_rebalance passes chordvis_tile_slot_capacity). */
int chordvis_tile_layout(uint32_t width, uint32_t height, uint32_t ranks, const uint32_t* loads, uint32_t maxTilesPerRank, uint8_t* ownersOut);
/* An explicit map, between frames (drains frames in flight; the history HZB carries over: it is not sharded).  owners NULL:
 * back to the default map. */
int chordvis_set_tile_owners(ChordCtx* ctx, const uint8_t* owners, uint32_t tiles);
int chordvis_get_tile_owners(ChordCtx* ctx, uint8_t* ownersOut, uint32_t tiles);
/* Bin entries per tile of the last frame, EVERY rank's tiles (they travel in the end-of-frame exchange); waits for the stream. */
int chordvis_read_tile_loads(ChordCtx* ctx, uint32_t* loadsOut, uint32_t tiles);
/* read_tile_loads -> tile_layout -> set_tile_owners.  Every rank calls it at the same frame boundary (same loads -> same map).
 * imbalancePermille (may be NULL): the OLD map's heaviest rank / the mean, x 1000. */
int chordvis_rebalance(ChordCtx* ctx, uint32_t* imbalancePermille);
/* Number of uint64 words of the (rank-major, tile-linear when sharded) visibility buffer as allocated, and of one rank's chunk
 * under the current tile map (the all-gather's count; rank r's chunk starts at r x that). */
uint64_t chordvis_visibility_words(ChordCtx* ctx);
uint64_t chordvis_visibility_chunk_words(ChordCtx* ctx);
/* Device pointer of the visibility buffer in use (row-major when ranks == 1). */
uint64_t* chordvis_visibility_ptr(ChordCtx* ctx);

/* ------------------------------------------------------------------ passes (stream-ordered) */

/* addClearGbufferPass — render_textures.cpp:74-102 (visibility = 0, depth = 0.0). */
int chordvis_clear_gbuffer(ChordCtx* ctx);

/* instanceCulling — instance_culling.cpp:83-161 (instanceCullingCS + clusterGroupCullingCS).
 * Slots are assigned in deterministic (objectId, groupIdx, meshlet) order. */
int chordvis_instance_culling(ChordCtx* ctx, ChordCountAndCmd* out);

/* detail::hzbCulling — instance_culling.cpp:286-351 (hzbMainViewCullingCS).
 * bFirstStage: project with last-frame matrices, also emit the rejected list. */
int chordvis_hzb_culling(ChordCtx* ctx, const ChordHZB* hzb, int bFirstStage, ChordCountAndCmd in,
                         ChordCountAndCmd* outVisible, ChordCountAndCmd* outRejected);

/* renderMesh — mesh_raster.cpp:208-254: the 4 material buckets (filterPipeForVisibility + renderMeshRasterPipe, alphaMode
 * 0/1 x two-sided 0/1) collapse into one software-raster pass that reads bTwoSided and alphaMode per cluster.  Masked
 * materials (mesh_raster.hlsl:34-38,107-112,198-204) are alpha-tested per pixel with a software texture fetch whose
 * level of detail and filter are pinned (the reference leaves them to the sampler hardware);
 * blended materials (alphaMode 2) are in no bucket and draw nothing, as in the reference. */
int chordvis_render_mesh(ChordCtx* ctx, ChordCountAndCmd in);

/* gltfVisibilityRenderingStage0 — mesh_raster.cpp:269-311.  hzbPrev NULL/invalid or HZB culling
 * disabled => draws `in`, *shouldStage1 = 0. */
int chordvis_visibility_stage0(ChordCtx* ctx, const ChordHZB* hzbPrev, ChordCountAndCmd in,
                               ChordCountAndCmd* outRejected, int* shouldStage1);

/* gltfVisibilityRenderingStage1 — mesh_raster.cpp:313-329. */
int chordvis_visibility_stage1(ChordCtx* ctx, const ChordHZB* hzb, ChordCountAndCmd in);

/* buildHZB — hzb.cpp:38-227 from the depth half of the visibility words.
 * slot 0 = temporary (post stage 0), slots 1/2 = history ping-pong. */
int chordvis_build_hzb(ChordCtx* ctx, int bBuildMin, int bBuildMax, int bBuildValidRange, int slot, ChordHZB* out);

/* DeferredRenderer::render hot segment (renderer.cpp:315-345,489): clear -> instanceCulling ->
 * stage0 -> [buildHZB -> stage1] -> buildHZB(min,max,validRange); keeps the HZB as history for
 * the next call.  On a sharded context (ranks > 1) this needs a communicator (chordvis_comm_init_rank below) and runs the
 * three phases with the two all-gathers in between; a host that owns its collectives (e.g. torch.distributed) drives
 * the phases itself -- on the context's stream, so that kernels and collectives are ordered:
 *   chordvis_frame_phase_cull  (optional; 2..8 ranks, flat cull mode) the sharded group cull (SURVEY 8e "shard by object range"): the
 *                           object pass + the group / meshlet tests of THIS rank's share of the group instances only, one word per group
 *                           instance into the rank's chunk of the cull exchange buffer: byte i = the set of ranks whose tiles meshlet i of the
 *                           group touches, 0 = culled.  A frame that starts at phase a instead tests every group on every rank.
 *   [all-gather the cull exchange buffer: chordvis_cull_exchange_ptr, chunk = chordvis_cull_exchange_chunk_bytes]
 *   chordvis_frame_phase_a  clear .. stage 0 raster of the rank's tiles; the tile kernel also reduces every tile to its HZB texels
 *                           (mips 0..5), into the tile's slots of the two exchange buffers
 *   [all-gather the mid-frame exchange buffer: chordvis_hzb_exchange_ptr, chunk = chordvis_hzb_exchange_chunk_halves]
 *   chordvis_frame_phase_b  HZB chain from the exchanged texels, stage 1 cull + raster
 *   [all-gather the end-of-frame exchange buffer (chordvis_hzb_final_exchange_ptr / _chunk_bytes) and the visibility buffer, in place]
 *   chordvis_frame_phase_c  row-major copy of the image, history HZB from the exchanged texels, history swap            */
int chordvis_render_frame(ChordCtx* ctx);
int chordvis_frame_phase_cull(ChordCtx* ctx);
/* cull exchange buffer: ranks x (B x 256 mask words + B triangle sums), B = ceil(count blocks / ranks); made on the first request after
 * chordvis_upload_scene + chordvis_set_shard (NULL / 0 when the sharded cull does not apply: one rank, more than 8, no scene) */
uint32_t* chordvis_cull_exchange_ptr(ChordCtx* ctx);
uint64_t chordvis_cull_exchange_chunk_bytes(ChordCtx* ctx);   /* one rank */
int chordvis_frame_phase_a(ChordCtx* ctx);
int chordvis_frame_phase_b(ChordCtx* ctx);
int chordvis_frame_phase_c(ChordCtx* ctx);
/* Pipelined form of phase c, for hosts that let the visibility all-gather of frame i travel beside frame i + 1 (two frames'
 * words alive: chordvis_swap_visibility before every phase a).  The history HZB needs only the small end-of-frame exchange:
 *   [all-gather chordvis_hzb_final_exchange_ptr]
 *   chordvis_frame_phase_c_finish   the history chain from the exchanged texels, history swap; the frame is over
 *   [whenever the visibility all-gather of the frame has landed: chordvis_frame_resolve_visibility, on any stream]   */
int chordvis_frame_phase_c_finish(ChordCtx* ctx);
int chordvis_frame_resolve_visibility(ChordCtx* ctx, void* hipStream /* NULL: the context's */);
int chordvis_swap_visibility(ChordCtx* ctx);
/* end-of-frame exchange buffer: per tile slot the min and max chains' texels (mips 0..5), the tile's valid range and bin length */
uint16_t* chordvis_hzb_final_exchange_ptr(ChordCtx* ctx);
uint64_t chordvis_hzb_final_exchange_chunk_bytes(ChordCtx* ctx);   /* one rank */
int chordvis_reset_history(ChordCtx* ctx);
/* mid-frame exchange buffer: per tile slot the min chain's texels (mips 0..5, f16) after the first raster pass, rank-major */
uint16_t* chordvis_hzb_exchange_ptr(ChordCtx* ctx);
uint64_t chordvis_hzb_exchange_halves(ChordCtx* ctx);        /* whole buffer */
uint64_t chordvis_hzb_exchange_chunk_halves(ChordCtx* ctx);  /* one rank     */
/* row-major visibility after phase_c (== chordvis_visibility_ptr when ranks == 1) */
uint64_t* chordvis_resolved_visibility_ptr(ChordCtx* ctx);

/* ------------------------------------------------------------------ multi-GPU (the reference is single-device,
 * graphics.cpp:524-548).  The frame shards by screen tiles (chordvis_set_shard); the exchanges of a sharded frame -- the owned
 * tiles' HZB texels between the raster passes, their HZB texels and visibility words at the end -- are issued by the library,
 * so the host keeps ONE call per frame, like DeferredRenderer::render (renderer.cpp:319-345). */

/* (a) one process per GPU (torch.distributed / MPI hosts): attach an RCCL communicator to a sharded context; from then on
 * chordvis_render_frame(ctx) runs phase a -> ncclAllGather -> phase b -> ncclAllGather -> phase c on the context's stream.
 * Rank 0 makes the id (ncclGetUniqueId), the host distributes the 128 bytes by its own means, every rank calls init_rank
 * after chordvis_set_shard(nranks, rank).  librccl.so is resolved at run time, preferring a copy already loaded
 * into the process (CHORDVIS_RCCL=<path> overrides). */
#define CHORDVIS_UNIQUE_ID_BYTES 128
int chordvis_comm_unique_id(void* out128);
int chordvis_comm_init_rank(ChordCtx* ctx, uint32_t nranks, uint32_t rank, const void* id128);
int chordvis_comm_destroy(ChordCtx* ctx);
/* Pipelined frames over RCCL (the ChordGroup form: chordvis_group_set_pipelined below).  id128: a SECOND unique id (the same
 * on every rank) for the communicator that carries the image of frame i, on a stream of its own, beside frame i + 1; the
 * history HZB then waits only for the small end-of-frame exchange, not for the image.  chordvis_readback_visibility / chordvis_visibility_mark / chordvis_wait_visibility wait for the image.
 * NULL switches back to the plain protocol.  The context must own its visibility buffer.
 * Two communicators of one process run on two streams of one device, and RCCL orders collectives per communicator only.
 * What makes that safe here: (1) each communicator is used from exactly one stream, always the same one; (2) every rank
 * issues the same collectives in the same order on each communicator (frame after frame: small, image, small -- whether the
 * mid-frame exchange happens is decided from state every rank shares); (3) no collective of one communicator waits, on the
 * device, for a LATER collective of the other on any rank: the image gather waits for the compute stream's "phase b done"
 * event, which lies before the next small exchange.  A host that adds collectives of its own must keep (1)-(3), and must not
 * run a blocking call (hipMalloc, hipFree, a synchronous copy) on one rank between the two enqueues while its peers are
 * already inside them -- the usual NCCL multi-communicator rule.  With one rank (all a one-GPU box can host) the call sets up
 * the same second communicator, stream and events; the frame is the unsharded one followed by the image step.
 * A frame that fails on one rank (capacity, HIP error) still issues every collective of the frame, so its peers do not hang,
 * returns the first error, and leaves the context outside a frame: the next chordvis_render_frame starts clean (its history is
 * the last complete frame's only if the host calls chordvis_reset_history on EVERY rank; otherwise that rank culls against a
 * chain its peers do not share and the images may differ -- treat a failed frame as a reason to reset or to stop). */
int chordvis_comm_set_pipelined(ChordCtx* ctx, const void* id128);
/* NCCL_VERSION_CODE of the loaded library, ranks of ctx's communicator (0 = none; ctx may be NULL), where librccl came from */
int chordvis_comm_info(ChordCtx* ctx, int* ncclVersion, uint32_t* nranks, char* libraryOrigin, uint32_t originBytes);

/* (b) one process, n devices: one context + one host thread per device; the exchanges are direct all-gathers -- every rank
 * pushes its chunk to each peer with its own hipMemcpyPeerAsync (n-1 concurrent copies per rank, one per xGMI link).
 * Ordinals may repeat (protocol tests on a one-GPU box).  The scene is replicated; per-rank readback and stats go through
 * chordvis_group_ctx(group, rank) (borrowed; every rank ends a frame with the complete row-major image and HZB). */
typedef struct ChordGroup ChordGroup;
int chordvis_create_group(uint32_t n, const int* deviceOrdinals, ChordGroup** outGroup);
int chordvis_destroy_group(ChordGroup* group);
uint32_t chordvis_group_size(ChordGroup* group);
ChordCtx* chordvis_group_ctx(ChordGroup* group, uint32_t rank);
const char* chordvis_group_last_error(ChordGroup* group);
int chordvis_group_set_limits(ChordGroup* group, const ChordLimits* limits);
int chordvis_group_upload_scene(ChordGroup* group, const ChordSceneDesc* scene);
int chordvis_group_allocate_gbuffer(ChordGroup* group, uint32_t width, uint32_t height);
/* chordvis_rebalance on every rank (drains the frames in flight first) */
int chordvis_group_rebalance(ChordGroup* group, uint32_t* imbalancePermille);
int chordvis_group_update_objects(ChordGroup* group, const ChordObject* hostObjects, uint32_t count);
/* chordvis_set_object_list on every rank (the list is replicated like the scene; a list one rank refuses every rank refuses, and
 * each keeps the list it had).  On the sharded ranks the call re-makes the cull exchange buffer for the new count blocks. */
int chordvis_group_set_object_list(ChordGroup* group, const ChordObject* hostObjects, uint32_t count);
/* chordvis_upload_world_transforms / chordvis_build_objects on every rank (the transforms are replicated like the scene).  There is no
 * group scatter: the device arrays are per device, so a host that needs one goes through the ranks' contexts (chordvis_group_ctx). */
int chordvis_group_upload_world_transforms(ChordGroup* group, const double* hostLocalToWorld, const double* hostPrevLocalToWorld, uint32_t count);
int chordvis_group_build_objects(ChordGroup* group, const double cameraPos[3], const double cameraPosLast[3]);
int chordvis_group_set_view(ChordGroup* group, const ChordCameraView* view, const ChordInstanceCullingView* instanceView, uint32_t switchFlags);
/* DeferredRenderer::render hot segment (renderer.cpp:315-345,489) on n devices; returns when the frame is ENQUEUED on every
 * device (no host synchronisation; chordvis_group_sync waits) */
int chordvis_group_render_frame(ChordGroup* group);
int chordvis_group_sync(ChordGroup* group);
/* mean host time per frame (ms) each rank's worker spent inside chordvis_group_render_frame since the last call; n = group size */
int chordvis_group_enqueue_ms(ChordGroup* group, double* msPerRank, uint32_t n);
/* Pipelined frames: chordvis_group_render_frame returns once frame i is enqueued with its visibility all-gather and row-major
 * copy running beside whatever follows (frame i + 1); every rank's history HZB is complete at the end of the call's work as
 * before.  chordvis_readback_visibility / the consumer entry points of a rank's context wait for ITS image;
 * chordvis_readback_previous_visibility reads the frame before the last submitted one. */
int chordvis_group_set_pipelined(ChordGroup* group, int enable);

/* ------------------------------------------------------------------ depth-only views (what renderShadow runs per
 * cascade, mesh_raster.cpp:331-546).  Every pass of the reference takes (instanceViewId, instanceViewOffset) -- a buffer of
 * InstanceCullingViewInfo and an index into it (gltf_rendering.h:38-43,54-64,89-110); here the buffer is set once and the
 * passes take the offset.  Views have their own square size (CascadeShadowMapConfig::cascadeDim, render_helper.h:469). */
typedef struct ChordDepthTarget {     /* a VK_FORMAT_D32_SFLOAT image (mesh_raster.cpp:407-416): device floats, row-major, reverse-Z, clear 0 */
    float*   depth;
    uint32_t width, height;
} ChordDepthTarget;
/* after upload_scene: targets + work lists for `viewCount` views of dim x dim pixels.  Called again -- with the same dim and count
 * too -- it makes new, empty images and drops the cascade cache of chordvis_render_shadow with the old ones (bCacheValid,
 * mesh_raster.cpp:367-371, wants depth images that exist): the next chordvis_render_shadow renders every cascade. */
int chordvis_allocate_depth_views(ChordCtx* ctx, uint32_t dim, uint32_t viewCount);
/* the InstanceCullingViewInfo[] of the views ("CascadeViewInfos", mesh_raster.cpp:417-421); host array, copied */
int chordvis_set_instance_views(ChordCtx* ctx, const ChordInstanceCullingView* hostViews, uint32_t count);
/* instanceCulling(queue, ctx, instanceCullingViewInfo, instanceCullingViewInfoOffset) for a view other than the main one
 * (mesh_raster.cpp:452): object / meshlet frustum tests against the view (orthoFrustumCulling for an orthographic one,
 * base.hlsli:251-272), LOD cut by the MAIN camera (chordvis_set_view).  The list stays valid until the next call. */
int chordvis_instance_culling_view(ChordCtx* ctx, uint32_t instanceViewOffset, ChordCountAndCmd* out);
/* detail::hzbCullingGeneric (instance_culling.cpp:232-284, hzb_culling_generic.hlsl): one-pass occlusion cull of a view's list
 * against an HZB of that view's depth (chordvis_build_hzb_from_depth) */
int chordvis_hzb_culling_generic(ChordCtx* ctx, const ChordHZB* hzb, float extentScale, uint32_t instanceViewOffset,
                                 int bObjectUseLastFrameProject, ChordCountAndCmd in, ChordCountAndCmd* out);
/* queue.clearDepthStencil(depth, 0) + renderMeshDepth(PASS_TYPE_DEPTH) (mesh_raster.cpp:159-206,500-522): both alpha buckets,
 * cull mode NONE, depth test GREATER_OR_EQUAL, optional depth clamp and vkCmdSetDepthBias(const, 0, slope).  The view must
 * be the one of the last chordvis_instance_culling_view. */
int chordvis_render_mesh_depth(ChordCtx* ctx, uint32_t instanceViewOffset, int bDepthClamped, float depthBiasConst, float depthBiasSlope,
                               ChordCountAndCmd in, ChordDepthTarget* out);
/* buildHZB(queue, depth, true, false, false) on a depth target (mesh_raster.cpp:466,527) */
int chordvis_build_hzb_from_depth(ChordCtx* ctx, const ChordDepthTarget* depth, ChordHZB* out);
int chordvis_readback_depth(ChordCtx* ctx, const ChordDepthTarget* depth, float* host);
/* renderShadow (mesh_raster.cpp:331-546): cascade setup, then per cascade from the farthest to the nearest: instanceCulling for
 * its view, hzbCullingGeneric against the previous cascade's HZB (or, for the first one, against the HZB of its own cached
 * depth from last frame's view), clear + renderMeshDepth with depth clamp and the configured bias, buildHZB.  The context
 * keeps the depth images and views from call to call (CascadeShadowHistory): with an unchanged config and light direction
 * the far cascades are refreshed one per tick (isCascadeCacheValid, cascade_setup.hlsl:8-22).  validDepthMinMax: the
 * valid range of the main view's last buildHZB (chordvis_readback_hzb) or NULL.  outRenderedMask: bit i = cascade i was
 * re-rendered by this call. */
int chordvis_render_shadow(ChordCtx* ctx, const ChordCascadeConfig* config, const float lightDir[3], const uint32_t validDepthMinMax[2],
                           uint32_t tickCount, int bHzbCulling, ChordDepthTarget* outDepths /* [cascadeCount] or NULL */,
                           ChordInstanceCullingView* outViews /* [cascadeCount] or NULL */, uint32_t* outRenderedMask);
/* chordvis_stats of the depth views' last pass (overflow flag, record / bin counts) */
int chordvis_depth_view_stats(ChordCtx* ctx, ChordStats* out);

/* handles of the last frame (post-instanceCulling list: consumer contract, lighting.hlsl:318-345) */
int chordvis_last_frame_cmds(ChordCtx* ctx, ChordCountAndCmd* out);
int chordvis_history_hzb(ChordCtx* ctx, ChordHZB* out);

/* ------------------------------------------------------------------ consumers' first step */
/* visibilityMark — visibility_tile.cpp:20-57 (tilerMarkerCS, visibility_tile.hlsl:65-134): marks, per 8x8 pixels of
 * the (resolved, row-major) visibility buffer, which material shading types occur.  drawedMeshletCmd = the list
 * the visibility ids index, i.e. chordvis_last_frame_cmds (renderer.cpp:354,359). */
int chordvis_visibility_mark(ChordCtx* ctx, ChordCountAndCmd drawedMeshletCmd, ChordTileMarker* out);
/* Consumers that read chordvis_resolved_visibility_ptr() on a stream of their own (lighting.hlsl:318-329 is the reference's):
 * orders `hipStream` (NULL: the context's) behind the completion of the last submitted frame's image.  After pipelined
 * ChordGroup frames the image is gathered beside the context's stream, so this -- or one of the library's own consumers /
 * read-backs, which wait by themselves -- must come before the first read. */
int chordvis_wait_visibility(ChordCtx* ctx, void* hipStream);
/* prepareShadingTileParam — visibility_tile.cpp:59-110 (tilePrepareCS + prepareTileParamCS, visibility_tile.hlsl:136-219) */
int chordvis_prepare_shading_tile_param(ChordCtx* ctx, uint32_t shadingType, const ChordTileMarker* marker, ChordShadingTiles* out);

/* ------------------------------------------------------------------ per-pixel attributes of the visible triangle */
/* lighting.hlsl:278-371 (getTriangleMiscInfo, nanite_shared.hlsli:111-179) / material.hlsli:41-64 / nanite_debug.hlsl:
 * pixel -> visibility word -> draw command -> object, meshlet, triangle -> three vertices -> perspective-correct barycentrics
 * and their screen derivatives (calculateTriangleBarycentrics, base.hlsli:457-495) -> interpolated attributes. */
#define CHORD_NANITE_DEBUG_MESHLET      0u   /* simpleHashColor(meshlet id)           nanite_debug.hlsl:6-10 */
#define CHORD_NANITE_DEBUG_TRIANGLE     1u   /* simpleHashColor(triangle index word)  */
#define CHORD_NANITE_DEBUG_LOD          2u   /* LOD palette                            */
#define CHORD_NANITE_DEBUG_LOD_MESHLET  3u   /* pow(meshlet colour, 0.5) x LOD palette */
#define CHORD_NANITE_DEBUG_BARYCENTRICS 4u
typedef struct ChordResolveDesc {
    ChordMat4 translatedWorldToClipNoJitter;           /* read when useNoJitter != 0 (motion vectors only)                           */
    ChordMat4 translatedWorldToClipLastFrameNoJitter;
    uint32_t  useNoJitter;     /* 0: motion from the frame's own VP and VP_last (== the reference when jitter is 0)                   */
    uint32_t  debugMode;       /* CHORD_NANITE_DEBUG_*, for debugRGBA8                                                              */
    uint32_t  pad[2];
} ChordResolveDesc;
/* Caller-owned DEVICE images of width x height texels, row-major; NULL = not written; at least one non-NULL.  An empty pixel (id 0)
 * or one whose id is not below the list's count holds 0 in every image, and opaque black (0xFF000000) in debugRGBA8. */
typedef struct ChordResolveTargets {
    float*    barycentrics;   /* float4: interpolation.xyz, 0                   */
    float*    baryDdx;        /* float4: ddx.xyz, 0                             */
    float*    baryDdy;        /* float4: ddy.xyz, 0                             */
    float*    uv;             /* float2: texcoord0 ((0, 0) when the scene has none) */
    float*    uvGrad;         /* float4: du/dx, dv/dx, du/dy, dv/dy             */
    float*    positionRS;     /* float4: translated-world position xyz, 1       */
    float*    motionVector;   /* float2: material.hlsli:55-61                   */
    uint32_t* debugRGBA8;     /* R in the low byte                              */
} ChordResolveTargets;
/* One launch on the context's stream over the image chordvis_visibility_mark reads (the resolved one of a sharded context), after
 * the same wait for it.  drawedMeshletCmd = the list the ids index (chordvis_last_frame_cmds).  The matrices are the objects' and
 * the view's of the frame that made the image: CHORDVIS_E_INVALID after chordvis_update_objects / chordvis_bind_objects /
 * chordvis_set_view until the next frame, and before the first one.  The contents of an array bound with chordvis_bind_objects
 * are the caller's to keep unchanged from the frame until the resolve has run (the library cannot see a write into it).
 * desc NULL: all zero. */
int chordvis_resolve_attributes(ChordCtx* ctx, ChordCountAndCmd drawedMeshletCmd, const ChordResolveDesc* desc,
                                const ChordResolveTargets* targets);
/* The surface frame of the visible triangle -- getTriangleMiscInfo (nanite_shared.hlsli:157-175) and
 * loadGLTFMetallicRoughnessPBRMaterial (material.hlsli:95-108).  Per vertex, float32, every step in source order:
 *   nRS = normalize(mul(float4(nLS, 0), translatedWorldToLocal).xyz)   row-vector product (the inverse transpose), component j
 *                                                                      = (x * m0j + y * m1j) + z * m2j (the w = 0 term dropped)
 *   t   = mul(localToTranslatedWorld, float4(tLS.xyz, 0)).xyz          component i = (mi0 * x + mi1 * y) + mi2 * z
 *   tRS = normalize(t - dot(t, nRS) * nRS)                             (Gram-Schmidt)
 *   bRS = cross(nRS, tRS) * tLS.w
 * normalize(v) = v / sqrt(dot(v, v)), dot = (x * x + y * y) + z * z, each component divided separately.  Departure: a vector
 * whose dot(v, v) is not above 0 normalises to 0, not NaN (a G-buffer carries no NaN).  Per pixel each is interpolated with the
 * barycentrics, (a0 * b.x + a1 * b.y) + a2 * b.z, NOT renormalised (material.hlsli:98-99).  The reference forms tangents only
 * for materials with a normal texture; here they are formed whenever the scene has tangents.  Caller-owned device images as in
 * ChordResolveTargets; empty pixels hold 0. */
typedef struct ChordSurfaceTargets {
    float* vertexNormal; /* float4: xyz, 0 */
    float* tangent;      /* float4: xyz, 0 */
    float* bitangent;    /* float4: xyz, 0 */
    float* pad;          /* must be NULL   */
} ChordSurfaceTargets;
/* chordvis_resolve_attributes plus the surface images, any subset of the eleven in ONE launch, under the same preconditions and
 * refusals; targets may be NULL.  CHORDVIS_E_INVALID also when a vertexNormal target is asked of a scene uploaded without
 * normals, or a tangent / bitangent target of one without tangents or without normals (Gram-Schmidt needs both).  Assets of a
 * scene without a stream read it as 0. */
int chordvis_resolve_surface(ChordCtx* ctx, ChordCountAndCmd drawedMeshletCmd, const ChordResolveDesc* desc,
                             const ChordResolveTargets* targets, const ChordSurfaceTargets* surface);
/* The material of the visible triangle -- loadGLTFMetallicRoughnessPBRMaterial, material.hlsli:66-153: what a lighting pass reads
 * after the surface frame.  Opt-in: chordvis_upload_scene keeps only the alpha of the textures its alpha test samples; this call,
 * AFTER chordvis_upload_scene and with the same descriptor, keeps all four channels of every level of every texture that a
 * material of the scene names in baseColorId / emissiveTexture / normalTexture / metallicRoughnessTexture (id < textureCount), and
 * a per-material record with the four (texture, sampler) pairs resolved (sampler id >= samplerCount: REPEAT, NEAREST).  A named
 * texture without data, wider or higher than 16384, or with more than 15 levels: CHORDVIS_E_INVALID, nothing kept (what an earlier
 * call kept is dropped too).  Dropped by the next chordvis_upload_scene.  Frames, culls and the other resolves do not read it. */
int chordvis_upload_material_textures(ChordCtx* ctx, const ChordSceneDesc* scene);
/* Block-compressed textures (ChordTexture::format = CHORD_TEXFMT_BC1_RGB / BC3 / BC4 / BC5).  Both upload calls take them: the
 * compressed bytes of the textures they look at go to one staging buffer on the device, ONE kernel launch on the context's stream
 * expands every level of every such texture into the texel store RGBA8 textures are copied to (chordvis_upload_material_textures:
 * all four channels; chordvis_upload_scene: the alpha the masked buckets test -- BC3 decodes its alpha block, the other block
 * formats are 255 throughout), and the staging buffer is freed after the synchronise: the calls stay synchronous, the offsets of
 * every level are those of an RGBA8 texture of the same size, and nothing downstream knows the difference.  The decode is pinned
 * (DESIGN.md 2 item 9(h)).  A format other than 0..4 on a texture a call looks at: CHORDVIS_E_INVALID, chordvis_last_error names
 * the allowed values; textures nothing names are ignored, their format included.
 * Size in bytes of a chain in the layout ChordTexture wants (host call, no context), for RGBA8 as well.  An unknown format, a zero
 * width, height or mipCount, or NULL `bytes`: CHORDVIS_E_INVALID. */
int chordvis_texture_chain_bytes(uint32_t format, uint32_t width, uint32_t height, uint32_t mipCount, uint64_t* bytes);
/* The expanded texels of one level of a texture as chordvis_resolve_material reads them (RGBA8, width x height of the level,
 * row-major; RGBA8 textures too); synchronises.  CHORDVIS_E_INVALID when no material textures are uploaded, when no material of the
 * scene names the texture, or when the level is not below its mipCount. */
int chordvis_readback_material_texture(ChordCtx* ctx, uint32_t textureId, uint32_t level, uint8_t* hostRgba8);
/* Mip chains built on the GPU at upload (opt-in per texture).  Entry i belongs to texture id i of the
 * descriptors given to LATER chordvis_upload_scene / chordvis_upload_material_textures calls; textures at or beyond `count` have
 * none.  The entries are copied and held per context, across both uploads (as the anisotropy setting is); both uploads read them.
 *   levels        0: the texture stays as supplied.  Otherwise it ends up with L = min(levels, full) levels, full =
 *                 bit_length(max(width, height)) (down to 1 x 1; at most 15).  The host supplies the first mipCount levels in the
 *                 layout of ChordTexture; where L > mipCount, levels mipCount .. L-1 are made on the device from the last supplied
 *                 one (a block-compressed one is decoded first; made levels live in the RGBA8 / alpha stores only), and every
 *                 level count downstream is L: the samplers see a longer chain, chordvis_readback_material_texture reaches the
 *                 made levels, the 4 G texel caps of the uploads count them (CHORDVIS_E_CAPACITY, nothing kept).  Where
 *                 L <= mipCount nothing changes for the texture.
 *   flags         level l+1 is a 2 x 2 box of level l (texel (x, y) from columns min(2x, w-1), min(2x+1, w-1), rows likewise: an
 *                 odd size drops its last column / row), (sum of four codes + 2) >> 2 per channel.  CHORD_TEXMIPS_SRGB: r, g, b
 *                 are averaged in linear light instead (decoded through the table of chordvis_material_constants, the nearest
 *                 code of the float32 mean); chordvis_upload_scene stores alpha only and ignores it.  CHORD_TEXMIPS_COVERAGE: the
 *                 alpha of every MADE level is rescaled, a' = min(255, a * alphaCutoff8 / t'), with t' chosen per level so that
 *                 the share of texels with a' >= alphaCutoff8 is, as nearly as the level's alpha values allow and not below, the
 *                 share of level 0's texels with a >= alphaCutoff8.  Supplied levels are never changed.
 *   alphaCutoff8  the cutoff as an 8-bit code, 1..255; read only with CHORD_TEXMIPS_COVERAGE.
 * CHORDVIS_E_INVALID, the setting unchanged, chordvis_last_error naming the allowed values: a flag bit other than the two, a
 * non-zero pad, or CHORD_TEXMIPS_COVERAGE with alphaCutoff8 outside 1..255.  NULL or count 0: no texture has a setting (the
 * default: both uploads launch and store exactly what they do without this call).  On a ChordGroup, set the ranks' contexts
 * before the group's scene upload. */
#define CHORD_TEXMIPS_SRGB      1u          /* r, g, b averaged in linear light; alpha is always averaged as a code */
#define CHORD_TEXMIPS_COVERAGE  2u          /* rescale the alpha of generated levels to keep level 0's coverage at alphaCutoff8 */
#define CHORD_TEXMIPS_FULL      0xFFFFFFFFu /* levels: down to 1 x 1 */
typedef struct ChordTextureMips { uint32_t levels, flags, alphaCutoff8, pad; } ChordTextureMips;
int chordvis_set_texture_mips(ChordCtx* ctx, const ChordTextureMips* perTexture, uint32_t count);
/* What is set for one texture id; all zero at or beyond the count of the last accepted call. */
int chordvis_texture_mips(const ChordCtx* ctx, uint32_t textureId, ChordTextureMips* out);
/* Caller-owned device images as in ChordResolveTargets.  Empty pixels, pixels whose id is not below the list's count and pixels
 * whose material's materialType is not kLightingType_GLTF_MetallicRoughnessPBR (1; base.h:423, lighting.hlsl:369) hold 0.
 * Float32, source order, one rounding per operation; the texture sampler is the pinned one of DESIGN.md 2 item 9 (isotropic level
 * of detail in 1/256 steps from the bit pattern of the squared footprint, the filters and wraps of the material's glTF samplers,
 * sRGB texels decoded through a 256-entry table before filtering):
 *   baseColor    = sample(baseColorId) * baseColorFactor, rgb then mul(sRGB_2_AP1, rgb); no texture: white (1, 1, 1, 1)
 *   emissive     = sample(emissiveTexture).rgb * emissiveFactor; no texture: transparent black
 *   pixelNormal  = no normal texture: the interpolated vertex normal.  Else xy = sample.xy * 2 - 1, z = sqrt(max(0, 1 - dot(xy, xy)))
 *                  (departure: the reference's sqrt of a negative value is NaN), xy *= normalFactorScale,
 *                  mul(normalize(xyz), float3x3(tangent, bitangent, vertexNormal)) with the values of ChordSurfaceTargets
 *   roughMetalAO = metallic-roughness texture: (.g, .b, bExistOcclusion ? occlusionTextureStrength * .r : 1); none:
 *                  (roughnessFactor, metallicFactor >= 1 ? 0 : metallicFactor, 1)                              (gltf.h:53-58) */
typedef struct ChordMaterialTargets {
    float* baseColor;      /* float4: AP1 rgb, alpha                      material.hlsli:66-72,84 */
    float* emissive;       /* float4: rgb, 0                              :74-81                  */
    float* pixelNormal;    /* float4: xyz, 0                              :91-120                 */
    float* roughMetalAO;   /* float4: roughness, metallic, materialAO, 0  :122-153                */
} ChordMaterialTargets;
/* chordvis_resolve_surface plus the four material images: any subset of the fifteen in ONE launch on the same stream, under the
 * same preconditions, waits and refusals; targets and surface may be NULL.  CHORDVIS_E_INVALID also when a material target is
 * asked for and no chordvis_upload_material_textures came since the last chordvis_upload_scene; when pixelNormal is asked of a scene
 * uploaded without normals; and when pixelNormal is asked, some material has an uploaded normal texture and the scene has no
 * tangents. */
int chordvis_resolve_material(ChordCtx* ctx, ChordCountAndCmd drawedMeshletCmd, const ChordResolveDesc* desc,
                              const ChordResolveTargets* targets, const ChordSurfaceTargets* surface,
                              const ChordMaterialTargets* material);
/* Opt-in anisotropic filtering of chordvis_resolve_material's sampler: maxAnisotropy N = 1 (the default: the isotropic sampler
 * above, the same kernel and the same bits as without this call), 2, 4, 8 or 16; any other value: CHORDVIS_E_INVALID, the setting
 * unchanged, chordvis_last_error names the allowed values.  Per context (each rank of a sharded set-up sets its own); kept across
 * chordvis_upload_scene and chordvis_upload_material_textures; read by no other entry point (the visibility pass's alpha test keeps
 * its own sampler, so frames are the same at every N).  The definition, per texture slot of a pixel, with
 * ra = ax * ax + ay * ay and rb = bx * bx + by * by the squared lengths of the x and y derivatives in level-0 texels:
 *   axes    rmaj2 = max(ra, rb), rmin2 = min(ra, rb); the major axis is (dudx, dvdx) when ra >= rb, else (dudy, dvdy)
 *   logs    lmaj = lodq of rmaj2 (the isotropic sampler's lodq, same bits), lmin = lodq of rmin2, kmax = log2 N
 *   k       0 when ra or rb is not finite, rmaj2 is not above 0, or lmaj <= 0 (magnified); else
 *           min(kmax, (max(lmaj - lmin, 0) + 255) >> 8 [kmax when rmin2 is not above 0], (lmaj + 255) >> 8)
 *   level   lodq' = max(lmaj - (k << 8), 0) takes lodq's place in the levels, their fraction and clamps; min / mag still asks lmaj > 0
 *   taps    n = 1 << k; t_i = float(2i + 1 - n) * (1 / (2n)); u_i = u + dmaj_u * t_i, v_i = v + dmaj_v * t_i; each tap is the whole
 *           per-level pipeline (decode, nearest / bilinear, wraps, the two-level lerp); d = 0, d = d + (c_i - c_0) for i = 1 .. n - 1
 *           in index order, result c_0 + d * (1 / n) (equal taps give c_0 exactly).  k = 0 forms no offset: the isotropic sampler's
 *           path and bits. */
int chordvis_set_material_anisotropy(ChordCtx* ctx, uint32_t maxAnisotropy);
uint32_t chordvis_material_anisotropy(const ChordCtx* ctx);   /* the last accepted value (1 after chordvis_create) */
/* Opt-in: how LATER chordvis_upload_material_textures calls store block-compressed textures on the device.
 *   CHORD_TEXSTORE_EXPANDED (the default)  every texture is expanded to RGBA8 at upload, 4 bytes per texel: what the library does
 *                                          without this call, the same launches, kernels and bits.
 *   CHORD_TEXSTORE_BLOCKS                  a texture a material slot names whose format is CHORD_TEXFMT_BC1_RGB / BC3 / BC4 / BC5 and
 *                                          whose every level is supplied (chordvis_set_texture_mips gives it no made level: levels ==
 *                                          0 or L <= mipCount) keeps its blocks: its chain is copied as it is into a block store
 *                                          (8-byte units, every chain 16-byte aligned, the levels in ChordTexture's order), takes no
 *                                          texel of the RGBA8 store, and needs no staging buffer and no decode launch.
 *                                          chordvis_resolve_material then decodes the texels of each footprint from their blocks (the
 *                                          pinned decode of DESIGN.md 2 item 9(h)) and produces exactly the images of mode EXPANDED;
 *                                          it takes kernels of its own for that only while the uploaded store holds such a chain.
 *                                          Everything else -- RGBA8 textures, block-compressed textures that get made levels (expanded
 *                                          whole first) -- is stored as in mode EXPANDED, and both kinds may sit in one upload;
 *                                          chordvis_set_texture_compress (below) turns such textures into blocks too.
 * Any other value: CHORDVIS_E_INVALID, the setting unchanged, chordvis_last_error names the allowed values.  Per context; kept across
 * chordvis_upload_scene and chordvis_upload_material_textures; read by chordvis_upload_material_textures alone: a store that is
 * already uploaded stays as it is, and chordvis_upload_scene (the alpha its masked buckets test) never keeps blocks, so frames are
 * the same words in both modes.  On a ChordGroup, set the ranks' contexts before the group's material upload.
 * Caps: the 4 G texel cap of chordvis_upload_material_textures counts expanded texels only; the block store has its own, 2^32
 * units (32 GiB), beyond which the upload returns CHORDVIS_E_CAPACITY and keeps nothing.
 * chordvis_readback_material_texture keeps its contract for a texture kept as blocks: the asked level is expanded into a temporary
 * device buffer by the upload decoder (one launch) and copied out. */
#define CHORD_TEXSTORE_EXPANDED 0u
#define CHORD_TEXSTORE_BLOCKS   1u
int chordvis_set_material_texture_store(ChordCtx* ctx, uint32_t mode);
uint32_t chordvis_material_texture_store(const ChordCtx* ctx);   /* the last accepted value (0 after chordvis_create) */
/* Device memory of the uploaded material textures: texelBytes = 4 x the texels of the RGBA8 store, blockBytes = the sum over the
 * chains kept as blocks of chordvis_texture_chain_bytes rounded up to 16.  Either pointer may be NULL.  CHORDVIS_E_INVALID when no
 * material textures are uploaded. */
int chordvis_material_texture_memory(ChordCtx* ctx, uint64_t* texelBytes, uint64_t* blockBytes);
/* Opt-in: block compression on the GPU at upload, so that a host that has RGBA8 texels only (a decoded PNG, level 0 and
 * chordvis_set_texture_mips for the rest) gets the block store of CHORD_TEXSTORE_BLOCKS too.  Entry i is the target format of
 * texture id i of the descriptors given to LATER chordvis_upload_material_textures calls: 0 (none: the default) or
 * CHORD_TEXFMT_BC1_RGB / BC3 / BC4 / BC5; textures at or beyond `count` have none.  The array is copied and held per context, across
 * both uploads (as the mips setting is).  NULL or count 0: no texture has a target.  Any other value: CHORDVIS_E_INVALID, the
 * setting unchanged, chordvis_last_error names the allowed values.
 * Read by chordvis_upload_material_textures alone, and only under CHORD_TEXSTORE_BLOCKS: in mode EXPANDED and in
 * chordvis_upload_scene it is ignored, and with no target every launch and every stored byte is what it is without this call.
 * Under CHORD_TEXSTORE_BLOCKS, a texture a material slot names that has a target:
 *   RGBA8 source          its supplied levels are copied to a staging buffer on the device, the levels chordvis_set_texture_mips
 *                         asks for are made there, then ONE launch on the context's stream encodes all L levels of every such
 *                         texture into the block store, in the layout of ChordTexture (level l: ceil(w / 4) x ceil(h / 4) blocks,
 *                         levels back to back, the chain 16-byte aligned); the staging buffer is freed after the synchronise.  None
 *                         of its texels stay resident: chordvis_material_texture_memory counts it in blockBytes only, and the 4 G
 *                         texel cap counts only what stays resident (the staging buffer has a 4 G texel cap of its own).  While the call
 *                         runs the staging buffer holds 4 bytes per texel of every texture being encoded, beside the block
 *                         store: that is the call's peak, not what it leaves.
 *   source in the target  format, with made levels (L > mipCount): the supplied levels keep their bytes verbatim -- they are never
 *                         re-encoded --, the made levels are encoded from the texels the mip generation made of the decoded chain.
 *                         (With every level supplied the chain is kept as it is, as without this call.)
 *   source in another     block format: CHORDVIS_E_INVALID, nothing kept.
 * Downstream nothing changes: chordvis_resolve_material samples the chain from its blocks, chordvis_readback_material_texture
 * expands a level through the upload decoder, the block store's 2^32-unit cap applies.
 * The encoder is pinned: the reference importer's (stb_dxt at HIGHQUAL), byte for byte, floats uncontracted.
 * Texel (x, y) of the block at block column bx, row by is the level's texel ((4 bx + x) mod w, (4 by + y) mod h): for sizes that are
 * multiples of 4 and for sizes below 4 the blocks are the reference importer's; for other sizes the reference drops the partial
 * blocks, this library keeps them, with that fill. */
int chordvis_set_texture_compress(ChordCtx* ctx, const uint32_t* perTextureFormat, uint32_t count);
/* What is set for one texture id; 0 at or beyond the count of the last accepted call. */
int chordvis_texture_compress(const ChordCtx* ctx, uint32_t textureId, uint32_t* format);
/* The whole chain of a texture kept as blocks, in the layout of ChordTexture (`bytes` = chordvis_texture_chain_bytes of its format,
 * size and level count), so that a host can cache it and supply it compressed next time; synchronises.  A chain that arrived
 * compressed comes back as the bytes supplied.  CHORDVIS_E_INVALID when no material textures are uploaded, when the texture is not
 * kept as blocks (no material names it, or it is stored as texels), or when `bytes` differs from the chain's size. */
int chordvis_readback_material_blocks(ChordCtx* ctx, uint32_t textureId, uint8_t* host, uint64_t bytes);
/* Opt-in: sampler feedback.  Which levels of which textures does the frame read?  The level rule is this library's (DESIGN.md 2 item
 * 9), so a host with a streaming or budgeted texture pool cannot work it out itself; this pass counts it, and
 * chordvis_set_texture_first_level (below) is the upload option that leaves out the levels nobody read.
 * The buffer is the context's: CHORD_FEEDBACK_LEVELS uint32 words per texture of the last chordvis_upload_material_textures
 * descriptor (levels 0..14 exist; word 15 stays 0).
 *   chordvis_material_feedback_reset   allocates it on first use after a material upload and zeroes it on the context's stream.
 *   chordvis_material_feedback         ONE launch on the context's stream that accumulates into it: calling it twice doubles the
 *                                      counts, and several views or lattice offsets may be summed.  Counts are uint32, modulo 2^32:
 *                                      reset before they can wrap (a call adds at most 4 x width x height / stride^2 in all).
 *   chordvis_readback_material_feedback synchronises and copies textureCount x CHORD_FEEDBACK_LEVELS words.
 * Definition.  A pixel of the lattice (x % stride == offset[0] and y % stride == offset[1]) contributes when it is covered, its id is
 * below the list's count, it has a valid triangle and its material is kLightingType_GLTF_MetallicRoughnessPBR: exactly the pixels
 * chordvis_resolve_material writes material images for.  For each slot s of slotMask in which its material names a texture, let l0 be
 * the finer of the two levels the sampler of chordvis_resolve_material would fetch for that pixel and slot under the context's current
 * chordvis_material_anisotropy (N = 1: from lodq; N > 1: from lodq'; a sampler without a mip filter: 0); the pass adds 1 to
 * taps[texture of the slot][l0].  A texture several materials or slots name gets the sum; one no material names stays 0.  All
 * adds are integers: the result does not depend on their order.  Levels count as the stored texture's do (a texture trimmed by
 * chordvis_set_texture_first_level: from its first stored level).
 * Preconditions, waits and image are those of chordvis_resolve_material asked for a material target (material textures uploaded, a
 * frame rendered, no chordvis_update_objects / chordvis_set_view since, the resolved row-major image after the same wait; a rank of a
 * sharded set-up counts the whole image); neither normals nor tangents are needed.  CHORDVIS_E_INVALID besides, chordvis_last_error
 * naming the allowed values: no chordvis_material_feedback_reset since the last material upload; desc NULL; slotMask 0 or above 15;
 * a stride other than 1, 2, 4 or 8; an offset not below the stride; a textureCount that differs from the uploaded count. */
#define CHORD_FEEDBACK_LEVELS      16u
#define CHORD_FEEDBACK_BASECOLOR    1u   /* slotMask bits, in the order of ChordMaterialTargets */
#define CHORD_FEEDBACK_EMISSIVE     2u
#define CHORD_FEEDBACK_NORMAL       4u
#define CHORD_FEEDBACK_METALROUGH   8u
typedef struct ChordFeedbackDesc {
    uint32_t slotMask;     /* 1..15 */
    uint32_t stride;       /* 1, 2, 4 or 8 */
    uint32_t offset[2];    /* each < stride */
} ChordFeedbackDesc;
int chordvis_material_feedback_reset(ChordCtx* ctx);
int chordvis_material_feedback(ChordCtx* ctx, ChordCountAndCmd drawedMeshletCmd, const ChordFeedbackDesc* desc);
int chordvis_readback_material_feedback(ChordCtx* ctx, uint32_t* hostTaps /* textureCount x CHORD_FEEDBACK_LEVELS */, uint32_t textureCount);
/* Opt-in: trimmed mip chains.  Entry i is the first level texture id i of the descriptors given to LATER
 * chordvis_upload_material_textures calls keeps; textures at or beyond `count` keep level 0.  The array is copied and held per
 * context (as the mips and compress settings are); NULL or count 0 clears it.  chordvis_upload_scene's alpha plane ignores it (the
 * raster's alpha test taps occluded fragments too, which no feedback from visible pixels covers), so frames stay word for word; with
 * no setting every launch and every stored byte is what it is without this call.
 * Rule.  Let L be the texture's level count after chordvis_set_texture_mips and f = min(first, L - 1).  The chain is finished exactly as
 * without the setting (supplied levels as they are, made levels from the last supplied one, COVERAGE measured on level 0); then levels
 * 0 .. f-1 are not stored.  From the upload on the texture IS the one whose level 0 is the chain's level f: max(1, w >> f) x
 * max(1, h >> f) with L - f levels, and every level index the library takes or reports counts from there
 * (chordvis_readback_material_texture, chordvis_readback_material_blocks -- whose `bytes` is the chain size of the smaller texture --,
 * the feedback rows).  RGBA8 and expanded BC textures keep texels of the kept levels only (and decode only those when no level has to
 * be made); a BC chain kept as blocks keeps the bytes from level f's offset; chordvis_set_texture_compress encodes only the kept
 * levels.  chordvis_material_texture_memory and both caps count what stays resident; staging buffers hold the finished chain while
 * the call runs.
 * Property (not a promise for all inputs): the images of chordvis_resolve_material equal the untrimmed ones bit for bit when the
 * texture's width and height are multiples of 2^f, no contributing pixel's l0 is below f, and the sampler's min and mag filters agree on
 * nearest versus bilinear -- scaling both dimensions by 2^-f scales the squared footprint by exactly 4^-f, which shifts lodq by exactly
 * 256 f, and the anisotropic k is not bound by its ceil(lmaj) cap while lodq' >= 256 f.  The exception the third condition covers: a
 * pixel with lodq in (256 f - 128, 256 f] under *_MIPMAP_NEAREST, or exactly 256 f under *_MIPMAP_LINEAR, is minified untrimmed and not
 * minified trimmed, where it takes the mag filter. */
int chordvis_set_texture_first_level(ChordCtx* ctx, const uint32_t* perTextureFirst, uint32_t count);
/* The setting of one texture id; 0 at or beyond the count of the last call. */
int chordvis_texture_first_level(const ChordCtx* ctx, uint32_t textureId, uint32_t* first);
/* What the store holds of a texture a material names: firstLevel = f of the upload (add it to a stored level's index for the level of
 * the finished chain), levelCount = L - f.  CHORDVIS_E_INVALID when no material textures are uploaded or no material names it. */
int chordvis_material_texture_levels(ChordCtx* ctx, uint32_t textureId, uint32_t* firstLevel, uint32_t* levelCount);
/* Opt-in: geometry feedback.  What did the frame SEE?  Which objects own a pixel (the occlusion-query answer), which LOD levels of
 * which primitive the cut selected and which of those reached the image, how many of the submitted clusters ended up visible, and the
 * visible clusters themselves as a command list.  The slot -> command mapping, a pixel's validity rule and a meshlet's LOD live in
 * device buffers, so a host cannot work this out; these calls count it on the device.  Integers throughout: the result does not depend
 * on the order of the adds.  No existing launch, record or image changes; the calls add launches only when made.
 * Inputs.  The row-major (resolved) visibility image chordvis_visibility_mark reads, and `drawed`, the list its ids index.  Let
 * n = min(*drawed.count, the context's command capacity -- the `capacity` of chordvis_last_frame_cmds' handle); drawed.cmds must hold
 * n records.  A pixel of the lattice has x % stride == offset[0] and y % stride == offset[1].  With low = word & 0xFFFFFFFF, a lattice
 * pixel CONTRIBUTES when low != 0, slot = ((low >> 8) & 0xFFFFFF) - 1 < n, cmd = cmds[slot] has objectId < objectCount and meshletId
 * < meshletCount, and tri = low & 0xFF is below the meshlet's triangle count: exactly the pixels chordvis_resolve_attributes writes.  A
 * lattice pixel with low != 0 that does not contribute is REJECTED.  For a command, prim = ChordObject::GLTFPrimitiveDetail of its object
 * as uploaded (the row of the descriptor's primitive array; chordvis_upload_scene refuses an object whose row is not below
 * primitiveCount, so prim is always in range and is no part of the validity rule) and lod = min(ChordMeshlet::lod of its meshlet, CHORD_GEOMETRY_LODS - 1)
 * (the reference's kNaniteMaxLODCount is 12).  A command i < n is SEEN when at least one contributing pixel of THIS call's lattice has
 * slot == i; it is VALID when its objectId and meshletId are in range.  With stride > 1 "seen" means seen on the lattice: a cluster that
 * covers only off-lattice pixels is missed.
 * One chordvis_geometry_feedback call ADDS to the context's buffer (uint32, modulo 2^32: reset before a count can wrap):
 *   objectPixels[o]      +1 per contributing pixel of object o          lodPixels[prim][lod]      +1 per contributing pixel of its command
 *   objectSubmitted[o]   +1 per valid command i < n of object o         lodSubmitted[prim][lod]   +1 per valid command i < n
 *   objectVisible[o]     +1 per seen command of object o                lodVisible[prim][lod]     +1 per seen command
 *   totals[0..3]         lattice pixels looked at, contributing pixels, rejected pixels, seen commands
 * so that sum(objectPixels) == sum(lodPixels) == totals[1], sum(objectVisible) == sum(lodVisible) == totals[3], objectVisible[o] <=
 * objectSubmitted[o], and objectPixels[o] > 0 exactly when objectVisible[o] > 0.
 * The seen bitmap has ceil(capacity / 32) words, bit i & 31 of word i >> 5 for command i.  It belongs to the LATEST call -- every call
 * clears it first: slots are per-frame names, so it is not accumulated.
 *   chordvis_geometry_feedback_reset     allocates the buffer on first use after a scene upload and zeroes it (counts and bitmap) on the
 *                                        context's stream; the next chordvis_upload_scene and chordvis_destroy free it.
 *   chordvis_geometry_feedback           one memset and two launches on the context's stream.  Preconditions, the wait for the image and
 *                                        the treatment of a sharded context are chordvis_resolve_attributes' (a frame rendered; no
 *                                        chordvis_update_objects / chordvis_set_view since; a rank of a sharded set-up counts the whole
 *                                        resolved image).  Material textures are not needed.
 *   chordvis_readback_geometry_feedback  synchronises and copies the arrays whose pointer is not NULL.
 *   chordvis_visible_clusters            writes the seen commands of the latest chordvis_geometry_feedback call into caller-owned DEVICE
 *                                        memory, IN LIST ORDER, records verbatim (`slot` keeps the original slot, so visibility ids still
 *                                        resolve through the full list; `meshletId` stays in the device lists' concatenated numbering
 *                                        -- the output is a device list for the calls that take one -- and is NOT the asset-relative
 *                                        id chordvis_readback_cmds returns: in a scene of several assets the two differ).  *deviceCount receives the number of seen commands even when
 *                                        it exceeds `capacity`; nothing is written at or beyond `capacity` (deviceOut may be NULL when
 *                                        capacity is 0).  The order is part of the contract and does not depend on scheduling.  Two
 *                                        launches.  CHORDVIS_E_INVALID when no feedback call has run since the last reset or scene
 *                                        upload, or when drawed.cmds is not the list the latest feedback call was given.  Only the
 *                                        pointer is compared: the list (records and count word) must be UNCHANGED since that feedback
 *                                        call.  The bitmap names slots of the list as it was then, so after a chordvis_render_frame or
 *                                        a cull that refills the list, call chordvis_geometry_feedback again first; otherwise the
 *                                        bits select whatever commands now sit in those slots.
 *   chordvis_geometry_feedback_seen      synchronises and copies the bitmap (tests and tools).
 * CHORDVIS_E_INVALID besides, chordvis_last_error naming the allowed values: no chordvis_geometry_feedback_reset since the scene
 * upload; desc NULL; a stride other than 1, 2, 4 or 8; an offset not below the stride; pad not 0; read-back counts that differ from the
 * uploaded scene's; a wordCount that is not ceil(capacity / 32). */
#define CHORD_GEOMETRY_LODS 16u
typedef struct ChordGeometryFeedbackDesc {
    uint32_t stride;       /* 1, 2, 4 or 8 */
    uint32_t offset[2];    /* each < stride */
    uint32_t pad;          /* 0 */
} ChordGeometryFeedbackDesc;
typedef struct ChordGeometryFeedback {      /* HOST pointers, NULL = not wanted */
    uint32_t *objectPixels, *objectSubmitted, *objectVisible;   /* objectCount each */
    uint32_t *lodPixels, *lodSubmitted, *lodVisible;            /* primitiveCount x CHORD_GEOMETRY_LODS each */
    uint32_t *totals;                                           /* 4 */
} ChordGeometryFeedback;
int chordvis_geometry_feedback_reset(ChordCtx* ctx);
int chordvis_geometry_feedback(ChordCtx* ctx, ChordCountAndCmd drawedMeshletCmd, const ChordGeometryFeedbackDesc* desc);
int chordvis_readback_geometry_feedback(ChordCtx* ctx, const ChordGeometryFeedback* out, uint32_t objectCount, uint32_t primitiveCount);
int chordvis_visible_clusters(ChordCtx* ctx, ChordCountAndCmd drawedMeshletCmd, ChordDrawCmd* deviceOut, uint32_t* deviceCount, uint32_t capacity);
int chordvis_geometry_feedback_seen(ChordCtx* ctx, uint32_t* hostWords, uint32_t wordCount);
/* Bounds queries -- the frame's frustum and occlusion tests for boxes the HOST owns (light volumes, particle systems, decals, portal
 * volumes: things the library never rasters): `count` ChordBoundsQuery records in device memory in, a ChordBoundsResult per box and a
 * compacted, ordered list of the visible ones out.  Stream-ordered: the call runs on the context's stream behind the work that made the
 * chain, and returns without synchronising.  Every test runs whatever switchFlags chordvis_set_view was given -- a query is a question,
 * not a frame setting.  
 *   1. Frustum.  M = localToTranslatedWorld (phase 1) or localToTranslatedWorldLastFrame (phase 0).  The test is the object stage's
 *      (instance_culling.hlsl:79-89) for an object whose primitive bounds are the box and whose localToTranslatedWorld is M: the
 *      current view's planes, and translatedWorldToClip * M where the orthographic branch projects.  A culled box's record is all zero
 *      and nothing further runs for it.
 *   2. Occlusion.  mvp = translatedWorldToClip * M (phase 1) or translatedWorldToClipLastFrame * M_last (phase 0); the test is the main
 *      view's (hzb_mainview_culling.hlsl:60-161) on (posMin, posMax): eight corners, zInRange, the uv reject, the pixel rectangle, the
 *      level choice, 4 x 4 clamped taps of hzb->minTexels, rejected when the farthest of them is nearer than the box (zMin > mx.z).
 *      UNOCCLUDED is that test's answer; the other bits, rect, nearestZ and the level say which way it went:
 *        NEAR         the box reaches the near plane or lies behind the camera: kept untested; nearestZ 1.0f, rect (0, 0, W-1, H-1)
 *        OFFSCREEN    rejected before any tap; rect 0, nearestZ = mx.z
 *        EMPTY_RECT   rejected before any tap; rect as computed (rz < rx or rw < ry), nearestZ = mx.z
 *        otherwise    rect, nearestZ = mx.z, and the level tapped in bits 8..11
 *      With hzb == NULL everything but the taps runs: UNOCCLUDED is set unless OFFSCREEN or EMPTY_RECT is, and the level bits are 0.
 *   3. Visible list.  A query is visible when IN_FRUSTUM and UNOCCLUDED are both set.  deviceVisible receives the indices of the visible
 *      queries in ASCENDING order, *deviceVisibleCount their number even when it exceeds `capacity`; nothing is written at or beyond
 *      `capacity`.  The order is part of the contract and does not depend on scheduling.
 *   4. View, stream and frame state.  The view is the host copy of the last chordvis_set_view: the call is valid straight after it,
 *      before or after a frame, with or without an uploaded scene.  It flushes a pending HZB tail first like every other reader of the
 *      chain (chordvis_history_hzb's handle is the usual `hzb`), and touches neither the frame's lists and counts, chordvis_stats'
 *      counters nor the history.  Two launches (one when neither the list nor the count is wanted; none for count == 0, which
 *      succeeds and writes *deviceVisibleCount = 0).  The context keeps a scratch of one bit per query and one word per workgroup step.
 *   5. CHORDVIS_E_INVALID, chordvis_last_error naming the rule: no view set; phase other than 0 or 1; count > 0 with deviceQueries NULL;
 *      all three outputs NULL; capacity > 0 with deviceVisible NULL; hzb given with minTexels NULL; hzb->desc not byte-equal to
 *      chordvis_hzb_desc(view width, view height) -- the main-view test has no level clamp, and this rule is what keeps its level
 *      choice inside the chain --; with hzb given, a view whose ChordCameraView::renderDimension differs from its
 *      ChordInstanceCullingView::renderDimension (the rectangle is formed in the former, the chain sized by the latter);
 *      deviceQueries or deviceResults not 16-byte aligned (the records move as 16-byte vectors). */
int chordvis_query_bounds(ChordCtx* ctx, const ChordHZB* hzb /* NULL: frustum only */, int phase /* 0 or 1 */,
                          const ChordBoundsQuery* deviceQueries, uint32_t count,
                          ChordBoundsResult* deviceResults      /* [count] or NULL */,
                          uint32_t* deviceVisible               /* [capacity] query indices, or NULL when capacity == 0 */,
                          uint32_t* deviceVisibleCount          /* one word, or NULL */,
                          uint32_t capacity);
/* Bounds tile lists -- the per-tile answer to the question chordvis_query_bounds answers for the whole screen: which of the visible
 * boxes can touch the pixels of each screen tile (the tile list of tiled deferred lighting, of decal and fog-volume application).
 * `count` ChordBoundsResult records in device memory in -- what chordvis_query_bounds wrote, or records the host made --, per tile the
 * number and the ascending indices of the boxes kept, the tile's depth bounds, and four totals out.  
 *   1. Image.  The row-major (resolved) visibility image chordvis_visibility_mark reads, waited for the same way; a rank of a sharded
 *      context bins the whole resolved image.  A pixel's depth word is the high 32 bits of its word; depth is reverse-Z and an empty
 *      pixel is 0, as chordvis_clear_gbuffer leaves it.  The low word is never looked at.
 *   2. Tiles.  T = desc->tileSize; tilesX = ceil(W / T), tilesY = ceil(H / T) (chordvis_bounds_tile_count); tile t = ty * tilesX + tx
 *      owns the pixels [tx T, min(W, tx T + T)) x [ty T, min(H, ty T + T)).  far(t) is the unsigned minimum of the tile's depth words,
 *      near(t) the unsigned maximum: the image is assumed to hold non-negative, non-NaN depths, as every raster path writes, so the
 *      order of the bits is the order of the floats.  tileDepth[2 t] = far(t), tileDepth[2 t + 1] = near(t).
 *   3. Participation.  Query i < count takes part when its status has both CHORD_BOUNDS_IN_FRUSTUM and CHORD_BOUNDS_UNOCCLUDED.
 *   4. Pair test.  A query that takes part is kept in tile t when all of these hold:
 *        rectangle   rect[0] <= x1 && rect[2] >= x0 && rect[1] <= y1 && rect[3] >= y0, with (x0, y0) the tile's first and (x1, y1) its
 *                    last pixel (a rectangle that reaches past the image overlaps nothing there);
 *        near side   with CHORD_BOUNDS_TILES_NEAR: not nearestZ < asfloat(far(t)) -- rejected is a box whose nearest point lies behind
 *                    every surface of the tile; a CHORD_BOUNDS_NEAR record (nearestZ == 1.0f) is therefore always kept;
 *        far side    with CHORD_BOUNDS_TILES_FAR: not farZ(i) > asfloat(near(t)) -- rejected is a box that ends in front of every
 *                    surface of the tile.  farZ(i) is 0.0f for a record with CHORD_BOUNDS_NEAR set; otherwise it is the smallest
 *                    projected z of the eight corners of deviceQueries[i]'s box -- the mn.z of the main view's occlusion test: fminf,
 *                    from 10.0f, in corner order -- under rule 2 of chordvis_query_bounds' mvp for desc->phase and the host copy of
 *                    the last chordvis_set_view.  A tile of empty pixels (near(t) == 0) under FAR keeps only the CHORD_BOUNDS_NEAR
 *                    records: by design -- there is nothing to shade there.
 *   5. Outputs, each optional (NULL), at least one given.  tileCounts[t] = the number of queries kept, even beyond maxPerTile.
 *      tileItems[t * maxPerTile + k], k < min(tileCounts[t], maxPerTile), = the kept queries' indices in ASCENDING order; no other word
 *      of tileItems is written.  The order is part of the contract and does not depend on scheduling.  totals[0] = the queries that
 *      take part, totals[1] = the sum of tileCounts (modulo 2^32), totals[2] = the tiles with tileCounts > maxPerTile, totals[3] = the
 *      largest tileCounts.
 *   6. Stream, state and launches.  Runs on the context's stream and returns without synchronising.  Needs an allocated G-buffer and a
 *      set view; no scene.  Touches neither the frame's lists and counts, chordvis_stats' counters nor the history.  count == 0
 *      succeeds: zero counts and totals, and tileDepth if asked.  Three launches, four with totals: two put the records that take part
 *      (rectangle, nearestZ, farZ, index) into a scratch of the context's in ascending order, one reduces the tiles' depth bounds and
 *      bins, one folds the totals; with count == 0, or when only tileDepth is asked for, the third alone (and a 16-byte memset when
 *      totals is given).  The scratch grows on demand and is freed with the context.
 *   7. The caller's part.  Results and queries belong together: the same array order, the same phase, the same view.
 *   8. CHORDVIS_E_INVALID, chordvis_last_error naming the rule: desc or out NULL; all four outputs NULL; tileSize not 8, 16, 32 or 64;
 *      unknown flag bits; phase not 0 or 1; FAR without deviceQueries; count > 0 with deviceResults NULL; tileItems with
 *      maxPerTile == 0; tiles * maxPerTile beyond 2^32 - 1; deviceResults or deviceQueries not 16-byte aligned; no G-buffer allocated;
 *      no view set; a view whose ChordCameraView::renderDimension or ChordInstanceCullingView::renderDimension differs from the
 *      image's size. */
uint32_t chordvis_bounds_tile_count(uint32_t width, uint32_t height, uint32_t tileSize,
                                    uint32_t* tilesX, uint32_t* tilesY);   /* tilesX * tilesY; 0 for a tileSize not allowed */
int chordvis_bin_bounds(ChordCtx* ctx, const ChordBoundsTilesDesc* desc,
                        const ChordBoundsResult* deviceResults, const ChordBoundsQuery* deviceQueries /* NULL unless FAR */,
                        uint32_t count, const ChordBoundsTiles* out);
/* The G-buffer in the reference's packed image formats -- what exportGbuffer (lighting.hlsl:62-73) writes into GBufferTextures
 * (render_textures.h:27-49) and every later pass reads: 28 bytes per pixel for the six images, where the float images of
 * chordvis_resolve_material take 88.  The packing is pinned; float32, source order, unfused; R in the low bits:
 *   unorm(x, M)  c = saturate(x) (NaN -> 0); code = (uint32_t)(c * (float)M + 0.5f), truncating (the product is rounded first)
 *   half(x)      binary32 -> binary16, round-to-nearest-even, subnormal results kept, overflow to +-inf, NaN -> +0
 *   baseColor            A2B10G10R10_UNORM_PACK32    unorm(r, 1023) | unorm(g, 1023) << 10 | unorm(b, 1023) << 20 | 3 << 30 of the AP1
 *                                                    rgb of the float image (the reference stores a float3: alpha is pinned to 3)
 *   vertexNormal,        A2B10G10R10_UNORM_PACK32    the same of n * 0.5f + 0.5f per component (one multiply, then one add), alpha 3
 *   pixelNormal
 *   motionVector         R16G16_SFLOAT               half(x) | half(y) << 16
 *   aoRoughnessMetallic  R8G8B8A8_UNORM              unorm(ao, 255) | unorm(roughness, 255) << 8 | unorm(metallic, 255) << 16, A = 0: the
 *                                                    reference's order (the float image roughMetalAO holds roughness, metallic, ao)
 *   emissive             R16G16B16A16_SFLOAT         half(r), half(g), half(b), half(0) in ascending 16-bit lanes: the reference's colour
 *                                                    target as the base pass leaves it
 * Caller-owned DEVICE images of width x height texels, row-major; NULL = not written.  The uint32 images must be 4-byte aligned,
 * emissive 8-byte aligned. */
typedef struct ChordGBufferTargets {
    uint32_t* baseColor;
    uint32_t* vertexNormal;
    uint32_t* pixelNormal;
    uint32_t* motionVector;
    uint32_t* aoRoughnessMetallic;
    uint64_t* emissive;
} ChordGBufferTargets;
/* The fused path: any subset of the six in ONE launch on the context's stream, over the image chordvis_resolve_material would read,
 * after the same wait and under the same preconditions and refusals as chordvis_resolve_material asked for the corresponding float
 * targets (ChordResolveTargets::motionVector, ChordSurfaceTargets::vertexNormal, the four of ChordMaterialTargets): a stale view or
 * objects, no chordvis_upload_material_textures when one of the four material images is asked for, vertexNormal or pixelNormal of a
 * scene without normals, pixelNormal with a normal texture and no tangents.  CHORDVIS_E_INVALID also when every target is NULL or one
 * is misaligned.  The values packed are those chordvis_resolve_material writes, bit for bit: chordvis_set_material_anisotropy and the
 * block store (chordvis_set_material_texture_store) are honoured as there.  No float image is written.
 * A texel is 0 (all bits: the reference's cleared state, render_textures.cpp:74-96) exactly where the corresponding float image holds
 * 0 because nothing was written there: vertexNormal and motionVector at empty pixels and pixels whose id is not below the list's
 * count; the four material images there too and where the material is not kLightingType_GLTF_MetallicRoughnessPBR.  A covered
 * pixel whose normal happens to be the zero vector packs to the code of 0.5 (0xE0080200), not to 0.
 * The launch is a packed twin of the material kernel chordvis_resolve_material would launch, whatever the subset: a call that asks
 * for vertexNormal / motionVector alone launches it too (its material loop is skipped). */
int chordvis_resolve_gbuffer(ChordCtx* ctx, ChordCountAndCmd drawedMeshletCmd, const ChordResolveDesc* desc,
                             const ChordGBufferTargets* targets);
/* Device float images as chordvis_resolve_material writes them, width x height texels, row-major; NULL = absent.  The float4 images
 * must be 16-byte aligned, motionVector 8-byte aligned. */
typedef struct ChordGBufferSources {
    const float* baseColor;      /* float4 */
    const float* vertexNormal;   /* float4 */
    const float* pixelNormal;    /* float4 */
    const float* motionVector;   /* float2 */
    const float* roughMetalAO;   /* float4 */
    const float* emissive;       /* float4 */
} ChordGBufferSources;
/* The stand-alone packer, for hosts that keep float images for some consumers and want the packed ones too: ONE launch on the
 * context's stream converts every texel of each source whose target is non-NULL with the packing above (the channels a layout does
 * not hold -- baseColor's alpha, the fourth float of the others -- are not read into the result).  It needs no scene, frame or
 * image of the context.  Unlike the fused path it is a pure per-texel conversion and knows nothing of coverage: an all-zero normal
 * texel packs to the code of 0.5 (0xE0080200) and an all-zero baseColor texel to 0xC0000000, not to 0, so over a float image of
 * chordvis_resolve_material it equals chordvis_resolve_gbuffer on the texels that were written, not elsewhere.
 * CHORDVIS_E_INVALID: no target, a target without its source, zero width or height, a misaligned pointer. */
int chordvis_pack_gbuffer(ChordCtx* ctx, uint32_t width, uint32_t height, const ChordGBufferSources* sources,
                          const ChordGBufferTargets* targets);
/* The two constant tables of the material resolve as the library holds them (host call, no context): the sRGB8 -> linear decode
 * (256 floats) and sRGB_2_AP1 (9 floats, row-major).  Either may be NULL. */
int chordvis_material_constants(float srgbToLinear[256], float srgbToAp1[9]);
/* The hipStream_t the context enqueues on (the one given to chordvis_create, or its own): a host that allocates targets on a
 * stream of its own orders the two against each other. */
void* chordvis_stream(ChordCtx* ctx);

/* ------------------------------------------------------------------ readback / stats (synchronize) */

int chordvis_readback_visibility(ChordCtx* ctx, uint64_t* hostWords /* width*height, row-major */);
int chordvis_readback_previous_visibility(ChordCtx* ctx, uint64_t* hostWords);   /* pipelined sharded frames: the other buffer pair */
int chordvis_readback_cmds(ChordCtx* ctx, ChordCountAndCmd handle, ChordDrawCmd* hostCmds, uint32_t cap, uint32_t* outCount);
int chordvis_readback_hzb(ChordCtx* ctx, const ChordHZB* hzb, uint16_t* hostMin, uint16_t* hostMax, uint32_t hostValidRange[2]);
/* host: 4 words per marker texel; tiles: 2 words per tile (at most hostCapacity tiles are copied) */
int chordvis_readback_tile_marker(ChordCtx* ctx, const ChordTileMarker* marker, uint32_t* host);
int chordvis_readback_shading_tiles(ChordCtx* ctx, const ChordShadingTiles* tiles, uint32_t* hostTiles, uint32_t hostCapacity,
                                    uint32_t* hostCount, uint32_t hostDispatchArgs[4]);
/* upload an HZB min chain from the host (tests: feed a known history) into history */
int chordvis_upload_history_hzb(ChordCtx* ctx, const uint16_t* hostMin);

/* mode (low 8 bits) 0: off.  1: GPU timestamps of the last frame.  2: accumulate over frames until the
 * next chordvis_stats, which then reports per-frame averages (and restarts the accumulation).
 * mode >> 8 = sampling period P (0/1 = every frame): only every P-th frame is stamped, because each
 * hipEventRecord between two kernels costs ~5 us of stream idle time on MI355X. */
int chordvis_enable_timers(ChordCtx* ctx, int mode);
int chordvis_stats(ChordCtx* ctx, ChordStats* out);
/* Measurement-only switches of the raster kernels (raster_params.h DBG_*).  The clocks (16, 512) and the ablation switches
 * are compiled into the kernels only with -DRASTER_PROFILE=1 / -DRASTER_ABLATION=1 (python chord_amd/build.py --tag NAME -D...;
 * load it with CHORDVIS_LIB): the product library REFUSES them (CHORDVIS_E_INVALID), because testing them at run time costs the
 * register-bound kernels 3-5 %.  1 no pixel writes, 2 setup
 * emits no records / bins, 16 per-tile clocks (chordvis_debug_tile_profile), 32 skip the per-lane scan of tiny
 * triangles, 64 tile kernel of later passes returns at once, 128 no tile-out, 256 tile-out without the HZB
 * reduction, 512 setup-kernel phase clocks (chordvis_debug_setup_profile), 1024 fused tile-out skips the visibility
 * stores, 2048 never split long bins, 4096 / 8192 / 16384 tile kernel skips its row units / entry set-up / the bin
 * altogether.  0 = production; any of those voids parity.  These switches do NOT change results (tests run them): 32768 small
 * clusters never leave the setup kernel as pixel blocks, 65536 every launch takes the setup kernel's pixel-block body
 * (by default it does when a launch has more than one cluster per 16 pixels), 131072 chordvis_render_frame launches
 * hzb_tail_kernel between the raster passes instead of letting the phase-1 cull reduce HZB levels 6.. itself, 262144 the
 * pixel-block kernel always runs its hot-tile variant and treats a bin of 64 entries as hot (by default the variant is chosen
 * when the previous frame had a bin of 65536 entries or more), 524288 the library's own sharded frames (chordvis_comm_*, ChordGroup)
 * keep the replicated group cull instead of the sharded one (A / B measurements; every rank of a frame must agree), 4194304
 * chordvis_material_feedback's workgroups use 2 entries of their on-chip count tables instead of 512, so that most adds find
 * the table full and go to global memory (the same counts, slower), 8388608 chordvis_geometry_feedback's workgroups likewise use
 * 2 entries of their count tables instead of 1024, 16777216 chordvis_query_bounds launches grids of at most two workgroups, so that
 * short lists walk the grid-stride loops of its kernels, 33554432 chordvis_bin_bounds likewise launches grids of at most two
 * workgroups and streams its records in chunks of 64 instead of 256, so that small counts walk every loop and chunk boundary of its
 * kernels (the same results). */
int chordvis_set_debug(ChordCtx* ctx, uint32_t flags);
/* measurement / test aid: fills EVERY rank's chunk of the cull exchange buffer on this context for the current view (what the
 * all-gather would deliver), so that one rank of a sharded frame can be timed alone on one device (tools/shard_time.py) */
int chordvis_debug_fill_cull_exchange(ChordCtx* ctx);
/* debugging aid: raw read of an internal buffer (0 tile counts, 1 fixed bins, 2 chunk table, 3 bin pool, 4 / 5 32- / 48-byte records,
 * 7 the alpha plane the masked buckets sample: one byte per texel, every level of every texture a masked material samples, in
 * texture order; CHORDVIS_E_INVALID when the scene has none; 8 the flattened (object, group) table, 24 bytes per group instance of
 * the current object list: owner, group | meshlet count << 28, four global meshlet ids; 9 the per-object static table, 48 bytes per
 * object: primitive, material flags | material << 8, first group instance, shading type, the primitive's bounds -- for 8 and 9 a
 * range beyond the current list's table is CHORDVIS_E_INVALID) */
int chordvis_debug_read(ChordCtx* ctx, int which, uint64_t offset, uint64_t bytes, void* host);
/* debugging aid: non-zero words in the split-tile accumulation slabs (must be 0 between raster passes) */
int chordvis_debug_slab_nonzero(ChordCtx* ctx, uint64_t* count);
/* measurement aid: ms per frame of 2*pairs stream-launched frames vs the same frames replayed from a hipGraph */
int chordvis_debug_graph_frames(ChordCtx* ctx, uint32_t pairs, float* msPerFrameStream, float* msPerFrameGraph);
/* debug bit 512: per-wave phase ticks (10 ns) of the setup kernel summed over waves: header wait / vertex / triangle / reserve / emit.
 * The clocks of bits 16 and 512 are compiled in only with -DRASTER_PROFILE=1 (python chord_amd/build.py --tag prof -DRASTER_PROFILE=1:
 * their accumulators cost the product kernels scalar registers they do not have); the product library leaves the ticks zero. */
int chordvis_debug_setup_profile(ChordCtx* ctx, int pass, uint64_t hostTicks[5], uint32_t* waves);
int chordvis_debug_tile_profile(ChordCtx* ctx, int pass, uint64_t* hostTicks, uint32_t* hostCounts, uint32_t capacity);
/* Which set-up kernel the latest launch of each raster pass took: wide[pass] = 1 for raster_setup_wide_kernel (a light later pass),
 * 0 for raster_setup_kernel. */
int chordvis_debug_setup_kernels(ChordCtx* ctx, uint32_t wide[2]);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CHORDVIS_H */
