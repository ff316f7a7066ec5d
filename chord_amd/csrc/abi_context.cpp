// C ABI, the context: create / destroy / sync, the error text, the view and the render targets, limits and modes, timers and
// chordvis_stats.  The host layer is cut per feature (abi_*.cpp); what the pieces share is declared in host_layer.h.

#include "host_layer.h"

using namespace chord;

namespace chord {

int fail(ChordCtx* ctx, int code, const char* what, hipError_t e)
{
    if (ctx) {
        char buf[512];
        if (e != hipSuccess) std::snprintf(buf, sizeof(buf), "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
        else std::snprintf(buf, sizeof(buf), "%s", what);
        ctx->lastError = buf;
    }
    return code;
}

static int alloc_hzb(ChordCtx* c, HzbBuffers& h)
{
    ChordHZBDesc d;
    if (chordvis_hzb_desc(c->width, c->height, &d) != CHORDVIS_OK) return fail(c, CHORDVIS_E_INVALID, "render size unsupported for HZB");
    h.desc = d;
    h.valid = false; h.uploaded = false;
    int rc;
    if ((rc = dalloc(c, &h.minTexels, d.totalTexels))) return rc;
    if ((rc = dalloc(c, &h.maxTexels, d.totalTexels))) return rc;
    if ((rc = dalloc(c, &h.validRange, 2))) return rc;
    CHORD_HIP(c, hipMemsetAsync(h.minTexels, 0, sizeof(uint16_t) * d.totalTexels, c->stream));
    CHORD_HIP(c, hipMemsetAsync(h.maxTexels, 0, sizeof(uint16_t) * d.totalTexels, c->stream));
    return CHORDVIS_OK;
}

int configure_targets(ChordCtx* c, uint64_t* external)
{
    c->resolveFrame = false;
    // visibility words (sharded: rank-major tile slots, ranks * slotsPerRank * 64 * 64 words)
    const uint32_t N = c->shard.ranks;
    c->tilesX = (c->width + CHORD_TILE - 1) >> CHORD_TILE_SHIFT; c->tilesY = (c->height + CHORD_TILE - 1) >> CHORD_TILE_SHIFT;
    c->shard.tilesX = c->tilesX;
    // (allocated for the slot capacity; an all-gather moves ranks x shard.slotsPerRank slots, what the current map uses)
    c->slotCapacity = N > 1 ? chordvis_tile_slot_capacity(c->width, c->height, N) : 0u;
    c->visWords = N > 1 ? (uint64_t)N * c->slotCapacity * (CHORD_TILE * CHORD_TILE) : (uint64_t)c->width * c->height;
    int rc;
    if (external) {
        dfree(c->dVisOwned);
        c->dVis = external; c->visExternal = true;
    } else {
        if ((rc = dalloc(c, &c->dVisOwned, c->visWords))) return rc;
        c->dVis = c->dVisOwned; c->visExternal = false;
    }
    if (N > 1) { if ((rc = dalloc(c, &c->dVisResolved, (uint64_t)c->width * c->height))) return rc; }
    else dfree(c->dVisResolved);
    for (int i = 0; i < 3; i++) if ((rc = alloc_hzb(c, c->hzb[i]))) return rc;
    c->historySlot = 0;
    c->pendingTailSlot = 0;
    {   // per-tile triangle bins of the rasterizer: 64x64-pixel tiles, binCap entries each
        c->binCap = CHORD_BIN_CAP;              // 4K: 2 passes x 2040 tiles x 16384 x 4 B = 267 MB
        if ((rc = dalloc(c, &c->dTileBins, (size_t)2 * c->tilesX * c->tilesY * c->binCap))) return rc;
        c->binPoolChunks = c->limitPoolChunks;  // default: 2 passes x 32 Ki chunks x 1024 entries x 4 B = 256 MB
        if ((rc = dalloc(c, &c->dBinPool, (size_t)2 * c->binPoolChunks * CHORD_BIN_CHUNK))) return rc;
        const size_t tabWords = (size_t)2 * c->tilesX * c->tilesY * c->binMaxChunks;
        if ((rc = dalloc(c, &c->dBinChunkTab, tabWords))) return rc;
        CHORD_HIP(c, hipMemset(c->dBinChunkTab, 0, tabWords * sizeof(unsigned long long)));
        // work items of the tile kernel: every tile once, plus the slices of split tiles (bounded by the entries
        // a pass can hold)
        const size_t tilesN = (size_t)c->tilesX * c->tilesY;
        c->tileItemCap = (uint32_t)(tilesN * (CHORD_TILE_MAX_SLICES + 1u));
        if ((rc = dalloc(c, &c->dTileOrder, ((size_t)1 + c->tileItemCap) * 2))) return rc;   // uint2 per item
        if ((rc = dalloc(c, &c->dTileOrderKeep, ((size_t)1 + c->tileItemCap) * 4))) return rc;    // (two schedules each: this frame's and the one being made for the next)
        if ((rc = dalloc(c, &c->dTileOrderKeep1, ((size_t)1 + c->tileItemCap) * 4))) return rc;
        c->orderAge = c->orderAge1 = 0xFFFFFFFFu;
        if ((rc = dalloc(c, &c->dTileSlabs, tilesN * CHORD_TILE * CHORD_TILE))) return rc;
        CHORD_HIP(c, hipMemset(c->dTileSlabs, 0, tilesN * CHORD_TILE * CHORD_TILE * sizeof(unsigned long long)));
    }
    if ((rc = dalloc(c, &c->dTileRange, (size_t)2 * CHORD_MAX_TILES))) return rc;
    if (!c->hBinHint) {     // what the tile order kernel tells the host about a pass (the longest bin): 64 bytes of mapped host memory
        void* h = nullptr; void* dh = nullptr;
        CHORD_HIP(c, hipHostMalloc(&h, 64, hipHostMallocMapped));
        std::memset(h, 0, 64);
        CHORD_HIP(c, hipHostGetDevicePointer(&dh, h, 0));
        c->hBinHint = static_cast<volatile uint32_t*>(h); c->dBinHint = static_cast<uint32_t*>(dh);
    }
    if (c->dHotTiles) CHORD_HIP(c, hipMemsetAsync(c->dHotTiles, 0, sizeof(uint32_t) * 2 * (1 + CHORD_HOT_TILES), c->stream));   // (tile ids of another target size)
    c->hBinHint[0] = 0u; c->hBinHint[1] = 0u;
    c->hBinHint[2] = 0xFFFFFFFFu; c->hBinHint[3] = 0xFFFFFFFFu;      // clusters per pass of the last finished frame: none yet
    for (int k = 4; k < 8; k++) c->hBinHint[k] = 0u;                  // serials of the last pass found heavy [4 + pass] / light [6 + pass] (launch_raster: TILE_DIRECT): none
    {   // one {min, max} partial per block of the mip-0 kernel (64 x 4 texels per block)
        const uint32_t vw = (c->width + 1) / 2, vh = (c->height + 1) / 2;
        if ((rc = dalloc(c, &c->dRangePartials, (size_t)((vw + 63) / 64) * ((vh + 3) / 4) * 2))) return rc;
    }
    // sharded: the tile map and the two HZB exchange buffers (one slot per tile slot of the visibility buffer)
    if (N > 1) {
        const size_t tilesN = (size_t)c->tilesX * c->tilesY;
        CHORD_HIP(c, hipMemsetAsync(c->dVis, 0, c->visWords * 8, c->stream));   // (slots of edge tiles are partly padding: defined bytes on the wire)
        if ((rc = dalloc(c, &c->dShardTables, 64 + (tilesN + 1) / 2))) return rc;
        if ((rc = dalloc(c, &c->dTileLoads, tilesN))) return rc;
        CHORD_HIP(c, hipMemsetAsync(c->dTileLoads, 0, tilesN * 4, c->stream));
        if (c->tileOwners.size() != tilesN || !c->tileOwnersExplicit) {
            c->tileOwners.assign(tilesN, 0);
            c->tileOwnersExplicit = false;
            if (tile_layout(c->tilesX, c->tilesY, N, nullptr, 0u, c->tileOwners.data()) != CHORDVIS_OK) return fail(c, CHORDVIS_E_INVALID, "tile layout");
        }
        const size_t slots = (size_t)N * c->slotCapacity;
        if ((rc = dalloc(c, &c->dHzbExchange, slots * CHORD_HZB_SLOT_HALVES))) return rc;
        CHORD_HIP(c, hipMemsetAsync(c->dHzbExchange, 0, slots * CHORD_HZB_SLOT_HALVES * 2, c->stream));
        if ((rc = dalloc(c, &c->dHzbFinalExchange, slots * CHORD_HZB_FINAL_SLOT_HALVES))) return rc;
        CHORD_HIP(c, hipMemsetAsync(c->dHzbFinalExchange, 0, slots * CHORD_HZB_FINAL_SLOT_HALVES * 2, c->stream));
        if ((rc = install_tile_owners(c))) return rc;
        if ((rc = prepare_cull_exchange(c))) return rc;
    } else {
        dfree(c->dHzbExchange); dfree(c->dHzbFinalExchange); dfree(c->dShardTables); dfree(c->dTileLoads); dfree(c->dTileOwner); dfree(c->dCullExchange);
        c->shard.ownedRows = nullptr; c->shard.tileSlot = nullptr;
        c->hzbExchangeHalves = c->hzbExchangeChunkHalves = 0; c->hzbFinalExchangeChunkBytes = 0;
    }
    // (a second pair of visibility buffers is made by chordvis_swap_visibility when a pipelined host first asks for it)
    dfree(c->dVisAlt); dfree(c->dVisResolvedAlt);
    return CHORDVIS_OK;
}

int ready(ChordCtx* c, const char* fn)
{
    if (!c) return CHORDVIS_E_INVALID;
    if (!c->sceneLoaded || !c->viewSet || !c->dVis) {
        char buf[160];
        std::snprintf(buf, sizeof(buf), "%s: upload_scene, allocate_gbuffer and set_view must come first", fn);
        return fail(c, CHORDVIS_E_INVALID, buf);
    }
    if (!chord::view_fits_target(c)) {
        // (chordvis_set_view holds a view to the target it meets; chordvis_allocate_gbuffer may have come after it)
        char buf[224];
        std::snprintf(buf, sizeof(buf), "%s: the view's renderDimension differs from the allocated gbuffer (chordvis_set_view must follow a chordvis_allocate_gbuffer of another size)", fn);
        return fail(c, CHORDVIS_E_INVALID, buf);
    }
    return CHORDVIS_OK;
}

// passes other than instance_culling that run before it in a frame still need the constants on the device
int flush_view(ChordCtx* c)
{
    if (c->viewDirty) {
        CHORD_HIP(c, hipMemcpyAsync(c->dView, &c->hView, sizeof(DView), hipMemcpyHostToDevice, c->stream));
        c->viewDirty = false;
    }
    if (c->zeroFrameStateInCull) {
        CHORD_HIP(c, hipMemsetAsync(c->dFrameState, 0, c->frameStateZeroBytes, c->stream));
        c->zeroFrameStateInCull = false;
    }
    return CHORDVIS_OK;
}

// The tail of the last fused frame's history HZB (mips 6.. + valid range) normally rides on the next frame's first
// kernel; anything else that is about to read that chain launches it now.
int flush_pending_tail(ChordCtx* c)
{
    if (c->pendingTailSlot) {
        launch_hzb_tail(c, c->hzb[c->pendingTailSlot], true, true);
        c->pendingTailSlot = 0;
        CHORD_HIP(c, hipGetLastError());
    }
    return CHORDVIS_OK;
}

void free_retired(ChordCtx* c)      // (the caller has let the stream run empty)
{
    for (void* p : c->retired) (void)hipFree(p);
    c->retired.clear();
    for (ChordCtx* k : c->retiredChildren) chordvis_destroy(k);
    c->retiredChildren.clear();
}

void stamp(ChordCtx* c, int tag)
{
    if (!c->timers || !c->stampThisFrame) return;
    const size_t i = c->stampTags.size();
    if (i >= c->evPool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        c->evPool.push_back(e);
    }
    (void)hipEventRecord(c->evPool[i], c->stream);
    c->stampTags.push_back(tag);
}

} // namespace chord

extern "C" {

int chordvis_create(int deviceOrdinal, void* hipStream, ChordCtx** outCtx)
{
    if (!outCtx) return CHORDVIS_E_INVALID;
    *outCtx = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || deviceOrdinal < 0 || deviceOrdinal >= n) return CHORDVIS_E_NO_DEVICE;
    ChordCtx* c = new ChordCtx();
    c->device = deviceOrdinal;
    if (hipSetDevice(deviceOrdinal) != hipSuccess) { delete c; return CHORDVIS_E_NO_DEVICE; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, deviceOrdinal) == hipSuccess) c->numCUs = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (hipStream) { c->stream = (hipStream_t)hipStream; c->ownStream = false; }
    else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return CHORDVIS_E_HIP; }
        c->ownStream = true;
    }
    bool ok = hipMalloc((void**)&c->dTileClocks, sizeof(unsigned long long) * 18 * CHORD_MAX_TILES) == hipSuccess &&
              hipMalloc((void**)&c->dHotTiles, sizeof(uint32_t) * 2 * (1 + CHORD_HOT_TILES)) == hipSuccess &&
              hipMemset(c->dHotTiles, 0, sizeof(uint32_t) * 2 * (1 + CHORD_HOT_TILES)) == hipSuccess &&
              hipMalloc((void**)&c->dView, sizeof(DView)) == hipSuccess &&
              hipMalloc((void**)&c->dFrameState, sizeof(FrameState)) == hipSuccess;
    if (!ok) { chordvis_destroy(c); return CHORDVIS_E_HIP; }
    c->dCounters = &c->dFrameState->counters;
    c->dCounts = c->dFrameState->listCounts;
    (void)hipMemsetAsync(c->dFrameState, 0, sizeof(FrameState), c->stream);
    *outCtx = c;
    return CHORDVIS_OK;
}

int chordvis_destroy(ChordCtx* c)
{
    if (!c) return CHORDVIS_E_INVALID;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    (void)chordvis_comm_destroy(c);
    free_retired(c);
    if (c->depthCtx) { chordvis_destroy(c->depthCtx); c->depthCtx = nullptr; }
    for (float*& d : c->dDepthImages) dfree(d);
    if (c->sharedScene) {       // a depth-view child: the scene buffers are the parent's
        c->dPrims = nullptr; c->dGroups = nullptr; c->dMeshlets = nullptr; c->dGroupIndices = nullptr; c->dMeshletData = nullptr;
        c->dPositions = nullptr; c->dObjStatic = nullptr; c->dGroupRefs = nullptr; c->dMaterials = nullptr; c->dTexAlpha = nullptr;
        c->dTexcoords = nullptr; c->dBvhNodes = nullptr; c->dMeshletLod = nullptr; c->dNormals = nullptr; c->dTangents = nullptr;
        c->dMatRecords = nullptr; c->dMatTexels = nullptr; c->dMatBlocks = nullptr;
    }
    dfree(c->dPrims); dfree(c->dGroups); dfree(c->dMeshlets); dfree(c->dGroupIndices); dfree(c->dMeshletData);
    dfree(c->dPositions); dfree(c->dObjStatic); dfree(c->dMaterials); dfree(c->dTexAlpha); dfree(c->dTexcoords); dfree(c->dBvhNodes); dfree(c->dGroupRefs); dfree(c->dObjectsOwned); dfree(c->dMeshletLod); dfree(c->dPrimVertexBase); dfree(c->dPrimAssetMeshlets);
    dfree(c->dNormals); dfree(c->dTangents); dfree(c->dMatRecords); dfree(c->dMatTexels); dfree(c->dMatBlocks); dfree(c->dMatFeedback); dfree(c->dGeoFeedback); dfree(c->dBoundsScratch); dfree(c->dBoundsTilesScratch); dfree(c->dTexEncTables);
    dfree(c->dView); dfree(c->dObjFrame); dfree(c->dGroupMask); dfree(c->dBlockCounts);
    drop_world_transforms(c);
    drop_ray_scene(c);
    for (int i = 0; i < 3; i++) dfree(c->lists[i].cmds);
    dfree(c->dRankCmds); dfree(c->dLeftCmds); dfree(c->dMineCmds);
    dfree(c->dCullLookback);
    dfree(c->dFrameState); c->dCounts = nullptr; c->dCounters = nullptr; dfree(c->dTileClocks); dfree(c->dHotTiles); dfree(c->dTileOrder); dfree(c->dTileOrderKeep); dfree(c->dTileOrderKeep1); c->orderAge = c->orderAge1 = 0xFFFFFFFFu; dfree(c->dTileSlabs); dfree(c->dTileMarker); dfree(c->dShadingTiles);
    dfree(c->dVisOwned); dfree(c->dVisResolved);
    for (int i = 0; i < 3; i++) { dfree(c->hzb[i].minTexels); dfree(c->hzb[i].maxTexels); dfree(c->hzb[i].validRange); }
    if (c->hBinHint) { (void)hipHostFree(const_cast<uint32_t*>(c->hBinHint)); c->hBinHint = nullptr; c->dBinHint = nullptr; }
    dfree(c->dRangePartials); dfree(c->dTileRange); dfree(c->dHzbExchange); dfree(c->dHzbFinalExchange); dfree(c->dShardTables); dfree(c->dTileLoads); dfree(c->dTileOwner); dfree(c->dCullExchange); dfree(c->dVisAlt); dfree(c->dVisResolvedAlt); dfree(c->dTris); dfree(c->dTrisC); dfree(c->dBlockPool); dfree(c->dTileBins); dfree(c->dBinPool); dfree(c->dBinChunkTab);
    dfree(c->dClipTris); dfree(c->dLargeList);
    for (hipEvent_t e : c->evPool) (void)hipEventDestroy(e);
    if (c->ownStream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return CHORDVIS_OK;
}

const char* chordvis_last_error(ChordCtx* c) { return c ? c->lastError.c_str() : "null context"; }

int chordvis_sync(ChordCtx* c)
{
    if (!c) return CHORDVIS_E_INVALID;
    { const int rc = flush_pending_tail(c); if (rc) return rc; }
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    free_retired(c);                                      // (what chordvis_set_object_list dropped without waiting)
    return CHORDVIS_OK;
}

int chordvis_set_view(ChordCtx* c, const ChordCameraView* view, const ChordInstanceCullingView* iv, uint32_t switchFlags)
{
    if (!c || !view || !iv) return fail(c, CHORDVIS_E_INVALID, "set_view: null argument");
    // (the rank masks on their way through the all-gather were computed with the current view, cull mode and tile map)
    if (c->cullPhaseDone) return fail(c, CHORDVIS_E_INVALID, "set_view: not between chordvis_frame_phase_cull and chordvis_frame_phase_a");
    // (refused before anything is taken over: the view set before stays the context's)
    if (c->dVis && ((uint32_t)iv->renderDimension[0] != c->width || (uint32_t)iv->renderDimension[1] != c->height))
        return fail(c, CHORDVIS_E_INVALID, "set_view: renderDimension differs from the allocated gbuffer");
    c->hView.view = *view; c->hView.iv = *iv; c->hView.flags = switchFlags;
    c->hView.width = (uint32_t)iv->renderDimension[0]; c->hView.height = (uint32_t)iv->renderDimension[1];
    // the 600-byte constant block travels as a kernel argument of the frame's first kernel (object_cull),
    // which publishes it for the later passes; see flush_view() for passes called out of frame order
    c->viewDirty = true;
    c->viewSet = true;
    c->resolveStale = true;
    return CHORDVIS_OK;
}

int chordvis_allocate_gbuffer(ChordCtx* c, uint32_t width, uint32_t height, uint64_t* deviceVisibility)
{
    if (!c || width < 64 || height < 64 || width > 4096 || height > 4096)      // renderer.h:52-53
        return fail(c, CHORDVIS_E_INVALID, "allocate_gbuffer: render size must be 64..4096 per axis (renderer.h:52-53)");
    CHORD_HIP(c, hipSetDevice(c->device));
    c->width = width; c->height = height;
    dfree(c->dTileMarker); dfree(c->dShadingTiles);                             // sized by the render size; re-made on demand
    // (a view of another size stays set but no longer fits: ready() refuses the passes until chordvis_set_view has come again)
    return configure_targets(c, deviceVisibility);
}

int chordvis_set_limits(ChordCtx* c, const ChordLimits* limits)
{
    if (c) c->orderAge = c->orderAge1 = 0xFFFFFFFFu;                    // (the kept tile schedule of launch_raster is made again)

    if (!c || !limits) return fail(c, CHORDVIS_E_INVALID, "set_limits: null argument");
    if (c->sceneLoaded || c->dVis) return fail(c, CHORDVIS_E_INVALID, "set_limits: call before upload_scene / allocate_gbuffer");
    if (limits->maxTriangleRecords) {
        if (limits->maxTriangleRecords < (1u << 16) || limits->maxTriangleRecords > 0x7FFFFFC0ull)
            return fail(c, CHORDVIS_E_INVALID, "set_limits: maxTriangleRecords out of range (record indices are 32-bit)");
        c->limitRecords = limits->maxTriangleRecords & ~(uint64_t)(CHORD_LIST_SHARDS - 1);
    }
    if (limits->binPoolChunks) {
        if (limits->binPoolChunks > (16u << 20)) return fail(c, CHORDVIS_E_INVALID, "set_limits: at most 16 Mi pool chunks per pass (64 GB)");
        c->limitPoolChunks = limits->binPoolChunks;
    }
    if (limits->binMaxChunksPerTile) {
        if (limits->binMaxChunksPerTile > CHORD_BIN_MAX_CHUNKS_LIMIT) return fail(c, CHORDVIS_E_INVALID, "set_limits: at most 3072 overflow chunks per tile");
        c->binMaxChunks = limits->binMaxChunksPerTile;
    }
    return CHORDVIS_OK;
}

int chordvis_set_tile_schedule_keep(ChordCtx* c, uint32_t frames)
{
    if (!c) return CHORDVIS_E_INVALID;
    c->orderKeepFrames = frames;
    c->orderAge = c->orderAge1 = 0xFFFFFFFFu;
    return CHORDVIS_OK;
}
uint32_t chordvis_tile_schedule_keep(ChordCtx* c) { return c ? c->orderKeepFrames : 0u; }

int chordvis_set_cull_mode(ChordCtx* c, int hierarchical)
{
    if (!c || hierarchical < 0 || hierarchical > 1) return fail(c, CHORDVIS_E_INVALID, "set_cull_mode: 0 (flat) or 1 (hierarchical)");
    if (hierarchical && c->sceneLoaded && !c->bvhComplete) return fail(c, CHORDVIS_E_INVALID, "set_cull_mode: the uploaded scene has primitives without a BVH");
    if (c->cullPhaseDone) return fail(c, CHORDVIS_E_INVALID, "set_cull_mode: not between chordvis_frame_phase_cull and chordvis_frame_phase_a");
    c->cullMode = hierarchical;
    return CHORDVIS_OK;
}

void* chordvis_stream(ChordCtx* c) { return c ? (void*)c->stream : nullptr; }

int chordvis_enable_timers(ChordCtx* c, int enable)
{
    if (!c) return CHORDVIS_E_INVALID;
    c->timers = enable < 0 ? 0 : ((enable & 0xFF) > 2 ? 2 : (enable & 0xFF));
    c->timerPeriod = (enable >> 8) > 0 ? (uint32_t)(enable >> 8) : 1u;
    c->stampTags.clear();
    c->framesStamped = 0;
    c->frameIndex = 0;
    c->stampThisFrame = false;
    return CHORDVIS_OK;
}

int chordvis_stats(ChordCtx* c, ChordStats* out)
{
    if (!c || !out) return fail(c, CHORDVIS_E_INVALID, "stats: null argument");
    std::memset(out, 0, sizeof(*out));
    { const int rc = flush_pending_tail(c); if (rc) return rc; }
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    uint32_t counts[4] = {0, 0, 0, 0};
    CHORD_HIP(c, hipMemcpy(counts, c->dCounts, sizeof(counts), hipMemcpyDeviceToHost));
    DeviceCounters dc;
    CHORD_HIP(c, hipMemcpy(&dc, c->dCounters, sizeof(dc), hipMemcpyDeviceToHost));
    out->countInstanceCulled = counts[0];
    if (c->shouldStage1) {
        out->countStage0Visible = counts[1]; out->countStage0Rejected = counts[2]; out->countStage1Visible = counts[3];
        out->trianglesSubmitted = dc.trisHzbVisible0 + dc.trisHzbVisible1;
    } else {
        out->countStage0Visible = counts[0];
        out->trianglesSubmitted = dc.trisInstanceCulled;
    }
    out->overflow = dc.overflow;
    out->rasterLaunches = c->rasterCalls;
    out->kernelLaunches = c->lastFrameLaunches;
    for (int pass = 0; pass < 2; pass++) {
        out->clipTriangles[pass] = dc.clipTriCount[pass];
        for (uint32_t i = 0; i < CHORD_LIST_SHARDS; i++) out->largeRecords[pass] += dc.largeCount[pass][i * CHORD_SHARD_STRIDE];
    }
    for (uint32_t i = 0; i < CHORD_LIST_SHARDS; i++) {
        out->triangleRecords += dc.triCount[i * CHORD_SHARD_STRIDE] + dc.triCountC[i * CHORD_SHARD_STRIDE];
        out->triangleRecordsCompact += dc.triCountC[i * CHORD_SHARD_STRIDE];
        out->pixelBlockBytes += (uint64_t)dc.blockGranules[i * CHORD_SHARD_STRIDE] * 16u;
    }
    if (c->tilesX) {
        std::vector<uint32_t> tc((size_t)c->tilesX * c->tilesY);
        for (int pass = 0; pass < 2; pass++) {
            CHORD_HIP(c, hipMemcpy2D(tc.data(), 4, c->dFrameState->tileCount + (size_t)pass * c->tilesX * c->tilesY * CHORD_TILECOUNT_STRIDE, 4 * CHORD_TILECOUNT_STRIDE, 4, tc.size(), hipMemcpyDeviceToHost));
            for (uint32_t v : tc) { out->binEntries += v; out->tilesTouched[pass] += v ? 1u : 0u; }
            CHORD_HIP(c, hipMemcpy2D(tc.data(), 4, c->dFrameState->tileCount + (size_t)pass * c->tilesX * c->tilesY * CHORD_TILECOUNT_STRIDE + 1, 4 * CHORD_TILECOUNT_STRIDE, 4, tc.size(), hipMemcpyDeviceToHost));
            for (uint32_t v : tc) out->pixelBlocks += v;
        }
    }
    if (c->timers && c->framesStamped && c->stampTags.size() > 1) {
        // walk the stamps: the segment ending at stamp i is attributed by its tag and the current stage
        float clear = 0, cull = 0, st0 = 0, hzb0 = 0, st1 = 0, hzbf = 0, rc_ = 0, rk = 0, rh = 0, other = 0, exh = 0, exv = 0, exc = 0, exf = 0;
        int stage = 0;   // 0 = stage 0, 1 = stage 1
        for (size_t i = 1; i < c->stampTags.size(); i++) {
            const int tag = c->stampTags[i];
            if (tag == S_FRAME_BEGIN) { stage = 0; continue; }           // gap between frames is not frame time
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, c->evPool[i - 1], c->evPool[i]) != hipSuccess) continue;
            switch (tag) {
            case S_CLEAR: clear += ms; break;
            case S_CULL: cull += ms; break;
            case S_HZBCULL: case S_STAGE0_END: case S_STAGE1_END: (stage == 0 ? st0 : st1) += ms; break;
            case S_R_CLUSTER: rc_ += ms; (stage == 0 ? st0 : st1) += ms; break;
            case S_R_CLIP: rk += ms; (stage == 0 ? st0 : st1) += ms; break;
            case S_R_CHUNK: rh += ms; (stage == 0 ? st0 : st1) += ms; break;
            case S_HZB0: hzb0 += ms; break;
            case S_HZBF: hzbf += ms; break;
            case S_EXCH_HZB: exh += ms; break;
            case S_EXCH_VIS: exv += ms; break;
            case S_EXCH_CULL: exc += ms; break;
            case S_EXCH_FINAL: exf += ms; break;
            default: other += ms; break;
            }
            if (tag == S_STAGE0_END) stage = 1;
        }
        const float inv = 1.0f / (float)c->framesStamped;
        out->msClear = clear * inv; out->msInstanceCulling = cull * inv; out->msStage0 = st0 * inv;
        out->msHzbStage0 = hzb0 * inv; out->msStage1 = st1 * inv; out->msHzbFinal = hzbf * inv;
        out->msRasterCluster = rc_ * inv; out->msRasterClip = rk * inv; out->msRasterChunk = rh * inv;
        out->msExchangeHzb = exh * inv; out->msExchangeVis = exv * inv; out->msExchangeCull = exc * inv; out->msExchangeFinal = exf * inv;
        out->msFrame = (clear + cull + st0 + hzb0 + st1 + hzbf + other + exh + exv + exc + exf) * inv;
        out->framesTimed = c->framesStamped;
        out->stampsPerFrame = (float)c->stampTags.size() * inv;
    }
    if (c->timers == 2) { c->stampTags.clear(); c->framesStamped = 0; }
    if (dc.overflow) return fail(c, CHORDVIS_E_CAPACITY, "a deferred raster list overflowed this frame; the visibility buffer is incomplete");
    return CHORDVIS_OK;
}

} // extern "C"
