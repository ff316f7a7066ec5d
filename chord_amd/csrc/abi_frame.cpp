// C ABI, the frame: the host-side mirror of the reference's pass surface, and the read-backs of what a frame made.
//
//   chordvis_instance_culling      <- instanceCulling                 instance_culling.cpp:83-161
//   chordvis_hzb_culling           <- detail::hzbCulling              instance_culling.cpp:286-351
//   chordvis_render_mesh           <- renderMesh / renderMeshRasterPipe  mesh_raster.cpp:76-254
//   chordvis_visibility_stage0/1   <- gltfVisibilityRenderingStage0/1 mesh_raster.cpp:269-329
//   chordvis_build_hzb             <- buildHZB                        hzb.cpp:38-227
//   chordvis_render_frame          <- DeferredRenderer::render hot segment  renderer.cpp:315-345,489
//
// Host code only records work on one HIP stream (the reference records Vulkan commands into one
// command buffer); counts never come back to the CPU inside a frame.

#include "host_layer.h"

using namespace chord;

namespace {

void record(ChordCtx* c, int tag) { chord::stamp(c, tag); }

void begin_frame_stamps(ChordCtx* c)
{
    c->frameLaunchBase = c->launchCount;
    c->stampThisFrame = c->timers && (c->frameIndex % c->timerPeriod) == 0;
    c->frameIndex++;
    if (!c->stampThisFrame) return;
    if (c->timers == 1) { c->stampTags.clear(); c->framesStamped = 0; }
    c->framesStamped++;
    chord::stamp(c, S_FRAME_BEGIN);
}

HzbBuffers from_handle(const ChordHZB* h)
{
    HzbBuffers b;
    b.desc = h->desc; b.minTexels = h->minTexels; b.maxTexels = h->maxTexels; b.validRange = h->validRange;
    b.valid = h->minTexels != nullptr;
    return b;
}

CmdList from_handle(const ChordCountAndCmd& h)
{
    CmdList l; l.count = h.count; l.cmds = h.cmds; l.capacity = h.capacity; return l;
}

// addClearGbufferPass inside a frame: the visibility words are not memset; the first raster pass of the
// frame starts every 64x64 tile from zero in LDS and writes every tile back, which is the clear.
int begin_frame_clear(ChordCtx* c)
{
    // counters, the four command-list counts and both passes' tile bin counts: zeroed by the frame's first
    // kernel (object_cull), not by a separate memset
    c->frameStateZeroBytes = offsetof(FrameState, tileCount) + sizeof(uint32_t) * CHORD_TILECOUNT_STRIDE * ((size_t)2 * c->tilesX * c->tilesY);
    c->zeroFrameStateInCull = true;
    c->rasterCalls = 0;
    c->pendingClear = true;
    c->inFrame = true;
    return CHORDVIS_OK;
}

int do_raster(ChordCtx* c, const CmdList& in)
{
    // renderMesh (mesh_raster.cpp:208-254): the four (alphaMode x twoSided) pipeline buckets and
    // their filter passes collapse into one launch; the kernels read bTwoSided and alphaMode per cluster (masked
    // triangles carry their texture coordinates and are alpha-tested per pixel; blended materials draw nothing).
    const hipError_t e = launch_raster(c, in, c->pendingClear);
    c->pendingClear = false;
    if (e != hipSuccess) return fail(c, CHORDVIS_E_HIP, "launch_raster", e);
    CHORD_HIP(c, hipGetLastError());
    c->resolveFrame = true; c->resolveStale = false;   // the image now holds ids of this frame's objects and view (chordvis_resolve_attributes)
    return CHORDVIS_OK;
}

} // namespace

extern "C" {

int chordvis_clear_gbuffer(ChordCtx* c)
{
    int rc = ready(c, "clear_gbuffer");
    if (rc) return rc;
    // visibility = 0 / depth = 0.0 (render_textures.cpp:81-85,98-100).  Sharded: only the rank's own
    // chunk needs clearing (the all-gather overwrites the rest).
    if (c->shard.ranks > 1) {
        const uint64_t chunk = (uint64_t)c->shard.slotsPerRank * (CHORD_TILE * CHORD_TILE);
        CHORD_HIP(c, hipMemsetAsync(c->dVis + chunk * c->shard.rank, 0, chunk * 8, c->stream));
    } else {
        CHORD_HIP(c, hipMemsetAsync(c->dVis, 0, c->visWords * 8, c->stream));
    }
    CHORD_HIP(c, hipMemsetAsync(c->dCounters, 0, sizeof(DeviceCounters), c->stream));
    c->rasterCalls = 0;
    c->pendingClear = false;
    c->inFrame = false;
    return CHORDVIS_OK;
}

int chordvis_instance_culling(ChordCtx* c, ChordCountAndCmd* out)
{
    int rc = ready(c, "instance_culling");
    if (rc) return rc;
    launch_group_cull(c, c->lists[0]);                   // instanceCullingCS + clusterGroupCullingCS (objects + count, scatter)
    CHORD_HIP(c, hipGetLastError());
    if (out) *out = c->lists[0].handle();
    return CHORDVIS_OK;
}

int chordvis_hzb_culling(ChordCtx* c, const ChordHZB* hzb, int bFirstStage, ChordCountAndCmd in,
                         ChordCountAndCmd* outVisible, ChordCountAndCmd* outRejected)
{
    int rc = ready(c, "hzb_culling");
    if (rc) return rc;
    if (!hzb || !hzb->minTexels || !in.count || !in.cmds) return fail(c, CHORDVIS_E_INVALID, "hzb_culling: invalid HZB or command list");
    if ((rc = flush_pending_tail(c))) return rc;
    if ((rc = flush_view(c))) return rc;
    const HzbBuffers hb = from_handle(hzb);
    CmdList inL = from_handle(in);
    // Sharded frames: a rank culls (and later rasters) only the clusters that touch its pixel rows -- the group cull wrote them
    // to a list of their own -- so the occlusion tests shard with the screen like the raster does.  The decision per cluster
    // is a function of the cluster and the (exchanged, identical) HZB, so every owner of a straddling cluster decides alike.
    bool inMine = false;
    if (c->shard.ranks > 1) {
        if (inL.cmds == c->lists[0].cmds && c->mineValid) { inL.count = c->dCounts + 4; inL.cmds = c->dMineCmds; inMine = true; }
        else if (inL.cmds == c->dMineCmds && c->mineValid) inMine = true;
        else for (int k = 1; k < 3; k++) if (inL.cmds == c->lists[k].cmds && c->listMine[k]) inMine = true;
    }
    if (bFirstStage) {
        if (inL.cmds == c->lists[1].cmds || inL.cmds == c->lists[2].cmds) return fail(c, CHORDVIS_E_INVALID, "hzb_culling: first stage input must be the instanceCulling list");
        if (c->fusedCullDone && inL.cmds == c->lists[0].cmds && hzb->minTexels == c->hzb[c->historySlot].minTexels) {
            // (chordvis_render_frame on a short scene: frame_cull_fused_kernel tested every command it emitted against this chain)
            c->fusedCullDone = false;
        } else {
        if (!c->inFrame) CHORD_HIP(c, hipMemsetAsync(c->dCounts + 1, 0, 8, c->stream));
        c->listMine[1] = c->listMine[2] = inMine;
        launch_hzb_cull(c, hb, 0, inL, c->lists[1], &c->lists[2]);
        }
        if (outVisible) *outVisible = c->lists[1].handle();
        if (outRejected) *outRejected = c->lists[2].handle();
    } else {
        if (inL.cmds == c->lists[1].cmds) return fail(c, CHORDVIS_E_INVALID, "hzb_culling: second stage input aliases its output");
        CmdList vis1 = c->lists[1];
        vis1.count = c->dCounts + 3;
        if (!c->inFrame) CHORD_HIP(c, hipMemsetAsync(c->dCounts + 3, 0, 4, c->stream));
        c->listMine[1] = inMine;
        launch_hzb_cull(c, hb, 1, inL, vis1, nullptr);
        if (outVisible) *outVisible = vis1.handle();
        if (outRejected) *outRejected = ChordCountAndCmd{nullptr, nullptr, 0};
    }
    CHORD_HIP(c, hipGetLastError());
    return CHORDVIS_OK;
}

int chordvis_render_mesh(ChordCtx* c, ChordCountAndCmd in)
{
    int rc = ready(c, "render_mesh");
    if (rc) return rc;
    if (!in.count || !in.cmds) return CHORDVIS_OK;       // {nullptr, nullptr}: nothing to render (instance_culling.cpp:92-95)
    if ((rc = flush_view(c))) return rc;
    return do_raster(c, from_handle(in));
}

int chordvis_visibility_stage0(ChordCtx* c, const ChordHZB* hzbPrev, ChordCountAndCmd in, ChordCountAndCmd* outRejected, int* shouldStage1)
{
    int rc = ready(c, "visibility_stage0");
    if (rc) return rc;
    if (shouldStage1) *shouldStage1 = 0;
    if (outRejected) *outRejected = ChordCountAndCmd{nullptr, nullptr, 0};
    const bool hzbOn = hzbPrev && hzbPrev->minTexels && (c->hView.flags & CHORD_FLAG_HZB_CULL);   // mesh_raster.cpp:293
    if (hzbOn) {
        ChordCountAndCmd vis, rej;
        if ((rc = chordvis_hzb_culling(c, hzbPrev, 1, in, &vis, &rej))) return rc;
        if ((rc = chordvis_render_mesh(c, vis))) return rc;
        if (outRejected) *outRejected = rej;
        if (shouldStage1) *shouldStage1 = 1;
    } else {
        if ((rc = chordvis_render_mesh(c, in))) return rc;
    }
    return CHORDVIS_OK;
}

int chordvis_visibility_stage1(ChordCtx* c, const ChordHZB* hzb, ChordCountAndCmd in)
{
    int rc = ready(c, "visibility_stage1");
    if (rc) return rc;
    ChordCountAndCmd vis;
    if ((rc = chordvis_hzb_culling(c, hzb, 0, in, &vis, nullptr))) return rc;
    return chordvis_render_mesh(c, vis);
}

int chordvis_build_hzb(ChordCtx* c, int bBuildMin, int bBuildMax, int bBuildValidRange, int slot, ChordHZB* out)
{
    int rc = ready(c, "build_hzb");
    if (rc) return rc;
    if (slot < 0 || slot > 2 || !(bBuildMin || bBuildMax) || (bBuildValidRange && !(bBuildMin && bBuildMax)))   // hzb.cpp:43-47
        return fail(c, CHORDVIS_E_INVALID, "build_hzb: slot in 0..2, at least one channel, valid range needs min and max");
    if ((rc = flush_pending_tail(c))) return rc;
    // (a sharded context: from the resolved, row-major image -- chordvis_frame_resolve_visibility / phase c)
    launch_hzb_build(c, c->hzb[slot], bBuildMin != 0, bBuildMax != 0, bBuildValidRange != 0);
    CHORD_HIP(c, hipGetLastError());
    if (out) {
        *out = c->hzb[slot].handle();
        if (!bBuildMax) out->maxTexels = nullptr;
        if (!bBuildValidRange) out->validRange = nullptr;
    }
    return CHORDVIS_OK;
}

int chordvis_reset_history(ChordCtx* c)
{
    if (!c) return CHORDVIS_E_INVALID;
    c->pendingTailSlot = 0;
    c->historySlot = 0;
    return CHORDVIS_OK;
}

static int render_frame_impl(ChordCtx* c)
{
    int rc = ready(c, "render_frame");
    if (rc) return rc;
    if (c->comm) return comm_render_frame(c);            // one process per GPU: the library runs the two all-gathers (RCCL)
    if (c->shard.ranks > 1) return fail(c, CHORDVIS_E_INVALID, "render_frame: a sharded context needs a communicator (chordvis_comm_init_rank), a ChordGroup, or the host drives frame_phase_a/b/c");
    begin_frame_stamps(c);
    if ((rc = begin_frame_clear(c))) return rc;                                       // renderer.cpp:315
    record(c, S_CLEAR);
    ChordHZB hist;
    const bool haveHist = c->historySlot != 0;
    if (haveHist) hist = c->hzb[c->historySlot].handle();
    const int next = c->historySlot == 1 ? 2 : 1;
    ChordCountAndCmd post;
    // (short scenes: instanceCulling and the phase-0 occlusion cull of stage 0 are one kernel -- launch_group_cull is told what stage 0
    // will cull against, and chordvis_hzb_culling finds its lists made)
    c->fuseCullFrame = true;
    c->fuseCullHzb = (haveHist && (c->hView.flags & CHORD_FLAG_HZB_CULL)) ? &c->hzb[c->historySlot] : nullptr;
    c->fusedCullDone = false;
    rc = chordvis_instance_culling(c, &post);                                         // :321 (its first kernel also carries the previous frame's HZB tail)
    c->fuseCullFrame = false; c->fuseCullHzb = nullptr;
    if (rc) return rc;
    record(c, S_CULL);
    // buildHZB is fused into the raster: the tile kernel reduces every finished 64x64 tile to mips 0..5 of the
    // chain kept as history (and of the temporary chain stage 1 culls against); only the one-block tail remains.
    c->fuseHzb = true;
    c->fuseHzbSlot = next;
    c->fuseHzbTemp = haveHist && (c->hView.flags & CHORD_FLAG_HZB_CULL);
    ChordCountAndCmd rejected;
    int stage1 = 0;
    rc = chordvis_visibility_stage0(c, haveHist ? &hist : nullptr, post, &rejected, &stage1);   // :326
    c->fusedCullDone = false;
    record(c, S_STAGE0_END);
    c->shouldStage1 = stage1 != 0;
    if (!rc && stage1) {
        // buildHZB(min) :334 -- levels 0..5 came out of the tile kernel; the one-block tail (levels 6..) is reduced by the
        // blocks of the phase-1 cull themselves unless the chain does not fit their LDS budget (never for targets <= 4096^2)
        const ChordHZBDesc& hd = c->hzb[0].desc;
        uint32_t tailFloats = 0;
        for (uint32_t l = 6; l < hd.mipCount; l++) tailFloats += std::max(1u, hd.width >> l) * std::max(1u, hd.height >> l);
        c->hzbTailInCull = hd.mipCount > 6u && tailFloats <= 1408u && !(c->debugFlags & 131072u);
        if (!c->hzbTailInCull) launch_hzb_tail(c, c->hzb[0], false, false);
        record(c, S_HZB0);
        ChordHZB tmp = c->hzb[0].handle();
        rc = chordvis_visibility_stage1(c, &tmp, rejected);                           // :337
        c->hzbTailInCull = false;
        record(c, S_STAGE1_END);
    }
    c->fuseHzb = false;
    if (rc) return rc;
    // buildHZB(min,max,range) :343 -- mips 0..5 are written; the one-block tail (mips 6.., range) is carried by the next
    // frame's first kernel, or launched by whoever reads the chain first (flush_pending_tail)
    c->hzb[next].valid = true;
    c->hzb[next].uploaded = false;                                                    // (the tile kernel wrote it: the library's own chain)
    c->pendingTailSlot = next;
    record(c, S_HZBF);
    c->historySlot = next;                                                            // :489
    c->inFrame = false;
    c->lastFrameLaunches = (uint32_t)(c->launchCount - c->frameLaunchBase);
    return CHORDVIS_OK;
}

// Sharded frame.  The single-GPU frame with two differences: the tile kernel writes each tile's words to the
// tile's slot of the rank's chunk and its HZB texels (mips 0..5) to the tile's slots of the two exchange buffers, and after
// each all-gather a copy kernel (launch_hzb_untile) moves every rank's texels to their places in the chain.
//   phase a   clear .. stage 0 raster (owned tiles; fused reduction into the exchange slots)
//   [all-gather of the mid-frame exchange buffer -- only when phase a reported a second stage]
//   phase b   chain 0 from the exchanged texels, phase-1 cull (reduces mips 6.. itself), stage 1 raster
//   [all-gather of the end-of-frame exchange buffer (small) and of the visibility words (the image)]
//   phase c   row-major copy of the image + the history chain from the exchanged texels; ends the frame
// Hosts that let the image travel beside the next frame call chordvis_frame_phase_c_finish once the small exchange has landed
// and chordvis_frame_resolve_visibility whenever the image has.
// The sharded group cull's first half (optional: a frame that starts at phase a culls every group on every rank, as before).
//   phase cull   object pass + the group tests of this rank's range of count blocks -> rank-mask words in its chunk of the cull exchange buffer
//   [all-gather of the cull exchange buffer: chordvis_cull_exchange_ptr, chunk = chordvis_cull_exchange_chunk_bytes]
//   phase a      masks and block counts from the exchanged words, prefix + scatter (the rank's own list), then as above
static int frame_phase_cull_impl(ChordCtx* c)
{
    int rc = ready(c, "frame_phase_cull");
    if (rc) return rc;
    if (c->shard.ranks <= 1) return fail(c, CHORDVIS_E_INVALID, "frame_phase_cull: the context is not sharded");
    if (c->cullPhaseDone) return fail(c, CHORDVIS_E_INVALID, "frame_phase_cull: called twice without chordvis_frame_phase_a in between");
    if (!cull_shardable_config(c)) return fail(c, CHORDVIS_E_INVALID, "frame_phase_cull: the sharded cull needs 2..8 ranks and the flat cull mode (start the frame at chordvis_frame_phase_a instead)");
    if ((rc = ensure_cull_exchange(c))) return rc;       // (made by upload_scene / set_shard already: a no-op)
    begin_frame_stamps(c);
    if ((rc = begin_frame_clear(c))) return rc;
    record(c, S_CLEAR);
    launch_cull_masks(c);
    CHORD_HIP(c, hipGetLastError());
    c->cullPhaseDone = true;
    record(c, S_CULL);
    return CHORDVIS_OK;
}

static int frame_phase_a_impl(ChordCtx* c)
{
    int rc = ready(c, "frame_phase_a");
    if (rc) return rc;
    if (c->shard.ranks <= 1) return fail(c, CHORDVIS_E_INVALID, "frame_phase_a: the context is not sharded");
    if (c->cullPhaseDone) record(c, S_EXCH_CULL);       // time spent in the all-gather of the rank masks (the library's or the caller's)
    else {
        begin_frame_stamps(c);
        if ((rc = begin_frame_clear(c))) return rc;
        record(c, S_CLEAR);
    }
    ChordCountAndCmd post;
    // (the post-cull list is not handed out here: a rank writes only its own share of it; chordvis_last_frame_cmds, the read-back
    // and the tile marker make the full list when they are asked for it -- from the cull's own masks, which every rank holds for every group)
    c->lazyFullList = true;
    rc = chordvis_instance_culling(c, &post);                                        // (its first kernel carries the previous frame's HZB tail)
    c->lazyFullList = false;
    if (rc) return rc;
    record(c, S_CULL);
    ChordHZB hist;
    const bool haveHist = c->historySlot != 0;
    if (haveHist) hist = c->hzb[c->historySlot].handle();
    c->fuseHzb = true;
    c->fuseHzbSlot = c->historySlot == 1 ? 2 : 1;
    c->fuseHzbTemp = haveHist && (c->hView.flags & CHORD_FLAG_HZB_CULL);
    c->exchangeSlotsFresh = true;                        // (the fused tile kernel of this frame's passes writes the rank's exchange slots)
    ChordCountAndCmd rejected;
    int stage1 = 0;
    rc = chordvis_visibility_stage0(c, haveHist ? &hist : nullptr, post, &rejected, &stage1);
    c->fuseHzb = false;
    if (rc) return rc;
    c->shouldStage1 = stage1 != 0;
    c->lastRejected = from_handle(rejected);
    record(c, S_STAGE0_END);
    return CHORDVIS_OK;
}

// phase b: [mid-frame exchange buffer all-gathered by the caller] -> HZB chain 0 -> stage 1.
static int frame_phase_b_impl(ChordCtx* c)
{
    int rc = ready(c, "frame_phase_b");
    if (rc) return rc;
    if (!c->shouldStage1) return CHORDVIS_OK;
    record(c, S_EXCH_HZB);       // time spent in the all-gather of the mid-frame exchange buffer (the library's or the caller's)
    launch_hzb_untile(c, c->hzb[0], false);
    CHORD_HIP(c, hipGetLastError());
    {   // levels 6.. of the chain: reduced by the blocks of the phase-1 cull themselves when they fit (render_frame_impl)
        const ChordHZBDesc& hd = c->hzb[0].desc;
        uint32_t tailFloats = 0;
        for (uint32_t l = 6; l < hd.mipCount; l++) tailFloats += std::max(1u, hd.width >> l) * std::max(1u, hd.height >> l);
        c->hzbTailInCull = hd.mipCount > 6u && tailFloats <= 1408u && !(c->debugFlags & 131072u);
        if (!c->hzbTailInCull) launch_hzb_tail(c, c->hzb[0], false, false);
    }
    record(c, S_HZB0);
    ChordHZB tmp = c->hzb[0].handle();
    c->fuseHzb = true;
    c->fuseHzbTemp = false;
    rc = chordvis_visibility_stage1(c, &tmp, c->lastRejected.handle());
    c->fuseHzb = false;
    c->hzbTailInCull = false;
    if (rc) return rc;
    record(c, S_STAGE1_END);
    return CHORDVIS_OK;
}

// [end-of-frame exchange buffer all-gathered by the caller] -> the history chain; the frame is over.  Mips 0..5 are copied
// from the slots; the one-block tail (mips 6.., valid range from the tiles' pairs) rides on the next frame's first kernel, or
// is launched by whoever reads the chain first (flush_pending_tail) -- as in the single-GPU frame.
static int frame_phase_c_finish_impl(ChordCtx* c)
{
    int rc = ready(c, "frame_phase_c_finish");
    if (rc) return rc;
    if (c->shard.ranks <= 1) return fail(c, CHORDVIS_E_INVALID, "frame_phase_c_finish: the context is not sharded");
    // the history chain, the tiles' valid ranges and their loads come from the end-of-frame exchange slots, which only the fused
    // tile kernel of chordvis_frame_phase_a / _b writes: a frame rastered with the stand-alone passes has none to unpack
    if (!c->exchangeSlotsFresh) return fail(c, CHORDVIS_E_INVALID, "frame_phase_c: no chordvis_frame_phase_a in this frame -- the end-of-frame exchange slots are stale (a frame rastered with the stand-alone passes builds its history with chordvis_build_hzb from the resolved image)");
    c->exchangeSlotsFresh = false;
    const int next = c->historySlot == 1 ? 2 : 1;
    launch_hzb_untile(c, c->hzb[next], true);
    CHORD_HIP(c, hipGetLastError());
    c->pendingTailSlot = next;
    record(c, S_HZBF);
    c->historySlot = next;
    c->inFrame = false;
    c->lastFrameLaunches = (uint32_t)(c->launchCount - c->frameLaunchBase);
    return CHORDVIS_OK;
}

// phase c: [both end-of-frame all-gathers done by the caller] -> row-major copy of the image + the history chain.
static int frame_phase_c_impl(ChordCtx* c)
{
    int rc = ready(c, "frame_phase_c");
    if (rc) return rc;
    if (c->shard.ranks <= 1) return fail(c, CHORDVIS_E_INVALID, "frame_phase_c: the context is not sharded");
    record(c, S_EXCH_VIS);       // time spent in the end-of-frame all-gathers
    launch_detile(c);
    CHORD_HIP(c, hipGetLastError());
    return frame_phase_c_finish_impl(c);
}

// A failed frame must not leave frame-scoped state behind (the stand-alone passes that may follow would skip their
// count resets, a later frame would inherit a fused-HZB request).
static int end_failed_frame(ChordCtx* c, int rc)
{
    if (rc && c) {
        if (c->zeroFrameStateInCull) { (void)hipMemsetAsync(c->dFrameState, 0, c->frameStateZeroBytes, c->stream); c->zeroFrameStateInCull = false; }
        c->inFrame = false; c->fuseHzb = false; c->pendingClear = false; c->shouldStage1 = false; c->cullPhaseDone = false; c->exchangeSlotsFresh = false;
    }
    return rc;
}
int chordvis_render_frame(ChordCtx* c) { return end_failed_frame(c, render_frame_impl(c)); }
int chordvis_frame_phase_cull(ChordCtx* c) { return end_failed_frame(c, frame_phase_cull_impl(c)); }
int chordvis_frame_phase_a(ChordCtx* c) { return end_failed_frame(c, frame_phase_a_impl(c)); }
int chordvis_frame_phase_b(ChordCtx* c) { return end_failed_frame(c, frame_phase_b_impl(c)); }
int chordvis_frame_phase_c(ChordCtx* c) { return end_failed_frame(c, frame_phase_c_impl(c)); }
int chordvis_frame_phase_c_finish(ChordCtx* c) { return end_failed_frame(c, frame_phase_c_finish_impl(c)); }

// The row-major copy of the (gathered) rank-major visibility words of the CURRENT buffer pair, on `hipStream` (NULL: the
// context's stream) -- phase c's first half, for pipelined hosts that run it beside the next frame.
int chordvis_frame_resolve_visibility(ChordCtx* c, void* hipStream)
{
    if (!c || !c->dVis || c->shard.ranks <= 1) return fail(c, CHORDVIS_E_INVALID, "frame_resolve_visibility: a sharded context with a gbuffer");
    launch_detile(c, (hipStream_t)hipStream);
    CHORD_HIP(c, hipGetLastError());
    return CHORDVIS_OK;
}

// Orders `hipStream` (NULL: the context's stream) behind the completion of the resolved image of the last submitted frame.
// Needed only after pipelined ChordGroup frames, whose image is gathered beside the context's stream; a no-op otherwise.
int chordvis_wait_visibility(ChordCtx* c, void* hipStream)
{
    if (!c || !c->dVis) return fail(c, CHORDVIS_E_INVALID, "wait_visibility: no gbuffer");
    hipStream_t s = hipStream ? (hipStream_t)hipStream : c->stream;
    if (c->visReadyEvent[0]) CHORD_HIP(c, hipStreamWaitEvent(s, c->visReadyEvent[0], 0));
    else if (s != c->stream) {
        // not pipelined: the image is complete when the context's stream is; order the foreign stream behind it
        hipEvent_t e = nullptr;
        CHORD_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        hipError_t rc = hipEventRecord(e, c->stream);
        if (rc == hipSuccess) rc = hipStreamWaitEvent(s, e, 0);
        (void)hipEventDestroy(e);                                    // (destruction is deferred until the event has completed)
        if (rc != hipSuccess) return fail(c, CHORDVIS_E_HIP, "wait_visibility", rc);
    }
    return CHORDVIS_OK;
}

int chordvis_last_frame_cmds(ChordCtx* c, ChordCountAndCmd* out)
{
    if (!c || !out || !c->sceneLoaded) return fail(c, CHORDVIS_E_INVALID, "last_frame_cmds: no scene");
    launch_full_list(c);                                             // (a sharded frame wrote only the rank's share of it)
    CHORD_HIP(c, hipGetLastError());
    *out = c->lists[0].handle();
    return CHORDVIS_OK;
}

int chordvis_history_hzb(ChordCtx* c, ChordHZB* out)
{
    if (!c || !out || c->historySlot == 0) return fail(c, CHORDVIS_E_INVALID, "history_hzb: no history yet");
    { const int rc = flush_pending_tail(c); if (rc) return rc; }
    *out = c->hzb[c->historySlot].handle();
    return CHORDVIS_OK;
}

// ----------------------------------------------------------------------------------- readback --

int chordvis_readback_visibility(ChordCtx* c, uint64_t* host)
{
    if (!c || !host || !c->dVis) return fail(c, CHORDVIS_E_INVALID, "readback_visibility: no gbuffer");
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    if (c->visReadyEvent[0]) CHORD_HIP(c, hipEventSynchronize(c->visReadyEvent[0]));   // (pipelined group: the image is resolved beside the stream)
    const uint64_t* src = c->shard.ranks > 1 ? c->dVisResolved : c->dVis;
    CHORD_HIP(c, hipMemcpy(host, src, (size_t)c->width * c->height * 8, hipMemcpyDeviceToHost));
    return CHORDVIS_OK;
}

// Pipelined sharded frames: the image of the frame BEFORE the last submitted one (the other buffer pair).
int chordvis_readback_previous_visibility(ChordCtx* c, uint64_t* host)
{
    if (!c || !host || !c->dVisResolvedAlt) return fail(c, CHORDVIS_E_INVALID, "readback_previous_visibility: no second frame in flight (chordvis_swap_visibility)");
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    if (c->visReadyEvent[1]) CHORD_HIP(c, hipEventSynchronize(c->visReadyEvent[1]));
    CHORD_HIP(c, hipMemcpy(host, c->dVisResolvedAlt, (size_t)c->width * c->height * 8, hipMemcpyDeviceToHost));
    return CHORDVIS_OK;
}

int chordvis_readback_cmds(ChordCtx* c, ChordCountAndCmd h, ChordDrawCmd* host, uint32_t cap, uint32_t* outCount)
{
    if (!c || !h.count || !h.cmds || !outCount) return fail(c, CHORDVIS_E_INVALID, "readback_cmds: invalid handle");
    if (h.cmds == c->lists[0].cmds) { launch_full_list(c); CHORD_HIP(c, hipGetLastError()); }
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    uint32_t n = 0;
    CHORD_HIP(c, hipMemcpy(&n, h.count, 4, hipMemcpyDeviceToHost));
    *outCount = n;
    const uint32_t m = std::min(std::min(n, cap), h.capacity);
    if (host && m) {
        CHORD_HIP(c, hipMemcpy(host, h.cmds, sizeof(ChordDrawCmd) * m, hipMemcpyDeviceToHost));
        // device meshlet ids are flattened over assets; hand back asset-relative ids (the reference's cmd.y)
        for (uint32_t i = 0; i < m; i++) {
            if (host[i].objectId < c->objectCount) host[i].meshletId -= c->hPrims[c->hObjStatic[host[i].objectId].prim].assetMeshletBase;
        }
    }
    return CHORDVIS_OK;
}

int chordvis_readback_hzb(ChordCtx* c, const ChordHZB* hzb, uint16_t* hostMin, uint16_t* hostMax, uint32_t hostValidRange[2])
{
    if (!c || !hzb) return fail(c, CHORDVIS_E_INVALID, "readback_hzb: null handle");
    { const int rc = flush_pending_tail(c); if (rc) return rc; }
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    const size_t bytes = sizeof(uint16_t) * hzb->desc.totalTexels;
    if (hostMin && hzb->minTexels) CHORD_HIP(c, hipMemcpy(hostMin, hzb->minTexels, bytes, hipMemcpyDeviceToHost));
    if (hostMax && hzb->maxTexels) CHORD_HIP(c, hipMemcpy(hostMax, hzb->maxTexels, bytes, hipMemcpyDeviceToHost));
    if (hostValidRange && hzb->validRange) CHORD_HIP(c, hipMemcpy(hostValidRange, hzb->validRange, 8, hipMemcpyDeviceToHost));
    return CHORDVIS_OK;
}

int chordvis_upload_history_hzb(ChordCtx* c, const uint16_t* hostMin)
{
    if (!c || !hostMin || !c->dVis) return fail(c, CHORDVIS_E_INVALID, "upload_history_hzb: no gbuffer");
    c->pendingTailSlot = 0;                              // the uploaded chain replaces whatever was pending
    const int slot = c->historySlot == 1 ? 2 : 1;
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    CHORD_HIP(c, hipMemcpy(c->hzb[slot].minTexels, hostMin, sizeof(uint16_t) * c->hzb[slot].desc.totalTexels, hipMemcpyHostToDevice));
    c->hzb[slot].valid = true;
    c->hzb[slot].uploaded = true;                        // (its levels 6.. are the host's: frame_cull_fused_kernel would reduce them from level 5)
    c->historySlot = slot;
    return CHORDVIS_OK;
}

} // extern "C"
