// launch_raster: one raster pass of the visibility path (overview: kernels_raster.hip).  Fills the kernels' one argument from the
// context, decides from the pass's place in the frame and from the reports of frames past which kernels it runs, and calls the
// launches of the two stages (kernels_raster_setup.hip, kernels_raster.hip).  Every choice here is one of speed: the image is the same.

#include "raster_params.h"

#include <algorithm>
#include <cstdlib>

namespace chord {

#define LR_HIP(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

// The environment switches of the launcher: measurements, A/B runs and tests.  Read once per process, at the first raster pass.
struct RasterEnv {
    bool binInSetup;     // CHORDVIS_BIN_IN_SETUP   unset / non-zero: the record kernel bins its large records and clips its clip triangles itself; 0: the lists and raster_clip_and_bin_large_kernel
    int tileSlots;       // CHORDVIS_TILE_SLOTS     unset (-1): RasterParams::tileSlots follows the frame (sharded frames only); 0: every bin up to the split length stays whole; a number: that many slots in every frame
    int tileSplitMin;    // CHORDVIS_TILE_SPLIT_MIN unset or <= 0: TILE_SPLIT_MIN; a number: bins longer than that are cut into slices
    int tileSlice;       // CHORDVIS_TILE_SLICE     unset or < 512: TILE_SLICE; a number: the slice length, rounded up to 512s
    bool tileDirect;     // CHORDVIS_TILE_DIRECT    unset / non-zero: a light later pass runs without a schedule; 0: it keeps its schedule
    int tileTouched;     // CHORDVIS_TILE_TOUCHED   unset (1): a direct pass takes only the tiles it touched; 0: the direct form over every tile; above 1: with at most that many workgroups
    int setupWide;       // CHORDVIS_SETUP_WIDE     unset (1): a light later pass is set up a workgroup per cluster, up to TILE_DIRECT_MAX_CLUSTERS clusters; 0: raster_setup_kernel everywhere; above 1: up to that many clusters
    bool tileKeepLater;  // CHORDVIS_TILE_KEEP_LATER unset / non-zero: a heavy second pass runs under a kept schedule too; 0: only the first pass
    bool tileNext;       // CHORDVIS_TILE_NEXT      unset / non-zero: the tile kernel makes the next frame's schedule; 0: a schedule kernel every (keep + 1)-th frame
};
static const RasterEnv& raster_env()
{
    static const RasterEnv env = [] {
        const auto on = [](const char* name) { const char* e = getenv(name); return !e || atoi(e) != 0; };
        const auto number = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
        RasterEnv r;
        r.binInSetup = on("CHORDVIS_BIN_IN_SETUP");
        r.tileSlots = number("CHORDVIS_TILE_SLOTS", -1);
        r.tileSplitMin = number("CHORDVIS_TILE_SPLIT_MIN", -1);
        r.tileSlice = number("CHORDVIS_TILE_SLICE", -1);
        r.tileDirect = on("CHORDVIS_TILE_DIRECT");
        r.tileTouched = number("CHORDVIS_TILE_TOUCHED", 1);
        r.setupWide = number("CHORDVIS_SETUP_WIDE", 1);
        r.tileKeepLater = on("CHORDVIS_TILE_KEEP_LATER");
        r.tileNext = on("CHORDVIS_TILE_NEXT");
        return r;
    }();
    return env;
}

// A frame zeroes every count once (begin_frame_clear); outside a frame, or from the third raster
// call of a frame on, the pass slot is recycled by the launcher (recycle_pass_slot and the lists and masks a pass takes up later).
static bool recycles_slot(const ChordCtx* c) { return !c->inFrame || c->rasterCalls >= 2; }

// The fields of RasterParams that follow from the context and the pass.  What the later steps decide is set to "off" here.
static hipError_t fill_params(ChordCtx* c, const CmdList& in, bool clearTiles, const RasterEnv& env, RasterParams& p)
{
    p.hzbFused = 0; p.hzbMinA = nullptr; p.hzbMinB = nullptr; p.hzbMaxB = nullptr; p.tileRange = c->dTileRange;
    p.hzbExA = nullptr; p.hzbExB = nullptr;
    p.hzbDesc = c->hzb[0].desc;
    if (c->fuseHzb && c->shard.ranks == 1) {
        p.hzbFused = 1;
        p.hzbMinA = (clearTiles && c->fuseHzbTemp) ? c->hzb[0].minTexels : nullptr;
        p.hzbMinB = c->hzb[c->fuseHzbSlot].minTexels; p.hzbMaxB = c->hzb[c->fuseHzbSlot].maxTexels;
    } else if (c->fuseHzb) {
        // sharded frame: the same reduction, into the owned tiles' slots of the exchange buffers (launch_hzb_untile after the all-gathers)
        p.hzbFused = 1;
        p.hzbExA = (clearTiles && c->fuseHzbTemp) ? c->dHzbExchange : nullptr;
        p.hzbExB = c->dHzbFinalExchange;
    }
    p.count = in.count; p.cmds = in.cmds; p.cmdCap = std::max(in.capacity, 1u);
    if (c->shard.ranks > 1) {
        // sharded frame: only the clusters that touch this rank's screen tiles reach the setup kernel.  The lists of a frame
        // are the rank's own already (the group cull writes the rank's share of list 0 beside the full list; the HZB culls
        // of a sharded frame start from it); a list of unknown origin goes through the rank filter first.
        bool mine = false;
        if (in.cmds == c->lists[0].cmds && c->mineValid) { p.count = c->dCounts + 4; p.cmds = c->dMineCmds; mine = true; }
        else if (in.cmds == c->dMineCmds && c->mineValid) mine = true;
        else for (int k = 1; k < 3; k++) if (in.cmds == c->lists[k].cmds && c->listMine[k]) mine = true;
        if (!mine) {
            if (!c->dRankCmds) LR_HIP(hipMalloc((void**)&c->dRankCmds, sizeof(ChordDrawCmd) * c->allocCmds));
            CmdList filtered;
            filtered.count = c->dCounts + 5; filtered.cmds = c->dRankCmds; filtered.capacity = in.capacity;
            LR_HIP(hipMemsetAsync(filtered.count, 0, sizeof(uint32_t), c->stream));
            launch_rank_filter(c, in, filtered);
            p.count = filtered.count; p.cmds = filtered.cmds;
        }
    }
    p.objFrame = c->dObjFrame; p.objStatic = c->dObjStatic;
    p.meshlets = c->dMeshlets; p.meshletData = c->dMeshletData; p.positions = c->dPositions;
    p.materials = c->dMaterials; p.texAlpha = c->dTexAlpha; p.texcoords = c->dTexcoords;
    p.vis = (unsigned long long*)c->dVis;
    p.depthOut = (p.hzbFused && clearTiles) ? c->depthOutTarget : nullptr;     // (only the fused first pass writes a whole image)
    p.W = (float)c->width; p.H = (float)c->height; p.Wi = (int32_t)c->width; p.Hi = (int32_t)c->height;
    p.shard = c->shard;
    p.blockPool = c->dBlockPool; p.blockCap = (c->debugFlags & DBG_NO_BLOCKS) ? 0u : c->blockCap;
    p.blockForce = (c->debugFlags & DBG_FORCE_BLOCKS) ? 1u : 0u;
    p.tris = c->dTris; p.triCap = c->triCap / CHORD_LIST_SHARDS;
    p.trisC = c->dTrisC; p.triCapC = c->triCapC / CHORD_LIST_SHARDS;
    const uint32_t tiles = c->tilesX * c->tilesY;
    const uint32_t pass = c->rasterCalls & 1u;
    p.tileCount = c->dFrameState->tileCount + (size_t)pass * tiles * TC_STRIDE;
    p.tileBins = c->dTileBins + (size_t)pass * tiles * c->binCap; p.binCap = c->binCap;
    p.binPool = c->dBinPool + (size_t)pass * c->binPoolChunks * CHORD_BIN_CHUNK; p.binPoolChunks = c->binPoolChunks;
    p.binPoolCount = &c->dCounters->binPoolCount[pass];
    p.binChunkTab = c->dBinChunkTab + (size_t)pass * tiles * c->binMaxChunks; p.binMaxChunks = c->binMaxChunks;
    p.binStamp = ++c->rasterSerial;
    p.tilesX = c->tilesX; p.tilesY = c->tilesY;
    p.clipTris = c->dClipTris + (size_t)pass * (c->clipTriCap / 2); p.clipTriCap = c->clipTriCap / 2; p.pass = pass;
    p.largeList = c->dLargeList + (size_t)pass * (c->largeCap / 2); p.largeCap = c->largeCap / 2 / CHORD_LIST_SHARDS;   // per shard
    // The record kernel bins its large records and clips its clip triangles itself: no lists, no binner launch.  CHORDVIS_BIN_IN_SETUP=0:
    // the lists and raster_clip_and_bin_large_kernel (A/B runs; the same bins and images)
    p.binInSetup = env.binInSetup ? 1u : 0u;
    p.counters = c->dCounters;
    p.clearTiles = clearTiles ? 1u : 0u;
    p.depthOnly = c->depthOnly ? 1u : 0u; p.depthClamp = c->depthClamp ? 1u : 0u;
    p.biasConst = c->depthBiasConst; p.biasSlope = c->depthBiasSlope;
    p.debug = c->debugFlags;
    p.tileClocks = c->dTileClocks + (size_t)pass * CHORD_MAX_TILES;
    p.tileOrder = reinterpret_cast<uint2*>(c->dTileOrder); p.tileSlabs = c->dTileSlabs;
    p.tilePhase = c->dTileClocks + (size_t)2 * CHORD_MAX_TILES + (size_t)pass * CHORD_MAX_TILES * 8;
    p.slotHot = (c->debugFlags & DBG_FORCE_HOT) ? 64u : SLOT_HOT;
    // Sharded frames only: a rank of an 8-rank 4K frame owns 255 tiles (config 4: tile kernel 0.088 -> 0.053 ms per rank); the
    // one single-GPU case with fewer tiles than slots, a 1080p target, measured the same with and without
    // (profiles/r05_tile_kernel_experiments.txt, item 8).  (CHORDVIS_TILE_SLOTS: measurements only -- 0 keeps every bin up to
    // TILE_SPLIT_MIN entries whole, a number applies to every frame)
    p.tileSlots = env.tileSlots >= 0 ? (uint32_t)env.tileSlots : c->shard.ranks > 1 ? (uint32_t)c->numCUs * (CHORD_TILE_SHIFT == 6 ? 2u : 6u) : 0u;
    // (CHORDVIS_TILE_SPLIT_MIN / CHORDVIS_TILE_SLICE: measurements only -- the image does not depend on the cut)
    p.tileSplitMin = env.tileSplitMin > 0 ? (uint32_t)env.tileSplitMin : TILE_SPLIT_MIN;
    p.tileSliceLen = env.tileSlice >= 512 ? ((uint32_t)env.tileSlice + 511u) & ~511u : TILE_SLICE;
    p.hotTiles = c->dHotTiles ? c->dHotTiles + (size_t)pass * (1u + CHORD_HOT_TILES) : nullptr;
    p.leftCount = nullptr; p.leftCmds = nullptr;
    p.binHint = nullptr; p.countHint = nullptr; p.heavyHint = nullptr;
    p.orderKept = 0u; p.orderAll = 0u; p.tileOrderNext = nullptr; p.tileTouched = nullptr;
    p.wideMax = env.setupWide > 1 ? (uint32_t)env.setupWide : TILE_DIRECT_MAX_CLUSTERS;
    return hipSuccess;
}

// The counts of a pass slot that no frame clear has zeroed (recycles_slot)
static hipError_t recycle_pass_slot(ChordCtx* c, const RasterParams& p)
{
    const uint32_t tiles = p.tilesX * p.tilesY, pass = p.pass;
    LR_HIP(hipMemsetAsync(p.tileCount, 0, sizeof(uint32_t) * TC_STRIDE * tiles, c->stream));
    LR_HIP(hipMemsetAsync(&c->dCounters->clipTriCount[pass], 0, sizeof(uint32_t), c->stream));
    LR_HIP(hipMemsetAsync(c->dCounters->largeCount[pass], 0, sizeof(c->dCounters->largeCount[pass]), c->stream));
    LR_HIP(hipMemsetAsync(&c->dCounters->binPoolCount[pass], 0, sizeof(uint32_t), c->stream));
    if (!c->inFrame) { LR_HIP(hipMemsetAsync(c->dCounters->triCount, 0, sizeof(c->dCounters->triCount), c->stream));
                       LR_HIP(hipMemsetAsync(c->dCounters->triCountC, 0, sizeof(c->dCounters->triCountC), c->stream));
                       LR_HIP(hipMemsetAsync(c->dCounters->blockGranules, 0, sizeof(c->dCounters->blockGranules), c->stream)); }
    return hipSuccess;
}

// Does the block kernel run ahead of the record kernel (blocks), and in its variant that draws bin slots ahead (hot)
static hipError_t decide_blocks(ChordCtx* c, const CmdList& in, RasterParams& p, bool& blocks, bool& hot)
{
    const uint32_t pass = p.pass;
    // Pixel blocks: a list can only be dense (launch_is_dense) when its capacity allows one cluster per 16 pixels of the rank's
    // screen; then the block kernel runs ahead of the record kernel, which sets up what the block kernel left over.
    const uint64_t rankPixels = (uint64_t)c->width * c->height / (c->shard.ranks > 1 ? c->shard.ranks : 1u);
    const bool maybeDense = p.blockCap != 0u && (p.blockForce != 0u || (uint64_t)in.capacity * 16ull >= rankPixels);
    // ... and whether it IS dense the device decides from the list's length (launch_is_dense).  A list that could be dense but was
    // nowhere near it in the last frame the GPU finished (BASELINE config 4: one cluster per 60 pixels, capacity for one per 30)
    // gets no block kernel at all -- the launch would find nothing to do and cost its 4.5 us, twice per frame.  Half the device's
    // threshold, so a list at the threshold keeps its block kernel whichever way the last frame fell; the record kernel then
    // sets up the input list itself (no leftover list: launch_is_dense is false without one), and either way renders the same image.
    blocks = maybeDense;
    if (maybeDense && c->dBinHint) {
        p.countHint = c->dBinHint + 2 + pass;
        const uint32_t last = c->hBinHint[2 + pass];              // (0xFFFFFFFF: no frame yet)
        if (p.blockForce == 0u && last != 0xFFFFFFFFu && (uint64_t)last * 32ull < rankPixels) blocks = false;
    }
    hot = false;
    if (blocks) {
        if (c->dBinHint) p.binHint = c->dBinHint + pass;          // (host-visible word per pass, allocated with the G-buffer)
        if (!c->dLeftCmds) LR_HIP(hipMalloc((void**)&c->dLeftCmds, sizeof(ChordDrawCmd) * c->allocCmds));
        p.leftCount = c->dCounts + 6 + pass; p.leftCmds = c->dLeftCmds;
        if (recycles_slot(c)) LR_HIP(hipMemsetAsync(p.leftCount, 0, sizeof(uint32_t), c->stream));
        // the longest bin of this pass in the last frame the GPU finished: a hot tile then -> the variant that draws ahead now
        hot = (c->hBinHint && c->hBinHint[pass] >= SLOT_HOT) || (c->debugFlags & DBG_FORCE_HOT);
    }
    return hipSuccess;
}

// Does a later pass run without a schedule (RasterParams::orderKept = 2), then over the tiles it touched only (tileTouched),
// set up by the wide kernel (wide)?  laterOk: the pass is one the direct form and the kept schedule of a later pass are written for.
static hipError_t decide_direct(ChordCtx* c, bool clearTiles, bool blocks, const RasterEnv& env, RasterParams& p, bool& laterOk, bool& wide)
{
    const uint32_t tiles = p.tilesX * p.tilesY, pass = p.pass;
    // LIGHT later passes of a frame (the read-modify-write passes behind the first: config 3's second pass is 205 clusters, 436 of its
    // 2 040 tiles touched with 60 entries each) run WITHOUT a schedule: one workgroup per tile of the target, tile = workgroup index, a
    // tile whose counter line says "no entries" ends after that one load.  What such a pass has no use for -- heaviest-first order,
    // bins cut into slices -- is what the schedule kernel was there for (config 3 0.1792 -> 0.1759 ms, a 1080p frame 0.112 -> 0.109).
    // A pass with work in every tile needs them (config 4's second pass: 57 -> 115 us of tile kernel without), so the pass says what
    // it is in two host-visible words -- its serial under "heavy" when a bin is longer than tileSplitMin or it set up more than
    // TILE_DIRECT_MAX_CLUSTERS clusters, under "light" otherwise; written by the schedule kernel, or by the tile kernel of a direct
    // pass -- and runs direct while the latest report the host has seen says light.  A camera cut that sends the scene
    // through the second pass costs that frame balance, never a pixel (-DTILE_DIRECT=0 compiles the path out; CHORDVIS_TILE_DIRECT=0
    // turns it off at run time: A/B runs).
    // (laterOk: a read-modify-write pass of a frame with the HZB fused into its tile-out -- what the direct form and the kept schedule of
    // a later pass are written for)
    laterOk = c->inFrame && !clearTiles && p.hzbFused && !c->depthOnly && c->dBinHint && !(c->debugFlags & ~(DBG_NO_BLOCKS | DBG_FORCE_BLOCKS | DBG_FORCE_HOT | 524288u));
    if (laterOk) p.heavyHint = c->dBinHint + 4 + pass;
    if (TILE_DIRECT && env.tileDirect && laterOk) {
        const uint32_t heavySeen = c->hBinHint[4 + pass], lightSeen = c->hBinHint[6 + pass];
        // (the host runs frames ahead of the device -- a bench loop enqueues hundreds: what it reads is the state of a pass long past,
        // so the rule is "the latest report says light", not "a report of the last few frames"; a pass that reports both is heavy)
        if (lightSeen != 0u && (heavySeen == 0u || (int32_t)(lightSeen - heavySeen) > 0)) {
            p.orderKept = 2u;
        }
    }
    // A light later pass takes only the tiles it touched: its reservations set a bit per tile (bin_alloc: whoever draws slot 0) and
    // its tile kernel launches one workgroup per tile slot of the device, each taking the set bits w, w + G, ... (touched_tile) -- the
    // workgroups of untouched tiles, which held a slot for one round trip each and queued the touched ones behind them, are not
    // launched.  The bits must be set by the set-up kernels, so the choice is made before them.  Not in sharded frames (a rank's work
    // items are its own tiles: those keep one workgroup each) nor above 4 096 tiles (touched_tile reads one 8-byte word per lane).
    // CHORDVIS_TILE_TOUCHED=0: the direct form over every tile (A/B runs); a number above 1: at most that many workgroups (tests: a
    // pass that touched more tiles than the grid has workgroups).
    if (p.orderKept == 2u && env.tileTouched != 0 && c->shard.ranks <= 1 && tiles <= 64u * 64u) {
        p.tileTouched = c->dFrameState->tileTouched + (size_t)pass * (CHORD_MAX_TILES / 32u);
        if (recycles_slot(c)) LR_HIP(hipMemsetAsync(p.tileTouched, 0, sizeof(uint32_t) * ((tiles + 31u) / 32u), c->stream));
    }
    // A light later pass (direct: the latest report says at most TILE_DIRECT_MAX_CLUSTERS clusters) is set up by the wide kernel, a
    // workgroup per cluster: its few clusters would leave most SIMDs idle under one wave each.
    // The report may be stale (the host runs frames ahead): a list that turns out longer than TILE_DIRECT_MAX_CLUSTERS is set up by
    // the same launch one wave per cluster, the form of raster_setup_kernel (RasterParams::wideMax).  First passes, heavy later
    // passes, dense and sharded launches keep raster_setup_kernel.  CHORDVIS_SETUP_WIDE=0: raster_setup_kernel everywhere (A/B runs;
    // the same records, bins and images); a number above 1: the wide form up to that many clusters instead (tests: the edge between
    // the two forms at a pass's own count).
    wide = env.setupWide != 0 && p.orderKept == 2u && p.binInSetup && !blocks && c->shard.ranks <= 1;
    return hipSuccess;
}

// After the set-up stage: which schedule the tile kernel runs under -- a kept one, the one the last frame's tile kernel made,
// or a fresh one; returns whether the schedule kernel runs.
static bool decide_schedule(ChordCtx* c, bool clearTiles, bool laterOk, const RasterEnv& env, RasterParams& p)
{
    const uint32_t pass = p.pass;
    // The first pass of a main-view frame on one GPU writes EVERY tile (it is the clear): its work items are all the tiles whatever
    // their bins hold, and only their order (heaviest first) and the cut of long bins depend on this frame.  Both change slowly from
    // frame to frame, so the schedule of such a pass is kept in a buffer of its own and made again only every orderKeepFrames + 1
    // frames (chordvis_set_tile_schedule_keep, default 7; -DTILE_ORDER_KEEP=0 compiles the path out); in between the tile kernel takes items and order from the kept schedule and a tile's bin length and flags from the
    // counter line (RasterParams::orderKept) -- one launch less in most frames.  The image does not depend on order or cut.  (The
    // hints the schedule kernel leaves for the next frame -- longest bin, cluster count, hot tiles -- age with it.)
    bool makeOrder = p.orderKept != 2u;
    // Kept schedules (chordvis_set_tile_schedule_keep != 0; sharded frames too: a rank's work items are its own tiles, and the map they
    // follow changes only through install_tile_owners, which invalidates the schedules).  Slot 0: the first pass of a frame, which writes
    // every tile -- its work items never change, only their order and the cut of long bins.  Slot 1: the second pass; its schedule lists
    // EVERY tile of the rank, the untouched ones last (orderAll) -- a tile that a later frame touches must be a work item --, and an
    // untouched tile's workgroup ends after the load of its counter line, as in a direct pass.  Under a kept schedule the tile kernel
    // takes a tile's bin length and flags from the counter line (orderKept).
    // WHO MAKES THE SCHEDULE (round 6, end): the tile kernel of the frame before.  Its workgroup 0 orders THIS launch's bin counts --
    // final before the kernel starts -- into the slot's other buffer (tileOrderNext) while the other workgroups raster; the next frame
    // reads that buffer.  Every frame then runs under a schedule exactly one frame old and no frame launches a schedule kernel: measured
    // along a moving camera a one-frame-old schedule is as good as a fresh one, while one kept for 3 / 7 frames costs a config-4 or
    // masked frame 3 / 7 % of balance (profiles/r06_experiments.txt item 15) -- the launch it saved was 2 %.  CHORDVIS_TILE_NEXT=0: the
    // form before -- a schedule kernel every (keep + 1)-th frame, the schedule kept in between (A/B runs).
    const bool keepOk = TILE_ORDER_KEEP && c->orderKeepFrames && c->inFrame && !c->depthOnly && !(c->debugFlags & ~524288u);
    int slot = -1;
    if (keepOk && clearTiles && pass == 0u && c->dTileOrderKeep) slot = 0;
    else if (keepOk && env.tileKeepLater && laterOk && pass == 1u && c->dTileOrderKeep1) slot = 1;
    if (slot >= 0) {
        uint32_t& age = slot ? c->orderAge1 : c->orderAge;
        uint2* buf = reinterpret_cast<uint2*>(slot ? c->dTileOrderKeep1 : c->dTileOrderKeep);     // two schedules of 1 + tileItemCap items
        const size_t half = (size_t)1 + c->tileItemCap;
        p.orderAll = slot ? 1u : 0u;
        if (env.tileNext && p.orderKept == 2u) {
            // a direct pass reads no schedule and makes none: its tile kernel is as long as its slowest tile's chain of fetches (config 3:
            // 23 us), and the schedule part -- one workgroup's three dependent passes over the counter lines -- would be the longest
            // chain of the launch (measured: 23.2 -> 26.4 us).  A pass that turns heavy makes its first schedule with the schedule kernel.
            age = 0xFFFFFFFFu; p.orderAll = 0u;
        } else if (env.tileNext) {
            uint32_t& flip = c->orderFlip[slot];
            p.tileOrder = buf + flip * half; p.tileOrderNext = buf + (flip ^ 1u) * half;
            if (age != 0xFFFFFFFFu) { p.orderKept = 1u; makeOrder = false; }      // the schedule the last frame's tile kernel made
            age = 0u; flip ^= 1u;
        } else if (p.orderKept != 2u) {
            p.tileOrder = buf;
            if (age < c->orderKeepFrames) { age++; p.orderKept = 1u; makeOrder = false; }
            else age = 0u;
        } else p.orderAll = 0u;
    }
    return makeOrder;
}

hipError_t launch_raster(ChordCtx* c, const CmdList& in, bool clearTiles)
{
    const RasterEnv& env = raster_env();
    RasterParams p;
    bool blocks, hot, laterOk, wide;
    LR_HIP(fill_params(c, in, clearTiles, env, p));
    if (recycles_slot(c)) LR_HIP(recycle_pass_slot(c, p));
    LR_HIP(decide_blocks(c, in, p, blocks, hot));
    LR_HIP(decide_direct(c, clearTiles, blocks, env, p, laterOk, wide));
    launch_raster_setup(c, p, in.capacity, c->anyMasked, blocks, hot, wide);
    c->setupWide[p.pass] = wide ? 1u : 0u;
    const bool makeOrder = decide_schedule(c, clearTiles, laterOk, env, p);
    launch_raster_tiles(c, p, c->anyMasked, c->depthClamp, makeOrder, env.tileTouched > 1 ? (uint32_t)env.tileTouched : 0u);
    c->rasterCalls++;
    return hipSuccess;
}
#undef LR_HIP

} // namespace chord
