// What host and device code of the software rasterizer share (overview: kernels_raster.hip): the kernels' one argument, the words
// of a tile's counter line, the debug bits, the tuning constants that both the kernels and launch_raster (raster_launch.cpp) read,
// and the launches of the two stages.  A constant that only device code reads stays beside it: in the stage's file, or in raster_device.h when both stages read it.

#pragma once

#include "device_layer.h"

namespace chord {

#define TC_STRIDE CHORD_TILECOUNT_STRIDE   // one bin counter per 64-byte line (no false sharing between tiles)
// words of a tile's counter line: 0 = bin entries, 1 = of which pixel blocks (words 0 and 1 are ONE 64-bit counter for the
// block path: a block's bin slot and the block count travel in a single atomic), 2 = ticket of the slices of a split tile
#define TC_BLOCKS 1u
#define TC_TICKET 2u
// 3 = the bin holds entries of alpha-tested triangles (a flag, plain stores).  Nothing reads it any more: it was the work list of a
// masked pass of its own in front of the tile kernel, 37 % slower than the tile kernel's MASKED instantiations and deleted
// (profiles/r05_masked_variants.txt).  The stores are part of live instruction streams; a later change can drop them.
#define TC_MASKED 3u

struct RasterParams {
    const uint32_t* count; const ChordDrawCmd* cmds;
    uint32_t cmdCap;                                    // entries the list `cmds` has room for (>= 1): a wave may read its first command before it knows the count
    uint32_t* leftCount; ChordDrawCmd* leftCmds;         // clusters of a dense launch that do not become pixel blocks (raster_setup_blocks_kernel -> raster_setup_kernel), or NULL
    const DObjFrame* objFrame; const DObjStatic* objStatic;
    const DMeshlet* meshlets; const uint32_t* meshletData; const float* positions;
    const DMaterial* materials; const uint8_t* texAlpha; const float* texcoords;   // masked materials (texcoords may be null: uv = 0)
    unsigned long long* vis;
    float* depthOut;                                    // depth-only views: the fused tile-out writes the D32 image itself (row-major floats) instead of the 64-bit words
    float W, H; int32_t Wi, Hi;
    ShardInfo shard;
    TriRec* tris; uint32_t triCap;                      // 48-byte records, capacity per list shard
    TriRecC* trisC; uint32_t triCapC;                   // 32-byte records
    uint32_t* tileCount; uint32_t* tileBins; uint32_t binCap; uint32_t tilesX, tilesY;
    uint32_t* binPool; uint32_t binPoolChunks; uint32_t* binPoolCount;   // overflow chunks of this pass
    unsigned long long* binChunkTab; uint32_t binStamp; uint32_t binMaxChunks;   // [tile][binMaxChunks] serial << 32 | chunk
    unsigned long long* blockPool; uint32_t blockCap;   // pixel blocks of small clusters, granules of 16 bytes per list shard (0: path off)
    uint32_t blockForce;                                // debug: every launch takes the setup kernel's BLOCKS body
    ClipTri* clipTris; uint32_t clipTriCap; uint32_t pass;   // raster pass of the frame (0 / 1): clip / large count slot
    uint32_t* largeList; uint32_t largeCap;                  // records touching more than 2x2 tiles (binned by raster_clip_and_bin_large_kernel), without binInSetup
    uint32_t binInSetup;                                // 1: the record kernel bins its large records and clips + bins its clip triangles itself (no lists, no
                                                        // raster_clip_and_bin_large_kernel); 0: the lists and the binner launch (launch_raster: CHORDVIS_BIN_IN_SETUP)
    DeviceCounters* counters;
    uint2* tileOrder;                                   // [0].x = work item count, [1..] = {tile | slice << 12 | (slices-1) << 22, bin count}, heaviest first
    unsigned long long* tileSlabs;                      // one TILE x TILE accumulation slab per tile (all zero between uses)
    // fused HZB (single-GPU frames): the tile kernel reduces its finished 64x64 tile to mips 0..5
    uint32_t hzbFused;                                  // 0: off (later passes merge with global atomicMax)
    ChordHZBDesc hzbDesc;
    uint16_t* hzbMinA;                                  // temporary chain for stage 1 (first pass only) or NULL
    uint16_t* hzbMinB; uint16_t* hzbMaxB;               // chain kept as history
    // sharded frames: the texels go to the tile's slot of the exchange buffers instead (all-gathered, then hzb_untile_kernel)
    uint16_t* hzbExA;                                   // mid-frame exchange (min chain after the first pass), or NULL
    uint16_t* hzbExB;                                   // end-of-frame exchange (min | max | valid range | bin entries)
    uint32_t* tileRange;                                // per tile {min bits, max bits} of valid depth
    unsigned long long* tileClocks;                     // debug: per-tile elapsed wall clock ticks (DBG_TILE_CLOCKS)
    unsigned long long* tilePhase;                      // debug: 8 phase accumulators per tile
    uint32_t depthOnly, depthClamp;                     // PASS_TYPE_DEPTH (renderMeshDepth, mesh_raster.cpp:159-206): cull NONE, no id; depth clamp: near / far do not clip
    float biasConst, biasSlope;                         // vkCmdSetDepthBias(const, 0, slope), applied to the vertex depths of a depth-pass triangle
    uint32_t clearTiles;                                // first raster pass of a frame: tiles start from 0
    uint32_t* binHint;                                  // host-visible word: the longest bin of this pass (tile order kernel -> launch_raster of later frames), or NULL
    uint32_t* countHint;                                // host-visible word: the number of clusters this pass set up, or NULL
    uint32_t slotHot;                                   // bin length from which a tile counts as hot (SLOT_HOT; tests lower it)
    uint32_t* hotTiles;                                 // [1 + CHORD_HOT_TILES] this pass's hot tiles of the LAST frame (count, then tile | very hot << 31): written by the tile schedule, read by the block kernel's hot variant
    uint32_t tileSlots;                                 // tile workgroups the device holds at once (2 per CU); a pass with fewer non-empty tiles than that cuts its bins finer (tile_order_part), 0: never
    uint32_t tileSplitMin, tileSliceLen;                // bins longer than tileSplitMin entries are cut into slices of tileSliceLen (TILE_SPLIT_MIN, TILE_SLICE)
    uint2* tileOrderNext;                               // non-null: the tile kernel's extra workgroup makes the NEXT frame's schedule of this pass here, from this frame's bin counts (launch_raster)
    uint32_t orderAll;                                  // the schedule lists every (owned) tile, empty ones last, also in a pass that does not clear: a KEPT schedule of such a pass must name the tiles a later frame touches
    uint32_t orderKept;                                 // 1: tileOrder is the schedule of an EARLIER frame's first pass (launch_raster: TILE_ORDER_KEEP) -- the items and their order are taken from it, a tile's bin length and flags from the counter line of this pass
                                                        // 2: no schedule at all (later passes of a frame: launch_raster TILE_DIRECT) -- work item i is tile i, whole; a tile without entries is left alone
    uint32_t* heavyHint;                                // host-visible words [0] / [2]: this pass's serial (binStamp) stored by whoever finds the pass HEAVY (a bin beyond tileSplitMin entries, more than
                                                        // TILE_DIRECT_MAX_CLUSTERS clusters) / LIGHT (launch_raster: only a pass that was light a moment ago runs without a schedule), or NULL
    uint32_t* tileTouched;                              // direct passes that take only touched tiles (launch_raster TILE_TOUCHED): this pass's bits of FrameState::tileTouched,
                                                        // set by bin_alloc for the slot 0 of a tile, read by the tile kernel (touched_tile); NULL: no bit is set or read
    uint32_t debug;                                     // ablation switches (chordvis_set_debug), 0 in production
    uint32_t wideMax;                                   // raster_setup_wide_kernel: a list longer than this is set up one wave per cluster (TILE_DIRECT_MAX_CLUSTERS)
};
// The per-phase clocks of the setup kernels (debug bit 512) and of the tile kernel (bit 16) exist only in a build with
// -DRASTER_PROFILE=1 (python chord_amd/build.py --tag prof -DRASTER_PROFILE=1; the profile tools load that library): their
// accumulators are 64-bit values held across the kernels' main loops, and those loops are at the 102-SGPR limit -- in the
// product build they cost the block kernel 90 of its 145 v_readlane / v_writelane and 5 % of its time.
// The measurement-only ablation switches below (everything but DBG_NO_BLOCKS / DBG_FORCE_BLOCKS / DBG_FORCE_HOT, which tests
// run because they do not change results) exist only in a build with -DRASTER_ABLATION=1: tested at run time they keep
// values alive and conditions in the innermost loops of kernels that are register-bound.  chordvis_set_debug refuses a switch
// the library was not built with (device_layer.h).
#define ABL(p, flag) (RASTER_ABLATION && ((p).debug & (flag)) != 0u)
#define DBG_NO_PIXELS   1u    // skip every visibility write
#define DBG_NO_BIN      2u    // setup only: no records, no bins
#define DBG_TILE_CLOCKS 16u   // tile kernel writes its elapsed wall-clock ticks per tile
#define DBG_NO_OUT      128u  // tile kernel skips tile-out and the HZB reduction
#define DBG_NO_HZB      256u  // tile kernel writes the tile but skips the HZB reduction
#define DBG_SETUP_CLOCKS 512u // setup kernel accumulates per-wave phase ticks (header / vertex / triangle / reserve / emit)
#define DBG_NO_VIS_STORE 1024u // fused tile-out skips the visibility stores (HZB texels still written: culling unchanged)
#define DBG_NO_SPLIT    2048u // tile order kernel never cuts a bin into slices
#define DBG_NO_TINY     32u   // tile kernel skips the per-lane scan of tiny triangles
#define DBG_TILE_EXIT   64u   // tile kernel of passes >= 1 returns at once (launch-floor measurement)
#define DBG_NO_ENTRY    8192u // tile kernel fetches bin entries and records but does nothing with them
#define DBG_NO_BATCH    16384u // tile kernel skips the bin altogether (tile in + tile out only)
#define DBG_NO_UNITS    4096u // tile kernel skips the row units (entries are still fetched, set up, scanned and listed)
#define DBG_SKIP_LIGHT  1048576u // tile kernel: work items of tiles with fewer than 64 bin entries end at once (what the light tiles cost the pass)
#define DBG_SKIP_HEAVY  2097152u // ... of tiles with 64 entries or more
#define DBG_NO_BLOCKS 32768u     // small clusters take the record path too (A/B of the pixel blocks; results identical)
#define DBG_FORCE_BLOCKS 65536u  // the setup kernel takes its BLOCKS body whatever the cluster count (tests: small scenes)
#define DBG_FORCE_HOT 262144u    // the block kernel's hot-tile variant whatever the hint says, tiles hot from 64 entries (tests: small scenes)

// ---- tuning constants that the kernels and launch_raster both read ------------------------------
// Hot tiles (the block kernel's reserve of bin slots, kernels_raster_setup.hip): a tile is hot once its bin holds SLOT_HOT entries --
// the value of RasterParams::slotHot outside tests, and the longest bin of the last frame from which launch_raster takes the block
// kernel's hot variant
#define SLOT_HOT 65536u
// The tile schedule (tile_order_part, kernels_raster.hip) and launch_raster's choice of a pass's schedule
#define TILE_SLICE_SHIFT CHORD_TILE_SLICE_SHIFT
#define TILE_SLICE (1u << TILE_SLICE_SHIFT)
#ifndef TILE_SPLIT_MIN
#define TILE_SPLIT_MIN 6144u       // bins up to this many entries stay whole
#endif
#ifndef TILE_ORDER_KEEP
#define TILE_ORDER_KEEP 1          // 0: the schedule kernel runs in every pass whatever chordvis_set_tile_schedule_keep says (A/B builds)
#endif
#ifndef TILE_DIRECT
#define TILE_DIRECT 1              // 0: later passes of a frame keep their schedule kernel (A/B builds)
#endif
#ifndef TILE_DIRECT_MAX_CLUSTERS
#define TILE_DIRECT_MAX_CLUSTERS 1024u   // a later pass with more clusters than this keeps its schedule (config 4's second pass, 30 k clusters in every tile of the screen: +15 % per frame without one)
#endif

// ---- the launches of the two stages (each in the file of its kernels: kernels_raster_setup.hip, kernels_raster.hip; launch_raster calls them in this order) ---------------
// Set-up: the block kernel (blocks; hot: its variant that draws bin slots ahead), then the wide kernel (wide) or the record kernel over
// a list of `capacity` entries, then the clipper and large-record binner of a pass without RasterParams::binInSetup.
void launch_raster_setup(ChordCtx* c, const RasterParams& p, uint32_t capacity, bool masked, bool blocks, bool hot, bool wide);
// Tiles: the schedule kernel (makeOrder), then the tile kernel.  touchedGroups: the workgroups of a pass that takes only touched
// tiles (RasterParams::tileTouched), 0: one per tile slot of the device.
void launch_raster_tiles(ChordCtx* c, const RasterParams& p, bool masked, bool depthClamp, bool makeOrder, uint32_t touchedGroups);

} // namespace chord
