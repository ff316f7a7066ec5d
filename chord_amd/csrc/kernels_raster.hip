// Software rasterizer of the visibility path, hand-written for gfx950 (wave64, LDS tiles).
//
// Replaces meshRasterPassMS + the fixed-function rasterizer + depth test + meshRasterPassPS
// (mesh_raster.hlsl:51-210; state mesh_raster.cpp:141-156, helper.h:7-13,304-324,395-407).
//
// Measured on MI355X (tools/microbench/atomics.hip): a 64-bit global atomicMax costs one L2/fabric
// request per 64-byte line touched — 26 Gop/s when every lane hits its own line (small triangles),
// 214 Gop/s for an 8x8 footprint — while ds_max_u64 in LDS sustains ~1 050 Gop/s and plain coalesced
// stores ~6.6 TB/s.  So fragments are resolved in LDS and the visibility words leave the CU once:
//
//   raster_setup_kernel   one wave per visible meshlet, software-pipelined over the wave's meshlets: coalesced
//                         meshletData / position stream -> clip-space transform -> LDS (SoA x,y,w,u,v,depth) ->
//                         per-triangle culls (mesh_raster.hlsl:143-179) -> snapped setup -> a 32-byte (vertices
//                         at most 64 px apart) or 48-byte triangle record + one bin entry per 64x64 screen tile
//                         touched; every reservation of a meshlet in one memory round trip.  Records touching more than 2x2
//                         tiles are binned by the same wave right after (wave_bin_large), and its clip triangles are clipped
//                         and binned by it once its clusters are done (clip_entry)
//   raster_setup_wide_kernel  light later passes only: the same set-up with one 256-thread workgroup per cluster (a vertex
//                         per thread, a triangle per lane, reservations merged through an LDS tile table)
//   raster_setup_blocks_kernel  dense launches (a cluster per 16 pixels or more: sub-pixel geometry) run this one first: a
//                         cluster that fits a 16x16-pixel window is resolved in LDS and leaves as a pixel block per
//                         touched tile (one bin entry each) instead of a record per triangle; the clusters it cannot
//                         take go to the record kernel through a leftover list.  <true>: bin slots of hot tiles drawn ahead
//   raster_clip_and_bin_large_kernel  only with CHORDVIS_BIN_IN_SETUP=0 (A/B runs): the same clipping and large-record
//                         binning from the lists the setup kernel then writes, one launch
//   raster_tile_order_kernel  work items of the tile kernel (tiles, or slices of tiles with long bins), heaviest first
//   raster_tile_kernel    one 512-thread workgroup per work item: the tile's 4096 packed words live in LDS;
//                         every binned triangle is scan-converted with ds_max_u64 (tiny: one lane per triangle;
//                         others: cut into (triangle, row) units that a block-wide prefix sum deals out one row
//                         per lane, each row a branch-free loop over an fp32-bounded span).  Tile-out: 16-byte
//                         coalesced stores (on the first pass of a frame this is also the clear) fused with the
//                         reduction of the tile to HZB mips 0..5; slices of a split tile meet in a per-tile slab.
// Bins hold 16 384 entries per tile and continue in 1024-entry pool chunks (bin_store).
// The packed word is (asuint(depth) << 32) | ((slot+1)&0xFFFFFF)<<8 | tri: reverse-Z "greater wins"
// and the id in one 64-bit max (GREATER_OR_EQUAL depth test + id write of the reference).
//
// Arithmetic is the canonical restatement of SURVEY.md §8c: snapped 24.8 coordinates, pixel
// centres at +0.5, top-left rule, integer edge functions, depth = (d0 + l1*(d1-d0)) + l2*(d2-d0).
// Integer / fp32 VALU + LDS atomics; no MFMA.  Built with -ffp-contract=off.
//
// THIS file holds the tile stage (raster_tile_order_kernel, raster_tile_kernel), the constants only it reads and its launches; the
// set-up kernels are in kernels_raster_setup.hip, the device helpers both stages use in raster_device.h, what host and device
// share in raster_params.h, launch_raster in raster_launch.cpp.

#include "raster_device.h"

#include <type_traits>

namespace chord {

// ---- tile schedule: heaviest work first ---------------------------------------------------------
// The tile kernel's duration is its slowest work item plus whatever is still queued behind it.  A tile
// whose bin is long is cut into slices of TILE_SLICE entries that different workgroups scan-convert
// concurrently (the last one to finish merges them, see raster_tile_kernel), and items are dispatched
// in descending order of their entry count (longest-processing-time first): one block lists the slices
// of split tiles first and bucket-sorts the other tiles by floor(log2(count)).  Tiles without entries
// come last on the first pass of a frame (they still have to be written: that is the clear) and are
// dropped otherwise.  Item = tile | slice << 12 | (slices - 1) << 22.
// (TILE_SLICE, TILE_SPLIT_MIN, TILE_ORDER_KEEP, TILE_DIRECT and TILE_DIRECT_MAX_CLUSTERS: raster_params.h -- launch_raster reads them too)
#ifndef TILE_SLICE_MIN
#define TILE_SLICE_MIN 1024u       // the shortest slice of a pass that has fewer tiles than the device has slots
#endif
template <uint32_t NT>
__device__ __forceinline__ void tile_order_part(const RasterParams& p, uint2* __restrict__ order)
{
    __shared__ uint32_t hist[20], base[20], cursor[20], splitItems, splitCursor, longest, hotCount, hotList[CHORD_HOT_TILES], entriesAll, tilesBusy;
    const uint32_t tiles = p.tilesX * p.tilesY;
    if (threadIdx.x < 20u) { hist[threadIdx.x] = 0; cursor[threadIdx.x] = 0; }
    if (threadIdx.x == 0) { splitItems = 0; splitCursor = 0; longest = 0; hotCount = 0; entriesAll = 0; tilesBusy = 0; }
    __syncthreads();
    // A tile's word: bin entries (clamped to the capacity) | bit 31: the bin holds pixel blocks (the tile kernel's block pass; it used to
    // ask the counter line itself, a dependent round trip per tile in front of its first bin fetch) | bit 30: the bin holds alpha-tested
    // triangles (TC_MASKED; nothing reads the bit any more -- it told the tile kernel that the deleted masked pass had written the
    // tile -- and a later change can drop it with the flag).  ~0: not a work item of this rank (sharded frames: another rank's tiles --
    // their bins are empty, and the clear pass must not touch them).
    // (Every thread asks for the lines of all its tiles at once and keeps ONE word per tile -- bucket, slices and position are worked out
    // again where they are needed: as a workgroup of the tile kernel this part is out of line and its registers are its own, but three
    // passes of dependent line fetches made it the longest chain of a short launch.)
    auto tile_word = [&](uint32_t t) -> uint32_t {
        if (!owns_tile(p.shard, (int32_t)(t % p.tilesX), (int32_t)(t / p.tilesX))) return 0xFFFFFFFFu;
        const uint32_t* __restrict__ line = &p.tileCount[(size_t)t * TC_STRIDE];
        const uint32_t n = line[0], nb = line[1], nm = line[3];
        return min(n, bin_capacity(p)) | (nb ? 0x80000000u : 0u) | (nm ? 0x40000000u : 0u);
    };
    constexpr uint32_t PER_THREAD = CHORD_MAX_TILES / NT;
    uint32_t mine[PER_THREAD];
#pragma unroll
    for (uint32_t k = 0; k < PER_THREAD; k++) { const uint32_t t = threadIdx.x + k * NT; mine[k] = t < tiles ? tile_word(t) : 0xFFFFFFFFu; }
    uint32_t sumMine = 0, tilesMine = 0;
    if (p.tileSlots) {
        // A pass with fewer non-empty tiles than the device holds tile workgroups (a rank of an 8-rank frame owns 255 tiles of a 4K
        // target, 256 CUs hold 512 workgroups; so does a 1080p target on one GPU) leaves slots idle while every tile is one
        // workgroup's serial work: its bins are cut finer -- into about as many equal shares as there are slots, never shorter than
        // TILE_SLICE_MIN entries (a slice pays for a tile of LDS zeroed and its touched words merged through the slab).
        // The image does not depend on the cut (64-bit max).
        // (a DPP reduction per wave, then one LDS atomic per wave: handed the 1 024 atomics, the compiler's atomic optimizer walks the
        // lanes of every wave in a scalar loop -- measured +6 us on a 4-us kernel)
#pragma unroll
        for (uint32_t k = 0; k < PER_THREAD; k++) {
            const uint32_t w = mine[k];
            if (w != 0xFFFFFFFFu) { const uint32_t c = w & 0x3FFFFFFFu; sumMine += c; tilesMine += c ? 1u : 0u; }
        }
        wave_sum2(sumMine, tilesMine);
        if ((threadIdx.x & 63u) == 0u) { atomicAdd(&entriesAll, sumMine); atomicAdd(&tilesBusy, tilesMine); }
        __syncthreads();
    }
    uint32_t splitMin = p.tileSplitMin, sliceLen = p.tileSliceLen;
    if (p.tileSlots && tilesBusy < p.tileSlots) {
        const uint32_t share = (entriesAll / p.tileSlots + 511u) & ~511u;   // (whole batches of the tile kernel)
        sliceLen = min(p.tileSliceLen, max(TILE_SLICE_MIN, share));
        splitMin = min(p.tileSplitMin, sliceLen + sliceLen / 2u);
    }
    // bucket of a tile: 18 = cut into slices, 4 = 2^11.., 16 = one entry, 17 = empty
    auto slices_of = [&](uint32_t c) -> uint32_t { return (c > splitMin && !ABL(p, DBG_NO_SPLIT)) ? min((c + sliceLen - 1u) / sliceLen, CHORD_TILE_MAX_SLICES) : 0u; };
#pragma unroll
    for (uint32_t k = 0; k < PER_THREAD; k++) {
        const uint32_t t = threadIdx.x + k * NT, w = mine[k];
        if (w == 0xFFFFFFFFu) continue;
        const uint32_t c = w & 0x3FFFFFFFu;
        // a bin this long is a hot tile: the next frame's block kernel draws its slots ahead from the first cluster on (hotTiles)
        if (c >= p.slotHot && p.hotTiles) { const uint32_t h = atomicAdd(&hotCount, 1u); if (h < CHORD_HOT_TILES) hotList[h] = t | (c >= SLOT_VERY_HOT ? 0x80000000u : 0u); }
        const uint32_t sl = slices_of(c);
        if (sl) {
            atomicAdd(&splitItems, sl);
            if (c > TILE_SPLIT_MIN) atomicMax(&longest, c);   // (the host's hint keeps its meaning: bins that a full launch would keep whole report 0)
        } else atomicAdd(&hist[c ? 16u - (31u - (uint32_t)__clz(c)) : 17u], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t acc = splitItems;
        for (int b = 0; b < 18; b++) { base[b] = acc; acc += hist[b]; }
        order[0] = make_uint2((p.clearTiles || p.orderAll) ? acc : acc - hist[17], 0u);
        if (p.binHint) *p.binHint = longest;                      // (bins short enough to stay whole report 0)
        if (p.heavyHint) p.heavyHint[(splitItems != 0u || *p.count > TILE_DIRECT_MAX_CLUSTERS) ? 0 : 2] = p.binStamp;   // (launch_raster TILE_DIRECT: heavy / light)
        if (p.countHint) *p.countHint = *p.count;
        if (p.hotTiles) p.hotTiles[0] = min(hotCount, (uint32_t)CHORD_HOT_TILES);
    }
    if (p.hotTiles && threadIdx.x < min(hotCount, (uint32_t)CHORD_HOT_TILES)) p.hotTiles[1u + threadIdx.x] = hotList[threadIdx.x];
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < PER_THREAD; k++) {
        const uint32_t t = threadIdx.x + k * NT, w = mine[k];
        if (w == 0xFFFFFFFFu) continue;
        const uint32_t c = w & 0x3FFFFFFFu, sl = slices_of(c);
        if (sl) {
            const uint32_t pos = atomicAdd(&splitCursor, sl);       // (the slices of a tile side by side, the split tiles in any order: all of them start the pass)
            for (uint32_t j = 0; j < sl; j++) order[1u + pos + j] = make_uint2(t | (j << 12) | ((sl - 1u) << 22), w);
        } else {
            const uint32_t b = c ? 16u - (31u - (uint32_t)__clz(c)) : 17u;
            order[1u + base[b] + atomicAdd(&cursor[b], 1u)] = make_uint2(t, w);   // the count rides along: one round trip less per tile
        }
    }
}

// The same part as ONE workgroup of the tile kernel (raster_tile_kernel, workgroup 0 of a launch with tileOrderNext): out of line,
// and reading the launch's arguments from the kernel-argument segment itself -- inlined, its scalars cost the tile kernel twelve
// spill slots (48 bytes of scratch in a kernel that has none).  (The KERNEL asks for the segment's address and hands it over: in a
// function that is not a kernel the compiler folds __builtin_amdgcn_kernarg_segment_ptr() to null -- every load of this part faulted.)
__device__ __noinline__ void tile_order_next_part(const RasterParams* q)
{
    tile_order_part<512u>(*q, q->tileOrderNext);
}

// (Ordering in the last workgroup of the binning launch was measured twice: with that launch's 1 088 workgroups the ticket
// alone costs 11 us; with the launch cut to 128 workgroups the merged kernel still takes 1.5 us longer per pass than these
// two -- the orderer must read the 2 040 counters with agent-scope loads, past its L2, after a ticket round trip.)
__global__ __launch_bounds__(1024) void raster_tile_order_kernel(RasterParams p)
{
    tile_order_part<1024u>(p, p.tileOrder);
}

// (Tried in round 2: clipper + large-record binning + this schedule in ONE launch of 128 workgroups, the last one --
// found by a ticket -- ordering the tiles with 256 threads: 11.5 us against 5 + 5 us for the two launches.  A kernel
// boundary costs 2.5 us on this GPU (tools/microbench/launch_floor); the rest of each 5 us is the dependent-load chain
// of a kernel with next to nothing to do, which merging does not remove.)

// ---- row units ------------------------------------------------------------------------------
// Triangles are not equal: a tile may hold thousands of 1-pixel triangles or a few that cover it
// completely.  Each batch of 512 bin entries is therefore cut into (triangle, pixel row) units; a
// block-wide prefix sum over the row counts hands every thread one row at a time, so a lane's loop
// length is one row span (<= 64 pixels) instead of one bbox area (<= 4096).  Tiny triangles (clipped
// bbox <= TINY_AREA / TINY_AREA_DENSE pixels) are scanned directly by the thread that set them up.
//
// Edge functions in the row loop are incremental (no multiplies).  Three exact representations:
//   kind 0  int32   vertices at most 64 px apart (|E| < 2^30)
//   kind 1  double  |coordinates| < 2^25 sub-pixels: every product and sum below 2^53, so fp64 is exact
//                   and v_cvt_f32_f64 IS the canonical (float)(double)E
//   kind 2  int64   anything else (guard-band monsters)
//   kind 3  a masked (alpha-tested) triangle: int32 or int64 by its extent (masked_rows)
// The threshold follows the tile: where a bin is long (>= TINY_DENSE_MIN entries: distant instances, a triangle or two per
// pixel) nearly everything is small and a lane's own loop of up to 48 pixels beats a unit list that is mostly one- and two-row
// triangles; where it is short the triangles are larger and more varied, and 8 keeps the lanes of a wave alike.  Measured
// (one threshold 8 / 16 / 32: config 3 0.1882 / 0.1897 / 0.1932 ms, config 4 0.443 / 0.429 / 0.419; 8 | 48 at 1 024 entries:
// 0.1875 and 0.4194).
#ifndef TINY_AREA
#define TINY_AREA 8
#endif
#ifndef TINY_AREA_DENSE
#define TINY_AREA_DENSE 48
#endif
#ifndef TINY_DENSE_MIN
#define TINY_DENSE_MIN 1024u
#endif

struct UnitParams {           // one batch entry, as the row loop wants it
    int32_t X[3], Y[3];
    float d0, e1, e2, invA;
    uint32_t payload;
    int32_t skind;            // s in bit 0 (1 = negative), kind << 1
};
#define TB 512                  // threads per tile workgroup = entries per batch
static_assert(TB == 512, "tile_order_part rounds a pass's slice length to batches of 512");
#define UNIT_CAP 4096           // units per round of a batch

// steps k0 .. k1 of a row loop that contain every covered step (span_bounds.h), with the device's reciprocal
__device__ __forceinline__ void row_span(float e0, float e1, float e2, float t0, float t1, float t2, int32_t n, int32_t& k0, int32_t& k1)
{
    const float e[3] = {e0, e1, e2}, t[3] = {t0, t1, t2};
    span_bounds(e, t, n, [](float x) { return __builtin_amdgcn_rcpf(x); }, k0, k1);
}

template <typename E_t>
__device__ __forceinline__ void scan_row(unsigned long long* __restrict__ tileRow, const UnitParams& u, int32_t ox, int32_t py,
                                         int32_t lx0, int32_t lx1, bool noPixels, const bool clampZ)
{
    const E_t s = (u.skind & 1) ? (E_t)-1 : (E_t)1;
    const E_t dx0 = (E_t)(u.X[2] - u.X[1]), dy0 = (E_t)(u.Y[2] - u.Y[1]);
    const E_t dx1 = (E_t)(u.X[0] - u.X[2]), dy1 = (E_t)(u.Y[0] - u.Y[2]);
    const E_t dx2 = (E_t)(u.X[1] - u.X[0]), dy2 = (E_t)(u.Y[1] - u.Y[0]);
    const E_t a0 = -s * dy0, b0 = s * dx0, a1 = -s * dy1, b1 = s * dx1, a2 = -s * dy2, b2 = s * dx2;
    const E_t bias0 = (a0 > 0 || (a0 == 0 && b0 > 0)) ? (E_t)0 : (E_t)-1;
    const E_t bias1 = (a1 > 0 || (a1 == 0 && b1 > 0)) ? (E_t)0 : (E_t)-1;
    const E_t bias2 = (a2 > 0 || (a2 == 0 && b2 > 0)) ? (E_t)0 : (E_t)-1;
    const E_t cx = (E_t)(ox + lx0) * (E_t)256 + (E_t)128, cy = (E_t)py * (E_t)256 + (E_t)128;
    E_t E0 = s * (dx0 * (cy - (E_t)u.Y[1]) - dy0 * (cx - (E_t)u.X[1])) + bias0;     // bias folded in: inside <=> all >= 0
    E_t E1 = s * (dx1 * (cy - (E_t)u.Y[2]) - dy1 * (cx - (E_t)u.X[2])) + bias1;
    E_t E2 = s * (dx2 * (cy - (E_t)u.Y[0]) - dy2 * (cx - (E_t)u.X[0])) + bias2;
    const E_t st0 = a0 * (E_t)256, st1 = a1 * (E_t)256, st2 = a2 * (E_t)256;
    // Span of the row in steps k from lx0: E_i + k * st_i >= 0 for all i.  The crossings are estimated in fp32
    // (v_rcp_f32; span_bounds.h has the error bound and the 2^-6 px it is cleared by) and only bound
    // the loop; coverage itself is decided by the exact edge values inside it, so the loop has no data-dependent
    // branch: a pixel outside merges the value 0, which ds_max ignores.
    int32_t k0, k1;
    row_span((float)E0, (float)E1, (float)E2, (float)st0, (float)st1, (float)st2, lx1 - lx0, k0, k1);
    E0 += (E_t)k0 * st0; E1 += (E_t)k0 * st1; E2 += (E_t)k0 * st2;
    unsigned long long* px = tileRow + lx0 + k0;
    const unsigned long long payload = noPixels ? 0ull : (unsigned long long)u.payload;
    for (int32_t k = k0; k <= k1; k++) {
        const bool inside = std::is_floating_point<E_t>::value ? (E0 >= (E_t)0 && E1 >= (E_t)0 && E2 >= (E_t)0)
                                                              : (((int64_t)E0 | (int64_t)E1 | (int64_t)E2) >= 0);
        // canonical l_i = float(E_i) * invA with E_i the unbiased integer
        const float l1 = (float)(double)(E1 - bias1) * u.invA, l2 = (float)(double)(E2 - bias2) * u.invA;
        float z = (u.d0 + l1 * u.e1) + l2 * u.e2;
        if (clampZ) z = fminf(fmaxf(z, 0.0f), 1.0f);
        const unsigned long long packed = ((unsigned long long)__float_as_uint(z) << 32) | payload;
        atomicMax(px, inside && !noPixels ? packed : 0ull);      // ds_max_u64
        E0 += st0; E1 += st1; E2 += st2; px++;
    }
}

// exclusive scan of one value per thread over the TB-thread block
__device__ __forceinline__ uint32_t block_scan_tb(uint32_t v, uint32_t* waveSums, uint32_t* total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t nb = __shfl_up(incl, d, 64);
        if (lane >= (uint32_t)d) incl += nb;
    }
    if (lane == 63u) waveSums[wave] = incl;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < TB / 64u; w++) { const uint32_t sw = waveSums[w]; if (w < wave) base += sw; tot += sw; }
    *total = tot;
    return base + incl - v;
}


// ---- batch entries with pre-computed edge constants ---------------------------------------------------------------
// The thread that fetches a bin entry also reduces it to what a pixel row needs, ONCE: for triangles whose vertices are
// at most 64 px apart (nearly all) the three edge functions as  E_i(lx, ly) = C_i + ((a_i * lx + b_i * ly) << 8)  with
// C_i the (top-left-biased) value at the tile's origin pixel and a_i, b_i the 16-bit pixel steps / 256 -- a row unit
// then costs two multiply-adds per edge instead of re-deriving deltas, orientation, biases and the 24.8 products
// (about 50 of the ~135 instructions a unit spent before its first pixel).  All values are exact 32-bit integers:
// |a|, |b| <= 2^14 and a pixel of the tile is at most 2^15 + 128 sub-pixels from a vertex, so |E| < 2^31.
// Wide triangles (kind 1: fp64 edges, kind 2: int64) keep their vertices and derive the edges per unit as before.
// A unit is one pixel row of one entry, of opaque and of masked (alpha-tested) triangles alike.  The unit word, the listing and the
// decode keep a segment of SEG pixels of the row (SEG_SHIFT, MASKED_SEG_SHIFT); SEG is the tile's width, so a row is ONE segment and
// the segment ALWAYS 0: where an entry's units are listed the count is the constant 1, not arithmetic on the box word.
#ifndef SEG_SHIFT
#define SEG_SHIFT 6             // 64: one unit per row
#endif
#define SEG (1 << SEG_SHIFT)
#ifndef MASKED_SEG_SHIFT
#define MASKED_SEG_SHIFT 6
#endif
#define MASKED_SEG (1 << MASKED_SEG_SHIFT)
// A batch is TB bin entries, one per thread, and a round of its unit list UNIT_CAP units: 26 + 16 KB of LDS beside the 33-KB tile = two
// workgroups per CU.
// Measured and rejected; the code of each is in the history at commit bb3c4eb:
//  * rows cut into segments of 16 / 32 pixels, one unit each (-DSEG_SHIFT=4 / 5): 3 % / 1 % slower on config 3, more units for the same
//    trips (round 3); masked segments of 32 / 16 / 8 px: tile kernel 419 / 421 / 498 us against 418 on street_4k_masked
//    (profiles/r04_masked_variants.txt).
//  * the segment count worked out from the box word where units are listed (-DUNIT_NSEG_CONST=0): a compare and two selects per trip
//    of a serial loop, 3 % of the flagship frame (profiles/r11_row_units.txt).
//  * units of 16 rows of a masked triangle (-DMASKED_ROWS=16), its set-up paid once per group: 1 012 us against 418; two pixels per
//    trip 488: the masked instantiations sit at 128 VGPRs, more live taps move spills into the loop (profiles/r04_masked_variants.txt).
//  * an entry's three step reciprocals made once by entry_store, in three more entry words beside a 16-bit unit list (-DENTRY_RCP=1):
//    bit-exact and 0.4 % of the flagship frame, but one masked instantiation spills a register (profiles/r11_row_units.txt).
//  * three workgroups per CU, batches of 256 entries and rounds of 1 536 units at 80 VGPRs (-DTILE_BATCH=256 -DTILE_UNIT_CAP=1536
//    -DTILE_MIN_BLOCKS=6): +5 % on config 3, +26 % on config 4, +71 % masked (profiles/r05_tile_kernel_experiments.txt).
//  * the masked pass with parts removed, to see what each costs (-DEXP_MASKED, results differ): of its ~250 us the bilinear taps are 80,
//    the remainders of non-power-of-two sizes were 45 (period_mod recovered 30), the two divisions 5 (profiles/r04_masked_variants.txt).
#define ENTRY_WORDS 13            // word 12: record index of a masked triangle (its extension follows it)
struct EntrySoA { uint32_t w[ENTRY_WORDS][TB]; };
#define EF_KIND_SHIFT 24          // box word: x0 | y0 << 6 | x1 << 12 | y1 << 18 | kind << 24 | bias1 << 26 | bias2 << 27 | sneg << 28

// One row of an entry with stored edge constants (kind 0), two pixels per trip; returns the loop's steps.  The int32 form of scan_row:
// the canonical (float)(double)E is (float)E for |E| < 2^31, one instruction instead of two.
// Span of the row in steps k from lx0 (see scan_row): fp32 estimates only BOUND the loop, coverage is exact inside.
__device__ __forceinline__ int32_t scan_span_i32(unsigned long long* __restrict__ tileRow, int32_t E0, int32_t E1, int32_t E2,
                                              int32_t st0, int32_t st1, int32_t st2, int32_t bias1, int32_t bias2,
                                              float d0, float e1, float e2, float invA, uint32_t payloadIn,
                                              int32_t lx0, int32_t lx1, bool noPixels, const bool clampZ)
{
    int32_t k0, k1;
    row_span((float)E0, (float)E1, (float)E2, (float)st0, (float)st1, (float)st2, lx1 - lx0, k0, k1);
    E0 += __mul24(k0, st0); E1 += __mul24(k0, st1); E2 += __mul24(k0, st2);     // |st| <= 2^22, 0 <= k0 <= 2^12: 24-bit operands
    // (Round 3: trimming the ~3 slack pixels that the bounds then had (floor(q) -+ 1) with exact edge tests before the loop --
    // 1.5 of a row's 5.6 two-pixel trips -- and predicating the merges instead of merging 0 were both measured: tile kernel
    // 107 -> 109 / 108 us on config 3, 197 -> 200 / 197 on config 4; profiles/r03_tile_kernel_experiments.txt.  The bounds of
    // span_bounds.h take most of that slack for no instruction; profiles/r10_span_bounds.txt.)
    int32_t U1 = E1 - bias1, U2 = E2 - bias2;                    // the unbiased values the canonical depth uses
    unsigned long long* px = tileRow + lx0 + k0;
    const unsigned long long payload = noPixels ? 0ull : (unsigned long long)payloadIn;
    const int32_t kFirst = k0;
    // two pixels per trip.  The second may lie one past the bound: coverage is decided by the exact edge values, and
    // the word it would touch is at most the row's padding word (lx1 <= 63), a pixel right of the screen or a pixel of
    // the next segment of the same row (which merges the same value) -- never another row.
    // (Round 11: the two pixels' l1, l2 and z as two-element vectors -- four v_pk_mul_f32 and two v_pk_add_f32 for the twelve scalar
    // multiplies and adds, -4.4 % of the first pass's VALU instructions -- was timed and left the frame 0.6 % slower: a packed
    // instruction issues at 2.7 cycles against 1.6 at four waves per SIMD; profiles/r11_row_units.txt.  Not kept, not even as a switch.)
    for (int32_t k = k0; k <= k1; k += 2) {
        const bool insideA = (E0 | E1 | E2) >= 0;
        const bool insideB = ((E0 + st0) | (E1 + st1) | (E2 + st2)) >= 0;
        const float l1a = (float)U1 * invA, l2a = (float)U2 * invA;   // (float)(double)E == (float)E: one rounding of an exact integer
        const float l1b = (float)(U1 + st1) * invA, l2b = (float)(U2 + st2) * invA;
        float za = (d0 + l1a * e1) + l2a * e2;
        float zb = (d0 + l1b * e1) + l2b * e2;
        if (clampZ) { za = fminf(fmaxf(za, 0.0f), 1.0f); zb = fminf(fmaxf(zb, 0.0f), 1.0f); }
        atomicMax(px, insideA && !noPixels ? (((unsigned long long)__float_as_uint(za) << 32) | payload) : 0ull);      // ds_max_u64
        atomicMax(px + 1, insideB && !noPixels ? (((unsigned long long)__float_as_uint(zb) << 32) | payload) : 0ull);
        E0 += 2 * st0; E1 += 2 * st1; E2 += 2 * st2; U1 += 2 * st1; U2 += 2 * st2; px += 2;
    }
    return max(k1 - kFirst + 1, 0);
}

// entry record of a triangle that needs row units; returns its unit count
__device__ __forceinline__ uint32_t entry_store(EntrySoA& en, uint32_t t, const TriSetup& ts, bool narrow,
                                                int32_t ox, int32_t oy, int32_t x0, int32_t y0, int32_t x1, int32_t y1,
                                                bool masked = false, uint32_t recIndex = 0u)
{
    const bool maskedNarrow = masked && narrow;                   // (bit 29 of the box word: masked_rows may use 32-bit edge functions)
    narrow = narrow && !masked;                                   // masked triangles keep their vertices (kind 3)
    uint32_t box = (uint32_t)(x0 - ox) | ((uint32_t)(y0 - oy) << 6) | ((uint32_t)(x1 - ox) << 12) | ((uint32_t)(y1 - oy) << 18);
    if (narrow) {
        const int32_t s = ts.s;
        const int32_t dx0 = ts.X[2] - ts.X[1], dy0 = ts.Y[2] - ts.Y[1];
        const int32_t dx1 = ts.X[0] - ts.X[2], dy1 = ts.Y[0] - ts.Y[2];
        const int32_t dx2 = ts.X[1] - ts.X[0], dy2 = ts.Y[1] - ts.Y[0];
        const int32_t a0 = -s * dy0, b0 = s * dx0, a1 = -s * dy1, b1 = s * dx1, a2 = -s * dy2, b2 = s * dx2;
        const int32_t bias0 = (a0 > 0 || (a0 == 0 && b0 > 0)) ? 0 : -1;
        const int32_t bias1 = (a1 > 0 || (a1 == 0 && b1 > 0)) ? 0 : -1;
        const int32_t bias2 = (a2 > 0 || (a2 == 0 && b2 > 0)) ? 0 : -1;
        const int32_t cx = ox * 256 + 128, cy = oy * 256 + 128;
        en.w[0][t] = ((uint32_t)a0 & 0xFFFFu) | ((uint32_t)b0 << 16);
        en.w[1][t] = ((uint32_t)a1 & 0xFFFFu) | ((uint32_t)b1 << 16);
        en.w[2][t] = ((uint32_t)a2 & 0xFFFFu) | ((uint32_t)b2 << 16);
        // |deltas| <= 2^14 and the tile origin is at most 2^15 + 128 sub-pixels from a vertex: 24-bit operands, |E| < 2^31
        en.w[3][t] = (uint32_t)(s * (__mul24(dx0, cy - ts.Y[1]) - __mul24(dy0, cx - ts.X[1])) + bias0);
        en.w[4][t] = (uint32_t)(s * (__mul24(dx1, cy - ts.Y[2]) - __mul24(dy1, cx - ts.X[2])) + bias1);
        en.w[5][t] = (uint32_t)(s * (__mul24(dx2, cy - ts.Y[0]) - __mul24(dy2, cx - ts.X[0])) + bias2);
        box |= (bias1 ? 1u << 26 : 0u) | (bias2 ? 1u << 27 : 0u);
    } else {
        int32_t mag = 0;
#pragma unroll
        for (int i = 0; i < 3; i++) mag = max(mag, max(abs(ts.X[i]), abs(ts.Y[i])));
        en.w[0][t] = (uint32_t)ts.X[0]; en.w[1][t] = (uint32_t)ts.X[1]; en.w[2][t] = (uint32_t)ts.X[2];
        en.w[3][t] = (uint32_t)ts.Y[0]; en.w[4][t] = (uint32_t)ts.Y[1]; en.w[5][t] = (uint32_t)ts.Y[2];
        box |= (masked ? 3u : (mag < (1 << 25) ? 1u : 2u)) << EF_KIND_SHIFT;
        box |= ts.s < 0 ? 1u << 28 : 0u;
        box |= maskedNarrow ? 1u << 29 : 0u;
        if (masked) en.w[12][t] = recIndex;
    }
    en.w[6][t] = __float_as_uint(ts.d0); en.w[7][t] = __float_as_uint(ts.e1); en.w[8][t] = __float_as_uint(ts.e2);
    en.w[9][t] = __float_as_uint(ts.invA); en.w[10][t] = ts.payload; en.w[11][t] = box;
    // units: one per (row, segment)
    if (masked) return ((uint32_t)(y1 - y0) + 1u) * ((uint32_t)((x1 - x0) >> MASKED_SEG_SHIFT) + 1u);
    return (uint32_t)(y1 - y0 + 1) * ((uint32_t)((x1 - x0) >> SEG_SHIFT) + 1u);
}

// The pixel rows of one unit of a masked triangle: exact integer edges, canonical depth, and per covered pixel the perspective-correct
// texture coordinates, one alpha fetch and the clip() of mesh_raster.hlsl:198-204.
// E_t: int32_t for triangles whose vertices are at most 64 px apart (|E| < 2^31, as in scan_span_i32; (float)E is then the
// canonical (float)(double)E), int64_t for the rest.  The span of a row is bounded first (row_span, the same bounds as
// scan_row's), so the loop runs over the covered pixels, not over the bbox row; a step outside the triangle skips the taps.
// A unit is ONE row: every caller passes nrows = 1 (units of 16 rows were measured and rejected, see above), and what a unit pays
// before its first pixel -- the triangle's extension record, its texture level, the edge set-up -- it pays per row.  The row loop and
// the per-row steps sy0 .. sy2 are dead at one row and their spelling is deliberate: the compiler removes them, but not before they
// have shaped the code -- with b_i used a second time it writes the top-left rule of the biases as selects, without it as a branch,
// and the three masked instantiations come out differently (profiles/r12_row_unit_cleanup.txt).  The same holds for the edge set-up
// that this function repeats from scan_row: moved into one function, all six instantiations change.  Both are instruction-stream
// changes for a pull request that measures them.
template <typename E_t>
__device__ __forceinline__ void masked_rows(const RasterParams& p, unsigned long long* __restrict__ tileRow0, const UnitParams& u, uint32_t recIndex,
                                            int32_t ox, int32_t py0, int32_t nrows, int32_t lx0, int32_t lx1, bool noPixels, const bool clampZ)
{
    // (60 bytes of the extension, one round trip: nothing here depends on another fetch)
    const TriRecMaskExt ext = *reinterpret_cast<const TriRecMaskExt*>(&p.tris[recIndex + 1u]);
    struct { float alphaFactor, alphaCutOff; } m = {ext.alphaFactor, ext.alphaCutOff};
    const AlphaLevel tex = alpha_level(p.texAlpha, ext);
    const E_t sgn = (u.skind & 1) ? (E_t)-1 : (E_t)1;
    const E_t dx0 = (E_t)(u.X[2] - u.X[1]), dy0 = (E_t)(u.Y[2] - u.Y[1]);
    const E_t dx1 = (E_t)(u.X[0] - u.X[2]), dy1 = (E_t)(u.Y[0] - u.Y[2]);
    const E_t dx2 = (E_t)(u.X[1] - u.X[0]), dy2 = (E_t)(u.Y[1] - u.Y[0]);
    const E_t a0 = -sgn * dy0, b0 = sgn * dx0, a1 = -sgn * dy1, b1 = sgn * dx1, a2 = -sgn * dy2, b2 = sgn * dx2;
    const E_t bias0 = (a0 > 0 || (a0 == 0 && b0 > 0)) ? (E_t)0 : (E_t)-1;
    const E_t bias1 = (a1 > 0 || (a1 == 0 && b1 > 0)) ? (E_t)0 : (E_t)-1;
    const E_t bias2 = (a2 > 0 || (a2 == 0 && b2 > 0)) ? (E_t)0 : (E_t)-1;
    const E_t cx = (E_t)(ox + lx0) * (E_t)256 + (E_t)128, cy = (E_t)py0 * (E_t)256 + (E_t)128;
    E_t R0 = sgn * (dx0 * (cy - (E_t)u.Y[1]) - dy0 * (cx - (E_t)u.X[1])) + bias0;       // bias folded in: inside <=> all >= 0
    E_t R1 = sgn * (dx1 * (cy - (E_t)u.Y[2]) - dy1 * (cx - (E_t)u.X[2])) + bias1;
    E_t R2 = sgn * (dx2 * (cy - (E_t)u.Y[0]) - dy2 * (cx - (E_t)u.X[0])) + bias2;
    const E_t st0 = a0 * (E_t)256, st1 = a1 * (E_t)256, st2 = a2 * (E_t)256;
    const E_t sy0 = b0 * (E_t)256, sy1 = b1 * (E_t)256, sy2 = b2 * (E_t)256;           // one row down
    for (int32_t r = 0; r < nrows; r++, R0 += sy0, R1 += sy1, R2 += sy2) {
        E_t E0 = R0, E1 = R1, E2 = R2;
        unsigned long long* __restrict__ tileRow = tileRow0 + r * TPITCH;
        int32_t k0, k1;
        row_span((float)E0, (float)E1, (float)E2, (float)st0, (float)st1, (float)st2, lx1 - lx0, k0, k1);
        E0 += (E_t)k0 * st0; E1 += (E_t)k0 * st1; E2 += (E_t)k0 * st2;
        // the packed word of the pixel with these (biased) edge values, 0 when it is outside or its alpha fails the cut-off.  No branch:
        // a pixel outside the triangle evaluates its texture coordinates anyway (whatever they are, texel_floor / wrap_index give an
        // index inside the level), so that the taps of both pixels of a trip are in flight together -- the loop is bound by the latency
        // of its dependent byte loads, one round trip per covered pixel before.
        auto pixel = [&](E_t e0, E_t e1, E_t e2) -> unsigned long long {
            const bool inside = (e0 | e1 | e2) >= 0;
            const float l1 = std::is_same<E_t, int32_t>::value ? (float)(e1 - bias1) * u.invA : (float)(double)(e1 - bias1) * u.invA;
            const float l2 = std::is_same<E_t, int32_t>::value ? (float)(e2 - bias2) * u.invA : (float)(double)(e2 - bias2) * u.invA;
            const float l0 = (1.0f - l1) - l2;
            const float den = (l0 * ext.iw[0] + l1 * ext.iw[1]) + l2 * ext.iw[2];
            float tu = (l0 * ext.uw[0] + l1 * ext.uw[1]) + l2 * ext.uw[2];
            float tv = (l0 * ext.vw[0] + l1 * ext.vw[1]) + l2 * ext.vw[2];
            tu = tu / den; tv = tv / den;
            const float alpha = sample_alpha(tex, tu, tv);
            const bool keep = inside && !(alpha * m.alphaFactor - m.alphaCutOff < 0.0f) && !noPixels;      // clip()
            float z = (u.d0 + l1 * u.e1) + l2 * u.e2;
            if (clampZ) z = fminf(fmaxf(z, 0.0f), 1.0f);
            return keep ? (((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)u.payload) : 0ull;
        };
        unsigned long long* px = tileRow + lx0 + k0;
        for (int32_t k = k0; k <= k1; k++, E0 += st0, E1 += st1, E2 += st2, px++) {
            if ((E0 | E1 | E2) < 0) continue;
            atomicMax(px, pixel(E0, E1, E2));                                         // ds_max_u64 (0 changes nothing)
        }
    }
}

// one unit = (entry e, its j-th (row, segment))
template <bool DEPTH>
__device__ __forceinline__ int32_t entry_unit(const EntrySoA& en, unsigned long long* tile, uint32_t e, uint32_t row, uint32_t seg,
                                           int32_t ox, int32_t oy, bool noPixels)
{
    const uint32_t box = en.w[11][e];
    const int32_t bx0 = (int32_t)(box & 63u), bx1 = (int32_t)((box >> 12) & 63u);
    const int32_t ly = (int32_t)row;
    // (seg is always 0 -- SEG is the tile's width -- and the compiler cannot know it: it comes out of LDS.  The arithmetic stays: with
    // the unit word (entry | row << 9), lx0 = bx0 and lx1 = bx1 the opaque instantiations hold 103 / 104 / 103 VGPRs for 105 / 106 /
    // 105 and the file is shorter, but street_x64_4k_hzb ran 0.3 % SLOWER than the library of commit bb3c4eb in seven of eight interleaved
    // pairs, 0.3837 against 0.3824 ms, tile kernel 168.4 against 167.0 us; profiles/r12_row_unit_cleanup.txt)
    const int32_t lx0 = bx0 + (int32_t)(seg << SEG_SHIFT), lx1 = min(bx1, lx0 + SEG - 1);
    unsigned long long* tileRow = tile + ly * TPITCH;
    const float d0 = __uint_as_float(en.w[6][e]), e1 = __uint_as_float(en.w[7][e]), e2 = __uint_as_float(en.w[8][e]);
    const float invA = __uint_as_float(en.w[9][e]);
    const uint32_t payload = en.w[10][e];
    const uint32_t kind = (box >> EF_KIND_SHIFT) & 3u;
    if (kind == 0u) {
        const uint32_t p0 = en.w[0][e], p1 = en.w[1][e], p2 = en.w[2][e];
        const int32_t a0 = (int32_t)(int16_t)(p0 & 0xFFFFu), b0 = (int32_t)p0 >> 16;
        const int32_t a1 = (int32_t)(int16_t)(p1 & 0xFFFFu), b1 = (int32_t)p1 >> 16;
        const int32_t a2 = (int32_t)(int16_t)(p2 & 0xFFFFu), b2 = (int32_t)p2 >> 16;
        // (16-bit steps times 6-bit pixel offsets: full-rate 24-bit multiplies)
        const int32_t E0 = (int32_t)en.w[3][e] + (__mul24(a0, lx0) + __mul24(b0, ly)) * 256;
        const int32_t E1 = (int32_t)en.w[4][e] + (__mul24(a1, lx0) + __mul24(b1, ly)) * 256;
        const int32_t E2 = (int32_t)en.w[5][e] + (__mul24(a2, lx0) + __mul24(b2, ly)) * 256;
        return scan_span_i32(tileRow, E0, E1, E2, a0 * 256, a1 * 256, a2 * 256, (box >> 26) & 1u ? -1 : 0, (box >> 27) & 1u ? -1 : 0,
                             d0, e1, e2, invA, payload, lx0, lx1, noPixels, DEPTH);
    } else {
        UnitParams u;
        u.X[0] = (int32_t)en.w[0][e]; u.X[1] = (int32_t)en.w[1][e]; u.X[2] = (int32_t)en.w[2][e];
        u.Y[0] = (int32_t)en.w[3][e]; u.Y[1] = (int32_t)en.w[4][e]; u.Y[2] = (int32_t)en.w[5][e];
        u.d0 = d0; u.e1 = e1; u.e2 = e2; u.invA = invA; u.payload = payload;
        u.skind = (int32_t)((box >> 28) & 1u) | (int32_t)(kind << 1);
        if (kind == 1u)      scan_row<double>(tileRow, u, ox, oy + ly, lx0, lx1, noPixels, DEPTH);
        else if (kind == 2u) scan_row<int64_t>(tileRow, u, ox, oy + ly, lx0, lx1, noPixels, DEPTH);
        // (kind 3, a masked triangle: entry_unit_masked, in a pass of its own over the round's units)
        return lx1 - lx0 + 1;
    }
}

// The units of alpha-tested triangles (kind 3) are listed and scanned apart from the others (the block-wide scan counts both
// kinds): the texture fetch of masked_rows (level offsets, wrap modes, four taps, two divisions per pixel) inlined into the loop
// above put every masked instantiation of the tile kernel 37-54 VGPRs past its 128 -- 144-224 bytes of scratch per lane that
// every unit of every triangle paid for, masked or not -- and in a list of their own the masked units fill whole waves instead
// of a lane here and there.  A batch without masked entries skips the pass.
template <bool DEPTH>
__device__ __forceinline__ void entry_unit_masked(const RasterParams& p, const EntrySoA& en, unsigned long long* tile, uint32_t e, uint32_t row, uint32_t seg,
                                                  int32_t ox, int32_t oy, bool noPixels)
{
    const uint32_t box = en.w[11][e];
    const int32_t bx0 = (int32_t)(box & 63u), bx1 = (int32_t)((box >> 12) & 63u);
    const int32_t ly = (int32_t)row;
    const int32_t lx0 = bx0 + (int32_t)(seg << MASKED_SEG_SHIFT), lx1 = min(bx1, lx0 + MASKED_SEG - 1);   // (seg: always 0, see entry_unit)
    UnitParams u;
    u.X[0] = (int32_t)en.w[0][e]; u.X[1] = (int32_t)en.w[1][e]; u.X[2] = (int32_t)en.w[2][e];
    u.Y[0] = (int32_t)en.w[3][e]; u.Y[1] = (int32_t)en.w[4][e]; u.Y[2] = (int32_t)en.w[5][e];
    u.d0 = __uint_as_float(en.w[6][e]); u.e1 = __uint_as_float(en.w[7][e]); u.e2 = __uint_as_float(en.w[8][e]);
    u.invA = __uint_as_float(en.w[9][e]); u.payload = en.w[10][e];
    u.skind = (int32_t)((box >> 28) & 1u) | (3 << 1);
    if ((box >> 29) & 1u) masked_rows<int32_t>(p, tile + ly * TPITCH, u, en.w[12][e], ox, oy + ly, 1, lx0, lx1, noPixels, DEPTH);   // vertices at most 64 px apart
    else                  masked_rows<int64_t>(p, tile + ly * TPITCH, u, en.w[12][e], ox, oy + ly, 1, lx0, lx1, noPixels, DEPTH);
}

// Tile-out of a finished tile fused with its HZB reduction (single-GPU frames): every word goes to the visibility
// buffer once (16-byte coalesced stores) and, from the same LDS reads, the tile is reduced to the HZB texels it owns
// -- mips 0..5 = 32x32 ... 1x1 -- exactly as hzb_mip0_kernel + hzb_mips_kernel would from memory (edge-clamped
// source, binary16 RNE, +1 ulp on the max chain at mip 5, hzb.hlsl:67-71), plus the tile's valid-depth range.
// Wave w owns pixel rows 8w..8w+7: lanes 0-31 read two pixels of an even row, lanes 32-63 of the odd row below, so a
// mip-0 texel is one cross-half shuffle away, mips 1-2 are shuffles + the running rows of the wave, and only mips
// 3-5 (8x8 values per tile) cross waves through LDS: one barrier per tile.
// INTERIOR: every HZB texel of the tile, at every level, lies inside the chain's valid extent (all tiles but those at the
// right / bottom screen edge): no per-texel bounds arithmetic.
// What the tile-out needs of the kernel's arguments, read again from the kernel-argument segment (scalar cache) when a tile is
// finished: held in scalar registers across the scan conversion, these ~30 dwords are spilled to VGPR lanes and back.
struct TileOutParams {
    ChordHZBDesc hzbDesc;                                   // (only the fields the reduction uses are loaded)
    uint16_t* hzbMinA; uint16_t* hzbMinB; uint16_t* hzbMaxB; uint32_t* tileRange;
    uint16_t* hzbExA; uint16_t* hzbExB;
    unsigned long long* vis; float* depthOut; int32_t Wi; uint32_t tilesX; uint32_t debug; uint32_t clearTiles;
};
__device__ __forceinline__ TileOutParams load_tile_out_params()
{
    const RasterParams* q = kernel_args();
    TileOutParams t;
    t.hzbDesc.srcWidth = scalar_load(&q->hzbDesc.srcWidth); t.hzbDesc.srcHeight = scalar_load(&q->hzbDesc.srcHeight);
    t.hzbDesc.width = scalar_load(&q->hzbDesc.width); t.hzbDesc.height = scalar_load(&q->hzbDesc.height);
    t.hzbDesc.mipCount = scalar_load(&q->hzbDesc.mipCount);
#pragma unroll
    for (int l = 0; l < 6; l++) t.hzbDesc.mipOffset[l] = scalar_load(&q->hzbDesc.mipOffset[l]);
    t.hzbMinA = scalar_load(&q->hzbMinA); t.hzbMinB = scalar_load(&q->hzbMinB); t.hzbMaxB = scalar_load(&q->hzbMaxB);
    t.hzbExA = scalar_load(&q->hzbExA); t.hzbExB = scalar_load(&q->hzbExB);
    t.tileRange = scalar_load(&q->tileRange); t.vis = scalar_load(&q->vis); t.depthOut = scalar_load(&q->depthOut);
    t.Wi = scalar_load(&q->Wi); t.tilesX = scalar_load(&q->tilesX); t.debug = scalar_load(&q->debug); t.clearTiles = scalar_load(&q->clearTiles);
    return t;
}

// SH: a tile of a sharded frame -- the words go to the tile's slot of the rank's chunk (tile-linear), the HZB texels, the valid
// range and the tile's bin length to its slots of the exchange buffers.
template <bool INTERIOR, bool SH>
__device__ __forceinline__ void tile_out_and_hzb_body(const TileOutParams& p, const unsigned long long* tile, float* sM2, uint32_t* sRange,
                                                      uint32_t tileId, uint32_t slotId, uint32_t binLength, int32_t ox, int32_t oy, int32_t tw, int32_t th)
{
    static_assert(TILE == 64 && TB == 512, "wave w <-> pixel rows 8w..8w+7");
    const ChordHZBDesc& d = p.hzbDesc;
    const uint32_t tX = tileId % p.tilesX, tY = tileId / p.tilesX;
    // (the thread index goes through an empty asm: everything the reduction derives from it -- a dozen texel offsets per lane -- is
    // loop-invariant over the kernel's work items, and hoisted out of that loop it sat in registers through the whole scan conversion:
    // 8 of them in scratch in the sharded instantiation)
    uint32_t tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const uint32_t lane = tid & 63u, wave = tid >> 6, half = lane >> 5, l = lane & 31u;
    uint16_t* exA = SH && p.hzbExA ? p.hzbExA + (size_t)slotId * CHORD_HZB_SLOT_HALVES : nullptr;
    uint16_t* exB = SH ? p.hzbExB + (size_t)slotId * CHORD_HZB_FINAL_SLOT_HALVES : nullptr;
    auto vw = [&](uint32_t lv) { return min(max(1u, d.width >> lv), (((d.srcWidth - 1u) >> 1) >> lv) + 1u); };
    auto vh = [&](uint32_t lv) { return min(max(1u, d.height >> lv), (((d.srcHeight - 1u) >> 1) >> lv) + 1u); };
    // texel (lx, ly) of the tile's (32 >> lv)^2 texels at level lv
    auto put = [&](uint32_t lv, uint32_t lx, uint32_t ly, float mn, float mx) {
        const uint32_t side = 32u >> lv, gx = tX * side + lx, gy = tY * side + ly;
        if (INTERIOR || (lv < d.mipCount && gx < vw(lv) && gy < vh(lv))) {
            const uint16_t hmn = f32_to_f16(mn);
            uint16_t hmx = f32_to_f16(mx);
            if (lv == 5u) hmx = (uint16_t)(hmx + 1u);                       // storeHZBMip5
            if (SH) {
                const uint32_t o = hzb_slot_level_offset(lv) + ly * side + lx;
                if (exA) exA[o] = hmn;
                exB[o] = hmn;
                exB[CHORD_HZB_FINAL_MAX_OFFSET + o] = hmx;
            } else {
                const size_t o = d.mipOffset[lv] + (size_t)gy * max(1u, d.width >> lv) + gx;
                if (p.hzbMinA) p.hzbMinA[o] = hmn;
                p.hzbMinB[o] = hmn;
                p.hzbMaxB[o] = hmx;
            }
        }
    };
    // (word index of the tile's first word; 32 bits: a 4096 x 4096 target has 2^24 words, a sharded one at most 1.25 x that)
    const uint32_t visBase = SH ? slotId << (2 * TILE_SHIFT) : (uint32_t)oy * (uint32_t)p.Wi + (uint32_t)ox;
    const uint32_t visPitch = SH ? (uint32_t)TILE : (uint32_t)p.Wi;
    // A lane owns 2x2 pixel quads: column pair l, row pairs q = 2 half + rp (rp = 0, 1) of the wave's four.  A mip-0 texel
    // is lane-local, a mip-1 texel is the lane's two iterations and its x neighbour (DPP), a mip-2 texel adds the x
    // neighbour two over and the other half of the wave (the one cross-half exchange per lane); 8-byte LDS reads of
    // consecutive words per half-wave, 512-byte coalesced visibility stores per row.
    uint32_t rmin = 0xFFFFFFFFu, rmax = 0u;
    float m1n = 0.0f, m1x = 0.0f;
#pragma unroll
    for (uint32_t rp = 0; rp < 2u; rp++) {
        const uint32_t q = 2u * half + rp;
        const int32_t row = (int32_t)(8u * wave + 2u * q), x2 = (int32_t)(2u * l);
        const int32_t r0 = min(row, th - 1), r1 = min(row + 1, th - 1), xa = min(x2, tw - 1), xb = min(x2 + 1, tw - 1);
        const unsigned long long v00 = tile[r0 * TPITCH + xa], v01 = tile[r0 * TPITCH + xb];
        const unsigned long long v10 = tile[r1 * TPITCH + xa], v11 = tile[r1 * TPITCH + xb];
        if (!SH && p.depthOut) {
            // depth-only pass (renderMeshDepth): what leaves the tile is the D32 image -- the high halves of the words, 8 bytes
            // per lane and row (no 64-bit image, no extract pass afterwards)
            if (INTERIOR || x2 < tw) {
                float* dst = p.depthOut + (size_t)(oy + row) * (size_t)p.Wi + ox + x2;
                const float d00 = __uint_as_float((uint32_t)(v00 >> 32)), d01 = __uint_as_float((uint32_t)(v01 >> 32));
                const float d10 = __uint_as_float((uint32_t)(v10 >> 32)), d11 = __uint_as_float((uint32_t)(v11 >> 32));
                if (INTERIOR || row < th) { if (INTERIOR || x2 + 1 < tw) *reinterpret_cast<float2*>(dst) = make_float2(d00, d01); else dst[0] = d00; }
                if (INTERIOR || row + 1 < th) { if (INTERIOR || x2 + 1 < tw) *reinterpret_cast<float2*>(dst + p.Wi) = make_float2(d10, d11); else dst[p.Wi] = d10; }
            }
        } else
        if (!ABL(p, DBG_NO_VIS_STORE) && (INTERIOR || x2 < tw)) {
            unsigned long long* dst = p.vis + visBase + (size_t)row * visPitch + x2;
            if (INTERIOR || row < th) { if (INTERIOR || x2 + 1 < tw) *reinterpret_cast<ulonglong2*>(dst) = make_ulonglong2(v00, v01); else dst[0] = v00; }
            if (INTERIOR || row + 1 < th) { if (INTERIOR || x2 + 1 < tw) *reinterpret_cast<ulonglong2*>(dst + visPitch) = make_ulonglong2(v10, v11); else dst[visPitch] = v10; }
        }
        const float dq[4] = {__uint_as_float((uint32_t)(v00 >> 32)), __uint_as_float((uint32_t)(v01 >> 32)),
                             __uint_as_float((uint32_t)(v10 >> 32)), __uint_as_float((uint32_t)(v11 >> 32))};
#pragma unroll
        for (int k = 0; k < 4; k++) {                                       // valid range (hzb.hlsl:163-176), branch-free
            const uint32_t bits = __float_as_uint(dq[k]);
            const bool drawn = dq[k] > 0.0f;
            rmax = max(rmax, drawn ? bits : 0u);
            rmin = min(rmin, (drawn && dq[k] < 1.0f) ? bits : 0xFFFFFFFFu);
        }
        const float mn = fminf(fminf(dq[0], dq[1]), fminf(dq[2], dq[3])), mx = fmaxf(fmaxf(dq[0], dq[1]), fmaxf(dq[2], dq[3]));
        put(0u, l, 4u * wave + q, mn, mx);                                  // mip 0 texel (l, 4 wave + q)
        if (rp == 0u) { m1n = mn; m1x = mx; } else { m1n = fminf(m1n, mn); m1x = fmaxf(m1x, mx); }
    }
    m1n = fminf(m1n, __shfl_xor(m1n, 1, 64)); m1x = fmaxf(m1x, __shfl_xor(m1x, 1, 64));   // mip 1 texel (l/2, 2 wave + half)
    if ((l & 1u) == 0u) put(1u, l >> 1, 2u * wave + half, m1n, m1x);
    float m2n = fminf(m1n, __shfl_xor(m1n, 2, 64)), m2x = fmaxf(m1x, __shfl_xor(m1x, 2, 64));
    m2n = fminf(m2n, __shfl_xor(m2n, 32, 64)); m2x = fmaxf(m2x, __shfl_xor(m2x, 32, 64));   // mip 2 texel (l/4, wave)
    if (half == 0u && (l & 3u) == 0u) {
        put(2u, l >> 2, wave, m2n, m2x);
        sM2[wave * 8u + (l >> 2)] = m2n; sM2[64u + wave * 8u + (l >> 2)] = m2x;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        rmin = min(rmin, (uint32_t)__shfl_down(rmin, off, 64));
        rmax = max(rmax, (uint32_t)__shfl_down(rmax, off, 64));
    }
    if (lane == 0u) { sRange[wave * 2u] = rmin; sRange[wave * 2u + 1u] = rmax; }
    __syncthreads();
    if (wave == 0u) {
        const uint32_t x = lane & 7u, y = lane >> 3;                        // mip 2 texel (x, y) of the tile
        float n3 = sM2[lane], x3 = sM2[64u + lane];
        n3 = fminf(n3, __shfl_xor(n3, 1, 64)); x3 = fmaxf(x3, __shfl_xor(x3, 1, 64));
        n3 = fminf(n3, __shfl_xor(n3, 8, 64)); x3 = fmaxf(x3, __shfl_xor(x3, 8, 64));
        if (!(x & 1u) && !(y & 1u)) put(3u, x >> 1, y >> 1, n3, x3);
        n3 = fminf(n3, __shfl_xor(n3, 2, 64)); x3 = fmaxf(x3, __shfl_xor(x3, 2, 64));
        n3 = fminf(n3, __shfl_xor(n3, 16, 64)); x3 = fmaxf(x3, __shfl_xor(x3, 16, 64));
        if (!(x & 3u) && !(y & 3u)) put(4u, x >> 2, y >> 2, n3, x3);
        n3 = fminf(n3, __shfl_xor(n3, 4, 64)); x3 = fmaxf(x3, __shfl_xor(x3, 4, 64));
        n3 = fminf(n3, __shfl_xor(n3, 32, 64)); x3 = fmaxf(x3, __shfl_xor(x3, 32, 64));
        if (lane == 0u) {
            put(5u, 0u, 0u, n3, x3);
            uint32_t lo = 0xFFFFFFFFu, hi = 0u;
#pragma unroll
            for (uint32_t w = 0; w < TB / 64u; w++) { lo = min(lo, sRange[2u * w]); hi = max(hi, sRange[2u * w + 1u]); }
            if (SH) {
                // the slot's tail: valid range of the tile, and its bin entries of the frame so far (what the tile map is balanced by)
                uint32_t* tail = reinterpret_cast<uint32_t*>(exB + CHORD_HZB_FINAL_RANGE_OFFSET);
                const uint32_t before = p.clearTiles ? 0u : tail[2];
                tail[0] = lo; tail[1] = hi; tail[2] = before + binLength; tail[3] = 0u;
            } else {
                p.tileRange[2u * tileId] = lo; p.tileRange[2u * tileId + 1u] = hi;   // reduced over tiles by hzb_tail_kernel
            }
        }
    }
}

template <bool SH>
__device__ __forceinline__ void tile_out_and_hzb(const unsigned long long* tile, float* sM2, uint32_t* sRange,
                                                 uint32_t tileId, uint32_t slotId, uint32_t binLength, int32_t ox, int32_t oy, int32_t tw, int32_t th)
{
    const TileOutParams p = load_tile_out_params();
    const ChordHZBDesc& d = p.hzbDesc;
    const uint32_t tX = tileId % p.tilesX, tY = tileId / p.tilesX;
    const uint32_t vw0 = min(max(1u, d.width), ((d.srcWidth - 1u) >> 1) + 1u), vh0 = min(max(1u, d.height), ((d.srcHeight - 1u) >> 1) + 1u);
    // (valid extents shrink by floor per level, so a tile inside level 0's is inside every level's up to 5)
    const bool interior = tw == TILE && th == TILE && d.mipCount > 5u && (tX + 1u) * 32u <= vw0 && (tY + 1u) * 32u <= vh0;
    if (interior) tile_out_and_hzb_body<true, SH>(p, tile, sM2, sRange, tileId, slotId, binLength, ox, oy, tw, th);
    else tile_out_and_hzb_body<false, SH>(p, tile, sM2, sRange, tileId, slotId, binLength, ox, oy, tw, th);
}

// Split tiles (see raster_tile_kernel): merges this slice's LDS tile into the tile's accumulation slab and draws a
// ticket; the last slice to arrive takes the merged words back into LDS and returns true.  Kept out of line so
// that its registers do not count against the scan-conversion loops (134 vs 109 VGPRs inlined).
__device__ __noinline__ bool merge_slices(unsigned long long* tile, unsigned long long* slab, uint32_t* ticket, uint32_t slices,
                                          uint32_t* sTicket, uint32_t* overflow)
{
    // all of a thread's atomics are in flight together (one round trip, not TILE*TILE/TB of them)
    constexpr uint32_t PER = TILE * TILE / TB;
    unsigned long long got[PER];
#pragma unroll
    for (uint32_t k = 0; k < PER; k++) {
        const uint32_t i = threadIdx.x + k * TB;
        const unsigned long long v = tile[(i >> TILE_SHIFT) * TPITCH + (i & (TILE - 1))];
        got[k] = v != 0ull ? atomicMax(slab + i, v) : 0ull;       // the returned value makes the wave wait for the atomic
    }
    unsigned long long seen = 0ull;
#pragma unroll
    for (uint32_t k = 0; k < PER; k++) seen |= got[k];
    if (seen == 0xFFFFFFFFFFFFFFFFull) *overflow = 8u;            // (never true: keeps the returns live)
    __syncthreads();
    if (threadIdx.x == 0) *sTicket = atomicAdd(ticket, 1u);
    __syncthreads();
    if (*sTicket != slices - 1u) return false;                    // (no thread touches LDS `tile` past this point)
#pragma unroll
    for (uint32_t k = 0; k < PER; k++) got[k] = atomicExch(slab + threadIdx.x + k * TB, 0ull);
#pragma unroll
    for (uint32_t k = 0; k < PER; k++) {
        const uint32_t i = threadIdx.x + k * TB;
        tile[(i >> TILE_SHIFT) * TPITCH + (i & (TILE - 1))] = got[k];
    }
    __syncthreads();                                              // the caller's next pass over `tile` maps words to threads differently
    return true;
}

// DEPTH: a depth-only pass with depth clamp (shadow views): the interpolated depth is clamped to [0, 1]
// Pixel blocks of small clusters (CHORD_REC_BLOCK): the wave merges the blocks its lanes hold as bin entries, two at a time,
// every lane a word: coalesced 8-byte loads and one ds_max_u64 per non-empty word.  (header: see device_layer.h)
__device__ __forceinline__ void merge_block_word(unsigned long long* tile, unsigned long long v, uint32_t i, uint32_t hdr, uint32_t rcp)
{
    const uint32_t w = ((hdr >> 12) & 15u) + 1u;
    const uint32_t row = (i * rcp) >> 16, col = i - row * w;              // exact for i < 256, w <= 16
    const uint32_t lx = (hdr & 63u) + col, ly = ((hdr >> 6) & 63u) + row;
    if (v != 0ull && lx < (uint32_t)TILE && ly < (uint32_t)TILE) atomicMax(&tile[ly * TPITCH + lx], v);
}

__device__ __forceinline__ void merge_blocks(unsigned long long* tile, const unsigned long long* __restrict__ pool, unsigned long long todo,
                                             uint32_t name, uint32_t hdrLo, uint32_t hdrHi, uint32_t lane)
{
    // four blocks per step, a 16-byte granule per lane and block: granule g holds the block's words 2g - 1 and 2g (word -1 is
    // the header), so the first 127 words of each of the four are in flight together (a block of sub-pixel geometry has
    // 64..121) -- ~4 KB of loads outstanding per wave instead of one block's worth per memory round trip, in 16-byte
    // requests (8-byte loads run at 0.54-0.70x their rate, MI355X_MICROARCH.md).  Two groups of four alternate (A, B): the
    // loads of the next group are issued before the current one is merged, so a step's memory round trip hides behind the
    // previous step's LDS merges instead of following them -- what a workgroup that is alone on its CU needs (a rank of an
    // 8-rank frame owns 255 tiles: one workgroup per CU, nothing else to switch to).
#define MB_PICK(H, R, N, SRC)                                                                                             \
    _Pragma("unroll") for (int j = 0; j < 4; j++) {                                                                       \
        const bool any = todo != 0ull;                                                                                    \
        const int l = any ? __ffsll((long long)todo) - 1 : 0;                                                             \
        todo &= todo - 1ull;                                    /* (0 stays 0) */                                         \
        H[j] = bcast(hdrLo, l); R[j] = bcast(hdrHi, l);                                                                   \
        SRC[j] = reinterpret_cast<const ulonglong2*>(pool + (size_t)(bcast(name, l) & CHORD_REC_INDEX_MASK) * 2u);        \
        N[j] = any ? (((H[j] >> 12) & 15u) + 1u) * (((H[j] >> 16) & 15u) + 1u) : 0u;                                      \
    }
    // granule g exists iff 2g - 1 < n
#define MB_LOAD(A, N, SRC)                                                                                                \
    _Pragma("unroll") for (int j = 0; j < 4; j++) A[j] = 2u * lane <= N[j] && N[j] != 0u ? SRC[j][lane] : make_ulonglong2(0ull, 0ull);
#define MB_MERGE(A, H, R, N, SRC)                                                                                         \
    _Pragma("unroll") for (int j = 0; j < 4; j++) {                                                                       \
        if (lane != 0u) merge_block_word(tile, A[j].x, 2u * lane - 1u, H[j], R[j]);                                       \
        if (2u * lane < N[j]) merge_block_word(tile, A[j].y, 2u * lane, H[j], R[j]);                                      \
    }                                                                                                                     \
    _Pragma("unroll") for (int j = 0; j < 4; j++)                                                                         \
        for (uint32_t g = lane + 64u; 2u * g <= N[j]; g += 64u) {                                                         \
            const ulonglong2 v = SRC[j][g];                                                                               \
            merge_block_word(tile, v.x, 2u * g - 1u, H[j], R[j]);                                                         \
            if (2u * g < N[j]) merge_block_word(tile, v.y, 2u * g, H[j], R[j]);                                           \
        }
    if (!todo) return;
    // two groups of four in flight (three were measured in round 5: the third group's 20 scalars are lane spills inside the merge
    // loop, subpixel_64m 136 -> 147 us -- profiles/r05_tile_kernel_experiments.txt)
    uint32_t hA[4], rA[4], nA[4], hB[4], rB[4], nB[4];
    const ulonglong2* srcA[4];
    const ulonglong2* srcB[4];
    ulonglong2 aA[4], aB[4];
    MB_PICK(hA, rA, nA, srcA)
    MB_LOAD(aA, nA, srcA)
    for (;;) {
        const bool moreB = todo != 0ull;
        if (moreB) { MB_PICK(hB, rB, nB, srcB) MB_LOAD(aB, nB, srcB) }
        MB_MERGE(aA, hA, rA, nA, srcA)
        if (!moreB) break;
        const bool moreA = todo != 0ull;
        if (moreA) { MB_PICK(hA, rA, nA, srcA) MB_LOAD(aA, nA, srcA) }
        MB_MERGE(aB, hB, rB, nB, srcB)
        if (!moreA) break;
    }
#undef MB_PICK
#undef MB_LOAD
#undef MB_MERGE
}

// Direct passes that take only touched tiles (RasterParams::tileTouched): of the pass's mask, the tile of set bit k and the tile
// behind set bit g - 1 (bits in tile order), and the number of set bits.  One 8-byte load per lane covers 4 096 tiles
// (launch_raster takes this form for targets of at most that many); every wave of the workgroup works it out for itself -- no LDS,
// no barrier.  Everything stays in vector registers up to the readlanes of the answers (the kernel sits at its scalar-register
// limit).  A k or g - 1 beyond the set bits gives tile 0.
__device__ __forceinline__ uint32_t touched_tile(const uint32_t* __restrict__ mask, uint32_t k, uint32_t g, uint32_t& total, uint32_t& tail)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint2 w = reinterpret_cast<const uint2*>(mask)[lane];
    const uint32_t c = (uint32_t)(__popc(w.x) + __popc(w.y));
    uint32_t incl = c;                                          // set bits in the words of lanes 0 .. lane
#pragma unroll
    for (uint32_t d = 1u; d < 64u; d <<= 1) { const uint32_t t = __shfl_up(incl, d, 64); if (lane >= d) incl += t; }
    total = bcast(incl, 63);
    // the lane whose word holds set bit j finds the bit's place in the word
    auto select = [&](uint32_t j) -> uint32_t {
        uint32_t r = j - (incl - c), m = w.x, pos = 0u;
        const uint32_t nLo = (uint32_t)__popc(w.x);
        if (r >= nLo) { r -= nLo; m = w.y; pos = 32u; }
#pragma unroll
        for (uint32_t s = 16u; s != 0u; s >>= 1) {
            const uint32_t n = (uint32_t)__popc(m & ((1u << s) - 1u));
            if (r >= n) { r -= n; m >>= s; pos += s; }
        }
        const unsigned long long holder = __ballot(incl - c <= j && j < incl);
        return holder ? bcast(lane * 64u + pos, (int)__ffsll((long long)holder) - 1) : 0u;
    };
    tail = select(g - 1u) + 1u;
    return select(k);
}

#ifndef TILE_MIN_BLOCKS
#define TILE_MIN_BLOCKS 4               // waves per SIMD the register allocation aims at (launch bounds: 4 -> 128 VGPRs, 6 -> 80)
#endif
template <bool SH, bool MASKED, bool DEPTH>
__global__ __launch_bounds__(TB, TILE_MIN_BLOCKS) void raster_tile_kernel(RasterParams p)
{
    __shared__ __align__(16) unsigned long long tile[TILE * TPITCH];   // 32.5 KB
    __shared__ EntrySoA prm;                                     // 26 KB: the batch's entries that need row units
    __shared__ uint32_t unitList[UNIT_CAP];                      // 16 KB: (entry | row << 9 | segment << 15) of the units of a round
    static_assert(sizeof(tile) + sizeof(EntrySoA) + sizeof(unitList) + 512 <= 81920, "two workgroups per CU need at most 80 KB of LDS each (512: the small arrays below)");
    __shared__ uint32_t offs[16];                                // (scratch of the tile-out reduction)
    __shared__ uint32_t waveSums[2][TB / 64];
    __shared__ uint32_t chunkTab[64];                            // the overflow chunks this item's entries live in
    __shared__ uint32_t sTicket;
    if (ABL(p, DBG_TILE_EXIT) && !p.clearTiles) return;
    // (the item count and the block's first item are fetched together: one round trip, not two dependent ones; the
    // list has an entry for every tile, so slot 1 + blockIdx.x exists whether or not it is active)
    // (direct passes -- orderKept 2 -- have no list: item i is tile i, and the first thing a workgroup asks memory for is its tile's counter line)
    // Workgroup 0 of a launch with tileOrderNext makes the NEXT frame's schedule of this pass: the bin counts it orders are final before
    // this kernel starts, the schedule kernel's work is one workgroup's, and here it costs one of the device's 512 tile slots for the
    // first microseconds of the launch instead of a launch of its own between the binner and this kernel (launch_raster).
    // The kernel sits at its scalar-register limit, so where that skew of the workgroup index is needed decides how it is had:
    //  * in front of the loop -- the workgroup's first item, on every tile's chain of dependent fetches -- from the argument as the
    //    launch handed it over (dead once the loop is entered).  Re-read there it was a scalar load and a wait in front of every tile's
    //    first fetch, and of every untouched tile's workgroup of a direct pass: config 3 0.1597 -> 0.1585 ms, config 4 0.3886 -> 0.3871;
    //  * at the loop's end -- the stride, off every chain -- re-read from the kernel-argument segment (wgs): held across the body, skew
    //    or stride is one more scalar to keep through the scan conversion and around the call of merge_slices.  Measured both ways:
    //    48 bytes of scratch in a kernel that had none; and with a skew of 1 in EVERY launch (a constant: workgroup 0 of a launch without
    //    a schedule to make just ends) and the stride gridDim.x - 1 held instead, config 3 0.1595 -> 0.1607 ms.  (And the other way --
    //    item, item count and stride ALL worked out again at the loop's end, only the index carried: 0.1582 -> 0.1591.)
#define TILE_SKEW (scalar_load(&kernel_args()->tileOrderNext) != nullptr ? 1u : 0u)
#define wgs (gridDim.x - TILE_SKEW)
    const uint32_t tilesAll = p.tilesX * p.tilesY;
    const uint32_t wg0 = blockIdx.x - (p.tileOrderNext != nullptr ? 1u : 0u);
    if (p.tileOrderNext && blockIdx.x == 0u) {
        tile_order_next_part(kernel_args());
        return;
    }
    const bool direct = p.orderKept == 2u;
    // (the list is asked under `!direct`: asked for before anything branches -- so that the arguments it needs come in one scalar load
    // with the others -- a direct pass's workgroups, 1 604 of 2 040 of them with nothing else to do, waited for a fetch they drop:
    // config 3 0.1581 -> 0.1593 ms, while config 4, which has no direct pass, gained 0.5 %)
    uint2 firstItem = make_uint2(wg0, 0u);
    uint32_t active = tilesAll;
    if (!direct) { firstItem = p.tileOrder[1u + min(wg0, tilesAll - 1u)]; active = p.tileOrder[0].x; }
    else if (p.tileTouched) {
        // (a direct pass over the touched tiles only, G workgroups, one per tile slot of the device: workgroup w's first item is the
        // w-th set bit of the mask -- the chain head is one round trip longer, the mask before the counter line; the 1 604 of config
        // 3's 2 040 workgroups that found an empty counter line are not launched.  A pass that touched more than G tiles gives the
        // tiles behind the G-th set bit to the items from G on, one each, as the direct form over every tile does -- tile
        // oi + tilesAll - active, the untouched ones ending at their counter line -- so that no mask is searched in the loop)
        // (G is gridDim.x: a direct pass has no schedule-making workgroup, and wgs would be two more scalar loads on the chain head)
        uint32_t touched, tail;
        firstItem.x = touched_tile(p.tileTouched, wg0, gridDim.x, touched, tail);
        active = touched > gridDim.x ? gridDim.x + tilesAll - tail : touched;
        // (the pass's cluster-count report is item 0's: a pass that touched no tile has no item 0, and workgroup 0 makes it here)
        if (active == 0u && wg0 == 0u && threadIdx.x == 0u && p.heavyHint) p.heavyHint[*p.count > TILE_DIRECT_MAX_CLUSTERS ? 0 : 2] = p.binStamp;
    }
    // (bit 31 of the loop's index: not the workgroup's first item -- asked of gridDim.x, "first" was a scalar load from the dispatch
    // packet and a wait at the top of every item)
    for (uint32_t oiw = wg0; (oiw & 0x7FFFFFFFu) < active; oiw = ((oiw & 0x7FFFFFFFu) + wgs) | 0x80000000u) {
    const uint32_t oi = oiw & 0x7FFFFFFFu;
    // (the thread index of this work item goes through an empty asm: whatever the body derives from it is invariant over the
    // item loop, and hoisted out of it those values -- offsets, masks, lane roles -- sat in registers across the whole kernel)
    uint32_t tix = threadIdx.x;
    asm volatile("" : "+v"(tix));
    const uint2 itemCount = (oiw >> 31) == 0u ? firstItem : (direct ? make_uint2(oi + tilesAll - active, 0u) : p.tileOrder[1u + oi]);   // (direct: oi when active is every tile)
    const uint32_t item = itemCount.x;
    const uint32_t tileId = item & 0xFFFu, slice = (item >> 12) & 0x3FFu, slices = (item >> 22) + 1u;
    // (kept order: the tile's counter line is read here, and -- the address needs the tile only -- a whole tile's first bin entries
    // beside it, so that the chain item -> bin entry -> record does not grow by the round trip for the length)
    const uint32_t* bin = p.tileBins + (size_t)tileId * p.binCap;
    uint32_t countWord = itemCount.y, wordSpec = 0xFFFFFFFFu;
    if (p.orderKept) {
        // (the bin words are asked for whatever the item is -- a slice's first entries are elsewhere and these are dropped --, and the
        // counter line with a SCALAR load (words 0 and 1: final since the binner ended; the kernel's own atomics touch word 2 only):
        // under `slices == 1`, and with the line in a vector register the allocator used again for the bin words' address, the compiler
        // put the fetch it was meant to travel beside behind the wait for the line -- a round trip in front of every tile)
        wordSpec = bin[tix];
        const unsigned long long cnt = scalar_load(reinterpret_cast<const unsigned long long*>(&p.tileCount[(size_t)tileId * TC_STRIDE]));
        countWord = min((uint32_t)cnt, bin_capacity(p)) | ((uint32_t)(cnt >> 32) ? 0x80000000u : 0u);
    }
    const uint32_t nAll = countWord & 0x3FFFFFFFu;                // (already clamped to the bin capacity)
    if (ABL(p, DBG_SKIP_LIGHT) && nAll < 64u) continue;
    if (ABL(p, DBG_SKIP_HEAVY) && nAll >= 64u) continue;
    if (direct) {
        // a later pass of the frame touches a fraction of the tiles (config 3: 436 of 2 040): the others' workgroups end here, one round
        // trip after their start, and the touched ones have saved the trip to a work list -- what raster_tile_order_kernel cost the
        // pass was its place in the chain of dependent launches.  No slices, no order: a bin long enough to want them says so to the
        // host, and the pass gets its schedule back from the next frame on (a choice of speed: this workgroup does the whole bin).
        if (p.heavyHint && tix == 0u) {
            if (nAll > p.tileSplitMin) p.heavyHint[0] = p.binStamp;
            if (oi == 0u) p.heavyHint[*p.count > TILE_DIRECT_MAX_CLUSTERS ? 0 : 2] = p.binStamp;     // (the pass's cluster count: one workgroup reports it)
        }
        if (nAll == 0u) continue;
    }
    if (p.orderAll && !p.clearTiles && nAll == 0u) continue;     // (a later pass's schedule that lists every tile: the untouched ones end here)
    const bool hasBlocks = (countWord >> 31) != 0u;               // (the order kernel saw pixel blocks in the tile's bin)
    const int32_t tinyArea = nAll >= TINY_DENSE_MIN ? TINY_AREA_DENSE : TINY_AREA;
    // entries [lo, n) of the bin are this item's
    // (equal parts rounded up to whole batches: with the schedule's slice count -- ceil(entries / slice length), slice length
    // TILE_SLICE, or shorter in a pass with fewer tiles than the device has slots -- that is slices of the schedule's length)
    const uint32_t per = slices > 1u ? ((nAll + slices - 1u) / slices + TB - 1u) & ~(TB - 1u) : nAll;
    const uint32_t lo = slices > 1u ? min(nAll, slice * per) : 0u;
    const uint32_t n = ABL(p, DBG_NO_BATCH) ? lo : (slices > 1u ? min(nAll, lo + per) : nAll);
    const bool prof = RASTER_PROFILE && (p.debug & DBG_TILE_CLOCKS) != 0;
    const unsigned long long t0 = prof ? wall_clock64() : 0ull;
    unsigned long long ph[6] = {0, 0, 0, 0, 0, 0}, tp = t0;
    uint32_t cUnits = 0, cUnitIters = 0, cTiny = 0, cTinyIters = 0;      // (profile only)
    // (profile build: a phase ends at a barrier of its own, and what a wave spends AT that barrier -- from its arrival to the release, i.e.
    // waiting for the workgroup's slowest wave -- is summed per phase: bw[])
    unsigned long long bw[6] = {0, 0, 0, 0, 0, 0};
#define PHASE(i) do { if (prof) { const unsigned long long ta = wall_clock64(); __syncthreads(); const unsigned long long tn = wall_clock64(); bw[i] += tn - ta; ph[i] += tn - tp; tp = tn; } } while (0)
    const int32_t ox = (int32_t)(tileId % p.tilesX) * TILE, oy = (int32_t)(tileId / p.tilesX) * TILE;
    const int32_t tw = min(TILE, p.Wi - ox), th = min(TILE, p.Hi - oy);
    const bool noPixels = ABL(p, DBG_NO_PIXELS);
    // where the tile's words live: row-major in the image, or (sharded frames: SH) tile-linear in the tile's slot of the rank's
    // chunk -- 64 rows of 64 words, the whole slot also for a tile cut by the screen edge.  (Only owned tiles are work items.)
    // (the slot is read again from the tile map where it is needed -- tile-in and tile-out, a scalar-cache hit -- rather than held
    // across the scan conversion: the kernel sits at its 128 VGPRs / 102 SGPRs)
    auto slot_of_tile = [&]() -> uint32_t { return SH ? __builtin_amdgcn_readfirstlane(scalar_load(&kernel_args()->shard.tileSlot)[tileId]) : 0u; };
    // word index of the tile's first word (32 bits: a 4096 x 4096 target has 2^24 words, a sharded one at most 1.25 x that) and its row pitch
    auto vis_base = [&]() -> uint32_t { return SH ? slot_of_tile() << (2 * TILE_SHIFT) : (uint32_t)oy * (uint32_t)p.Wi + (uint32_t)ox; };
    const uint32_t visPitch = SH ? (uint32_t)TILE : (uint32_t)p.Wi;

    // The item's first bin entries are requested BEFORE the tile-in, and the records they name before its barrier: the chain
    // item -> bin entry -> record is what a light tile waits for (profiles/r03_tile_profile_config3.txt: a third of a tile's time),
    // and the tile-in -- 33 KB of LDS stores, or the tile's words from memory -- depends on none of it.  (Bins that continue in
    // pool chunks name them through chunkTab, which is filled behind the barrier: they keep the old order.)
    const bool early = n <= p.binCap && !hasBlocks;               // (uniform)
    const uint32_t k0 = lo + tix;
    const uint32_t word0 = (early && k0 < n) ? ((p.orderKept && slices == 1u) ? wordSpec : bin[k0]) : 0xFFFFFFFFu;

    // ---- tile in: zero (first pass: this is the clear; un-fused later passes merge by max at tile-out), or the
    //      current words when a later pass must leave the finished tile in LDS for the fused HZB reduction ----
    // (an assignment under a branch, not `p.hzbFused && !p.clearTiles`: the same value, but the expression form moves two of the kernel's
    // scalar lane spills -- this spelling keeps the instruction stream the deleted `|| preloaded` term left behind)
    bool rmw = false;
    if (p.hzbFused && !p.clearTiles) rmw = true;
    // slices of a split tile start from zero; when the tile must leave this kernel complete (first pass, fused HZB)
    // they meet in memory and the last one to arrive merges them (below)
    const bool mergeSlices = slices > 1u && (p.clearTiles || rmw);
    if (!(rmw && !mergeSlices)) {
        // (the whole array incl. the padding words, 16 bytes per store)
        static_assert((TILE * TPITCH) % 2 == 0, "whole 16-byte words");
        for (uint32_t i = tix; i < TILE * TPITCH / 2; i += TB) reinterpret_cast<ulonglong2*>(tile)[i] = make_ulonglong2(0ull, 0ull);
    } else
    for (uint32_t i = tix, visBase = vis_base(); i < TILE * TILE / 2; i += TB) {
        const int32_t ly = (int32_t)(i >> (TILE_SHIFT - 1)), lx = (int32_t)(i & (TILE / 2 - 1)) * 2;
        ulonglong2 v = make_ulonglong2(0ull, 0ull);
        if (ly < th && lx < tw) {
            const unsigned long long* src = scalar_load(&kernel_args()->vis) + (size_t)(visBase + (uint32_t)ly * visPitch + (uint32_t)lx);
            if (lx + 1 < tw) v = *reinterpret_cast<const ulonglong2*>(src);
            else v.x = src[0];
        }
        tile[ly * TPITCH + lx] = v.x; tile[ly * TPITCH + lx + 1] = v.y;
    }
    // a record in flight: 32 or 48 raw bytes (which, says bit 31 of its name) in three named registers quads (an
    // array or a struct passed by reference ends up in scratch memory), expanded when its batch is processed
#define FETCH_REC(gi, a, b, c)                                                                       \
    do {                                                                                             \
        if ((gi) & CHORD_REC_WIDE) {                                                                 \
            const uint4* src_ = reinterpret_cast<const uint4*>(&p.tris[(gi) & CHORD_REC_WIDE_INDEX]); \
            a = src_[0]; b = src_[1]; c = src_[2];                                                   \
        } else {                                                                                     \
            const uint4* src_ = reinterpret_cast<const uint4*>(&p.trisC[(gi)]);                      \
            a = src_[0]; b = src_[1];                                                                \
        }                                                                                            \
    } while (0)
    uint32_t idxNext = 0xFFFFFFFFu, nameNext = 0xFFFFFFFFu;
    uint4 nq0 = make_uint4(0, 0, 0, 0), nq1 = nq0, nq2 = nq0;
    // (pixel blocks have a pass of their own below; alpha-tested triangles are records of the MASKED instantiations' pipeline only)
    auto record_name = [](uint32_t w) -> uint32_t { return (w >= CHORD_REC_BLOCK || (!MASKED && (w & 0xE0000000u) == CHORD_REC_MASKED)) ? 0xFFFFFFFFu : w; };
    if (early) {
        nameNext = record_name(word0);                                          // (binEntry of an entry of the fixed bin)
        if (nameNext != 0xFFFFFFFFu) FETCH_REC(nameNext, nq0, nq1, nq2);        // record of batch 0
        if (k0 + TB < n) idxNext = record_name(bin[k0 + TB]);                    // bin entry of batch 1
    }
    __syncthreads();
    PHASE(0);

    // ---- scan-convert the bin, 512 entries per batch -------------------------------------------
    // Software pipeline over the two dependent fetches of a batch (bin entry -> 48-byte record): the
    // record of batch b+1 and the bin entry of batch b+2 are in flight while batch b is scan-converted.
    // Overflow chunks the item's entries [lo, n) live in: a WINDOW of 64 chunk names in LDS (chunk c at chunkTab[c & 63], names of
    // chunks [chunk0, chunkEnd); an entry of another pass or a failed allocation reads as invalid and its entries are skipped).
    // A fresh schedule cuts a bin into slices of at most ~33 chunks, so the window holds a whole item; an item of a KEPT schedule
    // (orderKept) was cut for an earlier frame's bin and may now span any number of chunks -- a camera cut into a hotspot view --,
    // so the loops below slide the window along (window_advance): 32 chunks at a time once the loop has passed the window's middle.
    // Their look-ahead is at most three batches = 1.5 chunks, and names below the current batch's chunk are dead.
    uint32_t chunk0 = 0, chunkEnd = 0;
    const uint32_t chunksAll = n > p.binCap ? (n - p.binCap + CHORD_BIN_CHUNK - 1u) >> CHORD_BIN_CHUNK_SHIFT : 0u;   // chunks [0, chunksAll) hold entries below n
    auto window_load = [&](uint32_t from, uint32_t to) {
        const RasterParams* q = kernel_args();                                // (long bins only: not worth registers across the kernel)
        for (uint32_t j = from + tix; j < to; j += TB) {
            const unsigned long long e = scalar_load(&q->binChunkTab)[(size_t)tileId * scalar_load(&q->binMaxChunks) + j];
            chunkTab[j & 63u] = (uint32_t)(e >> 32) == scalar_load(&q->binStamp) ? (uint32_t)e : CHORD_BIN_CHUNK_INVALID;
        }
    };
    auto window_reset = [&]() {                                  // (callers: n > binCap; every thread of the workgroup)
        __syncthreads();                                          // (readers of an earlier window are done)
        chunk0 = lo > p.binCap ? (lo - p.binCap) >> CHORD_BIN_CHUNK_SHIFT : 0u;
        chunkEnd = min(chunksAll, chunk0 + 64u);
        window_load(chunk0, chunkEnd);
        __syncthreads();
    };
    auto window_advance = [&](uint32_t base) {                   // top of a loop iteration over entries [base, ...): uniform
        if (chunkEnd >= chunksAll || base < p.binCap + ((chunk0 + 32u) << CHORD_BIN_CHUNK_SHIFT)) return;
        __syncthreads();
        const uint32_t to = min(chunksAll, chunkEnd + 32u);
        window_load(chunkEnd, to);
        chunk0 += 32u; chunkEnd = to;
        __syncthreads();
    };
    if (n > p.binCap) window_reset();
    const uint32_t wideLimit = p.triCap * CHORD_LIST_SHARDS, compactLimit = p.triCapC * CHORD_LIST_SHARDS;
    auto binWord = [&](uint32_t k) -> uint32_t {               // bin entry k as stored, ~0u = none
        if (k < p.binCap) return bin[k];
        const uint32_t o = k - p.binCap, c = o >> CHORD_BIN_CHUNK_SHIFT;
        const uint32_t id = (c - chunk0) < (chunkEnd - chunk0) ? chunkTab[c & 63u] : CHORD_BIN_CHUNK_INVALID;
        if (id == CHORD_BIN_CHUNK_INVALID) return 0xFFFFFFFFu;
        return p.binPool[(size_t)id * CHORD_BIN_CHUNK + (o & (CHORD_BIN_CHUNK - 1u))];
    };
    // ---- pixel blocks of small clusters first: their own pass over the item's entries (nothing of the triangle
    //      pipeline below is live here; tiles without blocks -- word 2 of the tile's counter line -- skip it) ----------
    // (the block pool and its size are read from the kernel arguments here: frames without blocks -- all but the densest -- do
    // not hold them in registers)
    if (hasBlocks && !noPixels) {
        const uint32_t blockCap = scalar_load(&kernel_args()->blockCap);
        const unsigned long long* blockPool = scalar_load(&kernel_args()->blockPool);
        const uint32_t blockLimit = blockCap * CHORD_LIST_SHARDS;
        uint32_t giNext = lo + tix < n ? binWord(lo + tix) : 0xFFFFFFFFu;
        for (uint32_t base = lo; base < n; base += TB) {
            window_advance(base);
            const uint32_t gi = giNext;
            giNext = base + TB + tix < n ? binWord(base + TB + tix) : 0xFFFFFFFFu;
            // (never a block outside the pool: a slot drawn but not written after a reported overflow holds anything)
            const bool isBlock = gi != 0xFFFFFFFFu && gi >= CHORD_REC_BLOCK && (gi & CHORD_REC_INDEX_MASK) < blockLimit;
            uint2 hdr = make_uint2(0u, 0u);
            if (isBlock) hdr = *reinterpret_cast<const uint2*>(blockPool + (size_t)(gi & CHORD_REC_INDEX_MASK) * 2u);
            merge_blocks(tile, blockPool, __ballot(isBlock), gi, hdr.x, hdr.y, tix & 63u);
        }
        // (the triangle pass below walks the same entries from `lo` again: a window that was slid along goes back)
        if (n > p.binCap && chunk0 != (lo > p.binCap ? (lo - p.binCap) >> CHORD_BIN_CHUNK_SHIFT : 0u)) window_reset();
    }
    auto binEntry = [&](uint32_t k) -> uint32_t {              // record name of bin entry k, ~0u = none (or a pixel block)
        const uint32_t gi = record_name(binWord(k));           // (~0u stays ~0u)
        if (gi == 0xFFFFFFFFu || k < p.binCap) return gi;
        const bool okIdx = (gi & CHORD_REC_WIDE) ? (gi & CHORD_REC_WIDE_INDEX) < wideLimit : gi < compactLimit;
        return okIdx ? gi : 0xFFFFFFFFu;                       // (only after a reported overflow)
    };
    if (!early) {
        idxNext = k0 < n ? binEntry(k0) : 0xFFFFFFFFu;                           // bin entry of batch 0
        nameNext = idxNext;
        if (nameNext != 0xFFFFFFFFu) FETCH_REC(nameNext, nq0, nq1, nq2);         // record of batch 0
        idxNext = k0 + TB < n ? binEntry(k0 + TB) : 0xFFFFFFFFu;                 // bin entry of batch 1
    }
    // One batch in two parts, so that the caller can re-load the record registers in between (by value: a record handed over by
    // reference ends up in scratch memory).  batch_setup: the records q0..q2 named `name` of the batch's entries (one per entry
    // thread) are set up -- tiny triangles scanned at once, the others stored as entries; returns the thread's unit count.
    // batch_units: block-wide scan, unit lists, row units.
    auto batch_setup = [&](const uint4 q0, const uint4 q1, const uint4 q2, const uint32_t name) -> uint32_t {
        const bool have = name != 0xFFFFFFFFu && !ABL(p, DBG_NO_ENTRY);
        if (prof) { volatile uint32_t sink = q1.w; (void)sink; }
        PHASE(1);
        uint32_t rows = 0;
        if (have) {
            TriSetup ts;
            // (fields are picked out of the raw dwords by value: a pointer cast would put the record in scratch memory)
            if (name & CHORD_REC_WIDE) {
                TriRec w;
                w.X[0] = (int32_t)q0.x; w.X[1] = (int32_t)q0.y; w.X[2] = (int32_t)q0.z; w.Y[0] = (int32_t)q0.w;
                w.Y[1] = (int32_t)q1.x; w.Y[2] = (int32_t)q1.y;
                w.d[0] = __uint_as_float(q1.z); w.d[1] = __uint_as_float(q1.w); w.d[2] = __uint_as_float(q2.x);
                w.payload = q2.y; w.twoSided = q2.z; w.pad = q2.w;
                tri_setup_from_record(ts, w, p.Wi, p.Hi);
            } else {
                TriRecC cr;
                cr.X0 = (int32_t)q0.x; cr.Y0 = (int32_t)q0.y;
                cr.dX1 = (int16_t)(q0.z & 0xFFFFu); cr.dY1 = (int16_t)(q0.z >> 16);
                cr.dX2 = (int16_t)(q0.w & 0xFFFFu); cr.dY2 = (int16_t)(q0.w >> 16);
                cr.d[0] = __uint_as_float(q1.x); cr.d[1] = __uint_as_float(q1.y); cr.d[2] = __uint_as_float(q1.z);
                cr.payload = q1.w;
                tri_setup_from_compact(ts, cr, p.Wi, p.Hi);
            }
            {
                const int32_t x0 = max(ts.px0, ox), y0 = max(ts.py0, oy);
                const int32_t x1 = min(ts.px1, ox + tw - 1), y1 = min(ts.py1, oy + th - 1);
                if (x1 >= x0 && y1 >= y0) {
                    const bool narrow = narrow_extent(ts);
                    const bool maskedRec = MASKED && (name & CHORD_REC_WIDE) && (q2.z & 4u);   // a TriRecMaskExt follows the record
                    if (narrow && !maskedRec && (x1 - x0 + 1) * (y1 - y0 + 1) <= tinyArea) {
                        if (!ABL(p, DBG_NO_TINY)) tile_raster_narrow<TPITCH>(tile, ts, ox, oy, x0, y0, x1, y1, noPixels, DEPTH);
                        if (prof) { cTiny++; cTinyIters += (uint32_t)((x1 - x0 + 1) * (y1 - y0 + 1)); }
                    } else {
                        rows = entry_store(prm, tix, ts, narrow, ox, oy, x0, y0, x1, y1, maskedRec, name & CHORD_REC_WIDE_INDEX);   // (units, not rows)
                    }
                }
            }
        }
        return rows;
    };
    auto batch_units = [&](const uint32_t rows, const uint32_t batchNo) {
        PHASE(2);
        uint32_t total;
        // (the wave sums alternate between two buffers: a batch without units then needs no barrier but the scan's own)
        // (MASKED: one scan for both populations -- units of opaque entries in the low half, of masked entries (kind 3) in the high
        // half: a batch has at most 512 x 64 units)
        const bool mine3 = MASKED && rows && ((prm.w[11][tix] >> EF_KIND_SHIFT) & 3u) == 3u;
        const uint32_t rowsN = mine3 ? 0u : rows, rowsM = mine3 ? rows : 0u;
        const uint32_t offAll = block_scan_tb(rowsN | (rowsM << 16), waveSums[batchNo & 1u], &total);
        const uint32_t offN = offAll & 0xFFFFu, offM = offAll >> 16, totalM = MASKED ? total >> 16 : 0u;
        total &= 0xFFFFu;
        PHASE(3);
        // my units [off, off + n) of a population, cut to the round's window [r0, r0 + UNIT_CAP): one LDS word each
        auto list_units = [&](uint32_t off, uint32_t n, uint32_t r0) {
            if (!n) return;
            const uint32_t box = prm.w[11][tix];
            const uint32_t nseg = SEG_SHIFT == 6 ? 1u : ((((box >> 12) & 63u) - (box & 63u)) >> SEG_SHIFT) + 1u, y0l = (box >> 6) & 63u;
            const uint32_t lo2 = max(off, r0), hi2 = min(off + n, r0 + UNIT_CAP);
            if (lo2 < hi2) {
                uint32_t j = lo2 - off;
                uint32_t row = y0l + (nseg == 1u ? j : nseg == 2u ? j >> 1 : nseg == 4u ? j >> 2 : j / 3u);
                uint32_t seg = nseg == 1u ? 0u : nseg == 2u ? (j & 1u) : nseg == 4u ? (j & 3u) : j % 3u;
                for (uint32_t u = lo2; u < hi2; u++) {
                    unitList[u - r0] = tix | (row << 9) | (seg << 15);
                    if (++seg == nseg) { seg = 0u; row++; }
                }
            }
        };
        // rounds of UNIT_CAP units: every entry thread lists its units of the round, then every thread takes units TB apart -- a
        // unit finds its entry with ONE read instead of a 9-step binary search
        for (uint32_t r0 = 0; r0 < total; r0 += UNIT_CAP) {
            list_units(offN, rowsN, r0);
            __syncthreads();
            const uint32_t nr = min(total - r0, (uint32_t)UNIT_CAP);
            for (uint32_t ui = tix; ui < nr; ui += TB) {
                const uint32_t d = unitList[ui];
                if (ABL(p, DBG_NO_UNITS)) continue;
                const int32_t trips = entry_unit<DEPTH>(prm, tile, d & 511u, (d >> 9) & 63u, (d >> 15) & 3u, ox, oy, noPixels);
                if (prof) { cUnits++; cUnitIters += (uint32_t)trips; }
            }
            if (r0 + UNIT_CAP < total || totalM) __syncthreads(); // the list is rewritten by the next round
        }
        for (uint32_t r0 = 0; r0 < totalM; r0 += UNIT_CAP) {      // (MASKED only) the alpha-tested triangles' units
            if (rowsM) {
                const uint32_t box = prm.w[11][tix];
                const uint32_t nseg = MASKED_SEG_SHIFT == 6 ? 1u : ((((box >> 12) & 63u) - (box & 63u)) >> MASKED_SEG_SHIFT) + 1u, y0l = (box >> 6) & 63u;
                const uint32_t lo2 = max(offM, r0), hi2 = min(offM + rowsM, r0 + UNIT_CAP);
                if (lo2 < hi2) {
                    const uint32_t j = lo2 - offM, g = j / nseg;
                    uint32_t row = y0l + g, seg = j - g * nseg;
                    for (uint32_t u = lo2; u < hi2; u++) {
                        unitList[u - r0] = tix | (row << 9) | (seg << 15);
                        if (++seg == nseg) { seg = 0u; row++; }
                    }
                }
            }
            __syncthreads();
            const uint32_t nr = min(totalM - r0, (uint32_t)UNIT_CAP);
            for (uint32_t ui = tix; ui < nr; ui += TB) {
                const uint32_t d = unitList[ui];
                entry_unit_masked<DEPTH>(p, prm, tile, d & 511u, (d >> 9) & 63u, (d >> 15) & 7u, ox, oy, noPixels);
            }
            if (r0 + UNIT_CAP < totalM) __syncthreads();
        }
        total |= totalM;
        if (total) __syncthreads();                               // prm / the unit list are rewritten by the next batch
        PHASE(4);
    };
    uint32_t batchNo = 0;
    for (uint32_t base = lo; base < n; base += TB, batchNo++) {
        window_advance(base);
        const uint32_t k = base + tix;
        const uint4 q0 = nq0, q1 = nq1, q2 = nq2;
        const uint32_t name = nameNext;
        nameNext = idxNext;
        if (nameNext != 0xFFFFFFFFu) FETCH_REC(nameNext, nq0, nq1, nq2);         // record of the next batch
        idxNext = k + 2u * TB < n ? binEntry(k + 2u * TB) : 0xFFFFFFFFu;         // bin entry of the batch after
        batch_units(batch_setup(q0, q1, q2, name), batchNo);
    }
    __syncthreads();

    // ---- split tile: the slices meet in the tile's accumulation slab (device-scope atomic max of the pixels a
    //      slice touched); the last slice to arrive takes the merged words back -- with an atomic exchange that
    //      also restores the slab's invariant (all zero between uses).  Only atomics touch the slab, and a slice
    //      draws its ticket after every one of its atomics has returned, so no cache-wide release/acquire is
    //      needed (an agent-scope fence writes back the whole L2 of the XCD: measured 2x slower here). ----------
    if (mergeSlices) {
        const RasterParams* q = kernel_args();                                    // (split tiles only)
        if (!merge_slices(tile, scalar_load(&q->tileSlabs) + (size_t)tileId * (TILE * TILE), &scalar_load(&q->tileCount)[(size_t)tileId * TC_STRIDE + TC_TICKET],
                          slices, &sTicket, &scalar_load(&q->counters)->overflow)) continue;   // not the last slice: done
        if (rmw) {
            for (uint32_t i = tix, visBase = vis_base(); i < TILE * TILE / 2; i += TB) {
                const int32_t ly = (int32_t)(i >> (TILE_SHIFT - 1)), lx = (int32_t)(i & (TILE / 2 - 1)) * 2;
                if (ly >= th || lx >= tw) continue;
                const unsigned long long* src = p.vis + (size_t)(visBase + (uint32_t)ly * visPitch + (uint32_t)lx);
                tile[ly * TPITCH + lx] = max(tile[ly * TPITCH + lx], src[0]);
                if (lx + 1 < tw) tile[ly * TPITCH + lx + 1] = max(tile[ly * TPITCH + lx + 1], src[1]);
            }
        }
        __syncthreads();
    }

    // ---- tile out ------------------------------------------------------------------------------------
    if (ABL(p, DBG_NO_OUT)) {
    } else if (p.hzbFused && !ABL(p, DBG_NO_HZB)) {
        // single-GPU frame: the whole tile goes out (first pass: this is the clear; later passes loaded it), and its
        // HZB texels with it; the batch buffers are free now and hold the cross-wave part of the reduction
        tile_out_and_hzb<SH>(tile, reinterpret_cast<float*>(&prm.w[0][0]), offs, tileId, slot_of_tile(), nAll, ox, oy, tw, th);
    } else if (p.clearTiles || p.hzbFused) {
        // first pass of the frame: every word is written (16-byte coalesced stores); this is the clear
        for (uint32_t i = tix, visBase = vis_base(); i < TILE * TILE / 2; i += TB) {
            const int32_t ly = (int32_t)(i >> (TILE_SHIFT - 1)), lx = (int32_t)(i & (TILE / 2 - 1)) * 2;
            if (ly >= th || lx >= tw) continue;
            const ulonglong2 v = make_ulonglong2(tile[ly * TPITCH + lx], tile[ly * TPITCH + lx + 1]);
            unsigned long long* dst = p.vis + (size_t)(visBase + (uint32_t)ly * visPitch + (uint32_t)lx);
            if (lx + 1 < tw) *reinterpret_cast<ulonglong2*>(dst) = v;
            else dst[0] = v.x;
        }
    } else {
        // later passes: only the pixels this pass touched are merged, with a row-coalesced global atomicMax
        // (8 lanes per 64-byte line) — no read-modify-write of the whole tile
        for (uint32_t i = tix, visBase = vis_base(); i < TILE * TILE; i += TB) {
            const int32_t ly = (int32_t)(i >> TILE_SHIFT), lx = (int32_t)(i & (TILE - 1));
            const unsigned long long v = tile[ly * TPITCH + lx];
            if (v != 0ull && ly < th && lx < tw) atomicMax(p.vis + (size_t)(visBase + (uint32_t)ly * visPitch + (uint32_t)lx), v);
        }
    }
    PHASE(5);
    if (prof) {
        if (tix == 0) {
            p.tileClocks[tileId] = wall_clock64() - t0;
            for (int i = 0; i < 6; i++) p.tilePhase[(size_t)tileId * 8 + i] = ph[i];
            p.tilePhase[(size_t)tileId * 8 + 6] = 0ull; p.tilePhase[(size_t)tileId * 8 + 7] = 0ull;
        }
        __syncthreads();
        // work counters of the tile: units << 32 | row-loop trips, tiny triangles << 32 | their bbox pixels
        atomicAdd(&p.tilePhase[(size_t)tileId * 8 + 6], ((unsigned long long)cUnits << 32) | cUnitIters);
        atomicAdd(&p.tilePhase[(size_t)tileId * 8 + 7], ((unsigned long long)cTiny << 32) | cTinyIters);
        // the eight waves' time at the phase barriers, in the high halves of the phase words (ticks of 10 ns: a phase stays far below 2^32)
        if ((tix & 63u) == 0u) for (int i = 0; i < 6; i++) atomicAdd(&p.tilePhase[(size_t)tileId * 8 + i], bw[i] << 32);
    }
    __syncthreads();                                              // the LDS tile is reused by the next iteration
    }
}
#undef wgs
#undef TILE_SKEW


// ---- launches of the tile stage -----------------------------------------------------------------
void launch_raster_tiles(ChordCtx* c, const RasterParams& p, bool masked, bool depthClamp, bool makeOrder, uint32_t touchedGroups)
{
    if (makeOrder) CHORD_LAUNCH(c, raster_tile_order_kernel, dim3(1), dim3(1024), 0, c->stream, p);
    stamp(c, S_R_CLIP);
    // first pass of a frame: every tile is written, one block each, dispatched heaviest first; later passes touch
    // few tiles: one resident wave of blocks strides over the (device-side) active list
    // (a static snake assignment of 2 or 4 items per block with the next item prefetched -- half / a quarter of the blocks,
    // start-up round trips paid once, also with a loop-end barrier that does not wait for the visibility stores to drain --
    // was measured: tile kernel +4..6 % on config 3, +11..18 % on config 4; the dispatcher's dynamic hand-out of one item
    // per block balances better than any static split)
    // (sharded frames: the work items are the rank's own tiles)
    // (a rank's slices: its bins are cut into about tileSlots shares when it owns fewer tiles than that; blocks beyond the item count leave at once)
    const bool sh = p.shard.ranks > 1, clearTiles = p.clearTiles != 0u;
    const uint32_t tiles = p.tilesX * p.tilesY;
    const uint32_t slots = (uint32_t)c->numCUs * (CHORD_TILE_SHIFT == 6 ? 2u : 6u);
    const uint32_t tileBlocks = (p.tileOrderNext ? 1u : 0u) + ((clearTiles || (p.orderKept == 2u && !p.tileTouched) || p.orderAll) ? ((sh && clearTiles) ? min(tiles, max(p.shard.slotsPerRank, p.tileSlots + p.tileSlots / 2u)) : tiles)
                                                               : min(tiles, p.tileTouched && touchedGroups ? touchedGroups : slots));
    // (scenes with alpha-tested materials take the MASKED instantiations, which scan-convert those triangles in a pass of their own
    // over the batch's units)
    if (masked) {
        if (depthClamp && !sh) CHORD_LAUNCH(c, (raster_tile_kernel<false, true, true>), dim3(tileBlocks), dim3(TB), 0, c->stream, p);
        else if (sh)           CHORD_LAUNCH(c, (raster_tile_kernel<true, true, false>), dim3(tileBlocks), dim3(TB), 0, c->stream, p);
        else                   CHORD_LAUNCH(c, (raster_tile_kernel<false, true, false>), dim3(tileBlocks), dim3(TB), 0, c->stream, p);
    } else if (depthClamp && !sh) {
        CHORD_LAUNCH(c, (raster_tile_kernel<false, false, true>), dim3(tileBlocks), dim3(TB), 0, c->stream, p);
    } else {
        if (sh) CHORD_LAUNCH(c, (raster_tile_kernel<true, false, false>), dim3(tileBlocks), dim3(TB), 0, c->stream, p);
        else    CHORD_LAUNCH(c, (raster_tile_kernel<false, false, false>), dim3(tileBlocks), dim3(TB), 0, c->stream, p);
    }
    stamp(c, S_R_CHUNK);
}

} // namespace chord
