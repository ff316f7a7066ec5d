// chordvis — consumers' first step on the visibility buffer: the tile marker and the shading tile lists
// (SURVEY 8f-1).  Reference: install/resource/shader/visibility_tile.hlsl:39-219 (tilerMarkerCS,
// tilePrepareCS, prepareTileParamCS) recorded by source/renderer/visibility_tile.cpp:20-110.
//
//   visibility_mark_kernel   a wave per 128 x 8 pixels: 16-byte loads, 1 KB contiguous per wave instruction ->
//                            shading type of each pixel (visibility id -> draw command -> object ->
//                            material type, the last two folded into a per-object table at upload) ->
//                            128-bit mask per lane; the 4 lanes of a tile meet through two xor-shuffles.
//                            HBM-bound: reads every visibility word once (8 W H bytes; the reference's
//                            R32_UINT target would be 4 W H).
//   shading_tiles_kernel     a thread per 4 marker texels, block-wide scan, one reservation per 1024 texels;
//                            then the dispatch argument.
//   bounds_tiles_kernel<T>   chordvis_bin_bounds (no counterpart in the reference): a workgroup per 64 x 64 pixels reduces its tiles'
//                            depth bounds and lists the host's visible boxes that can touch each tile (end of file).
//
// The reference walks a 32x32-pixel region per 64-thread group through an 8x8 quad swizzle and reduces
// 4x4-pixel partial masks through groupshared memory in three barrier steps; none of that shapes the
// result (an OR over the tile), so the layout here is chosen for coalescing on 64-wide waves instead.

#include <algorithm>

#include "device_layer.h"
#include "device_math.h"

namespace chord {

// A wave covers 128 x 8 pixels = 16 tiles: per pixel row every lane loads the two words at x = 2 lane (16 bytes,
// 1 KB contiguous per wave instruction), accumulates the types of its 2-pixel column strip over the 8 rows, and
// the four lanes of a tile meet through two xor-shuffles.
__global__ __launch_bounds__(256) void visibility_mark_kernel(const unsigned long long* __restrict__ vis, uint32_t W, uint32_t H,
                                                              const ChordDrawCmd* __restrict__ cmds, const uint32_t* __restrict__ cmdCount,
                                                              const DObjStatic* __restrict__ objStatic, uint4* __restrict__ marker,
                                                              uint32_t mW, uint32_t mH)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t groupsX = (mW + 15u) / 16u;
    const uint32_t waves = gridDim.x * 4u, total = groupsX * mH;
    const uint32_t n = *cmdCount;
    for (uint32_t g = blockIdx.x * 4u + (threadIdx.x >> 6); g < total; g += waves) {
        const uint32_t my = g / groupsX, mx = (g % groupsX) * 16u + (lane >> 2);
        const uint32_t x = (g % groupsX) * 128u + 2u * lane;
        uint32_t m0 = 0, m1 = 0, m2 = 0, m3 = 0;
        uint32_t lastId = 0xFFFFFFFFu, lastType = 0;
        auto add = [&](uint32_t pack) {
            uint32_t type;
            if ((pack >> 8) == lastId) type = lastType;                // same cluster as the pixel before
            else {
                type = 0u;                                             // kLightingType_None
                if (pack != 0u) {
                    const uint32_t instanceId = ((pack >> 8) & CHORD_MAX_INSTANCE_ID) - 1u;    // base.hlsli:443-447
                    if (instanceId < n) type = objStatic[cmds[instanceId].objectId].shadingType;   // visibility_tile.hlsl:51-60
                }
                lastId = pack >> 8; lastType = type;
            }
            const uint32_t bit = 1u << (type & 31u);
            const uint32_t w = (type >> 5) & 3u;
            m0 |= w == 0u ? bit : 0u; m1 |= w == 1u ? bit : 0u; m2 |= w == 2u ? bit : 0u; m3 |= w == 3u ? bit : 0u;
        };
        // pixels past the right / bottom edge: the reference's clamp-to-edge Gather repeats edge pixels of this same
        // tile, which adds nothing to an OR (visibility_tile.hlsl:83-87)
        if (x < W) {
            const bool pair = x + 1u < W && (((size_t)W & 1u) == 0u);   // 16-byte aligned pair loads need an even row pitch
#pragma unroll
            for (uint32_t r = 0; r < 8u; r++) {
                const uint32_t y = my * 8u + r;
                if (y >= H) break;
                const unsigned long long* src = vis + (size_t)y * W + x;
                if (pair) {
                    const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(src);
                    add((uint32_t)v.x); add((uint32_t)v.y);
                } else {
                    add((uint32_t)src[0]);
                    if (x + 1u < W) add((uint32_t)src[1]);
                }
            }
        }
#pragma unroll
        for (int d = 1; d < 4; d <<= 1) {
            m0 |= (uint32_t)__shfl_xor((int)m0, d, 64); m1 |= (uint32_t)__shfl_xor((int)m1, d, 64);
            m2 |= (uint32_t)__shfl_xor((int)m2, d, 64); m3 |= (uint32_t)__shfl_xor((int)m3, d, 64);
        }
        if ((lane & 3u) == 0u && mx < mW) marker[(size_t)my * mW + mx] = make_uint4(m0, m1, m2, m3);
    }
}

// One thread per 4 consecutive marker texels, block-wide exclusive scan of the per-thread counts, ONE reservation
// per 1024 texels: the reference's one InterlockedAdd per wave (visibility_tile.hlsl:184-190) on a single word would
// be 2 025 returning atomics at 4K = 23 us here (~88/us per address, measured).
__global__ __launch_bounds__(256) void shading_tiles_kernel(const uint4* __restrict__ marker, uint32_t mW, uint32_t mH,
                                                            uint32_t index, uint32_t bit, uint2* __restrict__ tiles, uint32_t* __restrict__ count)
{
    __shared__ uint32_t sWave[4], sBase;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, total = mW * mH;
    for (uint32_t base = blockIdx.x * 1024u; base < total; base += gridDim.x * 1024u) {
        const uint32_t t0 = base + threadIdx.x * 4u;
        uint32_t flags = 0;
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) {
            if (t0 + i < total) {
                const uint4 m = marker[t0 + i];
                const uint32_t word = index == 0u ? m.x : index == 1u ? m.y : index == 2u ? m.z : m.w;
                if (word & bit) flags |= 1u << i;                      // visibility_tile.hlsl:169-170
            }
        }
        const uint32_t mine = (uint32_t)__popc(flags);
        uint32_t incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t nb = (uint32_t)__shfl_up((int)incl, d, 64); if (lane >= (uint32_t)d) incl += nb; }
        if (lane == 63u) sWave[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4u; w++) { const uint32_t c = sWave[w]; if (w < wave) before += c; all += c; }
        if (threadIdx.x == 0) sBase = all ? atomicAdd(count, all) : 0u;
        __syncthreads();
        uint32_t slot = sBase + before + incl - mine;
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++)
            if (flags & (1u << i)) { const uint32_t t = t0 + i; tiles[slot++] = make_uint2((t % mW) * 8u, (t / mW) * 8u); }   // :174,204
        __syncthreads();                                               // sWave / sBase are rewritten by the next chunk
    }
}

__global__ void shading_tile_args_kernel(const uint32_t* __restrict__ count, uint4* __restrict__ args)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) *args = make_uint4((*count + 3u) / 4u, 1u, 1u, 1u);   // :208-219
}

void launch_visibility_mark(ChordCtx* c, const unsigned long long* vis, const ChordDrawCmd* cmds, const uint32_t* cmdCount, uint32_t* marker)
{
    const uint32_t mW = (c->width + 7u) / 8u, mH = (c->height + 7u) / 8u;
    const uint32_t groups = ((mW + 15u) / 16u) * mH;
    uint32_t blocks = (groups + 3u) / 4u;
    const uint32_t maxBlocks = (uint32_t)c->numCUs * 8u;
    if (blocks > maxBlocks) blocks = maxBlocks;
    if (blocks < 1u) blocks = 1u;
    CHORD_LAUNCH(c, visibility_mark_kernel, dim3(blocks), dim3(256), 0, c->stream, vis, c->width, c->height, cmds, cmdCount,
                       c->dObjStatic, reinterpret_cast<uint4*>(marker), mW, mH);
}

void launch_shading_tiles(ChordCtx* c, const uint32_t* marker, uint32_t shadingType, uint32_t* tiles, uint32_t* count, uint32_t* args)
{
    const uint32_t mW = (c->width + 7u) / 8u, mH = (c->height + 7u) / 8u, total = mW * mH;
    (void)hipMemsetAsync(count, 0, sizeof(uint32_t), c->stream);        // queue.clearUAV(countBuffer), visibility_tile.cpp:68
    uint32_t blocks = (total + 1023u) / 1024u;
    if (blocks > (uint32_t)c->numCUs * 4u) blocks = (uint32_t)c->numCUs * 4u;
    if (blocks < 1u) blocks = 1u;
    CHORD_LAUNCH(c, shading_tiles_kernel, dim3(blocks), dim3(256), 0, c->stream, reinterpret_cast<const uint4*>(marker), mW, mH,
                       (shadingType >> 5) & 3u, 1u << (shadingType & 31u), reinterpret_cast<uint2*>(tiles), count);
    CHORD_LAUNCH(c, shading_tile_args_kernel, dim3(1), dim3(64), 0, c->stream, count, reinterpret_cast<uint4*>(args));
}

// ---- bounds tile lists: the boxes of chordvis_query_bounds that can touch each screen tile -------------------------------------------
// (chordvis_bin_bounds, second step; DESIGN.md 4.13.  The records that take part arrive compacted in ascending order from
// kernels_cull.hip's bounds_tiles_prepare_kernel: {rect[0] | rect[1] << 16, rect[2] | rect[3] << 16, nearestZ, farZ} and an index each.)
// A 256-thread workgroup owns a 64 x 64-pixel block of the image, (64 / T)^2 tiles of T pixels, and walks the blocks grid-stride:
//   1. depth bounds: a wave instruction reads two rows of the block, 16 bytes (two pixels) per lane -- 8 bytes per pixel when the width
//      is odd, as visibility_mark_kernel --, eight of them in flight per lane; a lane folds its pixels of a tile row, the lanes of a
//      tile column meet by xor-shuffles, the four waves in LDS (unsigned min / max of the depth words: the order of non-negative floats);
//   2. candidates: the records stream through in chunks of a record per thread, four chunks in flight; those whose rectangle meets
//      the block are appended to an LDS list by ballot and prefix count -- in record order, so the list stays ascending; when the
//      next chunk might not fit (and after the last) the list is flushed;
//   3. flush: a wave per tile, a lane per candidate: rectangle against the tile, nearestZ against far(t), farZ against near(t); the
//      kept ones' indices go to the tile's list at the tile's count plus the lane's rank in the ballot.  A tile belongs to one wave, so
//      its count is a plain LDS word and the order needs no atomic.
// A block leaves what it adds to the totals -- its tiles' counts summed, how many exceed maxPerTile, the largest -- in three words of
// its own, and bounds_tiles_totals_kernel folds them.
#define BOUNDS_TILES_CAND 512u             // candidate slots of a workgroup: two chunks
#define BOUNDS_TILES_AHEAD 4u              // chunks in flight per step of the record stream
struct BoundsTilesParams {
    const unsigned long long* vis; uint32_t W, H;
    const uint32_t* recordCount;           // null: no records
    const uint4* records; const uint32_t* recordIndex;
    uint32_t* tileCounts; uint32_t* tileItems; uint32_t* tileDepth; uint32_t* blockTotals; // each may be null; blockTotals: three words per block
    uint32_t maxPerTile, flags, tilesX, blocks, chunk, depth;      // blocks: 64 x 64-pixel blocks of the image; chunk: records per step, at most 256; depth: the depth bounds are needed
};

template <uint32_t T>
__global__ __launch_bounds__(256) void bounds_tiles_kernel(const BoundsTilesParams a)
{
    constexpr uint32_t TPS = 64u / T, TILES = TPS * TPS, G = T / 8u;       // tiles per side and per block; 8-row groups of a tile row
    __shared__ uint32_t sFar[TILES], sNear[TILES], sCount[TILES];
    __shared__ uint32_t sR0[BOUNDS_TILES_CAND], sR1[BOUNDS_TILES_CAND], sZn[BOUNDS_TILES_CAND], sZf[BOUNDS_TILES_CAND], sIx[BOUNDS_TILES_CAND];
    __shared__ uint32_t sWave[2][4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t W = a.W, H = a.H;
    const uint32_t blocksX = (W + 63u) / 64u, blocks = a.blocks;
    const uint32_t M = a.recordCount ? *a.recordCount : 0u;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
        const uint32_t bx0 = (blk % blocksX) * 64u, by0 = (blk / blocksX) * 64u;
        const uint32_t bx1 = min(W, bx0 + 64u) - 1u, by1 = min(H, by0 + 64u) - 1u;
        if (threadIdx.x < TILES) { sFar[threadIdx.x] = 0xFFFFFFFFu; sNear[threadIdx.x] = 0u; sCount[threadIdx.x] = 0u; }
        __syncthreads();
        if (a.depth) {
            const uint32_t cx = lane & 31u, x = bx0 + 2u * cx;
            const bool pair = x + 1u < W && (W & 1u) == 0u;                // 16-byte aligned pair loads need an even row pitch
            uint32_t lo[8], hi[8];
#pragma unroll
            for (uint32_t it = 0; it < 8u; it++) {
                const uint32_t y = by0 + it * 8u + wave * 2u + (lane >> 5);
                lo[it] = 0xFFFFFFFFu; hi[it] = 0u;
                if (x < W && y < H) {
                    const unsigned long long* src = a.vis + (size_t)y * W + x;
                    if (pair) {
                        const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(src);
                        const uint32_t d0 = (uint32_t)(v.x >> 32), d1 = (uint32_t)(v.y >> 32);
                        lo[it] = min(d0, d1); hi[it] = max(d0, d1);
                    } else {
                        lo[it] = hi[it] = (uint32_t)(src[0] >> 32);
                        if (x + 1u < W) { const uint32_t d1 = (uint32_t)(src[1] >> 32); lo[it] = min(lo[it], d1); hi[it] = max(hi[it], d1); }
                    }
                }
            }
#pragma unroll
            for (uint32_t tr = 0; tr < TPS; tr++) {
                uint32_t mn = 0xFFFFFFFFu, mx = 0u;
#pragma unroll
                for (uint32_t g = 0; g < G; g++) { mn = min(mn, lo[tr * G + g]); mx = max(mx, hi[tr * G + g]); }
                // the T / 2 lanes of a tile column, then the wave's two rows
#pragma unroll
                for (uint32_t d = 1u; d < T / 2u; d <<= 1) {
                    mn = min(mn, (uint32_t)__shfl_xor((int)mn, (int)d, 64)); mx = max(mx, (uint32_t)__shfl_xor((int)mx, (int)d, 64));
                }
                mn = min(mn, (uint32_t)__shfl_xor((int)mn, 32, 64)); mx = max(mx, (uint32_t)__shfl_xor((int)mx, 32, 64));
                if (lane < 32u && (cx % (T / 2u)) == 0u) {
                    const uint32_t tl = tr * TPS + (2u * cx) / T;
                    atomicMin(&sFar[tl], mn); atomicMax(&sNear[tl], mx);
                }
            }
        }
        __syncthreads();

        uint32_t nCand = 0u;                                               // (the same in every thread)
        auto flush = [&]() {
            for (uint32_t tl = wave; tl < TILES; tl += 4u) {
                const uint32_t x0 = bx0 + (tl % TPS) * T, y0 = by0 + (tl / TPS) * T;
                if (x0 >= W || y0 >= H) continue;                          // (a tile of the block beyond the image)
                const uint32_t x1 = min(W, x0 + T) - 1u, y1 = min(H, y0 + T) - 1u;
                const uint32_t t = (y0 / T) * a.tilesX + x0 / T;
                const float zFar = __uint_as_float(sFar[tl]), zNear = __uint_as_float(sNear[tl]);
                uint32_t cnt = sCount[tl];
                for (uint32_t g = 0; g < nCand; g += 64u) {
                    const uint32_t j = g + lane;
                    bool keep = false;
                    if (j < nCand) {
                        const uint32_t r0 = sR0[j], r1 = sR1[j];
                        keep = (r0 & 0xFFFFu) <= x1 && (r1 & 0xFFFFu) >= x0 && (r0 >> 16) <= y1 && (r1 >> 16) >= y0;
                        if ((a.flags & CHORD_BOUNDS_TILES_NEAR) && __uint_as_float(sZn[j]) < zFar) keep = false;
                        if ((a.flags & CHORD_BOUNDS_TILES_FAR) && __uint_as_float(sZf[j]) > zNear) keep = false;
                    }
                    const unsigned long long kept = __ballot(keep);
                    if (keep && a.tileItems) {
                        const uint32_t k = cnt + (uint32_t)__popcll(kept & below);
                        if (k < a.maxPerTile) a.tileItems[(size_t)t * a.maxPerTile + k] = sIx[j];
                    }
                    cnt += (uint32_t)__popcll(kept);
                }
                if (lane == 0u) sCount[tl] = cnt;
            }
        };
        // (BOUNDS_TILES_AHEAD chunks are asked for before the first is looked at: a step costs one trip to memory, not four)
        uint32_t parity = 0u;
        for (uint32_t base = 0u; base < M;) {
            const uint32_t left = M - base;
            uint4 rec[BOUNDS_TILES_AHEAD];
            uint32_t index[BOUNDS_TILES_AHEAD], have = 0u;                 // have: bit k = this thread holds a record of chunk k
#pragma unroll
            for (uint32_t k = 0; k < BOUNDS_TILES_AHEAD; k++) {
                const uint32_t off = k * a.chunk + threadIdx.x;
                rec[k] = make_uint4(0u, 0u, 0u, 0u);
                index[k] = 0u;
                if (threadIdx.x < a.chunk && off < left) { rec[k] = a.records[base + off]; index[k] = a.recordIndex[base + off]; have |= 1u << k; }
            }
#pragma unroll
            for (uint32_t k = 0; k < BOUNDS_TILES_AHEAD; k++) {
                if (k * a.chunk >= left) break;
                const bool hit = ((have >> k) & 1u) && (rec[k].x & 0xFFFFu) <= bx1 && (rec[k].y & 0xFFFFu) >= bx0 && (rec[k].x >> 16) <= by1 && (rec[k].y >> 16) >= by0;
                const unsigned long long hits = __ballot(hit);
                if (lane == 0u) sWave[parity][wave] = (uint32_t)__popcll(hits);
                __syncthreads();                                           // (sWave has two sets: one barrier per chunk is enough)
                uint32_t before = 0u, all = 0u;
#pragma unroll
                for (uint32_t w = 0; w < 4u; w++) { const uint32_t n = sWave[parity][w]; if (w < wave) before += n; all += n; }
                parity ^= 1u;
                if (hit) {
                    const uint32_t s = nCand + before + (uint32_t)__popcll(hits & below);   // (< BOUNDS_TILES_CAND: see the flush rule)
                    sR0[s] = rec[k].x; sR1[s] = rec[k].y; sZn[s] = rec[k].z; sZf[s] = rec[k].w; sIx[s] = index[k];
                }
                nCand += all;
                if (left - k * a.chunk <= a.chunk || nCand + a.chunk > BOUNDS_TILES_CAND) {   // the last chunk, or the next might not fit
                    __syncthreads();                                       // the candidates are written
                    flush();
                    nCand = 0u;
                    __syncthreads();                                       // the list is read before it is written again
                }
            }
            if (left <= BOUNDS_TILES_AHEAD * a.chunk) break;
            base += BOUNDS_TILES_AHEAD * a.chunk;
        }

        if (wave == 0u) {
            const uint32_t x0 = bx0 + (lane % TPS) * T, y0 = by0 + (lane / TPS) * T;
            const bool mine = lane < TILES && x0 < W && y0 < H;
            const uint32_t cnt = mine ? sCount[lane] : 0u;
            if (mine) {
                const uint32_t t = (y0 / T) * a.tilesX + x0 / T;
                if (a.tileCounts) a.tileCounts[t] = cnt;
                if (a.tileDepth) { a.tileDepth[2u * (size_t)t] = sFar[lane]; a.tileDepth[2u * (size_t)t + 1u] = sNear[lane]; }
            }
            if (a.blockTotals) {
                uint32_t sum = cnt, over = cnt > a.maxPerTile ? 1u : 0u, most = cnt;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    sum += (uint32_t)__shfl_xor((int)sum, d, 64); over += (uint32_t)__shfl_xor((int)over, d, 64);
                    most = max(most, (uint32_t)__shfl_xor((int)most, d, 64));
                }
                if (lane == 0u) { a.blockTotals[3u * blk] = sum; a.blockTotals[3u * blk + 1u] = over; a.blockTotals[3u * blk + 2u] = most; }
            }
        }
        __syncthreads();                                                   // the tiles' words are set again for the next block
    }
}

// totals[1 .. 3] from the blocks' three words: one workgroup (an image has at most 4 096 blocks).  A launch of its own instead of
// three atomics per block: the 6 120 atomics on one cache line at 3840 x 2160 made the call 91 us where it now takes 33.
__global__ __launch_bounds__(256) void bounds_tiles_totals_kernel(const uint32_t* __restrict__ blockTotals, uint32_t blocks, uint32_t* __restrict__ totals)
{
    __shared__ uint32_t sPart[4][3];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t sum = 0u, over = 0u, most = 0u;
    for (uint32_t b = threadIdx.x; b < blocks; b += 256u) { sum += blockTotals[3u * b]; over += blockTotals[3u * b + 1u]; most = max(most, blockTotals[3u * b + 2u]); }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        sum += (uint32_t)__shfl_xor((int)sum, d, 64); over += (uint32_t)__shfl_xor((int)over, d, 64);
        most = max(most, (uint32_t)__shfl_xor((int)most, d, 64));
    }
    if (lane == 0u) { sPart[wave][0] = sum; sPart[wave][1] = over; sPart[wave][2] = most; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        totals[1] = (sPart[0][0] + sPart[1][0]) + (sPart[2][0] + sPart[3][0]);
        totals[2] = (sPart[0][1] + sPart[1][1]) + (sPart[2][1] + sPart[3][1]);
        totals[3] = max(max(sPart[0][2], sPart[1][2]), max(sPart[2][2], sPart[3][2]));
    }
}

void launch_bounds_tiles(ChordCtx* c, const unsigned long long* vis, const ChordBoundsTilesDesc& desc, uint32_t count, bool haveRecords,
                         uint32_t* scratch, const ChordBoundsTiles& out)
{
    BoundsTilesParams a = {};
    a.vis = vis; a.W = c->width; a.H = c->height;
    const uint32_t blocks = bounds_tiles_blocks(c->width, c->height);      // (the scratch's three words per block are sized by it)
    a.blocks = blocks;
    if (haveRecords) {
        a.recordCount = scratch;
        a.records = reinterpret_cast<const uint4*>(scratch + bounds_tiles_records_at(count, blocks));
        a.recordIndex = reinterpret_cast<const uint32_t*>(a.records + count);
        if (out.totals) a.blockTotals = scratch + 4u;
    }
    a.tileCounts = out.tileCounts; a.tileItems = out.tileItems; a.tileDepth = out.tileDepth;
    a.maxPerTile = desc.maxPerTile; a.flags = desc.flags;
    a.tilesX = (c->width + desc.tileSize - 1u) / desc.tileSize;
    // (debug bit 33554432: chunks of 64 records and two workgroups, so that small counts walk every loop and chunk boundary)
    const bool small = (c->debugFlags & 33554432u) != 0u;
    a.chunk = small ? 64u : 256u;
    a.depth = (out.tileDepth || (haveRecords && desc.flags)) ? 1u : 0u;
    const dim3 grid(small ? std::min(blocks, 2u) : blocks);
    switch (desc.tileSize) {
    case 8u:  CHORD_LAUNCH(c, bounds_tiles_kernel<8u>, grid, dim3(256), 0, c->stream, a); break;
    case 16u: CHORD_LAUNCH(c, bounds_tiles_kernel<16u>, grid, dim3(256), 0, c->stream, a); break;
    case 32u: CHORD_LAUNCH(c, bounds_tiles_kernel<32u>, grid, dim3(256), 0, c->stream, a); break;
    default:  CHORD_LAUNCH(c, bounds_tiles_kernel<64u>, grid, dim3(256), 0, c->stream, a); break;
    }
    if (a.blockTotals) CHORD_LAUNCH(c, bounds_tiles_totals_kernel, dim3(1), dim3(256), 0, c->stream, a.blockTotals, blocks, out.totals);
}

} // namespace chord
