// chordvis — geometry feedback (chordvis_geometry_feedback, chordvis_visible_clusters): what a frame SAW, counted
// on the device.  Everything is uint32 arithmetic; every add commutes, so no result depends on scheduling.
//
//   geometry_pixels_kernel      a wave per 16 x 4 LATTICE pixels (material_feedback_kernel's mapping and strips), the resolve kernels'
//                               leader loop with the SLOT as its key: one leader per distinct command of the wave.  A leader fetches its
//                               command, the meshlet's triangle count, the object's primitive and the meshlet's LOD once for all its
//                               lanes; every lane tests its own triangle byte against the leader's count, and the leader adds the
//                               popcount of its contributing lanes to objectPixels[object] and lodPixels[prim][lod], and ORs the
//                               command's seen bit into its bitmap word, all three through the workgroup's table.  The three pixel
//                               totals are ballot popcounts kept per wave, summed per workgroup, one global atomic each.
//   geometry_list_kernel        a thread per command i < n, grid-stride: its seen bit, object, primitive and LOD; the lanes of a wave
//                               are balloted per distinct object and per distinct (prim, lod), and one lane per key adds the
//                               submitted and the visible popcounts through the same kind of table.  totals[3] likewise.
//   visible_count_kernel        chordvis_visible_clusters, first launch: a workgroup per 8192 commands (256 words of the seen bitmap)
//                               stores how many of them are seen.
//   visible_scatter_kernel      second launch: a workgroup sums the counts before it (its base), scans its 256 word popcounts and every
//                               thread writes the seen commands of its word, in order, below `capacity`; the last one writes the total.
//
// The count table (geo_add): GEO_TABLE entries of (word index in the feedback buffer -> count) in LDS, open addressing from a
// multiplicative hash; a key that finds neither itself nor a free entry in GEO_PROBES steps goes to global memory.  At the end a
// workgroup adds every entry it filled with one global atomic.  The words of the seen bitmap are entries too, ORed instead of added.
// All device writes are vector stores and atomics.

#include "device_layer.h"

namespace chord {

#define GEO_TABLE 1024u                // entries of a workgroup's table
#define GEO_PROBES 32u
#define GEO_EMPTY 0xFFFFFFFFu

struct GeoArgs {
    const unsigned long long* vis;
    const ChordDrawCmd* cmds;
    const uint32_t* cmdCount;
    const DObjStatic* objStatic;
    const DMeshlet* meshlets;
    const uint8_t* meshletLod;
    uint32_t* words;                   // the feedback buffer (GeoLayout)
    GeoLayout lay;
    uint32_t W, H, blocksX, waveBlocks;   // the image; wave blocks (16 x 4 lattice pixels) per lattice row, and in all
    uint32_t blocksPerGroup;           // the strip of wave blocks a workgroup walks
    uint32_t objectCount, meshletCount, cmdCapacity;
    uint32_t stride, offX, offY;
    uint32_t tableMask;                // entries of the workgroup's table in use - 1: GEO_TABLE - 1 (chordvis_set_debug 8388608: 1)
};

// kOr false: count more of `key`; true: OR bits into it (the seen bitmap's words, which start at orFrom: geo_table_flush tells the two
// kinds of entry apart by their key)
template <bool kOr = false>
__device__ __forceinline__ void geo_add(uint32_t* sKeys, uint32_t* sVals, uint32_t* __restrict__ words, uint32_t tableMask, uint32_t key, uint32_t count)
{
    uint32_t h = ((key * 0x9E3779B1u) >> 22) & tableMask;               // 10 bits
    const uint32_t probes = min(GEO_PROBES, tableMask + 1u);
    for (uint32_t p = 0; p < probes; p++) {
        const uint32_t was = atomicCAS(&sKeys[h], GEO_EMPTY, key);
        if (was == GEO_EMPTY || was == key) {
            if (kOr) atomicOr(&sVals[h], count); else atomicAdd(&sVals[h], count);
            return;
        }
        h = (h + 1u) & tableMask;
    }
    if (kOr) atomicOr(&words[key], count); else atomicAdd(&words[key], count);
}

__device__ __forceinline__ void geo_table_init(uint32_t* sKeys, uint32_t* sVals, uint32_t* sTotals)
{
    for (uint32_t i = threadIdx.x; i < GEO_TABLE; i += 256u) { sKeys[i] = GEO_EMPTY; sVals[i] = 0u; }
    if (threadIdx.x < 4u) sTotals[threadIdx.x] = 0u;
    __syncthreads();
}

// every filled entry with one global atomic: an add for a count, an OR for a word of the bitmap (keys from orFrom on).  Bits only go
// from 0 to 1 within a call, so a plain load that already shows them set makes the OR redundant; a stale 0 costs one OR more
__device__ __forceinline__ void geo_table_flush(const uint32_t* sKeys, const uint32_t* sVals, const uint32_t* sTotals, uint32_t* __restrict__ words,
                                                uint32_t totalsAt, uint32_t orFrom)
{
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < GEO_TABLE; i += 256u) {
        const uint32_t key = sKeys[i], v = sVals[i];
        if (key == GEO_EMPTY || !v) continue;
        if (key < orFrom) atomicAdd(&words[key], v);
        else if ((words[key] & v) != v) atomicOr(&words[key], v);
    }
    if (threadIdx.x < 4u && sTotals[threadIdx.x]) atomicAdd(&words[totalsAt + threadIdx.x], sTotals[threadIdx.x]);
}

__global__ __launch_bounds__(256) void geometry_pixels_kernel(const GeoArgs a)
{
    static_assert(GEO_TABLE == 1024u, "geo_add's hash keeps 10 bits");
    __shared__ uint32_t sKeys[GEO_TABLE], sVals[GEO_TABLE], sTotals[4];
    geo_table_init(sKeys, sVals, sTotals);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n = min(*a.cmdCount, a.cmdCapacity);
    uint32_t looked = 0u, contributing = 0u, rejected = 0u;            // (wave-uniform)
    const uint32_t first = blockIdx.x * a.blocksPerGroup, end = min(first + a.blocksPerGroup, a.waveBlocks);
    // the lane's pixel of a wave block: inside the image?  its low word (0 outside)
    auto pixel = [&](uint32_t block, uint32_t* low) {
        const uint32_t bx = block % a.blocksX, by = block / a.blocksX;
        const uint32_t x = (bx * 16u + (lane & 15u)) * a.stride + a.offX, y = (by * 4u + (lane >> 4)) * a.stride + a.offY;
        const bool inside = x < a.W && y < a.H;
        *low = inside ? (uint32_t)a.vis[(size_t)y * a.W + x] : 0u;
        return inside;
    };
    uint32_t block = first + (threadIdx.x >> 6), low = 0u, lowNext = 0u;
    bool inside = block < end && pixel(block, &low), insideNext = false;
    for (; block < end; block += 4u, low = lowNext, inside = insideNext) {
        // (the next block's word is on its way while this one's commands are fetched: a wave's turns are chains of dependent loads)
        insideNext = block + 4u < end && pixel(block + 4u, &lowNext);
        const uint32_t slot = ((low >> 8) & CHORD_MAX_INSTANCE_ID) - 1u;   // base.hlsli:443-447
        const bool covered = low != 0u && slot < n;

        // one leader per distinct slot of the wave
        int leader = (int)lane;
        uint64_t pending = __ballot(covered), leaders = 0ull;
        while (pending) {
            const int l = __ffsll((unsigned long long)pending) - 1;
            const uint32_t s = (uint32_t)__builtin_amdgcn_readlane((int)slot, l);
            const bool mine = covered && slot == s;
            if (mine) leader = l;
            leaders |= 1ull << l;
            pending &= ~__ballot(mine);
        }
        // a leader fetches, once for all its lanes: the meshlet's triangle count (0: the command names no object / no meshlet) and
        // the two words its pixels are counted in
        uint32_t T = 0u, objKey = 0u, lodKey = 0u;
        if (covered && leader == (int)lane) {
            const ChordDrawCmd cmd = a.cmds[slot];
            if (cmd.objectId < a.objectCount && cmd.meshletId < a.meshletCount) {
                const uint32_t prim = a.objStatic[cmd.objectId].prim;
                const uint32_t lod = min((uint32_t)a.meshletLod[cmd.meshletId], CHORD_GEOMETRY_LODS - 1u);
                objKey = a.lay.objectPixels + cmd.objectId;
                lodKey = a.lay.lodPixels + prim * CHORD_GEOMETRY_LODS + lod;
                // chordvis_upload_scene refuses an object whose prim is not below primCount, and nothing rewrites objStatic, so the
                // key is always inside lodPixels: the comparison is no part of the validity rule, only a bound on the write
                if (lodKey < a.lay.lodSubmitted) T = (a.meshlets[cmd.meshletId].vertexTriangleCount >> 8) & 0xFFu;
            }
        }
        const bool hit = covered && (low & 0xFFu) < (uint32_t)__shfl((int)T, leader, 64);
        // per leader: popcount(its contributing lanes); then all leaders at once add theirs in one step each, and OR their command's seen bit
        uint32_t led = 0u;
        while (leaders) {
            const int l = __ffsll((unsigned long long)leaders) - 1;
            leaders &= leaders - 1ull;
            const uint32_t count = (uint32_t)__popcll((unsigned long long)__ballot(hit && leader == l));
            if ((int)lane == l) led = count;
        }
        if (led) {
            geo_add(sKeys, sVals, a.words, a.tableMask, objKey, led);
            geo_add(sKeys, sVals, a.words, a.tableMask, lodKey, led);
            geo_add<true>(sKeys, sVals, a.words, a.tableMask, a.lay.seen + (slot >> 5), 1u << (slot & 31u));
        }
        looked += (uint32_t)__popcll((unsigned long long)__ballot(inside));
        contributing += (uint32_t)__popcll((unsigned long long)__ballot(hit));
        rejected += (uint32_t)__popcll((unsigned long long)__ballot(low != 0u && !hit));
    }
    if (lane == 0u) {
        if (looked) atomicAdd(&sTotals[0], looked);
        if (contributing) atomicAdd(&sTotals[1], contributing);
        if (rejected) atomicAdd(&sTotals[2], rejected);
    }
    geo_table_flush(sKeys, sVals, sTotals, a.words, a.lay.totals, a.lay.seen);
}

// one table add per distinct key among the `active` lanes of the wave: `all` of them counted into key, those with `flagged` into
// key + flaggedOffset
__device__ __forceinline__ void geo_add_by_key(uint32_t* sKeys, uint32_t* sVals, uint32_t* __restrict__ words, uint32_t tableMask, uint32_t lane,
                                               bool active, uint32_t key, bool flagged, uint32_t flaggedOffset)
{
    uint64_t rest = __ballot(active);
    while (rest) {
        const int l = __ffsll((unsigned long long)rest) - 1;
        const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, l);
        const bool mine = active && key == k;
        const uint64_t same = __ballot(mine), vis = __ballot(mine && flagged);
        rest &= ~same;
        if ((int)lane == l) {
            geo_add(sKeys, sVals, words, tableMask, k, (uint32_t)__popcll((unsigned long long)same));
            if (vis) geo_add(sKeys, sVals, words, tableMask, k + flaggedOffset, (uint32_t)__popcll((unsigned long long)vis));
        }
    }
}

__global__ __launch_bounds__(256) void geometry_list_kernel(const GeoArgs a)
{
    __shared__ uint32_t sKeys[GEO_TABLE], sVals[GEO_TABLE], sTotals[4];
    geo_table_init(sKeys, sVals, sTotals);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n = min(*a.cmdCount, a.cmdCapacity);
    const uint32_t* __restrict__ seen = a.words + a.lay.seen;
    uint32_t visible = 0u;                                              // (wave-uniform)
    // (whole waves enter every turn: the ballots want all 64 lanes)
    for (uint64_t base = (uint64_t)blockIdx.x * 256u; base < n; base += (uint64_t)gridDim.x * 256u) {
        const uint32_t i = (uint32_t)min(base + threadIdx.x, (uint64_t)n);
        bool valid = false, isSeen = false;
        uint32_t objKey = 0u, lodKey = 0u;
        if (i < n) {
            const ChordDrawCmd cmd = a.cmds[i];
            if (cmd.objectId < a.objectCount && cmd.meshletId < a.meshletCount) {
                const uint32_t prim = a.objStatic[cmd.objectId].prim;
                const uint32_t lod = min((uint32_t)a.meshletLod[cmd.meshletId], CHORD_GEOMETRY_LODS - 1u);
                objKey = a.lay.objectSubmitted + cmd.objectId;
                lodKey = a.lay.lodSubmitted + prim * CHORD_GEOMETRY_LODS + lod;
                valid = lodKey < a.lay.lodVisible;                      // always true (prim < primCount since the upload): a bound on the write
                isSeen = valid && ((seen[i >> 5] >> (i & 31u)) & 1u);
            }
        }
        geo_add_by_key(sKeys, sVals, a.words, a.tableMask, lane, valid, objKey, isSeen, a.lay.objectVisible - a.lay.objectSubmitted);
        geo_add_by_key(sKeys, sVals, a.words, a.tableMask, lane, valid, lodKey, isSeen, a.lay.lodVisible - a.lay.lodSubmitted);
        visible += (uint32_t)__popcll((unsigned long long)__ballot(isSeen));
    }
    if (lane == 0u && visible) atomicAdd(&sTotals[3], visible);
    geo_table_flush(sKeys, sVals, sTotals, a.words, a.lay.totals, a.lay.seen);
}

// ---- the visible-cluster list: count, then scan + scatter.  No state survives a call (nothing a captured graph could replay stale) ----

struct VisibleArgs {
    const ChordDrawCmd* cmds;
    const uint32_t* cmdCount;
    const uint32_t* seen;              // the bitmap
    uint32_t* groupCounts;             // per workgroup of 256 bitmap words
    ChordDrawCmd* out;
    uint32_t* outCount;
    uint32_t cmdCapacity, capacity, seenWords;
};

// the bits of bitmap word w that name commands below n
__device__ __forceinline__ uint32_t visible_word(const VisibleArgs& a, uint32_t w, uint32_t n)
{
    if (w >= a.seenWords || w * 32u >= n) return 0u;
    const uint32_t bits = a.seen[w], left = n - w * 32u;
    return left >= 32u ? bits : bits & ((1u << left) - 1u);
}

// the sum of v over the workgroup's 256 threads (every thread gets it); *before: the sum over the threads below this one
__device__ __forceinline__ uint32_t group_scan(uint32_t* sWave, uint32_t v, uint32_t* before)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
        if ((int)lane >= d) incl += up;
    }
    __syncthreads();                                                    // (sWave may still be read from the call before)
    if (lane == 63u) sWave[wave] = incl;
    __syncthreads();
    uint32_t below = 0u, total = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) { const uint32_t s = sWave[k]; if (k < wave) below += s; total += s; }
    if (before) *before = below + incl - v;
    return total;
}

__global__ __launch_bounds__(256) void visible_count_kernel(const VisibleArgs a)
{
    __shared__ uint32_t sWave[4];
    const uint32_t n = min(*a.cmdCount, a.cmdCapacity);
    const uint32_t total = group_scan(sWave, (uint32_t)__popc(visible_word(a, blockIdx.x * 256u + threadIdx.x, n)), nullptr);
    if (threadIdx.x == 0u) a.groupCounts[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void visible_scatter_kernel(const VisibleArgs a)
{
    __shared__ uint32_t sWave[4];
    const uint32_t n = min(*a.cmdCount, a.cmdCapacity);
    // the seen commands of the workgroups before this one (and, for the last workgroup, of all: the total)
    uint32_t part = 0u, all = 0u;
    for (uint32_t g = threadIdx.x; g < gridDim.x; g += 256u) {
        const uint32_t cnt = a.groupCounts[g];
        if (g < blockIdx.x) part += cnt;
        all += cnt;
    }
    const uint32_t base = group_scan(sWave, part, nullptr);
    if (blockIdx.x == gridDim.x - 1u) {
        const uint32_t total = group_scan(sWave, all, nullptr);
        if (threadIdx.x == 0u) *a.outCount = total;
    }
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    uint32_t bits = visible_word(a, w, n), before = 0u;
    (void)group_scan(sWave, (uint32_t)__popc(bits), &before);
    uint32_t at = base + before;
    while (bits && at < a.capacity) {
        const uint32_t b = (uint32_t)__ffs((int)bits) - 1u;
        bits &= bits - 1u;
        a.out[at++] = a.cmds[w * 32u + b];
    }
}

static GeoArgs geo_args(ChordCtx* c, const ChordDrawCmd* cmds, const uint32_t* cmdCount)
{
    GeoArgs a = {};
    a.cmds = cmds; a.cmdCount = cmdCount;
    a.objStatic = c->dObjStatic; a.meshlets = c->dMeshlets; a.meshletLod = c->dMeshletLod;
    a.words = c->dGeoFeedback; a.lay = c->geoLayout;
    a.objectCount = c->objectCount; a.meshletCount = c->meshletCount; a.cmdCapacity = c->cmdCapacity;
    a.tableMask = (c->debugFlags & 8388608u) ? 1u : GEO_TABLE - 1u;     // (the debug switch: two entries, so that most adds find the table full)
    return a;
}

void launch_geometry_feedback(ChordCtx* c, const unsigned long long* vis, const ChordDrawCmd* cmds, const uint32_t* cmdCount,
                              const ChordGeometryFeedbackDesc& desc)
{
    GeoArgs a = geo_args(c, cmds, cmdCount);
    a.vis = vis;
    a.W = c->width; a.H = c->height;
    a.stride = desc.stride; a.offX = desc.offset[0]; a.offY = desc.offset[1];
    // lattice pixels per row / column: those x = i * stride + offset below the size (none when the offset is not)
    const uint32_t latW = a.offX < a.W ? (a.W - a.offX + a.stride - 1u) / a.stride : 0u, latH = a.offY < a.H ? (a.H - a.offY + a.stride - 1u) / a.stride : 0u;
    a.blocksX = (latW + 15u) / 16u;
    a.waveBlocks = a.blocksX * ((latH + 3u) / 4u);
    if (a.waveBlocks) {
        // strips: at most eight workgroups per CU (all a CU holds), each at least 16 wave blocks, four per wave, over which its
        // table's set-up and flush are spread (measured: DESIGN.md 4.11)
        const uint32_t groups = min((a.waveBlocks + 15u) / 16u, (uint32_t)c->numCUs * 8u);
        a.blocksPerGroup = (a.waveBlocks + groups - 1u) / groups;
        CHORD_LAUNCH(c, geometry_pixels_kernel, dim3((a.waveBlocks + a.blocksPerGroup - 1u) / a.blocksPerGroup), dim3(256), 0, c->stream, a);
    }
    const uint32_t listGroups = min((c->cmdCapacity + 255u) / 256u, (uint32_t)c->numCUs * 4u);
    CHORD_LAUNCH(c, geometry_list_kernel, dim3(max(listGroups, 1u)), dim3(256), 0, c->stream, a);
}

void launch_visible_clusters(ChordCtx* c, const ChordDrawCmd* cmds, const uint32_t* cmdCount, ChordDrawCmd* out, uint32_t* outCount, uint32_t capacity)
{
    VisibleArgs a;
    a.cmds = cmds; a.cmdCount = cmdCount;
    a.seen = c->dGeoFeedback + c->geoLayout.seen; a.groupCounts = c->dGeoFeedback + c->geoLayout.groupCounts;
    a.out = out; a.outCount = outCount;
    a.cmdCapacity = c->cmdCapacity; a.capacity = capacity; a.seenWords = c->geoLayout.seenWords;
    const dim3 grid(c->geoLayout.groups), block(256);
    CHORD_LAUNCH(c, visible_count_kernel, grid, block, 0, c->stream, a);
    CHORD_LAUNCH(c, visible_scatter_kernel, grid, block, 0, c->stream, a);
}

} // namespace chord
