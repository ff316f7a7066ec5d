// Device helpers of the software rasterizer that more than one of its kernels uses (overview: kernels_raster.hip): scalar loads of
// the kernel arguments, wave helpers, the triangle set-up and the record readers and writers, bin reservation, the alpha test, the
// clipper, and the per-lane scan of a narrow triangle into an LDS tile (the block kernel's pixel window, the tile kernel's tiny
// triangles).  A macro or constant that only one stage reads is defined in that stage's file (kernels_raster_setup.hip,
// kernels_raster.hip), not here; one that launch_raster reads too is in raster_params.h.

#pragma once

#include "raster_params.h"
#include "device_math.h"
#include "texel_wrap.h"
#include "span_bounds.h"

namespace chord {

#define GUARD_BAND 1024.0f
#define TILE CHORD_TILE         // pixels per tile side
#define TILE_SHIFT CHORD_TILE_SHIFT
// LDS row pitch of the tile in 8-byte words: one word of padding rotates the banks by 2 per row, so lanes
// that walk different rows at the same x (the row-unit loop) do not all hit the same bank pair
#define TPITCH (TILE + 1)
#define SMALL_AREA 256          // clipped bbox pixels a single lane scans on its own
// a tile whose bin holds this many entries is VERY hot: the tile schedule marks it in RasterParams::hotTiles, and the block kernel
// draws SLOT_AHEAD_VERY_HOT bin slots ahead on it (kernels_raster_setup.hip, "Hot tiles")
#define SLOT_VERY_HOT 262144u

// Scalar loads and the kernel arguments re-read at their point of use.  The raster kernels take ONE by-value RasterParams; the
// compiler loads every field a kernel touches into scalar registers up front and keeps it there, and the loops of these
// kernels sit at the 102-SGPR limit: what does not fit lives in VGPR lanes, one v_readlane / v_writelane per use (the record
// setup kernel: 900 of them, a tenth of its instructions).  Fields needed once per cluster / tile are therefore read again
// from the kernel-argument segment (scalar cache) where they are used; the pointer goes through an empty asm so that the
// loads cannot be hoisted back to the top.
template <typename T>
__device__ __forceinline__ T scalar_load(const T* ptr)
{
    // uniform address, data written by an earlier kernel: the scalar cache is coherent at kernel boundaries
    return *reinterpret_cast<const __attribute__((address_space(4))) T*>(reinterpret_cast<uintptr_t>(ptr));
}
__device__ __forceinline__ const RasterParams* kernel_args()
{
    unsigned long long kp = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kp));
    return reinterpret_cast<const RasterParams*>(kp);
}

// number of set bits of a wave mask below this lane
__device__ __forceinline__ uint32_t mbcnt64(unsigned long long m) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }
__device__ __forceinline__ int32_t bcast(int32_t v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ uint32_t bcast(uint32_t v, int src) { return (uint32_t)__builtin_amdgcn_readlane((int)v, src); }
__device__ __forceinline__ float bcast(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }

// Sharded frames: does this rank own tile (tx, ty) / a tile under the pixel rectangle?  (ranks == 1: always)
__device__ __forceinline__ bool owns_tile(const ShardInfo& s, int32_t tx, int32_t ty)
{
    if (s.ranks <= 1) return true;
    return shard_owns_tile(s, (uint32_t)tx, (uint32_t)ty);
}
__device__ __forceinline__ bool owns_rect(const ShardInfo& s, int32_t px0, int32_t py0, int32_t px1, int32_t py1)
{
    if (s.ranks <= 1) return true;
    return shard_owns_any_tile(s, (uint32_t)px0 >> TILE_SHIFT, (uint32_t)py0 >> TILE_SHIFT, (uint32_t)px1 >> TILE_SHIFT, (uint32_t)py1 >> TILE_SHIFT);
}

// depth clamp (shadow views): the near / far planes do not clip
__device__ __forceinline__ bool in_fast_volume_xy(const f4& h)
{
    return h.w > 0.0f && (GUARD_BAND * h.w + h.x) >= 0.0f && (GUARD_BAND * h.w - h.x) >= 0.0f &&
           (GUARD_BAND * h.w + h.y) >= 0.0f && (GUARD_BAND * h.w - h.y) >= 0.0f;
}

__device__ __forceinline__ bool in_fast_volume(const f4& h)
{
    return h.w > 0.0f && (h.w - h.z) >= 0.0f && h.z >= 0.0f &&
           (GUARD_BAND * h.w + h.x) >= 0.0f && (GUARD_BAND * h.w - h.x) >= 0.0f &&
           (GUARD_BAND * h.w + h.y) >= 0.0f && (GUARD_BAND * h.w - h.y) >= 0.0f;
}

// Per-triangle setup shared by every path.  Edge i is opposite vertex i:
// E0 = orient(V1,V2,P), E1 = orient(V2,V0,P), E2 = orient(V0,V1,P), times s so the interior is positive.
struct TriSetup {
    int32_t X[3], Y[3];
    float d0, e1, e2, invA;
    int32_t px0, py0, px1, py1;       // pixel bbox clamped to the screen
    int64_t area;                     // |2A|
    int32_t s;                        // orientation sign
    uint32_t payload;
};

// Returns false when the triangle is rejected (zero area, back face after snapping, empty bbox).
__device__ __forceinline__ bool narrow_extent(const TriSetup& ts)
{
    const int32_t extX = max(ts.X[0], max(ts.X[1], ts.X[2])) - min(ts.X[0], min(ts.X[1], ts.X[2]));
    const int32_t extY = max(ts.Y[0], max(ts.Y[1], ts.Y[2])) - min(ts.Y[0], min(ts.Y[1], ts.Y[2]));
    return extX <= (1 << 14) && extY <= (1 << 14);       // 32-bit edge functions are exact
}

// the 32-byte form holds a triangle iff its 16-bit deltas and 32-bit anchor are exact
__device__ __forceinline__ bool fits_compact(const TriSetup& ts)
{
    return narrow_extent(ts);
}

__device__ __forceinline__ void write_record_c(TriRecC* dst, const TriSetup& ts, const float d[3])
{
    TriRecC r;
    r.X0 = ts.X[0]; r.Y0 = ts.Y[0];
    r.dX1 = (int16_t)(ts.X[1] - ts.X[0]); r.dY1 = (int16_t)(ts.Y[1] - ts.Y[0]);
    r.dX2 = (int16_t)(ts.X[2] - ts.X[0]); r.dY2 = (int16_t)(ts.Y[2] - ts.Y[0]);
    r.d[0] = d[0]; r.d[1] = d[1]; r.d[2] = d[2];
    r.payload = ts.payload;
    *dst = r;
}

__device__ __forceinline__ bool tri_setup(TriSetup& ts, bool twoSided, int32_t Wi, int32_t Hi)
{
    const int32_t dx1 = ts.X[1] - ts.X[0], dy1 = ts.Y[1] - ts.Y[0], dx2 = ts.X[2] - ts.X[0], dy2 = ts.Y[2] - ts.Y[0];
    int64_t area2;
    // deltas below 2^15 (vertices within 128 px of vertex 0 -- nearly every triangle): both products fit 2^30 and their
    // difference an int32, from full-rate 24-bit multiplies; v_mul_lo/hi_u32 of the general form are quarter rate.  The choice is
    // made per WAVE (a scalar branch): as a per-lane select the compiler evaluates both forms for every triangle -- four
    // quarter-rate multiplies here and the int64 -> double -> float conversion below, the price of ~30 plain instructions.
    const bool small = (uint32_t)(dx1 + 32767) < 65535u && (uint32_t)(dy1 + 32767) < 65535u &&
                       (uint32_t)(dx2 + 32767) < 65535u && (uint32_t)(dy2 + 32767) < 65535u;
    const bool allSmall = __ballot(!small) == 0ull;
    if (allSmall) area2 = (int64_t)(__mul24(dx1, dy2) - __mul24(dx2, dy1));
    else area2 = (int64_t)dx1 * (int64_t)dy2 - (int64_t)dx2 * (int64_t)dy1;
    if (area2 == 0) return false;
    if (!twoSided && area2 > 0) return false;            // VK_CULL_MODE_BACK_BIT (mesh_raster.cpp:235)
    ts.s = area2 < 0 ? -1 : 1;
    ts.area = area2 < 0 ? -area2 : area2;
    const int32_t minX = min(ts.X[0], min(ts.X[1], ts.X[2])), maxX = max(ts.X[0], max(ts.X[1], ts.X[2]));
    const int32_t minY = min(ts.Y[0], min(ts.Y[1], ts.Y[2])), maxY = max(ts.Y[0], max(ts.Y[1], ts.Y[2]));
    ts.px0 = max(0, (minX + 127) >> 8);                  // arithmetic shift == floor
    ts.py0 = max(0, (minY + 127) >> 8);
    ts.px1 = min(Wi - 1, (maxX - 128) >> 8);
    ts.py1 = min(Hi - 1, (maxY - 128) >> 8);
    if (ts.px1 < ts.px0 || ts.py1 < ts.py0) return false;
    // (float)(double)area: one rounding of an exact value either way -- an int32 conversion when the area fits (|2A| < 2^31)
    if (allSmall) ts.invA = 1.0f / (float)(int32_t)ts.area;
    else ts.invA = 1.0f / (float)(double)ts.area;
    return true;
}

// Depth bias of a depth-pass triangle (oracle.c header item 10): o = slope * max(|dz/dx|, |dz/dy|) + const * 2^(exponent(max |d|) - 23)
__device__ __forceinline__ float depth_bias(const TriSetup& ts, const float d[3], float biasConst, float biasSlope)
{
    const int64_t s = ts.s;
    const float invA = ts.invA;
    const int64_t a1 = -s * (int64_t)(ts.Y[0] - ts.Y[2]), b1 = s * (int64_t)(ts.X[0] - ts.X[2]);
    const int64_t a2 = -s * (int64_t)(ts.Y[1] - ts.Y[0]), b2 = s * (int64_t)(ts.X[1] - ts.X[0]);
    const float e1 = d[1] - d[0], e2 = d[2] - d[0];
    const float dzdx = ((float)(double)(a1 * 256) * invA) * e1 + ((float)(double)(a2 * 256) * invA) * e2;
    const float dzdy = ((float)(double)(b1 * 256) * invA) * e1 + ((float)(double)(b2 * 256) * invA) * e2;
    const float m = fmaxf(fabsf(dzdx), fabsf(dzdy));
    const float mz = fmaxf(fabsf(d[0]), fmaxf(fabsf(d[1]), fabsf(d[2])));
    const int32_t e = (int32_t)((__float_as_uint(mz) >> 23) & 0xFFu) - 23;
    const float r = (e > 0 && e < 255) ? __uint_as_float((uint32_t)e << 23) : 0.0f;
    return biasSlope * m + biasConst * r;
}

// Setup of a record that raster_setup_kernel / raster_clip_kernel already validated: bbox + stored sign / invA.
__device__ __forceinline__ void tri_setup_from_compact(TriSetup& ts, const TriRecC& r, int32_t Wi, int32_t Hi)
{
    ts.X[0] = r.X0; ts.Y[0] = r.Y0;
    ts.X[1] = r.X0 + r.dX1; ts.Y[1] = r.Y0 + r.dY1;
    ts.X[2] = r.X0 + r.dX2; ts.Y[2] = r.Y0 + r.dY2;
    ts.payload = r.payload;
    // the same integers tri_setup reduced: |deltas| <= 2^14, so the 32-bit product is exact
    const int32_t area2 = (int32_t)r.dX1 * (int32_t)r.dY2 - (int32_t)r.dX2 * (int32_t)r.dY1;
    ts.s = area2 < 0 ? -1 : 1;
    ts.invA = 1.0f / (float)(area2 < 0 ? -area2 : area2);           // (|2A| <= 2^29: the int32 conversion is the canonical (float)(double)|2A|)
    ts.d0 = r.d[0]; ts.e1 = r.d[1] - r.d[0]; ts.e2 = r.d[2] - r.d[0];
    const int32_t minX = min(ts.X[0], min(ts.X[1], ts.X[2])), maxX = max(ts.X[0], max(ts.X[1], ts.X[2]));
    const int32_t minY = min(ts.Y[0], min(ts.Y[1], ts.Y[2])), maxY = max(ts.Y[0], max(ts.Y[1], ts.Y[2]));
    ts.px0 = max(0, (minX + 127) >> 8);
    ts.py0 = max(0, (minY + 127) >> 8);
    ts.px1 = min(Wi - 1, (maxX - 128) >> 8);
    ts.py1 = min(Hi - 1, (maxY - 128) >> 8);
    ts.area = 0;
}

__device__ __forceinline__ void tri_setup_from_record(TriSetup& ts, const TriRec& r, int32_t Wi, int32_t Hi)
{
#pragma unroll
    for (int i = 0; i < 3; i++) { ts.X[i] = r.X[i]; ts.Y[i] = r.Y[i]; }
    ts.payload = r.payload;
    ts.s = (r.twoSided & 2u) ? -1 : 1;
    ts.invA = __uint_as_float(r.pad);
    ts.d0 = r.d[0]; ts.e1 = r.d[1] - r.d[0]; ts.e2 = r.d[2] - r.d[0];
    const int32_t minX = min(ts.X[0], min(ts.X[1], ts.X[2])), maxX = max(ts.X[0], max(ts.X[1], ts.X[2]));
    const int32_t minY = min(ts.Y[0], min(ts.Y[1], ts.Y[2])), maxY = max(ts.Y[0], max(ts.Y[1], ts.Y[2]));
    ts.px0 = max(0, (minX + 127) >> 8);
    ts.py0 = max(0, (minY + 127) >> 8);
    ts.px1 = min(Wi - 1, (maxX - 128) >> 8);
    ts.py1 = min(Hi - 1, (maxY - 128) >> 8);
    ts.area = 0;
}


// ---- record + bin emission --------------------------------------------------------------------

// What the record kernel's emission (list and bin reservations, record stores) needs of the kernel arguments, per cluster.
struct RecordEmitParams {
    DeviceCounters* counters; ClipTri* clipTris; uint32_t clipTriCap; uint32_t pass;
    TriRec* tris; uint32_t triCap; TriRecC* trisC; uint32_t triCapC; uint32_t* largeList; uint32_t largeCap;
    uint32_t* tileCount; uint32_t* tileBins; uint32_t binCap; uint32_t tilesX;
    uint32_t* binPool; uint32_t binPoolChunks; uint32_t* binPoolCount;
    unsigned long long* binChunkTab; uint32_t binStamp; uint32_t binMaxChunks;
    uint32_t* tileTouched;
    uint32_t binInSetup;
    ShardInfo shard;
};
__device__ __forceinline__ RecordEmitParams load_record_emit_params()
{
    const RasterParams* q = kernel_args();
    RecordEmitParams e;
    e.counters = scalar_load(&q->counters); e.clipTris = scalar_load(&q->clipTris); e.clipTriCap = scalar_load(&q->clipTriCap); e.pass = scalar_load(&q->pass);
    e.tris = scalar_load(&q->tris); e.triCap = scalar_load(&q->triCap); e.trisC = scalar_load(&q->trisC); e.triCapC = scalar_load(&q->triCapC);
    e.largeList = scalar_load(&q->largeList); e.largeCap = scalar_load(&q->largeCap);
    e.tileCount = scalar_load(&q->tileCount); e.tileBins = scalar_load(&q->tileBins); e.binCap = scalar_load(&q->binCap); e.tilesX = scalar_load(&q->tilesX);
    e.binPool = scalar_load(&q->binPool); e.binPoolChunks = scalar_load(&q->binPoolChunks); e.binPoolCount = scalar_load(&q->binPoolCount);
    e.binChunkTab = scalar_load(&q->binChunkTab); e.binStamp = scalar_load(&q->binStamp); e.binMaxChunks = scalar_load(&q->binMaxChunks);
    e.tileTouched = scalar_load(&q->tileTouched); e.binInSetup = scalar_load(&q->binInSetup);
    e.shard.ranks = scalar_load(&q->shard.ranks); e.shard.rank = scalar_load(&q->shard.rank); e.shard.slotsPerRank = 0u; e.shard.tilesX = 0u;
    e.shard.ownedRows = scalar_load(&q->shard.ownedRows); e.shard.tileSlot = nullptr;
    return e;
}

// One bin slot per lane, reserved with ONE atomic per distinct tile in the wave: lanes that target the
// same tile elect a leader (pure ALU), all leaders issue their atomicAdd in a single wave instruction, and
// the base is handed back through the lanes.  (64 lanes hitting one counter would serialise at the L2.)
struct BinElect { int leader; uint32_t rank, group; };

__device__ __forceinline__ BinElect wave_bin_elect(bool has, uint32_t tile, uint32_t lane)
{
    BinElect e; e.leader = 0; e.rank = 0; e.group = 0;
    unsigned long long todo = __ballot(has);
    const unsigned long long lt = (1ull << lane) - 1ull;
    while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        const uint32_t k = bcast(tile, l);
        const unsigned long long same = __ballot(has && tile == k);
        if (has && tile == k) { e.leader = l; e.rank = (uint32_t)__popcll(same & lt); e.group = (uint32_t)__popcll(same); }
        todo &= ~same;
    }
    return e;
}

// ---- tile bins ----------------------------------------------------------------------------------
// Entry `slot` of a tile's bin: the first binCap entries have a fixed home; beyond that, entries live in
// 1024-entry chunks from a pool.  The lane that drew the first slot of a chunk allocates it and publishes
// `serial << 32 | id` in the tile's chunk table; lanes that drew other slots of that chunk wait for the entry
// to carry this pass's serial.  Every allocation for the slots a wave has drawn is issued before any of its lanes
// starts waiting (bin_alloc for all of them, then bin_put), and an allocator never waits, so the wait always ends;
// it is bounded anyway (overflow bit 2) so that a logic error cannot hang the device.
__device__ __forceinline__ uint32_t bin_capacity(const RasterParams& p) { return p.binCap + p.binMaxChunks * CHORD_BIN_CHUNK; }

// step 1 of a bin write: the lane that drew the first slot of an overflow chunk allocates it and publishes it.  Never waits.
// Every slot drawn goes through here, so the drawer of a tile's slot 0 -- exactly one reservation per tile and pass, whichever
// binner made it -- also marks the tile touched (a non-returning OR: nothing waits for it).
template <class P>
__device__ __forceinline__ void bin_alloc(const P& p, uint32_t tile, uint32_t slot)
{
    if (slot == 0u && p.tileTouched) atomicOr(&p.tileTouched[tile >> 5], 1u << (tile & 31u));
    if (slot < p.binCap) return;
    const uint32_t o = slot - p.binCap, j = o >> CHORD_BIN_CHUNK_SHIFT;
    if (j >= p.binMaxChunks || (o & (CHORD_BIN_CHUNK - 1u)) != 0u) return;
    uint32_t id = atomicAdd(p.binPoolCount, 1u);
    if (id >= p.binPoolChunks) { id = CHORD_BIN_CHUNK_INVALID; atomicOr(&p.counters->overflow, 1u); }
    __hip_atomic_store(p.binChunkTab + (__umul24(tile, p.binMaxChunks) + j), ((unsigned long long)p.binStamp << 32) | id,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// step 2: store the entry; a slot inside an overflow chunk waits for the chunk's allocator (the drawer of the chunk's
// first slot, whose atomicAdd preceded this lane's: it has passed every wait of its own earlier writes and reaches its
// bin_alloc without waiting -- PROVIDED every caller runs bin_alloc for ALL the slots it has drawn before its first
// bin_put; wave_bin_commit draws eight slots per lane at once and therefore allocates for all eight first).
template <class P>
__device__ __forceinline__ void bin_put(const P& p, uint32_t tile, uint32_t slot, uint32_t gi)
{
    // (tile < 4096 and the fixed part of a bin at most 2^20 entries: the index is a full-rate 24-bit multiply and fits 32 bits)
    if (slot < p.binCap) { p.tileBins[__umul24(tile, p.binCap) + slot] = gi; return; }
    const uint32_t o = slot - p.binCap, j = o >> CHORD_BIN_CHUNK_SHIFT;
    if (j >= p.binMaxChunks) { atomicOr(&p.counters->overflow, 1u); return; }
    const unsigned long long* ent = p.binChunkTab + (__umul24(tile, p.binMaxChunks) + j);
    const unsigned long long stamp = (unsigned long long)p.binStamp << 32;
    unsigned long long e = 0;
    uint32_t spins = 0;
    for (;;) {
        e = __hip_atomic_load(ent, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((e & 0xFFFFFFFF00000000ull) == stamp) break;
        if (++spins > (1u << 20)) { atomicOr(&p.counters->overflow, 4u); return; }
        __builtin_amdgcn_s_sleep(4);
    }
    const uint32_t id = (uint32_t)e;
    if (id != CHORD_BIN_CHUNK_INVALID) p.binPool[((size_t)id << CHORD_BIN_CHUNK_SHIFT) + (o & (CHORD_BIN_CHUNK - 1u))] = gi;
}

// one slot drawn, written at once (the looped binners: a slot is drawn, allocated for and stored within one iteration)
template <class P>
__device__ __forceinline__ void bin_store(const P& p, uint32_t tile, uint32_t slot, uint32_t gi)
{
    bin_alloc(p, tile, slot);
    bin_put(p, tile, slot, gi);
}

// Bin reservations of two records per lane (triangles lane and lane + 64 of the meshlet) whose clamped bboxes touch
// at most 2x2 tiles each, split into ISSUE and COMMIT so that the caller can put every atomic of a cluster -- list
// reservations and bin reservations -- into ONE memory round trip and do all its stores afterwards (returning
// atomics and stores share the in-order vmcnt: a reservation issued behind the 48-byte record stores waits for
// them; reserve + emit were 30 of 40 us per cluster in the profile of config 3):
//   * the primary tile of every record (almost all entries) is reserved once per distinct tile of the wave;
//   * the up to three further tiles of a record that straddles a tile boundary (few lanes) are reserved by the
//     lane itself, one entry each.
struct BinTicket {
    uint32_t tileA[4], tileB[4], slotA[4], slotB[4];
    uint32_t has;                 // bit r: A has tile r, bit 4 + r: B
    uint32_t eA[4], eB[4];        // per tile slot r: leader lane | rank among the wave's lanes with the same tile << 8 (wave_bin_elect)
};

template <class P>
__device__ __forceinline__ void wave_bin_issue(const P& p, bool emitA, const TriSetup& tsA, bool emitB, const TriSetup& tsB,
                                               uint32_t lane, BinTicket& k, const bool masked = false)
{
    auto tile_of = [&](const TriSetup& ts, int r, bool emit, uint32_t& tile) -> bool {
        const int32_t tx0 = ts.px0 >> TILE_SHIFT, tx1 = ts.px1 >> TILE_SHIFT, ty0 = ts.py0 >> TILE_SHIFT, ty1 = ts.py1 >> TILE_SHIFT;
        const int32_t tx = (r & 1) ? tx1 : tx0, ty = (r & 2) ? ty1 : ty0;
        bool has = emit && !((r & 1) && tx1 == tx0) && !((r & 2) && ty1 == ty0);
        if (has) has = owns_tile(p.shard, tx, ty);
        tile = has ? __umul24((uint32_t)ty, p.tilesX) + (uint32_t)tx : 0u;
        return has;
    };
    k.has = 0u;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        k.slotA[r] = 0u; k.slotB[r] = 0u;
        if (tile_of(tsA, r, emitA, k.tileA[r])) k.has |= 1u << r;
        if (tile_of(tsB, r, emitB, k.tileB[r])) k.has |= 16u << r;
    }
    // ONE atomic per distinct tile of the wave, for the primary tile of a record AND for the up to three further tiles of a record that
    // straddles a tile boundary.  (Until round 6 the further tiles were reserved by every lane for itself: 18 % of config 3's bin entries,
    // 85 k returning atomics per frame against 12 k leader atomics, a straddling cluster's 30-60 of them on ONE counter line in one
    // wave instruction -- a line retires ~88 per microsecond: the reservation round trip was 8 of the 19.5 us a cluster took in config
    // 3's first pass, tools/setup_profile.py.)
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const BinElect a = wave_bin_elect((k.has & (1u << r)) != 0u, k.tileA[r], lane);
        const BinElect b = wave_bin_elect((k.has & (16u << r)) != 0u, k.tileB[r], lane);
        k.eA[r] = (uint32_t)a.leader | a.rank << 8; k.eB[r] = (uint32_t)b.leader | b.rank << 8;
        if ((k.has & (1u << r)) && (int)lane == a.leader) k.slotA[r] = atomicAdd(&p.tileCount[(size_t)k.tileA[r] * TC_STRIDE], a.group);
        if ((k.has & (16u << r)) && (int)lane == b.leader) k.slotB[r] = atomicAdd(&p.tileCount[(size_t)k.tileB[r] * TC_STRIDE], b.group);
    }
    if (masked) {
        // an alpha-tested cluster: the tiles its triangles are binned into are work items of the masked pass (a flag per tile, plain
        // stores of the same value: one per distinct primary tile of the wave, one per straddled tile of a lane)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            if ((k.has & (1u << r)) && lane == (k.eA[r] & 0xFFu)) p.tileCount[(size_t)k.tileA[r] * TC_STRIDE + TC_MASKED] = 1u;
            if ((k.has & (16u << r)) && lane == (k.eB[r] & 0xFFu)) p.tileCount[(size_t)k.tileB[r] * TC_STRIDE + TC_MASKED] = 1u;
        }
    }
}

// (a record that did not fit its list leaves its reserved bin slots unwritten: the frame is reported incomplete
// anyway, and a stale entry of an earlier frame is a valid index)
template <class P>
__device__ __forceinline__ void wave_bin_commit(const P& p, BinTicket& k, bool okA, uint32_t giA, bool okB, uint32_t giB)
{
#pragma unroll
    for (int r = 0; r < 4; r++) {
        k.slotA[r] = __shfl(k.slotA[r], (int)(k.eA[r] & 0xFFu), 64) + (k.eA[r] >> 8);
        k.slotB[r] = __shfl(k.slotB[r], (int)(k.eB[r] & 0xFFu), 64) + (k.eB[r] >> 8);
    }
    // all eight slots of a lane were drawn together (wave_bin_issue): every chunk allocation they owe comes before
    // the first wait -- a wait ahead of a later allocation could close a cycle between two waves (each waiting for a
    // chunk the other allocates in a later step), which costs 2^20 spins and drops entries.  A record that did not fit
    // its list still allocates (its slots are drawn; other lanes may be waiting for the chunk).
    if (k.has) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            if (k.has & (1u << r)) bin_alloc(p, k.tileA[r], k.slotA[r]);
            if (k.has & (16u << r)) bin_alloc(p, k.tileB[r], k.slotB[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        if (okA && (k.has & (1u << r))) bin_put(p, k.tileA[r], k.slotA[r], giA);
        if (okB && (k.has & (16u << r))) bin_put(p, k.tileB[r], k.slotB[r], giB);
    }
}

__device__ __forceinline__ bool touches_many_tiles(const TriSetup& ts)
{
    return ((ts.px1 >> TILE_SHIFT) - (ts.px0 >> TILE_SHIFT)) > 1 || ((ts.py1 >> TILE_SHIFT) - (ts.py0 >> TILE_SHIFT)) > 1;
}

__device__ __forceinline__ void write_record(TriRec* dst, const TriSetup& ts, const float d[3], bool twoSided, bool masked = false)
{
    TriRec r;
#pragma unroll
    for (int i = 0; i < 3; i++) { r.X[i] = ts.X[i]; r.Y[i] = ts.Y[i]; r.d[i] = d[i]; }
    r.payload = ts.payload;
    r.twoSided = (twoSided ? 1u : 0u) | (ts.s < 0 ? 2u : 0u) | (masked ? 4u : 0u);   // bit 1: orientation sign of the snapped triangle, bit 2: a TriRecMaskExt follows
    r.pad = __float_as_uint(ts.invA);                             // 1 / float(2A): the tile kernel does not redo the division
    *dst = r;
}

// ---- masked materials (mesh_raster.hlsl:34-38,107-112,198-204) -----------------------------------------------------------
// The reference samples the base-colour texture in the pixel shader and clip()s on its alpha.  Level of detail and
// filtering are the sampler hardware's business there; here they are pinned (oracle.c header item 9):
// perspective-correct uv from u/w, v/w, 1/w; ONE level per triangle from the ratio of its doubled uv area (in level-0
// texels) to its doubled pixel area, level = floor(log2(ratio)) >> 1; nearest or bilinear as the sampler's min / mag
// filter says; wrap modes on the integer texel index.  A masked triangle takes a 48-byte record (bit 2 of `twoSided`)
// plus a TriRecMaskExt in the next two slots of the same list.
__device__ __forceinline__ bool filter_is_linear(uint32_t f)
{
    return f == CHORD_FILTER_LINEAR || f == CHORD_FILTER_LINEAR_MIPMAP_NEAREST || f == CHORD_FILTER_LINEAR_MIPMAP_LINEAR;
}

__device__ __forceinline__ uint32_t mask_level_filter(const DMaterial& m, int64_t absArea2, const float u[3], const float v[3])
{
    uint32_t level = 0u;
    bool linear = filter_is_linear(m.magFilter);
    if (m.texOffset != 0xFFFFFFFFu) {
        const float texels = (float)m.texWidth * (float)m.texHeight;
        const float auv = fabsf((u[1] - u[0]) * (v[2] - v[0]) - (u[2] - u[0]) * (v[1] - v[0])) * texels;
        const float apx = (float)(double)absArea2 * (1.0f / 65536.0f);
        const float ratio = auv / apx;
        if (ratio >= 1.0f) {
            const int32_t e = (int32_t)((__float_as_uint(ratio) >> 23) & 0xFFu) - 127;
            level = min((uint32_t)(e >> 1), m.texMips - 1u);
            linear = filter_is_linear(m.minFilter);
        }
    }
    return level | (linear ? 256u : 0u);
}

__device__ __forceinline__ void write_mask_ext(TriRec* slot, const DMaterial* mp, uint32_t material, int64_t absArea2,
                                               const float u[3], const float v[3], const float w[3])
{
    // (the header fields by value; the one level the triangle samples is read where it is known)
    DMaterial m;
    m.texOffset = mp->texOffset; m.texWidth = mp->texWidth; m.texHeight = mp->texHeight; m.texMips = mp->texMips;
    m.minFilter = mp->minFilter; m.magFilter = mp->magFilter; m.wrapS = mp->wrapS; m.wrapT = mp->wrapT;
    m.alphaFactor = mp->alphaFactor; m.alphaCutOff = mp->alphaCutOff;
    TriRecMaskExt e;
#pragma unroll
    for (int i = 0; i < 3; i++) { e.iw[i] = 1.0f / w[i]; e.uw[i] = u[i] * e.iw[i]; e.vw[i] = v[i] * e.iw[i]; }
    e.levelFilter = mask_level_filter(m, absArea2, u, v);
    (void)material;
    const uint32_t level = e.levelFilter & 0xFFu;
    e.levelBase = 0xFFFFFFFFu; e.dims = 0u; e.magicS = e.biasS = e.magicT = e.biasT = 0u;
    if (m.texOffset != 0xFFFFFFFFu) {
        const DMatLevel L = mp->levels[level];                  // (resolved at upload: no loop over the levels, no division here)
        e.levelBase = L.base; e.dims = L.dims;
        e.magicS = L.magicS; e.biasS = L.biasS; e.magicT = L.magicT; e.biasT = L.biasT;
    }
    e.wraps = (m.wrapS & 0xFFFFu) | m.wrapT << 16;
    e.alphaFactor = m.alphaFactor; e.alphaCutOff = m.alphaCutOff;
    // (the 76 bytes in use: four 16-byte stores and three dwords; the rest of the second slot is never read)
    uint4* dst = reinterpret_cast<uint4*>(slot);
    const uint4* src = reinterpret_cast<const uint4*>(&e);
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
    reinterpret_cast<uint32_t*>(slot)[16] = e.biasS; reinterpret_cast<uint32_t*>(slot)[17] = e.magicT; reinterpret_cast<uint32_t*>(slot)[18] = e.biasT;
}

// One level of a material's alpha texture, resolved once per row unit (not once per pixel): base address, size, wraps, filter.
struct AlphaLevel {
    const uint8_t* base;            // NULL: no texture (white fallback, alpha 1)
    int32_t W, H;
    float fW, fH;
    uint32_t wrapS, wrapT;
    uint32_t magicS, biasS, magicT, biasT;
    bool linear;
};
__device__ __forceinline__ AlphaLevel alpha_level(const uint8_t* __restrict__ texAlpha, const TriRecMaskExt& e)
{
    const uint32_t levelBase = e.levelBase, dims = e.dims;
    AlphaLevel a;
    a.base = nullptr; a.W = 1; a.H = 1; a.fW = 1.0f; a.fH = 1.0f; a.wrapS = e.wraps & 0xFFFFu; a.wrapT = e.wraps >> 16; a.linear = (e.levelFilter & 256u) != 0u;
    a.magicS = e.magicS; a.biasS = e.biasS; a.magicT = e.magicT; a.biasT = e.biasT;
    if (levelBase == 0xFFFFFFFFu) return a;
    a.W = (int32_t)(dims & 0xFFFFu) + 1; a.H = (int32_t)(dims >> 16) + 1;
    a.fW = (float)a.W; a.fH = (float)a.H;
    a.base = texAlpha + levelBase;
    return a;
}
__device__ __forceinline__ float sample_alpha(const AlphaLevel& t, float u, float v)
{
    if (!t.base) return 1.0f;
    if (!t.linear) {
        const int32_t ix = wrap_index(texel_floor(u * t.fW), t.W, t.wrapS, t.magicS, t.biasS), iy = wrap_index(texel_floor(v * t.fH), t.H, t.wrapT, t.magicT, t.biasT);
        return (float)t.base[iy * t.W + ix] * (1.0f / 255.0f);
    }
    const float x = u * t.fW - 0.5f, y = v * t.fH - 0.5f;
    const int32_t x0 = texel_floor(x), y0 = texel_floor(y);
    float fx = x - (float)x0, fy = y - (float)y0;
    if (!(fabsf(x) < 1.0e9f)) fx = 0.0f;
    if (!(fabsf(y) < 1.0e9f)) fy = 0.0f;
    int32_t ix0, ix1, iy0, iy1;
    wrap_pair(x0, t.W, t.wrapS, t.magicS, t.biasS, ix0, ix1);
    wrap_pair(y0, t.H, t.wrapT, t.magicT, t.biasT, iy0, iy1);
    const float a00 = (float)t.base[iy0 * t.W + ix0] * (1.0f / 255.0f), a10 = (float)t.base[iy0 * t.W + ix1] * (1.0f / 255.0f);
    const float a01 = (float)t.base[iy1 * t.W + ix0] * (1.0f / 255.0f), a11 = (float)t.base[iy1 * t.W + ix1] * (1.0f / 255.0f);
    const float top = a00 + (a10 - a00) * fx, bot = a01 + (a11 - a01) * fx;
    return top + (bot - top) * fy;
}

// extension of a masked triangle of the cluster in flight: texture coordinates from the vertex stream, w from the
// wave's LDS copy of the clip-space vertices.
__device__ __forceinline__ void setup_emit_mask_ext(const RasterParams& p, TriRec* slot, uint32_t triWord, const float uv[6],
                                                 const float* lW, uint32_t material, int64_t absArea2)
{
    float u[3], v[3], w[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        u[i] = uv[2 * i]; v[i] = uv[2 * i + 1];               // (fetched at the start of the triangle phase; 0 without texture coordinates)
        w[i] = lW[(triWord >> (8 * i)) & 0xFFu];
    }
    write_mask_ext(slot, &p.materials[material], material, absArea2, u, v, w);
}

// wave-wide minimum of a and b, maximum of c and d (all 64 lanes active), results wave-uniform.  Each step's operand is a
// DPP-permuted copy (within quads, within rows of 16, then lane 15 / 31 of a row broadcast to the rows above) folded into the
// v_min / v_max itself: 24 VALU instructions for the four reductions and no LDS traffic -- the __shfl_xor form was 24
// ds_bpermute round trips plus ~40 instructions of address arithmetic and min / max.  Written as one asm block because the
// compiler expands the update_dpp builtin to copy + nop + v_mov_dpp + min; the four chains are interleaved, which also keeps
// every DPP read two instructions behind the write it depends on (the hazard the leading s_nop covers for the inputs).
__device__ __forceinline__ void wave_min2_max2(int32_t& a, int32_t& b, int32_t& c, int32_t& d)
{
#define DPP_STEP(ctrl)                                                \
    "v_min_i32_dpp %0, %0, %0 " ctrl "\n\t"                           \
    "v_min_i32_dpp %1, %1, %1 " ctrl "\n\t"                           \
    "v_max_i32_dpp %2, %2, %2 " ctrl "\n\t"                           \
    "v_max_i32_dpp %3, %3, %3 " ctrl "\n\t"
    asm volatile("s_nop 1\n\t"
                 DPP_STEP("quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf")
                 DPP_STEP("quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf")
                 DPP_STEP("row_ror:4 row_mask:0xf bank_mask:0xf")
                 DPP_STEP("row_ror:8 row_mask:0xf bank_mask:0xf")
                 DPP_STEP("row_bcast:15 row_mask:0xa bank_mask:0xf")
                 DPP_STEP("row_bcast:31 row_mask:0xc bank_mask:0xf")
                 "s_nop 0"
                 : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
#undef DPP_STEP
    a = __builtin_amdgcn_readlane(a, 63); b = __builtin_amdgcn_readlane(b, 63);
    c = __builtin_amdgcn_readlane(c, 63); d = __builtin_amdgcn_readlane(d, 63);
}

// wave-wide sums of a and b (all 64 lanes active), results wave-uniform: the same DPP ladder with v_add
__device__ __forceinline__ void wave_sum2(uint32_t& a, uint32_t& b)
{
#define DPP_STEP(ctrl)                                                \
    "v_add_u32_dpp %0, %0, %0 " ctrl "\n\t"                           \
    "v_add_u32_dpp %1, %1, %1 " ctrl "\n\t"
    asm volatile("s_nop 1\n\t"
                 DPP_STEP("quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf") "s_nop 0\n\t"
                 DPP_STEP("quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf") "s_nop 0\n\t"
                 DPP_STEP("row_ror:4 row_mask:0xf bank_mask:0xf") "s_nop 0\n\t"
                 DPP_STEP("row_ror:8 row_mask:0xf bank_mask:0xf") "s_nop 0\n\t"
                 DPP_STEP("row_bcast:15 row_mask:0xa bank_mask:0xf") "s_nop 0\n\t"
                 DPP_STEP("row_bcast:31 row_mask:0xc bank_mask:0xf")
                 "s_nop 0"
                 : "+v"(a), "+v"(b));
#undef DPP_STEP
    a = (uint32_t)__builtin_amdgcn_readlane((int)a, 63); b = (uint32_t)__builtin_amdgcn_readlane((int)b, 63);
}

// One lane bins one record into every tile its clamped bbox may touch (conservative edge test at the tile
// corners).  Only the clipped pieces use it; the hot paths go through wave_bin_issue / wave_bin_large.
template <class P>
__device__ __forceinline__ void bin_record_tiles(const P& p, const TriSetup& ts, uint32_t gi)
{
    const int ea[3] = {1, 2, 0}, eb[3] = {2, 0, 1};
    const int32_t tx0 = ts.px0 >> TILE_SHIFT, tx1 = ts.px1 >> TILE_SHIFT;
    const int32_t ty0 = ts.py0 >> TILE_SHIFT, ty1 = ts.py1 >> TILE_SHIFT;
    for (int32_t ty = ty0; ty <= ty1; ty++)
        for (int32_t tx = tx0; tx <= tx1; tx++) {
            const int32_t rx0 = max(ts.px0, tx << TILE_SHIFT), rx1 = min(ts.px1, (tx << TILE_SHIFT) + TILE - 1);
            const int32_t ry0 = max(ts.py0, ty << TILE_SHIFT), ry1 = min(ts.py1, (ty << TILE_SHIFT) + TILE - 1);
            bool hit = owns_tile(p.shard, tx, ty);
#pragma unroll
            for (int i = 0; i < 3; i++) {                         // (unrolled, no early exit: the vertex arrays stay in registers)
                const int64_t dxe = (int64_t)(ts.X[eb[i]] - ts.X[ea[i]]), dye = (int64_t)(ts.Y[eb[i]] - ts.Y[ea[i]]);
                const int64_t a = -(int64_t)ts.s * dye, b = (int64_t)ts.s * dxe;
                const int64_t bias = (a > 0 || (a == 0 && b > 0)) ? 0 : -1;
                const int64_t cx = (int64_t)(a > 0 ? rx1 : rx0) * 256 + 128, cy = (int64_t)(b > 0 ? ry1 : ry0) * 256 + 128;
                hit = hit && !((int64_t)ts.s * (dxe * (cy - ts.Y[ea[i]]) - dye * (cx - ts.X[ea[i]])) + bias < 0);
            }
            if (!hit) continue;
            const uint32_t tile = (uint32_t)ty * p.tilesX + (uint32_t)tx;
            const uint32_t slot = atomicAdd(&p.tileCount[(size_t)tile * TC_STRIDE], 1u);
            bin_store(p, tile, slot, gi);
            if ((gi & 0xE0000000u) == CHORD_REC_MASKED) p.tileCount[(size_t)tile * TC_STRIDE + TC_MASKED] = 1u;
        }
}

// ---- large records: binned by the set-up wave that made them ----------------------------------------------------
// A record whose bbox spans more than 2x2 tiles (touches_many_tiles) is binned into every tile that passes the conservative
// corner test of bin_record_tiles.  The (record, candidate tile) pairs of ALL the wave's large records of a cluster are laid
// end to end (lane order, A before B within a lane) and dealt out LARGE_ROUND per lane (64 pairs per round): a lane finds the record of its pair by a
// binary search over the wave's prefix counts and tests the tile; every reservation of a round is issued before the first is
// waited for, then every slot is allocated for before the first store (bin_put's contract).  The records wait in the wave's
// slice of sVert (LargeLds: held in registers across the record stores and the small records' bin writes they cost the kernel
// its occupancy), record k = lane (A) or 64 + lane (B).
#define LARGE_ROUND 1           // (2 or more: the record kernel spills)
struct LargeLds {
    float* f[5];                                        // the wave's x, y, u, v, depth arrays: fields 2i and 2i + 1 in f[i]
    __device__ __forceinline__ uint32_t& at(int field, uint32_t k) const { return reinterpret_cast<uint32_t*>(f[field >> 1])[(uint32_t)(field & 1) * 128u + k]; }
};
enum { LG_X0 = 0, LG_Y0 = 3, LG_S = 6, LG_BX = 7, LG_BY = 8, LG_GI = 9 };
// (bbox packed in halves: the pixel coordinates of a clamped bbox fit 16 bits)
__device__ __forceinline__ void large_put(const LargeLds& L, uint32_t k, const TriSetup& ts)
{
#pragma unroll
    for (int i = 0; i < 3; i++) { L.at(LG_X0 + i, k) = (uint32_t)ts.X[i]; L.at(LG_Y0 + i, k) = (uint32_t)ts.Y[i]; }
    L.at(LG_S, k) = (uint32_t)ts.s;
    L.at(LG_BX, k) = (uint32_t)ts.px0 | (uint32_t)ts.px1 << 16; L.at(LG_BY, k) = (uint32_t)ts.py0 | (uint32_t)ts.py1 << 16;
}
__device__ __forceinline__ uint32_t large_tiles(uint32_t bx, uint32_t by)
{
    return (((bx >> 16) >> TILE_SHIFT) - ((bx & 0xFFFFu) >> TILE_SHIFT) + 1u) * (((by >> 16) >> TILE_SHIFT) - ((by & 0xFFFFu) >> TILE_SHIFT) + 1u);
}
template <class P>
__device__ __forceinline__ void wave_bin_large(const P& e, const LargeLds& L, bool hasA, bool hasB, uint32_t lane)
{
    const uint32_t nA = hasA ? large_tiles(L.at(LG_BX, lane), L.at(LG_BY, lane)) : 0u;
    const uint32_t n = nA + (hasB ? large_tiles(L.at(LG_BX, 64u + lane), L.at(LG_BY, 64u + lane)) : 0u);
    uint32_t incl = n;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t nb = (uint32_t)__shfl_up((int)incl, d, 64); if (lane >= (uint32_t)d) incl += nb; }
    const uint32_t total = bcast(incl, 63), excl = incl - n;
    for (uint32_t base = 0; base < total; base += 64u * LARGE_ROUND) {
        uint32_t tile[LARGE_ROUND], slot[LARGE_ROUND], gi[LARGE_ROUND];
        bool hit[LARGE_ROUND];
#pragma unroll
        for (int r = 0; r < LARGE_ROUND; r++) {
            const uint32_t j = base + (uint32_t)r * 64u + lane, jj = min(j, total - 1u);   // (every lane shuffles: no lane is inactive)
            int src = 0;                                                                // the first lane whose inclusive count exceeds jj
#pragma unroll
            for (int st = 32; st > 0; st >>= 1) if ((uint32_t)__shfl((int)incl, src + st - 1, 64) <= jj) src += st;
            const uint32_t off = jj - (uint32_t)__shfl((int)excl, src, 64), offA = (uint32_t)__shfl((int)nA, src, 64);
            const uint32_t k = (uint32_t)src + (off >= offA ? 64u : 0u), t = off >= offA ? off - offA : off;
            TriSetup ts;
#pragma unroll
            for (int i = 0; i < 3; i++) { ts.X[i] = (int32_t)L.at(LG_X0 + i, k); ts.Y[i] = (int32_t)L.at(LG_Y0 + i, k); }
            ts.s = (int32_t)L.at(LG_S, k);
            const uint32_t bx = L.at(LG_BX, k), by = L.at(LG_BY, k);
            gi[r] = L.at(LG_GI, k);
            ts.px0 = (int32_t)(bx & 0xFFFFu); ts.px1 = (int32_t)(bx >> 16); ts.py0 = (int32_t)(by & 0xFFFFu); ts.py1 = (int32_t)(by >> 16);
            const int32_t tx0 = ts.px0 >> TILE_SHIFT, ty0 = ts.py0 >> TILE_SHIFT;
            const uint32_t tw = (uint32_t)((ts.px1 >> TILE_SHIFT) - tx0 + 1);
            const int32_t tx = tx0 + (int32_t)(t % tw), ty = ty0 + (int32_t)(t / tw);
            // pixel rectangle of this tile clipped to the triangle's bbox; conservative edge test at its corners (bin_record_tiles)
            const int32_t rx0 = max(ts.px0, tx << TILE_SHIFT), rx1 = min(ts.px1, (tx << TILE_SHIFT) + TILE - 1);
            const int32_t ry0 = max(ts.py0, ty << TILE_SHIFT), ry1 = min(ts.py1, (ty << TILE_SHIFT) + TILE - 1);
            const int ea[3] = {1, 2, 0}, eb[3] = {2, 0, 1};
            bool h = j < total && owns_tile(e.shard, tx, ty);
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const int64_t dxe = (int64_t)(ts.X[eb[i]] - ts.X[ea[i]]), dye = (int64_t)(ts.Y[eb[i]] - ts.Y[ea[i]]);
                const int64_t a = -(int64_t)ts.s * dye, b = (int64_t)ts.s * dxe;
                const int64_t bias = (a > 0 || (a == 0 && b > 0)) ? 0 : -1;
                const int64_t cx = (int64_t)(a > 0 ? rx1 : rx0) * 256 + 128, cy = (int64_t)(b > 0 ? ry1 : ry0) * 256 + 128;
                h = h && !((int64_t)ts.s * (dxe * (cy - ts.Y[ea[i]]) - dye * (cx - ts.X[ea[i]])) + bias < 0);
            }
            hit[r] = h;
            tile[r] = h ? (uint32_t)ty * e.tilesX + (uint32_t)tx : 0u;
            slot[r] = h ? atomicAdd(&e.tileCount[(size_t)tile[r] * TC_STRIDE], 1u) : 0u;
        }
#pragma unroll
        for (int r = 0; r < LARGE_ROUND; r++) if (hit[r]) bin_alloc(e, tile[r], slot[r]);
#pragma unroll
        for (int r = 0; r < LARGE_ROUND; r++) {
            if (!hit[r]) continue;
            bin_put(e, tile[r], slot[r], gi[r]);
            if ((gi[r] & 0xE0000000u) == CHORD_REC_MASKED) e.tileCount[(size_t)tile[r] * TC_STRIDE + TC_MASKED] = 1u;
        }
    }
}

// ---- the vertex and triangle arithmetic of the set-up kernels --------------------------------------------------------------
// The pieces that the record kernel (raster_setup_body), the block kernel (raster_setup_blocks_body) and the wide kernel
// (raster_setup_wide_kernel) share: cluster header, draw command, object matrix (the wide kernel keeps its own loop), snap.  The three are bit-exact against the oracle
// only while they say the same thing, and which of them a cluster meets is a run-time choice of the host.  The vertex transform, the
// culls and the clip-or-set-up tail (mesh_raster.hlsl:84-179) are still written out in each of the three: as shared functions they
// changed the register allocation of the wave-per-cluster bodies, which sit at 106 SGPRs, and the record kernel, held to 96 VGPRs by
// its fifth wave per SIMD, spilled (16-28 bytes of scratch per lane) -- profiles/raster_kernel_resources.md.
enum { K_NONE = 0, K_EMIT = 1, K_CLIP = 2 };
#define WAVE_LDS_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

// Wave-uniform header of a cluster: its draw command and what the meshlet and object records say of it.
// (scalar loads through the constant address space: the addresses are wave-uniform, and a vector load + v_readfirstlane per
// dword was 26 VALU instructions per header -- the record kernel is bound by VALU issue on dense scenes like the block kernel)
struct SetupHeader { uint32_t objectId, meshletId, slot, V, T, dataOffset, vertexBase, matFlags; };
// meshlets / objStatic: the caller says where the scene's pointers come from -- the wave-per-cluster bodies re-read them from the
// kernel-argument segment at each use (kernel_args: not held across the cluster loop), the wide kernel takes them from its parameters
__device__ __forceinline__ SetupHeader load_setup_header(const DMeshlet* __restrict__ meshlets, const DObjStatic* __restrict__ objStatic,
                                                         uint32_t objectId, uint32_t meshletId, uint32_t slot)
{
    SetupHeader h;
    h.objectId = objectId; h.meshletId = meshletId; h.slot = slot;
    const DMeshlet* __restrict__ mm = &meshlets[meshletId];
    const uint32_t vt = scalar_load(&mm->vertexTriangleCount);
    h.V = vt & 0xFFu; h.T = (vt >> 8) & 0xFFu;
    h.dataOffset = scalar_load(&mm->dataOffset);
    h.vertexBase = scalar_load(&mm->vertexBase);
    h.matFlags = scalar_load(&objStatic[objectId].matFlags);
    if (CHORD_MATFLAG_ALPHA(h.matFlags) >= CHORD_ALPHA_BLEND) h.T = 0u;   // blended: in no bucket of renderMesh (mesh_raster.cpp:224)
    return h;
}
// the three words of command min(i, count - 1) of a list (a wave asks for headers past the end of its list: the last one again)
__device__ __forceinline__ ChordDrawCmd load_command(const ChordDrawCmd* __restrict__ cmds, uint32_t count, uint32_t i)
{
    const uint32_t k = __builtin_amdgcn_readfirstlane(min(i, count - 1u));
    const uint32_t* __restrict__ cw = reinterpret_cast<const uint32_t*>(cmds + k);
    ChordDrawCmd c;
    c.objectId = scalar_load(cw); c.meshletId = scalar_load(cw + 1); c.slot = scalar_load(cw + 2);
    return c;
}
// the object's matrix (wave-uniform: sixteen scalar loads)
__device__ __forceinline__ Mat4 load_mvp(const DObjFrame* __restrict__ frames, uint32_t objectId)
{
    Mat4 m;
    const float* __restrict__ mv = frames[objectId].mvp;
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int cc = 0; cc < 4; cc++) m.r[r][cc] = scalar_load(mv + r * 4 + cc);
    return m;
}

// u or v -> 24.8 fixed-point pixels (extent: the target's width or height).  A vertex outside the guard band may overflow the
// conversion: its triangles take the clipper and never read the result.
__device__ __forceinline__ int32_t snap(float u, float extent) { return (int32_t)rintf((u * extent) * 256.0f); }

// ---- clipper kernel (rare path) ---------------------------------------------------------------
__device__ __forceinline__ float clip_dist(const f4& v, int k)
{
    switch (k) {
    case 0: return v.w - v.z;
    case 1: return v.z;
    case 2: return GUARD_BAND * v.w + v.x;
    case 3: return GUARD_BAND * v.w - v.x;
    case 4: return GUARD_BAND * v.w + v.y;
    default: return GUARD_BAND * v.w - v.y;
    }
}

__device__ __forceinline__ f4 clip_intersect(const f4& in, const f4& out, float din, float dout)
{
    const float t = din / (din - dout);
    f4 r;
    r.x = in.x + (out.x - in.x) * t;
    r.y = in.y + (out.y - in.y) * t;
    r.z = in.z + (out.z - in.z) * t;
    r.w = in.w + (out.w - in.w) * t;
    return r;
}

// The polygon being clipped (Sutherland-Hodgman ping-pong, <= 3 + 6 vertices) is indexed dynamically, which in registers means
// scratch memory (round 2: 592 bytes per lane).  It lives in LDS instead, slot-major ([buffer][vertex][thread]: consecutive
// threads in consecutive banks); one wave per clip block works, which bounds the arrays to 38 KB.
#define CLIP_MAXV 10
#define CLIP_THREADS 64u
// LDS polygon storage of STRIDE threads (thread tl): two ping-pong buffers of clip-space vertices + texture coordinates, and
// the projected vertices of the result
template <uint32_t STRIDE>
struct ClipLds {
    float4* poly; float* pu; float* pv; int32_t* px; int32_t* py; float* pd; uint32_t tl;
    __device__ __forceinline__ float4& P(int bf, int i) const { return poly[((uint32_t)bf * CLIP_MAXV + (uint32_t)i) * STRIDE + tl]; }
    __device__ __forceinline__ float& U(int bf, int i) const { return pu[((uint32_t)bf * CLIP_MAXV + (uint32_t)i) * STRIDE + tl]; }
    __device__ __forceinline__ float& V(int bf, int i) const { return pv[((uint32_t)bf * CLIP_MAXV + (uint32_t)i) * STRIDE + tl]; }
    __device__ __forceinline__ int32_t& X(int i) const { return px[(uint32_t)i * STRIDE + tl]; }
    __device__ __forceinline__ int32_t& Y(int i) const { return py[(uint32_t)i * STRIDE + tl]; }
    __device__ __forceinline__ float& D(int i) const { return pd[(uint32_t)i * STRIDE + tl]; }
};

// One triangle of a cluster through the homogeneous clipper: its vertices are transformed again from the position stream (the
// clip-space z is not kept by the setup kernels), clipped against near / far (unless depth-clamped) and the guard band, and
// projected + snapped into L.X / L.Y / L.D.  Returns the vertex count of the resulting polygon (a fan around vertex 0), 0 when
// nothing is left; `cur` is the buffer that holds its clip-space vertices and texture coordinates.
template <uint32_t STRIDE, class Prm>
__device__ __forceinline__ int clip_triangle(const Prm& p, const ClipLds<STRIDE>& L, uint32_t dataOffset, uint32_t vertexBase, uint32_t V, uint32_t tri,
                                             const Mat4& mvp, bool masked, int& cur)
{
    const uint32_t packedIdx = p.meshletData[dataOffset + V + tri];
    for (int i = 0; i < 3; i++) {
        const uint32_t li = (packedIdx >> (8 * i)) & 0xFFu;
        const uint32_t vi = p.meshletData[dataOffset + li] + vertexBase;
        const float* pos = p.positions + (size_t)vi * 3;
        const f4 h = mul_mv(mvp, pos[0], pos[1], pos[2], 1.0f);
        L.P(0, i) = make_float4(h.x, h.y, h.z, h.w);
        float u = 0.0f, v = 0.0f;
        if (masked && p.texcoords) { u = p.texcoords[(size_t)vi * 2]; v = p.texcoords[(size_t)vi * 2 + 1]; }
        L.U(0, i) = u; L.V(0, i) = v;
    }
    int np = 3;
    cur = 0;
    for (int pl = p.depthClamp ? 2 : 0; pl < 6 && np >= 3; pl++) {
        int m2 = 0;
        for (int i = 0; i < np; i++) {
            const int j = (i + 1) % np;
            const float4 Pv = L.P(cur, i), Qv = L.P(cur, j);
            const f4 P = {Pv.x, Pv.y, Pv.z, Pv.w}, Q = {Qv.x, Qv.y, Qv.z, Qv.w};
            const float pui = L.U(cur, i), pvi = L.V(cur, i), puj = L.U(cur, j), pvj = L.V(cur, j);
            const float dp = clip_dist(P, pl), dq = clip_dist(Q, pl);
            const bool pin = dp >= 0.0f, qin = dq >= 0.0f;
            if (pin && m2 < CLIP_MAXV) { L.U(cur ^ 1, m2) = pui; L.V(cur ^ 1, m2) = pvi; L.P(cur ^ 1, m2) = Pv; m2++; }
            if (pin && !qin && m2 < CLIP_MAXV) {
                const float t = dp / (dp - dq);
                L.U(cur ^ 1, m2) = pui + (puj - pui) * t; L.V(cur ^ 1, m2) = pvi + (pvj - pvi) * t;
                const f4 x = clip_intersect(P, Q, dp, dq);
                L.P(cur ^ 1, m2) = make_float4(x.x, x.y, x.z, x.w); m2++;
            } else if (!pin && qin && m2 < CLIP_MAXV) {
                const float t = dq / (dq - dp);
                L.U(cur ^ 1, m2) = puj + (pui - puj) * t; L.V(cur ^ 1, m2) = pvj + (pvi - pvj) * t;
                const f4 x = clip_intersect(Q, P, dq, dp);
                L.P(cur ^ 1, m2) = make_float4(x.x, x.y, x.z, x.w); m2++;
            }
        }
        np = m2; cur ^= 1;
    }
    if (np < 3) return 0;
    for (int i = 0; i < np; i++) {
        const float4 h = L.P(cur, i);
        if (!(h.w > 0.0f)) return 0;
        const float u = h.x / fabsf(h.w) * 0.5f + 0.5f;
        const float v = h.y / fabsf(h.w) * -0.5f + 0.5f;
        L.X(i) = snap(u, p.W);
        L.Y(i) = snap(v, p.H);
        L.D(i) = h.z / h.w;
    }
    return np;
}

// The pieces of a clipped polygon (a fan around its vertex 0, clip_triangle): set up, stored as 48-byte records (+ the mask
// extension) and binned by the lane itself.  listShard: the record list shard the pieces go to.
template <uint32_t STRIDE, class P>
__device__ __forceinline__ void clip_emit(const P& p, const ClipLds<STRIDE>& L, int np, int cur, uint32_t payload, bool twoSided, bool masked,
                                          uint32_t matFlags, uint32_t listShard)
{
    const uint32_t slots = masked ? 1u + CHORD_MASK_EXT_SLOTS : 1u;
    for (int i = 1; i + 1 < np; i++) {
        TriSetup ts;
        ts.X[0] = L.X(0); ts.X[1] = L.X(i); ts.X[2] = L.X(i + 1);
        ts.Y[0] = L.Y(0); ts.Y[1] = L.Y(i); ts.Y[2] = L.Y(i + 1);
        float d[3] = {L.D(0), L.D(i), L.D(i + 1)};
        ts.payload = payload;
        if (!tri_setup(ts, twoSided, p.Wi, p.Hi) || !owns_rect(p.shard, ts.px0, ts.py0, ts.px1, ts.py1)) continue;
        if (p.biasConst != 0.0f || p.biasSlope != 0.0f) { const float o = depth_bias(ts, d, p.biasConst, p.biasSlope); d[0] += o; d[1] += o; d[2] += o; }
        const uint32_t li = atomicAdd(&p.counters->triCount[listShard * CHORD_SHARD_STRIDE], slots);
        if (li + slots > p.triCap) { atomicOr(&p.counters->overflow, 1u); continue; }
        const uint32_t gi = listShard * p.triCap + li;
        write_record(&p.tris[gi], ts, d, twoSided, masked);
        if (masked) {
            const uint32_t material = CHORD_MATFLAG_MATERIAL(matFlags);
            const float u3[3] = {L.U(cur, 0), L.U(cur, i), L.U(cur, i + 1)}, v3[3] = {L.V(cur, 0), L.V(cur, i), L.V(cur, i + 1)};
            const float w3[3] = {L.P(cur, 0).w, L.P(cur, i).w, L.P(cur, i + 1).w};
            write_mask_ext(&p.tris[gi + 1u], &p.materials[material], material, ts.area, u3, v3, w3);
        }
        // clipped pieces are rare: binned right here, one (scattered) atomic per tile they may touch
        bin_record_tiles(p, ts, gi | (masked ? CHORD_REC_MASKED : CHORD_REC_WIDE));   // clipped pieces take the 48-byte form
    }
}

// One entry of the clip list through the clipper: the cluster's records, matrix and flags, then clip_triangle + clip_emit.
// MASKED = false: the scene has no alpha-tested material (the record kernel's plain instantiation).
template <bool MASKED, uint32_t STRIDE, class P>
__device__ __forceinline__ void clip_entry(const P& p, const ClipLds<STRIDE>& L, const ClipTri ct, uint32_t listShard)
{
    const DMeshlet& m = p.meshlets[ct.meshletId];
    const uint32_t V = m.vertexTriangleCount & 0xFFu;
    const uint32_t matFlags = p.objStatic[ct.objectId].matFlags;
    const bool twoSided = (matFlags & CHORD_MATFLAG_TWO_SIDED) != 0u || p.depthOnly != 0u;
    const bool masked = MASKED && CHORD_MATFLAG_ALPHA(matFlags) == CHORD_ALPHA_MASK;
    const float* mv = p.objFrame[ct.objectId].mvp;
    Mat4 mvp;
    for (int r = 0; r < 4; r++) for (int cc = 0; cc < 4; cc++) mvp.r[r][cc] = mv[r * 4 + cc];
    int cur;
    const int np = clip_triangle(p, L, m.dataOffset, m.vertexBase, V, ct.tri, mvp, masked, cur);
    if (np < 3) return;
    const uint32_t payload = p.depthOnly ? 0u : encode_triangle_instance(ct.tri, ct.slot);
    clip_emit(p, L, np, cur, payload, twoSided, masked, matFlags, listShard);
}

// What the set-up wave needs to clip and emit the clip triangles of its clusters (the record emission's parameters + the scene's),
// read from the kernel-argument segment where it is used (RecordEmitParams)
struct SetupClipParams : RecordEmitParams {
    const DObjFrame* objFrame; const DObjStatic* objStatic; const DMeshlet* meshlets;
    const uint32_t* meshletData; const float* positions; const float* texcoords; const DMaterial* materials;
    uint32_t depthOnly; float W, H; int32_t Wi, Hi; uint32_t depthClamp; float biasConst, biasSlope;
};
__device__ __forceinline__ SetupClipParams load_setup_clip_params()
{
    const RasterParams* q = kernel_args();
    SetupClipParams c;
    static_cast<RecordEmitParams&>(c) = load_record_emit_params();
    c.objFrame = scalar_load(&q->objFrame); c.objStatic = scalar_load(&q->objStatic); c.meshlets = scalar_load(&q->meshlets); c.depthOnly = scalar_load(&q->depthOnly);
    c.meshletData = scalar_load(&q->meshletData); c.positions = scalar_load(&q->positions); c.texcoords = scalar_load(&q->texcoords);
    c.materials = scalar_load(&q->materials);
    c.W = scalar_load(&q->W); c.H = scalar_load(&q->H); c.Wi = scalar_load(&q->Wi); c.Hi = scalar_load(&q->Hi);
    c.depthClamp = scalar_load(&q->depthClamp); c.biasConst = scalar_load(&q->biasConst); c.biasSlope = scalar_load(&q->biasSlope);
    return c;
}

// ---- edge functions of wide triangles; one lane scans a narrow triangle ---------------------------------------------
struct WideEdges {
    int64_t a[3], b[3], bias[3], dx[3], dy[3];
    int32_t Xa[3], Ya[3];
    int32_t s;
};

__device__ __forceinline__ void wide_edges(const TriSetup& ts, WideEdges& w)
{
    const int ea[3] = {1, 2, 0}, eb[3] = {2, 0, 1};
    w.s = ts.s;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        w.dx[i] = (int64_t)(ts.X[eb[i]] - ts.X[ea[i]]);
        w.dy[i] = (int64_t)(ts.Y[eb[i]] - ts.Y[ea[i]]);
        w.Xa[i] = ts.X[ea[i]]; w.Ya[i] = ts.Y[ea[i]];
        w.a[i] = -(int64_t)ts.s * w.dy[i];
        w.b[i] = (int64_t)ts.s * w.dx[i];
        w.bias[i] = (w.a[i] > 0 || (w.a[i] == 0 && w.b[i] > 0)) ? 0 : -1;
    }
}

__device__ __forceinline__ int64_t edge_at(const WideEdges& w, int i, int32_t px, int32_t py)
{
    const int64_t cx = (int64_t)px * 256 + 128, cy = (int64_t)py * 256 + 128;
    return (int64_t)w.s * (w.dx[i] * (cy - w.Ya[i]) - w.dy[i] * (cx - w.Xa[i]));
}

__device__ __forceinline__ void lds_write(unsigned long long* tile, int32_t lx, int32_t ly, float z, uint32_t payload)
{
    const unsigned long long packed = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)payload;
    atomicMax(&tile[ly * TPITCH + lx], packed);            // ds_max_u64
}

// one lane scans its own (tile-clipped) tiny bbox with 32-bit edge functions.  ONE flattened loop over the
// bbox pixels: with nested row/column loops a wave pays max(rows) x max(cols) over its lanes (a 1x16 and a
// 16x1 box in the same wave = 256 trips); flattened it pays max(area) <= the tile's tiny-area threshold.
template <int PITCH>
__device__ __forceinline__ void tile_raster_narrow(unsigned long long* tile, const TriSetup& ts, int32_t ox, int32_t oy,
                                                   int32_t x0, int32_t y0, int32_t x1, int32_t y1, bool noPixels, const bool clampZ)
{
    // (32-bit multiplies are quarter rate on this GPU; every product here has factors below 2^23 -- vertices at most 64 px
    // apart, a pixel centre inside their bbox -- and takes the full-rate 24-bit form; +-s is a select, not a multiply)
    const bool neg = ts.s < 0;
    const int32_t dx0 = ts.X[2] - ts.X[1], dy0 = ts.Y[2] - ts.Y[1];
    const int32_t dx1 = ts.X[0] - ts.X[2], dy1 = ts.Y[0] - ts.Y[2];
    const int32_t dx2 = ts.X[1] - ts.X[0], dy2 = ts.Y[1] - ts.Y[0];
    const int32_t a0 = neg ? dy0 : -dy0, b0 = neg ? -dx0 : dx0;
    const int32_t a1 = neg ? dy1 : -dy1, b1 = neg ? -dx1 : dx1;
    const int32_t a2 = neg ? dy2 : -dy2, b2 = neg ? -dx2 : dx2;
    const int32_t bias0 = (a0 > 0 || (a0 == 0 && b0 > 0)) ? 0 : -1;
    const int32_t bias1 = (a1 > 0 || (a1 == 0 && b1 > 0)) ? 0 : -1;
    const int32_t bias2 = (a2 > 0 || (a2 == 0 && b2 > 0)) ? 0 : -1;
    const int32_t cx0 = x0 * 256 + 128, cy0 = y0 * 256 + 128;
    // s * (dx * (cy - Y) - dy * (cx - X)) = b * (cy - Y) + a * (cx - X)
    int32_t r0 = __mul24(b0, cy0 - ts.Y[1]) + __mul24(a0, cx0 - ts.X[1]) + bias0;   // bias folded in: inside <=> all >= 0
    int32_t r1 = __mul24(b1, cy0 - ts.Y[2]) + __mul24(a1, cx0 - ts.X[2]) + bias1;
    int32_t r2 = __mul24(b2, cy0 - ts.Y[0]) + __mul24(a2, cx0 - ts.X[0]) + bias2;
    int32_t E0 = r0, E1 = r1, E2 = r2;
    const int32_t w = x1 - x0 + 1, count = __mul24(w, y1 - y0 + 1);
    // step to the next pixel / from the last pixel of a row to the first of the next; the body is branch-free:
    // a pixel outside the triangle merges 0, which ds_max ignores
    const int32_t sx0 = a0 * 256, sx1 = a1 * 256, sx2 = a2 * 256;
    const int32_t sw0 = b0 * 256 - __mul24(w - 1, sx0), sw1 = b1 * 256 - __mul24(w - 1, sx1), sw2 = b2 * 256 - __mul24(w - 1, sx2);
    int32_t col = 0;
    unsigned long long* px = tile + (y0 - oy) * PITCH + (x0 - ox);
    const unsigned long long payload = (unsigned long long)ts.payload;
    for (int32_t i = 0; i < count; i++) {
        const bool inside = (E0 | E1 | E2) >= 0 && !noPixels;
        const float l1 = (float)(E1 - bias1) * ts.invA, l2 = (float)(E2 - bias2) * ts.invA;
        float z = (ts.d0 + l1 * ts.e1) + l2 * ts.e2;
        if (clampZ) z = fminf(fmaxf(z, 0.0f), 1.0f);
        atomicMax(px, inside ? (((unsigned long long)__float_as_uint(z) << 32) | payload) : 0ull);   // ds_max_u64
        col++;
        const bool wrap = col == w;
        E0 += wrap ? sw0 : sx0; E1 += wrap ? sw1 : sx1; E2 += wrap ? sw2 : sx2;
        px += wrap ? PITCH - w + 1 : 1;
        col = wrap ? 0 : col;
    }
}

} // namespace chord
