// chordvis -- the ray scene's TLAS topology built on the device (chordvis_rebuild_ray_tlas; include/chordvis.h RAY QUERIES, "rebuilding
// the TLAS"; ray_tlas_shape.h).  The tree is a pure function of the object boxes (tests/spec_ray_tlas_np.py): objects in
// ascending (Morton key of the box centre, index) order, four to a node, level by level.  Everything runs on the context's stream
// and nothing is read back; ray_refit_kernel (kernels_rays.hip), launched last and unchanged, fills the boxes.
//
//   ray_tlas_group_kernel     at most CHORD_RAY_TLAS_GROUP_MAX objects: ONE workgroup of 1 024 lanes does everything before the refit.
//                             Centres stay in registers, their bounds are LDS atomics, the (key << 32 | index) words are sorted by a
//                             bitonic network in 32 KB of LDS, and the sorted words become the node table and the leaf references.
//   ray_tlas_centres_kernel   more objects: a lane per object writes the centre and folds it into six bounds words -- LDS atomics
//                             within the workgroup, then one vector atomicMin / atomicMax per word and workgroup on global memory.
//   ray_tlas_hist_kernel      } an LSD radix sort of the 30 key bits, 8 bits a pass (8, 8, 8, 6), from index order: stable passes give
//   ray_tlas_scan_kernel      } the (key, index) order.  A workgroup owns kTlasSortItems consecutive positions; hist counts its digits
//   ray_tlas_scatter_kernel   } (the first pass forms the keys on the way), scan turns the (digit, workgroup) table into offsets in one
//                             workgroup, scatter ranks a wave's lanes among equal digits with ballots -- in position order, so the pass
//                             is stable -- and moves key and index.
//   ray_tlas_nodes_kernel     a lane per node and per sorted position: node words, zeroed arrival counters, leaf references; it also
//                             resets the bounds words for the next rebuild.
//
// The launch count is a function of the object count alone (ray::tlas_launches).  Every loop over a table is bounded by a count the
// host passed; every index that came out of memory is compared with the count of the array it goes into before it is used.

#include "device_layer.h"
#include "device_math.h"
#include "ray_scene.h"
#include "ray_tlas_shape.h"
#include "ray_walk.h"

namespace chord {

struct RayTlasArgs {
    const ChordObject* objects;
    const DObjStatic* objStatic;
    ray::Node* nodes;
    uint32_t* leafRef;             // per object: node * 4 + slot
    uint32_t* counters;            // per node: the refit's arrivals, zero when the refit starts
    uint32_t* bounds;              // six words: tlas_mono of the centre minima, then of the maxima (the sort path)
    float* centres;                // three per object (the sort path)
    const uint32_t* keysIn; uint32_t* keysOut;
    const uint32_t* valsIn; uint32_t* valsOut;
    uint32_t* table;               // [digit][workgroup]: counts, then offsets
    ray::TlasShape shape;
    uint32_t sortGroups;           // workgroups of a sort pass
    uint32_t shift, digitBits;     // of the pass
};

// the centre of object o's box: the refit's box (ray_refit_kernel), then ray::tlas_centre per axis
__device__ __forceinline__ void object_centre(const RayTlasArgs& a, uint32_t o, float c[3])
{
    const DObjStatic& st = a.objStatic[o];
    const Mat4 M = load_mat(a.objects[o].basicData.localToTranslatedWorld);
    f3 cen, ext;
    aabb_center_extent(st.posMin, st.posMax, cen, ext);
    float lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 8; k++) box_corner(cen, ext, M, k, lo, hi);
#pragma unroll
    for (int i = 0; i < 3; i++) c[i] = ray::tlas_centre(lo[i], hi[i]);
}

__device__ __forceinline__ void store_node(ray::Node* dst, const ray::Node& nd)
{
    const uint4* s = reinterpret_cast<const uint4*>(&nd);
    uint4* d = reinterpret_cast<uint4*>(dst);
#pragma unroll
    for (int i = 0; i < 8; i++) d[i] = s[i];
}

// ---- one workgroup -----------------------------------------------------------------------------------------------------------------

constexpr uint32_t kGroupThreads = 1024u;
constexpr uint32_t kGroupSlots = CHORD_RAY_TLAS_GROUP_MAX > 0u ? CHORD_RAY_TLAS_GROUP_MAX : kGroupThreads;
constexpr uint32_t kGroupPer = kGroupSlots / kGroupThreads;
static_assert(kGroupSlots % kGroupThreads == 0u && (kGroupSlots & (kGroupSlots - 1u)) == 0u, "CHORD_RAY_TLAS_GROUP_MAX: a power of two, a multiple of 1 024");
static_assert(kGroupSlots * 8u + 64u <= 65536u, "the sort's words must fit 64 KB of LDS");

__global__ __launch_bounds__(kGroupThreads) void ray_tlas_group_kernel(const RayTlasArgs a)
{
    __shared__ unsigned long long sKeys[kGroupSlots];
    __shared__ uint32_t sBounds[6];
    const uint32_t t = threadIdx.x;
    const uint32_t n = a.shape.cnt[0] < kGroupSlots ? a.shape.cnt[0] : kGroupSlots;
    if (t < 3u) { sBounds[t] = 0xFFFFFFFFu; sBounds[3u + t] = 0u; }
    __syncthreads();

    float c[kGroupPer][3];
#pragma unroll
    for (uint32_t r = 0; r < kGroupPer; r++) {
        const uint32_t o = t + r * kGroupThreads;
        c[r][0] = c[r][1] = c[r][2] = 0.0f;
        if (o < n) {
            object_centre(a, o, c[r]);
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const uint32_t m = ray::tlas_mono(c[r][i]);
                atomicMin(&sBounds[i], m);
                atomicMax(&sBounds[3 + i], m);
            }
        }
    }
    __syncthreads();
    float blo[3], bhi[3];
#pragma unroll
    for (int i = 0; i < 3; i++) { blo[i] = ray::tlas_unmono(sBounds[i]); bhi[i] = ray::tlas_unmono(sBounds[3 + i]); }

    uint32_t P = 1u;                                       // the network's size: the power of two at or above n
    for (uint32_t k = 0; k < 32u && P < n; k++) P <<= 1;
#pragma unroll
    for (uint32_t r = 0; r < kGroupPer; r++) {
        const uint32_t o = t + r * kGroupThreads;
        if (o < P) sKeys[o] = o < n ? ((unsigned long long)ray::tlas_key(c[r], blo, bhi) << 32) | o : ~0ull;
    }
    __syncthreads();

    // bitonic network, ascending: the words are unique (the index is in them), so the result is THE (key, index) order
    for (uint32_t k = 2u; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            for (uint32_t e = t; e < (P >> 1); e += kGroupThreads) {
                const uint32_t i = ((e & ~(j - 1u)) << 1) | (e & (j - 1u)), p = i + j;
                const unsigned long long x = sKeys[i], y = sKeys[p];
                const bool up = (i & k) == 0u;
                if ((x > y) == up) { sKeys[i] = y; sKeys[p] = x; }
            }
            __syncthreads();
        }
    }

    const auto order = [&](uint32_t p) -> uint32_t { return p < n ? (uint32_t)sKeys[p] : 0u; };
    for (uint32_t g = t; g < a.shape.nodes; g += kGroupThreads) {
        ray::Node nd;
        ray::tlas_node_words(a.shape, g, order, nd);
        store_node(a.nodes + g, nd);
        a.counters[g] = 0u;
    }
    for (uint32_t p = t; p < n; p += kGroupThreads) {
        const uint32_t o = (uint32_t)sKeys[p];
        if (o < n) a.leafRef[o] = ray::tlas_leaf_ref(a.shape, p);
    }
}

// ---- many workgroups ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void ray_tlas_centres_kernel(const RayTlasArgs a)
{
    __shared__ uint32_t sBounds[6];
    const uint32_t t = threadIdx.x, n = a.shape.cnt[0];
    const uint32_t o = blockIdx.x * 256u + t;
    if (t < 3u) { sBounds[t] = 0xFFFFFFFFu; sBounds[3u + t] = 0u; }
    __syncthreads();
    if (o < n) {
        float c[3];
        object_centre(a, o, c);
#pragma unroll
        for (int i = 0; i < 3; i++) {
            a.centres[3u * o + i] = c[i];
            const uint32_t m = ray::tlas_mono(c[i]);
            atomicMin(&sBounds[i], m);
            atomicMax(&sBounds[3 + i], m);
        }
    }
    __syncthreads();
    if (t < 3u) atomicMin(&a.bounds[t], sBounds[t]);
    else if (t < 6u) atomicMax(&a.bounds[t], sBounds[t]);
}

template <bool FIRST>
__global__ __launch_bounds__(256) void ray_tlas_hist_kernel(const RayTlasArgs a)
{
    __shared__ uint32_t sHist[256];
    const uint32_t t = threadIdx.x, n = a.shape.cnt[0];
    sHist[t] = 0u;
    __syncthreads();
    float blo[3] = {0.0f, 0.0f, 0.0f}, bhi[3] = {0.0f, 0.0f, 0.0f};
    if (FIRST) {
#pragma unroll
        for (int i = 0; i < 3; i++) { blo[i] = ray::tlas_unmono(a.bounds[i]); bhi[i] = ray::tlas_unmono(a.bounds[3 + i]); }
    }
    const uint32_t mask = (1u << a.digitBits) - 1u;
    for (uint32_t r = 0; r < ray::kTlasSortItems / 256u; r++) {
        const uint32_t idx = blockIdx.x * ray::kTlasSortItems + r * 256u + t;
        if (idx >= n) break;
        uint32_t key;
        if (FIRST) {
            const float c[3] = {a.centres[3u * idx], a.centres[3u * idx + 1u], a.centres[3u * idx + 2u]};
            key = ray::tlas_key(c, blo, bhi);
            a.keysOut[idx] = key;
        } else key = a.keysIn[idx];
        atomicAdd(&sHist[(key >> a.shift) & mask], 1u);
    }
    __syncthreads();
    a.table[t * a.sortGroups + blockIdx.x] = sHist[t];
}

// exclusive prefix sums over the table in (digit, workgroup) order, in place: one workgroup, a run of consecutive entries per lane
__global__ __launch_bounds__(1024) void ray_tlas_scan_kernel(const RayTlasArgs a)
{
    __shared__ uint32_t sSum[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t entries = 256u * a.sortGroups;
    const uint32_t per = (entries + 1023u) / 1024u;
    const uint32_t first = t * per < entries ? t * per : entries;
    const uint32_t last = first + per < entries ? first + per : entries;
    uint32_t sum = 0u;
    for (uint32_t e = first; e < last; e++) sum += a.table[e];
    sSum[t] = sum;
    __syncthreads();
    for (uint32_t d = 1u; d < 1024u; d <<= 1) {
        const uint32_t add = t >= d ? sSum[t - d] : 0u;
        __syncthreads();
        sSum[t] += add;
        __syncthreads();
    }
    uint32_t run = sSum[t] - sum;
    for (uint32_t e = first; e < last; e++) { const uint32_t v = a.table[e]; a.table[e] = run; run += v; }
}

template <bool FIRST>
__global__ __launch_bounds__(256) void ray_tlas_scatter_kernel(const RayTlasArgs a)
{
    __shared__ uint32_t sBase[256];            // where the workgroup's next item of a digit goes
    __shared__ uint32_t sWave[4][256];         // per wave of the round: count, then offset
    const uint32_t t = threadIdx.x, n = a.shape.cnt[0];
    const uint32_t wave = t >> 6, lane = t & 63u;
    const uint32_t mask = (1u << a.digitBits) - 1u;
    sBase[t] = a.table[t * a.sortGroups + blockIdx.x];
    for (uint32_t r = 0; r < ray::kTlasSortItems / 256u; r++) {
        const uint32_t idx = blockIdx.x * ray::kTlasSortItems + r * 256u + t;
        if (blockIdx.x * ray::kTlasSortItems + r * 256u >= n) break;             // (the whole workgroup alike)
#pragma unroll
        for (uint32_t w = 0; w < 4u; w++) sWave[w][t] = 0u;
        __syncthreads();
        const bool valid = idx < n;
        const uint32_t key = valid ? a.keysIn[idx] : 0u;
        const uint32_t val = valid ? (FIRST ? idx : a.valsIn[idx]) : 0u;
        const uint32_t digit = (key >> a.shift) & mask;
        // the lanes of this wave that hold the same digit
        unsigned long long peers = __ballot(valid);
        for (uint32_t b = 0; b < 8u; b++) {
            const bool bit = ((digit >> b) & 1u) != 0u;
            const unsigned long long set = __ballot(valid && bit);
            peers &= bit ? set : ~set;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        if (valid && rank == 0u) sWave[wave][digit] = (uint32_t)__popcll(peers);
        __syncthreads();
        {
            uint32_t run = sBase[t];
#pragma unroll
            for (uint32_t w = 0; w < 4u; w++) { const uint32_t cnt = sWave[w][t]; sWave[w][t] = run; run += cnt; }
            sBase[t] = run;
        }
        __syncthreads();
        if (valid) {
            const uint32_t dst = sWave[wave][digit] + rank;
            if (dst < n) { a.keysOut[dst] = key; a.valsOut[dst] = val; }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void ray_tlas_nodes_kernel(const RayTlasArgs a)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x, n = a.shape.cnt[0];
    const uint32_t* sorted = a.valsIn;
    if (g < a.shape.nodes) {
        const auto order = [&](uint32_t p) -> uint32_t { return p < n ? sorted[p] : 0u; };
        ray::Node nd;
        ray::tlas_node_words(a.shape, g, order, nd);
        store_node(a.nodes + g, nd);
        a.counters[g] = 0u;
    }
    if (g < n) {
        const uint32_t o = sorted[g];
        if (o < n) a.leafRef[o] = ray::tlas_leaf_ref(a.shape, g);
    }
    if (g < 3u) a.bounds[g] = 0xFFFFFFFFu;
    else if (g < 6u) a.bounds[g] = 0u;
}

// The launches of one rebuild before the refit: ray::tlas_launches(n) - 1 of them.  The context's rebuild buffers hold at least
// c->objectCount objects (abi_raytlas.cpp grew them).
void launch_ray_tlas_rebuild(ChordCtx* c, const ray::TlasShape& shape)
{
    RayTlasArgs a = {};
    a.objects = c->dObjects; a.objStatic = c->dObjStatic;
    a.nodes = c->dRayTlas; a.leafRef = c->dRayLeafRef; a.counters = c->dRayCounters;
    a.shape = shape;
    const uint32_t n = shape.cnt[0];
    if (n <= CHORD_RAY_TLAS_GROUP_MAX) {
        CHORD_LAUNCH(c, ray_tlas_group_kernel, dim3(1), dim3(kGroupThreads), 0, c->stream, a);
        return;
    }
    const ray::TlasScratch lay = ray::tlas_scratch(c->rayRebuildCapacity);
    uint32_t* s = c->dRayRebuildScratch;
    a.bounds = s + lay.bounds; a.centres = reinterpret_cast<float*>(s + lay.centres); a.table = s + lay.table;
    uint32_t* keys[2] = {s + lay.keysA, s + lay.keysB};
    uint32_t* vals[2] = {s + lay.valsA, s + lay.valsB};
    a.sortGroups = ray::tlas_sort_groups(n);
    CHORD_LAUNCH(c, ray_tlas_centres_kernel, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, a);
    for (uint32_t pass = 0; pass < ray::kTlasSortPasses; pass++) {
        a.shift = 8u * pass;
        a.digitBits = ray::kTlasKeyBits - a.shift < 8u ? ray::kTlasKeyBits - a.shift : 8u;
        a.keysIn = keys[pass & 1u]; a.keysOut = keys[(pass & 1u) ^ 1u];
        a.valsIn = vals[pass & 1u]; a.valsOut = vals[(pass & 1u) ^ 1u];
        if (pass == 0u) {
            RayTlasArgs h = a;
            h.keysOut = keys[0];                           // the first count forms the keys where the first scatter reads them
            CHORD_LAUNCH(c, ray_tlas_hist_kernel<true>, dim3(a.sortGroups), dim3(256), 0, c->stream, h);
        } else CHORD_LAUNCH(c, ray_tlas_hist_kernel<false>, dim3(a.sortGroups), dim3(256), 0, c->stream, a);
        CHORD_LAUNCH(c, ray_tlas_scan_kernel, dim3(1), dim3(1024), 0, c->stream, a);
        if (pass == 0u) CHORD_LAUNCH(c, ray_tlas_scatter_kernel<true>, dim3(a.sortGroups), dim3(256), 0, c->stream, a);
        else CHORD_LAUNCH(c, ray_tlas_scatter_kernel<false>, dim3(a.sortGroups), dim3(256), 0, c->stream, a);
    }
    a.valsIn = vals[ray::kTlasSortPasses & 1u];            // an even number of passes ends where it began
    const uint32_t lanes = n > shape.nodes ? n : shape.nodes;
    CHORD_LAUNCH(c, ray_tlas_nodes_kernel, dim3((lanes + 255u) / 256u), dim3(256), 0, c->stream, a);
}

} // namespace chord
