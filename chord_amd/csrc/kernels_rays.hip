// chordvis -- ray queries on the resident scene (chordvis_refit_ray_scene, chordvis_trace_rays; include/chordvis.h RAY QUERIES;
// DESIGN.md 4.16).  The reference traces inline ray queries (TraceRayInline on topLevelAS: gi_rt_ao.hlsl, ddgi_probe_trace.hlsl, ...)
// against hardware acceleration structures; this part has no ray hardware, so the trees of ray_scene.h are walked by VALU code.
//
//   ray_refit_kernel    a lane per object of the current list.  It forms the object's box -- the eight corners of the primitive's bounds
//                       through localToTranslatedWorld in the object stage's arithmetic (aabb_center_extent, extent_corner, mul_mv), their
//                       componentwise min / max -- writes it to the leaf-box array and into its slot of the parent node, then climbs: an
//                       arrival counter per node, bumped with a device-scope acquire-release add; whoever brings it to the node's child
//                       count is the last arrival, sees every child box, resets the counter (no clear launch), forms the union, writes
//                       it into the node's slot of ITS parent and goes on; the others leave.  The root's union goes to the root record.
//   ray_trace_kernel    wave64, a ray per lane, a stack of ray::kStackEntries words per lane in scratch (DESIGN.md 4.16 says why): it
//                       loads the ray, calls walk_ray and stores the hit.
//
// The per-ray and per-box statements are ray_walk.h's (walk_ray, box_corner, node_union), which the host compiler builds too (tests/
// ray_walk_main.cpp); what stays here is indexing, loads and stores, the climb's atomics and the measuring build's sums.

#include "device_layer.h"
#include "device_math.h"
#include "ray_scene.h"
#include "ray_walk.h"

namespace chord {

struct RayRefitArgs {
    const ChordObject* objects;
    const DObjStatic* objStatic;
    ray::Node* nodes;
    const uint32_t* leafRef;       // per object: node * 4 + slot
    uint32_t* counters;            // per node, zero between launches
    float4* leafBox;               // per object: lo.xyz, hi.xyz in two vectors
    float4* root;                  // two vectors
    uint32_t objectCount, nodeCount;
};

__global__ __launch_bounds__(256) void ray_refit_kernel(const RayRefitArgs a)
{
    const uint32_t o = blockIdx.x * 256u + threadIdx.x;
    if (o >= a.objectCount) return;
    const DObjStatic& st = a.objStatic[o];
    const Mat4 M = load_mat(a.objects[o].basicData.localToTranslatedWorld);
    f3 c, e;
    aabb_center_extent(st.posMin, st.posMax, c, e);
    float lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 8; k++) box_corner(c, e, M, k, lo, hi);
    a.leafBox[2u * o] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    a.leafBox[2u * o + 1u] = make_float4(hi[0], hi[1], hi[2], 0.0f);

    uint32_t ref = a.leafRef[o];
    // (at most ray::kMaxDepth levels: the bound also ends the climb over a damaged table)
    for (uint32_t level = 0; level <= ray::kMaxDepth; level++) {
        const uint32_t node = ref >> 2, slot = ref & 3u;
        if (node >= a.nodeCount) return;
        ray::Node& nd = a.nodes[node];
#pragma unroll
        for (int i = 0; i < 3; i++) { nd.lo[i][slot] = lo[i]; nd.hi[i][slot] = hi[i]; }
        const uint32_t children = nd.childCount;
        // release: this lane's box is visible before the count; acquire: the last arrival sees every earlier arrival's box
        const uint32_t before = __hip_atomic_fetch_add(&a.counters[node], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (before + 1u != children) return;
        a.counters[node] = 0u;                                  // (the next launch is ordered behind this one by the stream)
        node_union(nd, children, lo, hi);
        ref = nd.parentRef;
        if (ref == ray::kNoChild) {
            a.root[0] = make_float4(lo[0], lo[1], lo[2], 0.0f);
            a.root[1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
            return;
        }
    }
}

struct RayTraceArgs {
    const float4* rays;            // ChordRay as two vectors
    uint4* hits;                   // ChordRayHit as two vectors
    const ChordObject* objects;
    const DObjStatic* objStatic;
    const ray::Node* tlas;
    const float4* leafBox;
    const uint32_t* blasRoot;      // per primitive: the child word of its BLAS root, ray::kNoChild: no LOD-0 triangle
    const ray::Node* blas;
    const float4* triangles;       // ray::Triangle as three vectors
    uint32_t count, objectCount, primCount, tlasNodes, blasNodes, triangleCount;
#if CHORD_RAY_COUNTERS
    unsigned long long* counters;  // the measuring build: CHORD_RAY_COUNTER_WORDS sums, one per 64-byte line
#endif
};

#if CHORD_RAY_COUNTERS
struct RayCountStats {
    unsigned long long nTlas = 0ull, nBlas = 0ull, nTris = 0ull, nLeaves = 0ull;
    __device__ __forceinline__ void tlas_node() { nTlas++; }
    __device__ __forceinline__ void tlas_leaf() { nLeaves++; }
    __device__ __forceinline__ void blas_node() { nBlas++; }
    __device__ __forceinline__ void triangle() { nTris++; }
    __device__ __forceinline__ void push(uint32_t) {}
};
#endif

template <bool ANY>
__global__ __launch_bounds__(64) void ray_trace_kernel(const RayTraceArgs a)
{
    const uint64_t i = (uint64_t)blockIdx.x * 64u + threadIdx.x;          // (count may be any uint32: 2 i + 1 does not fit 32 bits)
    if (i >= a.count) return;
    const float4 r0 = a.rays[2u * i], r1 = a.rays[2u * i + 1u];
#if CHORD_RAY_COUNTERS
    RayCountStats stats;
#else
    RayNoStats stats;
#endif
    uint32_t stack[ray::kStackEntries];
    const RayWords out = walk_ray<ANY>(a, r0, r1, stack, stats);
    a.hits[2u * i] = out.h0;
    a.hits[2u * i + 1u] = out.h1;
#if CHORD_RAY_COUNTERS
    atomicAdd(&a.counters[0], 1ull); atomicAdd(&a.counters[8], stats.nTlas); atomicAdd(&a.counters[16], stats.nLeaves);
    atomicAdd(&a.counters[24], stats.nBlas); atomicAdd(&a.counters[32], stats.nTris);
#endif
}

void launch_ray_refit(ChordCtx* c)
{
    RayRefitArgs a;
    a.objects = c->dObjects; a.objStatic = c->dObjStatic;
    a.nodes = c->dRayTlas; a.leafRef = c->dRayLeafRef; a.counters = c->dRayCounters;
    a.leafBox = reinterpret_cast<float4*>(c->dRayLeafBox); a.root = reinterpret_cast<float4*>(c->dRayRoot);
    a.objectCount = c->objectCount; a.nodeCount = c->rayTlasNodes;
    CHORD_LAUNCH(c, ray_refit_kernel, dim3((c->objectCount + 255u) / 256u), dim3(256), 0, c->stream, a);
}

void launch_ray_trace(ChordCtx* c, const ChordRay* rays, uint32_t count, bool anyHit, ChordRayHit* hits)
{
    RayTraceArgs a;
    a.rays = reinterpret_cast<const float4*>(rays); a.hits = reinterpret_cast<uint4*>(hits);
    a.objects = c->dObjects; a.objStatic = c->dObjStatic;
    a.tlas = c->dRayTlas; a.leafBox = reinterpret_cast<const float4*>(c->dRayLeafBox);
    a.blasRoot = c->dRayBlasRoot; a.blas = c->dRayBlas; a.triangles = reinterpret_cast<const float4*>(c->dRayTriangles);
    a.count = count; a.objectCount = c->objectCount; a.primCount = c->primCount;
    a.tlasNodes = c->rayTlasNodes; a.blasNodes = c->rayBlasNodes; a.triangleCount = c->rayBlasTriangles;
#if CHORD_RAY_COUNTERS
    a.counters = c->dRayCounts;
#endif
    const dim3 grid((uint32_t)(((uint64_t)count + 63u) / 64u)), block(64);
    if (anyHit) CHORD_LAUNCH(c, ray_trace_kernel<true>, grid, block, 0, c->stream, a);
    else CHORD_LAUNCH(c, ray_trace_kernel<false>, grid, block, 0, c->stream, a);
}

} // namespace chord
