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
//   ray_trace_kernel    wave64, a ray per lane, a stack of ray::kStackEntries words per lane in scratch (DESIGN.md 4.16 says why).  One
//                       loop pops TLAS nodes, TLAS leaves, BLAS nodes and BLAS leaves alike: a child word carries its kind.  Popping a
//                       TLAS leaf forms the local ray and the object interval and pushes the primitive's BLAS root; the stack discipline
//                       finishes that BLAS before the next TLAS entry comes up.  Children are pushed far to near (a speed choice: the
//                       answer is the brute-force specification's for any order, tests/spec_rays_np.py).
//
// Arithmetic: binary32, no contraction, correctly rounded divide, subnormals kept; min and max are the selects `a < b ? a : b` and
// `a > b ? a : b` of the specification (so a NaN behaves the same on both sides), never fminf / fmaxf.

#include "device_layer.h"
#include "device_math.h"
#include "ray_scene.h"

namespace chord {

namespace {

__device__ __forceinline__ float rmin(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float rmax(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

struct Interval { float n, f; };

// one axis of the slab test: r = 1 / d of that axis, rf = r is finite
__device__ __forceinline__ void slab_axis(float lo, float hi, float o, float r, bool rf, float& n, float& f)
{
    if (rf) {
        const float a = (lo - o) * r, b = (hi - o) * r;
        n = rmin(a, b); f = rmax(a, b);
    } else {
        const bool inside = lo <= o && o <= hi;
        n = inside ? -__builtin_inff() : __builtin_inff();
        f = inside ? __builtin_inff() : -__builtin_inff();
    }
}

struct RayAxes { float o[3], r[3]; bool rf[3]; };

__device__ __forceinline__ Interval slab(const RayAxes& ray, const float lo[3], const float hi[3])
{
    float n[3], f[3];
#pragma unroll
    for (int a = 0; a < 3; a++) slab_axis(lo[a], hi[a], ray.o[a], ray.r[a], ray.rf[a], n[a], f[a]);
    Interval iv;
    iv.n = rmax(rmax(n[0], n[1]), n[2]);
    iv.f = rmin(rmin(f[0], f[1]), f[2]);
    return iv;
}

__device__ __forceinline__ void make_axes(RayAxes& ax, const float o[3], const float d[3])
{
#pragma unroll
    for (int a = 0; a < 3; a++) { ax.o[a] = o[a]; ax.r[a] = 1.0f / d[a]; ax.rf[a] = finite_f(ax.r[a]); }
}

} // namespace

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
    for (int k = 0; k < 8; k++) {
        const f3 q = extent_corner(c, e, k);
        const f4 h = mul_mv(M, q.x, q.y, q.z, 1.0f);
        const float p[3] = {h.x, h.y, h.z};
#pragma unroll
        for (int i = 0; i < 3; i++) {
            lo[i] = k == 0 ? p[i] : rmin(lo[i], p[i]);
            hi[i] = k == 0 ? p[i] : rmax(hi[i], p[i]);
        }
    }
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
#pragma unroll
        for (int i = 0; i < 3; i++) {
            float l = nd.lo[i][0], h = nd.hi[i][0];
            for (uint32_t k = 1; k < children; k++) { l = rmin(l, nd.lo[i][k]); h = rmax(h, nd.hi[i][k]); }
            lo[i] = l; hi[i] = h;
        }
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

namespace {

struct Best {
    float t, u, v;
    uint32_t object, meshlet, triangle, status;
};

// the four children of a node against a ray: which to visit, pushed far to near
template <bool BLAS>
__device__ __forceinline__ void visit_node(const ray::Node* __restrict__ node, const RayAxes& ax, float nO, float fO, float tMin, float limit,
                                           uint32_t* stack, uint32_t& sp)
{
    const float4* v = reinterpret_cast<const float4*>(node);
    const float4 lx = v[0], ly = v[1], lz = v[2], hx = v[3], hy = v[4], hz = v[5];
    const uint4 ch = reinterpret_cast<const uint4*>(node)[6];
    const float lo4[3][4] = {{lx.x, lx.y, lx.z, lx.w}, {ly.x, ly.y, ly.z, ly.w}, {lz.x, lz.y, lz.z, lz.w}};
    const float hi4[3][4] = {{hx.x, hx.y, hx.z, hx.w}, {hy.x, hy.y, hy.z, hy.w}, {hz.x, hz.y, hz.z, hz.w}};
    const uint32_t child[4] = {ch.x, ch.y, ch.z, ch.w};
    float key[4];
    uint32_t word[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float lo[3] = {lo4[0][k], lo4[1][k], lo4[2][k]}, hi[3] = {hi4[0][k], hi4[1][k], hi4[2][k]};
        const Interval iv = slab(ax, lo, hi);
        // a BLAS interval counts after the clamp into the object's interval, like the t of the triangles beneath it
        const float n = BLAS ? rmin(rmax(iv.n, nO), fO) : iv.n, f = BLAS ? rmin(rmax(iv.f, nO), fO) : iv.f;
        const bool skip = child[k] == ray::kNoChild || iv.n > iv.f || f < tMin || n > limit;
        word[k] = skip ? ray::kNoChild : child[k];
        key[k] = n;
    }
    // far to near: a sorting network over (key, word), skipped children last in, first out of consideration
#define RAY_SWAP(i, j)                                                                                                        \
    {                                                                                                                         \
        const bool sw = word[i] == ray::kNoChild ? false : (word[j] == ray::kNoChild ? true : key[i] < key[j]);                \
        const float ka = sw ? key[j] : key[i], kb = sw ? key[i] : key[j];                                                     \
        const uint32_t wa = sw ? word[j] : word[i], wb = sw ? word[i] : word[j];                                              \
        key[i] = ka; key[j] = kb; word[i] = wa; word[j] = wb;                                                                 \
    }
    RAY_SWAP(0, 1) RAY_SWAP(2, 3) RAY_SWAP(0, 2) RAY_SWAP(1, 3) RAY_SWAP(1, 2)
#undef RAY_SWAP
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (word[k] != ray::kNoChild && sp < ray::kStackEntries) stack[sp++] = word[k];
}

} // namespace

template <bool ANY>
__global__ __launch_bounds__(64) void ray_trace_kernel(const RayTraceArgs a)
{
    const uint64_t i = (uint64_t)blockIdx.x * 64u + threadIdx.x;          // (count may be any uint32: 2 i + 1 does not fit 32 bits)
    if (i >= a.count) return;
    const float4 r0 = a.rays[2u * i], r1 = a.rays[2u * i + 1u];
#if CHORD_RAY_COUNTERS
    unsigned long long nTlas = 0ull, nBlas = 0ull, nTris = 0ull, nLeaves = 0ull;
#endif
    const float o[3] = {r0.x, r0.y, r0.z}, d[3] = {r1.x, r1.y, r1.z};
    const float tMin = r0.w, tMax = r1.w;

    Best best;
    best.t = __builtin_inff(); best.u = 0.0f; best.v = 0.0f; best.object = 0u; best.meshlet = 0u; best.triangle = 0u; best.status = 0u;

    RayAxes world;
    make_axes(world, o, d);
    bool live = finite_f(r0.x) && finite_f(r0.y) && finite_f(r0.z) && finite_f(r0.w) && finite_f(r1.x) && finite_f(r1.y) && finite_f(r1.z) && finite_f(r1.w);
    live = live && (world.rf[0] || world.rf[1] || world.rf[2]) && !(tMin > tMax);

    uint32_t stack[ray::kStackEntries];
    uint32_t sp = 0;
    if (live) stack[sp++] = (ray::kTlasNode << ray::kTagShift) | 0u;

    // the object whose BLAS is being walked
    RayAxes local;
    float dl[3] = {0.0f, 0.0f, 0.0f};
    float nO = 0.0f, fO = 0.0f;
    uint32_t object = 0u;
#pragma unroll
    for (int k = 0; k < 3; k++) { local.o[k] = 0.0f; local.r[k] = 0.0f; local.rf[k] = false; }

    while (sp > 0u) {
        const uint32_t w = stack[--sp];
        const uint32_t tag = w >> ray::kTagShift, idx = w & ray::kIndexMask;
        // the best t so far bounds what is still worth a visit; the comparison is strict, so that ties are still visited
        const float limit = rmin(best.t, tMax);
        if (tag == ray::kTlasNode) {
#if CHORD_RAY_COUNTERS
            nTlas++;
#endif
            if (idx < a.tlasNodes) visit_node<false>(a.tlas + idx, world, 0.0f, 0.0f, tMin, limit, stack, sp);
        } else if (tag == ray::kTlasLeaf) {
            if (idx >= a.objectCount) continue;
#if CHORD_RAY_COUNTERS
            nLeaves++;
#endif
            const float4 b0 = a.leafBox[2u * idx], b1 = a.leafBox[2u * idx + 1u];
            const float lo[3] = {b0.x, b0.y, b0.z}, hi[3] = {b1.x, b1.y, b1.z};
            const Interval iv = slab(world, lo, hi);
            if (iv.n > iv.f || iv.f < tMin || iv.n > limit) continue;
            const uint32_t prim = a.objStatic[idx].prim;
            const uint32_t root = prim < a.primCount ? a.blasRoot[prim] : ray::kNoChild;
            if (root == ray::kNoChild) continue;
            const Mat4 W = load_mat(a.objects[idx].basicData.translatedWorldToLocal);
            const f4 ol = mul_mv(W, o[0], o[1], o[2], 1.0f);
            float olv[3] = {ol.x, ol.y, ol.z};
#pragma unroll
            for (int r = 0; r < 3; r++) dl[r] = (W.r[r][0] * d[0] + W.r[r][1] * d[1]) + W.r[r][2] * d[2];
            make_axes(local, olv, dl);
            nO = iv.n; fO = iv.f; object = idx;
            if (sp < ray::kStackEntries) stack[sp++] = root;
        } else if (tag == ray::kBlasNode) {
#if CHORD_RAY_COUNTERS
            nBlas++;
#endif
            if (idx < a.blasNodes) visit_node<true>(a.blas + idx, local, nO, fO, tMin, limit, stack, sp);
        } else {
            const uint32_t first = idx >> 2, n = (idx & 3u) + 1u;
            for (uint32_t k = 0; k < n; k++) {
                if (first + k >= a.triangleCount) break;
#if CHORD_RAY_COUNTERS
                nTris++;
#endif
                const float4* tv = a.triangles + 3ull * (first + k);
                const float4 t0 = tv[0], t1 = tv[1], t2 = tv[2];
                const float v0[3] = {t0.x, t0.y, t0.z}, v1[3] = {t0.w, t1.x, t1.y}, v2[3] = {t1.z, t1.w, t2.x};
                const uint32_t meshlet = __float_as_uint(t2.y), triangle = __float_as_uint(t2.z);
                float blo[3], bhi[3];
#pragma unroll
                for (int c = 0; c < 3; c++) { blo[c] = rmin(rmin(v0[c], v1[c]), v2[c]); bhi[c] = rmax(rmax(v0[c], v1[c]), v2[c]); }
                const Interval it = slab(local, blo, bhi);
                if (it.n > it.f) continue;
                const float e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]}, e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
                const float p[3] = {dl[1] * e2[2] - dl[2] * e2[1], dl[2] * e2[0] - dl[0] * e2[2], dl[0] * e2[1] - dl[1] * e2[0]};
                const float det = (e1[0] * p[0] + e1[1] * p[1]) + e1[2] * p[2];
                if (det == 0.0f || !finite_f(det)) continue;
                const float inv = 1.0f / det;
                const float s[3] = {local.o[0] - v0[0], local.o[1] - v0[1], local.o[2] - v0[2]};
                const float u = ((s[0] * p[0] + s[1] * p[1]) + s[2] * p[2]) * inv;
                if (!(0.0f <= u && u <= 1.0f)) continue;
                const float q[3] = {s[1] * e1[2] - s[2] * e1[1], s[2] * e1[0] - s[0] * e1[2], s[0] * e1[1] - s[1] * e1[0]};
                const float v = ((dl[0] * q[0] + dl[1] * q[1]) + dl[2] * q[2]) * inv;
                if (!(v >= 0.0f && u + v <= 1.0f)) continue;
                const float tMT = ((e2[0] * q[0] + e2[1] * q[1]) + e2[2] * q[2]) * inv;
                const float t = rmin(rmax(rmin(rmax(tMT, it.n), it.f), nO), fO);
                if (!(t >= tMin && t <= tMax)) continue;
                if (ANY) { best.status = 1u; sp = 0u; break; }
                bool better = best.status == 0u || t < best.t;
                if (!better && t == best.t) {
                    better = object < best.object || (object == best.object && (meshlet < best.meshlet || (meshlet == best.meshlet && triangle < best.triangle)));
                }
                if (better) {
                    best.t = t; best.u = u; best.v = v; best.object = object; best.meshlet = meshlet; best.triangle = triangle;
                    best.status = 1u | (det < 0.0f ? 2u : 0u);
                }
            }
        }
    }

    uint4 h0 = make_uint4(0u, 0u, 0u, 0u), h1 = make_uint4(0u, 0u, 0u, 0u);
    if (best.status != 0u) {
        if (ANY) h1.w = 1u;
        else {
            h0 = make_uint4(__float_as_uint(best.t), __float_as_uint(best.u), __float_as_uint(best.v), best.object);
            h1 = make_uint4(best.meshlet, best.triangle, a.objStatic[best.object].prim, best.status);
        }
    }
    a.hits[2u * i] = h0;
    a.hits[2u * i + 1u] = h1;
#if CHORD_RAY_COUNTERS
    atomicAdd(&a.counters[0], 1ull); atomicAdd(&a.counters[8], nTlas); atomicAdd(&a.counters[16], nLeaves);
    atomicAdd(&a.counters[24], nBlas); atomicAdd(&a.counters[32], nTris);
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
