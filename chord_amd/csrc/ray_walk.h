// chordvis -- one ray through the ray scene's trees, and one object's box (chordvis_trace_rays, chordvis_refit_ray_scene; include/
// chordvis.h RAY QUERIES).  The answer is tests/spec_rays_np.trace's word for word.  Everything here is float32 /
// integer C++ in source order behind __device__, so the host compiler builds it too: tests/ray_walk_main.cpp runs walk_ray under the
// address and undefined-behaviour sanitizers over arrays of exactly their size -- the stack among them -- and kernels_rays.hip runs
// the same statements a ray per lane.
//
//   walk_ray     wave64 on the device, a ray per lane, a stack of ray::kStackEntries words per lane (DESIGN.md 4.16 says why).  One
//                loop pops TLAS nodes, TLAS leaves, BLAS nodes and BLAS leaves alike: a child word carries its kind.  Popping a TLAS
//                leaf forms the local ray and the object interval and pushes the primitive's BLAS root; the stack discipline finishes
//                that BLAS before the next TLAS entry comes up.  Children are pushed far to near (a speed choice: the answer is the
//                brute-force specification's for any order, tests/spec_rays_np.py).
//   box_corner   a corner of a primitive's bounds through localToTranslatedWorld in the object stage's arithmetic (extent_corner,
//                mul_mv), folded into the componentwise min / max that is the object's box; node_union: what the refit's climb
//                forms of a node's children.
//
// Every index is compared with the COUNT of its array before it is used.  `Stats` is told of every node, leaf and triangle visited
// and of every push BEFORE it happens (with the stack pointer of that moment): the kernel passes RayNoStats, which does nothing; the
// measuring build (CHORD_RAY_COUNTERS) and the host program pass types that count.
//
// Arithmetic: binary32, no contraction, correctly rounded divide, subnormals kept; min and max are the selects `a < b ? a : b` and
// `a > b ? a : b` of the specification (so a NaN behaves the same on both sides), never fminf / fmaxf.
#pragma once

#include "device_layer.h"
#include "device_math.h"
#include "ray_scene.h"

namespace chord {

__device__ __forceinline__ float rmin(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float rmax(float a, float b) { return a > b ? a : b; }
__device__ static inline uint32_t rw_bits(float x) { uint32_t w; __builtin_memcpy(&w, &x, 4); return w; }
__device__ __forceinline__ bool finite_f(float x) { return (rw_bits(x) & 0x7F800000u) != 0x7F800000u; }

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

// One corner of an object's box: corner k of the bounds (centre c, extent e: aabb_center_extent) under M = localToTranslatedWorld,
// folded into lo / hi.  The box is k = 0 .. 7 in turn.  (The loop over k stays with the caller: inside a function of this header it
// compiles to other, equivalent, instructions in ray_refit_kernel.)
__device__ __forceinline__ void box_corner(f3 c, f3 e, const Mat4& M, int k, float lo[3], float hi[3])
{
    const f3 q = extent_corner(c, e, k);
    const f4 h = mul_mv(M, q.x, q.y, q.z, 1.0f);
    const float p[3] = {h.x, h.y, h.z};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        lo[i] = k == 0 ? p[i] : rmin(lo[i], p[i]);
        hi[i] = k == 0 ? p[i] : rmax(hi[i], p[i]);
    }
}

// the union of a node's `children` child boxes
__device__ __forceinline__ void node_union(const ray::Node& nd, uint32_t children, float lo[3], float hi[3])
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
        float l = nd.lo[i][0], h = nd.hi[i][0];
        for (uint32_t k = 1; k < children; k++) { l = rmin(l, nd.lo[i][k]); h = rmax(h, nd.hi[i][k]); }
        lo[i] = l; hi[i] = h;
    }
}

struct RayWalkScene {              // pointers and the counts of what they point at
    const ChordObject* objects;
    const DObjStatic* objStatic;
    const ray::Node* tlas;
    const float4* leafBox;         // per object: lo.xyz, hi.xyz in two vectors
    const uint32_t* blasRoot;      // per primitive: the child word of its BLAS root, ray::kNoChild: no LOD-0 triangle
    const ray::Node* blas;
    const float4* triangles;       // ray::Triangle as three vectors
    uint32_t objectCount, primCount, tlasNodes, blasNodes, triangleCount;
};

struct RayNoStats {
    __device__ __forceinline__ void tlas_node() {}
    __device__ __forceinline__ void tlas_leaf() {}
    __device__ __forceinline__ void blas_node() {}
    __device__ __forceinline__ void triangle() {}
    __device__ __forceinline__ void push(uint32_t) {}      // sp before the push: sp == ray::kStackEntries is a push the stack refuses
};

struct RayWords { uint4 h0, h1; };       // a ChordRayHit as two vectors

struct Best {
    float t, u, v;
    uint32_t object, meshlet, triangle, status;
};

// the four children of a node against a ray: which to visit, pushed far to near
template <bool BLAS, typename Stats>
__device__ __forceinline__ void visit_node(const ray::Node* __restrict__ node, const RayAxes& ax, float nO, float fO, float tMin, float limit,
                                           uint32_t* stack, uint32_t& sp, Stats& stats)
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
    for (int k = 0; k < 4; k++) {
        if (word[k] != ray::kNoChild) stats.push(sp);
        if (word[k] != ray::kNoChild && sp < ray::kStackEntries) stack[sp++] = word[k];
    }
}

// One ray, whole: r0 = (origin, tMin), r1 = (direction, tMax), the two halves of a ChordRay; the answer's h0 = (t, u, v, object), h1 =
// (meshlet, triangle, primitive, status), the two halves of its ChordRayHit.  `a` names the arrays and their counts: a RayWalkScene,
// or the kernel's own argument record, which has the same members.  stack: ray::kStackEntries words of the caller's.
template <bool ANY, typename Scene, typename Stats>
__device__ __forceinline__ RayWords walk_ray(const Scene& a, const float4& r0, const float4& r1, uint32_t* stack, Stats& stats)
{
    const float o[3] = {r0.x, r0.y, r0.z}, d[3] = {r1.x, r1.y, r1.z};
    const float tMin = r0.w, tMax = r1.w;

    Best best;
    best.t = __builtin_inff(); best.u = 0.0f; best.v = 0.0f; best.object = 0u; best.meshlet = 0u; best.triangle = 0u; best.status = 0u;

    RayAxes world;
    make_axes(world, o, d);
    bool live = finite_f(r0.x) && finite_f(r0.y) && finite_f(r0.z) && finite_f(r0.w) && finite_f(r1.x) && finite_f(r1.y) && finite_f(r1.z) && finite_f(r1.w);
    live = live && (world.rf[0] || world.rf[1] || world.rf[2]) && !(tMin > tMax);

    uint32_t sp = 0;
    if (live) { stats.push(sp); stack[sp++] = (ray::kTlasNode << ray::kTagShift) | 0u; }

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
            stats.tlas_node();
            if (idx < a.tlasNodes) visit_node<false>(a.tlas + idx, world, 0.0f, 0.0f, tMin, limit, stack, sp, stats);
        } else if (tag == ray::kTlasLeaf) {
            if (idx >= a.objectCount) continue;
            stats.tlas_leaf();
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
            stats.push(sp);
            if (sp < ray::kStackEntries) stack[sp++] = root;
        } else if (tag == ray::kBlasNode) {
            stats.blas_node();
            if (idx < a.blasNodes) visit_node<true>(a.blas + idx, local, nO, fO, tMin, limit, stack, sp, stats);
        } else {
            const uint32_t first = idx >> 2, n = (idx & 3u) + 1u;
            for (uint32_t k = 0; k < n; k++) {
                if (first + k >= a.triangleCount) break;
                stats.triangle();
                const float4* tv = a.triangles + 3ull * (first + k);
                const float4 t0 = tv[0], t1 = tv[1], t2 = tv[2];
                const float v0[3] = {t0.x, t0.y, t0.z}, v1[3] = {t0.w, t1.x, t1.y}, v2[3] = {t1.z, t1.w, t2.x};
                const uint32_t meshlet = rw_bits(t2.y), triangle = rw_bits(t2.z);
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
            h0 = make_uint4(rw_bits(best.t), rw_bits(best.u), rw_bits(best.v), best.object);
            h1 = make_uint4(best.meshlet, best.triangle, a.objStatic[best.object].prim, best.status);
        }
    }
    RayWords out; out.h0 = h0; out.h1 = h1;
    return out;
}

} // namespace chord
