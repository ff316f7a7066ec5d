// chordvis -- the TLAS chordvis_rebuild_ray_tlas builds on the device (include/chordvis.h RAY QUERIES, "rebuilding the TLAS"; DESIGN.md
// 4.19; tests/spec_ray_tlas_np.py states the same in numpy).  The tree is a PURE FUNCTION OF THE OBJECT BOXES: objects in ascending
// (Morton key of the box centre, index) order, four to a leaf-level node, nodes four to a parent, level by level to one root.  So its
// shape -- levels, nodes per level, node numbers -- depends on the object count alone, and the host sizes buffers and launches from
// the count without reading anything back.  Plain C++ like ray_scene.h (no HIP header in here): the host layer, the kernels of
// kernels_raytlas.hip and the stand-alone program tests/ray_tlas_main.cpp all call these functions.
//
//   centre      c[a] = lo[a] * 0.5f + hi[a] * 0.5f of the refit's box (ray_walk.h box_corner)
//   bounds      Blo[a], Bhi[a]: min and max of c[a] under the total order of tlas_mono (the key of ray_scene.cpp equal_split): -0 below
//               +0, a NaN at an end.  An integer min / max, so arrival order does not matter
//   quantised   tlas_quantise: 10 bits per axis, 0 on an axis without a usable extent
//   key         tlas_morton: bit 3k + a of the 30-bit key is bit k of q[a]
//   levels      cnt[0] = n, cnt[j] = ceil(cnt[j-1] / 4) up to the first j >= 1 with cnt[j] == 1: the depth D; base[D] = 0,
//               base[j-1] = base[j] + cnt[j]; node (j, i) is base[j] + i, the root node 0
//   words       tlas_node_words; leaf references tlas_leaf_ref.  The boxes of used slots are the refit's to write.
// Arithmetic: binary32, one rounding per operation, no contraction.
#pragma once

#include <stdint.h>

#include "chordvis_types.h"
#include "ray_scene.h"

#if defined(__HIPCC__)
#define CHORD_TLAS_FN __host__ __device__ inline
#else
#define CHORD_TLAS_FN inline
#endif

namespace chord {
namespace ray {

constexpr uint32_t kTlasKeyBits = 30u;
constexpr uint32_t kTlasMaxObjects = 1u << (2u * kMaxDepth);       // 4^12

struct TlasShape {
    uint32_t depth;                    // D, 1 .. kMaxDepth
    uint32_t nodes;                    // cnt[1] + .. + cnt[D]
    uint32_t cnt[kMaxDepth + 1u];      // cnt[0] = objects; cnt[j > D] = 0
    uint32_t base[kMaxDepth + 2u];     // base[j] for 1 <= j <= D: the first node of level j; base[0] and base[j > D] = 0 (unused)
};

// 0: `s` is the shape over n objects; -4 (CHORDVIS_E_CAPACITY): n == 0 or more than 4^12 objects, `s` is all zero
CHORD_TLAS_FN int tlas_shape(uint64_t n, TlasShape& s)
{
    s.depth = 0u; s.nodes = 0u;
    for (uint32_t j = 0; j <= kMaxDepth; j++) s.cnt[j] = 0u;
    for (uint32_t j = 0; j <= kMaxDepth + 1u; j++) s.base[j] = 0u;
    if (n == 0u || n > kTlasMaxObjects) return -4;
    s.cnt[0] = (uint32_t)n;
    uint32_t d = 0u;
    for (uint32_t j = 1; j <= kMaxDepth; j++) {
        s.cnt[j] = (s.cnt[j - 1u] + 3u) / 4u;
        s.nodes += s.cnt[j];
        d = j;
        if (s.cnt[j] == 1u) break;
    }
    s.depth = d;                                                   // (n <= 4^12: cnt[12] == 1 at the latest)
    for (uint32_t j = d; j > 1u; j--) s.base[j - 1u] = s.base[j] + s.cnt[j];
    return 0;
}

CHORD_TLAS_FN uint32_t tlas_float_bits(float x) { uint32_t w; __builtin_memcpy(&w, &x, 4); return w; }
CHORD_TLAS_FN float tlas_bits_float(uint32_t w) { float x; __builtin_memcpy(&x, &w, 4); return x; }

// the float's bits made monotone, and back
CHORD_TLAS_FN uint32_t tlas_mono(float x) { const uint32_t u = tlas_float_bits(x); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
CHORD_TLAS_FN float tlas_unmono(uint32_t k) { return tlas_bits_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

CHORD_TLAS_FN float tlas_centre(float lo, float hi) { return lo * 0.5f + hi * 0.5f; }

// one axis of a centre against the centre bounds of that axis: 0 .. 1023 (the shape of ray_scene.cpp bin_of)
CHORD_TLAS_FN uint32_t tlas_quantise(float c, float blo, float bhi)
{
    const float extent = bhi - blo;
    if (!(extent > 0.0f) || !(extent < 3.0e38f)) return 0u;
    const float scale = 1024.0f / extent;
    const float f = (c - blo) * scale;
    return f > 0.0f ? (f < 1024.0f ? (uint32_t)f : 1023u) : 0u;
}

CHORD_TLAS_FN uint32_t tlas_spread3(uint32_t q)                   // bit k of q (k < 10) to bit 3k
{
    uint32_t m = 0u;
    for (uint32_t k = 0; k < 10u; k++) m |= ((q >> k) & 1u) << (3u * k);
    return m;
}

CHORD_TLAS_FN uint32_t tlas_morton(uint32_t qx, uint32_t qy, uint32_t qz) { return tlas_spread3(qx) | (tlas_spread3(qy) << 1) | (tlas_spread3(qz) << 2); }

CHORD_TLAS_FN uint32_t tlas_key(const float c[3], const float blo[3], const float bhi[3])
{
    return tlas_morton(tlas_quantise(c[0], blo[0], bhi[0]), tlas_quantise(c[1], blo[1], bhi[1]), tlas_quantise(c[2], blo[2], bhi[2]));
}

// the level of node g < s.nodes (at most kMaxDepth steps)
CHORD_TLAS_FN uint32_t tlas_node_level(const TlasShape& s, uint32_t g)
{
    uint32_t level = 1u;
    for (uint32_t j = 1; j <= kMaxDepth; j++)
        if (j <= s.depth && g >= s.base[j] && g - s.base[j] < s.cnt[j]) level = j;
    return level;
}

// Every word of node g < s.nodes but the boxes of its used slots, which get the empty box like the unused ones until the refit
// writes them.  order(p): the object at position p < s.cnt[0] of the sorted list (read for a level-1 node only).
template <typename Order>
CHORD_TLAS_FN void tlas_node_words(const TlasShape& s, uint32_t g, Order order, Node& nd)
{
    const uint32_t j = tlas_node_level(s, g), i = g - s.base[j];
    const uint32_t below = s.cnt[j - 1u], first = 4u * i;
    const uint32_t children = below - first < 4u ? below - first : 4u;
    for (uint32_t k = 0; k < 4u; k++) {
        for (int a = 0; a < 3; a++) { nd.lo[a][k] = __builtin_inff(); nd.hi[a][k] = -__builtin_inff(); }
        uint32_t w = kNoChild;
        if (k < children) w = j == 1u ? ((kTlasLeaf << kTagShift) | order(first + k)) : ((kTlasNode << kTagShift) | (s.base[j - 1u] + first + k));
        nd.child[k] = w;
    }
    nd.parentRef = j == s.depth ? kNoChild : (s.base[j + 1u] + (i >> 2)) * 4u + (i & 3u);
    nd.childCount = children;
    nd.pad[0] = 0u; nd.pad[1] = 0u;
}

// the leaf slot of the object at position p of the sorted list
CHORD_TLAS_FN uint32_t tlas_leaf_ref(const TlasShape& s, uint32_t p) { return (s.base[1] + (p >> 2)) * 4u + (p & 3u); }

// ---- what the host decides from the count alone ----

// nodes of the tree over n objects, 1 <= n <= 4^12 (0 otherwise)
CHORD_TLAS_FN uint32_t tlas_node_count(uint64_t n) { TlasShape s; return tlas_shape(n, s) ? 0u : s.nodes; }

constexpr uint32_t kTlasGroupMax = CHORD_RAY_TLAS_GROUP_MAX;       // at most this many objects: one workgroup sorts in LDS
constexpr uint32_t kTlasSortItems = 2048u;                         // above: positions a workgroup of a radix pass owns
constexpr uint32_t kTlasSortPasses = 4u;                           // 8 + 8 + 8 + 6 key bits (an even number: the order ends where it began)

CHORD_TLAS_FN uint32_t tlas_sort_groups(uint64_t n) { return (uint32_t)((n + kTlasSortItems - 1u) / kTlasSortItems); }

// kernel launches of one rebuild of n objects, the refit included
CHORD_TLAS_FN uint32_t tlas_launches(uint64_t n) { return n <= kTlasGroupMax ? 2u : 1u + 3u * kTlasSortPasses + 1u + 1u; }

// The sort's scratch for a capacity of `cap` objects, in 32-bit words from the buffer's start (nothing at or below the one-workgroup
// bound): the six bounds words (eight kept), the centres, two key and two index arrays, and the (digit, workgroup) table.
struct TlasScratch { uint64_t bounds, centres, keysA, keysB, valsA, valsB, table, words; };

CHORD_TLAS_FN TlasScratch tlas_scratch(uint64_t cap)
{
    TlasScratch l;
    l.bounds = 0u; l.centres = 8u;
    if (cap <= kTlasGroupMax) { l.keysA = l.keysB = l.valsA = l.valsB = l.table = 8u; l.words = 8u; return l; }
    l.keysA = l.centres + 3u * cap; l.keysB = l.keysA + cap; l.valsA = l.keysB + cap; l.valsB = l.valsA + cap;
    l.table = l.valsB + cap;
    l.words = l.table + 256u * (uint64_t)tlas_sort_groups(cap);
    return l;
}

} // namespace ray
} // namespace chord
