// chordvis -- host builder of the ray scene's trees (ray_scene.h).  Plain C++: no HIP header, so that a host compiler
// builds it alone (tests/ray_build_main.cpp runs it under the address and undefined-behaviour sanitizers).
//
// build_tree: top down.  A node's range of items is cut in two and each half in two again (a half that fits a leaf stays whole): two to
// four children.  A cut is a binned surface-area split -- 16 bins over the centroid bounds on each axis, the cheapest of the 45 planes
// by area(left) * count(left) + area(right) * count(right), ties to the lower axis and plane -- and falls back to an EQUAL-COUNT split
// (stable sort by centroid on the widest axis, cut in the middle) whenever a side would be empty: coincident items cannot deepen the
// tree beyond the logarithm of their count.  Depth is bounded the same way: a node keeps its surface-area cuts only if every child can
// still be finished by equal-count cuts within kMaxDepth levels; otherwise the node is cut again by equal counts, whose children can.
// Everything is a function of the input alone (stable partitions, no hashing, no threads): two builds are byte-identical.

#include "ray_scene.h"

#include <algorithm>
#include <cstring>

namespace chord {
namespace ray {

uint32_t balanced_levels(uint64_t n, uint32_t leafItems)
{
    uint32_t levels = 0;
    while (n > leafItems) { n = ((n + 1u) / 2u + 1u) / 2u; levels++; }
    return levels;
}

namespace {

constexpr int kBins = 16;

struct Builder {
    const Box* boxes;
    uint32_t leafItems, nodeTag, leafTag, nodeBase, itemBase;
    Tree* out;
    std::vector<float> centroid;       // 3 per item
    std::vector<uint32_t> scratch;

    static Box empty_box()
    {
        Box b;
        for (int a = 0; a < 3; a++) { b.lo[a] = __builtin_inff(); b.hi[a] = -__builtin_inff(); }
        return b;
    }
    static void grow(Box& b, const Box& o)
    {
        for (int a = 0; a < 3; a++) { b.lo[a] = fmin_(b.lo[a], o.lo[a]); b.hi[a] = fmax_(b.hi[a], o.hi[a]); }
    }
    static double half_area(const Box& b)
    {
        const double x = (double)b.hi[0] - b.lo[0], y = (double)b.hi[1] - b.lo[1], z = (double)b.hi[2] - b.lo[2];
        const double a = x * y + y * z + z * x;
        return a == a && a >= 0.0 && a < 1.0e300 ? a : 1.0e300;       // (an overflowing or non-finite box: any finite cost beats it)
    }

    // [b, e) -> [b, mid), [mid, e), b < mid < e, by equal counts along the widest centroid axis
    uint32_t equal_split(uint32_t b, uint32_t e)
    {
        uint32_t* ord = out->order.data();
        float lo[3], hi[3];
        for (int a = 0; a < 3; a++) { lo[a] = __builtin_inff(); hi[a] = -__builtin_inff(); }
        for (uint32_t i = b; i < e; i++)
            for (int a = 0; a < 3; a++) { const float c = centroid[3u * ord[i] + a]; lo[a] = fmin_(lo[a], c); hi[a] = fmax_(hi[a], c); }
        int axis = 0;
        for (int a = 1; a < 3; a++) if (hi[a] - lo[a] > hi[axis] - lo[axis]) axis = a;
        // (by a total key -- the float's bits made monotone -- so that a NaN position, which an upload does not refuse, still leaves
        // the comparator a strict weak order: NaNs sort to the ends, the numbers as numbers, -0 just before +0)
        const float* cen = centroid.data();
        auto key = [cen, axis](uint32_t x) {
            uint32_t u;
            std::memcpy(&u, &cen[3u * x + axis], 4);
            return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
        };
        std::stable_sort(ord + b, ord + e, [key](uint32_t x, uint32_t y) { return key(x) < key(y); });
        return b + (e - b + 1u) / 2u;
    }

    // the binned surface-area split; returns b when no plane leaves both sides non-empty
    uint32_t sah_split(uint32_t b, uint32_t e)
    {
        uint32_t* ord = out->order.data();
        float lo[3], hi[3];
        for (int a = 0; a < 3; a++) { lo[a] = __builtin_inff(); hi[a] = -__builtin_inff(); }
        for (uint32_t i = b; i < e; i++)
            for (int a = 0; a < 3; a++) { const float c = centroid[3u * ord[i] + a]; lo[a] = fmin_(lo[a], c); hi[a] = fmax_(hi[a], c); }
        double bestCost = 0.0;
        int bestAxis = -1, bestPlane = 0;
        float bestScale = 0.0f;
        for (int a = 0; a < 3; a++) {
            const float extent = hi[a] - lo[a];
            if (!(extent > 0.0f) || !(extent < 3.0e38f)) continue;
            const float scale = (float)kBins / extent;
            Box bin[kBins];
            uint32_t cnt[kBins];
            for (int k = 0; k < kBins; k++) { bin[k] = empty_box(); cnt[k] = 0; }
            for (uint32_t i = b; i < e; i++) {
                const int k = bin_of(centroid[3u * ord[i] + a], lo[a], scale);
                grow(bin[k], boxes[ord[i]]);
                cnt[k]++;
            }
            double rightArea[kBins];
            uint32_t rightCnt[kBins];
            Box acc = empty_box();
            uint32_t n = 0;
            for (int k = kBins - 1; k > 0; k--) { grow(acc, bin[k]); n += cnt[k]; rightArea[k] = half_area(acc); rightCnt[k] = n; }
            acc = empty_box(); n = 0;
            for (int k = 1; k < kBins; k++) {                  // plane k: bins [0, k) | [k, kBins)
                grow(acc, bin[k - 1]); n += cnt[k - 1];
                if (n == 0 || rightCnt[k] == 0) continue;
                const double cost = half_area(acc) * (double)n + rightArea[k] * (double)rightCnt[k];
                if (bestAxis < 0 || cost < bestCost) { bestCost = cost; bestAxis = a; bestPlane = k; bestScale = scale; }
            }
        }
        if (bestAxis < 0) return b;
        const float* cen = centroid.data();
        const float l = lo[bestAxis];
        const int axis = bestAxis, plane = bestPlane;
        const float scale = bestScale;
        uint32_t* mid = std::stable_partition(ord + b, ord + e, [cen, axis, l, scale, plane](uint32_t x) { return bin_of(cen[3u * x + axis], l, scale) < plane; });
        return (uint32_t)(mid - ord);
    }
    static int bin_of(float c, float lo, float scale)
    {
        const float f = (c - lo) * scale;
        int k = f > 0.0f ? (f < (float)kBins ? (int)f : kBins - 1) : 0;       // (NaN: bin 0)
        return k < kBins ? k : kBins - 1;
    }

    uint32_t split(uint32_t b, uint32_t e, bool equalOnly)
    {
        if (!equalOnly) {
            const uint32_t mid = sah_split(b, e);
            if (mid > b && mid < e) return mid;
        }
        return equal_split(b, e);
    }

    // the node over [b, e) at `level` (the root is level 0); returns its box
    Box build_node(uint32_t node, uint32_t b, uint32_t e, uint32_t level, uint32_t parentRef)
    {
        uint32_t cut[5];
        uint32_t parts = 0;
        for (int attempt = 0; attempt < 2; attempt++) {
            const bool equalOnly = attempt == 1;
            parts = 0;
            if (e - b <= leafItems) { cut[0] = b; cut[1] = e; parts = 1; break; }     // (only the root: a tree of one leaf)
            const uint32_t mid = split(b, e, equalOnly);
            cut[parts++] = b;
            if (mid - b > leafItems) cut[parts++] = split(b, mid, equalOnly);
            cut[parts++] = mid;
            if (e - mid > leafItems) cut[parts++] = split(mid, e, equalOnly);
            cut[parts] = e;
            bool fits = true;
            for (uint32_t k = 0; k < parts; k++)
                fits = fits && level + 1u + balanced_levels(cut[k + 1] - cut[k], leafItems) <= kMaxDepth;
            if (fits) break;                                   // (the equal-count attempt always does: its children are the bound's own)
        }
        if (out->depth < level + 1u) out->depth = level + 1u;
        {
            Node& nd = out->nodes[node];
            std::memset(&nd, 0, sizeof(nd));
            nd.parentRef = parentRef;
            nd.childCount = parts;
            for (int a = 0; a < 3; a++) for (uint32_t k = 0; k < kWidth; k++) { nd.lo[a][k] = __builtin_inff(); nd.hi[a][k] = -__builtin_inff(); }
            for (uint32_t k = 0; k < kWidth; k++) nd.child[k] = kNoChild;
        }
        Box whole = empty_box();
        for (uint32_t k = 0; k < parts; k++) {
            const uint32_t cb = cut[k], ce = cut[k + 1];
            Box cbx;
            uint32_t word;
            if (ce - cb <= leafItems) {
                cbx = empty_box();
                for (uint32_t i = cb; i < ce; i++) { grow(cbx, boxes[out->order[i]]); out->leafRef[out->order[i]] = node * kWidth + k; }
                word = leafItems == 1u ? (leafTag << kTagShift) | (itemBase + out->order[cb])
                                       : (leafTag << kTagShift) | ((itemBase + cb) << 2) | (ce - cb - 1u);
            } else {
                const uint32_t child = (uint32_t)out->nodes.size();
                out->nodes.push_back(Node{});
                cbx = build_node(child, cb, ce, level + 1u, node * kWidth + k);
                word = (nodeTag << kTagShift) | (nodeBase + child);
            }
            Node& nd = out->nodes[node];                       // (the vector may have grown)
            for (int a = 0; a < 3; a++) { nd.lo[a][k] = cbx.lo[a]; nd.hi[a][k] = cbx.hi[a]; }
            nd.child[k] = word;
            grow(whole, cbx);
        }
        return whole;
    }
};

} // namespace

int build_tree(const Box* boxes, uint32_t count, uint32_t leafItems, uint32_t nodeTag, uint32_t leafTag, uint32_t nodeBase, uint32_t itemBase, Tree& out)
{
    out = Tree{};
    if (count == 0 || leafItems == 0 || leafItems > kLeafTriangles) return -1;
    if (balanced_levels(count, leafItems) > kMaxDepth) return -4;
    Builder bl;
    bl.boxes = boxes; bl.leafItems = leafItems; bl.nodeTag = nodeTag; bl.leafTag = leafTag; bl.nodeBase = nodeBase; bl.itemBase = itemBase;
    bl.out = &out;
    bl.centroid.resize((size_t)count * 3u);
    for (uint32_t i = 0; i < count; i++)
        for (int a = 0; a < 3; a++) bl.centroid[3u * i + a] = boxes[i].lo[a] * 0.5f + boxes[i].hi[a] * 0.5f;
    out.order.resize(count);
    for (uint32_t i = 0; i < count; i++) out.order[i] = i;
    out.leafRef.assign(count, kNoChild);
    out.nodes.reserve((size_t)count / 2u + 2u);
    out.nodes.push_back(Node{});
    out.rootBox = bl.build_node(0u, 0u, count, 0u, kNoChild);
    return out.depth <= kMaxDepth ? 0 : -4;
}

} // namespace ray
} // namespace chord
