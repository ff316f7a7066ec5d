// chordvis -- the ray scene's trees (include/chordvis.h RAY QUERIES): the records the host builder (ray_scene.cpp,
// plain C++: no HIP header in here either) makes and the kernels of kernels_rays.hip walk.
//
// One tree shape serves both levels: a 4-wide node holds the BOXES OF ITS CHILDREN, axis by axis, so that a lane tests four children
// from six 16-byte loads.  A child word is pushable on the traversal stack as it is: bits 31..30 say what it names.
//   CHORD_RAY_TLAS_NODE  index of a TLAS node                 CHORD_RAY_TLAS_LEAF  index of an object of the current list
//   CHORD_RAY_BLAS_NODE  index of a BLAS node (all BLASes     CHORD_RAY_BLAS_LEAF  first triangle record << 2 | (count - 1),
//                        share one array)                                          count 1..4, records of all BLASes in one array
// 0xFFFFFFFF is "no child" (so the triangle array ends below 2^28 - 4 records).  A node box is the exact componentwise min / max of
// the boxes beneath it -- no padding: the traversal's answer must not depend on the tree.
#pragma once

#include <stdint.h>

#include <vector>

namespace chord {
namespace ray {

constexpr uint32_t kWidth = 4u;
constexpr uint32_t kLeafTriangles = 4u;
constexpr uint32_t kMaxDepth = 12u;             // CHORD_RAY_MAX_DEPTH: interior levels of one tree
constexpr uint32_t kStackEntries = 76u;         // >= 3 * (kMaxDepth + kMaxDepth) + 2: four children pushed, one popped, per level
constexpr uint32_t kNoChild = 0xFFFFFFFFu;
constexpr uint32_t kTagShift = 30u;
constexpr uint32_t kTlasNode = 0u, kTlasLeaf = 1u, kBlasNode = 2u, kBlasLeaf = 3u;
constexpr uint32_t kIndexMask = 0x3FFFFFFFu;
constexpr uint32_t kMaxTriangles = (1u << 28) - 4u;

struct Node {                  // 128 B
    float    lo[3][4];         // [axis][child]
    float    hi[3][4];
    uint32_t child[4];
    uint32_t parentRef;        // parent node * 4 + the slot this node's box lives in; kNoChild: the root
    uint32_t childCount;       // 1..4, the children are slots 0 .. childCount - 1
    uint32_t pad[2];
};
static_assert(sizeof(Node) == 128, "ray::Node");

struct Triangle {              // 48 B: positions as uploaded, and what a hit reports
    float    v[9];
    uint32_t meshlet;          // index into the asset's meshlets
    uint32_t triangle;         // index within the meshlet
    uint32_t pad;
};
static_assert(sizeof(Triangle) == 48, "ray::Triangle");

struct Box { float lo[3], hi[3]; };

inline float fmin_(float a, float b) { return a < b ? a : b; }
inline float fmax_(float a, float b) { return a > b ? a : b; }

inline Box triangle_box(const Triangle& t)
{
    Box b;
    for (int a = 0; a < 3; a++) {
        b.lo[a] = fmin_(fmin_(t.v[a], t.v[3 + a]), t.v[6 + a]);
        b.hi[a] = fmax_(fmax_(t.v[a], t.v[3 + a]), t.v[6 + a]);
    }
    return b;
}

// Interior levels a subtree over n items takes when every split is an equal-count one (the bound the builder keeps: a binned
// surface-area split is taken only where the levels left still allow the equal-count finish of every child).
uint32_t balanced_levels(uint64_t n, uint32_t leafItems);

struct Tree {
    std::vector<Node> nodes;           // node 0 is the root (always a node: one object or one triangle is a root with one leaf child)
    std::vector<uint32_t> order;       // the items in leaf order
    std::vector<uint32_t> leafRef;     // per item: node * 4 + slot of the leaf child that holds it
    Box rootBox;
    uint32_t depth = 0;                // interior levels
};

// A deterministic 4-wide tree over `count` >= 1 boxes: leaves of at most leafItems items (1 or kLeafTriangles).  Child words are
// (nodeTag << 30 | nodeBase + node) and (leafTag << 30 | leaf word): the leaf word is itemBase + the item's own index for
// leafItems == 1, else (itemBase + first position in `order`) << 2 | (count - 1).  0: built; -4 (CHORDVIS_E_CAPACITY): deeper than
// kMaxDepth even with equal-count splits.
int build_tree(const Box* boxes, uint32_t count, uint32_t leafItems, uint32_t nodeTag, uint32_t leafTag, uint32_t nodeBase, uint32_t itemBase, Tree& out);

} // namespace ray
} // namespace chord
