// A program of its own over chord_amd/csrc/ray_scene.cpp (the host builder of the ray scene's trees): built by tests/test_ray_build.py
// with the host compiler under -fsanitize=address,undefined and run on the CPU.  It builds BLAS-shaped trees (leaves of up to four
// triangles) and TLAS-shaped trees (leaves of one box) and checks, from the nodes alone:
//   every item sits in exactly one leaf, and leafRef names that leaf;
//   every node's box -- kept in its parent's slot, the root's in Tree::rootBox -- is the exact union of its children's boxes, and a
//   leaf's box the exact union of its items' boxes;
//   parentRef and childCount are consistent, children come after their parent;
//   depth is what the tree says, within ray::kMaxDepth and within the equal-count bound plus the levels a surface-area split may add;
//   two builds of the same input are byte-identical.
// Prints "name value" lines and exits 0 only if every check held.

#include "ray_scene.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace chord::ray;

static int g_failures = 0;
#define CHECK(cond, what)                                                        \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED %s: %s (line %d)\n", g_case, what, __LINE__); g_failures++; } \
    } while (0)
static const char* g_case = "";

static uint32_t rng_state = 12345u;
static float rnd()
{
    rng_state = rng_state * 747796405u + 2891336453u;
    const uint32_t w = ((rng_state >> ((rng_state >> 28u) + 4u)) ^ rng_state) * 277803737u;
    return (float)(((w >> 22u) ^ w) >> 8) / 16777216.0f;
}

static bool same_box(const Box& a, const Box& b) { return std::memcmp(&a, &b, sizeof(Box)) == 0; }

static Box union_of(const Box& a, const Box& b)
{
    Box o;
    for (int k = 0; k < 3; k++) { o.lo[k] = fmin_(a.lo[k], b.lo[k]); o.hi[k] = fmax_(a.hi[k], b.hi[k]); }
    return o;
}

struct Walk {
    const Tree* t;
    const Box* boxes;
    uint32_t count, leafItems, nodeTag, leafTag, nodeBase, itemBase;
    std::vector<uint32_t> seen;
    uint32_t maxLevel = 0, leaves = 0;

    Box node_box(uint32_t n, uint32_t level, uint32_t parentRef)
    {
        const Node& nd = t->nodes[n];
        if (level + 1 > maxLevel) maxLevel = level + 1;
        CHECK(nd.parentRef == parentRef, "parentRef");
        CHECK(nd.childCount >= 1 && nd.childCount <= kWidth, "childCount");
        Box whole{};
        for (uint32_t k = 0; k < kWidth; k++) {
            if (k >= nd.childCount) { CHECK(nd.child[k] == kNoChild, "unused slot holds a child"); continue; }
            Box slot;
            for (int a = 0; a < 3; a++) { slot.lo[a] = nd.lo[a][k]; slot.hi[a] = nd.hi[a][k]; }
            const uint32_t w = nd.child[k], tag = w >> kTagShift, idx = w & kIndexMask;
            Box below{};
            if (tag == nodeTag) {
                const uint32_t c = idx - nodeBase;
                CHECK(c > n && c < t->nodes.size(), "child node index");
                if (c > n && c < t->nodes.size()) below = node_box(c, level + 1, n * kWidth + k);
            } else {
                CHECK(tag == leafTag, "child tag");
                leaves++;
                uint32_t first, cnt;
                if (leafItems == 1u) { first = idx - itemBase; cnt = 1u; }
                else { first = (idx >> 2) - itemBase; cnt = (idx & 3u) + 1u; }
                CHECK(cnt <= leafItems, "leaf size");
                for (uint32_t i = 0; i < cnt; i++) {
                    const uint32_t item = leafItems == 1u ? first : (first + i < count ? t->order[first + i] : count);
                    CHECK(item < count, "leaf item index");
                    if (item >= count) continue;
                    seen[item]++;
                    CHECK(t->leafRef[item] == n * kWidth + k, "leafRef");
                    below = i == 0 ? boxes[item] : union_of(below, boxes[item]);
                }
            }
            CHECK(same_box(slot, below), "a slot's box is not the exact union of what is beneath it");
            whole = k == 0 ? slot : union_of(whole, slot);
        }
        return whole;
    }
};

static void check_tree(const char* name, const std::vector<Box>& boxes, uint32_t leafItems, uint32_t nodeBase, uint32_t itemBase)
{
    g_case = name;
    const uint32_t nodeTag = leafItems == 1u ? kTlasNode : kBlasNode, leafTag = leafItems == 1u ? kTlasLeaf : kBlasLeaf;
    Tree a, b;
    const int rc = build_tree(boxes.data(), (uint32_t)boxes.size(), leafItems, nodeTag, leafTag, nodeBase, itemBase, a);
    CHECK(rc == 0, "build_tree failed");
    if (rc) return;
    CHECK(build_tree(boxes.data(), (uint32_t)boxes.size(), leafItems, nodeTag, leafTag, nodeBase, itemBase, b) == 0, "second build failed");
    CHECK(a.nodes.size() == b.nodes.size() && std::memcmp(a.nodes.data(), b.nodes.data(), a.nodes.size() * sizeof(Node)) == 0 &&
          a.order == b.order && a.leafRef == b.leafRef && same_box(a.rootBox, b.rootBox) && a.depth == b.depth, "two builds differ");
    Walk w{&a, boxes.data(), (uint32_t)boxes.size(), leafItems, nodeTag, leafTag, nodeBase, itemBase, std::vector<uint32_t>(boxes.size(), 0u)};
    const Box root = w.node_box(0u, 0u, kNoChild);
    CHECK(same_box(root, a.rootBox), "rootBox");
    for (size_t i = 0; i < boxes.size(); i++) CHECK(w.seen[i] == 1u, "an item is not in exactly one leaf");
    std::vector<uint32_t> perm(boxes.size(), 0u);
    for (uint32_t i : a.order) if (i < boxes.size()) perm[i]++;
    for (size_t i = 0; i < boxes.size(); i++) CHECK(perm[i] == 1u, "order is not a permutation");
    CHECK(w.maxLevel == a.depth, "depth");
    CHECK(a.depth <= kMaxDepth, "deeper than kMaxDepth");
    std::printf("%s_items %zu\n%s_nodes %zu\n%s_leaves %u\n%s_depth %u\n%s_balanced_levels %u\n", name, boxes.size(), name, a.nodes.size(), name,
                w.leaves, name, a.depth, name, balanced_levels(boxes.size(), leafItems));
}

static Box tri_box(const float* v)
{
    Triangle t{};
    std::memcpy(t.v, v, sizeof(t.v));
    return triangle_box(t);
}

int main()
{
    {   // one triangle
        const float v[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0};
        check_tree("one_triangle", {tri_box(v)}, kLeafTriangles, 0u, 0u);
    }
    {   // a primitive without LOD-0 triangles has no tree: the builder refuses an empty input
        g_case = "no_triangle";
        Tree t;
        CHECK(build_tree(nullptr, 0u, kLeafTriangles, kBlasNode, kBlasLeaf, 0u, 0u, t) != 0 && t.nodes.empty(), "an empty input must be refused");
        std::printf("no_triangle_refused 1\n");
    }
    {   // 1 024 coincident triangles: no plane separates them, depth stays logarithmic
        const float v[9] = {0.25f, 0.5f, -1.0f, 1.25f, 0.5f, -1.0f, 0.25f, 1.5f, -1.0f};
        std::vector<Box> boxes(1024, tri_box(v));
        check_tree("coincident", boxes, kLeafTriangles, 7u, 100u);
        CHECK(balanced_levels(1024, kLeafTriangles) == 4u, "balanced_levels(1024, 4)");
    }
    {   // a 255-vertex meshlet: 85 disjoint triangles, vertex ids descending (the shape of tests/meshlet_shapes.py)
        std::vector<Box> boxes;
        for (int t = 84; t >= 0; t--) {
            const float x = (float)(t % 10), y = (float)(t / 10);
            const float v[9] = {x, y, 0.0f, x + 0.8f, y, 0.1f, x, y + 0.8f, -0.1f};
            boxes.push_back(tri_box(v));
        }
        check_tree("meshlet255", boxes, kLeafTriangles, 0u, 0u);
    }
    {   // a random mesh: triangles of mixed sizes, some degenerate, some huge
        std::vector<Box> boxes;
        for (int t = 0; t < 5000; t++) {
            float v[9];
            const float s = t % 97 == 0 ? 50.0f : (t % 13 == 0 ? 0.0f : 0.2f);
            const float c[3] = {rnd() * 20.0f - 10.0f, rnd() * 4.0f, rnd() * 20.0f - 10.0f};
            for (int k = 0; k < 9; k++) v[k] = c[k % 3] + (rnd() - 0.5f) * s;
            boxes.push_back(tri_box(v));
        }
        check_tree("random_mesh", boxes, kLeafTriangles, 3u, 11u);
    }
    {   // exponentially spaced items: a surface-area split peels one off at a time; the depth bound must switch to equal counts
        std::vector<Box> boxes;
        float x = 1.0f;
        for (int t = 0; t < 120; t++) { Box b{{x, 0.0f, 0.0f}, {x * 1.01f, 1.0f, 1.0f}}; boxes.push_back(b); x *= 2.0f; }
        check_tree("exponential", boxes, kLeafTriangles, 0u, 0u);
    }
    {   // the deep scene of tests/ray_deep_cases.py: its primitive's 128 triangles, x = 2^(j - 125), and its 120 instance boxes, moved
        // along x by 0, 8, 16, ... 2^121 (formed from centre and extent, as an object's box is).  Both must use the depth bound fully.
        std::vector<Box> boxes;
        for (int j = 0; j < 128; j++) {
            const float x = std::ldexp(1.0f, j - 125), x2 = x * (1.0f + 0.0078125f);
            const float v[9] = {x, 0.0f, 0.0f, x, 1.0f, 0.0f, x2, 0.0f, 1.0f};
            boxes.push_back(tri_box(v));
        }
        check_tree("deep_blas", boxes, kLeafTriangles, 0u, 0u);
        const float mn = std::ldexp(1.0f, -125), mx = 4.0f * (1.0f + 0.0078125f), c = (mn + mx) * 0.5f, e = mx - c;
        boxes.clear();
        for (int k = 0; k < 120; k++) {
            const float t = k == 0 ? 0.0f : std::ldexp(1.0f, k + 2);
            Box b{{(c - e) + t, 0.0f, 0.0f}, {(c + e) + t, 1.0f, 1.0f}};
            boxes.push_back(b);
        }
        check_tree("deep_tlas", boxes, 1u, 0u, 0u);
    }
    {   // NaN and infinite boxes among ordinary ones (an upload does not refuse them; the library's own build does, before it gets
        // here): the equal-count sort's key is total, so the builder still ends, with every item in one leaf
        std::vector<Box> boxes;
        for (int t = 0; t < 300; t++) {
            const float c = (float)(t % 17);
            Box b{{c, 0.0f, (float)(t / 17)}, {c + 0.5f, 1.0f, (float)(t / 17) + 0.5f}};
            if (t % 5 == 0) b.lo[0] = b.hi[0] = __builtin_nanf("");
            if (t % 7 == 0) b.hi[2] = __builtin_inff();
            if (t % 11 == 0) b.lo[1] = -__builtin_nanf("");
            boxes.push_back(b);
        }
        check_tree("non_finite", boxes, kLeafTriangles, 0u, 0u);
    }
    const uint32_t tlasSizes[4] = {1u, 2u, 9u, 600u};
    for (uint32_t n : tlasSizes) {
        std::vector<Box> boxes;
        for (uint32_t i = 0; i < n; i++) {
            const float c[3] = {rnd() * 100.0f - 50.0f, rnd() * 5.0f, rnd() * 100.0f - 50.0f};
            Box b;
            for (int k = 0; k < 3; k++) { const float e = rnd() * 3.0f; b.lo[k] = c[k] - e; b.hi[k] = c[k] + e; }
            boxes.push_back(b);
        }
        char name[32];
        std::snprintf(name, sizeof(name), "tlas%u", n);
        check_tree(name, boxes, 1u, 0u, 0u);
    }
    {   // 600 identical boxes (instances with one matrix)
        Box b{{-1.0f, -1.0f, -1.0f}, {1.0f, 1.0f, 1.0f}};
        check_tree("tlas600_same", std::vector<Box>(600, b), 1u, 0u, 0u);
    }
    std::printf("failures %d\n", g_failures);
    return g_failures == 0 ? 0 : 1;
}
