// Stand-alone run of chord_amd/csrc/ray_tlas_shape.h on the host (built and run by tests/test_ray_tlas_host.py; no GPU, no python in
// the process).  The header is plain C++, so the functions the kernels of kernels_raytlas.hip call per lane are the functions this
// program calls per object and per node.  It reads one request and writes one answer, uint32 words:
//   request   mode, n, six zero words.  mode 0: then n boxes of six floats (lo.xyz, hi.xyz).  mode 1: nothing more -- the bare shape
//             over n objects in index order.
//   answer    mode 0: depth, nodes, six zero words; the node table (32 words a node) with every box -- leaf slots from the boxes,
//             higher slots by the refit's fold, children before parents --; leafRef (n words).
//             mode 1: depth, nodes, then four 64-bit sums as pairs of words (low, high), all modulo 2^64: of child[g][k] * (4 g + k
//             + 1), of parentRef[g] * (g + 1), of childCount[g], of leafRef[o] * (o + 1).
// The node table and leafRef live in heap allocations of exactly their size, so a write one element past either is a sanitizer
// error.  Exit status 2 on a malformed request, 3 when the shape is refused.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ray_tlas_shape.h"

using namespace chord;

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<uint32_t> req;
    uint32_t buf[4096];
    size_t got;
    while ((got = std::fread(buf, 4, 4096, in)) > 0) req.insert(req.end(), buf, buf + got);
    std::fclose(in);
    if (req.size() < 8) return 2;
    const uint32_t mode = req[0], n = req[1];
    if (mode > 1u || (mode == 0u && req.size() != 8u + 6u * (size_t)n)) return 2;

    ray::TlasShape s;
    if (ray::tlas_shape(n, s)) return 3;
    if (ray::tlas_node_count(n) != s.nodes) return 3;

    // the sorted order
    uint32_t* order = static_cast<uint32_t*>(std::malloc((size_t)n * 4u));
    const float* boxes = reinterpret_cast<const float*>(req.data() + 8);
    if (mode == 0u) {
        std::vector<float> c((size_t)n * 3u);
        uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
        for (uint32_t i = 0; i < n; i++)
            for (int a = 0; a < 3; a++) {
                c[3u * i + a] = ray::tlas_centre(boxes[6u * i + a], boxes[6u * i + 3 + a]);
                const uint32_t m = ray::tlas_mono(c[3u * i + a]);
                lo[a] = std::min(lo[a], m); hi[a] = std::max(hi[a], m);
            }
        float blo[3], bhi[3];
        for (int a = 0; a < 3; a++) { blo[a] = ray::tlas_unmono(lo[a]); bhi[a] = ray::tlas_unmono(hi[a]); }
        std::vector<uint64_t> words(n);
        for (uint32_t i = 0; i < n; i++) words[i] = ((uint64_t)ray::tlas_key(&c[3u * i], blo, bhi) << 32) | i;
        std::sort(words.begin(), words.end());
        for (uint32_t p = 0; p < n; p++) order[p] = (uint32_t)words[p];
    } else {
        for (uint32_t p = 0; p < n; p++) order[p] = p;
    }

    // node table and leaf references, each in an allocation of exactly its size
    ray::Node* nodes = static_cast<ray::Node*>(std::malloc((size_t)s.nodes * sizeof(ray::Node)));
    uint32_t* leafRef = static_cast<uint32_t*>(std::malloc((size_t)n * 4u));
    if (!order || !nodes || !leafRef) return 2;
    const auto at = [&](uint32_t p) -> uint32_t { return order[p]; };
    for (uint32_t g = 0; g < s.nodes; g++) ray::tlas_node_words(s, g, at, nodes[g]);
    for (uint32_t p = 0; p < n; p++) leafRef[order[p]] = ray::tlas_leaf_ref(s, p);

    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    if (mode == 0u) {
        // the refit: leaf boxes into their slots, then every node's fold into its parent's slot, children before parents (a lower
        // level has the higher node numbers)
        for (uint32_t o = 0; o < n; o++) {
            ray::Node& nd = nodes[leafRef[o] >> 2];
            for (int a = 0; a < 3; a++) { nd.lo[a][leafRef[o] & 3u] = boxes[6u * o + a]; nd.hi[a][leafRef[o] & 3u] = boxes[6u * o + 3 + a]; }
        }
        for (uint32_t g = s.nodes; g-- > 1u;) {
            const ray::Node& nd = nodes[g];
            ray::Node& up = nodes[nd.parentRef >> 2];
            for (int a = 0; a < 3; a++) {
                float l = nd.lo[a][0], h = nd.hi[a][0];
                for (uint32_t k = 1; k < nd.childCount; k++) { l = ray::fmin_(l, nd.lo[a][k]); h = ray::fmax_(h, nd.hi[a][k]); }
                up.lo[a][nd.parentRef & 3u] = l; up.hi[a][nd.parentRef & 3u] = h;
            }
        }
        const uint32_t head[8] = {s.depth, s.nodes, 0u, 0u, 0u, 0u, 0u, 0u};
        std::fwrite(head, 4, 8, out);
        std::fwrite(nodes, sizeof(ray::Node), s.nodes, out);
        std::fwrite(leafRef, 4, n, out);
    } else {
        uint64_t sums[4] = {0u, 0u, 0u, 0u};
        for (uint32_t g = 0; g < s.nodes; g++) {
            for (uint32_t k = 0; k < 4u; k++) sums[0] += (uint64_t)nodes[g].child[k] * (4ull * g + k + 1ull);
            sums[1] += (uint64_t)nodes[g].parentRef * (g + 1ull);
            sums[2] += nodes[g].childCount;
        }
        for (uint32_t o = 0; o < n; o++) sums[3] += (uint64_t)leafRef[o] * (o + 1ull);
        uint32_t head[10] = {s.depth, s.nodes};
        for (int i = 0; i < 4; i++) { head[2 + 2 * i] = (uint32_t)sums[i]; head[3 + 2 * i] = (uint32_t)(sums[i] >> 32); }
        std::fwrite(head, 4, 10, out);
    }
    std::fclose(out);
    std::free(order); std::free(nodes); std::free(leafRef);
    return 0;
}
