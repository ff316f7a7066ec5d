// Stand-alone run of chord_amd/csrc/ray_walk.h on the host (built and run by tests/test_ray_walk_host.py together with chord_amd/csrc/
// ray_scene.cpp; no GPU, no python in the process).  The header's per-ray function is plain float32 / integer C++ behind __device__,
// which the host compiler reads as nothing, so the statements ray_trace_kernel executes per lane are the statements this program
// executes per ray; the device built-ins that device_math.h names in functions nobody calls here (__clz, the binary16 bit casts) are
// supplied below.  It reads one request, builds the ray scene as chordvis_build_ray_scene and chordvis_refit_ray_scene do -- one BLAS
// per primitive and the TLAS with ray::build_tree, the object boxes with box_corner, the node boxes with node_union, children before
// parents -- calls walk_ray for every ray and writes:
//   request   uint32 words.  Eight of header: objects, primitives, rays, any-hit (0 / 1), four zero words.  Then the object records
//             (ChordObject, 56 words each); per primitive posMin, posMax (3 floats each), its LOD-0 triangle count T and T records of
//             9 floats, meshlet, triangle (ascending (meshlet, triangle): tests/spec_rays_np.lod0_triangles); the rays (ChordRay, 8
//             words each).
//   answer    eight words of header: the deepest BLAS's levels, the TLAS's levels, BLAS nodes, TLAS nodes, BLAS triangles, three
//             zero words.  Then per ray ten words: the eight of its ChordRayHit, the stack's high-water mark (entries), and the
//             pushes the full stack refused.
// Every array lives in a heap allocation of exactly its size -- the stack of ray::kStackEntries words too -- so a read or write one
// element past any of them is a sanitizer error.  Exit status 2 on a malformed request, 3 when a tree cannot be built.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

static inline int __clz(int v) { return v ? __builtin_clz((unsigned)v) : 32; }
static inline unsigned short __half_as_ushort(__half h) { unsigned short u; std::memcpy(&u, (const void*)&h, 2); return u; }
static inline __half __ushort_as_half(unsigned short u) { __half h; std::memcpy((void*)&h, &u, 2); return h; }

#include "ray_walk.h"

using namespace chord;

struct WalkStats {
    uint32_t high = 0, refused = 0;
    void tlas_node() {}
    void tlas_leaf() {}
    void blas_node() {}
    void triangle() {}
    void push(uint32_t sp)
    {
        if (sp >= ray::kStackEntries) refused++;
        else if (sp + 1u > high) high = sp + 1u;
    }
};

// `count` elements of T copied into an allocation of exactly that size (one byte for none: a read of element 0 is still an error)
template <typename T>
static T* exact(const void* src, size_t count)
{
    void* p = std::malloc(count ? count * sizeof(T) : 1u);
    if (count) std::memcpy(p, src, count * sizeof(T));
    return static_cast<T*>(p);
}

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
    const uint32_t nObjects = req[0], nPrims = req[1], nRays = req[2], anyHit = req[3];
    static_assert(sizeof(ChordObject) == 224 && sizeof(ChordRay) == 32 && sizeof(ChordRayHit) == 32 && sizeof(ray::Triangle) == 48, "request records");
    if (nObjects == 0u) return 2;

    size_t at = 8;
    auto take = [&](size_t words) -> const uint32_t* {
        if (at + words > req.size()) std::exit(2);
        const uint32_t* p = req.data() + at;
        at += words;
        return p;
    };
    ChordObject* objects = exact<ChordObject>(take((size_t)nObjects * 56u), nObjects);

    // one BLAS per primitive, all in one node array and one triangle array (abi_rays.cpp ray_build_blases)
    std::vector<float> bounds((size_t)nPrims * 6u);
    std::vector<ray::Node> blasNodes;
    std::vector<ray::Triangle> blasTris;
    std::vector<uint32_t> roots(nPrims, ray::kNoChild);
    uint32_t blasDepth = 0;
    for (uint32_t p = 0; p < nPrims; p++) {
        const uint32_t* h = take(7);
        std::memcpy(&bounds[6u * p], h, 24);
        const uint32_t T = h[6];
        const uint32_t* tw = take((size_t)T * 11u);
        if (T == 0u) continue;
        std::vector<ray::Triangle> tris(T);
        std::vector<ray::Box> boxes(T);
        for (uint32_t t = 0; t < T; t++) {
            std::memset(&tris[t], 0, sizeof(ray::Triangle));
            std::memcpy(tris[t].v, tw + 11u * t, 36);
            tris[t].meshlet = tw[11u * t + 9u]; tris[t].triangle = tw[11u * t + 10u];
            boxes[t] = ray::triangle_box(tris[t]);
        }
        ray::Tree tree;
        if (ray::build_tree(boxes.data(), T, ray::kLeafTriangles, ray::kBlasNode, ray::kBlasLeaf, (uint32_t)blasNodes.size(), (uint32_t)blasTris.size(), tree))
            return 3;
        roots[p] = (ray::kBlasNode << ray::kTagShift) | (uint32_t)blasNodes.size();
        blasNodes.insert(blasNodes.end(), tree.nodes.begin(), tree.nodes.end());
        for (uint32_t i : tree.order) blasTris.push_back(tris[i]);
        blasDepth = std::max(blasDepth, tree.depth);
    }
    const uint32_t* rayWords = take((size_t)nRays * 8u);
    if (at != req.size()) return 2;

    // the object boxes (ray_refit_kernel's statements), the TLAS over them, and the refit: a leaf's box into its slot, then every node's
    // union into its slot of its parent, children before parents (a child's index is above its parent's)
    DObjStatic* objStatic = static_cast<DObjStatic*>(std::malloc(nObjects * sizeof(DObjStatic)));
    float4* leafBox = static_cast<float4*>(std::malloc((size_t)nObjects * 2u * sizeof(float4)));
    std::vector<ray::Box> boxes(nObjects);
    for (uint32_t o = 0; o < nObjects; o++) {
        DObjStatic& st = objStatic[o];
        std::memset(&st, 0, sizeof(st));
        st.prim = objects[o].GLTFPrimitiveDetail;
        if (st.prim >= nPrims) return 2;                       // (chordvis_upload_scene refuses such an object)
        std::memcpy(st.posMin, &bounds[6u * st.prim], 12); std::memcpy(st.posMax, &bounds[6u * st.prim + 3u], 12);
        const Mat4 M = load_mat(objects[o].basicData.localToTranslatedWorld);
        f3 c, e;
        aabb_center_extent(st.posMin, st.posMax, c, e);
        float lo[3], hi[3];
        for (int k = 0; k < 8; k++) box_corner(c, e, M, k, lo, hi);
        leafBox[2u * o] = make_float4(lo[0], lo[1], lo[2], 0.0f);
        leafBox[2u * o + 1u] = make_float4(hi[0], hi[1], hi[2], 0.0f);
        for (int a = 0; a < 3; a++) { boxes[o].lo[a] = lo[a]; boxes[o].hi[a] = hi[a]; }
    }
    ray::Tree tlasTree;
    if (ray::build_tree(boxes.data(), nObjects, 1u, ray::kTlasNode, ray::kTlasLeaf, 0u, 0u, tlasTree)) return 3;
    for (uint32_t o = 0; o < nObjects; o++) {
        const uint32_t ref = tlasTree.leafRef[o];
        ray::Node& nd = tlasTree.nodes[ref >> 2];
        for (int a = 0; a < 3; a++) { nd.lo[a][ref & 3u] = boxes[o].lo[a]; nd.hi[a][ref & 3u] = boxes[o].hi[a]; }
    }
    for (size_t n = tlasTree.nodes.size(); n-- > 1u;) {
        const ray::Node& nd = tlasTree.nodes[n];
        float lo[3], hi[3];
        node_union(nd, nd.childCount, lo, hi);
        ray::Node& up = tlasTree.nodes[nd.parentRef >> 2];
        if ((nd.parentRef >> 2) >= n) return 3;
        for (int a = 0; a < 3; a++) { up.lo[a][nd.parentRef & 3u] = lo[a]; up.hi[a][nd.parentRef & 3u] = hi[a]; }
    }

    RayWalkScene s;
    ray::Node* tlas = exact<ray::Node>(tlasTree.nodes.data(), tlasTree.nodes.size());
    ray::Node* blas = exact<ray::Node>(blasNodes.data(), blasNodes.size());
    float4* triangles = exact<float4>(blasTris.data(), blasTris.size() * 3u);
    uint32_t* blasRoot = exact<uint32_t>(roots.data(), roots.size());
    float4* rays = exact<float4>(rayWords, (size_t)nRays * 2u);
    uint32_t* stack = static_cast<uint32_t*>(std::malloc(ray::kStackEntries * sizeof(uint32_t)));
    s.objects = objects; s.objStatic = objStatic; s.tlas = tlas; s.leafBox = leafBox; s.blasRoot = blasRoot; s.blas = blas; s.triangles = triangles;
    s.objectCount = nObjects; s.primCount = nPrims; s.tlasNodes = (uint32_t)tlasTree.nodes.size(); s.blasNodes = (uint32_t)blasNodes.size();
    s.triangleCount = (uint32_t)blasTris.size();

    std::vector<uint32_t> out(8u + (size_t)nRays * 10u, 0u);
    out[0] = blasDepth; out[1] = tlasTree.depth; out[2] = s.blasNodes; out[3] = s.tlasNodes; out[4] = s.triangleCount;
    for (uint32_t i = 0; i < nRays; i++) {
        WalkStats stats;
        const RayWords h = anyHit ? walk_ray<true>(s, rays[2u * i], rays[2u * i + 1u], stack, stats)
                                  : walk_ray<false>(s, rays[2u * i], rays[2u * i + 1u], stack, stats);
        uint32_t* w = &out[8u + (size_t)i * 10u];
        std::memcpy(w, &h.h0, 16); std::memcpy(w + 4, &h.h1, 16);
        w[8] = stats.high; w[9] = stats.refused;
    }

    std::free(objects); std::free(objStatic); std::free(leafBox); std::free(tlas); std::free(blas); std::free(triangles); std::free(blasRoot);
    std::free(rays); std::free(stack);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    const bool ok = std::fwrite(out.data(), 4, out.size(), o) == out.size();
    std::fclose(o);
    return ok ? 0 : 2;
}
