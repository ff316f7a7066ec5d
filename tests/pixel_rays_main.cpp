// Stand-alone run of chord_amd/csrc/pixel_rays.h on the host (built and run by tests/test_pixel_rays_host.py together with chord_amd/
// csrc/ray_scene.cpp; no GPU, no python in the process).  The header's per-pixel functions and ray_walk.h's walk_ray are plain float32 /
// integer C++ behind __device__, which the host compiler reads as nothing, so the statements pixel_rays_kernel executes per lane are
// the statements this program executes per pixel: pixel_of_lane over every wave and lane of the image (a pixel outside it is skipped,
// as the kernel's lane leaves), table_index, make_pixel_ray -> walk_ray -> finish_pixel_ray.  The ray scene is built as tests/
// ray_walk_main.cpp builds it.
//   request   uint32 words.  Eight of header: objects, primitives, cases, five zero words.  Then the object records (ChordObject, 56
//             words each); per primitive posMin, posMax (3 floats each), its LOD-0 triangle count T and T records of 9 floats, meshlet,
//             triangle.  Then per case: the sixteen words of its ChordPixelRaysDesc, whether there is a depth image (0 / 1), whether hit
//             records are asked for (0 / 1); the position image and the normal image (width * height * 4 floats each); the depth image
//             (width * height * deviceZStride floats) when there is one; the table (tableW * tableH * 4 floats) in HEMISPHERE mode.
//   answer    per case width * height floats of out, then width * height * 8 words of hit records (zero when none were asked for),
//             then one word: the pixels visited, which must be width * height.
// Every image and table lives in a heap allocation of exactly its size, the stack in one of exactly ray::kStackEntries words, out and
// hits likewise, so a read or write one element past any of them is a sanitizer error.  Exit status 2 on a malformed request, 3 when a
// tree cannot be built, 4 when a push was refused or a pixel was visited twice.
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

#include "pixel_rays.h"

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
    const uint32_t nObjects = req[0], nPrims = req[1], nCases = req[2];
    static_assert(sizeof(ChordObject) == 224 && sizeof(ChordPixelRaysDesc) == 64 && sizeof(ChordRayHit) == 32 && sizeof(ray::Triangle) == 48, "request records");
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
    }

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
    uint32_t* stack = static_cast<uint32_t*>(std::malloc(ray::kStackEntries * sizeof(uint32_t)));
    s.objects = objects; s.objStatic = objStatic; s.tlas = tlas; s.leafBox = leafBox; s.blasRoot = blasRoot; s.blas = blas; s.triangles = triangles;
    s.objectCount = nObjects; s.primCount = nPrims; s.tlasNodes = (uint32_t)tlasTree.nodes.size(); s.blasNodes = (uint32_t)blasNodes.size();
    s.triangleCount = (uint32_t)blasTris.size();

    std::vector<uint32_t> answer;
    for (uint32_t k = 0; k < nCases; k++) {
        ChordPixelRaysDesc d;
        std::memcpy(&d, take(16), 64);
        const uint32_t* opt = take(2);
        const bool hasZ = opt[0] != 0u, wantHits = opt[1] != 0u;
        const bool hemisphere = d.mode == CHORD_PIXEL_RAYS_HEMISPHERE, anyHit = (d.flags & CHORD_PIXEL_RAYS_ANY_HIT) != 0u;
        const uint64_t pixels = (uint64_t)d.width * d.height;
        if (pixels == 0u || pixels > (1u << 24) || (hasZ && d.deviceZStride == 0u) || (wantHits && anyHit)) return 2;
        if (hemisphere && (d.tableW == 0u || d.tableH == 0u || (d.tableW & (d.tableW - 1u)) || (d.tableH & (d.tableH - 1u)))) return 2;
        float4* position = exact<float4>(take(pixels * 4u), pixels);
        float4* normal = exact<float4>(take(pixels * 4u), pixels);
        float* z = hasZ ? exact<float>(take(pixels * d.deviceZStride), pixels * d.deviceZStride) : nullptr;
        float4* table = hemisphere ? exact<float4>(take((size_t)d.tableW * d.tableH * 4u), (size_t)d.tableW * d.tableH) : nullptr;
        float* out = static_cast<float*>(std::malloc(pixels * sizeof(float)));
        uint4* hits = static_cast<uint4*>(std::malloc(pixels * 2u * sizeof(uint4)));
        std::memset(hits, 0, pixels * 2u * sizeof(uint4));
        std::vector<uint8_t> seen(pixels, 0);
        uint32_t visited = 0;
        const uint64_t waves = pixel_wave_count(d.width, d.height);
        for (uint64_t wave = 0; wave < waves; wave++) {
            for (uint32_t lane = 0; lane < 64u; lane++) {
                uint64_t x, y;
                pixel_of_lane(wave, lane, d.width, x, y);
                if (x >= d.width || y >= d.height) continue;
                const uint64_t i = y * d.width + x;
                if (seen[i]) return 4;
                seen[i] = 1; visited++;
                const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                const float zv = z ? z[i * d.deviceZStride] : 0.0f;
                const float4 dT = table ? table[table_index((uint32_t)x, (uint32_t)y, d.tableW, d.tableH)] : zero4;
                const PixelRay r = make_pixel_ray(d, position[i], normal[i], z != nullptr, zv, dT);
                float o = r.disposition == kPixelZero ? 0.0f : 1.0f;
                RayWords w;
                w.h0 = make_uint4(0u, 0u, 0u, 0u); w.h1 = make_uint4(0u, 0u, 0u, 0u);
                if (r.disposition == kPixelTrace) {
                    WalkStats stats;
                    if (anyHit) { w = walk_ray<true>(s, r.r0, r.r1, stack, stats); o = finish_pixel_ray<true>(w, d.rayLength); }
                    else { w = walk_ray<false>(s, r.r0, r.r1, stack, stats); o = finish_pixel_ray<false>(w, d.rayLength); }
                    if (stats.refused) return 4;
                }
                out[i] = o;
                if (!anyHit && wantHits) { hits[2u * i] = w.h0; hits[2u * i + 1u] = w.h1; }
            }
        }
        const size_t base = answer.size();
        answer.resize(base + pixels * 9u + 1u);
        std::memcpy(&answer[base], out, pixels * 4u);
        std::memcpy(&answer[base + pixels], hits, pixels * 32u);
        answer[base + pixels * 9u] = visited;
        std::free(position); std::free(normal); std::free(z); std::free(table); std::free(out); std::free(hits);
    }
    if (at != req.size()) return 2;

    std::free(objects); std::free(objStatic); std::free(leafBox); std::free(tlas); std::free(blas); std::free(triangles); std::free(blasRoot);
    std::free(stack);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    const bool ok = std::fwrite(answer.data(), 4, answer.size(), o) == answer.size();
    std::fclose(o);
    return ok ? 0 : 2;
}
