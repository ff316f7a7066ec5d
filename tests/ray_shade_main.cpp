// Stand-alone run of chord_amd/csrc/ray_shade.h on the host (built and run by tests/test_ray_shade_host.py; no GPU, no python in the
// process).  The header's per-hit function is plain float32 / integer C++ behind __device__, which the host compiler reads as nothing,
// so the statements the kernel executes per lane are the statements this program executes per hit; the two device built-ins the
// sampler's includes use (__umulhi, min) are supplied here.  It reads one request, calls shade_ray_hit for every hit and writes the
// sixteen words of every record:
//   request   uint32 words.  Sixteen of header: objects, meshlets, primitives, materials, samplers, textures, meshlet-data words,
//             vertices, has texcoords, has normals, hits, has per-hit levels, the uniform level (float bits), three zero words.  Then
//             the object records (ChordObject, 56 words each); per primitive its vertexOffset; per primitive the first meshlet and the
//             meshlet count of its asset (a hit's meshlet is asset-relative; one asset: 0 and the meshlet count); per meshlet dataOffset and
//             vertexTriangleCount; the meshlet data; the texture coordinates (2 floats a vertex) and the normals (3 floats a vertex) where the header says so; the
//             materials (ChordMaterial, 24 words each); the samplers (4 words each); per texture width, height, mips and its RGBA8
//             chain, a word a texel; the hits (ChordRayHit, 8 words each); the per-hit levels.
//   answer    hits x 16 uint32
// Every array lives in a heap allocation of exactly its size, so a read one element past any of them is a sanitizer error.  The
// DMatRecords are filled as chordvis_upload_material_textures fills them (texel store only).  Exit status 2 on a malformed request.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

static inline uint32_t __umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
using std::max;
using std::min;

#include "ray_shade.h"
#include "material_tables.h"

using namespace chord;

static const uint32_t kSrgbBits[256] = {CHORD_SRGB_TABLE_BITS};
static const uint32_t kAp1Bits[9] = {CHORD_SRGB_2_AP1_BITS};

static void wrap_consts(uint32_t n, uint32_t mode, uint32_t& magic, uint32_t& bias)
{
    magic = 0u; bias = 0u;
    if (mode == CHORD_WRAP_CLAMP_TO_EDGE) return;
    const uint32_t period = mode == CHORD_WRAP_MIRRORED_REPEAT ? 2u * n : n;
    if ((period & (period - 1u)) == 0u) return;
    magic = (uint32_t)(0x100000000ull / period);
    bias = (uint32_t)(((0x40000000ull + period - 1u) / period) * period);
}

static bool linear_filter(uint32_t f) { return f == CHORD_FILTER_LINEAR || f == CHORD_FILTER_LINEAR_MIPMAP_NEAREST || f == CHORD_FILTER_LINEAR_MIPMAP_LINEAR; }

// `count` elements of T copied into an allocation of exactly that size (one byte for none: a read of element 0 is still an error)
template <typename T>
static T* exact(const uint32_t* src, size_t count)
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
    if (req.size() < 16) return 2;
    const uint32_t nObjects = req[0], nMeshlets = req[1], nPrims = req[2], nMaterials = req[3], nSamplers = req[4], nTextures = req[5];
    const uint32_t nData = req[6], nVertices = req[7], hasUv = req[8], hasNormals = req[9], nHits = req[10], hasLods = req[11];
    float lod;
    std::memcpy(&lod, &req[12], 4);
    static_assert(sizeof(ChordObject) == 224 && sizeof(ChordMaterial) == 96 && sizeof(ChordSampler) == 16 && sizeof(ChordRayHit) == 32, "request records");

    size_t at = 16;
    auto take = [&](size_t words) -> const uint32_t* {
        if (at + words > req.size()) std::exit(2);
        const uint32_t* p = req.data() + at;
        at += words;
        return p;
    };
    RayShadeScene s;
    std::memset(&s, 0, sizeof(s));
    ChordObject* objects = exact<ChordObject>(take((size_t)nObjects * 56u), nObjects);
    uint32_t* primVertexBase = exact<uint32_t>(take(nPrims), nPrims);
    uint2* primAssetMeshlets = exact<uint2>(take((size_t)nPrims * 2u), nPrims);
    const uint32_t* mw = take((size_t)nMeshlets * 2u);
    DMeshlet* meshlets = static_cast<DMeshlet*>(std::malloc(nMeshlets ? nMeshlets * sizeof(DMeshlet) : 1u));
    for (uint32_t i = 0; i < nMeshlets; i++) {
        std::memset(&meshlets[i], 0, sizeof(DMeshlet));
        meshlets[i].dataOffset = mw[2u * i]; meshlets[i].vertexTriangleCount = mw[2u * i + 1u]; meshlets[i].vertexBase = 0xFFFFFFFFu;   // (not read)
    }
    uint32_t* data = exact<uint32_t>(take(nData), nData);
    float* texcoords = hasUv ? exact<float>(take((size_t)nVertices * 2u), (size_t)nVertices * 2u) : nullptr;
    float* normals = hasNormals ? exact<float>(take((size_t)nVertices * 3u), (size_t)nVertices * 3u) : nullptr;
    const ChordMaterial* mats = reinterpret_cast<const ChordMaterial*>(take((size_t)nMaterials * 24u));
    const ChordSampler* samplers = reinterpret_cast<const ChordSampler*>(take((size_t)nSamplers * 4u));

    // the texel store: every chain back to back, in one allocation of exactly their size
    struct Tex { uint32_t width, height, mips, base; };
    std::vector<Tex> tex(nTextures);
    std::vector<uint32_t> store;
    for (uint32_t t = 0; t < nTextures; t++) {
        const uint32_t* h = take(3);
        tex[t] = Tex{h[0], h[1], h[2], (uint32_t)store.size()};
        if (h[0] == 0u || h[1] == 0u || h[2] == 0u || h[2] > CHORD_MAX_TEX_LEVELS) return 2;
        size_t texels = 0;
        for (uint32_t l = 0; l < h[2]; l++) texels += (size_t)std::max(1u, h[0] >> l) * std::max(1u, h[1] >> l);
        const uint32_t* w = take(texels);
        store.insert(store.end(), w, w + texels);
    }
    uint32_t* texels = exact<uint32_t>(store.data(), store.size());

    DMatRecord* recs = static_cast<DMatRecord*>(std::malloc(nMaterials ? nMaterials * sizeof(DMatRecord) : 1u));
    for (uint32_t m = 0; m < nMaterials; m++) {
        const ChordMaterial& mat = mats[m];
        DMatRecord& d = recs[m];
        std::memset(&d, 0, sizeof(d));
        std::memcpy(d.baseColorFactor, mat.baseColorFactor, 16); std::memcpy(d.emissiveFactor, mat.emissiveFactor, 12);
        d.roughnessFactor = mat.roughnessFactor; d.metallicFactor = mat.metallicFactor; d.normalFactorScale = mat.normalFactorScale;
        d.occlusionTextureStrength = mat.occlusionTextureStrength; d.bExistOcclusion = mat.bExistOcclusion != 0u;
        d.pbr = mat.materialType == 1u;
        d.twoSided = mat.bTwoSided != 0u;
        const uint32_t tid[4] = {mat.baseColorId, mat.emissiveTexture, mat.normalTexture, mat.metallicRoughnessTexture};
        const uint32_t sid[4] = {mat.baseColorSampler, mat.emissiveSampler, mat.normalSampler, mat.metallicRoughnessSampler};
        for (int k = 0; k < 4; k++) {
            DMatSlot& S = d.slot[k];
            ChordSampler sm{CHORD_FILTER_NEAREST, CHORD_FILTER_NEAREST, CHORD_WRAP_REPEAT, CHORD_WRAP_REPEAT};
            if (sid[k] < nSamplers) sm = samplers[sid[k]];
            S.wrapS = sm.wrapS; S.wrapT = sm.wrapT;
            S.filter = (linear_filter(sm.magFilter) ? CHORD_MATSLOT_MAG_LINEAR : 0u) | (linear_filter(sm.minFilter) ? CHORD_MATSLOT_MIN_LINEAR : 0u) |
                       ((sm.minFilter == CHORD_FILTER_NEAREST_MIPMAP_NEAREST || sm.minFilter == CHORD_FILTER_LINEAR_MIPMAP_NEAREST) ? CHORD_MATSLOT_MIP_NEAREST : 0u) |
                       ((sm.minFilter == CHORD_FILTER_NEAREST_MIPMAP_LINEAR || sm.minFilter == CHORD_FILTER_LINEAR_MIPMAP_LINEAR) ? CHORD_MATSLOT_MIP_LINEAR : 0u);
            if (tid[k] >= nTextures) continue;
            const Tex& tx = tex[tid[k]];
            S.mips = tx.mips; S.texture = tid[k];
            uint32_t off = tx.base;
            for (uint32_t l = 0; l < S.mips; l++) {
                const uint32_t w = std::max(1u, tx.width >> l), h = std::max(1u, tx.height >> l);
                DMatLevel& L = S.levels[l];
                L.base = off; L.dims = (w - 1u) | (h - 1u) << 16;
                wrap_consts(w, S.wrapS, L.magicS, L.biasS);
                wrap_consts(h, S.wrapT, L.magicT, L.biasT);
                off += w * h;
            }
        }
    }
    uint4* hits = exact<uint4>(take((size_t)nHits * 8u), (size_t)nHits * 2u);
    float* lods = hasLods ? exact<float>(take(nHits), nHits) : nullptr;
    if (at != req.size()) return 2;

    s.objects = objects; s.meshlets = meshlets; s.materials = recs; s.primVertexBase = primVertexBase; s.primAssetMeshlets = primAssetMeshlets; s.meshletData = data; s.texcoords = texcoords; s.normals = normals;
    s.texels = texels; s.blocks = nullptr;
    s.objectCount = nObjects; s.meshletCount = nMeshlets; s.primCount = nPrims; s.materialCount = nMaterials; s.dataWords = nData; s.vertexCount = nVertices;
    float table[256], ap1[9];
    std::memcpy(table, kSrgbBits, sizeof(table));
    std::memcpy(ap1, kAp1Bits, sizeof(ap1));

    std::vector<uint4> out((size_t)nHits * 4u);
    for (uint32_t i = 0; i < nHits; i++)
        shade_ray_hit<false>(s, hits[2u * i], hits[2u * i + 1u], lods ? lods[i] : lod, table, ap1, &out[4u * i]);

    std::free(objects); std::free(primVertexBase); std::free(primAssetMeshlets); std::free(meshlets); std::free(data); std::free(texcoords); std::free(normals); std::free(texels); std::free(recs);
    std::free(hits); std::free(lods);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    const bool ok = out.empty() || std::fwrite(out.data(), 16, out.size(), o) == out.size();
    std::fclose(o);
    return ok ? 0 : 2;
}
