// chordvis -- shading one ray hit (chordvis_shade_ray_hits; include/chordvis.h RAY QUERIES): the counterpart of
// RayHitMaterialInfo::init (raytrace_shared.hlsli) over the pinned sampler of material_sampler.h.  The answer is tests/
// spec_ray_shade_np.shade's word for word.  Everything here is float32 / integer C++ in source order behind __device__, so the host
// compiler builds it too: tests/ray_shade_main.cpp runs shade_ray_hit under the address and undefined-behaviour sanitizers over arrays
// of exactly their size, and kernels_rayshade.hip runs the same statements a hit per lane.
//
// Every index is compared with the COUNT of its array before it is used, in the order of the specification's validate: status bit 0 and
// finite u, v; the object; the object's primitive and material ids; the meshlet against the meshlet count of the primitive's ASSET; the
// triangle against the meshlet's count; the triangle word; the three vertex-id words and the three vertex ids.  An invalid hit gives
// sixteen zero words and reads nothing further.
//
// The hit's meshlet is ASSET-RELATIVE, as chordvis_trace_rays and chordvis_pixel_rays write it (ChordRayHit::meshlet): it is read at
// primAssetMeshlets[primitive].x + meshlet of the concatenated meshlet array, and is valid below primAssetMeshlets[primitive].y, the
// asset's own count.  With one asset the pair is (0, the scene's meshlet count).
#pragma once

#include "device_layer.h"
#include "material_sampler.h"

namespace chord {

struct RayShadeScene {             // pointers and the counts of what they point at
    const ChordObject* objects;    // the array the frames read now
    const DMeshlet* meshlets;
    const DMatRecord* materials;
    const uint32_t* primVertexBase; // per primitive: its vertexOffset, made global over the assets
    const uint2* primAssetMeshlets; // per primitive: (first meshlet, meshlet count) of its asset in `meshlets`, or null: ONE asset, (0, meshletCount)
    const uint32_t* meshletData;
    const float* texcoords;        // float2 per vertex, or null: uv (0, 0)
    const float* normals;          // float3 per vertex, or null: a zero normal
    const uint32_t* texels;        // the texel store
    const uint2* blocks;           // the block store (kBlocks), or null
    uint32_t objectCount, meshletCount, primCount, materialCount, dataWords, vertexCount;
};

// what the geometry half hands the material half
struct RayShadeHit {
    bool     valid;
    uint32_t material, flags;      // CHORD_RAYSURF_VALID | BACK_FACE (TWO_SIDED and PBR come from the material)
    float    u, v;                 // the texture coordinates
    float    n[3];                 // the interpolated, normalised vertex normal, not yet flipped
    int32_t  lodq;
};

__device__ __forceinline__ uint32_t rs_bits(float x) { uint32_t w; __builtin_memcpy(&w, &x, 4); return w; }
__device__ __forceinline__ float rs_float(uint32_t w) { float x; __builtin_memcpy(&x, &w, 4); return x; }
__device__ __forceinline__ bool rs_finite(uint32_t w) { return (w & 0x7F800000u) != 0x7F800000u; }

// v / sqrt(dot(v, v)) per component, 0 where dot(v, v) is not above 0 (spec_surface_np.normalize; kernels_resolve.hip normalize_or_zero)
__device__ __forceinline__ void rs_normalize(float v[3])
{
    const float l2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    if (!(l2 > 0.0f)) { v[0] = 0.0f; v[1] = 0.0f; v[2] = 0.0f; return; }
    const float s = sqrtf(l2);
    v[0] = v[0] / s; v[1] = v[1] / s; v[2] = v[2] / s;
}

// lodq = (int32) floor(min(max(lod, 0), 15) * 256), NaN -> 0
__device__ __forceinline__ int32_t rs_lodq(float lod)
{
    float l = lod > 0.0f ? lod : 0.0f;
    l = l < 15.0f ? l : 15.0f;
    return (int32_t)floorf(l * 256.0f);
}

// Validation, the walk to the three vertex ids, b, uv, the vertex normals through translatedWorldToLocal, normalise, interpolate,
// normalise, and the lodq.  h0 = (t, u, v, object), h1 = (meshlet, triangle, primitive, status): the two halves of a ChordRayHit.
__device__ __forceinline__ void ray_shade_geometry(const RayShadeScene& s, uint4 h0, uint4 h1, float lod, RayShadeHit& o)
{
    o.valid = false; o.material = 0u; o.flags = 0u; o.u = 0.0f; o.v = 0.0f; o.n[0] = 0.0f; o.n[1] = 0.0f; o.n[2] = 0.0f; o.lodq = 0;
    const uint32_t status = h1.w, object = h0.w, meshlet = h1.x, triangle = h1.y;
    if (!(status & CHORD_RAY_HIT) || !rs_finite(h0.y) || !rs_finite(h0.z)) return;
    if (object >= s.objectCount) return;
    const ChordObject& ob = s.objects[object];
    const uint32_t prim = ob.GLTFPrimitiveDetail, mat = ob.GLTFMaterialData;
    if (prim >= s.primCount || mat >= s.materialCount) return;
    // (first meshlet, count) of the primitive's asset; a scene handed over without the table is one asset
    const uint2 asset = s.primAssetMeshlets ? s.primAssetMeshlets[prim] : make_uint2(0u, s.meshletCount);
    if (meshlet >= asset.y || (uint64_t)asset.x + meshlet >= s.meshletCount) return;
    const DMeshlet& m = s.meshlets[asset.x + meshlet];
    const uint32_t vtc = m.vertexTriangleCount, V = vtc & 0xFFu, T = (vtc >> 8) & 0xFFu;
    if (triangle >= T) return;
    const uint64_t base = m.dataOffset, vertexBase = s.primVertexBase[prim];   // (the OBJECT's primitive's vertexOffset, as the specification's)
    const uint64_t at = base + V + triangle;
    if (at >= s.dataWords) return;
    const uint32_t triWord = s.meshletData[at];
    size_t vi[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint64_t w = base + ((triWord >> (8 * k)) & 0xFFu);
        if (w >= s.dataWords) return;
        const uint64_t id = (uint64_t)s.meshletData[w] + vertexBase;
        if (id >= s.vertexCount) return;
        vi[k] = (size_t)id;
    }
    o.valid = true;
    o.material = mat;
    o.flags = CHORD_RAYSURF_VALID | ((status & CHORD_RAY_BACK_FACE) ? CHORD_RAYSURF_BACK_FACE : 0u);
    o.lodq = rs_lodq(lod);
    const float hu = rs_float(h0.y), hv = rs_float(h0.z);
    const float b[3] = {(1.0f - hu) - hv, hu, hv};
    if (s.texcoords) {
        const float* t0 = s.texcoords + vi[0] * 2u; const float* t1 = s.texcoords + vi[1] * 2u; const float* t2 = s.texcoords + vi[2] * 2u;
        o.u = (t0[0] * b[0] + t1[0] * b[1]) + t2[0] * b[2];
        o.v = (t0[1] * b[0] + t1[1] * b[1]) + t2[1] * b[2];
    }
    if (s.normals) {
        // nRS = normalize(mul(float4(nLS, 0), translatedWorldToLocal).xyz): the row-vector product, component j = (x * m0j + y * m1j)
        // + z * m2j with mij = m[j * 4 + i] (kernels_resolve.hip states the same for the surface resolve, which does not renormalise)
        const float* W = ob.basicData.translatedWorldToLocal.m;
        float nv[3][3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float* nl = s.normals + vi[k] * 3u;
            const float x = nl[0], y = nl[1], z = nl[2];
#pragma unroll
            for (int j = 0; j < 3; j++) nv[k][j] = (x * W[j * 4] + y * W[j * 4 + 1]) + z * W[j * 4 + 2];
            rs_normalize(nv[k]);
        }
#pragma unroll
        for (int j = 0; j < 3; j++) o.n[j] = (nv[0][j] * b[0] + nv[1][j] * b[1]) + nv[2][j] * b[2];
        rs_normalize(o.n);                                                 // raytrace_shared.hlsli:92
    }
}

// The flip, the flags and the three slots from one material record.  M is the lane's own record: only the words named here and what
// sample_slot_lod reads of a slot are loaded.  ap1: the nine floats of sRGB -> AP1, row-major.
template <bool kBlocks>
__device__ __forceinline__ void ray_shade_material(const RayShadeScene& s, const DMatRecord& M, const RayShadeHit& h, const float* srgb, const float* ap1,
                                                   uint4 out[4])
{
    const bool twoSided = M.twoSided != 0u, pbr = M.pbr != 0u;
    const bool flip = twoSided && (h.flags & CHORD_RAYSURF_BACK_FACE) != 0u;
    const float nx = flip ? -h.n[0] : h.n[0], ny = flip ? -h.n[1] : h.n[1], nz = flip ? -h.n[2] : h.n[2];
    const uint32_t flags = h.flags | (twoSided ? CHORD_RAYSURF_TWO_SIDED : 0u) | (pbr ? CHORD_RAYSURF_PBR : 0u);
    float4 base = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float er = 0.0f, eg = 0.0f, eb = 0.0f, rough = 0.0f, metal = 0.0f;
    if (pbr) {                                                             // (another materialType leaves the material fields zero)
        TexelStores<kBlocks> T;
        T.texels = s.texels;
        if constexpr (kBlocks) T.blocks = s.blocks;
        {
            const DMatSlot& S = M.slot[CHORD_MATSLOT_BASECOLOR];
            float4 c = make_float4(1.0f, 1.0f, 1.0f, 1.0f);                // the white fallback
            if (S.mips) {
                if constexpr (kBlocks) T.format = S.format;
                c = sample_slot_lod<true, kBlocks>(T, S, h.u, h.v, h.lodq, srgb);
            }
            const float r = c.x * M.baseColorFactor[0], g = c.y * M.baseColorFactor[1], b = c.z * M.baseColorFactor[2];
            base = make_float4((ap1[0] * r + ap1[1] * g) + ap1[2] * b, (ap1[3] * r + ap1[4] * g) + ap1[5] * b, (ap1[6] * r + ap1[7] * g) + ap1[8] * b,
                               c.w * M.baseColorFactor[3]);
        }
        {
            const DMatSlot& S = M.slot[CHORD_MATSLOT_EMISSIVE];
            float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);                // the transparent-black fallback
            if (S.mips) {
                if constexpr (kBlocks) T.format = S.format;
                c = sample_slot_lod<true, kBlocks>(T, S, h.u, h.v, h.lodq, srgb);
            }
            er = c.x * M.emissiveFactor[0]; eg = c.y * M.emissiveFactor[1]; eb = c.z * M.emissiveFactor[2];   // (not through sRGB -> AP1)
        }
        {
            const DMatSlot& S = M.slot[CHORD_MATSLOT_METALROUGH];
            rough = M.roughnessFactor; metal = M.metallicFactor >= 1.0f ? 0.0f : M.metallicFactor;           // gltf.h:53-58
            if (S.mips) {
                if constexpr (kBlocks) T.format = S.format;
                const float4 c = sample_slot_lod<false, kBlocks>(T, S, h.u, h.v, h.lodq, srgb);
                rough = c.y; metal = c.z;
            }
        }
    }
    out[0] = make_uint4(rs_bits(base.x), rs_bits(base.y), rs_bits(base.z), rs_bits(base.w));
    out[1] = make_uint4(rs_bits(er), rs_bits(eg), rs_bits(eb), rs_bits(rough));
    out[2] = make_uint4(rs_bits(nx), rs_bits(ny), rs_bits(nz), rs_bits(metal));
    out[3] = make_uint4(rs_bits(h.u), rs_bits(h.v), h.material, flags);
}

// One hit, whole: the sixteen words of its ChordRayHitSurface.
template <bool kBlocks>
__device__ __forceinline__ void shade_ray_hit(const RayShadeScene& s, uint4 h0, uint4 h1, float lod, const float* srgb, const float* ap1, uint4 out[4])
{
    RayShadeHit h;
    ray_shade_geometry(s, h0, h1, lod, h);
    if (!h.valid) {
        out[0] = out[1] = out[2] = out[3] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    ray_shade_material<kBlocks>(s, s.materials[h.material], h, srgb, ap1, out);
}

} // namespace chord
