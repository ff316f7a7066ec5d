// chordvis -- shading ray hits (chordvis_shade_ray_hits; include/chordvis.h RAY QUERIES).  The reference's consumers
// of TraceRayInline other than the AO pass (ddgi_probe_trace.hlsl, gi_screen_probe_*.hlsl, gi_specular_trace.hlsl) go on to
// RayHitMaterialInfo::init (raytrace_shared.hlsli); this is that step for the hits of chordvis_trace_rays, or a host's own.
//
//   ray_shade_kernel    wave64, a hit per lane, four waves per workgroup.  The per-hit code is ray_shade.h's shade_ray_hit (which the
//                       host compiler builds too and tests/ray_shade_main.cpp runs under the sanitizers): two 16-byte loads of the hit,
//                       the walk object -> primitive -> asset-relative meshlet -> triangle word -> three vertex ids with every index checked against its count,
//                       uv and the normal at the barycentrics, and the three material slots at an explicit level through the pinned
//                       sampler.  The sRGB table is in LDS, as in the resolve kernels.  Four plain 16-byte stores per lane.
//
// Arithmetic: binary32, no contraction, correctly rounded divide and square root, subnormals kept.

#include "device_layer.h"
#include "material_tables.h"
#include "ray_shade.h"

namespace chord {

namespace {

__device__ const uint32_t kShadeSrgbBits[256] = {CHORD_SRGB_TABLE_BITS};
__device__ const uint32_t kShadeSrgb2Ap1Bits[9] = {CHORD_SRGB_2_AP1_BITS};

}  // namespace

struct RayShadeArgs {
    RayShadeScene scene;
    const uint4* hits;             // two per hit
    const float* lods;             // null: `lod` for every hit
    uint4* out;                    // four per hit
    uint32_t count;
    float lod;
};

template <bool kBlocks>
__global__ __launch_bounds__(256) void ray_shade_kernel(const RayShadeArgs a)
{
    __shared__ float sSrgb[256];
    sSrgb[threadIdx.x] = __uint_as_float(kShadeSrgbBits[threadIdx.x]);
    __syncthreads();
    float ap1[9];
#pragma unroll
    for (int k = 0; k < 9; k++) ap1[k] = __uint_as_float(kShadeSrgb2Ap1Bits[k]);
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= a.count) return;
    // Lanes of a wave may name different materials: each lane loads the words of its own DMatRecord that it needs.  A waterfall over
    // the wave's distinct materials (wave-uniform slot constants through scalar loads) was built and measured slower on every hit
    // set and in both stores -- 3 to 9 % in pixel order, 4 to 40 % shuffled, 15 to 27 % with alternating materials -- and is gone
    // (profiles/ray_shade_time.txt).
    uint4 out[4];
    shade_ray_hit<kBlocks>(a.scene, a.hits[2u * i], a.hits[2u * i + 1u], a.lods ? a.lods[i] : a.lod, sSrgb, ap1, out);
#pragma unroll
    for (int k = 0; k < 4; k++) a.out[4u * i + k] = out[k];
}

void launch_ray_shade(ChordCtx* c, const ChordRayHit* hits, uint32_t count, float lod, const float* lods, ChordRayHitSurface* surfaces)
{
    RayShadeArgs a;
    RayShadeScene& s = a.scene;
    s.objects = c->dObjects; s.meshlets = c->dMeshlets; s.materials = c->dMatRecords; s.primVertexBase = c->dPrimVertexBase;
    s.primAssetMeshlets = c->dPrimAssetMeshlets; s.meshletData = c->dMeshletData;
    s.texcoords = c->dTexcoords; s.normals = c->dNormals;
    s.texels = c->dMatTexels; s.blocks = reinterpret_cast<const uint2*>(c->dMatBlocks);
    s.objectCount = c->objectCount; s.meshletCount = c->meshletCount; s.primCount = c->primCount; s.materialCount = c->materialCount;
    s.dataWords = c->meshletDataWords; s.vertexCount = c->vertexTotal;
    a.hits = reinterpret_cast<const uint4*>(hits); a.lods = lods; a.out = reinterpret_cast<uint4*>(surfaces);
    a.count = count; a.lod = lod;
    const dim3 grid((uint32_t)(((uint64_t)count + 255u) / 256u)), block(256);
    // the block store's kernel only where some chain is kept as blocks: the texel store's carries no block decode
    if (c->matBlockUnits) CHORD_LAUNCH(c, ray_shade_kernel<true>, grid, block, 0, c->stream, a);
    else CHORD_LAUNCH(c, ray_shade_kernel<false>, grid, block, 0, c->stream, a);
}

} // namespace chord
