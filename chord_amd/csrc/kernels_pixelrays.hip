// chordvis -- pixel rays (chordvis_pixel_rays; include/chordvis.h RAY QUERIES, "pixel rays"): the reference's
// gi_rt_ao.hlsl -- one ray per pixel from the G-buffer position about the G-buffer normal, the closest hit's distance as the AO term --
// and a sun-shadow mask, over the ray scene of kernels_rays.hip.
//
//   pixel_rays_kernel   wave64, a pixel per lane, a wave per 8 x 8 pixel block (pixel_rays.h pixel_of_lane), the stack of
//                       ray::kStackEntries words per lane in scratch as in ray_trace_kernel.  It loads the pixel's position, normal,
//                       depth and table texel, forms the ray (make_pixel_ray), walks it (ray_walk.h walk_ray, unchanged) and stores the
//                       answer (finish_pixel_ray): one float, and the two vectors of the ChordRayHit when they are asked for.  The ray
//                       never reaches memory.  Lanes outside the image leave; invalid and fixed-answer pixels skip the walk and still
//                       write their answer.
//
// The per-pixel statements are pixel_rays.h's, which the host compiler builds too (tests/pixel_rays_main.cpp); what stays here is
// indexing, loads and stores.  Arithmetic: binary32, no contraction, correctly rounded divide and square root, subnormals kept.

#include "device_layer.h"
#include "device_math.h"
#include "ray_scene.h"
#include "ray_walk.h"
#include "pixel_rays.h"

namespace chord {

struct PixelRaysArgs {
    const float4* position;        // width x height
    const float4* normal;          // width x height, or null where no statement reads it (DIRECTION without FRONT_ONLY)
    const float* z;                // the pixel's depth at z[i * desc.deviceZStride], or null
    const float4* table;           // desc.tableW x desc.tableH (HEMISPHERE), or null
    float* out;                    // width x height
    uint4* hits;                   // ChordRayHit as two vectors, or null
    const ChordObject* objects;    // from here on ray_walk.h's RayWalkScene, member for member
    const DObjStatic* objStatic;
    const ray::Node* tlas;
    const float4* leafBox;
    const uint32_t* blasRoot;
    const ray::Node* blas;
    const float4* triangles;
    uint32_t objectCount, primCount, tlasNodes, blasNodes, triangleCount;
    uint32_t gridX;                // the launch's gridDim.x: the wave is blockIdx.y * gridX + blockIdx.x
    uint64_t waves;                // pixel_wave_count(width, height)
    ChordPixelRaysDesc desc;
};

template <bool ANY>
__global__ __launch_bounds__(64) void pixel_rays_kernel(const PixelRaysArgs a)
{
    const uint64_t wave = (uint64_t)blockIdx.y * a.gridX + blockIdx.x;
    if (wave >= a.waves) return;
    uint64_t x, y;
    pixel_of_lane(wave, threadIdx.x, a.desc.width, x, y);
    if (x >= a.desc.width || y >= a.desc.height) return;
    const uint64_t i = y * a.desc.width + x;                                   // (below width * height, which fits 32 bits; 2 i + 1 does not)

    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 p = a.position[i];
    const float4 nrm = a.normal ? a.normal[i] : zero4;
    const float z = a.z ? a.z[i * a.desc.deviceZStride] : 0.0f;
    const float4 dT = a.table ? a.table[table_index((uint32_t)x, (uint32_t)y, a.desc.tableW, a.desc.tableH)] : zero4;
    const PixelRay r = make_pixel_ray(a.desc, p, nrm, a.z != nullptr, z, dT);

    float out = r.disposition == kPixelZero ? 0.0f : 1.0f;
    RayWords w;
    w.h0 = make_uint4(0u, 0u, 0u, 0u); w.h1 = make_uint4(0u, 0u, 0u, 0u);
    if (r.disposition == kPixelTrace) {
        RayNoStats stats;
        uint32_t stack[ray::kStackEntries];
        w = walk_ray<ANY>(a, r.r0, r.r1, stack, stats);
        out = finish_pixel_ray<ANY>(w, a.desc.rayLength);
    }
    a.out[i] = out;
    if (!ANY && a.hits) {
        a.hits[2u * i] = w.h0;
        a.hits[2u * i + 1u] = w.h1;
    }
}

void launch_pixel_rays(ChordCtx* c, const ChordPixelRaysDesc& desc, const float* position, const float* normal, const float* z, const float* table,
                       float* out, ChordRayHit* hits)
{
    PixelRaysArgs a;
    a.position = reinterpret_cast<const float4*>(position); a.normal = reinterpret_cast<const float4*>(normal); a.z = z;
    a.table = reinterpret_cast<const float4*>(table); a.out = out; a.hits = reinterpret_cast<uint4*>(hits);
    a.objects = c->dObjects; a.objStatic = c->dObjStatic;
    a.tlas = c->dRayTlas; a.leafBox = reinterpret_cast<const float4*>(c->dRayLeafBox);
    a.blasRoot = c->dRayBlasRoot; a.blas = c->dRayBlas; a.triangles = reinterpret_cast<const float4*>(c->dRayTriangles);
    a.objectCount = c->objectCount; a.primCount = c->primCount;
    a.tlasNodes = c->rayTlasNodes; a.blasNodes = c->rayBlasNodes; a.triangleCount = c->rayBlasTriangles;
    a.desc = desc;
    a.waves = pixel_wave_count(desc.width, desc.height);
    // (a wave per workgroup; more waves than one grid dimension holds go into the second)
    const uint64_t kRow = 1ull << 20;
    a.gridX = (uint32_t)(a.waves < kRow ? a.waves : kRow);
    const dim3 grid(a.gridX, (uint32_t)((a.waves + a.gridX - 1u) / a.gridX)), block(64);
    if (desc.flags & CHORD_PIXEL_RAYS_ANY_HIT) CHORD_LAUNCH(c, pixel_rays_kernel<true>, grid, block, 0, c->stream, a);
    else CHORD_LAUNCH(c, pixel_rays_kernel<false>, grid, block, 0, c->stream, a);
}

} // namespace chord
