// chordvis -- one pixel's ray from the G-buffer and its answer (chordvis_pixel_rays; include/chordvis.h RAY QUERIES, "pixel rays";
// DESIGN.md 4.18): the ray generation of gi_rt_ao.hlsl:40-75 and the reduction of its closest hit to one float.  The answer is tests/
// spec_pixel_rays_np.pixel_rays' word for word.  Everything here is float32 / integer C++ in source order behind __device__, so the
// host compiler builds it too: tests/pixel_rays_main.cpp runs make_pixel_ray -> walk_ray -> finish_pixel_ray under the address and
// undefined-behaviour sanitizers over images of exactly their size, and kernels_pixelrays.hip runs the same statements a pixel per lane.
//
//   make_pixel_ray     the pixel's position, normal, device depth and table texel, and the desc -> the two halves of its ChordRay and a
//                      disposition: trace it, or a fixed answer (1: an invalid pixel; 0: FRONT_ONLY and the normal faces away).
//   finish_pixel_ray   the RayWords of walk_ray -> out.
//   pixel_of_lane      which pixel a lane of a wave takes: an 8 x 8 block per wave, blocks in row-major order (DESIGN.md 4.18 has the
//                      measurement); CHORD_PIXEL_RAYS_ROWS=1 deals 64 x 1 row segments instead, for that measurement only.
//   table_index        the texel of a pixel: both coordinates masked with the table's power-of-two size.
// The walk between the two is ray_walk.h's walk_ray, unchanged.  There is no transcendental here: the hemisphere directions come from a
// table the host baked (uniformSampleHemisphere of its blue noise, one slice per frame), and the reference's pow(out, power) stays with
// the consumer, whose denoiser reads the image next -- no pow is pinned on the device.
//
// Arithmetic: binary32, no contraction, correctly rounded divide and square root, subnormals kept; min and max are ray_walk.h's selects.
#pragma once

#include "ray_walk.h"

namespace chord {

enum PixelDisposition : uint32_t { kPixelTrace = 0u, kPixelOne = 1u, kPixelZero = 2u };

struct PixelRay {
    float4 r0, r1;                 // (origin, tMin), (direction, tMax)
    uint32_t disposition;
};

#ifndef CHORD_PIXEL_RAYS_ROWS
#define CHORD_PIXEL_RAYS_ROWS 0
#endif

// the waves that cover a width x height image
__host__ __device__ __forceinline__ uint64_t pixel_wave_count(uint32_t width, uint32_t height)
{
#if CHORD_PIXEL_RAYS_ROWS
    return (((uint64_t)width + 63u) / 64u) * height;
#else
    return (((uint64_t)width + 7u) / 8u) * (((uint64_t)height + 7u) / 8u);
#endif
}

// lane `lane` of wave `wave`: its pixel, which may lie outside the image (the caller compares x < width, y < height)
__host__ __device__ __forceinline__ void pixel_of_lane(uint64_t wave, uint32_t lane, uint32_t width, uint64_t& x, uint64_t& y)
{
#if CHORD_PIXEL_RAYS_ROWS
    const uint64_t perRow = ((uint64_t)width + 63u) / 64u;
    x = (wave % perRow) * 64u + lane;
    y = wave / perRow;
#else
    const uint64_t blocksX = ((uint64_t)width + 7u) / 8u;
    x = (wave % blocksX) * 8u + (lane & 7u);
    y = (wave / blocksX) * 8u + (lane >> 3);
#endif
}

// tableW, tableH: powers of two (the entry point refuses anything else), so the masked coordinates lie inside the table
__host__ __device__ __forceinline__ uint64_t table_index(uint32_t x, uint32_t y, uint32_t tableW, uint32_t tableH)
{
    return (uint64_t)(y & (tableH - 1u)) * tableW + (x & (tableW - 1u));
}

// hasZ: a depth image was given, z is the pixel's word of it.  dT: the pixel's table texel (HEMISPHERE; anything otherwise).
__device__ __forceinline__ PixelRay make_pixel_ray(const ChordPixelRaysDesc& d, const float4& p, const float4& nrm, bool hasZ, float z, const float4& dT)
{
    PixelRay r;
    r.r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f); r.r1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    r.disposition = kPixelOne;
    const bool valid = hasZ ? z > 0.0f : p.w != 0.0f;
    if (!valid) return r;

    // normalize of chordvis_resolve_surface: v / sqrt(dot(v, v)) per component, 0 where dot(v, v) is not above 0
    float n[3] = {nrm.x, nrm.y, nrm.z};
    const float l2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    if (l2 > 0.0f) {
        const float s = sqrtf(l2);
        n[0] = n[0] / s; n[1] = n[1] / s; n[2] = n[2] / s;
    } else {
        n[0] = 0.0f; n[1] = 0.0f; n[2] = 0.0f;
    }

    float dir[3];
    if (d.mode == CHORD_PIXEL_RAYS_HEMISPHERE) {
        // createTBN, base.hlsli:1001-1025
        float u[3];
        if (__builtin_fabsf(n[2]) > 0.0f) {
            const float k = sqrtf(n[1] * n[1] + n[2] * n[2]);
            u[0] = 0.0f; u[1] = -n[2] / k; u[2] = n[1] / k;
        } else {
            const float k = sqrtf(n[0] * n[0] + n[1] * n[1]);
            u[0] = n[1] / k; u[1] = -n[0] / k; u[2] = 0.0f;
        }
        const float b[3] = {n[1] * u[2] - n[2] * u[1], n[2] * u[0] - n[0] * u[2], n[0] * u[1] - n[1] * u[0]};
#pragma unroll
        for (int k = 0; k < 3; k++) dir[k] = (dT.x * u[k] + dT.y * b[k]) + dT.z * n[k];
    } else {
        dir[0] = d.direction[0]; dir[1] = d.direction[1]; dir[2] = d.direction[2];
        if (d.flags & CHORD_PIXEL_RAYS_FRONT_ONLY) {
            const float facing = (n[0] * dir[0] + n[1] * dir[1]) + n[2] * dir[2];
            if (!(facing > 0.0f)) { r.disposition = kPixelZero; return r; }
        }
    }

    float tMin = d.tMin;
    if (d.flags & CHORD_PIXEL_RAYS_START_FROM_DEPTH) {
        // getRayTraceStartOffset, raytrace_shared.hlsli:10-17
        const float lin = d.zNear / z;
        const float s = lin * 0.01f;
        const float w = s / (s + 1.0f);
        tMin = 5e-3f + w * (1e-1f - 5e-3f);
    }
    r.r0 = make_float4(p.x, p.y, p.z, tMin);
    r.r1 = make_float4(dir[0], dir[1], dir[2], d.rayLength);
    r.disposition = kPixelTrace;
    return r;
}

// closest: t / rayLength clamped to [0, 1], 1 on a miss; any-hit: 0 when a candidate exists, 1 otherwise
template <bool ANY>
__device__ __forceinline__ float finish_pixel_ray(const RayWords& w, float rayLength)
{
    if (!(w.h1.w & CHORD_RAY_HIT)) return 1.0f;
    if (ANY) return 0.0f;
    float t;
    const uint32_t bits = w.h0.x;
    __builtin_memcpy(&t, &bits, 4);
    return rmin(rmax(t / rayLength, 0.0f), 1.0f);
}

} // namespace chord
