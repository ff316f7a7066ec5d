// Texel addressing shared by the raster's alpha test (raster_device.h sample_alpha) and the material resolve
// (kernels_resolve.hip): floor of a texel coordinate with the +-1e9 guard, and the three wrap modes with the level's
// precomputed remainder constants (DMatLevel).  One definition, so the two samplers address texels identically.
#pragma once

#include "device_layer.h"

namespace chord {

// Texel indices are 32-bit here: texel_floor maps everything beyond +-1e9 to 0, so an index and its +1 neighbour fit an int32
// (the oracle's 64-bit arithmetic gives the same values); a 64-bit modulo is ~200 instructions on this GPU and the bilinear
// fetch of round 2 did eight of them per covered pixel.  Power-of-two periods (every level of a power-of-two texture) wrap with
// a mask: i & (n - 1) is the non-negative remainder in two's complement.  Any other period divides by a constant of the level
// (DMatLevel: magic = floor(2^32 / period), bias = a multiple of the period >= 2^30): iu = i + bias is in [0, 2^31) and has
// i's remainder; floor(iu * magic / 2^32) is floor(iu / period) or one less (iu * (2^32 / period - magic) / 2^32 < 1/2), so one
// multiply-high, one multiply and one conditional subtraction replace the ~50 issue slots of a 32-bit signed remainder.
__device__ __forceinline__ int32_t period_mod(int32_t i, int32_t period, uint32_t magic, uint32_t bias)
{
    if (magic == 0u) return i & (period - 1);
    const uint32_t iu = (uint32_t)i + bias;
    uint32_t r = iu - __umulhi(iu, magic) * (uint32_t)period;
    if (r >= (uint32_t)period) r -= (uint32_t)period;
    return (int32_t)r;
}
__device__ __forceinline__ int32_t wrap_index(int32_t i, int32_t n, uint32_t mode, uint32_t magic, uint32_t bias)
{
    if (mode == CHORD_WRAP_CLAMP_TO_EDGE) return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
    if (mode == CHORD_WRAP_MIRRORED_REPEAT) {
        const int32_t m = period_mod(i, 2 * n, magic, bias);
        return m < n ? m : 2 * n - 1 - m;
    }
    return period_mod(i, n, magic, bias);
}

// wrap_index(i) and wrap_index(i + 1) with ONE remainder: the neighbour's follows from the remainder's successor
__device__ __forceinline__ void wrap_pair(int32_t i, int32_t n, uint32_t mode, uint32_t magic, uint32_t bias, int32_t& w0, int32_t& w1)
{
    if (mode == CHORD_WRAP_CLAMP_TO_EDGE) {
        w0 = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
        w1 = i + 1 < 0 ? 0 : (i + 1 > n - 1 ? n - 1 : i + 1);
        return;
    }
    const bool mirror = mode == CHORD_WRAP_MIRRORED_REPEAT;
    const int32_t period = mirror ? 2 * n : n;
    const int32_t m = period_mod(i, period, magic, bias);
    const int32_t m1 = m + 1 == period ? 0 : m + 1;                          // (i + 1) mod period
    w0 = mirror ? (m < n ? m : 2 * n - 1 - m) : m;
    w1 = mirror ? (m1 < n ? m1 : 2 * n - 1 - m1) : m1;
}

__device__ __forceinline__ int32_t texel_floor(float x)
{
    if (!(fabsf(x) < 1.0e9f)) return 0;
    return (int32_t)floorf(x);
}

} // namespace chord
