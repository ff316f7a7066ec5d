// The pinned decode of block-compressed textures: integers only, floor divisions.  ONE definition for the
// upload decoder (kernels_texture.hip: a lane expands a whole block) and for the material resolve's sampler when it reads a chain
// kept as blocks (kernels_resolve.hip: a lane decodes the texels of its footprint).
//
// A block is one or two 8-byte units, read as uint2 (x: bytes 0..3, y: bytes 4..7, little-endian):
//   colour unit    x = c0 | c1 << 16 (RGB565 endpoints), y = sixteen 2-bit palette indices, texel 4 * row + column least significant first
//   channel unit   x = a0 | a1 << 8 | index bits 0..15 << 16, y = index bits 16..47: sixteen 3-bit indices in the same order
//   BC1_RGB: colour.  BC3: channel (alpha), colour.  BC4: channel (r).  BC5: channel (r), channel (g).
#pragma once

#include "device_layer.h"

namespace chord {

// value k of an alpha / single-channel block with the endpoints a0, a1
__device__ __forceinline__ uint32_t bc_channel_value(uint32_t a0, uint32_t a1, uint32_t k)
{
    if (k < 2u) return k ? a1 : a0;
    if (a0 > a1) return ((8u - k) * a0 + (k - 1u) * a1) / 7u;
    if (k < 6u) return ((6u - k) * a0 + (k - 1u) * a1) / 5u;
    return k == 6u ? 0u : 255u;
}

// the 48 index bits of a channel unit, least significant first
__device__ __forceinline__ unsigned long long bc_channel_bits(uint2 q) { return ((unsigned long long)q.y << 16) | (q.x >> 16); }

// the four colours of a colour unit as R | G << 8 | B << 16.  Four-colour palette: BC3 (always), BC1 when c0 > c1; else three colours and black
__device__ __forceinline__ void bc_colour_palette(uint32_t ends, bool alwaysFour, uint32_t& p0, uint32_t& p1, uint32_t& p2, uint32_t& p3)
{
    const uint32_t c0 = ends & 0xFFFFu, c1 = ends >> 16;
    const uint32_t r0 = c0 >> 11, g0 = (c0 >> 5) & 63u, b0 = c0 & 31u, r1 = c1 >> 11, g1 = (c1 >> 5) & 63u, b1 = c1 & 31u;
    const uint32_t R0 = (r0 << 3) | (r0 >> 2), G0 = (g0 << 2) | (g0 >> 4), B0 = (b0 << 3) | (b0 >> 2);
    const uint32_t R1 = (r1 << 3) | (r1 >> 2), G1 = (g1 << 2) | (g1 >> 4), B1 = (b1 << 3) | (b1 >> 2);
    p0 = R0 | G0 << 8 | B0 << 16; p1 = R1 | G1 << 8 | B1 << 16;
    if (alwaysFour || c0 > c1) {
        p2 = (2u * R0 + R1) / 3u | ((2u * G0 + G1) / 3u) << 8 | ((2u * B0 + B1) / 3u) << 16;
        p3 = (R0 + 2u * R1) / 3u | ((G0 + 2u * G1) / 3u) << 8 | ((B0 + 2u * B1) / 3u) << 16;
    } else {
        p2 = (R0 + R1) / 2u | ((G0 + G1) / 2u) << 8 | ((B0 + B1) / 2u) << 16;
        p3 = 0u;
    }
}
// entry k of that palette
__device__ __forceinline__ uint32_t bc_palette_pick(uint32_t k, uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3) 
{
    const uint32_t lo = (k & 1u) ? p1 : p0, hi = (k & 1u) ? p3 : p2;
    return (k & 2u) ? hi : lo;
}

// texel i = 4 * row + column of a unit
__device__ __forceinline__ uint32_t bc_channel_texel(uint2 q, uint32_t i)
{
    return bc_channel_value(q.x & 0xFFu, (q.x >> 8) & 0xFFu, (uint32_t)(bc_channel_bits(q) >> (3u * i)) & 7u);
}
__device__ __forceinline__ uint32_t bc_colour_texel(uint2 q, bool alwaysFour, uint32_t i)
{
    uint32_t p0, p1, p2, p3;
    bc_colour_palette(q.x, alwaysFour, p0, p1, p2, p3);
    return bc_palette_pick((q.y >> (2u * i)) & 3u, p0, p1, p2, p3);
}

} // namespace chord
