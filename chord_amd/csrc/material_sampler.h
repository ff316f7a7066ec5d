// chordvis -- the pinned sampler as a header of its own: texel decode, one level of a slot in the texel store or in
// the block store, and the level rule from a lodq (the level of detail in 1/256 steps).  kernels_resolve.hip includes it
// (resolve_attributes_kernel<2> .. <5>: the lodq comes from screen-space uv gradients); a kernel that samples at an explicit level -- the
// shading of ray hits, DESIGN.md 4.17 -- takes the same functions with a lodq of its own.  The sRGB table is the caller's (a pointer to
// 256 floats, in LDS in the resolve kernels): each translation unit defines its own constant tables from the material_tables.h macros.
#pragma once

#include "device_layer.h"
#include "bc_decode.h"
#include "texel_wrap.h"

namespace chord {

// the texel stores a slot's levels may live in; blocks == null at compile time (kBlocks false): texels alone
template <bool kBlocks> struct TexelStores { const uint32_t* __restrict__ texels; };
template <> struct TexelStores<true> { const uint32_t* __restrict__ texels; const uint2* __restrict__ blocks; uint32_t format; };

// texel decode BEFORE filtering: alpha and linear slots byte / 255, rgb of sRGB slots through the table (in LDS)
template <bool kSrgb>
__device__ __forceinline__ float4 decode_texel(uint32_t w, const float* srgb)
{
    if constexpr (kSrgb) return make_float4(srgb[w & 255u], srgb[(w >> 8) & 255u], srgb[(w >> 16) & 255u], (float)(w >> 24) * (1.0f / 255.0f));
    return make_float4((float)(w & 255u) * (1.0f / 255.0f), (float)((w >> 8) & 255u) * (1.0f / 255.0f),
                       (float)((w >> 16) & 255u) * (1.0f / 255.0f), (float)(w >> 24) * (1.0f / 255.0f));
}

// one level, per channel sample_alpha's arithmetic (raster_device.h)
template <bool kSrgb>
__device__ __forceinline__ float4 sample_level(const uint32_t* __restrict__ texels, const DMatLevel& L, uint32_t wrapS, uint32_t wrapT, bool linear,
                                               float u, float v, const float* srgb)
{
    const int32_t W = (int32_t)(L.dims & 0xFFFFu) + 1, H = (int32_t)(L.dims >> 16) + 1;
    const float fW = (float)W, fH = (float)H;
    const uint32_t* base = texels + L.base;
    if (!linear) {
        const int32_t ix = wrap_index(texel_floor(u * fW), W, wrapS, L.magicS, L.biasS), iy = wrap_index(texel_floor(v * fH), H, wrapT, L.magicT, L.biasT);
        return decode_texel<kSrgb>(base[iy * W + ix], srgb);
    }
    const float x = u * fW - 0.5f, y = v * fH - 0.5f;
    const int32_t x0 = texel_floor(x), y0 = texel_floor(y);
    float fx = x - (float)x0, fy = y - (float)y0;
    if (!(fabsf(x) < 1.0e9f)) fx = 0.0f;
    if (!(fabsf(y) < 1.0e9f)) fy = 0.0f;
    int32_t ix0, ix1, iy0, iy1;
    wrap_pair(x0, W, wrapS, L.magicS, L.biasS, ix0, ix1);
    wrap_pair(y0, H, wrapT, L.magicT, L.biasT, iy0, iy1);
    const float4 a00 = decode_texel<kSrgb>(base[iy0 * W + ix0], srgb), a10 = decode_texel<kSrgb>(base[iy0 * W + ix1], srgb);
    const float4 a01 = decode_texel<kSrgb>(base[iy1 * W + ix0], srgb), a11 = decode_texel<kSrgb>(base[iy1 * W + ix1], srgb);
    auto bil = [&](float c00, float c10, float c01, float c11) {
        const float top = c00 + (c10 - c00) * fx, bot = c01 + (c11 - c01) * fx;
        return top + (bot - top) * fy;
    };
    return make_float4(bil(a00.x, a10.x, a01.x, a11.x), bil(a00.y, a10.y, a01.y, a11.y), bil(a00.z, a10.z, a01.z, a11.z), bil(a00.w, a10.w, a01.w, a11.w));
}

// Texel (ix, iy), already wrapped, of a level kept as blocks: the unit(s) of block (ix >> 2, iy >> 2), row-major, and DESIGN.md 2 item
// 9(h)'s decode of the one texel -- the RGBA8 word texture_decode_kernel would have stored.  format is wave-uniform.
__device__ __forceinline__ uint32_t block_texel(const uint2* __restrict__ level, uint32_t blocksPerRow, uint32_t format, int32_t ix, int32_t iy)
{
    const uint32_t b = (uint32_t)(iy >> 2) * blocksPerRow + (uint32_t)(ix >> 2), i = (uint32_t)(iy & 3) * 4u + (uint32_t)(ix & 3);
    uint2 q0, q1;                                                                       // the block's first unit, and its last (the same one in BC1_RGB and BC4)
    if (format == CHORD_TEXFMT_BC1_RGB || format == CHORD_TEXFMT_BC4) q0 = q1 = level[b];
    else {
        const uint4 q = *reinterpret_cast<const uint4*>(level + 2u * b);                // (16-byte aligned: chains are, and every level before is whole pairs)
        q0 = make_uint2(q.x, q.y); q1 = make_uint2(q.z, q.w);
    }
    uint32_t w = 0xFF000000u;
    if (format != CHORD_TEXFMT_BC1_RGB) {                                               // BC3: alpha; BC4, BC5: r
        const uint32_t v = bc_channel_texel(q0, i);
        w = format == CHORD_TEXFMT_BC3 ? v << 24 : w | v;
    }
    if (format == CHORD_TEXFMT_BC5) w |= bc_channel_texel(q1, i) << 8;                  // g
    else if (format != CHORD_TEXFMT_BC4) w |= bc_colour_texel(q1, format == CHORD_TEXFMT_BC3, i);
    return w;
}

// sample_level over a level kept as blocks: the same statements, block_texel in place of the texel load
template <bool kSrgb>
__device__ __forceinline__ float4 sample_level_blocks(const uint2* __restrict__ blocks, uint32_t format, const DMatLevel& L, uint32_t wrapS, uint32_t wrapT,
                                                      bool linear, float u, float v, const float* srgb)
{
    const int32_t W = (int32_t)(L.dims & 0xFFFFu) + 1, H = (int32_t)(L.dims >> 16) + 1;
    const float fW = (float)W, fH = (float)H;
    const uint2* base = blocks + L.base;
    const uint32_t bpr = ((L.dims & 0xFFFFu) + 4u) >> 2;
    if (!linear) {
        const int32_t ix = wrap_index(texel_floor(u * fW), W, wrapS, L.magicS, L.biasS), iy = wrap_index(texel_floor(v * fH), H, wrapT, L.magicT, L.biasT);
        return decode_texel<kSrgb>(block_texel(base, bpr, format, ix, iy), srgb);
    }
    const float x = u * fW - 0.5f, y = v * fH - 0.5f;
    const int32_t x0 = texel_floor(x), y0 = texel_floor(y);
    float fx = x - (float)x0, fy = y - (float)y0;
    if (!(fabsf(x) < 1.0e9f)) fx = 0.0f;
    if (!(fabsf(y) < 1.0e9f)) fy = 0.0f;
    int32_t ix0, ix1, iy0, iy1;
    wrap_pair(x0, W, wrapS, L.magicS, L.biasS, ix0, ix1);
    wrap_pair(y0, H, wrapT, L.magicT, L.biasT, iy0, iy1);
    // four independent fetches: taking the footprints that lie in one block (9 of 16) through a branch of their own that loads and
    // prepares the block once was measured 10 to 35 % slower -- lanes of a wave rarely agree, so it runs both paths
    const uint32_t w00 = block_texel(base, bpr, format, ix0, iy0), w10 = block_texel(base, bpr, format, ix1, iy0);
    const uint32_t w01 = block_texel(base, bpr, format, ix0, iy1), w11 = block_texel(base, bpr, format, ix1, iy1);
    const float4 a00 = decode_texel<kSrgb>(w00, srgb), a10 = decode_texel<kSrgb>(w10, srgb);
    const float4 a01 = decode_texel<kSrgb>(w01, srgb), a11 = decode_texel<kSrgb>(w11, srgb);
    auto bil = [&](float c00, float c10, float c01, float c11) {
        const float top = c00 + (c10 - c00) * fx, bot = c01 + (c11 - c01) * fx;
        return top + (bot - top) * fy;
    };
    return make_float4(bil(a00.x, a10.x, a01.x, a11.x), bil(a00.y, a10.y, a01.y, a11.y), bil(a00.z, a10.z, a01.z, a11.z), bil(a00.w, a10.w, a01.w, a11.w));
}

// one level of a slot wherever it lives
template <bool kSrgb, bool kBlocks>
__device__ __forceinline__ float4 sample_level(const TexelStores<kBlocks>& T, const DMatLevel& L, uint32_t wrapS, uint32_t wrapT, bool linear,
                                               float u, float v, const float* srgb)
{
    if constexpr (kBlocks) {
        if (T.format) return sample_level_blocks<kSrgb>(T.blocks, T.format, L, wrapS, wrapT, linear, u, v, srgb);
    }
    return sample_level<kSrgb>(T.texels, L, wrapS, wrapT, linear, u, v, srgb);
}

// S: a slot with mips > 0; u, v per lane; lodq: the level of detail in 1/256 steps, however the caller came by it (sample_slot of
// kernels_resolve.hip: from the footprint).  Minified iff lodq > 0; the rule of DESIGN.md 2 item 9(c).  S may be wave-uniform or per
// lane: only mips, filter, the wraps and the one or two levels taken are read.
template <bool kSrgb, bool kBlocks>
__device__ __forceinline__ float4 sample_slot_lod(const TexelStores<kBlocks>& texels, const DMatSlot& S, float u, float v, int32_t lodq, const float* srgb)
{
    const uint32_t filter = S.filter, last = S.mips - 1u;
    uint32_t l0 = 0u, l1 = 0u;
    bool linear = (filter & CHORD_MATSLOT_MAG_LINEAR) != 0u;
    if (lodq > 0) {
        linear = (filter & CHORD_MATSLOT_MIN_LINEAR) != 0u;
        if (filter & CHORD_MATSLOT_MIP_NEAREST) l0 = l1 = min((uint32_t)(lodq + 128) >> 8, last);
        else if (filter & CHORD_MATSLOT_MIP_LINEAR) { l0 = min((uint32_t)lodq >> 8, last); l1 = min(l0 + 1u, last); }
    }
    const DMatLevel L0 = S.levels[l0];
    float4 c = sample_level<kSrgb, kBlocks>(texels, L0, S.wrapS, S.wrapT, linear, u, v, srgb);
    if (l1 != l0) {                                       // (c0 + (c0 - c0) * f is c0: the second level is skipped when it is the first)
        const DMatLevel L1 = S.levels[l1];
        const float4 c1 = sample_level<kSrgb, kBlocks>(texels, L1, S.wrapS, S.wrapT, linear, u, v, srgb);
        const float f = (float)(lodq & 255) * (1.0f / 256.0f);
        c = make_float4(c.x + (c1.x - c.x) * f, c.y + (c1.y - c.y) * f, c.z + (c1.z - c.z) * f, c.w + (c1.w - c.w) * f);
    }
    return c;
}

} // namespace chord
