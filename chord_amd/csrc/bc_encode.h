// The pinned encode of block-compressed textures: what chordvis_set_texture_compress makes of RGBA8 texels at
// upload (kernels_texture.hip: a lane encodes a whole block).  The definition is the reference importer's (stb_dxt at HIGHQUAL: the
// PCA endpoints, the projection match and two least-squares refinement rounds for colour; max / min endpoints and the
// three-compare index for channels), restated: integers throughout, and where it computes in floating point every multiply, add
// and divide is rounded on its own, left to right, nothing fused (__fmul_rn, __fadd_rn, __fdiv_rn).  The blocks have the layout
// bc_decode.h reads.
//
// px[16]: the block's texels as RGBA8 words (R in the low byte), texel 4 * row + column.  Every loop over them is fully unrolled
// with compile-time indices: nothing here needs scratch.  tab: the four tables of device_layer.h (CHORD_TEXENC_*), in LDS.
#pragma once

#include "device_layer.h"

namespace chord {

// A channel unit from bits shift .. shift + 7 of the texels: a0 = the maximum, a1 = the minimum (the eight-value mode; six
// values where they are equal), the index of each texel by three compares on its seven-fold distance from the minimum
__device__ __forceinline__ uint2 bc_encode_channel(const uint32_t px[16], uint32_t shift)
{
    int mx = (int)((px[0] >> shift) & 0xFFu), mn = mx;
#pragma unroll
    for (int i = 1; i < 16; i++) {
        const int v = (int)((px[i] >> shift) & 0xFFu);
        mx = max(mx, v); mn = min(mn, v);
    }
    const int dist = mx - mn, dist4 = dist * 4, dist2 = dist * 2;
    const int bias = (dist < 8 ? dist - 1 : dist / 2 + 2) - 7 * mn;
    uint32_t lo = 0u, hi = 0u;                              // index bits 0..23 and 24..47
#pragma unroll
    for (int i = 0; i < 16; i++) {
        int a = (int)((px[i] >> shift) & 0xFFu) * 7 + bias, ind = 0;
        if (a >= dist4) { ind = 4; a -= dist4; }
        if (a >= dist2) { ind += 2; a -= dist2; }
        ind += a >= dist ? 1 : 0;
        ind = -ind & 7;                                     // linear scale 0 (minimum) .. 7 (maximum) -> the block's index
        ind ^= 2 > ind ? 1 : 0;
        if (i < 8) lo |= (uint32_t)ind << (3 * i); else hi |= (uint32_t)ind << (3 * (i - 8));
    }
    return make_uint2((uint32_t)mx | (uint32_t)mn << 8 | (lo & 0xFFFFu) << 16, lo >> 16 | hi << 8);
}

__device__ __forceinline__ int bc_mul8bit(int a, int b) { const int t = a * b + 128; return (t + (t >> 8)) >> 8; }
// RGBA8 word -> 5:6:5
__device__ __forceinline__ uint32_t bc_as16bit(uint32_t p)
{
    return (uint32_t)((bc_mul8bit((int)(p & 0xFFu), 31) << 11) + (bc_mul8bit((int)((p >> 8) & 0xFFu), 63) << 5) + bc_mul8bit((int)((p >> 16) & 0xFFu), 31));
}
// the optimal single-colour endpoints of (r, g, b): max16 in the low half, min16 in the high half
__device__ __forceinline__ uint32_t bc_single_colour(const uint32_t* tab, uint32_t r, uint32_t g, uint32_t b)
{
    const uint32_t pr = (tab[CHORD_TEXENC_OMATCH5 + (r >> 1)] >> (16u * (r & 1u))) & 0xFFFFu;
    const uint32_t pg = (tab[CHORD_TEXENC_OMATCH6 + (g >> 1)] >> (16u * (g & 1u))) & 0xFFFFu;
    const uint32_t pb = (tab[CHORD_TEXENC_OMATCH5 + (b >> 1)] >> (16u * (b & 1u))) & 0xFFFFu;
    const uint32_t max16 = (pr & 0xFFu) << 11 | (pg & 0xFFu) << 5 | (pb & 0xFFu), min16 = (pr >> 8) << 11 | (pg >> 8) << 5 | (pb >> 8);
    return max16 | min16 << 16;
}

// The projection match: the palette of (max16, min16) -- the endpoints expanded by (33 c) >> 2 and (65 c) >> 4, the 1/3 points by
// (2 a + b) / 3 --, every texel projected onto the line through the endpoints and sorted by three cut points
__device__ __forceinline__ uint32_t bc_match_colours(const uint32_t px[16], uint32_t max16, uint32_t min16)
{
    const int r0 = (int)(((max16 >> 11) * 33u) >> 2), g0 = (int)((((max16 >> 5) & 63u) * 65u) >> 4), b0 = (int)(((max16 & 31u) * 33u) >> 2);
    const int r1 = (int)(((min16 >> 11) * 33u) >> 2), g1 = (int)((((min16 >> 5) & 63u) * 65u) >> 4), b1 = (int)(((min16 & 31u) * 33u) >> 2);
    const int r2 = (2 * r0 + r1) / 3, g2 = (2 * g0 + g1) / 3, b2 = (2 * b0 + b1) / 3;
    const int r3 = (2 * r1 + r0) / 3, g3 = (2 * g1 + g0) / 3, b3 = (2 * b1 + b0) / 3;
    const int dr = r0 - r1, dg = g0 - g1, db = b0 - b1;
    const int s0 = r0 * dr + g0 * dg + b0 * db, s1 = r1 * dr + g1 * dg + b1 * db, s2 = r2 * dr + g2 * dg + b2 * db, s3 = r3 * dr + g3 * dg + b3 * db;
    const int c0Point = s1 + s3, halfPoint = s3 + s2, c3Point = s2 + s0;
    uint32_t mask = 0u;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int dot = 2 * ((int)(px[i] & 0xFFu) * dr + (int)((px[i] >> 8) & 0xFFu) * dg + (int)((px[i] >> 16) & 0xFFu) * db);
        const uint32_t idx = dot < halfPoint ? (dot < c0Point ? 1u : 3u) : (dot < c3Point ? 2u : 0u);
        mask |= idx << (2 * i);
    }
    return mask;
}

__device__ __forceinline__ uint32_t bc_quantize(float x, float scale, const uint32_t* mid)
{
    x = x < 0.0f ? 0.0f : x > 1.0f ? 1.0f : x;
    const uint32_t q = (uint32_t)__fmul_rn(x, scale);
    return q + (x > __uint_as_float(mid[q]) ? 1u : 0u);
}

// A colour unit.  opaque: BC3 -- the constancy test sees the alpha as 255 throughout; BC1_RGB compares the whole words, so a
// block of one colour under varying alpha takes the general path
__device__ __forceinline__ uint2 bc_encode_colour(const uint32_t px[16], bool opaque, const uint32_t* tab)
{
    const uint32_t seen = opaque ? 0x00FFFFFFu : 0xFFFFFFFFu;
    uint32_t differ = 0u;
    int sr = 0, sg = 0, sb = 0, loR = 255, loG = 255, loB = 255, hiR = 0, hiG = 0, hiB = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int r = (int)(px[i] & 0xFFu), g = (int)((px[i] >> 8) & 0xFFu), b = (int)((px[i] >> 16) & 0xFFu);
        differ |= (px[i] ^ px[0]) & seen;
        sr += r; sg += g; sb += b;
        loR = min(loR, r); loG = min(loG, g); loB = min(loB, b);
        hiR = max(hiR, r); hiG = max(hiG, g); hiB = max(hiB, b);
    }
    uint32_t max16, min16, mask;
    if (!differ) {
        const uint32_t e = bc_single_colour(tab, px[0] & 0xFFu, (px[0] >> 8) & 0xFFu, (px[0] >> 16) & 0xFFu);
        max16 = e & 0xFFFFu; min16 = e >> 16; mask = 0xAAAAAAAAu;
    } else {
        // the principal axis: covariance about the rounded mean, four power iterations from the extent of the bounding box
        const int muR = (sr + 8) >> 4, muG = (sg + 8) >> 4, muB = (sb + 8) >> 4;         // (also the average of the singular branch)
        int cov0 = 0, cov1 = 0, cov2 = 0, cov3 = 0, cov4 = 0, cov5 = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int r = (int)(px[i] & 0xFFu) - muR, g = (int)((px[i] >> 8) & 0xFFu) - muG, b = (int)((px[i] >> 16) & 0xFFu) - muB;
            cov0 += r * r; cov1 += r * g; cov2 += r * b; cov3 += g * g; cov4 += g * b; cov5 += b * b;
        }
        const float f0 = __fdiv_rn((float)cov0, 255.0f), f1 = __fdiv_rn((float)cov1, 255.0f), f2 = __fdiv_rn((float)cov2, 255.0f);
        const float f3 = __fdiv_rn((float)cov3, 255.0f), f4 = __fdiv_rn((float)cov4, 255.0f), f5 = __fdiv_rn((float)cov5, 255.0f);
        float vr = (float)(hiR - loR), vg = (float)(hiG - loG), vb = (float)(hiB - loB);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float r = __fadd_rn(__fadd_rn(__fmul_rn(vr, f0), __fmul_rn(vg, f1)), __fmul_rn(vb, f2));
            const float g = __fadd_rn(__fadd_rn(__fmul_rn(vr, f1), __fmul_rn(vg, f3)), __fmul_rn(vb, f4));
            const float b = __fadd_rn(__fadd_rn(__fmul_rn(vr, f2), __fmul_rn(vg, f4)), __fmul_rn(vb, f5));
            vr = r; vg = g; vb = b;
        }
        const double magn = fmax(fmax(fabs((double)vr), fabs((double)vg)), fabs((double)vb));
        int ar = 299, ag = 587, ab = 114;                   // too short an axis: luminance
        if (!(magn < 4.0)) {
            const double s = 512.0 / magn;
            ar = (int)((double)vr * s); ag = (int)((double)vg * s); ab = (int)((double)vb * s);
        }
        // the extreme texels along the axis (the first of equals)
        uint32_t pmin = px[0], pmax = px[0];
        int mind = (int)(px[0] & 0xFFu) * ar + (int)((px[0] >> 8) & 0xFFu) * ag + (int)((px[0] >> 16) & 0xFFu) * ab, maxd = mind;
#pragma unroll
        for (int i = 1; i < 16; i++) {
            const int dot = (int)(px[i] & 0xFFu) * ar + (int)((px[i] >> 8) & 0xFFu) * ag + (int)((px[i] >> 16) & 0xFFu) * ab;
            if (dot < mind) { mind = dot; pmin = px[i]; }
            if (dot > maxd) { maxd = dot; pmax = px[i]; }
        }
        max16 = bc_as16bit(pmax); min16 = bc_as16bit(pmin);
        mask = max16 != min16 ? bc_match_colours(px, max16, min16) : 0u;

        // two refinement rounds: the endpoints that fit the texels best under the indices they have (least squares by Cramer's
        // rule), then the match again; ends early where nothing moves.  Diverges per lane
        for (int round = 0; round < 2; round++) {
            const uint32_t last = mask;
            uint32_t nmax, nmin;
            if ((mask ^ (mask << 2)) < 4u) {                // one index in all 16 texels: the system is singular
                const uint32_t e = bc_single_colour(tab, (uint32_t)muR, (uint32_t)muG, (uint32_t)muB);
                nmax = e & 0xFFFFu; nmin = e >> 16;
            } else {
                int a1r = 0, a1g = 0, a1b = 0, xx = 0, yy = 0, xy = 0;
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const int w1 = (int)((0x1203u >> (4u * ((mask >> (2 * i)) & 3u))) & 3u), w2 = 3 - w1;    // index 0, 1, 2, 3: weight 3, 0, 2, 1 of the first endpoint
                    xx += w1 * w1; yy += w2 * w2; xy += w1 * w2;
                    a1r += w1 * (int)(px[i] & 0xFFu); a1g += w1 * (int)((px[i] >> 8) & 0xFFu); a1b += w1 * (int)((px[i] >> 16) & 0xFFu);
                }
                const int a2r = 3 * sr - a1r, a2g = 3 * sg - a1g, a2b = 3 * sb - a1b;
                const float f = __fdiv_rn(__fdiv_rn(3.0f, 255.0f), (float)(xx * yy - xy * xy));
                nmax = bc_quantize(__fmul_rn((float)(a1r * yy - a2r * xy), f), 31.0f, tab + CHORD_TEXENC_MID5) << 11 |
                       bc_quantize(__fmul_rn((float)(a1g * yy - a2g * xy), f), 63.0f, tab + CHORD_TEXENC_MID6) << 5 |
                       bc_quantize(__fmul_rn((float)(a1b * yy - a2b * xy), f), 31.0f, tab + CHORD_TEXENC_MID5);
                nmin = bc_quantize(__fmul_rn((float)(a2r * xx - a1r * xy), f), 31.0f, tab + CHORD_TEXENC_MID5) << 11 |
                       bc_quantize(__fmul_rn((float)(a2g * xx - a1g * xy), f), 63.0f, tab + CHORD_TEXENC_MID6) << 5 |
                       bc_quantize(__fmul_rn((float)(a2b * xx - a1b * xy), f), 31.0f, tab + CHORD_TEXENC_MID5);
            }
            const bool moved = nmax != max16 || nmin != min16;
            max16 = nmax; min16 = nmin;
            if (moved) {
                if (max16 == min16) { mask = 0u; break; }
                mask = bc_match_colours(px, max16, min16);
            }
            if (mask == last) break;
        }
    }
    if (max16 < min16) { const uint32_t t = min16; min16 = max16; max16 = t; mask ^= 0x55555555u; }
    return make_uint2(max16 | min16 << 16, mask);
}

} // namespace chord
