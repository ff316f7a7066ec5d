// Block-compressed textures (CHORD_TEXFMT_BC1_RGB / BC3 / BC4 / BC5: what the reference's material import stores,
// asset_gltf_material.cpp:80-110, written by stb_dxt through asset_texture_helper.cpp's mipmapCompressBC1/3/4/5) expanded at upload
// into the texel stores the library already has: RGBA8 words of dMatTexels (chordvis_upload_material_textures) or the alpha bytes of
// dTexAlpha (chordvis_upload_scene).  The decode is the pinned one of DESIGN.md 2 item 9(h): integers only, floor divisions.
//
// One launch per upload.  The grid is flat over the blocks of every level of every compressed texture of the upload; a lane owns
// one block: it reads the block once (8 or 16 bytes; consecutive lanes read consecutive blocks) and writes its four texel rows, so
// that the lanes of a wave write consecutive 16-byte pieces (RGBA8) or 4-byte pieces (alpha) of one texel row per store
// instruction.  Texels of an edge block outside the level are never written.
#include "device_layer.h"

namespace chord {

namespace {

// value k of an alpha / single-channel block with the endpoints a0, a1
__device__ __forceinline__ uint32_t channel_value(uint32_t a0, uint32_t a1, uint32_t k)
{
    if (k < 2u) return k ? a1 : a0;
    if (a0 > a1) return ((8u - k) * a0 + (k - 1u) * a1) / 7u;
    if (k < 6u) return ((6u - k) * a0 + (k - 1u) * a1) / 5u;
    return k == 6u ? 0u : 255u;
}

// the 16 values of a channel block, shifted to bit `shift` of out[i] (OR-ed in)
__device__ __forceinline__ void channel_block(uint2 q, uint32_t shift, uint32_t out[16])
{
    const uint32_t a0 = q.x & 0xFFu, a1 = (q.x >> 8) & 0xFFu;
    const unsigned long long bits = ((unsigned long long)q.y << 16) | (q.x >> 16);     // the 48 index bits, least significant first
#pragma unroll
    for (uint32_t i = 0; i < 16u; i++) out[i] |= channel_value(a0, a1, (uint32_t)(bits >> (3u * i)) & 7u) << shift;
}

// the 16 colours of a colour block as R | G << 8 | B << 16 (OR-ed in).  fourColour: BC3 (always), BC1 when c0 > c1
__device__ __forceinline__ void colour_block(uint2 q, bool alwaysFour, uint32_t out[16])
{
    const uint32_t c0 = q.x & 0xFFFFu, c1 = q.x >> 16;
    const uint32_t r0 = c0 >> 11, g0 = (c0 >> 5) & 63u, b0 = c0 & 31u, r1 = c1 >> 11, g1 = (c1 >> 5) & 63u, b1 = c1 & 31u;
    const uint32_t R0 = (r0 << 3) | (r0 >> 2), G0 = (g0 << 2) | (g0 >> 4), B0 = (b0 << 3) | (b0 >> 2);
    const uint32_t R1 = (r1 << 3) | (r1 >> 2), G1 = (g1 << 2) | (g1 >> 4), B1 = (b1 << 3) | (b1 >> 2);
    const uint32_t p0 = R0 | G0 << 8 | B0 << 16, p1 = R1 | G1 << 8 | B1 << 16;
    uint32_t p2, p3;
    if (alwaysFour || c0 > c1) {
        p2 = (2u * R0 + R1) / 3u | ((2u * G0 + G1) / 3u) << 8 | ((2u * B0 + B1) / 3u) << 16;
        p3 = (R0 + 2u * R1) / 3u | ((G0 + 2u * G1) / 3u) << 8 | ((B0 + 2u * B1) / 3u) << 16;
    } else {
        p2 = (R0 + R1) / 2u | ((G0 + G1) / 2u) << 8 | ((B0 + B1) / 2u) << 16;
        p3 = 0u;
    }
#pragma unroll
    for (uint32_t i = 0; i < 16u; i++) {
        const uint32_t k = (q.y >> (2u * i)) & 3u;
        out[i] |= (k & 2u) ? ((k & 1u) ? p3 : p2) : ((k & 1u) ? p1 : p0);
    }
}

template <bool ALPHA>
__global__ __launch_bounds__(256) void texture_decode_kernel(const DTexLevelRec* __restrict__ recs, uint32_t count, uint32_t totalBlocks,
                                                             const uint2* __restrict__ staging, uint32_t* __restrict__ texels,
                                                             uint8_t* __restrict__ alpha)
{
    // the record of the workgroup's first block: the last one whose firstBlock is not above it (recs[0].firstBlock = 0,
    // recs[count].firstBlock = totalBlocks); uniform, so the table is read with scalar loads
    const uint32_t first = blockIdx.x * 256u;
    uint32_t lo = 0u, hi = count;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (recs[mid].firstBlock <= first) lo = mid; else hi = mid;
    }
    const uint32_t b = first + threadIdx.x;
    if (b >= totalBlocks) return;
    while (recs[lo + 1u].firstBlock <= b) lo++;             // (ends: the closing record's firstBlock is above every block)
    const DTexLevelRec R = recs[lo];

    const uint32_t lb = b - R.firstBlock, by = lb / R.blocksPerRow, bx = lb - by * R.blocksPerRow;
    const bool two = R.format == CHORD_TEXFMT_BC3 || R.format == CHORD_TEXFMT_BC5;      // 16-byte blocks
    const uint2* p = staging + (size_t)R.src + (size_t)lb * (two ? 2u : 1u);
    const uint2 q0 = p[0];
    uint32_t out[16];
    if (ALPHA) {                                            // (BC3 levels only: the alpha block is the first of the two)
#pragma unroll
        for (int i = 0; i < 16; i++) out[i] = 0u;
        channel_block(q0, 0u, out);
    } else {
        uint2 q1 = make_uint2(0u, 0u);
        if (two) q1 = p[1];
#pragma unroll
        for (int i = 0; i < 16; i++) out[i] = 0xFF000000u;
        if (R.format == CHORD_TEXFMT_BC1_RGB) colour_block(q0, false, out);
        else if (R.format == CHORD_TEXFMT_BC3) {
#pragma unroll
            for (int i = 0; i < 16; i++) out[i] = 0u;
            channel_block(q0, 24u, out);
            colour_block(q1, true, out);
        } else {
            channel_block(q0, 0u, out);                     // BC4: (v, 0, 0, 255)
            if (R.format == CHORD_TEXFMT_BC5) channel_block(q1, 8u, out);               // BC5: (r, g, 0, 255)
        }
    }

    const uint32_t x0 = bx * 4u, n = min(4u, R.width - x0);
#pragma unroll
    for (uint32_t r = 0; r < 4u; r++) {
        const uint32_t y = by * 4u + r;
        if (y >= R.height) break;
        const size_t t = (size_t)R.dst + (size_t)y * R.width + x0;                     // texel index = alpha byte index
        if (ALPHA) {
            // four bytes at once where the row piece is whole and 4-byte aligned (not behind a level of odd size)
            if (n == 4u && (t & 3u) == 0u) *reinterpret_cast<uint32_t*>(alpha + t) = out[4 * r] | out[4 * r + 1] << 8 | out[4 * r + 2] << 16 | out[4 * r + 3] << 24;
            else {
#pragma unroll
                for (uint32_t x = 0; x < 4u; x++) if (x < n) alpha[t + x] = (uint8_t)out[4 * r + x];
            }
        } else {
            // 16 bytes at once where the row piece is whole and 16-byte aligned (not behind a 2 x 2 or 1 x 1 level, not when
            // width % 4 != 0)
            if (n == 4u && (t & 3u) == 0u) *reinterpret_cast<uint4*>(texels + t) = make_uint4(out[4 * r], out[4 * r + 1], out[4 * r + 2], out[4 * r + 3]);
            else {
#pragma unroll
                for (uint32_t x = 0; x < 4u; x++) if (x < n) texels[t + x] = out[4 * r + x];
            }
        }
    }
}

} // namespace

void launch_texture_decode(ChordCtx* c, const DTexLevelRec* recs, uint32_t count, uint32_t totalBlocks, const void* staging,
                           uint32_t* texels, uint8_t* alpha, bool alphaOnly)
{
    if (!count || !totalBlocks) return;
    const dim3 grid((totalBlocks + 255u) / 256u), block(256);
    if (alphaOnly) CHORD_LAUNCH(c, texture_decode_kernel<true>, grid, block, 0, c->stream, recs, count, totalBlocks, (const uint2*)staging, texels, alpha);
    else CHORD_LAUNCH(c, texture_decode_kernel<false>, grid, block, 0, c->stream, recs, count, totalBlocks, (const uint2*)staging, texels, alpha);
}

} // namespace chord
