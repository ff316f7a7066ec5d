// Block-compressed textures (CHORD_TEXFMT_BC1_RGB / BC3 / BC4 / BC5: what the reference's material import stores,
// asset_gltf_material.cpp:80-110, written by stb_dxt through asset_texture_helper.cpp's mipmapCompressBC1/3/4/5) expanded at upload
// into the texel stores the library already has: RGBA8 words of dMatTexels (chordvis_upload_material_textures) or the alpha bytes of
// dTexAlpha (chordvis_upload_scene).  The decode is the pinned one of DESIGN.md 2 item 9(h), defined in bc_decode.h.
//
// One launch per upload.  The grid is flat over the blocks of every level of every compressed texture of the upload; a lane owns
// one block: it reads the block once (8 or 16 bytes; consecutive lanes read consecutive blocks) and writes its four texel rows, so
// that the lanes of a wave write consecutive 16-byte pieces (RGBA8) or 4-byte pieces (alpha) of one texel row per store
// instruction.  Texels of an edge block outside the level are never written.
#include "device_layer.h"
#include "bc_decode.h"
#include "bc_encode.h"

namespace chord {

namespace {

// the 16 values of a channel block, shifted to bit `shift` of out[i] (OR-ed in)
__device__ __forceinline__ void channel_block(uint2 q, uint32_t shift, uint32_t out[16])
{
    const uint32_t a0 = q.x & 0xFFu, a1 = (q.x >> 8) & 0xFFu;
    const unsigned long long bits = bc_channel_bits(q);
#pragma unroll
    for (uint32_t i = 0; i < 16u; i++) out[i] |= bc_channel_value(a0, a1, (uint32_t)(bits >> (3u * i)) & 7u) << shift;
}

// the 16 colours of a colour block as R | G << 8 | B << 16 (OR-ed in).  alwaysFour: BC3
__device__ __forceinline__ void colour_block(uint2 q, bool alwaysFour, uint32_t out[16])
{
    uint32_t p0, p1, p2, p3;
    bc_colour_palette(q.x, alwaysFour, p0, p1, p2, p3);
#pragma unroll
    for (uint32_t i = 0; i < 16u; i++) out[i] |= bc_palette_pick((q.y >> (2u * i)) & 3u, p0, p1, p2, p3);
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

// ---- mip generation (chordvis_set_texture_mips) ----
// Level l+1 is a 2 x 2 box of level l, in place in the texel store (RGBA8 words of dMatTexels, or ALPHA: bytes of dTexAlpha).
// Levels whose source is larger than 64 x 64 take one launch per level step, shared by every texture of the upload
// (texture_mips_step_kernel); from a source of at most 64 x 64 on, one workgroup finishes a texture's chain through LDS
// (texture_mips_tail_kernel).  CHORD_TEXMIPS_COVERAGE then rescales the alpha of the made levels (the three coverage kernels).

// (sum of four codes + 2) >> 2 in each byte of the word: two 16-bit fields per half, no carry between them (4 x 255 + 2 < 2^16)
__device__ __forceinline__ uint32_t box_codes(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const uint32_t M = 0x00FF00FFu, R = 0x00020002u;
    const uint32_t lo = (((a & M) + (b & M) + (c & M) + (d & M) + R) >> 2) & M;
    const uint32_t hi = ((((a >> 8) & M) + ((b >> 8) & M) + ((c >> 8) & M) + ((d >> 8) & M) + R) >> 2) & M;
    return lo | hi << 8;
}

// tab: the sRGB8 -> linear table T[256], then mid[256] with mid[k] = (T[k-1] + T[k]) * 0.5f.  The number of k in 1..255 with
// mid[k] <= v (mid is strictly increasing): the nearest code in linear light
__device__ __forceinline__ uint32_t linear_code(const float* tab, float v)
{
    uint32_t lo = 0u, hi = 255u;                            // mid[k] <= v for k in 1..lo, mid[k] > v for k > hi
    while (lo < hi) {
        const uint32_t m = (lo + hi + 1u) >> 1;
        if (tab[256u + m] <= v) lo = m; else hi = m - 1u;
    }
    return lo;
}

// a = (2x, 2y), b = (2x+1, 2y), c = (2x, 2y+1), d = (2x+1, 2y+1)
__device__ __forceinline__ uint32_t box_texel(bool srgb, const float* tab, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const uint32_t codes = box_codes(a, b, c, d);
    if (!srgb) return codes;
    uint32_t out = codes & 0xFF000000u;
#pragma unroll
    for (uint32_t s = 0; s < 24u; s += 8u) {
        const float v = __fmul_rn(__fadd_rn(__fadd_rn(tab[(a >> s) & 0xFFu], tab[(b >> s) & 0xFFu]),
                                            __fadd_rn(tab[(c >> s) & 0xFFu], tab[(d >> s) & 0xFFu])), 0.25f);
        out |= linear_code(tab, v) << s;
    }
    return out;
}

// the last record whose first word is not above g (recs[0]'s is 0, the closing record's is above every g); FIELD: word of the record
template <typename Rec, uint32_t Rec::*FIELD>
__device__ __forceinline__ uint32_t find_record(const Rec* __restrict__ recs, uint32_t count, uint32_t g)
{
    uint32_t lo = 0u, hi = count;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (recs[mid].*FIELD <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// One level step of every texture that has one: the grid is flat over units of four adjacent output texels of a row; a lane
// reads 2 x 8 source texels (two 16-byte loads per row; ALPHA: one 8-byte load) and writes 16 bytes (ALPHA: 4), where the
// pieces are whole and aligned -- they are not behind a level of odd size, nor at the end of a row whose width is no multiple of 4.
template <bool ALPHA>
__global__ __launch_bounds__(256) void texture_mips_step_kernel(const DTexMipRec* __restrict__ recs, uint32_t count, uint32_t totalUnits,
                                                                const float* __restrict__ tables, uint32_t* __restrict__ texels,
                                                                uint8_t* __restrict__ alpha)
{
    __shared__ float tab[512];
    if (!ALPHA && tables) {                                 // (null: no record of the upload has CHORD_TEXMIPS_SRGB)
        tab[threadIdx.x] = tables[threadIdx.x]; tab[threadIdx.x + 256u] = tables[threadIdx.x + 256u];
        __syncthreads();
    }
    const uint32_t first = blockIdx.x * 256u;
    uint32_t lo = find_record<DTexMipRec, &DTexMipRec::firstUnit>(recs, count, first);
    const uint32_t u = first + threadIdx.x;
    if (u >= totalUnits) return;
    while (recs[lo + 1u].firstUnit <= u) lo++;
    const DTexMipRec R = recs[lo];

    const uint32_t lu = u - R.firstUnit, y = lu / R.unitsPerRow, x0 = (lu - y * R.unitsPerRow) * 4u;
    const uint32_t dw = max(1u, R.sw >> 1), n = min(4u, dw - x0);
    const size_t s0 = (size_t)R.src + (size_t)min(2u * y, R.sh - 1u) * R.sw, s1 = (size_t)R.src + (size_t)min(2u * y + 1u, R.sh - 1u) * R.sw;
    uint32_t p0[8], p1[8];
    // (n == 4 means dw >= x0 + 4, so the eight source columns 2 x0 .. 2 x0 + 7 exist: sw >= 2 dw)
    const size_t c0 = s0 + 2u * x0, c1 = s1 + 2u * x0;
    if (ALPHA) {
        if (n == 4u && ((c0 | c1) & 7u) == 0u) {
            const uint2 q0 = *reinterpret_cast<const uint2*>(alpha + c0), q1 = *reinterpret_cast<const uint2*>(alpha + c1);
#pragma unroll
            for (uint32_t i = 0; i < 4u; i++) {
                p0[i] = (q0.x >> (8u * i)) & 0xFFu; p0[4u + i] = (q0.y >> (8u * i)) & 0xFFu;
                p1[i] = (q1.x >> (8u * i)) & 0xFFu; p1[4u + i] = (q1.y >> (8u * i)) & 0xFFu;
            }
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 8u; i++) {
                const uint32_t col = min(2u * x0 + i, R.sw - 1u);               // (the clamp acts only where sw == 1)
                p0[i] = alpha[s0 + col]; p1[i] = alpha[s1 + col];
            }
        }
    } else {
        if (n == 4u && ((c0 | c1) & 3u) == 0u) {
            const uint4 a0 = *reinterpret_cast<const uint4*>(texels + c0), a1 = *reinterpret_cast<const uint4*>(texels + c0 + 4u);
            const uint4 b0 = *reinterpret_cast<const uint4*>(texels + c1), b1 = *reinterpret_cast<const uint4*>(texels + c1 + 4u);
            p0[0] = a0.x; p0[1] = a0.y; p0[2] = a0.z; p0[3] = a0.w; p0[4] = a1.x; p0[5] = a1.y; p0[6] = a1.z; p0[7] = a1.w;
            p1[0] = b0.x; p1[1] = b0.y; p1[2] = b0.z; p1[3] = b0.w; p1[4] = b1.x; p1[5] = b1.y; p1[6] = b1.z; p1[7] = b1.w;
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 8u; i++) {
                const uint32_t col = min(2u * x0 + i, R.sw - 1u);
                p0[i] = texels[s0 + col]; p1[i] = texels[s1 + col];
            }
        }
    }
    const bool srgb = !ALPHA && (R.flags & CHORD_TEXMIPS_SRGB);
    uint32_t out[4];
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) out[j] = box_texel(srgb, tab, p0[2 * j], p0[2 * j + 1], p1[2 * j], p1[2 * j + 1]);

    const size_t t = (size_t)R.dst + (size_t)y * dw + x0;
    if (ALPHA) {
        if (n == 4u && (t & 3u) == 0u) *reinterpret_cast<uint32_t*>(alpha + t) = out[0] | out[1] << 8 | out[2] << 16 | out[3] << 24;
        else {
#pragma unroll
            for (uint32_t x = 0; x < 4u; x++) if (x < n) alpha[t + x] = (uint8_t)out[x];
        }
    } else {
        if (n == 4u && (t & 3u) == 0u) *reinterpret_cast<uint4*>(texels + t) = make_uint4(out[0], out[1], out[2], out[3]);
        else {
#pragma unroll
            for (uint32_t x = 0; x < 4u; x++) if (x < n) texels[t + x] = out[x];
        }
    }
}

// The rest of a chain from a source level of at most 64 x 64: the workgroup holds the source in LDS, makes a level into a second
// LDS buffer and the store, and goes on from there; the two buffers change roles (a made level has at most 32 x 32 texels).
template <bool ALPHA>
__global__ __launch_bounds__(256) void texture_mips_tail_kernel(const DTexTailRec* __restrict__ recs, const float* __restrict__ tables,
                                                                uint32_t* __restrict__ texels, uint8_t* __restrict__ alpha)
{
    __shared__ uint32_t buf[CHORD_TEXMIPS_TAIL * CHORD_TEXMIPS_TAIL + CHORD_TEXMIPS_TAIL * CHORD_TEXMIPS_TAIL / 4u];
    __shared__ float tab[512];
    const DTexTailRec R = recs[blockIdx.x];
    const bool srgb = !ALPHA && (R.flags & CHORD_TEXMIPS_SRGB);                      // (uniform)
    if (srgb) { tab[threadIdx.x] = tables[threadIdx.x]; tab[threadIdx.x + 256u] = tables[threadIdx.x + 256u]; }
    uint32_t sw = R.sw, sh = R.sh;
    size_t off = R.src;
    for (uint32_t i = threadIdx.x; i < sw * sh; i += 256u) buf[i] = ALPHA ? (uint32_t)alpha[off + i] : texels[off + i];
    __syncthreads();
    uint32_t* s = buf;
    uint32_t* d = buf + CHORD_TEXMIPS_TAIL * CHORD_TEXMIPS_TAIL;
    off += sw * sh;
    for (uint32_t l = 0; l < R.levels; l++) {
        const uint32_t dw = max(1u, sw >> 1), dh = max(1u, sh >> 1);
        for (uint32_t i = threadIdx.x; i < dw * dh; i += 256u) {
            const uint32_t y = i / dw, x = i - y * dw;
            const uint32_t x0 = min(2u * x, sw - 1u), x1 = min(2u * x + 1u, sw - 1u), r0 = min(2u * y, sh - 1u) * sw, r1 = min(2u * y + 1u, sh - 1u) * sw;
            const uint32_t v = box_texel(srgb, tab, s[r0 + x0], s[r0 + x1], s[r1 + x0], s[r1 + x1]);
            d[i] = v;
            if (ALPHA) alpha[off + i] = (uint8_t)v; else texels[off + i] = v;
        }
        __syncthreads();
        uint32_t* const k = s; s = d; d = k;
        off += dw * dh; sw = dw; sh = dh;
    }
}

// Coverage, step 1 and 2: the 256-bin histogram of the alpha of a workgroup's 4096 texels in LDS (a lane adds a run of equal
// values at once: masks are mostly 0 and 255), then one global add per non-empty bin into the level's row of `work`.
template <bool ALPHA>
__global__ __launch_bounds__(256) void texture_coverage_hist_kernel(const DTexCovRec* __restrict__ recs, uint32_t count, uint32_t* __restrict__ work,
                                                                    const uint32_t* __restrict__ texels, const uint8_t* __restrict__ alpha)
{
    __shared__ uint32_t hist[256];
    const uint32_t r = find_record<DTexCovRec, &DTexCovRec::firstGroup>(recs, count, blockIdx.x);      // (uniform)
    const DTexCovRec R = recs[r];
    hist[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t begin = (blockIdx.x - R.firstGroup) * CHORD_TEXCOV_GROUP, end = min(begin + CHORD_TEXCOV_GROUP, R.texels);
    uint32_t prev = 0u, run = 0u;
    for (uint32_t i = begin + threadIdx.x; i < end; i += 256u) {
        const uint32_t a = ALPHA ? (uint32_t)alpha[(size_t)R.base + i] : texels[(size_t)R.base + i] >> 24;
        if (a == prev) run++;
        else { if (run) atomicAdd(&hist[prev], run); prev = a; run = 1u; }
    }
    if (run) atomicAdd(&hist[prev], run);
    __syncthreads();
    const uint32_t h = hist[threadIdx.x];
    if (h) atomicAdd(&work[(size_t)r * 256u + threadIdx.x], h);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// Coverage, step 3: one wave per generated level.  cnt(t) = texels with a >= t by a suffix scan of the histogram (a lane holds
// four bins); t* = the largest t in 1..255 with cnt(t) N0 >= P0 N, or 1 (cnt does not grow with t, so the t that satisfy it are
// 1 .. t*: t* is how many there are); tlo = the smallest t with cnt(t) = cnt(t*); t' = clamp(cutoff, tlo, t*) goes to
// work[count * 256 + level].
__global__ __launch_bounds__(64) void texture_coverage_pick_kernel(const DTexCovRec* __restrict__ recs, uint32_t count, uint32_t* __restrict__ work)
{
    __shared__ uint32_t cnt[256];
    const uint32_t r = blockIdx.x, lane = threadIdx.x;
    const DTexCovRec R = recs[r];
    if (R.level0 == r) return;                              // (level 0 as supplied: counted, never rescaled)
    const uint4 b = *reinterpret_cast<const uint4*>(work + (size_t)r * 256u + 4u * lane);
    const uint4 z = *reinterpret_cast<const uint4*>(work + (size_t)R.level0 * 256u + 4u * lane);
    const uint32_t sum = b.x + b.y + b.z + b.w;
    uint32_t incl = sum;                                    // bins of this lane and of the lanes above
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t v = __shfl_down(incl, d);
        if (lane + d < 64u) incl += v;
    }
    const uint32_t c3 = incl - sum + b.w, c2 = c3 + b.z, c1 = c2 + b.y, c0 = c1 + b.x;
    cnt[4u * lane] = c0; cnt[4u * lane + 1u] = c1; cnt[4u * lane + 2u] = c2; cnt[4u * lane + 3u] = c3;
    const uint32_t t0 = 4u * lane;
    const unsigned long long P0 = wave_sum((t0 >= R.cutoff ? z.x : 0u) + (t0 + 1u >= R.cutoff ? z.y : 0u) + (t0 + 2u >= R.cutoff ? z.z : 0u) + (t0 + 3u >= R.cutoff ? z.w : 0u));
    const unsigned long long N0 = recs[R.level0].texels, N = R.texels;
    __syncthreads();
    uint32_t k = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) k += (t0 + j >= 1u && (unsigned long long)cnt[t0 + j] * N0 >= P0 * N) ? 1u : 0u;
    const uint32_t tStar = max(1u, wave_sum(k));
    const uint32_t cStar = cnt[tStar];
    uint32_t m = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) m += (t0 + j >= 1u && cnt[t0 + j] > cStar) ? 1u : 0u;
    const uint32_t tLo = 1u + wave_sum(m);
    if (lane == 0u) work[(size_t)count * 256u + r] = min(max(R.cutoff, tLo), tStar);
}

// Coverage, step 4: a' = min(255, a * cutoff / t') over the generated levels, through a 256-entry table in LDS.
template <bool ALPHA>
__global__ __launch_bounds__(256) void texture_coverage_rescale_kernel(const DTexCovRec* __restrict__ recs, uint32_t count, const uint32_t* __restrict__ work,
                                                                       uint32_t* __restrict__ texels, uint8_t* __restrict__ alpha)
{
    __shared__ uint32_t lut[256];
    const uint32_t r = find_record<DTexCovRec, &DTexCovRec::firstScaleGroup>(recs, count, blockIdx.x);  // (uniform)
    const DTexCovRec R = recs[r];
    const uint32_t tp = work[(size_t)count * 256u + r];
    if (tp == R.cutoff) return;                             // a' = a
    lut[threadIdx.x] = min(255u, threadIdx.x * R.cutoff / tp);
    __syncthreads();
    const uint32_t begin = (blockIdx.x - R.firstScaleGroup) * CHORD_TEXCOV_GROUP, end = min(begin + CHORD_TEXCOV_GROUP, R.texels);
    for (uint32_t i = begin + threadIdx.x; i < end; i += 256u) {
        const size_t t = (size_t)R.base + i;
        if (ALPHA) alpha[t] = (uint8_t)lut[alpha[t]];
        else { const uint32_t w = texels[t]; texels[t] = (w & 0x00FFFFFFu) | lut[w >> 24] << 24; }
    }
}

// ---- block compression (chordvis_set_texture_compress; the encoder is bc_encode.h's) ----
// One launch per upload, behind the mip generation.  The grid is flat over the output blocks of every level of every texture to
// encode; a lane owns one block: it reads the block's four texel rows (16 bytes at once where the row piece is whole and aligned;
// single words elsewhere and where the fill wraps: texel (x, y) of block (bx, by) is the level's ((4 bx + x) mod w, (4 by + y) mod
// h)), keeps the 16 words in registers, and stores the block with one 8- or 16-byte store, consecutive lanes consecutive blocks.
// The format is a field of the record, not a template argument: a workgroup's first record is uniform, but a lane steps on into
// the records behind it (a chain's small levels hold a handful of blocks each), so one launch mixes formats within a wave.
__global__ __launch_bounds__(256) void texture_encode_kernel(const DTexEncRec* __restrict__ recs, uint32_t count, uint32_t totalBlocks,
                                                             const uint32_t* __restrict__ tables, const uint32_t* __restrict__ texels,
                                                             uint2* __restrict__ blocks)
{
    __shared__ uint32_t tab[CHORD_TEXENC_TABLE_WORDS];
    tab[threadIdx.x] = tables[threadIdx.x];
    if (threadIdx.x + 256u < CHORD_TEXENC_TABLE_WORDS) tab[threadIdx.x + 256u] = tables[threadIdx.x + 256u];
    __syncthreads();
    const uint32_t first = blockIdx.x * 256u;
    uint32_t lo = find_record<DTexEncRec, &DTexEncRec::firstBlock>(recs, count, first);
    const uint32_t b = first + threadIdx.x;
    if (b >= totalBlocks) return;
    while (recs[lo + 1u].firstBlock <= b) lo++;             // (ends: the closing record's firstBlock is above every block)
    const DTexEncRec R = recs[lo];

    const uint32_t lb = b - R.firstBlock, by = lb / R.blocksPerRow, bx = lb - by * R.blocksPerRow;
    const uint32_t x0 = bx * 4u;
    uint32_t px[16];
#pragma unroll
    for (uint32_t r = 0; r < 4u; r++) {
        uint32_t y = by * 4u + r;
        if (y >= R.height) y %= R.height;
        const size_t t = (size_t)R.src + (size_t)y * R.width;
        if (x0 + 4u <= R.width && ((t + x0) & 3u) == 0u) {
            const uint4 q = *reinterpret_cast<const uint4*>(texels + t + x0);
            px[4 * r] = q.x; px[4 * r + 1] = q.y; px[4 * r + 2] = q.z; px[4 * r + 3] = q.w;
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 4u; i++) {
                uint32_t x = x0 + i;
                if (x >= R.width) x %= R.width;
                px[4 * r + i] = texels[t + x];
            }
        }
    }
    if (R.format == CHORD_TEXFMT_BC1_RGB) blocks[(size_t)R.dst + lb] = bc_encode_colour(px, false, tab);
    else if (R.format == CHORD_TEXFMT_BC4) blocks[(size_t)R.dst + lb] = bc_encode_channel(px, 0u);
    else {
        uint2 q0, q1;
        if (R.format == CHORD_TEXFMT_BC3) { q0 = bc_encode_channel(px, 24u); q1 = bc_encode_colour(px, true, tab); }
        else { q0 = bc_encode_channel(px, 0u); q1 = bc_encode_channel(px, 8u); }
        *reinterpret_cast<uint4*>(blocks + (size_t)R.dst + 2u * lb) = make_uint4(q0.x, q0.y, q1.x, q1.y);     // (a chain starts 16-byte aligned and 16-byte blocks keep it so)
    }
}

} // namespace

void launch_texture_encode(ChordCtx* c, const DTexEncRec* recs, uint32_t count, uint32_t totalBlocks, const uint32_t* tables,
                           const uint32_t* texels, void* blocks)
{
    if (!count || !totalBlocks) return;
    CHORD_LAUNCH(c, texture_encode_kernel, dim3((totalBlocks + 255u) / 256u), dim3(256), 0, c->stream, recs, count, totalBlocks, tables, texels, (uint2*)blocks);
}

void launch_texture_decode(ChordCtx* c, const DTexLevelRec* recs, uint32_t count, uint32_t totalBlocks, const void* staging,
                           uint32_t* texels, uint8_t* alpha, bool alphaOnly)
{
    if (!count || !totalBlocks) return;
    const dim3 grid((totalBlocks + 255u) / 256u), block(256);
    if (alphaOnly) CHORD_LAUNCH(c, texture_decode_kernel<true>, grid, block, 0, c->stream, recs, count, totalBlocks, (const uint2*)staging, texels, alpha);
    else CHORD_LAUNCH(c, texture_decode_kernel<false>, grid, block, 0, c->stream, recs, count, totalBlocks, (const uint2*)staging, texels, alpha);
}

void launch_texture_mips_step(ChordCtx* c, const DTexMipRec* recs, uint32_t count, uint32_t totalUnits, const float* tables,
                              uint32_t* texels, uint8_t* alpha, bool alphaOnly)
{
    if (!count || !totalUnits) return;
    const dim3 grid((totalUnits + 255u) / 256u), block(256);
    if (alphaOnly) CHORD_LAUNCH(c, texture_mips_step_kernel<true>, grid, block, 0, c->stream, recs, count, totalUnits, tables, texels, alpha);
    else CHORD_LAUNCH(c, texture_mips_step_kernel<false>, grid, block, 0, c->stream, recs, count, totalUnits, tables, texels, alpha);
}

void launch_texture_mips_tail(ChordCtx* c, const DTexTailRec* recs, uint32_t count, const float* tables, uint32_t* texels,
                              uint8_t* alpha, bool alphaOnly)
{
    if (!count) return;
    const dim3 grid(count), block(256);
    if (alphaOnly) CHORD_LAUNCH(c, texture_mips_tail_kernel<true>, grid, block, 0, c->stream, recs, tables, texels, alpha);
    else CHORD_LAUNCH(c, texture_mips_tail_kernel<false>, grid, block, 0, c->stream, recs, tables, texels, alpha);
}

void launch_texture_coverage(ChordCtx* c, const DTexCovRec* recs, uint32_t count, uint32_t groups, uint32_t scaleGroups,
                             uint32_t* work, uint32_t* texels, uint8_t* alpha, bool alphaOnly)
{
    if (!count || !groups || !scaleGroups) return;
    if (alphaOnly) CHORD_LAUNCH(c, texture_coverage_hist_kernel<true>, dim3(groups), dim3(256), 0, c->stream, recs, count, work, texels, alpha);
    else CHORD_LAUNCH(c, texture_coverage_hist_kernel<false>, dim3(groups), dim3(256), 0, c->stream, recs, count, work, texels, alpha);
    CHORD_LAUNCH(c, texture_coverage_pick_kernel, dim3(count), dim3(64), 0, c->stream, recs, count, work);
    if (alphaOnly) CHORD_LAUNCH(c, texture_coverage_rescale_kernel<true>, dim3(scaleGroups), dim3(256), 0, c->stream, recs, count, work, texels, alpha);
    else CHORD_LAUNCH(c, texture_coverage_rescale_kernel<false>, dim3(scaleGroups), dim3(256), 0, c->stream, recs, count, work, texels, alpha);
}

} // namespace chord
