// Stand-alone run of chord_amd/csrc/material_sampler.h on the host (built and run by tests/test_material_sampler_host.py; no GPU, no
// python in the process).  The header's functions are plain float32 / integer C++ behind __device__, which the host compiler reads as
// nothing, so the statements the kernels execute are the statements this program executes; the two device built-ins the header's
// includes use (__umulhi, min) are supplied here.  It reads one request, samples one texture slot with sample_slot_lod at an explicit
// level per sample, from the texel store or from a chain kept as blocks, and writes the results:
//   request   uint32 words: format (0: RGBA8 texels, else CHORD_TEXFMT_BC*), width, height, mips, minFilter, magFilter, wrapS, wrapT,
//             srgb (0 / 1), samples n; then the chain (texels: one word each; blocks: their bytes, the chain padded to 8 bytes); then n
//             records of three words: u, v (float bits) and lodq (int32)
//   answer    n x 4 float32: the sampled rgba
// The DMatSlot is filled as chordvis_upload_material_textures fills it (filter bits, level bases in texels or 8-byte units, wrap
// constants).  Exit status 2 on a malformed request.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

static inline uint32_t __umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
using std::max;
using std::min;

#include "material_sampler.h"
#include "material_tables.h"

using namespace chord;

static const uint32_t kSrgbBits[256] = {CHORD_SRGB_TABLE_BITS};

static void wrap_consts(uint32_t n, uint32_t mode, uint32_t& magic, uint32_t& bias)
{
    magic = 0u; bias = 0u;
    if (mode == CHORD_WRAP_CLAMP_TO_EDGE) return;
    const uint32_t period = mode == CHORD_WRAP_MIRRORED_REPEAT ? 2u * n : n;
    if ((period & (period - 1u)) == 0u) return;
    magic = (uint32_t)(0x100000000ull / period);
    bias = (uint32_t)(((0x40000000ull + period - 1u) / period) * period);
}

static bool linear_filter(uint32_t f) { return f == CHORD_FILTER_LINEAR || f == CHORD_FILTER_LINEAR_MIPMAP_NEAREST || f == CHORD_FILTER_LINEAR_MIPMAP_LINEAR; }

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<uint32_t> req;
    uint32_t word;
    while (std::fread(&word, 4, 1, in) == 1) req.push_back(word);
    std::fclose(in);
    if (req.size() < 10) return 2;
    const uint32_t format = req[0], width = req[1], height = req[2], mips = req[3], minF = req[4], magF = req[5], wrapS = req[6], wrapT = req[7];
    const bool srgb = req[8] != 0u;
    const uint32_t n = req[9];
    if (mips == 0u || mips > CHORD_MAX_TEX_LEVELS || width == 0u || height == 0u || format > CHORD_TEXFMT_BC5) return 2;

    DMatSlot S;
    std::memset(&S, 0, sizeof(S));
    S.mips = mips; S.wrapS = wrapS; S.wrapT = wrapT; S.format = format;
    S.filter = (linear_filter(magF) ? CHORD_MATSLOT_MAG_LINEAR : 0u) | (linear_filter(minF) ? CHORD_MATSLOT_MIN_LINEAR : 0u) |
               ((minF == CHORD_FILTER_NEAREST_MIPMAP_NEAREST || minF == CHORD_FILTER_LINEAR_MIPMAP_NEAREST) ? CHORD_MATSLOT_MIP_NEAREST : 0u) |
               ((minF == CHORD_FILTER_NEAREST_MIPMAP_LINEAR || minF == CHORD_FILTER_LINEAR_MIPMAP_LINEAR) ? CHORD_MATSLOT_MIP_LINEAR : 0u);
    const uint32_t unitsPerBlock = format == 0u ? 0u : ((format == CHORD_TEXFMT_BC1_RGB || format == CHORD_TEXFMT_BC4) ? 1u : 2u);
    uint64_t off = 0;
    for (uint32_t l = 0; l < mips; l++) {
        const uint32_t w = std::max(1u, width >> l), h = std::max(1u, height >> l);
        DMatLevel& L = S.levels[l];
        L.base = (uint32_t)off; L.dims = (w - 1u) | (h - 1u) << 16;
        wrap_consts(w, wrapS, L.magicS, L.biasS);
        wrap_consts(h, wrapT, L.magicT, L.biasT);
        off += unitsPerBlock ? (uint64_t)((w + 3u) / 4u) * ((h + 3u) / 4u) * unitsPerBlock : (uint64_t)w * h;
    }
    const uint64_t chainWords = unitsPerBlock ? off * 2u : off;
    if (req.size() != 10u + chainWords + 3ull * n) return 2;
    // the chain in memory of its own, exactly as long as it is (the sanitizer sees a read one texel or one block too far); 16-byte aligned
    uint32_t* chain = static_cast<uint32_t*>(std::aligned_alloc(16, (size_t)((chainWords * 4u + 15u) / 16u) * 16u));
    std::memcpy(chain, req.data() + 10, (size_t)chainWords * 4u);
    float table[256];
    for (int i = 0; i < 256; i++) std::memcpy(&table[i], &kSrgbBits[i], 4);

    std::vector<float> out((size_t)n * 4u);
    const uint32_t* smp = req.data() + 10 + chainWords;
    for (uint32_t i = 0; i < n; i++) {
        float u, v;
        int32_t lodq;
        std::memcpy(&u, smp + 3u * i, 4); std::memcpy(&v, smp + 3u * i + 1u, 4); std::memcpy(&lodq, smp + 3u * i + 2u, 4);
        float4 c;
        if (format == 0u) {
            TexelStores<false> T;
            T.texels = chain;
            c = srgb ? sample_slot_lod<true, false>(T, S, u, v, lodq, table) : sample_slot_lod<false, false>(T, S, u, v, lodq, table);
        } else {
            TexelStores<true> T;
            T.texels = nullptr; T.blocks = reinterpret_cast<const uint2*>(chain); T.format = S.format;
            c = srgb ? sample_slot_lod<true, true>(T, S, u, v, lodq, table) : sample_slot_lod<false, true>(T, S, u, v, lodq, table);
        }
        out[4u * i] = c.x; out[4u * i + 1u] = c.y; out[4u * i + 2u] = c.z; out[4u * i + 3u] = c.w;
    }
    std::free(chain);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    const bool ok = std::fwrite(out.data(), 4, out.size(), o) == out.size();
    std::fclose(o);
    return ok ? 0 : 2;
}
