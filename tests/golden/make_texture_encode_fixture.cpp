// Runs the reference's block compressor (its vendored stb_dxt.h, included where it lies: nothing of it is copied) over the RGBA8
// blocks of a file: argv[1] holds n blocks of 64 bytes (texel 4 * y + x, RGBA), argv[2] receives, per block, 48 bytes:
//   BC1 (alpha = 0, HIGHQUAL; 8 B) | BC3 (alpha = 1, HIGHQUAL; 16 B) | BC4 of .r (8 B) | BC5 of .rg (16 B)
// -- the four calls of the reference's importer (asset_texture_helper.cpp mipmapCompressBC1/3/4/5).
#include <cstdio>
#include <cstring>
#include <vector>

#define STB_DXT_IMPLEMENTATION
#include "stb_dxt.h"

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s blocks.bin out.bin\n", argv[0]); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = in ? std::fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { std::perror("open"); return 1; }
    unsigned char block[64], r[16], rg[32], enc[48];
    size_t n = 0;
    while (std::fread(block, 1, 64, in) == 64) {
        for (int i = 0; i < 16; i++) { r[i] = block[4 * i]; rg[2 * i] = block[4 * i]; rg[2 * i + 1] = block[4 * i + 1]; }
        std::memset(enc, 0, sizeof(enc));
        stb_compress_dxt_block(enc, block, 0, STB_DXT_HIGHQUAL);
        stb_compress_dxt_block(enc + 8, block, 1, STB_DXT_HIGHQUAL);
        stb_compress_bc4_block(enc + 24, r);
        stb_compress_bc5_block(enc + 32, rg);
        if (std::fwrite(enc, 1, 48, out) != 48) { std::perror("write"); return 1; }
        n++;
    }
    std::fclose(in);
    if (std::fclose(out)) { std::perror("close"); return 1; }
    std::fprintf(stderr, "%zu blocks\n", n);
    return 0;
}
