// C ABI, material textures: chordvis_upload_material_textures, the upload jobs it shares with the alpha plane of chordvis_upload_scene
// (block decode, mip generation) and its own (block encode), the per-texture settings, and the read-backs of what was stored.

#include "host_layer.h"
#include "material_tables.h"

using namespace chord;

namespace chord {

// ---- block-compressed textures (ChordTexture::format; kernels_texture.hip) ----
uint32_t tex_block_bytes(uint32_t format)      // of a CHORD_TEXFMT_BC* format; 0: RGBA8 (or none of them)
{
    if (format == CHORD_TEXFMT_BC1_RGB || format == CHORD_TEXFMT_BC4) return 8u;
    if (format == CHORD_TEXFMT_BC3 || format == CHORD_TEXFMT_BC5) return 16u;
    return 0u;
}

void TexDecodeJob::add(const ChordTexture& tx, uint32_t dst, uint32_t first)
{
    const uint32_t bb = tex_block_bytes(tx.format);
    const uint64_t offset = (stagingBytes + 15ull) & ~15ull;
    uint64_t bytes = 0, skipped = 0;
    for (uint32_t l = 0; l < tx.mipCount; l++) {
        const uint32_t w = std::max(1u, tx.width >> l), h = std::max(1u, tx.height >> l), bw = (w + 3u) / 4u, bh = (h + 3u) / 4u;
        if (l < first) { skipped += (uint64_t)bw * bh * bb; continue; }
        recs.push_back(chord::DTexLevelRec{blocks, (uint32_t)((offset + bytes) / 8u), dst, w, h, bw, tx.format, 0u});
        blocks += bw * bh; bytes += (uint64_t)bw * bh * bb; dst += w * h;
    }
    copies.push_back(Copy{tx.rgba8 + skipped, offset, bytes});
    stagingBytes = offset + bytes;
}

int TexDecodeJob::run(ChordCtx* c, const char* who, uint32_t* texels, uint8_t* alpha, bool alphaOnly)
{
    if (recs.empty()) return CHORDVIS_OK;
    if (stagingBytes / 8u > 0xFFFFFFFFull) return fail(c, CHORDVIS_E_CAPACITY, "texture decode: more than 32 GiB of compressed texture levels in one upload");
    const uint32_t count = (uint32_t)recs.size();
    recs.push_back(chord::DTexLevelRec{blocks, 0u, 0u, 0u, 0u, 1u, 0u, 0u});      // closes the table
    DeviceTemp<uint8_t> dStaging;
    DeviceTemp<chord::DTexLevelRec> dRecs;
    hipError_t e = hipMalloc((void**)&dStaging.p, stagingBytes);
    if (e == hipSuccess) e = hipMalloc((void**)&dRecs.p, recs.size() * sizeof(recs[0]));
    if (e == hipSuccess) e = hipMemcpy(dRecs.p, recs.data(), recs.size() * sizeof(recs[0]), hipMemcpyHostToDevice);
    for (size_t i = 0; i < copies.size() && e == hipSuccess; i++)
        e = hipMemcpy(dStaging.p + copies[i].offset, copies[i].host, copies[i].bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        chord::launch_texture_decode(c, dRecs.p, count, blocks, dStaging.p, texels, alpha, alphaOnly);
        e = hipGetLastError();
        const hipError_t es = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = es;
    }
    return e == hipSuccess ? CHORDVIS_OK : fail(c, CHORDVIS_E_HIP, who, e);
}

// ---- mip chains made at upload (chordvis_set_texture_mips; kernels_texture.hip) ----
#define CHORD_TEXMIPS_NAMES "flags: 0, 1 (SRGB), 2 (COVERAGE) or 3; pad: 0; alphaCutoff8 with COVERAGE: 1..255"

// The levels texture `t` ends up with under the context's setting (`ms`: that setting, zero where there is none)
uint32_t tex_levels(const ChordCtx* c, uint32_t t, const ChordTexture& tx, ChordTextureMips& ms)
{
    ms = t < c->texMips.size() ? c->texMips[t] : ChordTextureMips{0u, 0u, 0u, 0u};
    if (!ms.levels) return tx.mipCount;
    uint32_t full = 0;
    for (uint32_t m = std::max(tx.width, tx.height); m; m >>= 1) full++;
    return std::max(tx.mipCount, std::min(ms.levels, full));
}

size_t tex_chain_texels(uint32_t width, uint32_t height, uint32_t levels)
{
    size_t n = 0;
    for (uint32_t l = 0; l < levels; l++) n += (size_t)std::max(1u, width >> l) * std::max(1u, height >> l);
    return n;
}

void TexMipJob::add(uint32_t base, uint32_t width, uint32_t height, uint32_t supplied, uint32_t L, const ChordTextureMips& ms, bool coverage)
{
    if (L <= supplied) return;
    const uint32_t flags = ms.flags & CHORD_TEXMIPS_SRGB;
    anySrgb = anySrgb || flags;
    uint32_t l = supplied - 1u, sw = std::max(1u, width >> l), sh = std::max(1u, height >> l);
    uint32_t src = base + (uint32_t)tex_chain_texels(width, height, l);
    for (size_t k = 0; l + 1u < L && (sw > CHORD_TEXMIPS_TAIL || sh > CHORD_TEXMIPS_TAIL); k++, l++) {
        if (steps.size() <= k) { steps.emplace_back(); stepUnits.push_back(0u); }
        const uint32_t dw = std::max(1u, sw >> 1), dh = std::max(1u, sh >> 1), perRow = (dw + 3u) / 4u;
        steps[k].push_back(chord::DTexMipRec{stepUnits[k], src, src + sw * sh, sw, sh, perRow, flags, 0u});
        stepUnits[k] += perRow * dh;
        src += sw * sh; sw = dw; sh = dh;
    }
    if (l + 1u < L) tails.push_back(chord::DTexTailRec{src, sw, sh, L - 1u - l, flags, {0u, 0u, 0u}});
    if (!coverage) return;
    const uint32_t level0 = (uint32_t)cov.size();
    uint32_t off = base;
    for (uint32_t k = 0; k < L; k++) {
        const uint32_t n = std::max(1u, width >> k) * std::max(1u, height >> k), groups = (n + CHORD_TEXCOV_GROUP - 1u) / CHORD_TEXCOV_GROUP;
        if (k == 0u || k >= supplied) {
            cov.push_back(chord::DTexCovRec{covGroups, covScaleGroups, off, n, level0, ms.alphaCutoff8, {0u, 0u}});
            covGroups += groups;
            if (k >= supplied) covScaleGroups += groups;
        }
        off += n;
    }
}

int TexMipJob::run(ChordCtx* c, const char* who, uint32_t* texels, uint8_t* alpha, bool alphaOnly)
{
    if (steps.empty() && tails.empty()) return CHORDVIS_OK;
    // the tables, 32-byte records all: every step's (each closed), the tails, the coverage levels (closed)
    std::vector<uint32_t> words;
    auto put = [&words](const void* p, size_t bytes) { const size_t at = words.size(); words.resize(at + bytes / 4u); if (bytes) std::memcpy(words.data() + at, p, bytes); return at * 4u; };
    std::vector<size_t> stepAt(steps.size());
    for (size_t k = 0; k < steps.size(); k++) {
        steps[k].push_back(chord::DTexMipRec{stepUnits[k], 0u, 0u, 1u, 1u, 1u, 0u, 0u});
        stepAt[k] = put(steps[k].data(), steps[k].size() * sizeof(chord::DTexMipRec));
    }
    const size_t tailAt = put(tails.data(), tails.size() * sizeof(chord::DTexTailRec));
    const uint32_t covCount = (uint32_t)cov.size();
    cov.push_back(chord::DTexCovRec{covGroups, covScaleGroups, 0u, 0u, 0u, 0u, {0u, 0u}});
    const size_t covAt = put(cov.data(), cov.size() * sizeof(chord::DTexCovRec));
    const bool srgb = anySrgb && !alphaOnly;
    float tables[512];
    if (srgb) {
        chordvis_material_constants(tables, nullptr);
        tables[256] = 0.0f;
        for (int k = 1; k < 256; k++) tables[256 + k] = (tables[k - 1] + tables[k]) * 0.5f;
    }
    DeviceTemp<uint8_t> dTables;
    DeviceTemp<float> dSrgb;
    DeviceTemp<uint32_t> dWork;
    const size_t workWords = (size_t)covCount * 257u;
    hipError_t e = hipMalloc((void**)&dTables.p, words.size() * 4u);
    if (e == hipSuccess) e = hipMemcpy(dTables.p, words.data(), words.size() * 4u, hipMemcpyHostToDevice);
    if (e == hipSuccess && srgb) e = hipMalloc((void**)&dSrgb.p, sizeof(tables));
    if (e == hipSuccess && srgb) e = hipMemcpy(dSrgb.p, tables, sizeof(tables), hipMemcpyHostToDevice);
    if (e == hipSuccess && covCount) e = hipMalloc((void**)&dWork.p, workWords * 4u);
    if (e == hipSuccess && covCount) e = hipMemsetAsync(dWork.p, 0, workWords * 4u, c->stream);
    if (e == hipSuccess) {
        for (size_t k = 0; k < steps.size(); k++)
            chord::launch_texture_mips_step(c, (const chord::DTexMipRec*)(dTables.p + stepAt[k]), (uint32_t)steps[k].size() - 1u, stepUnits[k], dSrgb.p, texels, alpha, alphaOnly);
        chord::launch_texture_mips_tail(c, (const chord::DTexTailRec*)(dTables.p + tailAt), (uint32_t)tails.size(), dSrgb.p, texels, alpha, alphaOnly);
        if (covCount) chord::launch_texture_coverage(c, (const chord::DTexCovRec*)(dTables.p + covAt), covCount, covGroups, covScaleGroups, dWork.p, texels, alpha, alphaOnly);
        e = hipGetLastError();
        const hipError_t es = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = es;
    }
    return e == hipSuccess ? CHORDVIS_OK : fail(c, CHORDVIS_E_HIP, who, e);
}

// what chordvis_upload_material_textures keeps
void drop_material_textures(ChordCtx* c)
{
    dfree(c->dMatRecords); dfree(c->dMatTexels); dfree(c->dMatBlocks); dfree(c->dMatFeedback);
    c->matTexelCount = 0; c->matBlockUnits = 0;
    c->matTexturesLoaded = false; c->matAnyNormalTexture = false; c->matTex.clear();
}

} // namespace chord

namespace {

// ---- block compression at upload (chordvis_set_texture_compress; kernels_texture.hip) ----
#define CHORD_TEXCOMPRESS_NAMES "0 (none), 1 (BC1_RGB), 2 (BC3), 3 (BC4), 4 (BC5)"

// The encoder's four tables (device_layer.h CHORD_TEXENC_*), derived: the optimal single-colour pairs by the exhaustive scan of
// DESIGN.md 2 item 9(j), the midpoints as the float nearest to (e(q) + e(q + 1)) / 510 rounded to six decimals
void tex_encode_tables(uint32_t out[CHORD_TEXENC_TABLE_WORDS])
{
    std::memset(out, 0, CHORD_TEXENC_TABLE_WORDS * 4u);
    for (int bits = 5; bits <= 6; bits++) {
        const int size = 1 << bits;
        auto e = [bits](int c) { return bits == 5 ? (c * 33) >> 2 : (c * 65) >> 4; };
        const uint32_t pairs = bits == 5 ? CHORD_TEXENC_OMATCH5 : CHORD_TEXENC_OMATCH6, mids = bits == 5 ? CHORD_TEXENC_MID5 : CHORD_TEXENC_MID6;
        for (int target = 0; target < 256; target++) {
            int bestMn = 0, bestMx = 0, bestErr = 256 * 100;
            for (int mn = 0; mn < size; mn++)
                for (int mx = 0; mx < size; mx++) {
                    const int err = std::abs((2 * e(mx) + e(mn)) / 3 - target) * 100 + std::abs(e(mx) - e(mn)) * 3;
                    if (err < bestErr) { bestMn = mn; bestMx = mx; bestErr = err; }
                }
            out[pairs + (target >> 1)] |= (uint32_t)(bestMx | bestMn << 8) << (16 * (target & 1));
        }
        for (int q = 0; q < size; q++) {
            float m = 1.0f;
            if (q + 1 < size) {
                // six decimals of k / 510, rounded to nearest (2 * 10^6 k = 510 (2 m + 1) has no solution: never a tie), then the
                // nearest float: the decimal's nearest double first, which sits far from every float's rounding boundary
                const long long k = e(q) + e(q + 1), micro = (k * 2000000ll + 510ll) / 1020ll;
                m = (float)((double)micro / 1000000.0);
            }
            std::memcpy(&out[mids + q], &m, 4);
        }
    }
}

// The levels one upload encodes: their texels are in a staging buffer when the job runs (copied, decoded or made there), one record
// per level goes to a small device table, ONE kernel launch encodes them all into dMatBlocks; the table is freed after the
// synchronise (the staging buffer is the caller's).
struct TexEncodeJob {
    std::vector<chord::DTexEncRec> recs;
    uint32_t blocks = 0;

    // src: level 0's first texel in the staging buffer; dst: the stored chain's first unit in dMatBlocks, where level `first` goes
    // (chordvis_set_texture_first_level: the levels before it take no unit); levels max(from, first) .. L-1 are encoded
    void add(uint32_t src, uint32_t dst, uint32_t width, uint32_t height, uint32_t from, uint32_t L, uint32_t format, uint32_t first = 0u)
    {
        const uint32_t unitsPerBlock = tex_block_bytes(format) / 8u;
        for (uint32_t l = 0; l < L; l++) {
            const uint32_t w = std::max(1u, width >> l), h = std::max(1u, height >> l), bw = (w + 3u) / 4u, bh = (h + 3u) / 4u;
            if (l >= from && l >= first) {
                recs.push_back(chord::DTexEncRec{blocks, src, dst, w, h, bw, format, 0u});
                blocks += bw * bh;
            }
            src += w * h;
            if (l >= first) dst += bw * bh * unitsPerBlock;
        }
    }

    int run(ChordCtx* c, const char* who, const uint32_t* staging, void* blockStore)
    {
        if (recs.empty()) return CHORDVIS_OK;
        if (!c->dTexEncTables) {
            uint32_t tables[CHORD_TEXENC_TABLE_WORDS];
            tex_encode_tables(tables);
            hipError_t e = hipMalloc((void**)&c->dTexEncTables, sizeof(tables));
            if (e == hipSuccess) e = hipMemcpy(c->dTexEncTables, tables, sizeof(tables), hipMemcpyHostToDevice);
            if (e != hipSuccess) { dfree(c->dTexEncTables); return fail(c, CHORDVIS_E_HIP, who, e); }
        }
        const uint32_t count = (uint32_t)recs.size();
        recs.push_back(chord::DTexEncRec{blocks, 0u, 0u, 1u, 1u, 1u, 0u, 0u});        // closes the table
        DeviceTemp<chord::DTexEncRec> dRecs;
        hipError_t e = hipMalloc((void**)&dRecs.p, recs.size() * sizeof(recs[0]));
        if (e == hipSuccess) e = hipMemcpy(dRecs.p, recs.data(), recs.size() * sizeof(recs[0]), hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            chord::launch_texture_encode(c, dRecs.p, count, blocks, c->dTexEncTables, staging, blockStore);
            e = hipGetLastError();
            const hipError_t es = hipStreamSynchronize(c->stream);
            if (e == hipSuccess) e = es;
        }
        return e == hipSuccess ? CHORDVIS_OK : fail(c, CHORDVIS_E_HIP, who, e);
    }
};

} // namespace

extern "C" {

// The RGBA texels and material records chordvis_resolve_material samples.  Nothing of the scene upload
// is touched: dTexAlpha / DMaterial stay what the raster reads.
int chordvis_upload_material_textures(ChordCtx* c, const ChordSceneDesc* s)
{
    if (!c || !s) return fail(c, CHORDVIS_E_INVALID, "upload_material_textures: null argument");
    if (c->sharedScene) return fail(c, CHORDVIS_E_INVALID, "upload_material_textures: not on a depth-view context");
    if (!c->sceneLoaded) return fail(c, CHORDVIS_E_INVALID, "upload_material_textures: no scene (call chordvis_upload_scene first)");
    if (!s->materials || s->materialCount != c->materialCount)
        return fail(c, CHORDVIS_E_INVALID, "upload_material_textures: the descriptor's materialCount differs from the uploaded scene's");
    (void)hipSetDevice(c->device);
    CHORD_HIP(c, hipStreamSynchronize(c->stream));                         // (a resolve in flight may read the records being replaced)
    drop_material_textures(c);

    const uint32_t nTex = s->textures ? s->textureCount : 0u;
    std::vector<uint8_t> named(nTex, 0);
    auto slot_ids = [](const ChordMaterial& m, uint32_t tex[4], uint32_t smp[4]) {
        tex[CHORD_MATSLOT_BASECOLOR] = m.baseColorId; smp[CHORD_MATSLOT_BASECOLOR] = m.baseColorSampler;
        tex[CHORD_MATSLOT_EMISSIVE] = m.emissiveTexture; smp[CHORD_MATSLOT_EMISSIVE] = m.emissiveSampler;
        tex[CHORD_MATSLOT_NORMAL] = m.normalTexture; smp[CHORD_MATSLOT_NORMAL] = m.normalSampler;
        tex[CHORD_MATSLOT_METALROUGH] = m.metallicRoughnessTexture; smp[CHORD_MATSLOT_METALROUGH] = m.metallicRoughnessSampler;
    };
    uint32_t tex[4], smp[4];
    for (uint32_t m = 0; m < s->materialCount; m++) {
        slot_ids(s->materials[m], tex, smp);
        for (int k = 0; k < 4; k++) if (tex[k] < nTex) named[tex[k]] = 1;
    }
    // RGBA8 chains are copied to their place in dMatTexels as they are (little-endian: R is the low byte of the word);
    // block-compressed ones are expanded there by one kernel launch
    // ... unless the context's store is CHORD_TEXSTORE_BLOCKS and every level is supplied: such a chain is copied as it is into
    // dMatBlocks (8-byte units, 16-byte aligned), and the sampler decodes what it taps
    size_t texelCount = 0;
    uint64_t blockUnits = 0;
    TexDecodeJob decode;
    TexMipJob mips;                                                        // chordvis_set_texture_mips: the levels made here
    std::vector<uint32_t> texBase(nTex, 0xFFFFFFFFu), texLevels(nTex, 0u), texKept(nTex, 0u);   // texKept: the format of a chain kept as blocks
    // chordvis_set_texture_compress: the chains encoded here.  Their texels live in a staging buffer of their own (texStage: level
    // 0's first texel in it) from the copy through the decode and the mip generation to the encode, and are freed with it
    size_t stageCount = 0;
    TexDecodeJob stageDecode;
    TexMipJob stageMips;
    TexEncodeJob encode;
    std::vector<uint32_t> texStage(nTex, 0xFFFFFFFFu);
    // chordvis_set_texture_first_level: the levels before texFirst[t] are not stored.  A texel chain that has levels to make is
    // finished in the staging buffer too, and its kept levels copied from there (trims)
    std::vector<uint32_t> texFirst(nTex, 0u);
    struct TrimCopy { uint32_t src, dst; size_t count; };
    std::vector<TrimCopy> trims;
    for (uint32_t t = 0; t < nTex; t++) {
        texLevels[t] = s->textures[t].mipCount;
        if (!named[t]) continue;
        const ChordTexture& tx = s->textures[t];
        if (tx.format != CHORD_TEXFMT_RGBA8 && !tex_block_bytes(tx.format))
            return fail(c, CHORDVIS_E_INVALID, "upload_material_textures: unknown ChordTexture::format on a texture a material names; allowed: " CHORD_TEXFMT_NAMES);
        if (!tx.rgba8 || tx.width == 0 || tx.height == 0 || tx.mipCount == 0 || tx.width > 16384u || tx.height > 16384u || tx.mipCount > CHORD_MAX_TEX_LEVELS)
            return fail(c, CHORDVIS_E_INVALID, "upload_material_textures: a texture a material names has no data, or is larger than 16384 / 15 levels");
        ChordTextureMips ms;
        const uint32_t L = tex_levels(c, t, tx, ms);                       // (>= mipCount; the levels beyond it are made on the device)
        const uint32_t f = std::min(t < c->texFirstLevel.size() ? c->texFirstLevel[t] : 0u, L - 1u);
        const uint32_t fw = std::max(1u, tx.width >> f), fh = std::max(1u, tx.height >> f);   // the stored texture: fw x fh, L - f levels
        texFirst[t] = f;
        const uint32_t target = (c->matTextureStore == CHORD_TEXSTORE_BLOCKS && t < c->texCompress.size()) ? c->texCompress[t] : 0u;
        if (target && tex_block_bytes(tx.format) && tx.format != target)
            return fail(c, CHORDVIS_E_INVALID, "upload_material_textures: a block-compressed texture's format differs from its chordvis_set_texture_compress target (supplied levels are never re-encoded)");
        if (c->matTextureStore == CHORD_TEXSTORE_BLOCKS && tex_block_bytes(tx.format) && L == tx.mipCount) {
            uint64_t bytes = 0;
            (void)chordvis_texture_chain_bytes(tx.format, fw, fh, L - f, &bytes);
            const uint64_t units = ((bytes + 15ull) & ~15ull) / 8u;
            if (blockUnits + units >= 0xFFFFFFFFull) return fail(c, CHORDVIS_E_CAPACITY, "upload_material_textures: more than 2^32 8-byte units of textures kept as blocks");
            texBase[t] = (uint32_t)blockUnits; texKept[t] = tx.format; texLevels[t] = L - f;
            blockUnits += units;
            continue;
        }
        if (target) {
            // an RGBA8 source: every level is encoded; a source in the target format with made levels: those alone
            uint64_t bytes = 0;
            (void)chordvis_texture_chain_bytes(target, fw, fh, L - f, &bytes);
            const uint64_t units = ((bytes + 15ull) & ~15ull) / 8u;
            if (blockUnits + units >= 0xFFFFFFFFull) return fail(c, CHORDVIS_E_CAPACITY, "upload_material_textures: more than 2^32 8-byte units of textures kept as blocks");
            const size_t count = tex_chain_texels(tx.width, tx.height, L);
            if (stageCount + count >= 0xFFFFFFFFull) return fail(c, CHORDVIS_E_CAPACITY, "upload_material_textures: more than 4 G texels staged for compression in one upload");
            texBase[t] = (uint32_t)blockUnits; texKept[t] = target; texLevels[t] = L - f; texStage[t] = (uint32_t)stageCount;
            if (tx.format != CHORD_TEXFMT_RGBA8) stageDecode.add(tx, (uint32_t)stageCount);
            stageMips.add((uint32_t)stageCount, tx.width, tx.height, tx.mipCount, L, ms,
                          (ms.flags & CHORD_TEXMIPS_COVERAGE) && (tx.format == CHORD_TEXFMT_RGBA8 || tx.format == CHORD_TEXFMT_BC3));
            encode.add((uint32_t)stageCount, (uint32_t)blockUnits, tx.width, tx.height, tx.format == CHORD_TEXFMT_RGBA8 ? 0u : tx.mipCount, L, target, f);
            stageCount += count; blockUnits += units;
            continue;
        }
        const size_t count = tex_chain_texels(fw, fh, L - f);
        if (texelCount + count >= 0xFFFFFFFFull) return fail(c, CHORDVIS_E_CAPACITY, "upload_material_textures: more than 4 G texels");
        texBase[t] = (uint32_t)texelCount; texLevels[t] = L - f;
        if (f && L > tx.mipCount) {
            // trimmed, with levels to make: the whole chain is finished in the staging buffer, as it would be in the store
            const size_t whole = tex_chain_texels(tx.width, tx.height, L);
            if (stageCount + whole >= 0xFFFFFFFFull) return fail(c, CHORDVIS_E_CAPACITY, "upload_material_textures: more than 4 G texels staged in one upload");
            texStage[t] = (uint32_t)stageCount;
            if (tx.format != CHORD_TEXFMT_RGBA8) stageDecode.add(tx, (uint32_t)stageCount);
            stageMips.add((uint32_t)stageCount, tx.width, tx.height, tx.mipCount, L, ms,
                          (ms.flags & CHORD_TEXMIPS_COVERAGE) && (tx.format == CHORD_TEXFMT_RGBA8 || tx.format == CHORD_TEXFMT_BC3));
            trims.push_back(TrimCopy{(uint32_t)(stageCount + tex_chain_texels(tx.width, tx.height, f)), (uint32_t)texelCount, count});
            stageCount += whole; texelCount += count;
            continue;
        }
        if (f) {                                                           // trimmed, every level supplied: the kept ones alone arrive
            if (tx.format != CHORD_TEXFMT_RGBA8) decode.add(tx, (uint32_t)texelCount, f);
            texelCount += count;
            continue;
        }
        if (tx.format != CHORD_TEXFMT_RGBA8) decode.add(tx, (uint32_t)texelCount);
        // (BC1_RGB, BC4, BC5: alpha 255 at every level, which the rescale would leave as it is)
        mips.add((uint32_t)texelCount, tx.width, tx.height, tx.mipCount, L, ms,
                 (ms.flags & CHORD_TEXMIPS_COVERAGE) && (tx.format == CHORD_TEXFMT_RGBA8 || tx.format == CHORD_TEXFMT_BC3));
        texelCount += count;
    }
    auto linear = [](uint32_t f) { return f == CHORD_FILTER_LINEAR || f == CHORD_FILTER_LINEAR_MIPMAP_NEAREST || f == CHORD_FILTER_LINEAR_MIPMAP_LINEAR; };
    std::vector<chord::DMatRecord> recs(s->materialCount);
    bool anyNormal = false;
    for (uint32_t m = 0; m < s->materialCount; m++) {
        const ChordMaterial& mat = s->materials[m];
        chord::DMatRecord& d = recs[m];
        std::memset(&d, 0, sizeof(d));
        std::memcpy(d.baseColorFactor, mat.baseColorFactor, 16); std::memcpy(d.emissiveFactor, mat.emissiveFactor, 12);
        d.roughnessFactor = mat.roughnessFactor; d.metallicFactor = mat.metallicFactor; d.normalFactorScale = mat.normalFactorScale;
        d.occlusionTextureStrength = mat.occlusionTextureStrength; d.bExistOcclusion = mat.bExistOcclusion != 0u;
        d.pbr = mat.materialType == 1u;                                    // kLightingType_GLTF_MetallicRoughnessPBR, base.h:423
        d.twoSided = mat.bTwoSided != 0u;
        slot_ids(mat, tex, smp);
        for (int k = 0; k < 4; k++) {
            chord::DMatSlot& S = d.slot[k];
            ChordSampler sm{CHORD_FILTER_NEAREST, CHORD_FILTER_NEAREST, CHORD_WRAP_REPEAT, CHORD_WRAP_REPEAT};
            if (s->samplers && smp[k] < s->samplerCount) sm = s->samplers[smp[k]];
            S.wrapS = sm.wrapS; S.wrapT = sm.wrapT;
            S.filter = (linear(sm.magFilter) ? CHORD_MATSLOT_MAG_LINEAR : 0u) | (linear(sm.minFilter) ? CHORD_MATSLOT_MIN_LINEAR : 0u) |
                       ((sm.minFilter == CHORD_FILTER_NEAREST_MIPMAP_NEAREST || sm.minFilter == CHORD_FILTER_LINEAR_MIPMAP_NEAREST) ? CHORD_MATSLOT_MIP_NEAREST : 0u) |
                       ((sm.minFilter == CHORD_FILTER_NEAREST_MIPMAP_LINEAR || sm.minFilter == CHORD_FILTER_LINEAR_MIPMAP_LINEAR) ? CHORD_MATSLOT_MIP_LINEAR : 0u);
            if (tex[k] >= nTex) continue;                                  // mips = 0: the slot's fallback
            const ChordTexture& tx = s->textures[tex[k]];
            S.mips = texLevels[tex[k]];
            S.format = texKept[tex[k]];
            S.texture = tex[k];
            const uint32_t first = texFirst[tex[k]];
            const uint32_t unitsPerBlock = tex_block_bytes(S.format) / 8u;  // (0: a level is w * h texels)
            uint32_t off = texBase[tex[k]];
            for (uint32_t l = 0; l < S.mips; l++) {
                const uint32_t w = std::max(1u, tx.width >> (first + l)), h = std::max(1u, tx.height >> (first + l));
                chord::DMatLevel& L = S.levels[l];
                L.base = off; L.dims = (w - 1u) | (h - 1u) << 16;
                tex_wrap_constants(w, S.wrapS, L.magicS, L.biasS);
                tex_wrap_constants(h, S.wrapT, L.magicT, L.biasT);
                off += unitsPerBlock ? ((w + 3u) / 4u) * ((h + 3u) / 4u) * unitsPerBlock : w * h;
            }
            if (k == (int)CHORD_MATSLOT_NORMAL) anyNormal = true;
        }
    }
    int rc;
    if ((rc = dalloc(c, &c->dMatRecords, recs.size()))) return rc;
    CHORD_HIP(c, hipMemcpy(c->dMatRecords, recs.data(), recs.size() * sizeof(recs[0]), hipMemcpyHostToDevice));
    if (texelCount) {
        if ((rc = dalloc(c, &c->dMatTexels, texelCount))) { drop_material_textures(c); return rc; }
        for (uint32_t t = 0; t < nTex; t++) {
            const ChordTexture& tx = s->textures[t];
            if (texBase[t] == 0xFFFFFFFFu || tx.format != CHORD_TEXFMT_RGBA8 || texKept[t]) continue;     // (texKept: encoded below, from the staging buffer)
            if (texStage[t] != 0xFFFFFFFFu) continue;                      // (trimmed, with made levels: copied below, from the staging buffer)
            const size_t skip = tex_chain_texels(tx.width, tx.height, texFirst[t]);   // (0 without chordvis_set_texture_first_level)
            const size_t count = tex_chain_texels(tx.width, tx.height, tx.mipCount) - skip;
            hipError_t e = hipMemcpy(c->dMatTexels + texBase[t], tx.rgba8 + skip * 4, count * 4, hipMemcpyHostToDevice);
            if (e != hipSuccess) { drop_material_textures(c); return fail(c, CHORDVIS_E_HIP, "upload_material_textures: hipMemcpy", e); }
        }
        if ((rc = decode.run(c, "upload_material_textures: texture decode", c->dMatTexels, nullptr, false))) { drop_material_textures(c); return rc; }
        if ((rc = mips.run(c, "upload_material_textures: texture mips", c->dMatTexels, nullptr, false))) { drop_material_textures(c); return rc; }
    }
    if (blockUnits) {
        if ((rc = dalloc(c, &c->dMatBlocks, blockUnits))) { drop_material_textures(c); return rc; }
        for (uint32_t t = 0; t < nTex; t++) {
            if (!texKept[t]) continue;
            const ChordTexture& tx = s->textures[t];
            uint64_t bytes = 0, supplied = 0, skip = 0;                    // of the stored chain / of the levels that arrive as blocks / of those not stored
            const uint32_t f = texFirst[t];
            (void)chordvis_texture_chain_bytes(texKept[t], std::max(1u, tx.width >> f), std::max(1u, tx.height >> f), texLevels[t], &bytes);
            if (tx.format != CHORD_TEXFMT_RGBA8) {
                (void)chordvis_texture_chain_bytes(tx.format, tx.width, tx.height, tx.mipCount, &supplied);
                if (f) (void)chordvis_texture_chain_bytes(tx.format, tx.width, tx.height, std::min(f, tx.mipCount), &skip);
                supplied -= skip;
            }
            hipError_t e = supplied ? hipMemcpy(c->dMatBlocks + texBase[t], tx.rgba8 + skip, supplied, hipMemcpyHostToDevice) : hipSuccess;
            if (e == hipSuccess && (bytes & 15ull)) e = hipMemset((uint8_t*)(c->dMatBlocks + texBase[t]) + bytes, 0, 16u - (bytes & 15ull));   // (the chain's padding)
            if (e != hipSuccess) { drop_material_textures(c); return fail(c, CHORDVIS_E_HIP, "upload_material_textures: hipMemcpy", e); }
        }
    }
    if (stageCount) {
        // the chains to encode: supplied texels copied, supplied blocks decoded, the other levels made -- the kernels of the texel
        // store on a buffer of their own --, then one launch encodes them all
        DeviceTemp<uint32_t> dStage;
        hipError_t e = hipMalloc((void**)&dStage.p, stageCount * 4u);
        for (uint32_t t = 0; t < nTex && e == hipSuccess; t++) {
            const ChordTexture& tx = s->textures[t];
            if (texStage[t] == 0xFFFFFFFFu || tx.format != CHORD_TEXFMT_RGBA8) continue;
            e = hipMemcpy(dStage.p + texStage[t], tx.rgba8, tex_chain_texels(tx.width, tx.height, tx.mipCount) * 4u, hipMemcpyHostToDevice);
        }
        rc = e == hipSuccess ? CHORDVIS_OK : fail(c, CHORDVIS_E_HIP, "upload_material_textures: staging for compression", e);
        if (!rc) rc = stageDecode.run(c, "upload_material_textures: texture decode", dStage.p, nullptr, false);
        if (!rc) rc = stageMips.run(c, "upload_material_textures: texture mips", dStage.p, nullptr, false);
        if (!rc) rc = encode.run(c, "upload_material_textures: texture encode", dStage.p, c->dMatBlocks);
        for (size_t i = 0; i < trims.size() && !rc; i++) {
            e = hipMemcpy(c->dMatTexels + trims[i].dst, dStage.p + trims[i].src, trims[i].count * 4u, hipMemcpyDeviceToDevice);
            if (e != hipSuccess) rc = fail(c, CHORDVIS_E_HIP, "upload_material_textures: copy of the kept levels", e);
        }
        if (rc) { drop_material_textures(c); return rc; }
    }
    c->matTex.resize(nTex);
    for (uint32_t t = 0; t < nTex; t++)
        c->matTex[t] = ChordCtx::MatTexInfo{texBase[t], std::max(1u, s->textures[t].width >> texFirst[t]), std::max(1u, s->textures[t].height >> texFirst[t]),
                                            texLevels[t], texKept[t], texFirst[t]};
    c->matTexelCount = texelCount; c->matBlockUnits = blockUnits;
    c->matTexturesLoaded = true; c->matAnyNormalTexture = anyNormal;
    return CHORDVIS_OK;
}

int chordvis_set_material_texture_store(ChordCtx* c, uint32_t mode)
{
    if (!c) return CHORDVIS_E_INVALID;
    if (mode != CHORD_TEXSTORE_EXPANDED && mode != CHORD_TEXSTORE_BLOCKS)
        return fail(c, CHORDVIS_E_INVALID, "set_material_texture_store: the store is 0 (CHORD_TEXSTORE_EXPANDED) or 1 (CHORD_TEXSTORE_BLOCKS)");
    c->matTextureStore = mode;
    return CHORDVIS_OK;
}
uint32_t chordvis_material_texture_store(const ChordCtx* c) { return c ? c->matTextureStore : 0u; }

int chordvis_material_texture_memory(ChordCtx* c, uint64_t* texelBytes, uint64_t* blockBytes)
{
    if (!c) return CHORDVIS_E_INVALID;
    if (!c->matTexturesLoaded) return fail(c, CHORDVIS_E_INVALID, "material_texture_memory: no chordvis_upload_material_textures since the last chordvis_upload_scene");
    if (texelBytes) *texelBytes = c->matTexelCount * 4u;
    if (blockBytes) *blockBytes = c->matBlockUnits * 8u;
    return CHORDVIS_OK;
}

int chordvis_texture_chain_bytes(uint32_t format, uint32_t width, uint32_t height, uint32_t mipCount, uint64_t* bytes)
{
    const uint32_t bb = tex_block_bytes(format);
    if (!bytes || (format != CHORD_TEXFMT_RGBA8 && !bb) || width == 0 || height == 0 || mipCount == 0) return CHORDVIS_E_INVALID;
    unsigned __int128 total = 0;
    for (uint32_t l = 0; l < mipCount && l < 32u; l++) {
        const uint64_t w = std::max(1u, width >> l), h = std::max(1u, height >> l);
        total += bb ? (unsigned __int128)((w + 3u) / 4u) * ((h + 3u) / 4u) * bb : (unsigned __int128)w * h * 4u;
    }
    if (mipCount > 32u) total += (unsigned __int128)(mipCount - 32u) * (bb ? bb : 4u);     // (1 x 1 from level 32 on)
    if (total > 0xFFFFFFFFFFFFFFFFull) return CHORDVIS_E_INVALID;
    *bytes = (uint64_t)total;
    return CHORDVIS_OK;
}

int chordvis_readback_material_blocks(ChordCtx* c, uint32_t textureId, uint8_t* host, uint64_t bytes)
{
    if (!c || !host) return fail(c, CHORDVIS_E_INVALID, "readback_material_blocks: null argument");
    if (!c->matTexturesLoaded) return fail(c, CHORDVIS_E_INVALID, "readback_material_blocks: no chordvis_upload_material_textures since the last chordvis_upload_scene");
    if (textureId >= c->matTex.size() || c->matTex[textureId].base == 0xFFFFFFFFu || !c->matTex[textureId].format)
        return fail(c, CHORDVIS_E_INVALID, "readback_material_blocks: the texture is not kept as blocks (no material names it, or it is stored as texels)");
    const ChordCtx::MatTexInfo& t = c->matTex[textureId];
    uint64_t chain = 0;
    (void)chordvis_texture_chain_bytes(t.format, t.width, t.height, t.mipCount, &chain);
    if (bytes != chain) return fail(c, CHORDVIS_E_INVALID, "readback_material_blocks: bytes differs from chordvis_texture_chain_bytes of the stored chain");
    (void)hipSetDevice(c->device);
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    CHORD_HIP(c, hipMemcpy(host, c->dMatBlocks + t.base, chain, hipMemcpyDeviceToHost));
    return CHORDVIS_OK;
}

int chordvis_readback_material_texture(ChordCtx* c, uint32_t textureId, uint32_t level, uint8_t* hostRgba8)
{
    if (!c || !hostRgba8) return fail(c, CHORDVIS_E_INVALID, "readback_material_texture: null argument");
    if (!c->matTexturesLoaded) return fail(c, CHORDVIS_E_INVALID, "readback_material_texture: no chordvis_upload_material_textures since the last chordvis_upload_scene");
    if (textureId >= c->matTex.size() || c->matTex[textureId].base == 0xFFFFFFFFu)
        return fail(c, CHORDVIS_E_INVALID, "readback_material_texture: no material of the scene names this texture");
    const ChordCtx::MatTexInfo& t = c->matTex[textureId];
    if (level >= t.mipCount) return fail(c, CHORDVIS_E_INVALID, "readback_material_texture: the level is not below the texture's mipCount");
    const uint32_t w = std::max(1u, t.width >> level), h = std::max(1u, t.height >> level);
    const size_t count = (size_t)w * h;
    (void)hipSetDevice(c->device);
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    if (t.format) {
        // kept as blocks: the upload decoder expands the one level into a temporary buffer (one record, one launch)
        const uint32_t unitsPerBlock = tex_block_bytes(t.format) / 8u, bw = (w + 3u) / 4u, bh = (h + 3u) / 4u;
        uint32_t src = t.base;
        for (uint32_t l = 0; l < level; l++) src += ((std::max(1u, t.width >> l) + 3u) / 4u) * ((std::max(1u, t.height >> l) + 3u) / 4u) * unitsPerBlock;
        const chord::DTexLevelRec recs[2] = {{0u, src, 0u, w, h, bw, t.format, 0u}, {bw * bh, 0u, 0u, 0u, 0u, 1u, 0u, 0u}};
        DeviceTemp<uint32_t> dOut;
        DeviceTemp<chord::DTexLevelRec> dRecs;
        hipError_t e = hipMalloc((void**)&dOut.p, count * 4);
        if (e == hipSuccess) e = hipMalloc((void**)&dRecs.p, sizeof(recs));
        if (e == hipSuccess) e = hipMemcpy(dRecs.p, recs, sizeof(recs), hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            chord::launch_texture_decode(c, dRecs.p, 1u, bw * bh, c->dMatBlocks, dOut.p, nullptr, false);
            e = hipGetLastError();
            const hipError_t es = hipStreamSynchronize(c->stream);
            if (e == hipSuccess) e = es;
        }
        if (e == hipSuccess) e = hipMemcpy(hostRgba8, dOut.p, count * 4, hipMemcpyDeviceToHost);
        return e == hipSuccess ? CHORDVIS_OK : fail(c, CHORDVIS_E_HIP, "readback_material_texture: texture decode", e);
    }
    size_t off = t.base;
    for (uint32_t l = 0; l < level; l++) off += (size_t)std::max(1u, t.width >> l) * std::max(1u, t.height >> l);
    CHORD_HIP(c, hipMemcpy(hostRgba8, c->dMatTexels + off, count * 4, hipMemcpyDeviceToHost));
    return CHORDVIS_OK;
}

int chordvis_set_texture_first_level(ChordCtx* c, const uint32_t* perTextureFirst, uint32_t count)
{
    if (!c) return CHORDVIS_E_INVALID;
    if (!perTextureFirst || !count) c->texFirstLevel.clear();
    else c->texFirstLevel.assign(perTextureFirst, perTextureFirst + count);
    return CHORDVIS_OK;
}

int chordvis_texture_first_level(const ChordCtx* c, uint32_t textureId, uint32_t* first)
{
    if (!c || !first) return CHORDVIS_E_INVALID;
    *first = textureId < c->texFirstLevel.size() ? c->texFirstLevel[textureId] : 0u;
    return CHORDVIS_OK;
}

int chordvis_material_texture_levels(ChordCtx* c, uint32_t textureId, uint32_t* firstLevel, uint32_t* levelCount)
{
    if (!c) return CHORDVIS_E_INVALID;
    if (!c->matTexturesLoaded) return fail(c, CHORDVIS_E_INVALID, "material_texture_levels: no chordvis_upload_material_textures since the last chordvis_upload_scene");
    if (textureId >= c->matTex.size() || c->matTex[textureId].base == 0xFFFFFFFFu)
        return fail(c, CHORDVIS_E_INVALID, "material_texture_levels: no material of the scene names this texture");
    if (firstLevel) *firstLevel = c->matTex[textureId].first;
    if (levelCount) *levelCount = c->matTex[textureId].mipCount;
    return CHORDVIS_OK;
}

int chordvis_set_material_anisotropy(ChordCtx* c, uint32_t maxAnisotropy)
{
    if (!c) return CHORDVIS_E_INVALID;
    if (maxAnisotropy != 1u && maxAnisotropy != 2u && maxAnisotropy != 4u && maxAnisotropy != 8u && maxAnisotropy != 16u)
        return fail(c, CHORDVIS_E_INVALID, "set_material_anisotropy: the maximum anisotropy is 1 (off), 2, 4, 8 or 16");
    c->matAnisotropy = maxAnisotropy;
    return CHORDVIS_OK;
}
uint32_t chordvis_material_anisotropy(const ChordCtx* c) { return c ? c->matAnisotropy : 0u; }

int chordvis_set_texture_mips(ChordCtx* c, const ChordTextureMips* perTexture, uint32_t count)
{
    if (!c) return CHORDVIS_E_INVALID;
    if (!perTexture || !count) { c->texMips.clear(); return CHORDVIS_OK; }
    for (uint32_t t = 0; t < count; t++) {
        const ChordTextureMips& m = perTexture[t];
        if ((m.flags & ~(CHORD_TEXMIPS_SRGB | CHORD_TEXMIPS_COVERAGE)) || m.pad ||
            ((m.flags & CHORD_TEXMIPS_COVERAGE) && (m.alphaCutoff8 < 1u || m.alphaCutoff8 > 255u)))
            return fail(c, CHORDVIS_E_INVALID, "set_texture_mips: an entry is not allowed; " CHORD_TEXMIPS_NAMES);
    }
    c->texMips.assign(perTexture, perTexture + count);
    return CHORDVIS_OK;
}

int chordvis_texture_mips(const ChordCtx* c, uint32_t textureId, ChordTextureMips* out)
{
    if (!c || !out) return CHORDVIS_E_INVALID;
    *out = textureId < c->texMips.size() ? c->texMips[textureId] : ChordTextureMips{0u, 0u, 0u, 0u};
    return CHORDVIS_OK;
}

int chordvis_set_texture_compress(ChordCtx* c, const uint32_t* perTextureFormat, uint32_t count)
{
    if (!c) return CHORDVIS_E_INVALID;
    if (!perTextureFormat || !count) { c->texCompress.clear(); return CHORDVIS_OK; }
    for (uint32_t t = 0; t < count; t++)
        if (perTextureFormat[t] && !tex_block_bytes(perTextureFormat[t]))
            return fail(c, CHORDVIS_E_INVALID, "set_texture_compress: an entry is not allowed; allowed: " CHORD_TEXCOMPRESS_NAMES);
    c->texCompress.assign(perTextureFormat, perTextureFormat + count);
    return CHORDVIS_OK;
}

int chordvis_texture_compress(const ChordCtx* c, uint32_t textureId, uint32_t* format)
{
    if (!c || !format) return CHORDVIS_E_INVALID;
    *format = textureId < c->texCompress.size() ? c->texCompress[textureId] : 0u;
    return CHORDVIS_OK;
}

int chordvis_material_constants(float srgbToLinear[256], float srgbToAp1[9])
{
    static const uint32_t srgb[256] = {CHORD_SRGB_TABLE_BITS};
    static const uint32_t ap1[9] = {CHORD_SRGB_2_AP1_BITS};
    if (srgbToLinear) std::memcpy(srgbToLinear, srgb, sizeof(srgb));
    if (srgbToAp1) std::memcpy(srgbToAp1, ap1, sizeof(ap1));
    return CHORDVIS_OK;
}

} // extern "C"
