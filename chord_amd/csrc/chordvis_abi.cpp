// C ABI entry points + the host-side mirror of the reference's pass surface.
//
//   chordvis_instance_culling      <- instanceCulling                 instance_culling.cpp:83-161
//   chordvis_hzb_culling           <- detail::hzbCulling              instance_culling.cpp:286-351
//   chordvis_render_mesh           <- renderMesh / renderMeshRasterPipe  mesh_raster.cpp:76-254
//   chordvis_visibility_stage0/1   <- gltfVisibilityRenderingStage0/1 mesh_raster.cpp:269-329
//   chordvis_build_hzb             <- buildHZB                        hzb.cpp:38-227
//   chordvis_render_frame          <- DeferredRenderer::render hot segment  renderer.cpp:315-345,489
//
// Host code only records work on one HIP stream (the reference records Vulkan commands into one
// command buffer); counts never come back to the CPU inside a frame.

#include "device_layer.h"
#include "material_tables.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>

using namespace chord;

namespace chord {

int fail(ChordCtx* ctx, int code, const char* what, hipError_t e)
{
    if (ctx) {
        char buf[512];
        if (e != hipSuccess) std::snprintf(buf, sizeof(buf), "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
        else std::snprintf(buf, sizeof(buf), "%s", what);
        ctx->lastError = buf;
    }
    return code;
}

} // namespace chord

namespace {

template <typename T>
int dalloc(ChordCtx* c, T** p, size_t count)
{
    if (*p) { (void)hipFree(*p); *p = nullptr; }
    if (count == 0) count = 1;
    CHORD_HIP(c, hipMalloc((void**)p, count * sizeof(T)));
    return CHORDVIS_OK;
}

template <typename T>
void dfree(T*& p) { if (p) { (void)hipFree((void*)p); p = nullptr; } }

// ---- block-compressed textures (ChordTexture::format; kernels_texture.hip) ----
uint32_t tex_block_bytes(uint32_t format)      // of a CHORD_TEXFMT_BC* format; 0: RGBA8 (or none of them)
{
    if (format == CHORD_TEXFMT_BC1_RGB || format == CHORD_TEXFMT_BC4) return 8u;
    if (format == CHORD_TEXFMT_BC3 || format == CHORD_TEXFMT_BC5) return 16u;
    return 0u;
}
#define CHORD_TEXFMT_NAMES "0 (RGBA8), 1 (BC1_RGB), 2 (BC3), 3 (BC4), 4 (BC5)"

// The compressed levels one upload expands: their bytes go to ONE staging buffer (every chain 16-byte aligned in it), one record
// per level to a small device table, one kernel launch decodes them all; buffer and table are freed after the synchronise.
struct TexDecodeJob {
    struct Copy { const uint8_t* host; uint64_t offset, bytes; };
    std::vector<chord::DTexLevelRec> recs;
    std::vector<Copy> copies;
    uint64_t stagingBytes = 0;
    uint32_t blocks = 0;

    // dst: where level `first` goes (a texel index of dMatTexels / a byte index of dTexAlpha); the levels follow as an RGBA8 chain's
    // do.  Levels below `first` (chordvis_set_texture_first_level) are neither staged nor decoded
    void add(const ChordTexture& tx, uint32_t dst, uint32_t first = 0u)
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

    int run(ChordCtx* c, const char* who, uint32_t* texels, uint8_t* alpha, bool alphaOnly)
    {
        if (recs.empty()) return CHORDVIS_OK;
        if (stagingBytes / 8u > 0xFFFFFFFFull) return fail(c, CHORDVIS_E_CAPACITY, "texture decode: more than 32 GiB of compressed texture levels in one upload");
        const uint32_t count = (uint32_t)recs.size();
        recs.push_back(chord::DTexLevelRec{blocks, 0u, 0u, 0u, 0u, 1u, 0u, 0u});      // closes the table
        uint8_t* dStaging = nullptr;
        chord::DTexLevelRec* dRecs = nullptr;
        hipError_t e = hipMalloc((void**)&dStaging, stagingBytes);
        if (e == hipSuccess) e = hipMalloc((void**)&dRecs, recs.size() * sizeof(recs[0]));
        if (e == hipSuccess) e = hipMemcpy(dRecs, recs.data(), recs.size() * sizeof(recs[0]), hipMemcpyHostToDevice);
        for (size_t i = 0; i < copies.size() && e == hipSuccess; i++)
            e = hipMemcpy(dStaging + copies[i].offset, copies[i].host, copies[i].bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            chord::launch_texture_decode(c, dRecs, count, blocks, dStaging, texels, alpha, alphaOnly);
            e = hipGetLastError();
            const hipError_t es = hipStreamSynchronize(c->stream);
            if (e == hipSuccess) e = es;
        }
        if (dStaging) (void)hipFree(dStaging);
        if (dRecs) (void)hipFree(dRecs);
        return e == hipSuccess ? CHORDVIS_OK : fail(c, CHORDVIS_E_HIP, who, e);
    }
};

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

// The levels one upload makes: one launch per level step over every texture that has that step, then one launch whose workgroups
// finish the chains from 64 x 64 down, then the coverage passes; the record tables go to ONE device buffer, freed after the
// synchronise.  Runs after the copies and the decode, on the same stream: it reads what they wrote.
struct TexMipJob {
    std::vector<std::vector<chord::DTexMipRec>> steps;     // [k]: the k-th step of every texture that has one
    std::vector<uint32_t> stepUnits;
    std::vector<chord::DTexTailRec> tails;
    std::vector<chord::DTexCovRec> cov;
    uint32_t covGroups = 0, covScaleGroups = 0;
    bool anySrgb = false;

    // base: where level 0 is (a texel index of dMatTexels / a byte index of dTexAlpha); the first `supplied` levels are there
    // when the job runs, levels supplied .. L-1 are made.  coverage: rescale their alpha (not asked for an alpha of 255 throughout)
    void add(uint32_t base, uint32_t width, uint32_t height, uint32_t supplied, uint32_t L, const ChordTextureMips& ms, bool coverage)
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

    int run(ChordCtx* c, const char* who, uint32_t* texels, uint8_t* alpha, bool alphaOnly)
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
        uint8_t* dTables = nullptr;
        float* dSrgb = nullptr;
        uint32_t* dWork = nullptr;
        const size_t workWords = (size_t)covCount * 257u;
        hipError_t e = hipMalloc((void**)&dTables, words.size() * 4u);
        if (e == hipSuccess) e = hipMemcpy(dTables, words.data(), words.size() * 4u, hipMemcpyHostToDevice);
        if (e == hipSuccess && srgb) e = hipMalloc((void**)&dSrgb, sizeof(tables));
        if (e == hipSuccess && srgb) e = hipMemcpy(dSrgb, tables, sizeof(tables), hipMemcpyHostToDevice);
        if (e == hipSuccess && covCount) e = hipMalloc((void**)&dWork, workWords * 4u);
        if (e == hipSuccess && covCount) e = hipMemsetAsync(dWork, 0, workWords * 4u, c->stream);
        if (e == hipSuccess) {
            for (size_t k = 0; k < steps.size(); k++)
                chord::launch_texture_mips_step(c, (const chord::DTexMipRec*)(dTables + stepAt[k]), (uint32_t)steps[k].size() - 1u, stepUnits[k], dSrgb, texels, alpha, alphaOnly);
            chord::launch_texture_mips_tail(c, (const chord::DTexTailRec*)(dTables + tailAt), (uint32_t)tails.size(), dSrgb, texels, alpha, alphaOnly);
            if (covCount) chord::launch_texture_coverage(c, (const chord::DTexCovRec*)(dTables + covAt), covCount, covGroups, covScaleGroups, dWork, texels, alpha, alphaOnly);
            e = hipGetLastError();
            const hipError_t es = hipStreamSynchronize(c->stream);
            if (e == hipSuccess) e = es;
        }
        if (dTables) (void)hipFree(dTables);
        if (dSrgb) (void)hipFree(dSrgb);
        if (dWork) (void)hipFree(dWork);
        return e == hipSuccess ? CHORDVIS_OK : fail(c, CHORDVIS_E_HIP, who, e);
    }
};

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
        chord::DTexEncRec* dRecs = nullptr;
        hipError_t e = hipMalloc((void**)&dRecs, recs.size() * sizeof(recs[0]));
        if (e == hipSuccess) e = hipMemcpy(dRecs, recs.data(), recs.size() * sizeof(recs[0]), hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            chord::launch_texture_encode(c, dRecs, count, blocks, c->dTexEncTables, staging, blockStore);
            e = hipGetLastError();
            const hipError_t es = hipStreamSynchronize(c->stream);
            if (e == hipSuccess) e = es;
        }
        if (dRecs) (void)hipFree(dRecs);
        return e == hipSuccess ? CHORDVIS_OK : fail(c, CHORDVIS_E_HIP, who, e);
    }
};

// what chordvis_upload_material_textures keeps
void drop_material_textures(ChordCtx* c)
{
    dfree(c->dMatRecords); dfree(c->dMatTexels); dfree(c->dMatBlocks); dfree(c->dMatFeedback);
    c->matTexelCount = 0; c->matBlockUnits = 0;
    c->matTexturesLoaded = false; c->matAnyNormalTexture = false; c->matTex.clear();
}

// what chordvis_upload_world_transforms keeps (hipFree waits for the device: a build in flight finishes on memory that is still its own)
void drop_world_transforms(ChordCtx* c)
{
    dfree(c->dWorldCur); dfree(c->dWorldPrev); dfree(c->dBuildStatus);
    c->buildCount = 0;
}

// Device memory chordvis_set_object_list drops: hipFree waits for the device, and that call must not, so the pointers are kept until a
// call that waits anyway comes by (chordvis_upload_scene, chordvis_destroy, a chordvis_set_object_list that has to grow).
template <typename T>
void retire(ChordCtx* c, T*& p) { if (p) { c->retired.push_back((void*)p); p = nullptr; } }

void free_retired(ChordCtx* c)      // (the caller has let the stream run empty)
{
    for (void* p : c->retired) (void)hipFree(p);
    c->retired.clear();
    for (ChordCtx* k : c->retiredChildren) chordvis_destroy(k);
    c->retiredChildren.clear();
}

// The ray scene (chordvis_build_ray_scene).  The TLAS belongs to an object list: chordvis_set_object_list parks its buffers without
// waiting; the BLASes belong to a scene upload, which has let the stream run empty before it frees them.
void drop_ray_tlas(ChordCtx* c, bool park)
{
    if (park) { retire(c, c->dRayTlas); retire(c, c->dRayLeafRef); retire(c, c->dRayCounters); retire(c, c->dRayLeafBox); retire(c, c->dRayRoot); }
    else { dfree(c->dRayTlas); dfree(c->dRayLeafRef); dfree(c->dRayCounters); dfree(c->dRayLeafBox); dfree(c->dRayRoot); }
    c->rayTlasBuilt = false; c->rayRefitDue = false; c->rayTlasNodes = c->rayTlasDepth = 0; c->rayTlasBytes = 0;
}

void drop_ray_scene(ChordCtx* c)          // (the caller has let the stream run empty)
{
    drop_ray_tlas(c, false);
    dfree(c->dRayBlas); dfree(c->dRayTriangles); dfree(c->dRayBlasRoot); dfree(c->dRayCounts);
    c->rayBlasBuilt = false; c->rayBlasNodes = c->rayBlasTriangles = c->rayBlasDepth = 0; c->rayBlasBytes = 0;
}

// The per-object static table and the totals every launch is sized by, from an object list and the resident scene's tables (hPrims,
// hPrimMeshlets, hPrimTriangles, hMatFlags, hMatType), in O(count): what chordvis_upload_scene and chordvis_set_object_list share.
// Nothing of the context is written but `out` (the caller's) and, on a refusal, the error text.
struct ObjectListTotals { uint64_t groupInst = 0, cmdCap = 0, instTriangles = 0; };

int derive_object_list(ChordCtx* c, const char* fn, const ChordObject* objects, uint32_t count, std::vector<DObjStatic>& out, ObjectListTotals& t)
{
    char buf[224];
    auto refuse = [&](int code, const char* why) { std::snprintf(buf, sizeof(buf), "%s: %s", fn, why); return fail(c, code, buf); };
    const size_t primCount = c->hPrims.size(), materialCount = c->hMatFlags.size();
    out.assign(count, DObjStatic{});
    t = ObjectListTotals{};
    for (uint32_t o = 0; o < count; o++) {
        const ChordObject& ob = objects[o];
        if (ob.GLTFPrimitiveDetail >= primCount || ob.GLTFMaterialData >= materialCount)
            return refuse(CHORDVIS_E_INVALID, "object primitive/material id out of range");
        if (ob.GLTFMaterialData >= (1u << 24)) return refuse(CHORDVIS_E_CAPACITY, "more than 2^24 materials");
        DObjStatic& d = out[o];
        d.prim = ob.GLTFPrimitiveDetail;
        d.matFlags = c->hMatFlags[ob.GLTFMaterialData] | (ob.GLTFMaterialData << 8);
        d.shadingType = c->hMatType[ob.GLTFMaterialData];
        d.groupBase = (uint32_t)t.groupInst;            // (a list past 2^31 - 1 group instances is refused below: the wrapped values are never used)
        for (int i = 0; i < 3; i++) { d.posMin[i] = c->hPrims[d.prim].posMin[i]; d.posMax[i] = c->hPrims[d.prim].posMax[i]; }
        t.groupInst += c->hPrims[d.prim].groupCount;
        t.cmdCap += c->hPrimMeshlets[d.prim];
        t.instTriangles += c->hPrimTriangles[d.prim];
    }
    if (t.cmdCap >= CHORD_MAX_INSTANCE_ID || t.groupInst > 0x7FFFFFFFull)
        return refuse(CHORDVIS_E_CAPACITY, "more than 2^24-2 cluster instances do not fit the 24-bit visibility id (base.h:412)");
    return CHORDVIS_OK;
}

void record(ChordCtx* c, int tag) { chord::stamp(c, tag); }

void begin_frame_stamps(ChordCtx* c)
{
    c->frameLaunchBase = c->launchCount;
    c->stampThisFrame = c->timers && (c->frameIndex % c->timerPeriod) == 0;
    c->frameIndex++;
    if (!c->stampThisFrame) return;
    if (c->timers == 1) { c->stampTags.clear(); c->framesStamped = 0; }
    c->framesStamped++;
    chord::stamp(c, S_FRAME_BEGIN);
}

int alloc_hzb(ChordCtx* c, HzbBuffers& h)
{
    ChordHZBDesc d;
    if (chordvis_hzb_desc(c->width, c->height, &d) != CHORDVIS_OK) return fail(c, CHORDVIS_E_INVALID, "render size unsupported for HZB");
    h.desc = d;
    h.valid = false; h.uploaded = false;
    int rc;
    if ((rc = dalloc(c, &h.minTexels, d.totalTexels))) return rc;
    if ((rc = dalloc(c, &h.maxTexels, d.totalTexels))) return rc;
    if ((rc = dalloc(c, &h.validRange, 2))) return rc;
    CHORD_HIP(c, hipMemsetAsync(h.minTexels, 0, sizeof(uint16_t) * d.totalTexels, c->stream));
    CHORD_HIP(c, hipMemsetAsync(h.maxTexels, 0, sizeof(uint16_t) * d.totalTexels, c->stream));
    return CHORDVIS_OK;
}

int configure_targets(ChordCtx* c, uint64_t* external)
{
    c->resolveFrame = false;
    // visibility words (sharded: rank-major tile slots, ranks * slotsPerRank * 64 * 64 words)
    const uint32_t N = c->shard.ranks;
    c->tilesX = (c->width + CHORD_TILE - 1) >> CHORD_TILE_SHIFT; c->tilesY = (c->height + CHORD_TILE - 1) >> CHORD_TILE_SHIFT;
    c->shard.tilesX = c->tilesX;
    // (allocated for the slot capacity; an all-gather moves ranks x shard.slotsPerRank slots, what the current map uses)
    c->slotCapacity = N > 1 ? chordvis_tile_slot_capacity(c->width, c->height, N) : 0u;
    c->visWords = N > 1 ? (uint64_t)N * c->slotCapacity * (CHORD_TILE * CHORD_TILE) : (uint64_t)c->width * c->height;
    int rc;
    if (external) {
        dfree(c->dVisOwned);
        c->dVis = external; c->visExternal = true;
    } else {
        if ((rc = dalloc(c, &c->dVisOwned, c->visWords))) return rc;
        c->dVis = c->dVisOwned; c->visExternal = false;
    }
    if (N > 1) { if ((rc = dalloc(c, &c->dVisResolved, (uint64_t)c->width * c->height))) return rc; }
    else dfree(c->dVisResolved);
    for (int i = 0; i < 3; i++) if ((rc = alloc_hzb(c, c->hzb[i]))) return rc;
    c->historySlot = 0;
    c->pendingTailSlot = 0;
    {   // per-tile triangle bins of the rasterizer: 64x64-pixel tiles, binCap entries each
        c->binCap = CHORD_BIN_CAP;              // 4K: 2 passes x 2040 tiles x 16384 x 4 B = 267 MB
        if ((rc = dalloc(c, &c->dTileBins, (size_t)2 * c->tilesX * c->tilesY * c->binCap))) return rc;
        c->binPoolChunks = c->limitPoolChunks;  // default: 2 passes x 32 Ki chunks x 1024 entries x 4 B = 256 MB
        if ((rc = dalloc(c, &c->dBinPool, (size_t)2 * c->binPoolChunks * CHORD_BIN_CHUNK))) return rc;
        const size_t tabWords = (size_t)2 * c->tilesX * c->tilesY * c->binMaxChunks;
        if ((rc = dalloc(c, &c->dBinChunkTab, tabWords))) return rc;
        CHORD_HIP(c, hipMemset(c->dBinChunkTab, 0, tabWords * sizeof(unsigned long long)));
        // work items of the tile kernel: every tile once, plus the slices of split tiles (bounded by the entries
        // a pass can hold)
        const size_t tilesN = (size_t)c->tilesX * c->tilesY;
        c->tileItemCap = (uint32_t)(tilesN * (CHORD_TILE_MAX_SLICES + 1u));
        if ((rc = dalloc(c, &c->dTileOrder, ((size_t)1 + c->tileItemCap) * 2))) return rc;   // uint2 per item
        if ((rc = dalloc(c, &c->dTileOrderKeep, ((size_t)1 + c->tileItemCap) * 4))) return rc;    // (two schedules each: this frame's and the one being made for the next)
        if ((rc = dalloc(c, &c->dTileOrderKeep1, ((size_t)1 + c->tileItemCap) * 4))) return rc;
        c->orderAge = c->orderAge1 = 0xFFFFFFFFu;
        if ((rc = dalloc(c, &c->dTileSlabs, tilesN * CHORD_TILE * CHORD_TILE))) return rc;
        CHORD_HIP(c, hipMemset(c->dTileSlabs, 0, tilesN * CHORD_TILE * CHORD_TILE * sizeof(unsigned long long)));
    }
    if ((rc = dalloc(c, &c->dTileRange, (size_t)2 * CHORD_MAX_TILES))) return rc;
    if (!c->hBinHint) {     // what the tile order kernel tells the host about a pass (the longest bin): 64 bytes of mapped host memory
        void* h = nullptr; void* dh = nullptr;
        CHORD_HIP(c, hipHostMalloc(&h, 64, hipHostMallocMapped));
        std::memset(h, 0, 64);
        CHORD_HIP(c, hipHostGetDevicePointer(&dh, h, 0));
        c->hBinHint = static_cast<volatile uint32_t*>(h); c->dBinHint = static_cast<uint32_t*>(dh);
    }
    if (c->dHotTiles) CHORD_HIP(c, hipMemsetAsync(c->dHotTiles, 0, sizeof(uint32_t) * 2 * (1 + CHORD_HOT_TILES), c->stream));   // (tile ids of another target size)
    c->hBinHint[0] = 0u; c->hBinHint[1] = 0u;
    c->hBinHint[2] = 0xFFFFFFFFu; c->hBinHint[3] = 0xFFFFFFFFu;      // clusters per pass of the last finished frame: none yet
    for (int k = 4; k < 8; k++) c->hBinHint[k] = 0u;                  // serials of the last pass found heavy [4 + pass] / light [6 + pass] (launch_raster: TILE_DIRECT): none
    {   // one {min, max} partial per block of the mip-0 kernel (64 x 4 texels per block)
        const uint32_t vw = (c->width + 1) / 2, vh = (c->height + 1) / 2;
        if ((rc = dalloc(c, &c->dRangePartials, (size_t)((vw + 63) / 64) * ((vh + 3) / 4) * 2))) return rc;
    }
    // sharded: the tile map and the two HZB exchange buffers (one slot per tile slot of the visibility buffer)
    if (N > 1) {
        const size_t tilesN = (size_t)c->tilesX * c->tilesY;
        CHORD_HIP(c, hipMemsetAsync(c->dVis, 0, c->visWords * 8, c->stream));   // (slots of edge tiles are partly padding: defined bytes on the wire)
        if ((rc = dalloc(c, &c->dShardTables, 64 + (tilesN + 1) / 2))) return rc;
        if ((rc = dalloc(c, &c->dTileLoads, tilesN))) return rc;
        CHORD_HIP(c, hipMemsetAsync(c->dTileLoads, 0, tilesN * 4, c->stream));
        if (c->tileOwners.size() != tilesN || !c->tileOwnersExplicit) {
            c->tileOwners.assign(tilesN, 0);
            c->tileOwnersExplicit = false;
            if (tile_layout(c->tilesX, c->tilesY, N, nullptr, 0u, c->tileOwners.data()) != CHORDVIS_OK) return fail(c, CHORDVIS_E_INVALID, "tile layout");
        }
        const size_t slots = (size_t)N * c->slotCapacity;
        if ((rc = dalloc(c, &c->dHzbExchange, slots * CHORD_HZB_SLOT_HALVES))) return rc;
        CHORD_HIP(c, hipMemsetAsync(c->dHzbExchange, 0, slots * CHORD_HZB_SLOT_HALVES * 2, c->stream));
        if ((rc = dalloc(c, &c->dHzbFinalExchange, slots * CHORD_HZB_FINAL_SLOT_HALVES))) return rc;
        CHORD_HIP(c, hipMemsetAsync(c->dHzbFinalExchange, 0, slots * CHORD_HZB_FINAL_SLOT_HALVES * 2, c->stream));
        if ((rc = install_tile_owners(c))) return rc;
        if ((rc = prepare_cull_exchange(c))) return rc;
    } else {
        dfree(c->dHzbExchange); dfree(c->dHzbFinalExchange); dfree(c->dShardTables); dfree(c->dTileLoads); dfree(c->dTileOwner); dfree(c->dCullExchange);
        c->shard.ownedRows = nullptr; c->shard.tileSlot = nullptr;
        c->hzbExchangeHalves = c->hzbExchangeChunkHalves = 0; c->hzbFinalExchangeChunkBytes = 0;
    }
    // (a second pair of visibility buffers is made by chordvis_swap_visibility when a pipelined host first asks for it)
    dfree(c->dVisAlt); dfree(c->dVisResolvedAlt);
    return CHORDVIS_OK;
}

HzbBuffers from_handle(const ChordHZB* h)
{
    HzbBuffers b;
    b.desc = h->desc; b.minTexels = h->minTexels; b.maxTexels = h->maxTexels; b.validRange = h->validRange;
    b.valid = h->minTexels != nullptr;
    return b;
}

CmdList from_handle(const ChordCountAndCmd& h)
{
    CmdList l; l.count = h.count; l.cmds = h.cmds; l.capacity = h.capacity; return l;
}

int ready(ChordCtx* c, const char* fn)
{
    if (!c) return CHORDVIS_E_INVALID;
    if (!c->sceneLoaded || !c->viewSet || !c->dVis) {
        char buf[160];
        std::snprintf(buf, sizeof(buf), "%s: upload_scene, allocate_gbuffer and set_view must come first", fn);
        return fail(c, CHORDVIS_E_INVALID, buf);
    }
    if (!chord::view_fits_target(c)) {
        // (chordvis_set_view holds a view to the target it meets; chordvis_allocate_gbuffer may have come after it)
        char buf[224];
        std::snprintf(buf, sizeof(buf), "%s: the view's renderDimension differs from the allocated gbuffer (chordvis_set_view must follow a chordvis_allocate_gbuffer of another size)", fn);
        return fail(c, CHORDVIS_E_INVALID, buf);
    }
    return CHORDVIS_OK;
}

// addClearGbufferPass inside a frame: the visibility words are not memset; the first raster pass of the
// frame starts every 64x64 tile from zero in LDS and writes every tile back, which is the clear.
// passes other than instance_culling that run before it in a frame still need the constants on the device
int flush_view(ChordCtx* c)
{
    if (c->viewDirty) {
        CHORD_HIP(c, hipMemcpyAsync(c->dView, &c->hView, sizeof(DView), hipMemcpyHostToDevice, c->stream));
        c->viewDirty = false;
    }
    if (c->zeroFrameStateInCull) {
        CHORD_HIP(c, hipMemsetAsync(c->dFrameState, 0, c->frameStateZeroBytes, c->stream));
        c->zeroFrameStateInCull = false;
    }
    return CHORDVIS_OK;
}

// The tail of the last fused frame's history HZB (mips 6.. + valid range) normally rides on the next frame's first
// kernel; anything else that is about to read that chain launches it now.
int flush_pending_tail(ChordCtx* c)
{
    if (c->pendingTailSlot) {
        launch_hzb_tail(c, c->hzb[c->pendingTailSlot], true, true);
        c->pendingTailSlot = 0;
        CHORD_HIP(c, hipGetLastError());
    }
    return CHORDVIS_OK;
}

int begin_frame_clear(ChordCtx* c)
{
    // counters, the four command-list counts and both passes' tile bin counts: zeroed by the frame's first
    // kernel (object_cull), not by a separate memset
    c->frameStateZeroBytes = offsetof(FrameState, tileCount) + sizeof(uint32_t) * CHORD_TILECOUNT_STRIDE * ((size_t)2 * c->tilesX * c->tilesY);
    c->zeroFrameStateInCull = true;
    c->rasterCalls = 0;
    c->pendingClear = true;
    c->inFrame = true;
    return CHORDVIS_OK;
}

int do_raster(ChordCtx* c, const CmdList& in)
{
    // renderMesh (mesh_raster.cpp:208-254): the four (alphaMode x twoSided) pipeline buckets and
    // their filter passes collapse into one launch; the kernels read bTwoSided and alphaMode per cluster (masked
    // triangles carry their texture coordinates and are alpha-tested per pixel; blended materials draw nothing).
    const hipError_t e = launch_raster(c, in, c->pendingClear);
    c->pendingClear = false;
    if (e != hipSuccess) return fail(c, CHORDVIS_E_HIP, "launch_raster", e);
    CHORD_HIP(c, hipGetLastError());
    c->resolveFrame = true; c->resolveStale = false;   // the image now holds ids of this frame's objects and view (chordvis_resolve_attributes)
    return CHORDVIS_OK;
}

} // namespace

namespace chord {
void stamp(ChordCtx* c, int tag)
{
    if (!c->timers || !c->stampThisFrame) return;
    const size_t i = c->stampTags.size();
    if (i >= c->evPool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        c->evPool.push_back(e);
    }
    (void)hipEventRecord(c->evPool[i], c->stream);
    c->stampTags.push_back(tag);
}
}

namespace chord {
// c->tileOwners (host, the same on every rank) -> the two device tables the kernels read: this rank's tiles as one bit mask per
// tile row, and every tile's slot in the rank-major buffers (owner * slotsPerRank + index among the owner's tiles, by tile index).
int install_tile_owners(ChordCtx* c)
{
    const uint32_t N = c->shard.ranks, tiles = c->tilesX * c->tilesY;
    if (N <= 1 || !c->dShardTables || c->tileOwners.size() != tiles) return fail(c, CHORDVIS_E_INVALID, "tile owners: no sharded G-buffer");
    std::vector<uint32_t> used(N, 0);
    for (uint32_t t = 0; t < tiles; t++) {
        const uint32_t o = c->tileOwners[t];
        if (o >= N || ++used[o] > c->slotCapacity) return fail(c, CHORDVIS_E_INVALID, "tile owners: an owner out of range, or a rank with more tiles than chordvis_tile_slot_capacity");
    }
    // a rank's chunk: as many slots as the largest rank owns (every all-gather moves ranks x S slots)
    const uint32_t S = *std::max_element(used.begin(), used.end());
    std::vector<unsigned long long> tab(64 + (tiles + 1) / 2, 0ull);
    uint32_t* slot = reinterpret_cast<uint32_t*>(tab.data() + 64);
    std::fill(used.begin(), used.end(), 0u);
    for (uint32_t t = 0; t < tiles; t++) {
        const uint32_t o = c->tileOwners[t];
        slot[t] = o * S + used[o]++;
        if (o == c->shard.rank) tab[t / c->tilesX] |= 1ull << (t % c->tilesX);
    }
    c->shard.slotsPerRank = S;
    c->hzbExchangeChunkHalves = (uint64_t)S * CHORD_HZB_SLOT_HALVES;
    c->hzbExchangeHalves = c->hzbExchangeChunkHalves * N;
    c->hzbFinalExchangeChunkBytes = (uint64_t)S * CHORD_HZB_FINAL_SLOT_HALVES * 2;
    // (stream-ordered behind whatever still reads the old tables; the staging vector is pageable, so the call returns after the copy)
    CHORD_HIP(c, hipMemcpyAsync(c->dShardTables, tab.data(), tab.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    c->shard.ownedRows = c->dShardTables;
    c->shard.tileSlot = reinterpret_cast<const uint32_t*>(c->dShardTables + 64);
    // the owners themselves, one byte per tile: what the sharded cull makes its rank masks from (kernels_cull.hip cluster_rank_mask)
    if (c->dTileOwner) { (void)hipFree(c->dTileOwner); c->dTileOwner = nullptr; }
    CHORD_HIP(c, hipMalloc((void**)&c->dTileOwner, tiles));
    CHORD_HIP(c, hipMemcpy(c->dTileOwner, c->tileOwners.data(), tiles, hipMemcpyHostToDevice));
    c->mineValid = false; c->listMine[1] = c->listMine[2] = false;       // (lists culled for another ownership)
    c->orderAge = c->orderAge1 = 0xFFFFFFFFu;                                            // (a kept tile schedule lists the OLD map's tiles)
    return CHORDVIS_OK;
}

// The exchange buffer of the sharded group cull: ranks x (chunkBlocks x 256 mask words + chunkBlocks triangle sums), chunkBlocks =
// ceil(count blocks / ranks) -- the same on every rank of a frame (same scene, same rank count).
int ensure_cull_exchange(ChordCtx* c)
{
    if (!c->sceneLoaded || c->shard.ranks <= 1 || c->shard.ranks > 8u) return fail(c, CHORDVIS_E_INVALID, "cull exchange: a scene on a context sharded over 2..8 ranks");
    const uint32_t N = c->shard.ranks, chunkBlocks = (c->cullBlocks + N - 1u) / N;
    if (c->dCullExchange && c->cullChunkBlocks == chunkBlocks && c->cullExchangeRanks == N) return CHORDVIS_OK;
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    if (c->dCullExchange) { (void)hipFree(c->dCullExchange); c->dCullExchange = nullptr; }
    const size_t words = (size_t)N * chunkBlocks * 257u;
    CHORD_HIP(c, hipMalloc((void**)&c->dCullExchange, words * 4u));
    CHORD_HIP(c, hipMemsetAsync(c->dCullExchange, 0, words * 4u, c->stream));
    c->cullChunkBlocks = chunkBlocks; c->cullExchangeRanks = N;
    return CHORDVIS_OK;
}

// The exchange buffer is made when the LAST of {upload_scene, set_shard / allocate_gbuffer} has run, not inside a frame: whether a
// frame starts with the sharded cull -- i.e. whether its first collective happens -- must follow from state every rank shares
// (cull_shardable), never from an allocation that can fail on one rank while its peers are already inside the all-gather.  A failure
// here is the failure of a set-up call.
int prepare_cull_exchange(ChordCtx* c)
{
    if (!c->sceneLoaded || c->shard.ranks <= 1 || c->shard.ranks > 8u) return CHORDVIS_OK;
    return ensure_cull_exchange(c);
}

// Per-context work buffers that depend on the scene's counts (object frames, group masks, command lists, raster work
// lists): the tail of chordvis_upload_scene, shared with the depth-view child context (depth_views.cpp).
int alloc_scene_work_buffers(ChordCtx* c)
{
    int rc;
    if ((rc = dalloc(c, &c->dObjectsOwned, (size_t)c->objectCount))) return rc;
    if ((rc = dalloc(c, &c->dObjFrame, (size_t)c->objectCount))) return rc;
    if ((rc = dalloc(c, &c->dGroupMask, (size_t)c->groupInstances + 16))) return rc;   // (+16: zeroed in 16-byte vectors)
    if ((rc = dalloc(c, &c->dBlockCounts, (size_t)c->cullBlocks * 3))) return rc;   // counts, triangles, the rank's own counts (sharded), per count block
    c->fullListStale = false;          // (no cull of this scene has written the masks / block counts launch_full_list replays)
    for (int i = 0; i < 3; i++) {
        if ((rc = dalloc(c, &c->lists[i].cmds, (size_t)c->cmdCapacity))) return rc;
        c->lists[i].count = c->dCounts + i;
        c->lists[i].capacity = c->cmdCapacity;
    }
    scene_work_caps(c);
    if ((rc = dalloc(c, &c->dTris, (size_t)c->triCap))) return rc;
    if ((rc = dalloc(c, &c->dTrisC, (size_t)c->triCapC))) return rc;
    if ((rc = dalloc(c, &c->dBlockPool, (size_t)c->blockCap * CHORD_LIST_SHARDS * 2u))) return rc;
    if ((rc = dalloc(c, &c->dClipTris, (size_t)c->clipTriCap))) return rc;
    if ((rc = dalloc(c, &c->dLargeList, (size_t)c->largeCap))) return rc;
    // (what the buffers hold: the list's own counts here; chordvis_set_object_list grows them)
    c->allocObjects = std::max<size_t>(c->objectCount, 1); c->allocGroupInst = std::max<size_t>(c->groupInstances, 1);
    c->allocCullBlocks = c->cullBlocks; c->allocCmds = c->cmdCapacity;
    c->allocTris = c->triCap; c->allocTrisC = c->triCapC; c->allocBlocks = c->blockCap;
    return CHORDVIS_OK;
}

// The capacities the raster kernels see, from the list's triangles and the limits: the same for an uploaded list and for one set by
// chordvis_set_object_list, whatever the buffers hold.
void scene_work_caps(ChordCtx* c)
{
    const uint64_t instTriangles = c->instTriangles;
    // raster work lists, sized from the scene like the reference sizes its command buffers from lod0MeshletCount
    // (instance_culling.cpp:141): a triangle instance is set up at most once per frame (stage 0 or stage 1), so the
    // records of a frame never exceed the triangles of every meshlet instance (all LODs) plus the pieces the clipper
    // adds; chordvis_set_limits caps (or, for scenes beyond the default cap, raises) the budget.  Exhaustion is
    // detected on the device and reported by chordvis_stats.  Nearly all triangles take the 32-byte form; the 48-byte
    // list (triangles wider than 64 px, clipped pieces) gets the same bound up to a quarter of the limit.
    // (x2 + 256 Ki: the list is cut into 64 shards that fill unevenly, and a clipped triangle becomes several records)
    const uint64_t need = (2 * instTriangles + (256u << 10) + CHORD_LIST_SHARDS - 1) & ~(uint64_t)(CHORD_LIST_SHARDS - 1);
    c->triCapC = (uint32_t)std::min<uint64_t>(c->limitRecords, need);
    c->triCap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(c->limitRecords / 4, 1u << 20), need) & ~(CHORD_LIST_SHARDS - 1u);
    c->clipTriCap = 1u << 20;
    // pixel blocks of small clusters: a cluster takes the block form only when that is fewer bytes than its records would
    // be, so the compact list's byte budget bounds the pool too
    c->blockCap = (uint32_t)std::min<uint64_t>((uint64_t)c->triCapC * 2u / CHORD_LIST_SHARDS, CHORD_REC_INDEX_MASK / CHORD_LIST_SHARDS);
    c->largeCap = 8u << 20;
}
}

extern "C" {

// ------------------------------------------------------------------------------------ context --

int chordvis_create(int deviceOrdinal, void* hipStream, ChordCtx** outCtx)
{
    if (!outCtx) return CHORDVIS_E_INVALID;
    *outCtx = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || deviceOrdinal < 0 || deviceOrdinal >= n) return CHORDVIS_E_NO_DEVICE;
    ChordCtx* c = new ChordCtx();
    c->device = deviceOrdinal;
    if (hipSetDevice(deviceOrdinal) != hipSuccess) { delete c; return CHORDVIS_E_NO_DEVICE; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, deviceOrdinal) == hipSuccess) c->numCUs = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (hipStream) { c->stream = (hipStream_t)hipStream; c->ownStream = false; }
    else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return CHORDVIS_E_HIP; }
        c->ownStream = true;
    }
    bool ok = hipMalloc((void**)&c->dTileClocks, sizeof(unsigned long long) * 18 * CHORD_MAX_TILES) == hipSuccess &&
              hipMalloc((void**)&c->dHotTiles, sizeof(uint32_t) * 2 * (1 + CHORD_HOT_TILES)) == hipSuccess &&
              hipMemset(c->dHotTiles, 0, sizeof(uint32_t) * 2 * (1 + CHORD_HOT_TILES)) == hipSuccess &&
              hipMalloc((void**)&c->dView, sizeof(DView)) == hipSuccess &&
              hipMalloc((void**)&c->dFrameState, sizeof(FrameState)) == hipSuccess;
    if (!ok) { chordvis_destroy(c); return CHORDVIS_E_HIP; }
    c->dCounters = &c->dFrameState->counters;
    c->dCounts = c->dFrameState->listCounts;
    (void)hipMemsetAsync(c->dFrameState, 0, sizeof(FrameState), c->stream);
    *outCtx = c;
    return CHORDVIS_OK;
}

int chordvis_destroy(ChordCtx* c)
{
    if (!c) return CHORDVIS_E_INVALID;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    (void)chordvis_comm_destroy(c);
    free_retired(c);
    if (c->depthCtx) { chordvis_destroy(c->depthCtx); c->depthCtx = nullptr; }
    for (float*& d : c->dDepthImages) dfree(d);
    if (c->sharedScene) {       // a depth-view child: the scene buffers are the parent's
        c->dPrims = nullptr; c->dGroups = nullptr; c->dMeshlets = nullptr; c->dGroupIndices = nullptr; c->dMeshletData = nullptr;
        c->dPositions = nullptr; c->dObjStatic = nullptr; c->dGroupRefs = nullptr; c->dMaterials = nullptr; c->dTexAlpha = nullptr;
        c->dTexcoords = nullptr; c->dBvhNodes = nullptr; c->dMeshletLod = nullptr; c->dNormals = nullptr; c->dTangents = nullptr;
        c->dMatRecords = nullptr; c->dMatTexels = nullptr; c->dMatBlocks = nullptr;
    }
    dfree(c->dPrims); dfree(c->dGroups); dfree(c->dMeshlets); dfree(c->dGroupIndices); dfree(c->dMeshletData);
    dfree(c->dPositions); dfree(c->dObjStatic); dfree(c->dMaterials); dfree(c->dTexAlpha); dfree(c->dTexcoords); dfree(c->dBvhNodes); dfree(c->dGroupRefs); dfree(c->dObjectsOwned); dfree(c->dMeshletLod); dfree(c->dPrimVertexBase); dfree(c->dPrimAssetMeshlets);
    dfree(c->dNormals); dfree(c->dTangents); dfree(c->dMatRecords); dfree(c->dMatTexels); dfree(c->dMatBlocks); dfree(c->dMatFeedback); dfree(c->dGeoFeedback); dfree(c->dBoundsScratch); dfree(c->dBoundsTilesScratch); dfree(c->dTexEncTables);
    dfree(c->dView); dfree(c->dObjFrame); dfree(c->dGroupMask); dfree(c->dBlockCounts);
    drop_world_transforms(c);
    drop_ray_scene(c);
    for (int i = 0; i < 3; i++) dfree(c->lists[i].cmds);
    dfree(c->dRankCmds); dfree(c->dLeftCmds); dfree(c->dMineCmds);
    dfree(c->dCullLookback);
    dfree(c->dFrameState); c->dCounts = nullptr; c->dCounters = nullptr; dfree(c->dTileClocks); dfree(c->dHotTiles); dfree(c->dTileOrder); dfree(c->dTileOrderKeep); dfree(c->dTileOrderKeep1); c->orderAge = c->orderAge1 = 0xFFFFFFFFu; dfree(c->dTileSlabs); dfree(c->dTileMarker); dfree(c->dShadingTiles);
    dfree(c->dVisOwned); dfree(c->dVisResolved);
    for (int i = 0; i < 3; i++) { dfree(c->hzb[i].minTexels); dfree(c->hzb[i].maxTexels); dfree(c->hzb[i].validRange); }
    if (c->hBinHint) { (void)hipHostFree(const_cast<uint32_t*>(c->hBinHint)); c->hBinHint = nullptr; c->dBinHint = nullptr; }
    dfree(c->dRangePartials); dfree(c->dTileRange); dfree(c->dHzbExchange); dfree(c->dHzbFinalExchange); dfree(c->dShardTables); dfree(c->dTileLoads); dfree(c->dTileOwner); dfree(c->dCullExchange); dfree(c->dVisAlt); dfree(c->dVisResolvedAlt); dfree(c->dTris); dfree(c->dTrisC); dfree(c->dBlockPool); dfree(c->dTileBins); dfree(c->dBinPool); dfree(c->dBinChunkTab);
    dfree(c->dClipTris); dfree(c->dLargeList);
    for (hipEvent_t e : c->evPool) (void)hipEventDestroy(e);
    if (c->ownStream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return CHORDVIS_OK;
}

const char* chordvis_last_error(ChordCtx* c) { return c ? c->lastError.c_str() : "null context"; }

int chordvis_sync(ChordCtx* c)
{
    if (!c) return CHORDVIS_E_INVALID;
    { const int rc = flush_pending_tail(c); if (rc) return rc; }
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    free_retired(c);                                      // (what chordvis_set_object_list dropped without waiting)
    return CHORDVIS_OK;
}

// -------------------------------------------------------------------------------------- scene --

static int upload_scene_impl(ChordCtx* c, const ChordSceneDesc* s);

// A refused upload leaves NO scene behind (include/chordvis.h): the host tables and device buffers are replaced one by one, so
// after a failure part of them may be the new scene's and part the old one's.
int chordvis_upload_scene(ChordCtx* c, const ChordSceneDesc* s)
{
    if (c && !c->sharedScene) {                          // (the world transforms are per scene upload, refused uploads included)
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        drop_world_transforms(c);
        drop_ray_scene(c);
        free_retired(c);
    }
    const int rc = upload_scene_impl(c, s);
    if (rc && c) {
        c->sceneLoaded = false;
        if (c->depthCtx) { chordvis_destroy(c->depthCtx); c->depthCtx = nullptr; }   // (it aliases scene buffers that may be gone)
        c->shadowHistoryValid = false;
        c->resolveFrame = false;
        c->historySlot = 0; c->pendingTailSlot = 0;
        c->fullListStale = false; c->mineValid = false; c->cullPhaseDone = false;
    }
    return rc;
}

static int upload_scene_impl(ChordCtx* c, const ChordSceneDesc* s)
{
    if (c) c->orderAge = c->orderAge1 = 0xFFFFFFFFu;                    // (the kept tile schedule of launch_raster is made again)

    if (!c || !s || !s->objects || !s->primitives || !s->materials || !s->assets || s->objectCount == 0)
        return fail(c, CHORDVIS_E_INVALID, "upload_scene: null or empty scene");
    CHORD_HIP(c, hipSetDevice(c->device));

    // asset bases
    std::vector<uint32_t> mB(s->assetCount + 1, 0), gB(s->assetCount + 1, 0), iB(s->assetCount + 1, 0), dB(s->assetCount + 1, 0), vB(s->assetCount + 1, 0);
    for (uint32_t a = 0; a < s->assetCount; a++) {
        const ChordAssetDesc& as = s->assets[a];
        if (!as.meshlets || !as.meshletGroups || !as.meshletGroupIndices || !as.meshletData || !as.positions)
            return fail(c, CHORDVIS_E_INVALID, "upload_scene: asset with null stream");
        mB[a + 1] = mB[a] + as.meshletCount; gB[a + 1] = gB[a] + as.meshletGroupCount;
        iB[a + 1] = iB[a] + as.meshletGroupIndexCount; dB[a + 1] = dB[a] + as.meshletDataCount; vB[a + 1] = vB[a] + as.vertexCount;
    }
    {
        // (the raster kernels form vertex index x 3 in 32 bits -- one full-rate instruction instead of a quarter-rate 64-bit
        // multiply per vertex fetch: 1.43 G vertices = 17 GB of positions per scene; the reference's ByteAddressBuffer offsets
        // are 32-bit BYTE offsets, a third of that)
        uint64_t verts = 0;
        for (uint32_t a = 0; a < s->assetCount; a++) verts += s->assets[a].vertexCount;
        if (verts > 0x55555555ull) return fail(c, CHORDVIS_E_INVALID, "upload_scene: more than 0x55555555 vertices in one scene");
    }
    const uint32_t nM = mB.back(), nG = gB.back(), nI = iB.back(), nD = dB.back(), nV = vB.back();
    std::vector<uint32_t> nB(s->assetCount + 1, 0);
    for (uint32_t a = 0; a < s->assetCount; a++) nB[a + 1] = nB[a] + (s->assets[a].bvhNodes ? s->assets[a].bvhNodeCount : 0u);
    std::vector<DBVHNode> bvh(nB.back());
    bool bvhComplete = nB.back() > 0;

    std::vector<DMeshlet> meshlets(nM);
    std::vector<uint8_t> meshletLod(nM);
    std::vector<DGroup> groups(nG);
    std::vector<uint32_t> gidx(nI), mdata(nD);
    std::vector<float> pos((size_t)nV * 3);
    for (uint32_t a = 0; a < s->assetCount; a++) {
        const ChordAssetDesc& as = s->assets[a];
        for (uint32_t i = 0; i < as.meshletCount; i++) {
            const ChordMeshlet& m = as.meshlets[i];
            DMeshlet& d = meshlets[mB[a] + i];
            std::memcpy(&d, &m, sizeof(ChordMeshlet));
            const uint32_t V = m.vertexTriangleCount & 0xFFu, T = (m.vertexTriangleCount >> 8) & 0xFFu;
            if (T > CHORD_MESHLET_MAX_TRIANGLES || (uint64_t)m.dataOffset + V + T > as.meshletDataCount)
                return fail(c, CHORDVIS_E_INVALID, "upload_scene: meshlet exceeds 255 vertices / 128 triangles or its data stream");
            for (uint32_t t = 0; t < T; t++) {                      // local vertex indices of every triangle word
                const uint32_t w = as.meshletData[m.dataOffset + V + t];
                if ((w & 0xFFu) >= V || ((w >> 8) & 0xFFu) >= V || ((w >> 16) & 0xFFu) >= V)
                    return fail(c, CHORDVIS_E_INVALID, "upload_scene: triangle references a vertex beyond the meshlet's vertex count");
            }
            d.dataOffset = m.dataOffset + dB[a];
            d.vertexBase = 0xFFFFFFFFu;
            meshletLod[mB[a] + i] = (uint8_t)std::min(m.lod, 255u);   // (the resolve's debug view clamps to the 12-entry palette)
        }
        for (uint32_t i = 0; i < as.meshletGroupCount; i++) {
            const ChordMeshletGroup& g = as.meshletGroups[i];
            DGroup& d = groups[gB[a] + i];
            std::memcpy(&d, &g, sizeof(ChordMeshletGroup));
            d.pad0 = d.pad1 = 0;
            if (g.meshletCount > CHORD_GROUP_MAX_MESHLETS) return fail(c, CHORDVIS_E_INVALID, "upload_scene: group with more than 4 meshlets (nanite_builder.cpp:411-415)");
        }
        std::memcpy(gidx.data() + iB[a], as.meshletGroupIndices, sizeof(uint32_t) * as.meshletGroupIndexCount);
        std::memcpy(mdata.data() + dB[a], as.meshletData, sizeof(uint32_t) * as.meshletDataCount);
        std::memcpy(pos.data() + (size_t)vB[a] * 3, as.positions, sizeof(float) * 3 * as.vertexCount);
    }

    // primitives
    c->hPrims.assign(s->primitiveCount, DPrim{});
    std::vector<uint32_t> primMeshlets(s->primitiveCount, 0);
    std::vector<uint64_t> primTriangles(s->primitiveCount, 0);
    std::vector<uint32_t> primVertexBase(s->primitiveCount, 0);   // asset vertex base + primitive.vertexOffset (chordvis_shade_ray_hits)
    std::vector<uint2> primAssetMeshlets(s->primitiveCount, make_uint2(0u, 0u));   // (first meshlet, meshlet count) of the primitive's asset (the same call)
    for (uint32_t pi = 0; pi < s->primitiveCount; pi++) {
        const ChordPrimitive& p = s->primitives[pi];
        if (p.primitiveDatasBufferId >= s->assetCount) return fail(c, CHORDVIS_E_INVALID, "upload_scene: primitiveDatasBufferId out of range");
        const uint32_t a = p.primitiveDatasBufferId;
        const ChordAssetDesc& as = s->assets[a];
        // (every range of a primitive is held to its OWN asset's counts, in 64 bits: one past an asset's stream is still inside the
        // concatenation, and an offset near 2^32 must not wrap back into range)
        if ((uint64_t)p.meshletGroupOffset + p.meshletGroupCount > as.meshletGroupCount) return fail(c, CHORDVIS_E_INVALID, "upload_scene: primitive group range out of bounds");
        DPrim& d = c->hPrims[pi];
        std::memcpy(d.posMin, p.posMin, 12); std::memcpy(d.posMax, p.posMax, 12);
        d.meshletBase = mB[a] + p.meshletOffset;
        d.groupBase = gB[a] + p.meshletGroupOffset;
        d.groupIndicesBase = iB[a] + p.meshletGroupIndicesOffset;
        d.groupCount = p.meshletGroupCount;
        d.assetMeshletBase = mB[a];
        primVertexBase[pi] = vB[a] + p.vertexOffset;
        primAssetMeshlets[pi] = make_uint2(mB[a], as.meshletCount);
        d.bvhBase = 0xFFFFFFFFu;
        if (as.bvhNodes && as.bvhNodeCount && p.bvhNodeOffset < as.bvhNodeCount) {
            // GPUBVHNode tree of the primitive (gltf.h:16-24): copied, and checked for what the hierarchical cull relies on --
            // indices in range, every group of the primitive in exactly one node's leaf range, every non-root node's
            // sphere around the parent-error spheres of the groups beneath it
            const ChordBVHNode* nodes = as.bvhNodes + p.bvhNodeOffset;
            const uint32_t count = nodes[0].bvhNodeCount;
            if (count == 0 || (uint64_t)p.bvhNodeOffset + count > as.bvhNodeCount) return fail(c, CHORDVIS_E_INVALID, "upload_scene: BVH root's node count exceeds the node buffer");
            std::vector<uint8_t> seen(p.meshletGroupCount, 0);
            std::vector<std::vector<uint32_t>> below(count);    // parented groups of each node's subtree
            for (uint32_t n = count; n-- > 0;) {            // children come after their parent (breadth-first order)
                const ChordBVHNode& nd = nodes[n];
                if ((uint64_t)nd.leafMeshletGroupOffset + nd.leafMeshletGroupCount > p.meshletGroupCount) return fail(c, CHORDVIS_E_INVALID, "upload_scene: BVH leaf range outside the primitive's groups");
                for (uint32_t g = 0; g < nd.leafMeshletGroupCount; g++) {
                    const uint32_t gi = nd.leafMeshletGroupOffset + g;
                    if (seen[gi]++) return fail(c, CHORDVIS_E_INVALID, "upload_scene: a cluster group is listed by two BVH nodes");
                    const ChordMeshletGroup& gr = as.meshletGroups[p.meshletGroupOffset + gi];
                    if (n != 0) {
                        if (!(gr.parentError < CHORD_ERROR_RADIUS_ROOT)) return fail(c, CHORDVIS_E_INVALID, "upload_scene: an un-parented group below the BVH root");
                        below[n].push_back(gi);
                    }
                }
                for (uint32_t k = 0; k < CHORD_BVH_WIDTH; k++) {
                    const uint32_t ch = nd.children[k];
                    if (ch == CHORD_BVH_NO_CHILD) continue;
                    if (ch <= n || ch >= count) return fail(c, CHORDVIS_E_INVALID, "upload_scene: BVH child index out of order / range");
                    below[n].insert(below[n].end(), below[ch].begin(), below[ch].end());
                    std::vector<uint32_t>().swap(below[ch]);
                }
                // the sphere bounds the parent-error sphere of every group beneath (the root: beneath its children)
                for (uint32_t gi : below[n]) {
                    const ChordMeshletGroup& gr = as.meshletGroups[p.meshletGroupOffset + gi];
                    const float dx = gr.parentPosCenter[0] - nd.sphere[0], dy = gr.parentPosCenter[1] - nd.sphere[1], dz = gr.parentPosCenter[2] - nd.sphere[2];
                    if (!(std::sqrt(dx * dx + dy * dy + dz * dz) + gr.parentError <= nd.sphere[3] * 1.0001f + 1.0e-6f))
                        return fail(c, CHORDVIS_E_INVALID, "upload_scene: a BVH node's sphere does not contain the parent-error spheres beneath it");
                }
                DBVHNode& dn = bvh[nB[a] + p.bvhNodeOffset + n];
                std::memcpy(dn.sphere, nd.sphere, 16); std::memcpy(dn.children, nd.children, 32);
                dn.bvhNodeCount = nd.bvhNodeCount; dn.leafGroupOffset = nd.leafMeshletGroupOffset; dn.leafGroupCount = nd.leafMeshletGroupCount; dn.pad = 0;
            }
            for (uint32_t gi = 0; gi < p.meshletGroupCount; gi++) if (!seen[gi]) return fail(c, CHORDVIS_E_INVALID, "upload_scene: a cluster group is missing from the primitive's BVH");
            {   // breadth-first order: a level is a contiguous range; every node keeps the end of its level (DBVHNode::pad)
                std::vector<uint32_t> level(count, 0xFFFFFFFFu);
                level[0] = 0;
                for (uint32_t n = 0; n < count; n++) {
                    if (level[n] == 0xFFFFFFFFu) return fail(c, CHORDVIS_E_INVALID, "upload_scene: a BVH node is not reachable from the root");
                    for (uint32_t k = 0; k < CHORD_BVH_WIDTH; k++) {
                        const uint32_t ch = nodes[n].children[k];
                        if (ch == CHORD_BVH_NO_CHILD) continue;
                        if (level[ch] != 0xFFFFFFFFu) return fail(c, CHORDVIS_E_INVALID, "upload_scene: a BVH node has two parents");
                        level[ch] = level[n] + 1;
                    }
                    if (n && level[n] < level[n - 1]) return fail(c, CHORDVIS_E_INVALID, "upload_scene: BVH nodes are not in breadth-first order");
                    if (level[n] >= CHORD_BVH_MAX_LEVELS) return fail(c, CHORDVIS_E_INVALID, "upload_scene: BVH deeper than kNaniteMaxBVHLevelCount");
                }
                uint32_t end = count;
                for (uint32_t n = count; n-- > 0;) {
                    if (n + 1 < count && level[n + 1] != level[n]) end = n + 1;
                    bvh[nB[a] + p.bvhNodeOffset + n].pad = end;
                }
            }
            d.bvhBase = nB[a] + p.bvhNodeOffset;
        } else bvhComplete = false;
        for (uint32_t gi = 0; gi < p.meshletGroupCount; gi++) {
            const ChordMeshletGroup& g = as.meshletGroups[p.meshletGroupOffset + gi];
            for (uint32_t i = 0; i < g.meshletCount; i++) {
                const uint64_t ii = (uint64_t)p.meshletGroupIndicesOffset + g.meshletOffset + i;
                if (ii >= as.meshletGroupIndexCount) return fail(c, CHORDVIS_E_INVALID, "upload_scene: group index out of bounds");
                const uint64_t mi = (uint64_t)p.meshletOffset + as.meshletGroupIndices[ii];
                if (mi >= as.meshletCount) return fail(c, CHORDVIS_E_INVALID, "upload_scene: meshlet index out of bounds");
                DMeshlet& dm = meshlets[mB[a] + mi];
                if (dm.vertexBase == 0xFFFFFFFFu) {                  // first reference: check the vertex ids against the asset
                    const ChordMeshlet& sm = as.meshlets[mi];
                    const uint32_t V = sm.vertexTriangleCount & 0xFFu;
                    for (uint32_t v = 0; v < V; v++)
                        if ((uint64_t)p.vertexOffset + as.meshletData[sm.dataOffset + v] >= as.vertexCount)
                            return fail(c, CHORDVIS_E_INVALID, "upload_scene: meshlet vertex id out of the asset's position stream");
                }
                dm.vertexBase = vB[a] + p.vertexOffset;
                primMeshlets[pi]++;
                primTriangles[pi] += (as.meshlets[mi].vertexTriangleCount >> 8) & 0xFFu;
            }
        }
    }

    // objects (the per-primitive and per-material facts stay with the context: chordvis_set_object_list derives its lists from them)
    c->hPrimMeshlets = primMeshlets; c->hPrimTriangles = primTriangles;
    c->hMatFlags.assign(s->materialCount, 0u); c->hMatType.assign(s->materialCount, 0u);
    for (uint32_t m = 0; m < s->materialCount; m++) {
        const ChordMaterial& mat = s->materials[m];
        // alphaMode 0 / 1 / 2 = opaque / mask / blend (FILTER_CHECK of pipeline_filter.hlsl:100-101); anything else never
        // matches a bucket's targetAlphaMode and draws nothing, like blend
        c->hMatFlags[m] = (mat.bTwoSided != 0 ? CHORD_MATFLAG_TWO_SIDED : 0u) | ((mat.alphaMode > 2u ? 2u : mat.alphaMode) << 1);
        c->hMatType[m] = mat.materialType;
    }
    ObjectListTotals totals;
    { const int orc = derive_object_list(c, "upload_scene", s->objects, s->objectCount, c->hObjStatic, totals); if (orc) return orc; }
    const uint64_t groupInst = totals.groupInst, cmdCap = totals.cmdCap, instTriangles = totals.instTriangles;
    // the flattened (object, group) instances, every indirection of the group cull resolved (DGroupRef)
    std::vector<DGroupRef> refs((size_t)groupInst);
    for (uint32_t o = 0; o < s->objectCount; o++) {
        const DObjStatic& d = c->hObjStatic[o];
        const DPrim& pr = c->hPrims[d.prim];
        for (uint32_t gl = 0; gl < pr.groupCount; gl++) {
            const DGroup& g = groups[pr.groupBase + gl];
            DGroupRef& r = refs[(size_t)d.groupBase + gl];
            const uint32_t cnt = std::min(g.meshletCount, (uint32_t)CHORD_GROUP_MAX_MESHLETS);
            r.object = o;
            r.group = (pr.groupBase + gl) | (cnt << 28);
            for (uint32_t i = 0; i < CHORD_GROUP_MAX_MESHLETS; i++)
                r.meshlet[i] = cnt ? pr.meshletBase + gidx[pr.groupIndicesBase + g.meshletOffset + (i < cnt ? i : 0u)] : 0u;
        }
    }
    if (nG >= (1u << 28)) return fail(c, CHORDVIS_E_CAPACITY, "upload_scene: more than 2^28 cluster groups");

    dfree(c->dRankCmds);                                   // sized by cmdCapacity; re-made by the first sharded raster pass
    dfree(c->dLeftCmds); dfree(c->dMineCmds);
    c->mineValid = false; c->listMine[1] = c->listMine[2] = false;       // (the rank's lists went with the buffers)
    c->fullListStale = false; c->cullPhaseDone = false;                    // (the masks of the old scene's last cull are gone: nothing to replay)
    dfree(c->dCullExchange);                                               // (sized by the scene's count blocks: re-made on demand)
    c->objectCount = s->objectCount; c->primCount = s->primitiveCount; c->materialCount = s->materialCount;
    c->meshletCount = nM; c->groupCount = nG;
    c->groupIndexWords = nI; c->meshletDataWords = nD; c->vertexTotal = nV;     // (what chordvis_build_ray_scene reads back)
    c->groupInstances = (uint32_t)groupInst; c->cmdCapacity = (uint32_t)std::max<uint64_t>(cmdCap, 1);
    c->cullBlocks = std::max(1u, (c->groupInstances + 255u) / 256u);

    // what the masked buckets sample: alpha channels of every texture level, materials with texture + sampler resolved,
    // the per-vertex texture coordinates (mesh_raster.hlsl:107-112,198-204)
    std::vector<DMaterial> dmats(s->materialCount);
    // (the alpha of an RGBA8 texture is picked out on the host, per texture; a block-compressed one is expanded on the device)
    struct AlphaCopy { size_t base; std::vector<uint8_t> bytes; const uint8_t* rgba8; size_t texels; };
    std::vector<AlphaCopy> alphaCopies;
    std::vector<std::pair<size_t, size_t>> alphaOpaque;                    // (first byte, bytes) of BC1_RGB / BC4 / BC5 chains: 255 throughout
    TexDecodeJob alphaDecode;                                              // BC3 chains: their alpha blocks
    TexMipJob alphaMips;                                                   // chordvis_set_texture_mips: the levels made here
    size_t alphaTexels = 0;
    std::vector<uint32_t> texOffset(s->textureCount, 0xFFFFFFFFu), texLevels(s->textureCount, 0u);
    bool anyMasked = false;
    for (uint32_t m = 0; m < s->materialCount; m++) anyMasked = anyMasked || s->materials[m].alphaMode == CHORD_ALPHA_MASK;
    if (anyMasked && s->textures) {
        // only the textures an alpha-tested material samples are looked at (a host may hand over its whole bindless table, with
        // pixel data only where the visibility pass needs it); every other entry stays "white"
        std::vector<uint8_t> sampled(s->textureCount, 0);
        for (uint32_t m = 0; m < s->materialCount; m++)
            if (s->materials[m].alphaMode == CHORD_ALPHA_MASK && s->materials[m].baseColorId < s->textureCount) sampled[s->materials[m].baseColorId] = 1;
        for (uint32_t t = 0; t < s->textureCount; t++) {
            if (!sampled[t]) continue;
            const ChordTexture& tx = s->textures[t];
            if (tx.format != CHORD_TEXFMT_RGBA8 && !tex_block_bytes(tx.format))
                return fail(c, CHORDVIS_E_INVALID, "upload_scene: unknown ChordTexture::format on a texture a masked material samples; allowed: " CHORD_TEXFMT_NAMES);
            if (!tx.rgba8 || tx.width == 0 || tx.height == 0 || tx.mipCount == 0 || tx.width > 16384u || tx.height > 16384u || tx.mipCount > 15u)
                return fail(c, CHORDVIS_E_INVALID, "upload_scene: texture without data, or larger than 16384 / 15 levels");
            ChordTextureMips ms;
            const uint32_t L = tex_levels(c, t, tx, ms);                   // (>= mipCount; the levels beyond it are made on the device)
            const size_t texels = tex_chain_texels(tx.width, tx.height, L), supplied = tex_chain_texels(tx.width, tx.height, tx.mipCount);
            if (alphaTexels + texels >= 0xFFFFFFFFull) return fail(c, CHORDVIS_E_CAPACITY, "upload_scene: more than 4 G texels of alpha");
            texOffset[t] = (uint32_t)alphaTexels; texLevels[t] = L;
            const size_t base = alphaTexels;
            alphaTexels += texels;
            if (tx.format != CHORD_TEXFMT_RGBA8 && tx.format != CHORD_TEXFMT_BC3) { alphaOpaque.push_back({base, texels}); continue; }
            if (tx.format == CHORD_TEXFMT_BC3) alphaDecode.add(tx, (uint32_t)base);
            else alphaCopies.push_back(AlphaCopy{base, std::vector<uint8_t>(), tx.rgba8, supplied});
            alphaMips.add((uint32_t)base, tx.width, tx.height, tx.mipCount, L, ms, (ms.flags & CHORD_TEXMIPS_COVERAGE) != 0u);
        }
        for (AlphaCopy& a : alphaCopies) {                                 // (once the whole table is known to fit: no texel is read before)
            a.bytes.resize(a.texels);
            for (size_t i = 0; i < a.texels; i++) a.bytes[i] = a.rgba8[i * 4 + 3];
        }
    }
    for (uint32_t m = 0; m < s->materialCount; m++) {
        const ChordMaterial& mat = s->materials[m];
        DMaterial& d = dmats[m];
        std::memset(&d, 0, sizeof(d));
        d.texOffset = 0xFFFFFFFFu;
        if (s->textures && mat.baseColorId < s->textureCount && texOffset[mat.baseColorId] != 0xFFFFFFFFu) {
            const ChordTexture& tx = s->textures[mat.baseColorId];
            d.texOffset = texOffset[mat.baseColorId]; d.texWidth = tx.width; d.texHeight = tx.height; d.texMips = texLevels[mat.baseColorId];
        }
        if (s->samplers && mat.baseColorSampler < s->samplerCount) {
            const ChordSampler& sm = s->samplers[mat.baseColorSampler];
            d.minFilter = sm.minFilter; d.magFilter = sm.magFilter; d.wrapS = sm.wrapS; d.wrapT = sm.wrapT;
        } else { d.minFilter = d.magFilter = CHORD_FILTER_NEAREST; d.wrapS = d.wrapT = CHORD_WRAP_REPEAT; }
        d.alphaFactor = mat.baseColorFactor[3]; d.alphaCutOff = mat.alphaCutOff;
        // every level as the tile kernel's row units want it (DMatLevel)
        if (d.texOffset != 0xFFFFFFFFu) {
            uint32_t off = d.texOffset;
            auto wrap_consts = [](uint32_t n, uint32_t mode, uint32_t& magic, uint32_t& bias) {
                magic = 0u; bias = 0u;
                if (mode == CHORD_WRAP_CLAMP_TO_EDGE) return;
                const uint32_t period = mode == CHORD_WRAP_MIRRORED_REPEAT ? 2u * n : n;
                if ((period & (period - 1u)) == 0u) return;                  // masked, not divided
                magic = (uint32_t)(0x100000000ull / period);
                bias = (uint32_t)(((0x40000000ull + period - 1u) / period) * period);
            };
            for (uint32_t l = 0; l < d.texMips && l < CHORD_MAX_TEX_LEVELS; l++) {
                const uint32_t w = std::max(1u, d.texWidth >> l), h = std::max(1u, d.texHeight >> l);
                chord::DMatLevel& L = d.levels[l];
                L.base = off; L.dims = (w - 1u) | (h - 1u) << 16;
                wrap_consts(w, d.wrapS, L.magicS, L.biasS);
                wrap_consts(h, d.wrapT, L.magicT, L.biasT);
                off += w * h;
            }
        }
    }
    // texture coordinates: the masked buckets sample with them, chordvis_resolve_attributes interpolates them.  A scene without
    // masked materials whose streams do not match its vertex counts was accepted before the resolve existed: it still is, without uvs.
    std::vector<float> uvs;
    bool uvsUsable = true;
    for (uint32_t a = 0; a < s->assetCount; a++)
        if (s->assets[a].texcoord0 && s->assets[a].texcoord0Count && s->assets[a].texcoord0Count != s->assets[a].vertexCount) uvsUsable = false;
    if (anyMasked || uvsUsable) {
        bool anyUv = false;
        for (uint32_t a = 0; a < s->assetCount; a++) anyUv = anyUv || (s->assets[a].texcoord0 && s->assets[a].texcoord0Count);
        if (anyUv) {
            uvs.assign((size_t)nV * 2, 0.0f);
            for (uint32_t a = 0; a < s->assetCount; a++) {
                const ChordAssetDesc& as = s->assets[a];
                if (as.texcoord0 && as.texcoord0Count) {
                    // (a shorter array would silently read as uv = (0, 0) for the vertices beyond it)
                    if (as.texcoord0Count != as.vertexCount) return fail(c, CHORDVIS_E_INVALID, "upload_scene: texcoord0Count must equal vertexCount (or be 0: no texture coordinates)");
                    std::memcpy(uvs.data() + (size_t)vB[a] * 2, as.texcoord0, sizeof(float) * 2 * as.vertexCount);
                }
            }
        }
    }
    c->anyMasked = anyMasked;
    // normals (float3) and tangents (float4) per vertex: read by chordvis_resolve_surface alone.  Assets without a stream
    // contribute zeros; a scene where no asset has one allocates nothing for it.
    std::vector<float> nrm, tng;
    for (uint32_t a = 0; a < s->assetCount; a++) {
        const ChordAssetDesc& as = s->assets[a];
        if ((as.normals && as.normalCount && as.normalCount != as.vertexCount) || (as.tangents && as.tangentCount && as.tangentCount != as.vertexCount))
            return fail(c, CHORDVIS_E_INVALID, "upload_scene: normalCount / tangentCount must equal vertexCount (or be 0: no such stream)");
        if (as.normals && as.normalCount) {
            if (nrm.empty()) nrm.assign((size_t)nV * 3, 0.0f);
            std::memcpy(nrm.data() + (size_t)vB[a] * 3, as.normals, sizeof(float) * 3 * as.vertexCount);
        }
        if (as.tangents && as.tangentCount) {
            if (tng.empty()) tng.assign((size_t)nV * 4, 0.0f);
            std::memcpy(tng.data() + (size_t)vB[a] * 4, as.tangents, sizeof(float) * 4 * as.vertexCount);
        }
    }

    int rc;
#define UP(dst, vec)                                                                                          \
    if ((rc = dalloc(c, &dst, vec.size()))) return rc;                                                        \
    if (!vec.empty()) CHORD_HIP(c, hipMemcpy(dst, vec.data(), vec.size() * sizeof(vec[0]), hipMemcpyHostToDevice));
    UP(c->dMeshlets, meshlets) UP(c->dGroups, groups) UP(c->dGroupIndices, gidx) UP(c->dMeshletData, mdata)
    UP(c->dPositions, pos) UP(c->dPrims, c->hPrims) UP(c->dObjStatic, c->hObjStatic) UP(c->dGroupRefs, refs)
    UP(c->dMaterials, dmats) UP(c->dMeshletLod, meshletLod) UP(c->dPrimVertexBase, primVertexBase) UP(c->dPrimAssetMeshlets, primAssetMeshlets)
    if (!bvh.empty()) { UP(c->dBvhNodes, bvh) } else dfree(c->dBvhNodes);
    c->bvhComplete = bvhComplete;
    if (alphaTexels) {
        if ((rc = dalloc(c, &c->dTexAlpha, alphaTexels))) return rc;
        for (const AlphaCopy& a : alphaCopies) CHORD_HIP(c, hipMemcpy(c->dTexAlpha + a.base, a.bytes.data(), a.bytes.size(), hipMemcpyHostToDevice));
        for (const auto& o : alphaOpaque) CHORD_HIP(c, hipMemsetAsync(c->dTexAlpha + o.first, 0xFF, o.second, c->stream));
        if ((rc = alphaDecode.run(c, "upload_scene: texture decode", nullptr, c->dTexAlpha, true))) return rc;
        if ((rc = alphaMips.run(c, "upload_scene: texture mips", nullptr, c->dTexAlpha, true))) return rc;
        if (!alphaOpaque.empty()) CHORD_HIP(c, hipStreamSynchronize(c->stream));
    } else dfree(c->dTexAlpha);
    if (!uvs.empty()) { UP(c->dTexcoords, uvs) } else dfree(c->dTexcoords);
    if (!nrm.empty()) { UP(c->dNormals, nrm) } else dfree(c->dNormals);
    if (!tng.empty()) { UP(c->dTangents, tng) } else dfree(c->dTangents);
#undef UP
    c->instTriangles = instTriangles;
    drop_material_textures(c);                                             // (chordvis_upload_material_textures is per scene upload)
    dfree(c->dGeoFeedback); c->geoFeedbackCmds = nullptr;                  // (chordvis_geometry_feedback's counts are per scene upload too)
    if (c->depthCtx) { chordvis_destroy(c->depthCtx); c->depthCtx = nullptr; }       // (it aliased the old scene buffers)
    if ((rc = chord::alloc_scene_work_buffers(c))) return rc;
    CHORD_HIP(c, hipMemcpy(c->dObjectsOwned, s->objects, sizeof(ChordObject) * s->objectCount, hipMemcpyHostToDevice));
    c->dObjects = c->dObjectsOwned;
    c->sceneLoaded = true;
    c->resolveFrame = false;
    c->historySlot = 0;
    c->pendingTailSlot = 0;
    if ((rc = chord::prepare_cull_exchange(c))) { c->sceneLoaded = false; return rc; }     // (a sharded context: the rank-mask exchange buffer of this scene)
    if (c->cullMode == 1 && !c->bvhComplete) return fail(c, CHORDVIS_E_INVALID, "upload_scene: hierarchical culling is selected and a primitive has no BVH");
    return CHORDVIS_OK;
}

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
    auto wrap_consts = [](uint32_t n, uint32_t mode, uint32_t& magic, uint32_t& bias) {   // (DMatLevel; as chordvis_upload_scene's)
        magic = 0u; bias = 0u;
        if (mode == CHORD_WRAP_CLAMP_TO_EDGE) return;
        const uint32_t period = mode == CHORD_WRAP_MIRRORED_REPEAT ? 2u * n : n;
        if ((period & (period - 1u)) == 0u) return;
        magic = (uint32_t)(0x100000000ull / period);
        bias = (uint32_t)(((0x40000000ull + period - 1u) / period) * period);
    };
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
                wrap_consts(w, S.wrapS, L.magicS, L.biasS);
                wrap_consts(h, S.wrapT, L.magicT, L.biasT);
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
        uint32_t* dStage = nullptr;
        hipError_t e = hipMalloc((void**)&dStage, stageCount * 4u);
        for (uint32_t t = 0; t < nTex && e == hipSuccess; t++) {
            const ChordTexture& tx = s->textures[t];
            if (texStage[t] == 0xFFFFFFFFu || tx.format != CHORD_TEXFMT_RGBA8) continue;
            e = hipMemcpy(dStage + texStage[t], tx.rgba8, tex_chain_texels(tx.width, tx.height, tx.mipCount) * 4u, hipMemcpyHostToDevice);
        }
        rc = e == hipSuccess ? CHORDVIS_OK : fail(c, CHORDVIS_E_HIP, "upload_material_textures: staging for compression", e);
        if (!rc) rc = stageDecode.run(c, "upload_material_textures: texture decode", dStage, nullptr, false);
        if (!rc) rc = stageMips.run(c, "upload_material_textures: texture mips", dStage, nullptr, false);
        if (!rc) rc = encode.run(c, "upload_material_textures: texture encode", dStage, c->dMatBlocks);
        for (size_t i = 0; i < trims.size() && !rc; i++) {
            e = hipMemcpy(c->dMatTexels + trims[i].dst, dStage + trims[i].src, trims[i].count * 4u, hipMemcpyDeviceToDevice);
            if (e != hipSuccess) rc = fail(c, CHORDVIS_E_HIP, "upload_material_textures: copy of the kept levels", e);
        }
        if (dStage) (void)hipFree(dStage);
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
        uint32_t* dOut = nullptr;
        chord::DTexLevelRec* dRecs = nullptr;
        hipError_t e = hipMalloc((void**)&dOut, count * 4);
        if (e == hipSuccess) e = hipMalloc((void**)&dRecs, sizeof(recs));
        if (e == hipSuccess) e = hipMemcpy(dRecs, recs, sizeof(recs), hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            chord::launch_texture_decode(c, dRecs, 1u, bw * bh, c->dMatBlocks, dOut, nullptr, false);
            e = hipGetLastError();
            const hipError_t es = hipStreamSynchronize(c->stream);
            if (e == hipSuccess) e = es;
        }
        if (e == hipSuccess) e = hipMemcpy(hostRgba8, dOut, count * 4, hipMemcpyDeviceToHost);
        if (dOut) (void)hipFree(dOut);
        if (dRecs) (void)hipFree(dRecs);
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

int chordvis_update_objects(ChordCtx* c, const ChordObject* hostObjects, uint32_t count)
{
    if (!c || !c->sceneLoaded || !hostObjects || count != c->objectCount) return fail(c, CHORDVIS_E_INVALID, "update_objects: count must equal the uploaded scene's objectCount");
    CHORD_HIP(c, hipMemcpyAsync(c->dObjectsOwned, hostObjects, sizeof(ChordObject) * count, hipMemcpyHostToDevice, c->stream));
    c->dObjects = c->dObjectsOwned;
    c->resolveStale = true;
    c->rayRefitDue = true;
    return CHORDVIS_OK;
}

int chordvis_bind_objects(ChordCtx* c, const ChordObject* deviceObjects, uint32_t count)
{
    if (!c || !c->sceneLoaded || !deviceObjects || count != c->objectCount) return fail(c, CHORDVIS_E_INVALID, "bind_objects: count must equal the uploaded scene's objectCount");
    c->dObjects = deviceObjects;
    c->resolveStale = true;                               // (like chordvis_update_objects: the array a resolve would read is no longer the frame's)
    c->rayRefitDue = true;
    return CHORDVIS_OK;
}

// ---- the object list of a resident scene (include/chordvis.h OBJECTS COME AND GO; kernels_objects.hip) ----

// Everything is derived and checked before anything of the context is touched; the buffers a longer list needs are all made before
// the first old one is let go, so a refusal -- an allocation failure too -- leaves the context rendering the list it had.
int chordvis_set_object_list(ChordCtx* c, const ChordObject* hostObjects, uint32_t count)
{
    if (!c) return CHORDVIS_E_INVALID;
    if (c->sharedScene) return fail(c, CHORDVIS_E_INVALID, "set_object_list: not on a depth-view context");
    if (!c->sceneLoaded) return fail(c, CHORDVIS_E_INVALID, "set_object_list: no scene (call chordvis_upload_scene first)");
    if (!hostObjects || count == 0) return fail(c, CHORDVIS_E_INVALID, "set_object_list: count must be at least 1 (and hostObjects not NULL), as for chordvis_upload_scene");
    // (the rank masks on their way through the all-gather name the old list's group instances)
    if (c->cullPhaseDone) return fail(c, CHORDVIS_E_INVALID, "set_object_list: not between chordvis_frame_phase_cull and chordvis_frame_phase_a");
    std::vector<DObjStatic> stat;
    ObjectListTotals t;
    int rc = derive_object_list(c, "set_object_list", hostObjects, count, stat, t);
    if (rc) return rc;
    (void)hipSetDevice(c->device);

    // the logical counts and capacities of a fresh upload of this list (scene_work_caps reads instTriangles and the limits only)
    const uint32_t groupInstances = (uint32_t)t.groupInst, cmdCapacity = (uint32_t)std::max<uint64_t>(t.cmdCap, 1);
    const uint32_t cullBlocks = std::max(1u, (groupInstances + 255u) / 256u);
    ChordCtx caps;                                       // (a scratch record for the five capacities: no device state)
    caps.instTriangles = t.instTriangles; caps.limitRecords = c->limitRecords;
    chord::scene_work_caps(&caps);

    // grow what is too short: every new buffer first, then the old ones go
    struct Grow { void** slot; size_t bytes; void* fresh; };
    std::vector<Grow> grow;
    auto want = [&grow](auto*& p, size_t n) { grow.push_back(Grow{(void**)&p, std::max<size_t>(n, 1) * sizeof(*p), nullptr}); };
    const bool growObjects = count > c->allocObjects, growGroups = groupInstances > c->allocGroupInst, growBlocks = cullBlocks > c->allocCullBlocks;
    const bool growCmds = cmdCapacity > c->allocCmds, growTris = caps.triCap > c->allocTris, growTrisC = caps.triCapC > c->allocTrisC;
    const bool growPool = caps.blockCap > c->allocBlocks;
    if (growObjects) { want(c->dObjectsOwned, count); want(c->dObjFrame, count); want(c->dObjStatic, count); }
    if (growGroups) { want(c->dGroupRefs, groupInstances); want(c->dGroupMask, (size_t)groupInstances + 16); }
    if (growBlocks) want(c->dBlockCounts, (size_t)cullBlocks * 3);
    if (growCmds) for (int i = 0; i < 3; i++) want(c->lists[i].cmds, cmdCapacity);
    if (growTris) want(c->dTris, caps.triCap);
    if (growTrisC) want(c->dTrisC, caps.triCapC);
    if (growPool) want(c->dBlockPool, (size_t)caps.blockCap * CHORD_LIST_SHARDS * 2u);
    if (!grow.empty()) {
        for (Grow& g : grow) {
            const hipError_t e = hipMalloc(&g.fresh, g.bytes);
            if (e != hipSuccess) {
                for (Grow& u : grow) if (u.fresh) (void)hipFree(u.fresh);
                return fail(c, CHORDVIS_E_HIP, "set_object_list: hipMalloc of a buffer the longer list needs", e);
            }
        }
        CHORD_HIP(c, hipStreamSynchronize(c->stream));    // (a frame in flight keeps its buffers)
        // (the depth views' child aliases dObjStatic and dGroupRefs, and its own lists are sized by the old counts)
        if (c->depthCtx) { chordvis_destroy(c->depthCtx); c->depthCtx = nullptr; }
        for (Grow& g : grow) { if (*g.slot) (void)hipFree(*g.slot); *g.slot = g.fresh; }
        if (growObjects) c->allocObjects = count;
        if (growGroups) c->allocGroupInst = groupInstances;
        if (growBlocks) c->allocCullBlocks = cullBlocks;
        if (growCmds) {
            c->allocCmds = cmdCapacity;
            dfree(c->dRankCmds); dfree(c->dLeftCmds); dfree(c->dMineCmds);     // (sized by allocCmds; re-made on demand)
        }
        if (growTris) c->allocTris = caps.triCap;
        if (growTrisC) c->allocTrisC = caps.triCapC;
        if (growPool) c->allocBlocks = caps.blockCap;
        free_retired(c);
    }

    // (a host that re-makes what the call drops after every call and never calls anything that waits: the parked memory is bounded)
    if (c->retired.size() + c->retiredChildren.size() >= 32u) { CHORD_HIP(c, hipStreamSynchronize(c->stream)); free_retired(c); }

    // commit: host state, then one copy of the records, one of the static table, one launch -- all behind the frames in flight
    c->hObjStatic.swap(stat);
    c->objectCount = count; c->groupInstances = groupInstances; c->cmdCapacity = cmdCapacity; c->cullBlocks = cullBlocks;
    c->instTriangles = t.instTriangles;
    chord::scene_work_caps(c);
    for (int i = 0; i < 3; i++) c->lists[i].capacity = cmdCapacity;
    // what was sized by or named the old list goes, as with chordvis_upload_scene (the history HZB and a pending tail stay)
    c->mineValid = false; c->listMine[1] = c->listMine[2] = false; c->fullListStale = false;
    retire(c, c->dGeoFeedback); c->geoFeedbackCmds = nullptr;
    retire(c, c->dWorldCur); retire(c, c->dWorldPrev); retire(c, c->dBuildStatus); c->buildCount = 0;
    drop_ray_tlas(c, true);                               // (the BLASes are the scene's and stay)
    if (c->depthCtx) { c->retiredChildren.push_back(c->depthCtx); c->depthCtx = nullptr; }
    c->shadowHistoryValid = false; c->fusedDepthView = -1;
    c->resolveFrame = false;
    c->dObjects = c->dObjectsOwned;
    // (hostObjects and the static table are pageable: the copies read them before they return, as chordvis_update_objects' does)
    CHORD_HIP(c, hipMemcpyAsync(c->dObjectsOwned, hostObjects, sizeof(ChordObject) * (size_t)count, hipMemcpyHostToDevice, c->stream));
    CHORD_HIP(c, hipMemcpyAsync(c->dObjStatic, c->hObjStatic.data(), sizeof(DObjStatic) * (size_t)count, hipMemcpyHostToDevice, c->stream));
    chord::launch_group_refs_build(c);
    CHORD_HIP(c, hipGetLastError());
    // (a sharded context: cullChunkBlocks follows the new cullBlocks -- what chordvis_upload_scene runs)
    return chord::prepare_cull_exchange(c);
}

// ---- object records built on the device from resident f64 world transforms (kernels_objects.hip) ----

int chordvis_upload_world_transforms(ChordCtx* c, const double* hostLocalToWorld, const double* hostPrevLocalToWorld, uint32_t count)
{
    if (!c) return CHORDVIS_E_INVALID;
    if (c->sharedScene) return fail(c, CHORDVIS_E_INVALID, "upload_world_transforms: not on a depth-view context");
    if (!c->sceneLoaded) return fail(c, CHORDVIS_E_INVALID, "upload_world_transforms: no scene (call chordvis_upload_scene first)");
    if (!hostLocalToWorld || count != c->objectCount) return fail(c, CHORDVIS_E_INVALID, "upload_world_transforms: count must equal the uploaded scene's objectCount");
    (void)hipSetDevice(c->device);
    CHORD_HIP(c, hipStreamSynchronize(c->stream));                         // (a build in flight reads and writes the arrays being replaced)
    const size_t doubles = (size_t)count * 16u;
    if (!c->dWorldCur) {
        int rc;
        if ((rc = dalloc(c, &c->dWorldCur, doubles)) || (rc = dalloc(c, &c->dWorldPrev, doubles)) || (rc = dalloc(c, &c->dBuildStatus, (size_t)4))) {
            drop_world_transforms(c);
            return rc;
        }
    }
    const uint32_t cleared[4] = {0u, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu};
    CHORD_HIP(c, hipMemcpy(c->dWorldCur, hostLocalToWorld, doubles * sizeof(double), hipMemcpyHostToDevice));
    CHORD_HIP(c, hipMemcpy(c->dWorldPrev, hostPrevLocalToWorld ? hostPrevLocalToWorld : hostLocalToWorld, doubles * sizeof(double), hipMemcpyHostToDevice));
    CHORD_HIP(c, hipMemcpy(c->dBuildStatus, cleared, sizeof(cleared), hipMemcpyHostToDevice));
    c->buildCount = 0;
    return CHORDVIS_OK;
}

int chordvis_scatter_world_transforms(ChordCtx* c, const uint32_t* deviceIndices, const double* deviceLocalToWorld, uint32_t n)
{
    if (!c) return CHORDVIS_E_INVALID;
    if (!c->sceneLoaded || !c->dWorldCur) return fail(c, CHORDVIS_E_INVALID, "scatter_world_transforms: no chordvis_upload_world_transforms since the last chordvis_upload_scene");
    if (n == 0) return CHORDVIS_OK;
    if (!deviceIndices || !deviceLocalToWorld) return fail(c, CHORDVIS_E_INVALID, "scatter_world_transforms: null array with n > 0");
    if (((uintptr_t)deviceLocalToWorld & 15u) || ((uintptr_t)deviceIndices & 3u))
        return fail(c, CHORDVIS_E_INVALID, "scatter_world_transforms: deviceLocalToWorld must be 16-byte aligned (deviceIndices: 4-byte)");
    (void)hipSetDevice(c->device);
    chord::launch_scatter_world_transforms(c, deviceIndices, deviceLocalToWorld, n);
    CHORD_HIP(c, hipGetLastError());
    return CHORDVIS_OK;
}

int chordvis_build_objects(ChordCtx* c, const double cameraPos[3], const double cameraPosLast[3])
{
    if (!c) return CHORDVIS_E_INVALID;
    if (!c->sceneLoaded) return fail(c, CHORDVIS_E_INVALID, "build_objects: no scene (call chordvis_upload_scene first)");
    if (!c->dWorldCur) return fail(c, CHORDVIS_E_INVALID, "build_objects: no chordvis_upload_world_transforms since the last chordvis_upload_scene");
    if (!cameraPos) return fail(c, CHORDVIS_E_INVALID, "build_objects: cameraPos is NULL");
    (void)hipSetDevice(c->device);
    const uint32_t slot = (uint32_t)(c->buildCount & 1u);
    chord::launch_build_objects(c, cameraPos, cameraPosLast ? cameraPosLast : cameraPos, c->dBuildStatus + 2u * slot, c->dBuildStatus + 2u * (slot ^ 1u));
    CHORD_HIP(c, hipGetLastError());
    c->buildCount++;
    c->dObjects = c->dObjectsOwned;
    c->resolveStale = true;                               // (like chordvis_update_objects)
    c->rayRefitDue = true;
    return CHORDVIS_OK;
}

int chordvis_build_objects_status(ChordCtx* c, uint32_t* singularCount, uint32_t* firstSingular)
{
    if (!c) return CHORDVIS_E_INVALID;
    uint32_t words[2] = {0u, 0xFFFFFFFFu};
    if (c->dWorldCur && c->buildCount) {
        (void)hipSetDevice(c->device);
        CHORD_HIP(c, hipStreamSynchronize(c->stream));
        CHORD_HIP(c, hipMemcpy(words, c->dBuildStatus + 2u * (uint32_t)((c->buildCount - 1u) & 1u), sizeof(words), hipMemcpyDeviceToHost));
    }
    if (singularCount) *singularCount = words[0];
    if (firstSingular) *firstSingular = words[1];
    return CHORDVIS_OK;
}

int chordvis_readback_objects(ChordCtx* c, ChordObject* host, uint32_t count)
{
    if (!c || !c->sceneLoaded || !host || count != c->objectCount) return fail(c, CHORDVIS_E_INVALID, "readback_objects: count must equal the uploaded scene's objectCount");
    (void)hipSetDevice(c->device);
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    CHORD_HIP(c, hipMemcpy(host, c->dObjects, sizeof(ChordObject) * count, hipMemcpyDeviceToHost));
    return CHORDVIS_OK;
}

int chordvis_readback_world_transforms(ChordCtx* c, double* hostCur, double* hostPrev, uint32_t count)
{
    if (!c) return CHORDVIS_E_INVALID;
    if (!c->sceneLoaded || !c->dWorldCur) return fail(c, CHORDVIS_E_INVALID, "readback_world_transforms: no chordvis_upload_world_transforms since the last chordvis_upload_scene");
    if (count != c->objectCount) return fail(c, CHORDVIS_E_INVALID, "readback_world_transforms: count must equal the uploaded scene's objectCount");
    (void)hipSetDevice(c->device);
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    const size_t bytes = (size_t)count * 16u * sizeof(double);
    if (hostCur) CHORD_HIP(c, hipMemcpy(hostCur, c->dWorldCur, bytes, hipMemcpyDeviceToHost));
    if (hostPrev) CHORD_HIP(c, hipMemcpy(hostPrev, c->dWorldPrev, bytes, hipMemcpyDeviceToHost));
    return CHORDVIS_OK;
}

// ---- ray queries on the resident scene (include/chordvis.h RAY QUERIES; ray_scene.cpp; kernels_rays.hip) ----

extern "C++" {
namespace {

int ray_checks(ChordCtx* c, const char* fn, bool needTlas)
{
    char buf[160];
    auto refuse = [&](const char* why) { std::snprintf(buf, sizeof(buf), "%s: %s", fn, why); return fail(c, CHORDVIS_E_INVALID, buf); };
    if (c->sharedScene) return refuse("not on a depth-view context");
    if (!c->sceneLoaded) return refuse("no scene (call chordvis_upload_scene first)");
    if (needTlas && !(c->rayBlasBuilt && c->rayTlasBuilt))
        return refuse("no ray scene, or it was dropped by chordvis_upload_scene / chordvis_set_object_list (call chordvis_build_ray_scene)");
    return CHORDVIS_OK;
}

// the host's own copy of the object stage's box (kernels_rays.hip ray_refit_kernel): it shapes the TLAS, the device's boxes fill it
ray::Box host_object_box(const ChordObject& ob, const float* posMin, const float* posMax)
{
    const float* m = ob.basicData.localToTranslatedWorld.m;
    ray::Box b;
    for (int k = 0; k < 8; k++) {
        float q[3];
        for (int a = 0; a < 3; a++) {
            const float cen = (posMin[a] + posMax[a]) * 0.5f, ext = posMax[a] - cen;
            q[a] = ((k >> a) & 1) ? cen + ext : cen - ext;
        }
        for (int a = 0; a < 3; a++) {
            const float p = ((m[a] * q[0] + m[4 + a] * q[1]) + m[8 + a] * q[2]) + m[12 + a];
            b.lo[a] = k == 0 ? p : ray::fmin_(b.lo[a], p);
            b.hi[a] = k == 0 ? p : ray::fmax_(b.hi[a], p);
        }
    }
    return b;
}

struct RayBlasBuild {
    std::vector<ray::Node> nodes;
    std::vector<ray::Triangle> triangles;
    std::vector<uint32_t> roots;
    uint32_t depth = 0;
};

// One BLAS per primitive from the resident scene's streams, read back (the stream has run empty).
int ray_build_blases(ChordCtx* c, RayBlasBuild& out)
{
    std::vector<DMeshlet> meshlets(c->meshletCount);
    std::vector<uint8_t> lod(c->meshletCount);
    std::vector<DGroup> groups(c->groupCount);
    std::vector<uint32_t> gidx(c->groupIndexWords), mdata(c->meshletDataWords);
    std::vector<float> pos((size_t)c->vertexTotal * 3u);
#define DOWN(vec, src) if (!vec.empty()) CHORD_HIP(c, hipMemcpy(vec.data(), src, vec.size() * sizeof(vec[0]), hipMemcpyDeviceToHost));
    DOWN(meshlets, c->dMeshlets) DOWN(lod, c->dMeshletLod) DOWN(groups, c->dGroups) DOWN(gidx, c->dGroupIndices) DOWN(mdata, c->dMeshletData)
    DOWN(pos, c->dPositions)
#undef DOWN
    out.roots.assign(c->hPrims.size(), ray::kNoChild);
    std::vector<uint32_t> ids;
    std::vector<ray::Triangle> tris;
    std::vector<ray::Box> boxes;
    for (size_t pi = 0; pi < c->hPrims.size(); pi++) {
        const DPrim& pr = c->hPrims[pi];
        // the primitive's LOD-0 meshlets, reached through its groups, each once, in ascending order (upload_scene checked every index)
        ids.clear();
        for (uint32_t gl = 0; gl < pr.groupCount; gl++) {
            const DGroup& g = groups[pr.groupBase + gl];
            for (uint32_t i = 0; i < g.meshletCount; i++) {
                const uint32_t m = pr.meshletBase + gidx[pr.groupIndicesBase + g.meshletOffset + i];
                if (lod[m] == 0u) ids.push_back(m);
            }
        }
        std::sort(ids.begin(), ids.end());
        ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
        tris.clear();
        for (uint32_t m : ids) {
            const DMeshlet& ml = meshlets[m];
            const uint32_t V = ml.vertexTriangleCount & 0xFFu, T = (ml.vertexTriangleCount >> 8) & 0xFFu;
            for (uint32_t t = 0; t < T; t++) {
                const uint32_t w = mdata[ml.dataOffset + V + t];
                ray::Triangle tr{};
                for (int k = 0; k < 3; k++) {
                    const uint32_t vid = ml.vertexBase + mdata[ml.dataOffset + ((w >> (8 * k)) & 0xFFu)];
                    for (int a = 0; a < 3; a++) tr.v[3 * k + a] = pos[(size_t)vid * 3u + a];
                }
                for (int k = 0; k < 9; k++)
                    if (!std::isfinite(tr.v[k])) return fail(c, CHORDVIS_E_INVALID, "build_ray_scene: a LOD-0 triangle has a non-finite position");
                tr.meshlet = m - pr.assetMeshletBase; tr.triangle = t;
                tris.push_back(tr);
            }
        }
        if (tris.empty()) continue;
        if (out.triangles.size() + tris.size() >= ray::kMaxTriangles || out.nodes.size() + tris.size() >= ray::kIndexMask)
            return fail(c, CHORDVIS_E_CAPACITY, "build_ray_scene: 2^28 - 4 or more LOD-0 triangles in the scene");
        boxes.resize(tris.size());
        for (size_t i = 0; i < tris.size(); i++) boxes[i] = ray::triangle_box(tris[i]);
        ray::Tree tree;
        const int rc = ray::build_tree(boxes.data(), (uint32_t)tris.size(), ray::kLeafTriangles, ray::kBlasNode, ray::kBlasLeaf,
                                       (uint32_t)out.nodes.size(), (uint32_t)out.triangles.size(), tree);
        if (rc) return fail(c, CHORDVIS_E_CAPACITY, "build_ray_scene: a primitive's BLAS is deeper than CHORD_RAY_MAX_DEPTH levels (more than 4^12 leaves of four triangles)");
        out.roots[pi] = (ray::kBlasNode << ray::kTagShift) | (uint32_t)out.nodes.size();
        out.nodes.insert(out.nodes.end(), tree.nodes.begin(), tree.nodes.end());
        for (uint32_t i : tree.order) out.triangles.push_back(tris[i]);
        out.depth = std::max(out.depth, tree.depth);
    }
    return CHORDVIS_OK;
}

template <typename T>
int ray_upload(ChordCtx* c, T*& fresh, const void* host, size_t count, uint64_t& bytes)
{
    const size_t n = std::max<size_t>(count, 1) * sizeof(T);
    const hipError_t e = hipMalloc((void**)&fresh, n);
    if (e != hipSuccess) { fresh = nullptr; return fail(c, CHORDVIS_E_HIP, "build_ray_scene: hipMalloc of a ray scene buffer", e); }
    bytes += n;
    if (host && count) CHORD_HIP(c, hipMemcpy(fresh, host, count * sizeof(T), hipMemcpyHostToDevice));
    else if (!host) CHORD_HIP(c, hipMemsetAsync(fresh, 0, n, c->stream));
    return CHORDVIS_OK;
}

} // namespace
} // extern "C++"

int chordvis_ray_scene_info(ChordCtx* c, ChordRaySceneInfo* out)
{
    if (!c) return CHORDVIS_E_INVALID;
    if (!out) return fail(c, CHORDVIS_E_INVALID, "ray_scene_info: outInfo is NULL");
    { const int rc = ray_checks(c, "ray_scene_info", true); if (rc) return rc; }
    (void)hipSetDevice(c->device);
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    float root[8];
    CHORD_HIP(c, hipMemcpy(root, c->dRayRoot, sizeof(root), hipMemcpyDeviceToHost));
    std::memset(out, 0, sizeof(*out));
    out->blasCount = c->primCount; out->blasNodes = c->rayBlasNodes; out->blasTriangles = c->rayBlasTriangles;
    out->blasMaxDepth = c->rayBlasDepth; out->tlasNodes = c->rayTlasNodes; out->tlasDepth = c->rayTlasDepth;
    out->deviceBytes = c->rayBlasBytes + c->rayTlasBytes;
    for (int a = 0; a < 3; a++) { out->rootMin[a] = root[a]; out->rootMax[a] = root[4 + a]; }
    return CHORDVIS_OK;
}

// Everything is built on the host and every new device buffer made and filled before anything of the context's ray scene is touched.
int chordvis_build_ray_scene(ChordCtx* c, ChordRaySceneInfo* outInfo)
{
    if (!c) return CHORDVIS_E_INVALID;
    { const int rc = ray_checks(c, "build_ray_scene", false); if (rc) return rc; }
    (void)hipSetDevice(c->device);
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    free_retired(c);                                      // (what chordvis_set_object_list parked, a TLAS before this one among it)
#if CHORD_RAY_COUNTERS
    if (!c->dRayCounts) {
        CHORD_HIP(c, hipMalloc((void**)&c->dRayCounts, sizeof(unsigned long long) * CHORD_RAY_COUNTER_WORDS));
        CHORD_HIP(c, hipMemset(c->dRayCounts, 0, sizeof(unsigned long long) * CHORD_RAY_COUNTER_WORDS));
    }
#endif

    const bool buildBlas = !c->rayBlasBuilt;
    RayBlasBuild blas;
    if (buildBlas) { const int rc = ray_build_blases(c, blas); if (rc) return rc; }

    // the TLAS over the boxes of the object array the frames read now
    std::vector<ChordObject> objects(c->objectCount);
    CHORD_HIP(c, hipMemcpy(objects.data(), c->dObjects, sizeof(ChordObject) * objects.size(), hipMemcpyDeviceToHost));
    std::vector<ray::Box> boxes(c->objectCount);
    for (uint32_t o = 0; o < c->objectCount; o++) boxes[o] = host_object_box(objects[o], c->hObjStatic[o].posMin, c->hObjStatic[o].posMax);
    ray::Tree tlas;
    if (ray::build_tree(boxes.data(), c->objectCount, 1u, ray::kTlasNode, ray::kTlasLeaf, 0u, 0u, tlas))
        return fail(c, CHORDVIS_E_CAPACITY, "build_ray_scene: the TLAS is deeper than CHORD_RAY_MAX_DEPTH levels (more than 4^12 objects)");

    ray::Node *fBlas = nullptr, *fTlas = nullptr;
    ray::Triangle* fTris = nullptr;
    uint32_t *fRoots = nullptr, *fLeafRef = nullptr, *fCounters = nullptr;
    float *fLeafBox = nullptr, *fRoot = nullptr;
    uint64_t blasBytes = 0, tlasBytes = 0;
    int rc = CHORDVIS_OK;
    if (buildBlas) {
        if (!rc) rc = ray_upload(c, fBlas, blas.nodes.data(), blas.nodes.size(), blasBytes);
        if (!rc) rc = ray_upload(c, fTris, blas.triangles.data(), blas.triangles.size(), blasBytes);
        if (!rc) rc = ray_upload(c, fRoots, blas.roots.data(), blas.roots.size(), blasBytes);
    }
    if (!rc) rc = ray_upload(c, fTlas, tlas.nodes.data(), tlas.nodes.size(), tlasBytes);
    if (!rc) rc = ray_upload(c, fLeafRef, tlas.leafRef.data(), tlas.leafRef.size(), tlasBytes);
    if (!rc) rc = ray_upload(c, fCounters, nullptr, tlas.nodes.size(), tlasBytes);
    if (!rc) rc = ray_upload(c, fLeafBox, nullptr, (size_t)c->objectCount * 8u, tlasBytes);
    if (!rc) rc = ray_upload(c, fRoot, nullptr, 8u, tlasBytes);
    if (rc) {
        dfree(fBlas); dfree(fTris); dfree(fRoots); dfree(fTlas); dfree(fLeafRef); dfree(fCounters); dfree(fLeafBox); dfree(fRoot);
        return rc;
    }

    // commit (the stream is empty: nothing reads the old buffers)
    if (buildBlas) {
        dfree(c->dRayBlas); dfree(c->dRayTriangles); dfree(c->dRayBlasRoot);
        c->dRayBlas = fBlas; c->dRayTriangles = fTris; c->dRayBlasRoot = fRoots;
        c->rayBlasNodes = (uint32_t)blas.nodes.size(); c->rayBlasTriangles = (uint32_t)blas.triangles.size(); c->rayBlasDepth = blas.depth;
        c->rayBlasBytes = blasBytes; c->rayBlasBuilt = true;
    }
    drop_ray_tlas(c, false);
    c->dRayTlas = fTlas; c->dRayLeafRef = fLeafRef; c->dRayCounters = fCounters; c->dRayLeafBox = fLeafBox; c->dRayRoot = fRoot;
    c->rayTlasNodes = (uint32_t)tlas.nodes.size(); c->rayTlasDepth = tlas.depth; c->rayTlasBytes = tlasBytes; c->rayTlasBuilt = true;

    rc = chordvis_refit_ray_scene(c);
    if (rc) return rc;
    if (outInfo) {
        rc = chordvis_ray_scene_info(c, outInfo);
        if (rc) return rc;
        outInfo->blasBuilt = buildBlas ? c->primCount : 0u;
    }
    return CHORDVIS_OK;
}

int chordvis_refit_ray_scene(ChordCtx* c)
{
    if (!c) return CHORDVIS_E_INVALID;
    { const int rc = ray_checks(c, "refit_ray_scene", true); if (rc) return rc; }
    (void)hipSetDevice(c->device);
    chord::launch_ray_refit(c);
    CHORD_HIP(c, hipGetLastError());
    c->rayRefitDue = false;
    return CHORDVIS_OK;
}

int chordvis_trace_rays(ChordCtx* c, const ChordRay* deviceRays, uint32_t count, uint32_t flags, ChordRayHit* deviceHits)
{
    if (!c) return CHORDVIS_E_INVALID;
    { const int rc = ray_checks(c, "trace_rays", true); if (rc) return rc; }
    if (flags & ~CHORD_RAY_ANY_HIT) return fail(c, CHORDVIS_E_INVALID, "trace_rays: unknown flag bits (CHORD_RAY_ANY_HIT is the only flag)");
    if (c->rayRefitDue)
        return fail(c, CHORDVIS_E_INVALID, "trace_rays: the objects changed (chordvis_update_objects / chordvis_build_objects / chordvis_bind_objects): call chordvis_refit_ray_scene first");
    if (count == 0) return CHORDVIS_OK;
    if (!deviceRays || !deviceHits || ((uintptr_t)deviceRays & 15u) || ((uintptr_t)deviceHits & 15u))
        return fail(c, CHORDVIS_E_INVALID, "trace_rays: deviceRays and deviceHits must be non-NULL and 16-byte aligned when count > 0");
    (void)hipSetDevice(c->device);
    chord::launch_ray_trace(c, deviceRays, count, (flags & CHORD_RAY_ANY_HIT) != 0u, deviceHits);
    CHORD_HIP(c, hipGetLastError());
    return CHORDVIS_OK;
}

// Everything is checked before the device is touched; no device pointer is dereferenced here.  The refusals of chordvis_trace_rays
// first, in its order; then the desc; then -- behind the empty image, which launches nothing -- the pointers the desc asks for.
int chordvis_pixel_rays(ChordCtx* c, const ChordPixelRaysDesc* desc, const float* devicePosition, const float* deviceNormal, const float* deviceZ,
                        const float* deviceTable, float* deviceOut, ChordRayHit* deviceHits)
{
    if (!c) return CHORDVIS_E_INVALID;
    { const int rc = ray_checks(c, "pixel_rays", true); if (rc) return rc; }
    if (c->rayRefitDue)
        return fail(c, CHORDVIS_E_INVALID, "pixel_rays: the objects changed (chordvis_update_objects / chordvis_build_objects / chordvis_bind_objects): call chordvis_refit_ray_scene first");
    if (!desc) return fail(c, CHORDVIS_E_INVALID, "pixel_rays: desc is NULL");
    const uint32_t kFlags = CHORD_PIXEL_RAYS_ANY_HIT | CHORD_PIXEL_RAYS_FRONT_ONLY | CHORD_PIXEL_RAYS_START_FROM_DEPTH;
    if (desc->mode != CHORD_PIXEL_RAYS_HEMISPHERE && desc->mode != CHORD_PIXEL_RAYS_DIRECTION)
        return fail(c, CHORDVIS_E_INVALID, "pixel_rays: unknown mode (CHORD_PIXEL_RAYS_HEMISPHERE or CHORD_PIXEL_RAYS_DIRECTION)");
    if (desc->flags & ~kFlags)
        return fail(c, CHORDVIS_E_INVALID, "pixel_rays: unknown flag bits (CHORD_PIXEL_RAYS_ANY_HIT, _FRONT_ONLY and _START_FROM_DEPTH are the flags)");
    const bool hemisphere = desc->mode == CHORD_PIXEL_RAYS_HEMISPHERE;
    const bool anyHit = (desc->flags & CHORD_PIXEL_RAYS_ANY_HIT) != 0u, frontOnly = (desc->flags & CHORD_PIXEL_RAYS_FRONT_ONLY) != 0u;
    if (hemisphere) {
        const uint32_t tw = desc->tableW, th = desc->tableH;
        if (!deviceTable) return fail(c, CHORDVIS_E_INVALID, "pixel_rays: CHORD_PIXEL_RAYS_HEMISPHERE needs deviceTable");
        if (tw == 0u || th == 0u || (tw & (tw - 1u)) || (th & (th - 1u)))
            return fail(c, CHORDVIS_E_INVALID, "pixel_rays: tableW and tableH must be powers of two");
    }
    if ((desc->flags & CHORD_PIXEL_RAYS_START_FROM_DEPTH) && !deviceZ)
        return fail(c, CHORDVIS_E_INVALID, "pixel_rays: CHORD_PIXEL_RAYS_START_FROM_DEPTH needs deviceZ");
    if (deviceZ && desc->deviceZStride == 0u) return fail(c, CHORDVIS_E_INVALID, "pixel_rays: deviceZStride must not be 0 with a deviceZ");
    if (anyHit && deviceHits) return fail(c, CHORDVIS_E_INVALID, "pixel_rays: CHORD_PIXEL_RAYS_ANY_HIT writes no hit records (deviceHits must be NULL)");
    if (frontOnly && hemisphere) return fail(c, CHORDVIS_E_INVALID, "pixel_rays: CHORD_PIXEL_RAYS_FRONT_ONLY goes with CHORD_PIXEL_RAYS_DIRECTION only");
    const uint64_t pixels = (uint64_t)desc->width * desc->height;
    if (pixels > 0xFFFFFFFFull) return fail(c, CHORDVIS_E_INVALID, "pixel_rays: width * height must not exceed 2^32 - 1");
    if (pixels == 0u) return CHORDVIS_OK;
    if (!devicePosition || ((uintptr_t)devicePosition & 15u))
        return fail(c, CHORDVIS_E_INVALID, "pixel_rays: devicePosition must be non-NULL and 16-byte aligned");
    const bool needNormal = hemisphere || frontOnly;
    if (needNormal && (!deviceNormal || ((uintptr_t)deviceNormal & 15u)))
        return fail(c, CHORDVIS_E_INVALID, "pixel_rays: deviceNormal must be non-NULL and 16-byte aligned (HEMISPHERE, FRONT_ONLY)");
    if (hemisphere && ((uintptr_t)deviceTable & 15u)) return fail(c, CHORDVIS_E_INVALID, "pixel_rays: deviceTable must be 16-byte aligned");
    if ((uintptr_t)deviceZ & 3u) return fail(c, CHORDVIS_E_INVALID, "pixel_rays: deviceZ must be NULL or 4-byte aligned");
    if (!deviceOut || ((uintptr_t)deviceOut & 3u)) return fail(c, CHORDVIS_E_INVALID, "pixel_rays: deviceOut must be non-NULL and 4-byte aligned");
    if ((uintptr_t)deviceHits & 15u) return fail(c, CHORDVIS_E_INVALID, "pixel_rays: deviceHits must be NULL or 16-byte aligned");
    (void)hipSetDevice(c->device);
    // (a normal or a table no statement reads is not handed to the kernel)
    chord::launch_pixel_rays(c, *desc, devicePosition, needNormal ? deviceNormal : nullptr, deviceZ, hemisphere ? deviceTable : nullptr, deviceOut, deviceHits);
    CHORD_HIP(c, hipGetLastError());
    return CHORDVIS_OK;
}

// Everything is checked before the device is touched; no device pointer is dereferenced here.  Needs no ray scene: the hits may be a host's.
int chordvis_shade_ray_hits(ChordCtx* c, const ChordRayHit* deviceHits, uint32_t count, float lod, const float* deviceLods, ChordRayHitSurface* deviceSurfaces)
{
    if (!c) return CHORDVIS_E_INVALID;
    { const int rc = ray_checks(c, "shade_ray_hits", false); if (rc) return rc; }
    if (c->cullPhaseDone) return fail(c, CHORDVIS_E_INVALID, "shade_ray_hits: not between chordvis_frame_phase_cull and chordvis_frame_phase_a");
    if (!c->matTexturesLoaded || !c->dMatRecords)
        return fail(c, CHORDVIS_E_INVALID, "shade_ray_hits: no material textures since the last chordvis_upload_scene (call chordvis_upload_material_textures first)");
    if (count == 0) return CHORDVIS_OK;
    if (!deviceHits || !deviceSurfaces || ((uintptr_t)deviceHits & 15u) || ((uintptr_t)deviceSurfaces & 15u))
        return fail(c, CHORDVIS_E_INVALID, "shade_ray_hits: deviceHits and deviceSurfaces must be non-NULL and 16-byte aligned when count > 0");
    if ((uintptr_t)deviceLods & 3u)
        return fail(c, CHORDVIS_E_INVALID, "shade_ray_hits: deviceLods must be NULL (one lod for every hit) or 4-byte aligned");
    (void)hipSetDevice(c->device);
    chord::launch_ray_shade(c, deviceHits, count, lod, deviceLods, deviceSurfaces);
    CHORD_HIP(c, hipGetLastError());
    return CHORDVIS_OK;
}

int chordvis_set_view(ChordCtx* c, const ChordCameraView* view, const ChordInstanceCullingView* iv, uint32_t switchFlags)
{
    if (!c || !view || !iv) return fail(c, CHORDVIS_E_INVALID, "set_view: null argument");
    // (the rank masks on their way through the all-gather were computed with the current view, cull mode and tile map)
    if (c->cullPhaseDone) return fail(c, CHORDVIS_E_INVALID, "set_view: not between chordvis_frame_phase_cull and chordvis_frame_phase_a");
    // (refused before anything is taken over: the view set before stays the context's)
    if (c->dVis && ((uint32_t)iv->renderDimension[0] != c->width || (uint32_t)iv->renderDimension[1] != c->height))
        return fail(c, CHORDVIS_E_INVALID, "set_view: renderDimension differs from the allocated gbuffer");
    c->hView.view = *view; c->hView.iv = *iv; c->hView.flags = switchFlags;
    c->hView.width = (uint32_t)iv->renderDimension[0]; c->hView.height = (uint32_t)iv->renderDimension[1];
    // the 600-byte constant block travels as a kernel argument of the frame's first kernel (object_cull),
    // which publishes it for the later passes; see flush_view() for passes called out of frame order
    c->viewDirty = true;
    c->viewSet = true;
    c->resolveStale = true;
    return CHORDVIS_OK;
}

int chordvis_allocate_gbuffer(ChordCtx* c, uint32_t width, uint32_t height, uint64_t* deviceVisibility)
{
    if (!c || width < 64 || height < 64 || width > 4096 || height > 4096)      // renderer.h:52-53
        return fail(c, CHORDVIS_E_INVALID, "allocate_gbuffer: render size must be 64..4096 per axis (renderer.h:52-53)");
    CHORD_HIP(c, hipSetDevice(c->device));
    c->width = width; c->height = height;
    dfree(c->dTileMarker); dfree(c->dShadingTiles);                             // sized by the render size; re-made on demand
    // (a view of another size stays set but no longer fits: ready() refuses the passes until chordvis_set_view has come again)
    return configure_targets(c, deviceVisibility);
}

int chordvis_set_limits(ChordCtx* c, const ChordLimits* limits)
{
    if (c) c->orderAge = c->orderAge1 = 0xFFFFFFFFu;                    // (the kept tile schedule of launch_raster is made again)

    if (!c || !limits) return fail(c, CHORDVIS_E_INVALID, "set_limits: null argument");
    if (c->sceneLoaded || c->dVis) return fail(c, CHORDVIS_E_INVALID, "set_limits: call before upload_scene / allocate_gbuffer");
    if (limits->maxTriangleRecords) {
        if (limits->maxTriangleRecords < (1u << 16) || limits->maxTriangleRecords > 0x7FFFFFC0ull)
            return fail(c, CHORDVIS_E_INVALID, "set_limits: maxTriangleRecords out of range (record indices are 32-bit)");
        c->limitRecords = limits->maxTriangleRecords & ~(uint64_t)(CHORD_LIST_SHARDS - 1);
    }
    if (limits->binPoolChunks) {
        if (limits->binPoolChunks > (16u << 20)) return fail(c, CHORDVIS_E_INVALID, "set_limits: at most 16 Mi pool chunks per pass (64 GB)");
        c->limitPoolChunks = limits->binPoolChunks;
    }
    if (limits->binMaxChunksPerTile) {
        if (limits->binMaxChunksPerTile > CHORD_BIN_MAX_CHUNKS_LIMIT) return fail(c, CHORDVIS_E_INVALID, "set_limits: at most 3072 overflow chunks per tile");
        c->binMaxChunks = limits->binMaxChunksPerTile;
    }
    return CHORDVIS_OK;
}

int chordvis_set_tile_schedule_keep(ChordCtx* c, uint32_t frames)
{
    if (!c) return CHORDVIS_E_INVALID;
    c->orderKeepFrames = frames;
    c->orderAge = c->orderAge1 = 0xFFFFFFFFu;
    return CHORDVIS_OK;
}
uint32_t chordvis_tile_schedule_keep(ChordCtx* c) { return c ? c->orderKeepFrames : 0u; }

int chordvis_set_cull_mode(ChordCtx* c, int hierarchical)
{
    if (!c || hierarchical < 0 || hierarchical > 1) return fail(c, CHORDVIS_E_INVALID, "set_cull_mode: 0 (flat) or 1 (hierarchical)");
    if (hierarchical && c->sceneLoaded && !c->bvhComplete) return fail(c, CHORDVIS_E_INVALID, "set_cull_mode: the uploaded scene has primitives without a BVH");
    if (c->cullPhaseDone) return fail(c, CHORDVIS_E_INVALID, "set_cull_mode: not between chordvis_frame_phase_cull and chordvis_frame_phase_a");
    c->cullMode = hierarchical;
    return CHORDVIS_OK;
}

int chordvis_set_shard(ChordCtx* c, uint32_t ranks, uint32_t rank)
{
    if (c) c->orderAge = c->orderAge1 = 0xFFFFFFFFu;                    // (the kept tile schedule of launch_raster is made again)

    if (!c || ranks == 0 || ranks > 255u || rank >= ranks) return fail(c, CHORDVIS_E_INVALID, "set_shard: rank < ranks <= 255");
#if CHORD_TILE_SHIFT != 6
    if (ranks > 1) return fail(c, CHORDVIS_E_INVALID, "set_shard: this build's raster tiles are not 64 x 64");
#endif
    if (c->inFrame || c->cullPhaseDone) return fail(c, CHORDVIS_E_INVALID, "set_shard: not inside a frame");
    if (c->shard.ranks != ranks) { c->tileOwners.clear(); c->tileOwnersExplicit = false; }
    c->shard.ranks = ranks; c->shard.rank = rank;
    c->mineValid = false; c->listMine[1] = c->listMine[2] = false;       // (lists culled for another ownership)
    if (c->width) {
        if (c->visExternal) { c->dVis = nullptr; return fail(c, CHORDVIS_E_INVALID, "set_shard after allocate_gbuffer with an external buffer: call allocate_gbuffer again"); }
        return configure_targets(c, nullptr);
    }
    return CHORDVIS_OK;
}

// An explicit tile map (one owner per tile, row-major over the tile grid; the same table on every rank), e.g. from
// chordvis_tile_layout with the loads of a rendered frame.  Between frames; the history HZB carries over (it is not sharded).
int chordvis_set_tile_owners(ChordCtx* c, const uint8_t* owners, uint32_t tiles)
{
    if (!c || c->shard.ranks <= 1 || !c->width) return fail(c, CHORDVIS_E_INVALID, "set_tile_owners: a sharded context with a G-buffer");
    std::vector<uint8_t> def;
    if (!owners) {                                                        // NULL: back to the default map
        tiles = c->tilesX * c->tilesY;
        def.assign(tiles, 0);
        if (tile_layout(c->tilesX, c->tilesY, c->shard.ranks, nullptr, 0u, def.data()) != CHORDVIS_OK) return fail(c, CHORDVIS_E_INVALID, "tile layout");
        owners = def.data();
    }
    if (tiles != c->tilesX * c->tilesY) return fail(c, CHORDVIS_E_INVALID, "set_tile_owners: one owner per tile of the G-buffer");
    if (c->inFrame || c->cullPhaseDone) return fail(c, CHORDVIS_E_INVALID, "set_tile_owners: not inside a frame");
    // frames in flight (pipelined hosts: an image still travelling) were laid out with the old map
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    if (c->commResolveStream) CHORD_HIP(c, hipStreamSynchronize(c->commResolveStream));
    for (int k = 0; k < 2; k++) if (c->visReadyEvent[k]) CHORD_HIP(c, hipEventSynchronize(c->visReadyEvent[k]));
    std::vector<uint8_t> keep = c->tileOwners;
    c->tileOwners.assign(owners, owners + tiles);
    const int rc = install_tile_owners(c);
    if (rc) { c->tileOwners = keep; if (!keep.empty()) (void)install_tile_owners(c); return rc; }
    c->tileOwnersExplicit = def.empty();
    return CHORDVIS_OK;
}

int chordvis_get_tile_owners(ChordCtx* c, uint8_t* ownersOut, uint32_t tiles)
{
    if (!c || !ownersOut || c->shard.ranks <= 1 || c->tileOwners.size() != tiles) return fail(c, CHORDVIS_E_INVALID, "get_tile_owners: a sharded context with a G-buffer, one entry per tile");
    std::memcpy(ownersOut, c->tileOwners.data(), tiles);
    return CHORDVIS_OK;
}

// Bin entries per tile of the last frame this context finished, every rank's tiles (they travel in the end-of-frame exchange).
// Waits for the context's stream.
int chordvis_read_tile_loads(ChordCtx* c, uint32_t* loadsOut, uint32_t tiles)
{
    if (!c || !loadsOut || c->shard.ranks <= 1 || !c->dTileLoads || tiles != c->tilesX * c->tilesY) return fail(c, CHORDVIS_E_INVALID, "read_tile_loads: a sharded context with a G-buffer, one entry per tile");
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    CHORD_HIP(c, hipMemcpy(loadsOut, c->dTileLoads, sizeof(uint32_t) * tiles, hipMemcpyDeviceToHost));
    return CHORDVIS_OK;
}

// Re-balances the tile map from the last frame's loads: chordvis_read_tile_loads -> chordvis_tile_layout -> chordvis_set_tile_owners.
// Every rank of the frame must call it at the same frame boundary (they hold the same loads, so they compute the same map).
// imbalance (may be NULL): max over ranks of the OLD map's load / the mean, x 1000.
int chordvis_rebalance(ChordCtx* c, uint32_t* imbalancePermille)
{
    if (!c || c->shard.ranks <= 1 || !c->dTileLoads) return fail(c, CHORDVIS_E_INVALID, "rebalance: a sharded context with a G-buffer");
    const uint32_t tiles = c->tilesX * c->tilesY, N = c->shard.ranks;
    std::vector<uint32_t> loads(tiles);
    int rc = chordvis_read_tile_loads(c, loads.data(), tiles);
    if (rc) return rc;
    std::vector<uint64_t> per(N, 0);
    uint64_t total = 0;
    for (uint32_t t = 0; t < tiles; t++) { per[c->tileOwners[t]] += loads[t]; total += loads[t]; }
    if (imbalancePermille) *imbalancePermille = total ? (uint32_t)(*std::max_element(per.begin(), per.end()) * N * 1000u / total) : 1000u;
    if (total == 0) return CHORDVIS_OK;                                  // (no frame rendered yet: keep the map)
    std::vector<uint8_t> owners(tiles);
    if (tile_layout(c->tilesX, c->tilesY, N, loads.data(), c->slotCapacity, owners.data()) != CHORDVIS_OK) return fail(c, CHORDVIS_E_INVALID, "rebalance: tile layout");
    return chordvis_set_tile_owners(c, owners.data(), tiles);
}

uint64_t chordvis_visibility_words(ChordCtx* c)
{
    if (!c) return 0;
    if (c->width == 0) return 0;
    const uint32_t N = c->shard.ranks;
    return N > 1 ? (uint64_t)N * chordvis_tile_slot_capacity(c->width, c->height, N) * (CHORD_TILE * CHORD_TILE) : (uint64_t)c->width * c->height;
}
uint64_t chordvis_visibility_chunk_words(ChordCtx* c) { return !c ? 0 : c->shard.ranks > 1 ? (uint64_t)c->shard.slotsPerRank * (CHORD_TILE * CHORD_TILE) : chordvis_visibility_words(c); }
uint64_t* chordvis_visibility_ptr(ChordCtx* c) { return c ? c->dVis : nullptr; }
uint64_t* chordvis_resolved_visibility_ptr(ChordCtx* c) { return c ? (c->shard.ranks > 1 ? c->dVisResolved : c->dVis) : nullptr; }
uint16_t* chordvis_hzb_exchange_ptr(ChordCtx* c) { return c ? c->dHzbExchange : nullptr; }
uint16_t* chordvis_hzb_final_exchange_ptr(ChordCtx* c) { return c ? c->dHzbFinalExchange : nullptr; }
uint64_t chordvis_hzb_final_exchange_chunk_bytes(ChordCtx* c) { return c ? c->hzbFinalExchangeChunkBytes : 0; }

// Pipelined sharded frames keep TWO frames' visibility words alive: the one whose all-gather is still travelling and the
// one being rasterized.  Swaps the roles of the two buffer pairs (the second pair is allocated on first use); call between
// frames, before chordvis_frame_phase_a.
int chordvis_swap_visibility(ChordCtx* c)
{
    if (!c || !c->dVis) return fail(c, CHORDVIS_E_INVALID, "swap_visibility: allocate_gbuffer must come first");
    if (c->shard.ranks <= 1 || c->visExternal) return fail(c, CHORDVIS_E_INVALID, "swap_visibility: only for sharded contexts that own their visibility buffer");
    if (c->inFrame) return fail(c, CHORDVIS_E_INVALID, "swap_visibility: not inside a frame");
    int rc;
    if (!c->dVisAlt) {
        if ((rc = dalloc(c, &c->dVisAlt, c->visWords))) return rc;
        if ((rc = dalloc(c, &c->dVisResolvedAlt, (uint64_t)c->width * c->height))) return rc;
        CHORD_HIP(c, hipMemsetAsync(c->dVisAlt, 0, c->visWords * 8, c->stream));   // (incl. the padding of edge tiles' slots)
        CHORD_HIP(c, hipMemsetAsync(c->dVisResolvedAlt, 0, (uint64_t)c->width * c->height * 8, c->stream));
    }
    std::swap(c->dVisOwned, c->dVisAlt);
    c->dVis = c->dVisOwned;
    std::swap(c->dVisResolved, c->dVisResolvedAlt);
    std::swap(c->visReadyEvent[0], c->visReadyEvent[1]);
    return CHORDVIS_OK;
}
uint64_t chordvis_hzb_exchange_halves(ChordCtx* c) { return c ? c->hzbExchangeHalves : 0; }
// the sharded cull's exchange buffer (made on first request, after upload_scene and chordvis_set_shard; NULL / 0 when the sharded
// cull does not apply: one rank, more than 8, no scene)
uint32_t* chordvis_cull_exchange_ptr(ChordCtx* c) { return (c && c->sceneLoaded && c->shard.ranks > 1 && c->shard.ranks <= 8u && ensure_cull_exchange(c) == CHORDVIS_OK) ? c->dCullExchange : nullptr; }
uint64_t chordvis_cull_exchange_chunk_bytes(ChordCtx* c) { return chordvis_cull_exchange_ptr(c) ? (uint64_t)c->cullChunkBlocks * 257u * 4u : 0; }
// measurement / test aid: fills EVERY rank's chunk of the cull exchange buffer on this context (what the all-gather would deliver),
// for the current view -- tools/shard_time.py times one rank at a time on one device
int chordvis_debug_fill_cull_exchange(ChordCtx* c)
{
    int rc = ready(c, "debug_fill_cull_exchange");
    if (rc) return rc;
    if (!cull_shardable_config(c)) return fail(c, CHORDVIS_E_INVALID, "debug_fill_cull_exchange: the sharded cull does not apply");
    if ((rc = ensure_cull_exchange(c))) return rc;
    if (c->inFrame) return fail(c, CHORDVIS_E_INVALID, "debug_fill_cull_exchange: not inside a frame");
    if ((rc = flush_view(c))) return rc;
    launch_cull_masks(c, true);
    CHORD_HIP(c, hipGetLastError());
    return CHORDVIS_OK;
}
uint64_t chordvis_hzb_exchange_chunk_halves(ChordCtx* c) { return c ? c->hzbExchangeChunkHalves : 0; }

// -------------------------------------------------------------------------------------- passes --

int chordvis_clear_gbuffer(ChordCtx* c)
{
    int rc = ready(c, "clear_gbuffer");
    if (rc) return rc;
    // visibility = 0 / depth = 0.0 (render_textures.cpp:81-85,98-100).  Sharded: only the rank's own
    // chunk needs clearing (the all-gather overwrites the rest).
    if (c->shard.ranks > 1) {
        const uint64_t chunk = (uint64_t)c->shard.slotsPerRank * (CHORD_TILE * CHORD_TILE);
        CHORD_HIP(c, hipMemsetAsync(c->dVis + chunk * c->shard.rank, 0, chunk * 8, c->stream));
    } else {
        CHORD_HIP(c, hipMemsetAsync(c->dVis, 0, c->visWords * 8, c->stream));
    }
    CHORD_HIP(c, hipMemsetAsync(c->dCounters, 0, sizeof(DeviceCounters), c->stream));
    c->rasterCalls = 0;
    c->pendingClear = false;
    c->inFrame = false;
    return CHORDVIS_OK;
}

int chordvis_instance_culling(ChordCtx* c, ChordCountAndCmd* out)
{
    int rc = ready(c, "instance_culling");
    if (rc) return rc;
    launch_group_cull(c, c->lists[0]);                   // instanceCullingCS + clusterGroupCullingCS (objects + count, scatter)
    CHORD_HIP(c, hipGetLastError());
    if (out) *out = c->lists[0].handle();
    return CHORDVIS_OK;
}

int chordvis_hzb_culling(ChordCtx* c, const ChordHZB* hzb, int bFirstStage, ChordCountAndCmd in,
                         ChordCountAndCmd* outVisible, ChordCountAndCmd* outRejected)
{
    int rc = ready(c, "hzb_culling");
    if (rc) return rc;
    if (!hzb || !hzb->minTexels || !in.count || !in.cmds) return fail(c, CHORDVIS_E_INVALID, "hzb_culling: invalid HZB or command list");
    if ((rc = flush_pending_tail(c))) return rc;
    if ((rc = flush_view(c))) return rc;
    const HzbBuffers hb = from_handle(hzb);
    CmdList inL = from_handle(in);
    // Sharded frames: a rank culls (and later rasters) only the clusters that touch its pixel rows -- the group cull wrote them
    // to a list of their own -- so the occlusion tests shard with the screen like the raster does.  The decision per cluster
    // is a function of the cluster and the (exchanged, identical) HZB, so every owner of a straddling cluster decides alike.
    bool inMine = false;
    if (c->shard.ranks > 1) {
        if (inL.cmds == c->lists[0].cmds && c->mineValid) { inL.count = c->dCounts + 4; inL.cmds = c->dMineCmds; inMine = true; }
        else if (inL.cmds == c->dMineCmds && c->mineValid) inMine = true;
        else for (int k = 1; k < 3; k++) if (inL.cmds == c->lists[k].cmds && c->listMine[k]) inMine = true;
    }
    if (bFirstStage) {
        if (inL.cmds == c->lists[1].cmds || inL.cmds == c->lists[2].cmds) return fail(c, CHORDVIS_E_INVALID, "hzb_culling: first stage input must be the instanceCulling list");
        if (c->fusedCullDone && inL.cmds == c->lists[0].cmds && hzb->minTexels == c->hzb[c->historySlot].minTexels) {
            // (chordvis_render_frame on a short scene: frame_cull_fused_kernel tested every command it emitted against this chain)
            c->fusedCullDone = false;
        } else {
        if (!c->inFrame) CHORD_HIP(c, hipMemsetAsync(c->dCounts + 1, 0, 8, c->stream));
        c->listMine[1] = c->listMine[2] = inMine;
        launch_hzb_cull(c, hb, 0, inL, c->lists[1], &c->lists[2]);
        }
        if (outVisible) *outVisible = c->lists[1].handle();
        if (outRejected) *outRejected = c->lists[2].handle();
    } else {
        if (inL.cmds == c->lists[1].cmds) return fail(c, CHORDVIS_E_INVALID, "hzb_culling: second stage input aliases its output");
        CmdList vis1 = c->lists[1];
        vis1.count = c->dCounts + 3;
        if (!c->inFrame) CHORD_HIP(c, hipMemsetAsync(c->dCounts + 3, 0, 4, c->stream));
        c->listMine[1] = inMine;
        launch_hzb_cull(c, hb, 1, inL, vis1, nullptr);
        if (outVisible) *outVisible = vis1.handle();
        if (outRejected) *outRejected = ChordCountAndCmd{nullptr, nullptr, 0};
    }
    CHORD_HIP(c, hipGetLastError());
    return CHORDVIS_OK;
}

int chordvis_render_mesh(ChordCtx* c, ChordCountAndCmd in)
{
    int rc = ready(c, "render_mesh");
    if (rc) return rc;
    if (!in.count || !in.cmds) return CHORDVIS_OK;       // {nullptr, nullptr}: nothing to render (instance_culling.cpp:92-95)
    if ((rc = flush_view(c))) return rc;
    return do_raster(c, from_handle(in));
}

int chordvis_visibility_stage0(ChordCtx* c, const ChordHZB* hzbPrev, ChordCountAndCmd in, ChordCountAndCmd* outRejected, int* shouldStage1)
{
    int rc = ready(c, "visibility_stage0");
    if (rc) return rc;
    if (shouldStage1) *shouldStage1 = 0;
    if (outRejected) *outRejected = ChordCountAndCmd{nullptr, nullptr, 0};
    const bool hzbOn = hzbPrev && hzbPrev->minTexels && (c->hView.flags & CHORD_FLAG_HZB_CULL);   // mesh_raster.cpp:293
    if (hzbOn) {
        ChordCountAndCmd vis, rej;
        if ((rc = chordvis_hzb_culling(c, hzbPrev, 1, in, &vis, &rej))) return rc;
        if ((rc = chordvis_render_mesh(c, vis))) return rc;
        if (outRejected) *outRejected = rej;
        if (shouldStage1) *shouldStage1 = 1;
    } else {
        if ((rc = chordvis_render_mesh(c, in))) return rc;
    }
    return CHORDVIS_OK;
}

int chordvis_visibility_stage1(ChordCtx* c, const ChordHZB* hzb, ChordCountAndCmd in)
{
    int rc = ready(c, "visibility_stage1");
    if (rc) return rc;
    ChordCountAndCmd vis;
    if ((rc = chordvis_hzb_culling(c, hzb, 0, in, &vis, nullptr))) return rc;
    return chordvis_render_mesh(c, vis);
}

int chordvis_build_hzb(ChordCtx* c, int bBuildMin, int bBuildMax, int bBuildValidRange, int slot, ChordHZB* out)
{
    int rc = ready(c, "build_hzb");
    if (rc) return rc;
    if (slot < 0 || slot > 2 || !(bBuildMin || bBuildMax) || (bBuildValidRange && !(bBuildMin && bBuildMax)))   // hzb.cpp:43-47
        return fail(c, CHORDVIS_E_INVALID, "build_hzb: slot in 0..2, at least one channel, valid range needs min and max");
    if ((rc = flush_pending_tail(c))) return rc;
    // (a sharded context: from the resolved, row-major image -- chordvis_frame_resolve_visibility / phase c)
    launch_hzb_build(c, c->hzb[slot], bBuildMin != 0, bBuildMax != 0, bBuildValidRange != 0);
    CHORD_HIP(c, hipGetLastError());
    if (out) {
        *out = c->hzb[slot].handle();
        if (!bBuildMax) out->maxTexels = nullptr;
        if (!bBuildValidRange) out->validRange = nullptr;
    }
    return CHORDVIS_OK;
}

int chordvis_reset_history(ChordCtx* c)
{
    if (!c) return CHORDVIS_E_INVALID;
    c->pendingTailSlot = 0;
    c->historySlot = 0;
    return CHORDVIS_OK;
}

static int render_frame_impl(ChordCtx* c)
{
    int rc = ready(c, "render_frame");
    if (rc) return rc;
    if (c->comm) return comm_render_frame(c);            // one process per GPU: the library runs the two all-gathers (RCCL)
    if (c->shard.ranks > 1) return fail(c, CHORDVIS_E_INVALID, "render_frame: a sharded context needs a communicator (chordvis_comm_init_rank), a ChordGroup, or the host drives frame_phase_a/b/c");
    begin_frame_stamps(c);
    if ((rc = begin_frame_clear(c))) return rc;                                       // renderer.cpp:315
    record(c, S_CLEAR);
    ChordHZB hist;
    const bool haveHist = c->historySlot != 0;
    if (haveHist) hist = c->hzb[c->historySlot].handle();
    const int next = c->historySlot == 1 ? 2 : 1;
    ChordCountAndCmd post;
    // (short scenes: instanceCulling and the phase-0 occlusion cull of stage 0 are one kernel -- launch_group_cull is told what stage 0
    // will cull against, and chordvis_hzb_culling finds its lists made)
    c->fuseCullFrame = true;
    c->fuseCullHzb = (haveHist && (c->hView.flags & CHORD_FLAG_HZB_CULL)) ? &c->hzb[c->historySlot] : nullptr;
    c->fusedCullDone = false;
    rc = chordvis_instance_culling(c, &post);                                         // :321 (its first kernel also carries the previous frame's HZB tail)
    c->fuseCullFrame = false; c->fuseCullHzb = nullptr;
    if (rc) return rc;
    record(c, S_CULL);
    // buildHZB is fused into the raster: the tile kernel reduces every finished 64x64 tile to mips 0..5 of the
    // chain kept as history (and of the temporary chain stage 1 culls against); only the one-block tail remains.
    c->fuseHzb = true;
    c->fuseHzbSlot = next;
    c->fuseHzbTemp = haveHist && (c->hView.flags & CHORD_FLAG_HZB_CULL);
    ChordCountAndCmd rejected;
    int stage1 = 0;
    rc = chordvis_visibility_stage0(c, haveHist ? &hist : nullptr, post, &rejected, &stage1);   // :326
    c->fusedCullDone = false;
    record(c, S_STAGE0_END);
    c->shouldStage1 = stage1 != 0;
    if (!rc && stage1) {
        // buildHZB(min) :334 -- levels 0..5 came out of the tile kernel; the one-block tail (levels 6..) is reduced by the
        // blocks of the phase-1 cull themselves unless the chain does not fit their LDS budget (never for targets <= 4096^2)
        const ChordHZBDesc& hd = c->hzb[0].desc;
        uint32_t tailFloats = 0;
        for (uint32_t l = 6; l < hd.mipCount; l++) tailFloats += std::max(1u, hd.width >> l) * std::max(1u, hd.height >> l);
        c->hzbTailInCull = hd.mipCount > 6u && tailFloats <= 1408u && !(c->debugFlags & 131072u);
        if (!c->hzbTailInCull) launch_hzb_tail(c, c->hzb[0], false, false);
        record(c, S_HZB0);
        ChordHZB tmp = c->hzb[0].handle();
        rc = chordvis_visibility_stage1(c, &tmp, rejected);                           // :337
        c->hzbTailInCull = false;
        record(c, S_STAGE1_END);
    }
    c->fuseHzb = false;
    if (rc) return rc;
    // buildHZB(min,max,range) :343 -- mips 0..5 are written; the one-block tail (mips 6.., range) is carried by the next
    // frame's first kernel, or launched by whoever reads the chain first (flush_pending_tail)
    c->hzb[next].valid = true;
    c->hzb[next].uploaded = false;                                                    // (the tile kernel wrote it: the library's own chain)
    c->pendingTailSlot = next;
    record(c, S_HZBF);
    c->historySlot = next;                                                            // :489
    c->inFrame = false;
    c->lastFrameLaunches = (uint32_t)(c->launchCount - c->frameLaunchBase);
    return CHORDVIS_OK;
}

// Sharded frame.  The single-GPU frame with two differences: the tile kernel writes each tile's words to the
// tile's slot of the rank's chunk and its HZB texels (mips 0..5) to the tile's slots of the two exchange buffers, and after
// each all-gather a copy kernel (launch_hzb_untile) moves every rank's texels to their places in the chain.
//   phase a   clear .. stage 0 raster (owned tiles; fused reduction into the exchange slots)
//   [all-gather of the mid-frame exchange buffer -- only when phase a reported a second stage]
//   phase b   chain 0 from the exchanged texels, phase-1 cull (reduces mips 6.. itself), stage 1 raster
//   [all-gather of the end-of-frame exchange buffer (small) and of the visibility words (the image)]
//   phase c   row-major copy of the image + the history chain from the exchanged texels; ends the frame
// Hosts that let the image travel beside the next frame call chordvis_frame_phase_c_finish once the small exchange has landed
// and chordvis_frame_resolve_visibility whenever the image has.
// The sharded group cull's first half (optional: a frame that starts at phase a culls every group on every rank, as before).
//   phase cull   object pass + the group tests of this rank's range of count blocks -> rank-mask words in its chunk of the cull exchange buffer
//   [all-gather of the cull exchange buffer: chordvis_cull_exchange_ptr, chunk = chordvis_cull_exchange_chunk_bytes]
//   phase a      masks and block counts from the exchanged words, prefix + scatter (the rank's own list), then as above
static int frame_phase_cull_impl(ChordCtx* c)
{
    int rc = ready(c, "frame_phase_cull");
    if (rc) return rc;
    if (c->shard.ranks <= 1) return fail(c, CHORDVIS_E_INVALID, "frame_phase_cull: the context is not sharded");
    if (c->cullPhaseDone) return fail(c, CHORDVIS_E_INVALID, "frame_phase_cull: called twice without chordvis_frame_phase_a in between");
    if (!cull_shardable_config(c)) return fail(c, CHORDVIS_E_INVALID, "frame_phase_cull: the sharded cull needs 2..8 ranks and the flat cull mode (start the frame at chordvis_frame_phase_a instead)");
    if ((rc = ensure_cull_exchange(c))) return rc;       // (made by upload_scene / set_shard already: a no-op)
    begin_frame_stamps(c);
    if ((rc = begin_frame_clear(c))) return rc;
    record(c, S_CLEAR);
    launch_cull_masks(c);
    CHORD_HIP(c, hipGetLastError());
    c->cullPhaseDone = true;
    record(c, S_CULL);
    return CHORDVIS_OK;
}

static int frame_phase_a_impl(ChordCtx* c)
{
    int rc = ready(c, "frame_phase_a");
    if (rc) return rc;
    if (c->shard.ranks <= 1) return fail(c, CHORDVIS_E_INVALID, "frame_phase_a: the context is not sharded");
    if (c->cullPhaseDone) record(c, S_EXCH_CULL);       // time spent in the all-gather of the rank masks (the library's or the caller's)
    else {
        begin_frame_stamps(c);
        if ((rc = begin_frame_clear(c))) return rc;
        record(c, S_CLEAR);
    }
    ChordCountAndCmd post;
    // (the post-cull list is not handed out here: a rank writes only its own share of it; chordvis_last_frame_cmds, the read-back
    // and the tile marker make the full list when they are asked for it -- from the cull's own masks, which every rank holds for every group)
    c->lazyFullList = true;
    rc = chordvis_instance_culling(c, &post);                                        // (its first kernel carries the previous frame's HZB tail)
    c->lazyFullList = false;
    if (rc) return rc;
    record(c, S_CULL);
    ChordHZB hist;
    const bool haveHist = c->historySlot != 0;
    if (haveHist) hist = c->hzb[c->historySlot].handle();
    c->fuseHzb = true;
    c->fuseHzbSlot = c->historySlot == 1 ? 2 : 1;
    c->fuseHzbTemp = haveHist && (c->hView.flags & CHORD_FLAG_HZB_CULL);
    c->exchangeSlotsFresh = true;                        // (the fused tile kernel of this frame's passes writes the rank's exchange slots)
    ChordCountAndCmd rejected;
    int stage1 = 0;
    rc = chordvis_visibility_stage0(c, haveHist ? &hist : nullptr, post, &rejected, &stage1);
    c->fuseHzb = false;
    if (rc) return rc;
    c->shouldStage1 = stage1 != 0;
    c->lastRejected = from_handle(rejected);
    record(c, S_STAGE0_END);
    return CHORDVIS_OK;
}

// phase b: [mid-frame exchange buffer all-gathered by the caller] -> HZB chain 0 -> stage 1.
static int frame_phase_b_impl(ChordCtx* c)
{
    int rc = ready(c, "frame_phase_b");
    if (rc) return rc;
    if (!c->shouldStage1) return CHORDVIS_OK;
    record(c, S_EXCH_HZB);       // time spent in the all-gather of the mid-frame exchange buffer (the library's or the caller's)
    launch_hzb_untile(c, c->hzb[0], false);
    CHORD_HIP(c, hipGetLastError());
    {   // levels 6.. of the chain: reduced by the blocks of the phase-1 cull themselves when they fit (render_frame_impl)
        const ChordHZBDesc& hd = c->hzb[0].desc;
        uint32_t tailFloats = 0;
        for (uint32_t l = 6; l < hd.mipCount; l++) tailFloats += std::max(1u, hd.width >> l) * std::max(1u, hd.height >> l);
        c->hzbTailInCull = hd.mipCount > 6u && tailFloats <= 1408u && !(c->debugFlags & 131072u);
        if (!c->hzbTailInCull) launch_hzb_tail(c, c->hzb[0], false, false);
    }
    record(c, S_HZB0);
    ChordHZB tmp = c->hzb[0].handle();
    c->fuseHzb = true;
    c->fuseHzbTemp = false;
    rc = chordvis_visibility_stage1(c, &tmp, c->lastRejected.handle());
    c->fuseHzb = false;
    c->hzbTailInCull = false;
    if (rc) return rc;
    record(c, S_STAGE1_END);
    return CHORDVIS_OK;
}

// [end-of-frame exchange buffer all-gathered by the caller] -> the history chain; the frame is over.  Mips 0..5 are copied
// from the slots; the one-block tail (mips 6.., valid range from the tiles' pairs) rides on the next frame's first kernel, or
// is launched by whoever reads the chain first (flush_pending_tail) -- as in the single-GPU frame.
static int frame_phase_c_finish_impl(ChordCtx* c)
{
    int rc = ready(c, "frame_phase_c_finish");
    if (rc) return rc;
    if (c->shard.ranks <= 1) return fail(c, CHORDVIS_E_INVALID, "frame_phase_c_finish: the context is not sharded");
    // the history chain, the tiles' valid ranges and their loads come from the end-of-frame exchange slots, which only the fused
    // tile kernel of chordvis_frame_phase_a / _b writes: a frame rastered with the stand-alone passes has none to unpack
    if (!c->exchangeSlotsFresh) return fail(c, CHORDVIS_E_INVALID, "frame_phase_c: no chordvis_frame_phase_a in this frame -- the end-of-frame exchange slots are stale (a frame rastered with the stand-alone passes builds its history with chordvis_build_hzb from the resolved image)");
    c->exchangeSlotsFresh = false;
    const int next = c->historySlot == 1 ? 2 : 1;
    launch_hzb_untile(c, c->hzb[next], true);
    CHORD_HIP(c, hipGetLastError());
    c->pendingTailSlot = next;
    record(c, S_HZBF);
    c->historySlot = next;
    c->inFrame = false;
    c->lastFrameLaunches = (uint32_t)(c->launchCount - c->frameLaunchBase);
    return CHORDVIS_OK;
}

// phase c: [both end-of-frame all-gathers done by the caller] -> row-major copy of the image + the history chain.
static int frame_phase_c_impl(ChordCtx* c)
{
    int rc = ready(c, "frame_phase_c");
    if (rc) return rc;
    if (c->shard.ranks <= 1) return fail(c, CHORDVIS_E_INVALID, "frame_phase_c: the context is not sharded");
    record(c, S_EXCH_VIS);       // time spent in the end-of-frame all-gathers
    launch_detile(c);
    CHORD_HIP(c, hipGetLastError());
    return frame_phase_c_finish_impl(c);
}

// A failed frame must not leave frame-scoped state behind (the stand-alone passes that may follow would skip their
// count resets, a later frame would inherit a fused-HZB request).
static int end_failed_frame(ChordCtx* c, int rc)
{
    if (rc && c) {
        if (c->zeroFrameStateInCull) { (void)hipMemsetAsync(c->dFrameState, 0, c->frameStateZeroBytes, c->stream); c->zeroFrameStateInCull = false; }
        c->inFrame = false; c->fuseHzb = false; c->pendingClear = false; c->shouldStage1 = false; c->cullPhaseDone = false; c->exchangeSlotsFresh = false;
    }
    return rc;
}
int chordvis_render_frame(ChordCtx* c) { return end_failed_frame(c, render_frame_impl(c)); }
int chordvis_frame_phase_cull(ChordCtx* c) { return end_failed_frame(c, frame_phase_cull_impl(c)); }
int chordvis_frame_phase_a(ChordCtx* c) { return end_failed_frame(c, frame_phase_a_impl(c)); }
int chordvis_frame_phase_b(ChordCtx* c) { return end_failed_frame(c, frame_phase_b_impl(c)); }
int chordvis_frame_phase_c(ChordCtx* c) { return end_failed_frame(c, frame_phase_c_impl(c)); }
int chordvis_frame_phase_c_finish(ChordCtx* c) { return end_failed_frame(c, frame_phase_c_finish_impl(c)); }

// The row-major copy of the (gathered) rank-major visibility words of the CURRENT buffer pair, on `hipStream` (NULL: the
// context's stream) -- phase c's first half, for pipelined hosts that run it beside the next frame.
int chordvis_frame_resolve_visibility(ChordCtx* c, void* hipStream)
{
    if (!c || !c->dVis || c->shard.ranks <= 1) return fail(c, CHORDVIS_E_INVALID, "frame_resolve_visibility: a sharded context with a gbuffer");
    launch_detile(c, (hipStream_t)hipStream);
    CHORD_HIP(c, hipGetLastError());
    return CHORDVIS_OK;
}

// Orders `hipStream` (NULL: the context's stream) behind the completion of the resolved image of the last submitted frame.
// Needed only after pipelined ChordGroup frames, whose image is gathered beside the context's stream; a no-op otherwise.
int chordvis_wait_visibility(ChordCtx* c, void* hipStream)
{
    if (!c || !c->dVis) return fail(c, CHORDVIS_E_INVALID, "wait_visibility: no gbuffer");
    hipStream_t s = hipStream ? (hipStream_t)hipStream : c->stream;
    if (c->visReadyEvent[0]) CHORD_HIP(c, hipStreamWaitEvent(s, c->visReadyEvent[0], 0));
    else if (s != c->stream) {
        // not pipelined: the image is complete when the context's stream is; order the foreign stream behind it
        hipEvent_t e = nullptr;
        CHORD_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        hipError_t rc = hipEventRecord(e, c->stream);
        if (rc == hipSuccess) rc = hipStreamWaitEvent(s, e, 0);
        (void)hipEventDestroy(e);                                    // (destruction is deferred until the event has completed)
        if (rc != hipSuccess) return fail(c, CHORDVIS_E_HIP, "wait_visibility", rc);
    }
    return CHORDVIS_OK;
}

int chordvis_last_frame_cmds(ChordCtx* c, ChordCountAndCmd* out)
{
    if (!c || !out || !c->sceneLoaded) return fail(c, CHORDVIS_E_INVALID, "last_frame_cmds: no scene");
    launch_full_list(c);                                             // (a sharded frame wrote only the rank's share of it)
    CHORD_HIP(c, hipGetLastError());
    *out = c->lists[0].handle();
    return CHORDVIS_OK;
}

int chordvis_history_hzb(ChordCtx* c, ChordHZB* out)
{
    if (!c || !out || c->historySlot == 0) return fail(c, CHORDVIS_E_INVALID, "history_hzb: no history yet");
    { const int rc = flush_pending_tail(c); if (rc) return rc; }
    *out = c->hzb[c->historySlot].handle();
    return CHORDVIS_OK;
}

// ------------------------------------------------------------------------ tile marker (8f-1) --

int chordvis_visibility_mark(ChordCtx* c, ChordCountAndCmd drawed, ChordTileMarker* out)
{
    if (!c || !out || !c->dVis || !c->sceneLoaded) return fail(c, CHORDVIS_E_INVALID, "visibility_mark: no scene / gbuffer");
    if (!drawed.count || !drawed.cmds) return fail(c, CHORDVIS_E_INVALID, "visibility_mark: null command list");
    if (drawed.cmds == c->lists[0].cmds) { launch_full_list(c); CHORD_HIP(c, hipGetLastError()); }
    const uint32_t mW = (c->width + 7u) / 8u, mH = (c->height + 7u) / 8u;
    int rc;
    if (!c->dTileMarker) {
        if ((rc = dalloc(c, &c->dTileMarker, (size_t)mW * mH * 4))) return rc;
        if ((rc = dalloc(c, &c->dShadingTiles, (size_t)mW * mH * 2 + 8))) return rc;
    }
    const unsigned long long* vis = (const unsigned long long*)(c->shard.ranks > 1 ? c->dVisResolved : c->dVis);
    // (pipelined group frames: the image is gathered and resolved beside the context's stream)
    if (c->visReadyEvent[0]) CHORD_HIP(c, hipStreamWaitEvent(c->stream, c->visReadyEvent[0], 0));
    chord::launch_visibility_mark(c, vis, drawed.cmds, drawed.count, c->dTileMarker);
    CHORD_HIP(c, hipGetLastError());
    out->marker = c->dTileMarker;
    out->visibilityDim[0] = c->width; out->visibilityDim[1] = c->height;
    out->markerDim[0] = mW; out->markerDim[1] = mH;
    return CHORDVIS_OK;
}

// ---------------------------------------------------------------- per-pixel attributes of the visible triangle --

// The preconditions chordvis_resolve_attributes and chordvis_resolve_surface share, in this order: a scene and gbuffer, a frame
// since, no update_objects / set_view after it, a command list, a target, debugMode within range.  `fn` names the entry point in
// the messages.
static int resolve_checks(ChordCtx* c, const char* fn, ChordCountAndCmd drawed, bool anyTarget, bool wantDebug, const ChordResolveDesc& d)
{
    char buf[224];
    auto refuse = [&](const char* why) { std::snprintf(buf, sizeof(buf), "%s: %s", fn, why); return fail(c, CHORDVIS_E_INVALID, buf); };
    if (!c || !c->dVis || !c->sceneLoaded) return refuse("no scene / gbuffer");
    if (!c->resolveFrame) return refuse("no frame rendered yet");
    if (c->resolveStale) return refuse("chordvis_update_objects / chordvis_bind_objects / chordvis_set_view came after the frame (the image's matrices are gone)");
    if (!drawed.count || !drawed.cmds) return refuse("null command list");
    if (!anyTarget) return refuse("no target");
    if (wantDebug && d.debugMode > CHORD_NANITE_DEBUG_BARYCENTRICS) return refuse("debugMode beyond 4");
    return CHORDVIS_OK;
}

// What both do before their launch: the full list's fill when the list is the frame's, and the wait for a pipelined frame's
// gather.  *vis = the image chordvis_visibility_mark reads (the resolved one of a sharded context).
static int resolve_source(ChordCtx* c, ChordCountAndCmd drawed, const unsigned long long** vis)
{
    if (drawed.cmds == c->lists[0].cmds) { launch_full_list(c); CHORD_HIP(c, hipGetLastError()); }
    *vis = (const unsigned long long*)(c->shard.ranks > 1 ? c->dVisResolved : c->dVis);
    // (pipelined group frames: the image is gathered and resolved beside the context's stream)
    if (c->visReadyEvent[0]) CHORD_HIP(c, hipStreamWaitEvent(c->stream, c->visReadyEvent[0], 0));
    return CHORDVIS_OK;
}

static bool any_resolve_target(const ChordResolveTargets& t)
{
    return t.barycentrics || t.baryDdx || t.baryDdy || t.uv || t.uvGrad || t.positionRS || t.motionVector || t.debugRGBA8;
}

int chordvis_resolve_attributes(ChordCtx* c, ChordCountAndCmd drawed, const ChordResolveDesc* desc, const ChordResolveTargets* t)
{
    const ChordResolveTargets tt = t ? *t : ChordResolveTargets{};
    const ChordResolveDesc d = desc ? *desc : ChordResolveDesc{};
    int rc = resolve_checks(c, "resolve_attributes", drawed, any_resolve_target(tt), tt.debugRGBA8 != nullptr, d);
    const unsigned long long* vis = nullptr;
    if (rc || (rc = resolve_source(c, drawed, &vis))) return rc;
    chord::launch_resolve_attributes(c, vis, drawed.cmds, drawed.count, d, tt);
    CHORD_HIP(c, hipGetLastError());
    return CHORDVIS_OK;
}

// chordvis_resolve_attributes' preconditions and refusals, then those of the surface streams the targets need
int chordvis_resolve_surface(ChordCtx* c, ChordCountAndCmd drawed, const ChordResolveDesc* desc, const ChordResolveTargets* t,
                             const ChordSurfaceTargets* s)
{
    const ChordResolveTargets tt = t ? *t : ChordResolveTargets{};
    const ChordSurfaceTargets ss = s ? *s : ChordSurfaceTargets{};
    const ChordResolveDesc d = desc ? *desc : ChordResolveDesc{};
    const bool anySurface = ss.vertexNormal || ss.tangent || ss.bitangent;
    int rc = resolve_checks(c, "resolve_surface", drawed, any_resolve_target(tt) || anySurface, tt.debugRGBA8 != nullptr, d);
    if (rc) return rc;
    if (ss.pad) return fail(c, CHORDVIS_E_INVALID, "resolve_surface: ChordSurfaceTargets::pad must be NULL");
    if ((ss.tangent || ss.bitangent) && !c->dTangents)
        return fail(c, CHORDVIS_E_INVALID, "resolve_surface: the scene was uploaded without tangents (ChordAssetDesc::tangents)");
    if (anySurface && !c->dNormals)
        return fail(c, CHORDVIS_E_INVALID, "resolve_surface: the scene was uploaded without normals (ChordAssetDesc::normals)");
    const unsigned long long* vis = nullptr;
    if ((rc = resolve_source(c, drawed, &vis))) return rc;
    chord::launch_resolve_surface(c, vis, drawed.cmds, drawed.count, d, tt, ss);
    CHORD_HIP(c, hipGetLastError());
    return CHORDVIS_OK;
}

// What chordvis_resolve_material refuses beyond resolve_checks, in its order: the surface streams the targets need, then the material
// images' own preconditions.  `fn` names the entry point in the messages (chordvis_resolve_gbuffer asks the same of its targets).
static int material_checks(ChordCtx* c, const char* fn, const ChordSurfaceTargets& ss, const ChordMaterialTargets& mm)
{
    char buf[224];
    auto refuse = [&](const char* why) { std::snprintf(buf, sizeof(buf), "%s: %s", fn, why); return fail(c, CHORDVIS_E_INVALID, buf); };
    const bool anySurface = ss.vertexNormal || ss.tangent || ss.bitangent;
    const bool anyMaterial = mm.baseColor || mm.emissive || mm.pixelNormal || mm.roughMetalAO;
    if (ss.pad) return refuse("ChordSurfaceTargets::pad must be NULL");
    if ((ss.tangent || ss.bitangent) && !c->dTangents) return refuse("the scene was uploaded without tangents (ChordAssetDesc::tangents)");
    if (anySurface && !c->dNormals) return refuse("the scene was uploaded without normals (ChordAssetDesc::normals)");
    if (anyMaterial && !c->matTexturesLoaded) return refuse("no chordvis_upload_material_textures since the last chordvis_upload_scene");
    if (mm.pixelNormal && !c->dNormals) return refuse("pixelNormal needs a scene uploaded with normals (ChordAssetDesc::normals)");
    if (mm.pixelNormal && c->matAnyNormalTexture && !c->dTangents)
        return refuse("pixelNormal with a normal texture needs a scene uploaded with tangents (ChordAssetDesc::tangents)");
    return CHORDVIS_OK;
}

// chordvis_resolve_surface's preconditions and refusals, then those of the material images
int chordvis_resolve_material(ChordCtx* c, ChordCountAndCmd drawed, const ChordResolveDesc* desc, const ChordResolveTargets* t,
                              const ChordSurfaceTargets* s, const ChordMaterialTargets* m)
{
    const ChordResolveTargets tt = t ? *t : ChordResolveTargets{};
    const ChordSurfaceTargets ss = s ? *s : ChordSurfaceTargets{};
    const ChordMaterialTargets mm = m ? *m : ChordMaterialTargets{};
    const ChordResolveDesc d = desc ? *desc : ChordResolveDesc{};
    const bool anySurface = ss.vertexNormal || ss.tangent || ss.bitangent;
    const bool anyMaterial = mm.baseColor || mm.emissive || mm.pixelNormal || mm.roughMetalAO;
    int rc = resolve_checks(c, "resolve_material", drawed, any_resolve_target(tt) || anySurface || anyMaterial, tt.debugRGBA8 != nullptr, d);
    if (rc || (rc = material_checks(c, "resolve_material", ss, mm))) return rc;
    const unsigned long long* vis = nullptr;
    if ((rc = resolve_source(c, drawed, &vis))) return rc;
    chord::launch_resolve_material(c, vis, drawed.cmds, drawed.count, d, tt, chord::MaterialLaunch{ss, mm});
    CHORD_HIP(c, hipGetLastError());
    return CHORDVIS_OK;
}

int chordvis_material_feedback_reset(ChordCtx* c)
{
    if (!c) return CHORDVIS_E_INVALID;
    if (!c->matTexturesLoaded) return fail(c, CHORDVIS_E_INVALID, "material_feedback_reset: no chordvis_upload_material_textures since the last chordvis_upload_scene");
    (void)hipSetDevice(c->device);
    const size_t words = c->matTex.size() * CHORD_FEEDBACK_LEVELS;
    int rc;
    if (!c->dMatFeedback && (rc = dalloc(c, &c->dMatFeedback, words))) return rc;
    CHORD_HIP(c, hipMemsetAsync(c->dMatFeedback, 0, std::max<size_t>(words, 1u) * 4u, c->stream));
    return CHORDVIS_OK;
}

// chordvis_resolve_material's preconditions when asked for a material target other than pixelNormal, then the pass's own
int chordvis_material_feedback(ChordCtx* c, ChordCountAndCmd drawed, const ChordFeedbackDesc* desc)
{
    int rc = resolve_checks(c, "material_feedback", drawed, true, false, ChordResolveDesc{});
    if (rc) return rc;
    if (!c->matTexturesLoaded) return fail(c, CHORDVIS_E_INVALID, "material_feedback: no chordvis_upload_material_textures since the last chordvis_upload_scene");
    if (!c->dMatFeedback) return fail(c, CHORDVIS_E_INVALID, "material_feedback: no chordvis_material_feedback_reset since the last chordvis_upload_material_textures");
    if (!desc) return fail(c, CHORDVIS_E_INVALID, "material_feedback: null ChordFeedbackDesc");
    if (desc->slotMask == 0u || desc->slotMask > 15u)
        return fail(c, CHORDVIS_E_INVALID, "material_feedback: slotMask is 1..15 (CHORD_FEEDBACK_BASECOLOR 1 | EMISSIVE 2 | NORMAL 4 | METALROUGH 8)");
    if (desc->stride != 1u && desc->stride != 2u && desc->stride != 4u && desc->stride != 8u)
        return fail(c, CHORDVIS_E_INVALID, "material_feedback: stride is 1, 2, 4 or 8");
    if (desc->offset[0] >= desc->stride || desc->offset[1] >= desc->stride)
        return fail(c, CHORDVIS_E_INVALID, "material_feedback: each offset is 0 .. stride - 1");
    const unsigned long long* vis = nullptr;
    if ((rc = resolve_source(c, drawed, &vis))) return rc;
    chord::launch_material_feedback(c, vis, drawed.cmds, drawed.count, *desc, c->dMatFeedback, (uint32_t)c->matTex.size());
    CHORD_HIP(c, hipGetLastError());
    return CHORDVIS_OK;
}

int chordvis_readback_material_feedback(ChordCtx* c, uint32_t* hostTaps, uint32_t textureCount)
{
    if (!c || !hostTaps) return fail(c, CHORDVIS_E_INVALID, "readback_material_feedback: null argument");
    if (!c->matTexturesLoaded) return fail(c, CHORDVIS_E_INVALID, "readback_material_feedback: no chordvis_upload_material_textures since the last chordvis_upload_scene");
    if (!c->dMatFeedback) return fail(c, CHORDVIS_E_INVALID, "readback_material_feedback: no chordvis_material_feedback_reset since the last chordvis_upload_material_textures");
    if (textureCount != c->matTex.size()) {
        char buf[160];
        std::snprintf(buf, sizeof(buf), "readback_material_feedback: textureCount is the uploaded descriptor's, %u", (unsigned)c->matTex.size());
        return fail(c, CHORDVIS_E_INVALID, buf);
    }
    (void)hipSetDevice(c->device);
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    if (textureCount) CHORD_HIP(c, hipMemcpy(hostTaps, c->dMatFeedback, (size_t)textureCount * CHORD_FEEDBACK_LEVELS * 4u, hipMemcpyDeviceToHost));
    return CHORDVIS_OK;
}

// ---------------------------------------------------------------- geometry feedback (kernels_geometry.hip) --

int chordvis_geometry_feedback_reset(ChordCtx* c)
{
    if (!c) return CHORDVIS_E_INVALID;
    if (!c->sceneLoaded) return fail(c, CHORDVIS_E_INVALID, "geometry_feedback_reset: no scene (call chordvis_upload_scene first)");
    (void)hipSetDevice(c->device);
    if (!c->dGeoFeedback) {
        const uint64_t O = c->objectCount, P = (uint64_t)c->primCount * CHORD_GEOMETRY_LODS, B = ((uint64_t)c->cmdCapacity + 31u) / 32u, G = (B + 255u) / 256u;
        const uint64_t words = 3u * O + 3u * P + 4u + B + G;
        if (words >= 0xFFFFFFFFull || c->cmdCapacity > 0xFFFFFF00u) return fail(c, CHORDVIS_E_CAPACITY, "geometry_feedback_reset: more than 2^32 words of counts");
        chord::GeoLayout& l = c->geoLayout;
        l.objectPixels = 0u; l.objectSubmitted = (uint32_t)O; l.objectVisible = (uint32_t)(2u * O);
        l.lodPixels = (uint32_t)(3u * O); l.lodSubmitted = (uint32_t)(3u * O + P); l.lodVisible = (uint32_t)(3u * O + 2u * P);
        l.totals = (uint32_t)(3u * O + 3u * P);
        l.seen = l.totals + 4u; l.seenWords = (uint32_t)B;
        l.groupCounts = l.seen + l.seenWords; l.groups = (uint32_t)G;
        l.words = (uint32_t)words;
        int rc;
        if ((rc = dalloc(c, &c->dGeoFeedback, (size_t)words))) return rc;
    }
    CHORD_HIP(c, hipMemsetAsync(c->dGeoFeedback, 0, (size_t)c->geoLayout.words * 4u, c->stream));
    c->geoFeedbackCmds = nullptr;
    return CHORDVIS_OK;
}

// chordvis_resolve_attributes' preconditions, then the pass's own
int chordvis_geometry_feedback(ChordCtx* c, ChordCountAndCmd drawed, const ChordGeometryFeedbackDesc* desc)
{
    int rc = resolve_checks(c, "geometry_feedback", drawed, true, false, ChordResolveDesc{});
    if (rc) return rc;
    if (!c->dGeoFeedback) return fail(c, CHORDVIS_E_INVALID, "geometry_feedback: no chordvis_geometry_feedback_reset since the last chordvis_upload_scene");
    if (!desc) return fail(c, CHORDVIS_E_INVALID, "geometry_feedback: null ChordGeometryFeedbackDesc");
    if (desc->stride != 1u && desc->stride != 2u && desc->stride != 4u && desc->stride != 8u)
        return fail(c, CHORDVIS_E_INVALID, "geometry_feedback: stride is 1, 2, 4 or 8");
    if (desc->offset[0] >= desc->stride || desc->offset[1] >= desc->stride)
        return fail(c, CHORDVIS_E_INVALID, "geometry_feedback: each offset is 0 .. stride - 1");
    if (desc->pad) return fail(c, CHORDVIS_E_INVALID, "geometry_feedback: pad is 0");
    const unsigned long long* vis = nullptr;
    if ((rc = resolve_source(c, drawed, &vis))) return rc;
    // the bitmap is the latest call's
    CHORD_HIP(c, hipMemsetAsync(c->dGeoFeedback + c->geoLayout.seen, 0, (size_t)c->geoLayout.seenWords * 4u, c->stream));
    chord::launch_geometry_feedback(c, vis, drawed.cmds, drawed.count, *desc);
    CHORD_HIP(c, hipGetLastError());
    c->geoFeedbackCmds = drawed.cmds;
    return CHORDVIS_OK;
}

int chordvis_readback_geometry_feedback(ChordCtx* c, const ChordGeometryFeedback* out, uint32_t objectCount, uint32_t primitiveCount)
{
    if (!c || !out) return fail(c, CHORDVIS_E_INVALID, "readback_geometry_feedback: null argument");
    if (!c->sceneLoaded || !c->dGeoFeedback)
        return fail(c, CHORDVIS_E_INVALID, "readback_geometry_feedback: no chordvis_geometry_feedback_reset since the last chordvis_upload_scene");
    if (objectCount != c->objectCount || primitiveCount != c->primCount) {
        char buf[192];
        std::snprintf(buf, sizeof(buf), "readback_geometry_feedback: objectCount and primitiveCount are the uploaded scene's, %u and %u",
                      (unsigned)c->objectCount, (unsigned)c->primCount);
        return fail(c, CHORDVIS_E_INVALID, buf);
    }
    (void)hipSetDevice(c->device);
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    const chord::GeoLayout& l = c->geoLayout;
    const size_t lodWords = (size_t)primitiveCount * CHORD_GEOMETRY_LODS;
    const struct { uint32_t* host; uint32_t at; size_t words; } copies[7] = {
        {out->objectPixels, l.objectPixels, objectCount}, {out->objectSubmitted, l.objectSubmitted, objectCount}, {out->objectVisible, l.objectVisible, objectCount},
        {out->lodPixels, l.lodPixels, lodWords}, {out->lodSubmitted, l.lodSubmitted, lodWords}, {out->lodVisible, l.lodVisible, lodWords},
        {out->totals, l.totals, 4u}};
    for (const auto& cp : copies)
        if (cp.host && cp.words) CHORD_HIP(c, hipMemcpy(cp.host, c->dGeoFeedback + cp.at, cp.words * 4u, hipMemcpyDeviceToHost));
    return CHORDVIS_OK;
}

int chordvis_visible_clusters(ChordCtx* c, ChordCountAndCmd drawed, ChordDrawCmd* deviceOut, uint32_t* deviceCount, uint32_t capacity)
{
    if (!c || !c->sceneLoaded) return fail(c, CHORDVIS_E_INVALID, "visible_clusters: no scene");
    if (!drawed.count || !drawed.cmds) return fail(c, CHORDVIS_E_INVALID, "visible_clusters: null command list");
    if (!deviceCount || (!deviceOut && capacity)) return fail(c, CHORDVIS_E_INVALID, "visible_clusters: null output (deviceOut may be null only with capacity 0)");
    if (!c->dGeoFeedback || !c->geoFeedbackCmds)
        return fail(c, CHORDVIS_E_INVALID, "visible_clusters: no chordvis_geometry_feedback since the last chordvis_geometry_feedback_reset / chordvis_upload_scene");
    if (drawed.cmds != c->geoFeedbackCmds)
        return fail(c, CHORDVIS_E_INVALID, "visible_clusters: the list is not the one the latest chordvis_geometry_feedback was given");
    (void)hipSetDevice(c->device);
    chord::launch_visible_clusters(c, drawed.cmds, drawed.count, deviceOut, deviceCount, capacity);
    CHORD_HIP(c, hipGetLastError());
    return CHORDVIS_OK;
}

int chordvis_query_bounds(ChordCtx* c, const ChordHZB* hzb, int phase, const ChordBoundsQuery* deviceQueries, uint32_t count,
                          ChordBoundsResult* deviceResults, uint32_t* deviceVisible, uint32_t* deviceVisibleCount, uint32_t capacity)
{
    if (!c) return CHORDVIS_E_INVALID;
    if (!c->viewSet) return fail(c, CHORDVIS_E_INVALID, "query_bounds: no view set (chordvis_set_view comes first)");
    if (phase != 0 && phase != 1) return fail(c, CHORDVIS_E_INVALID, "query_bounds: phase is 0 (last frame's matrices) or 1");
    if (count && !deviceQueries) return fail(c, CHORDVIS_E_INVALID, "query_bounds: deviceQueries is NULL with count > 0");
    if (!deviceResults && !deviceVisible && !deviceVisibleCount) return fail(c, CHORDVIS_E_INVALID, "query_bounds: all three outputs are NULL");
    if (capacity && !deviceVisible) return fail(c, CHORDVIS_E_INVALID, "query_bounds: deviceVisible is NULL with capacity > 0");
    if (count > 0x80000000u) return fail(c, CHORDVIS_E_INVALID, "query_bounds: at most 2^31 queries per call");
    if (((uintptr_t)deviceQueries | (uintptr_t)deviceResults) & 15u)
        return fail(c, CHORDVIS_E_INVALID, "query_bounds: deviceQueries and deviceResults must be 16-byte aligned");
    if (hzb) {
        if (!hzb->minTexels) return fail(c, CHORDVIS_E_INVALID, "query_bounds: hzb given with minTexels NULL");
        ChordHZBDesc want;
        if (chordvis_hzb_desc(c->hView.width, c->hView.height, &want) != CHORDVIS_OK || std::memcmp(&want, &hzb->desc, sizeof(want)) != 0)
            return fail(c, CHORDVIS_E_INVALID, "query_bounds: hzb->desc is not chordvis_hzb_desc(view width, view height): the main-view test has no level clamp");
        if (c->hView.view.renderDimension[0] != c->hView.iv.renderDimension[0] || c->hView.view.renderDimension[1] != c->hView.iv.renderDimension[1])
            return fail(c, CHORDVIS_E_INVALID, "query_bounds: the view's ChordCameraView::renderDimension differs from its ChordInstanceCullingView::renderDimension");
    }
    (void)hipSetDevice(c->device);
    if (count == 0) {
        if (deviceVisibleCount) CHORD_HIP(c, hipMemsetAsync(deviceVisibleCount, 0, 4, c->stream));
        return CHORDVIS_OK;
    }
    { const int rc = flush_pending_tail(c); if (rc) return rc; }
    const uint32_t words = chord::bounds_query_scratch_words(count);
    if (words > c->boundsScratchWords) {
        // (an earlier call on the stream may still be reading the scratch that is about to go)
        CHORD_HIP(c, hipStreamSynchronize(c->stream));
        c->boundsScratchWords = 0;
        const int rc = dalloc(c, &c->dBoundsScratch, (size_t)words);
        if (rc) return rc;
        c->boundsScratchWords = words;
    }
    chord::launch_bounds_query(c, hzb, phase, deviceQueries, count, deviceResults, deviceVisible, deviceVisibleCount, capacity, c->dBoundsScratch);
    CHORD_HIP(c, hipGetLastError());
    return CHORDVIS_OK;
}

uint32_t chordvis_bounds_tile_count(uint32_t width, uint32_t height, uint32_t tileSize, uint32_t* tilesX, uint32_t* tilesY)
{
    uint64_t tx = 0, ty = 0;
    if (tileSize == 8u || tileSize == 16u || tileSize == 32u || tileSize == 64u) {
        tx = ((uint64_t)width + tileSize - 1u) / tileSize; ty = ((uint64_t)height + tileSize - 1u) / tileSize;
        if (tx * ty > 0xFFFFFFFFull) tx = ty = 0;
    }
    if (tilesX) *tilesX = (uint32_t)tx;
    if (tilesY) *tilesY = (uint32_t)ty;
    return (uint32_t)(tx * ty);
}

int chordvis_bin_bounds(ChordCtx* c, const ChordBoundsTilesDesc* desc, const ChordBoundsResult* deviceResults, const ChordBoundsQuery* deviceQueries,
                        uint32_t count, const ChordBoundsTiles* out)
{
    if (!c) return CHORDVIS_E_INVALID;
    if (!desc || !out) return fail(c, CHORDVIS_E_INVALID, "bin_bounds: desc or out is NULL");
    if (!out->tileCounts && !out->tileItems && !out->tileDepth && !out->totals) return fail(c, CHORDVIS_E_INVALID, "bin_bounds: all four outputs are NULL");
    if (desc->tileSize != 8u && desc->tileSize != 16u && desc->tileSize != 32u && desc->tileSize != 64u)
        return fail(c, CHORDVIS_E_INVALID, "bin_bounds: tileSize is 8, 16, 32 or 64");
    if (desc->flags & ~(CHORD_BOUNDS_TILES_NEAR | CHORD_BOUNDS_TILES_FAR)) return fail(c, CHORDVIS_E_INVALID, "bin_bounds: unknown flags bits");
    if (desc->phase > 1u) return fail(c, CHORDVIS_E_INVALID, "bin_bounds: phase is 0 (last frame's matrices) or 1");
    const bool farSide = (desc->flags & CHORD_BOUNDS_TILES_FAR) != 0u;
    if (farSide && !deviceQueries) return fail(c, CHORDVIS_E_INVALID, "bin_bounds: CHORD_BOUNDS_TILES_FAR needs deviceQueries");
    if (count && !deviceResults) return fail(c, CHORDVIS_E_INVALID, "bin_bounds: deviceResults is NULL with count > 0");
    if (out->tileItems && desc->maxPerTile == 0u) return fail(c, CHORDVIS_E_INVALID, "bin_bounds: tileItems given with maxPerTile == 0");
    if (((uintptr_t)deviceResults | (uintptr_t)deviceQueries) & 15u)
        return fail(c, CHORDVIS_E_INVALID, "bin_bounds: deviceResults and deviceQueries must be 16-byte aligned");
    if (!c->dVis) return fail(c, CHORDVIS_E_INVALID, "bin_bounds: no G-buffer allocated (chordvis_allocate_gbuffer comes first)");
    if (!c->viewSet) return fail(c, CHORDVIS_E_INVALID, "bin_bounds: no view set (chordvis_set_view comes first)");
    {
        const float W = (float)c->width, H = (float)c->height;
        const ChordCameraView& v = c->hView.view; const ChordInstanceCullingView& iv = c->hView.iv;
        if (v.renderDimension[0] != W || v.renderDimension[1] != H || iv.renderDimension[0] != W || iv.renderDimension[1] != H)
            return fail(c, CHORDVIS_E_INVALID, "bin_bounds: the view's renderDimension differs from the image's size");
    }
    const uint32_t tiles = chordvis_bounds_tile_count(c->width, c->height, desc->tileSize, nullptr, nullptr);
    if ((uint64_t)tiles * desc->maxPerTile > 0xFFFFFFFFull) return fail(c, CHORDVIS_E_INVALID, "bin_bounds: tiles * maxPerTile is beyond 2^32 - 1");
    (void)hipSetDevice(c->device);
    // the lists are wanted: the records that take part go through the scratch (tileDepth alone reads no record)
    const bool lists = count && (out->tileCounts || out->tileItems || out->totals);
    if (lists) {
        const size_t words = chord::bounds_tiles_scratch_words(count, chord::bounds_tiles_blocks(c->width, c->height));
        if (words > c->boundsTilesScratchWords) {
            // (an earlier call on the stream may still be reading the scratch that is about to go)
            CHORD_HIP(c, hipStreamSynchronize(c->stream));
            c->boundsTilesScratchWords = 0;
            const int rc = dalloc(c, &c->dBoundsTilesScratch, words);
            if (rc) return rc;
            c->boundsTilesScratchWords = words;
        }
    }
    const unsigned long long* vis = (const unsigned long long*)(c->shard.ranks > 1 ? c->dVisResolved : c->dVis);
    // (pipelined group frames: the image is gathered and resolved beside the context's stream)
    if (c->visReadyEvent[0]) CHORD_HIP(c, hipStreamWaitEvent(c->stream, c->visReadyEvent[0], 0));
    if (out->totals && !lists) CHORD_HIP(c, hipMemsetAsync(out->totals, 0, 16, c->stream));    // (with records the launches write all four)
    if (lists) chord::launch_bounds_tiles_prepare(c, *desc, deviceResults, deviceQueries, count, c->dBoundsTilesScratch, out->totals);
    chord::launch_bounds_tiles(c, vis, *desc, count, lists, c->dBoundsTilesScratch, *out);
    CHORD_HIP(c, hipGetLastError());
    return CHORDVIS_OK;
}

int chordvis_geometry_feedback_seen(ChordCtx* c, uint32_t* hostWords, uint32_t wordCount)
{
    if (!c || !hostWords) return fail(c, CHORDVIS_E_INVALID, "geometry_feedback_seen: null argument");
    if (!c->sceneLoaded || !c->dGeoFeedback)
        return fail(c, CHORDVIS_E_INVALID, "geometry_feedback_seen: no chordvis_geometry_feedback_reset since the last chordvis_upload_scene");
    if (wordCount != c->geoLayout.seenWords) {
        char buf[160];
        std::snprintf(buf, sizeof(buf), "geometry_feedback_seen: wordCount is ceil(capacity / 32), %u", (unsigned)c->geoLayout.seenWords);
        return fail(c, CHORDVIS_E_INVALID, buf);
    }
    (void)hipSetDevice(c->device);
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    CHORD_HIP(c, hipMemcpy(hostWords, c->dGeoFeedback + c->geoLayout.seen, (size_t)wordCount * 4u, hipMemcpyDeviceToHost));
    return CHORDVIS_OK;
}

static bool misaligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1u)) != 0u; }

// the alignment chordvis_resolve_gbuffer and chordvis_pack_gbuffer ask of the packed images: null when every target is aligned
static const char* gbuffer_target_misaligned(const ChordGBufferTargets& g)
{
    if (misaligned(g.baseColor, 4) || misaligned(g.vertexNormal, 4) || misaligned(g.pixelNormal, 4) || misaligned(g.motionVector, 4) ||
        misaligned(g.aoRoughnessMetallic, 4))
        return "a uint32 target is not 4-byte aligned";
    if (misaligned(g.emissive, 8)) return "the emissive target is not 8-byte aligned";
    return nullptr;
}

static bool any_gbuffer_target(const ChordGBufferTargets& g)
{
    return g.baseColor || g.vertexNormal || g.pixelNormal || g.motionVector || g.aoRoughnessMetallic || g.emissive;
}

// chordvis_resolve_material's preconditions and refusals for the float twins of the targets, then the alignment of the packed ones
int chordvis_resolve_gbuffer(ChordCtx* c, ChordCountAndCmd drawed, const ChordResolveDesc* desc, const ChordGBufferTargets* g)
{
    const ChordGBufferTargets gg = g ? *g : ChordGBufferTargets{};
    const ChordResolveDesc d = desc ? *desc : ChordResolveDesc{};
    int rc = resolve_checks(c, "resolve_gbuffer", drawed, any_gbuffer_target(gg), false, d);
    if (rc) return rc;
    ChordSurfaceTargets ss = {};
    ChordMaterialTargets mm = {};
    ss.vertexNormal = reinterpret_cast<float*>(gg.vertexNormal);
    mm.baseColor = reinterpret_cast<float*>(gg.baseColor); mm.emissive = reinterpret_cast<float*>(gg.emissive);
    mm.pixelNormal = reinterpret_cast<float*>(gg.pixelNormal); mm.roughMetalAO = reinterpret_cast<float*>(gg.aoRoughnessMetallic);
    if ((rc = material_checks(c, "resolve_gbuffer", ss, mm))) return rc;
    if (const char* why = gbuffer_target_misaligned(gg)) {
        char buf[96];
        std::snprintf(buf, sizeof(buf), "resolve_gbuffer: %s", why);
        return fail(c, CHORDVIS_E_INVALID, buf);
    }
    const unsigned long long* vis = nullptr;
    if ((rc = resolve_source(c, drawed, &vis))) return rc;
    chord::launch_resolve_gbuffer(c, vis, drawed.cmds, drawed.count, d, gg);
    CHORD_HIP(c, hipGetLastError());
    return CHORDVIS_OK;
}

int chordvis_pack_gbuffer(ChordCtx* c, uint32_t width, uint32_t height, const ChordGBufferSources* s, const ChordGBufferTargets* g)
{
    if (!c) return CHORDVIS_E_INVALID;
    const ChordGBufferSources ss = s ? *s : ChordGBufferSources{};
    const ChordGBufferTargets gg = g ? *g : ChordGBufferTargets{};
    if (!any_gbuffer_target(gg)) return fail(c, CHORDVIS_E_INVALID, "pack_gbuffer: no target");
    if (!width || !height) return fail(c, CHORDVIS_E_INVALID, "pack_gbuffer: zero width or height");
    if ((gg.baseColor && !ss.baseColor) || (gg.vertexNormal && !ss.vertexNormal) || (gg.pixelNormal && !ss.pixelNormal) ||
        (gg.motionVector && !ss.motionVector) || (gg.aoRoughnessMetallic && !ss.roughMetalAO) || (gg.emissive && !ss.emissive))
        return fail(c, CHORDVIS_E_INVALID, "pack_gbuffer: a target without its source");
    if (const char* why = gbuffer_target_misaligned(gg)) {
        char buf[96];
        std::snprintf(buf, sizeof(buf), "pack_gbuffer: %s", why);
        return fail(c, CHORDVIS_E_INVALID, buf);
    }
    // (only the sources that are read)
    if ((gg.baseColor && misaligned(ss.baseColor, 16)) || (gg.vertexNormal && misaligned(ss.vertexNormal, 16)) ||
        (gg.pixelNormal && misaligned(ss.pixelNormal, 16)) || (gg.aoRoughnessMetallic && misaligned(ss.roughMetalAO, 16)) ||
        (gg.emissive && misaligned(ss.emissive, 16)))
        return fail(c, CHORDVIS_E_INVALID, "pack_gbuffer: a float4 source is not 16-byte aligned");
    if (gg.motionVector && misaligned(ss.motionVector, 8)) return fail(c, CHORDVIS_E_INVALID, "pack_gbuffer: the motionVector source is not 8-byte aligned");
    chord::launch_pack_gbuffer(c, width, height, ss, gg);
    CHORD_HIP(c, hipGetLastError());
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

void* chordvis_stream(ChordCtx* c) { return c ? (void*)c->stream : nullptr; }

int chordvis_prepare_shading_tile_param(ChordCtx* c, uint32_t shadingType, const ChordTileMarker* marker, ChordShadingTiles* out)
{
    if (!c || !marker || !out || !marker->marker || marker->marker != c->dTileMarker)
        return fail(c, CHORDVIS_E_INVALID, "prepare_shading_tile_param: marker is not this context's");
    // (a handle from before chordvis_allocate_gbuffer may carry the address of the new marker: its dims place the count behind the list)
    if (marker->markerDim[0] != (c->width + 7u) / 8u || marker->markerDim[1] != (c->height + 7u) / 8u)
        return fail(c, CHORDVIS_E_INVALID, "prepare_shading_tile_param: the marker was made for another render size (call chordvis_visibility_mark again)");
    if (shadingType >= 128u) return fail(c, CHORDVIS_E_INVALID, "prepare_shading_tile_param: shading type does not fit the 128-bit marker");
    const uint32_t total = marker->markerDim[0] * marker->markerDim[1];
    uint32_t* count = c->dShadingTiles + (size_t)total * 2;
    chord::launch_shading_tiles(c, c->dTileMarker, shadingType, c->dShadingTiles, count, count + 4);
    CHORD_HIP(c, hipGetLastError());
    out->tileCmd = c->dShadingTiles; out->count = count; out->dispatchIndirect = count + 4; out->capacity = total;
    return CHORDVIS_OK;
}

int chordvis_readback_tile_marker(ChordCtx* c, const ChordTileMarker* marker, uint32_t* host)
{
    if (!c || !marker || !host || !marker->marker) return fail(c, CHORDVIS_E_INVALID, "readback_tile_marker: null argument");
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    CHORD_HIP(c, hipMemcpy(host, marker->marker, (size_t)marker->markerDim[0] * marker->markerDim[1] * 16, hipMemcpyDeviceToHost));
    return CHORDVIS_OK;
}

int chordvis_readback_shading_tiles(ChordCtx* c, const ChordShadingTiles* tiles, uint32_t* hostTiles, uint32_t hostCapacity,
                                    uint32_t* hostCount, uint32_t hostArgs[4])
{
    if (!c || !tiles || !tiles->count || !hostCount) return fail(c, CHORDVIS_E_INVALID, "readback_shading_tiles: null argument");
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    CHORD_HIP(c, hipMemcpy(hostCount, tiles->count, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (hostArgs) CHORD_HIP(c, hipMemcpy(hostArgs, tiles->dispatchIndirect, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    const uint32_t n = *hostCount < hostCapacity ? *hostCount : hostCapacity;
    if (hostTiles && n) CHORD_HIP(c, hipMemcpy(hostTiles, tiles->tileCmd, (size_t)n * 8, hipMemcpyDeviceToHost));
    return CHORDVIS_OK;
}

// ------------------------------------------------------------------------------ readback/stats --

int chordvis_readback_visibility(ChordCtx* c, uint64_t* host)
{
    if (!c || !host || !c->dVis) return fail(c, CHORDVIS_E_INVALID, "readback_visibility: no gbuffer");
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    if (c->visReadyEvent[0]) CHORD_HIP(c, hipEventSynchronize(c->visReadyEvent[0]));   // (pipelined group: the image is resolved beside the stream)
    const uint64_t* src = c->shard.ranks > 1 ? c->dVisResolved : c->dVis;
    CHORD_HIP(c, hipMemcpy(host, src, (size_t)c->width * c->height * 8, hipMemcpyDeviceToHost));
    return CHORDVIS_OK;
}

// Pipelined sharded frames: the image of the frame BEFORE the last submitted one (the other buffer pair).
int chordvis_readback_previous_visibility(ChordCtx* c, uint64_t* host)
{
    if (!c || !host || !c->dVisResolvedAlt) return fail(c, CHORDVIS_E_INVALID, "readback_previous_visibility: no second frame in flight (chordvis_swap_visibility)");
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    if (c->visReadyEvent[1]) CHORD_HIP(c, hipEventSynchronize(c->visReadyEvent[1]));
    CHORD_HIP(c, hipMemcpy(host, c->dVisResolvedAlt, (size_t)c->width * c->height * 8, hipMemcpyDeviceToHost));
    return CHORDVIS_OK;
}

int chordvis_readback_cmds(ChordCtx* c, ChordCountAndCmd h, ChordDrawCmd* host, uint32_t cap, uint32_t* outCount)
{
    if (!c || !h.count || !h.cmds || !outCount) return fail(c, CHORDVIS_E_INVALID, "readback_cmds: invalid handle");
    if (h.cmds == c->lists[0].cmds) { launch_full_list(c); CHORD_HIP(c, hipGetLastError()); }
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    uint32_t n = 0;
    CHORD_HIP(c, hipMemcpy(&n, h.count, 4, hipMemcpyDeviceToHost));
    *outCount = n;
    const uint32_t m = std::min(std::min(n, cap), h.capacity);
    if (host && m) {
        CHORD_HIP(c, hipMemcpy(host, h.cmds, sizeof(ChordDrawCmd) * m, hipMemcpyDeviceToHost));
        // device meshlet ids are flattened over assets; hand back asset-relative ids (the reference's cmd.y)
        for (uint32_t i = 0; i < m; i++) {
            if (host[i].objectId < c->objectCount) host[i].meshletId -= c->hPrims[c->hObjStatic[host[i].objectId].prim].assetMeshletBase;
        }
    }
    return CHORDVIS_OK;
}

int chordvis_readback_hzb(ChordCtx* c, const ChordHZB* hzb, uint16_t* hostMin, uint16_t* hostMax, uint32_t hostValidRange[2])
{
    if (!c || !hzb) return fail(c, CHORDVIS_E_INVALID, "readback_hzb: null handle");
    { const int rc = flush_pending_tail(c); if (rc) return rc; }
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    const size_t bytes = sizeof(uint16_t) * hzb->desc.totalTexels;
    if (hostMin && hzb->minTexels) CHORD_HIP(c, hipMemcpy(hostMin, hzb->minTexels, bytes, hipMemcpyDeviceToHost));
    if (hostMax && hzb->maxTexels) CHORD_HIP(c, hipMemcpy(hostMax, hzb->maxTexels, bytes, hipMemcpyDeviceToHost));
    if (hostValidRange && hzb->validRange) CHORD_HIP(c, hipMemcpy(hostValidRange, hzb->validRange, 8, hipMemcpyDeviceToHost));
    return CHORDVIS_OK;
}

int chordvis_upload_history_hzb(ChordCtx* c, const uint16_t* hostMin)
{
    if (!c || !hostMin || !c->dVis) return fail(c, CHORDVIS_E_INVALID, "upload_history_hzb: no gbuffer");
    c->pendingTailSlot = 0;                              // the uploaded chain replaces whatever was pending
    const int slot = c->historySlot == 1 ? 2 : 1;
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    CHORD_HIP(c, hipMemcpy(c->hzb[slot].minTexels, hostMin, sizeof(uint16_t) * c->hzb[slot].desc.totalTexels, hipMemcpyHostToDevice));
    c->hzb[slot].valid = true;
    c->hzb[slot].uploaded = true;                        // (its levels 6.. are the host's: frame_cull_fused_kernel would reduce them from level 5)
    c->historySlot = slot;
    return CHORDVIS_OK;
}

int chordvis_set_debug(ChordCtx* c, uint32_t flags)
{
    if (c) c->orderAge = c->orderAge1 = 0xFFFFFFFFu;                    // (the kept tile schedule of launch_raster is made again)

    if (!c) return CHORDVIS_E_INVALID;
    // measurement switches the library was not built with would silently measure the product: refuse them
    if (!RASTER_PROFILE && (flags & CHORD_DEBUG_PROFILE_BITS))
        return fail(c, CHORDVIS_E_INVALID, "set_debug: the phase clocks (bits 16, 512) need a library built with -DRASTER_PROFILE=1 (chord_amd/build.py --tag prof -DRASTER_PROFILE=1)");
    if (!RASTER_ABLATION && (flags & CHORD_DEBUG_ABLATION_BITS))
        return fail(c, CHORDVIS_E_INVALID, "set_debug: the ablation switches need a library built with -DRASTER_ABLATION=1 (chord_amd/build.py --tag abl -DRASTER_ABLATION=1)");
    c->debugFlags = flags;
    if (c->depthCtx) c->depthCtx->debugFlags = flags;      // (the depth views' child context follows)
    return CHORDVIS_OK;
}

int chordvis_debug_tile_profile(ChordCtx* c, int pass, uint64_t* hostTicks, uint32_t* hostCounts, uint32_t capacity)
{
    if (!c || pass < 0 || pass > 1 || !hostTicks || !hostCounts || capacity < c->tilesX * c->tilesY) return fail(c, CHORDVIS_E_INVALID, "debug_tile_profile: bad arguments");
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    const size_t n = (size_t)c->tilesX * c->tilesY;
    CHORD_HIP(c, hipMemcpy(hostTicks, c->dTileClocks + (size_t)pass * CHORD_MAX_TILES, n * 8, hipMemcpyDeviceToHost));
    CHORD_HIP(c, hipMemcpy2D(hostCounts, 4, c->dFrameState->tileCount + (size_t)pass * c->tilesX * c->tilesY * CHORD_TILECOUNT_STRIDE, 4 * CHORD_TILECOUNT_STRIDE, 4, n, hipMemcpyDeviceToHost));
    if (capacity >= 9 * n)   // optional: 8 phase accumulators per tile follow the totals
        CHORD_HIP(c, hipMemcpy(hostTicks + n, c->dTileClocks + (size_t)2 * CHORD_MAX_TILES + (size_t)pass * CHORD_MAX_TILES * 8, n * 64, hipMemcpyDeviceToHost));
    return CHORDVIS_OK;
}

int chordvis_debug_setup_kernels(ChordCtx* c, uint32_t wide[2])
{
    if (!c || !wide) return fail(c, CHORDVIS_E_INVALID, "debug_setup_kernels: bad arguments");
    wide[0] = c->setupWide[0]; wide[1] = c->setupWide[1];
    return CHORDVIS_OK;
}

// Measurement aid: captures two consecutive frames (the history slot alternates) into a hipGraph and replays it.
int chordvis_debug_graph_frames(ChordCtx* c, uint32_t pairs, float* msPerFrameStream, float* msPerFrameGraph)
{
    if (!c || !pairs || !msPerFrameStream || !msPerFrameGraph) return fail(c, CHORDVIS_E_INVALID, "debug_graph_frames: bad arguments");
    if (!c->ownStream) return fail(c, CHORDVIS_E_INVALID, "debug_graph_frames: needs a context-owned (capturable) stream");
    int rc;
    // (the kept tile schedule is off for both measurements: a captured frame either holds the schedule kernel or it does not, whatever the
    // age of the schedule at replay -- with it in every frame the stream's and the graph's frames are the same eleven + one launches)
    struct KeepOff { ChordCtx* c; uint32_t keep; ~KeepOff() { c->orderKeepFrames = keep; c->orderAge = c->orderAge1 = 0xFFFFFFFFu; } } keepOff{c, c->orderKeepFrames};
    c->orderKeepFrames = 0u;
    for (int i = 0; i < 4; i++) if ((rc = chordvis_render_frame(c))) return rc;
    hipEvent_t e0, e1;
    CHORD_HIP(c, hipEventCreate(&e0)); CHORD_HIP(c, hipEventCreate(&e1));
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    CHORD_HIP(c, hipEventRecord(e0, c->stream));
    for (uint32_t i = 0; i < 2 * pairs; i++) if ((rc = chordvis_render_frame(c))) return rc;
    CHORD_HIP(c, hipEventRecord(e1, c->stream));
    CHORD_HIP(c, hipEventSynchronize(e1));
    float ms = 0;
    CHORD_HIP(c, hipEventElapsedTime(&ms, e0, e1));
    *msPerFrameStream = ms / (2.0f * pairs);
    hipGraph_t graph; hipGraphExec_t exec;
    CHORD_HIP(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed));
    rc = chordvis_render_frame(c);
    if (!rc) rc = chordvis_render_frame(c);
    hipError_t ce = hipStreamEndCapture(c->stream, &graph);
    if (rc) return rc;
    CHORD_HIP(c, ce);
    CHORD_HIP(c, hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    for (int i = 0; i < 4; i++) CHORD_HIP(c, hipGraphLaunch(exec, c->stream));
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    CHORD_HIP(c, hipEventRecord(e0, c->stream));
    for (uint32_t i = 0; i < pairs; i++) CHORD_HIP(c, hipGraphLaunch(exec, c->stream));
    CHORD_HIP(c, hipEventRecord(e1, c->stream));
    CHORD_HIP(c, hipEventSynchronize(e1));
    CHORD_HIP(c, hipEventElapsedTime(&ms, e0, e1));
    *msPerFrameGraph = ms / (2.0f * pairs);
    (void)hipGraphExecDestroy(exec); (void)hipGraphDestroy(graph); (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return CHORDVIS_OK;
}

// Debugging aid: raw read of an internal buffer.  which: 0 tile counts (FrameState::tileCount), 1 fixed bins, 2 chunk table,
// 3 bin pool, 4 compact records, 5 wide records, 6 the fused cull kernel's look-back words, 7 the alpha plane (dTexAlpha),
// 10 the ray traversal sums of a measuring build; 8 the flattened (object, group) table (DGroupRef, 24 bytes per group instance), 9 the per-object static table (DObjStatic, 48
// bytes per object) -- the two checked against the current list's size.  offset / bytes in bytes.
int chordvis_debug_read(ChordCtx* c, int which, uint64_t offset, uint64_t bytes, void* host)
{
    if (!c || !host) return fail(c, CHORDVIS_E_INVALID, "debug_read: null argument");
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    const char* base = nullptr;
    switch (which) {
    case 0: base = (const char*)c->dFrameState->tileCount; break;
    case 1: base = (const char*)c->dTileBins; break;
    case 2: base = (const char*)c->dBinChunkTab; break;
    case 3: base = (const char*)c->dBinPool; break;
    case 4: base = (const char*)c->dTrisC; break;
    case 5: base = (const char*)c->dTris; break;
    case 6: base = (const char*)c->dCullLookback; break;       // look-back words of frame_cull_fused_kernel (profile build: stage clocks behind them)
    case 7: base = (const char*)c->dTexAlpha;                  // the alpha plane of the masked buckets
        if (!base) return fail(c, CHORDVIS_E_INVALID, "debug_read: the scene has no alpha plane (no masked material samples a texture)");
        break;
    case 8: case 9: {                                          // the group-ref table (groupInstances x 24 bytes) / the per-object static table (objectCount x 48)
        const uint64_t have = which == 8 ? (uint64_t)c->groupInstances * sizeof(chord::DGroupRef) : (uint64_t)c->objectCount * sizeof(chord::DObjStatic);
        if (!c->sceneLoaded || offset > have || bytes > have - offset) return fail(c, CHORDVIS_E_INVALID, "debug_read: no scene, or a range beyond the current object list's table");
        base = which == 8 ? (const char*)c->dGroupRefs : (const char*)c->dObjStatic;
        break;
    }
    case 10:                                                   // the traversal sums of a CHORD_RAY_COUNTERS build (device_layer.h)
        if (!c->dRayCounts || offset > sizeof(unsigned long long) * CHORD_RAY_COUNTER_WORDS || bytes > sizeof(unsigned long long) * CHORD_RAY_COUNTER_WORDS - offset)
            return fail(c, CHORDVIS_E_INVALID, "debug_read: no ray counters (a library built with -DCHORD_RAY_COUNTERS=1, after chordvis_build_ray_scene), or a range beyond them");
        base = (const char*)c->dRayCounts;
        break;
    default: return fail(c, CHORDVIS_E_INVALID, "debug_read: unknown buffer");
    }
    CHORD_HIP(c, hipMemcpy(host, base + offset, bytes, hipMemcpyDeviceToHost));
    return CHORDVIS_OK;
}

// Measurement / debugging aid: words of the split-tile accumulation slabs that are not zero (the invariant between
// raster passes is: none).
int chordvis_debug_slab_nonzero(ChordCtx* c, uint64_t* count)
{
    if (!c || !count || !c->dTileSlabs) return fail(c, CHORDVIS_E_INVALID, "debug_slab_nonzero: no gbuffer");
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    const size_t n = (size_t)c->tilesX * c->tilesY * CHORD_TILE * CHORD_TILE;
    std::vector<unsigned long long> h(n);
    CHORD_HIP(c, hipMemcpy(h.data(), c->dTileSlabs, n * 8, hipMemcpyDeviceToHost));
    uint64_t k = 0;
    for (size_t i = 0; i < n; i++) k += h[i] != 0ull;
    *count = k;
    return CHORDVIS_OK;
}

int chordvis_debug_setup_profile(ChordCtx* c, int pass, uint64_t hostTicks[5], uint32_t* waves)
{
    if (!c || pass < 0 || pass > 1 || !hostTicks) return fail(c, CHORDVIS_E_INVALID, "debug_setup_profile: bad arguments");
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    const size_t n = (size_t)CHORD_MAX_TILES * 8;
    std::vector<uint64_t> v(n);
    CHORD_HIP(c, hipMemcpy(v.data(), c->dTileClocks + (size_t)2 * CHORD_MAX_TILES + (size_t)pass * CHORD_MAX_TILES * 8, n * 8, hipMemcpyDeviceToHost));
    const uint32_t w = (uint32_t)std::min<size_t>((size_t)c->numCUs * 6 * 4, n / 5);
    for (int i = 0; i < 5; i++) hostTicks[i] = 0;
    for (uint32_t k = 0; k < w; k++) for (int i = 0; i < 5; i++) hostTicks[i] += v[(size_t)k * 5 + i];
    if (waves) *waves = w;
    return CHORDVIS_OK;
}

int chordvis_enable_timers(ChordCtx* c, int enable)
{
    if (!c) return CHORDVIS_E_INVALID;
    c->timers = enable < 0 ? 0 : ((enable & 0xFF) > 2 ? 2 : (enable & 0xFF));
    c->timerPeriod = (enable >> 8) > 0 ? (uint32_t)(enable >> 8) : 1u;
    c->stampTags.clear();
    c->framesStamped = 0;
    c->frameIndex = 0;
    c->stampThisFrame = false;
    return CHORDVIS_OK;
}

int chordvis_stats(ChordCtx* c, ChordStats* out)
{
    if (!c || !out) return fail(c, CHORDVIS_E_INVALID, "stats: null argument");
    std::memset(out, 0, sizeof(*out));
    { const int rc = flush_pending_tail(c); if (rc) return rc; }
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    uint32_t counts[4] = {0, 0, 0, 0};
    CHORD_HIP(c, hipMemcpy(counts, c->dCounts, sizeof(counts), hipMemcpyDeviceToHost));
    DeviceCounters dc;
    CHORD_HIP(c, hipMemcpy(&dc, c->dCounters, sizeof(dc), hipMemcpyDeviceToHost));
    out->countInstanceCulled = counts[0];
    if (c->shouldStage1) {
        out->countStage0Visible = counts[1]; out->countStage0Rejected = counts[2]; out->countStage1Visible = counts[3];
        out->trianglesSubmitted = dc.trisHzbVisible0 + dc.trisHzbVisible1;
    } else {
        out->countStage0Visible = counts[0];
        out->trianglesSubmitted = dc.trisInstanceCulled;
    }
    out->overflow = dc.overflow;
    out->rasterLaunches = c->rasterCalls;
    out->kernelLaunches = c->lastFrameLaunches;
    for (int pass = 0; pass < 2; pass++) {
        out->clipTriangles[pass] = dc.clipTriCount[pass];
        for (uint32_t i = 0; i < CHORD_LIST_SHARDS; i++) out->largeRecords[pass] += dc.largeCount[pass][i * CHORD_SHARD_STRIDE];
    }
    for (uint32_t i = 0; i < CHORD_LIST_SHARDS; i++) {
        out->triangleRecords += dc.triCount[i * CHORD_SHARD_STRIDE] + dc.triCountC[i * CHORD_SHARD_STRIDE];
        out->triangleRecordsCompact += dc.triCountC[i * CHORD_SHARD_STRIDE];
        out->pixelBlockBytes += (uint64_t)dc.blockGranules[i * CHORD_SHARD_STRIDE] * 16u;
    }
    if (c->tilesX) {
        std::vector<uint32_t> tc((size_t)c->tilesX * c->tilesY);
        for (int pass = 0; pass < 2; pass++) {
            CHORD_HIP(c, hipMemcpy2D(tc.data(), 4, c->dFrameState->tileCount + (size_t)pass * c->tilesX * c->tilesY * CHORD_TILECOUNT_STRIDE, 4 * CHORD_TILECOUNT_STRIDE, 4, tc.size(), hipMemcpyDeviceToHost));
            for (uint32_t v : tc) { out->binEntries += v; out->tilesTouched[pass] += v ? 1u : 0u; }
            CHORD_HIP(c, hipMemcpy2D(tc.data(), 4, c->dFrameState->tileCount + (size_t)pass * c->tilesX * c->tilesY * CHORD_TILECOUNT_STRIDE + 1, 4 * CHORD_TILECOUNT_STRIDE, 4, tc.size(), hipMemcpyDeviceToHost));
            for (uint32_t v : tc) out->pixelBlocks += v;
        }
    }
    if (c->timers && c->framesStamped && c->stampTags.size() > 1) {
        // walk the stamps: the segment ending at stamp i is attributed by its tag and the current stage
        float clear = 0, cull = 0, st0 = 0, hzb0 = 0, st1 = 0, hzbf = 0, rc_ = 0, rk = 0, rh = 0, other = 0, exh = 0, exv = 0, exc = 0, exf = 0;
        int stage = 0;   // 0 = stage 0, 1 = stage 1
        for (size_t i = 1; i < c->stampTags.size(); i++) {
            const int tag = c->stampTags[i];
            if (tag == S_FRAME_BEGIN) { stage = 0; continue; }           // gap between frames is not frame time
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, c->evPool[i - 1], c->evPool[i]) != hipSuccess) continue;
            switch (tag) {
            case S_CLEAR: clear += ms; break;
            case S_CULL: cull += ms; break;
            case S_HZBCULL: case S_STAGE0_END: case S_STAGE1_END: (stage == 0 ? st0 : st1) += ms; break;
            case S_R_CLUSTER: rc_ += ms; (stage == 0 ? st0 : st1) += ms; break;
            case S_R_CLIP: rk += ms; (stage == 0 ? st0 : st1) += ms; break;
            case S_R_CHUNK: rh += ms; (stage == 0 ? st0 : st1) += ms; break;
            case S_HZB0: hzb0 += ms; break;
            case S_HZBF: hzbf += ms; break;
            case S_EXCH_HZB: exh += ms; break;
            case S_EXCH_VIS: exv += ms; break;
            case S_EXCH_CULL: exc += ms; break;
            case S_EXCH_FINAL: exf += ms; break;
            default: other += ms; break;
            }
            if (tag == S_STAGE0_END) stage = 1;
        }
        const float inv = 1.0f / (float)c->framesStamped;
        out->msClear = clear * inv; out->msInstanceCulling = cull * inv; out->msStage0 = st0 * inv;
        out->msHzbStage0 = hzb0 * inv; out->msStage1 = st1 * inv; out->msHzbFinal = hzbf * inv;
        out->msRasterCluster = rc_ * inv; out->msRasterClip = rk * inv; out->msRasterChunk = rh * inv;
        out->msExchangeHzb = exh * inv; out->msExchangeVis = exv * inv; out->msExchangeCull = exc * inv; out->msExchangeFinal = exf * inv;
        out->msFrame = (clear + cull + st0 + hzb0 + st1 + hzbf + other + exh + exv + exc + exf) * inv;
        out->framesTimed = c->framesStamped;
        out->stampsPerFrame = (float)c->stampTags.size() * inv;
    }
    if (c->timers == 2) { c->stampTags.clear(); c->framesStamped = 0; }
    if (dc.overflow) return fail(c, CHORDVIS_E_CAPACITY, "a deferred raster list overflowed this frame; the visibility buffer is incomplete");
    return CHORDVIS_OK;
}

} // extern "C"
