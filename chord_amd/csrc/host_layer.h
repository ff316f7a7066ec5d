// What the host files of the C ABI share (one per feature: abi_*.cpp, and chordvis_abi.cpp for the scene): the device-memory helpers, the refusal text, the wrap constants
// of a texture level, and the helpers and upload jobs that more than one of those files uses.  Host only.  A helper that one file
// alone uses stays static or anonymous in that file.
#pragma once

#include "device_layer.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace chord {

// ---- device memory ----
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

// Device memory chordvis_set_object_list drops: hipFree waits for the device, and that call must not, so the pointers are kept until a
// call that waits anyway comes by (chordvis_upload_scene, chordvis_destroy, a chordvis_set_object_list that has to grow).
template <typename T>
void retire(ChordCtx* c, T*& p) { if (p) { c->retired.push_back((void*)p); p = nullptr; } }
void free_retired(ChordCtx* c);                 // abi_context.cpp (the caller has let the stream run empty)

// A device buffer one scope owns: the scope hipMallocs into `p`; it is freed when the scope ends unless release() handed it on.
template <typename T>
struct DeviceTemp {
    T* p = nullptr;
    DeviceTemp() = default;
    DeviceTemp(const DeviceTemp&) = delete;
    DeviceTemp& operator=(const DeviceTemp&) = delete;
    ~DeviceTemp() { if (p) (void)hipFree((void*)p); }
    T* release() { T* q = p; p = nullptr; return q; }
};

// ---- refusals: "<fn>: <why>" becomes the context's error text ----
inline int refuse(ChordCtx* c, int code, const char* fn, const char* why)
{
    char buf[224];
    std::snprintf(buf, sizeof(buf), "%s: %s", fn, why);
    return fail(c, code, buf);
}

// ---- the context's targets, view and stream (abi_context.cpp) ----
int configure_targets(ChordCtx* c, uint64_t* external);
int ready(ChordCtx* c, const char* fn);
int flush_view(ChordCtx* c);
int flush_pending_tail(ChordCtx* c);

// ---- what a scene upload, an object list or the context's end lets go ----
void drop_world_transforms(ChordCtx* c);        // chordvis_abi.cpp
void drop_ray_tlas(ChordCtx* c, bool park);     // abi_rays.cpp
void drop_ray_scene(ChordCtx* c);
void drop_ray_rebuild_buffers(ChordCtx* c);     // abi_raytlas.cpp (the caller has let the stream run empty)
void drop_material_textures(ChordCtx* c);       // abi_textures.cpp

// ---- textures (abi_textures.cpp; the alpha plane of chordvis_upload_scene is made with the same code) ----

// The constants a level's wrap is resolved to at upload (DMatLevel::magicS/T, biasS/T), for texel_wrap.h period_mod: magic =
// floor(2^32 / period), bias = the first multiple of the period at or above 2^30; both 0 where the kernels do not divide (a clamped
// axis; a power-of-two period, which they mask).  The raster's alpha test (chordvis_upload_scene) and the material resolve
// (chordvis_upload_material_textures) address texels alike because both take the constants from here.
inline void tex_wrap_constants(uint32_t n, uint32_t mode, uint32_t& magic, uint32_t& bias)
{
    magic = 0u; bias = 0u;
    if (mode == CHORD_WRAP_CLAMP_TO_EDGE) return;
    const uint32_t period = mode == CHORD_WRAP_MIRRORED_REPEAT ? 2u * n : n;
    if ((period & (period - 1u)) == 0u) return;                  // masked, not divided
    magic = (uint32_t)(0x100000000ull / period);
    bias = (uint32_t)(((0x40000000ull + period - 1u) / period) * period);
}

uint32_t tex_block_bytes(uint32_t format);      // of a CHORD_TEXFMT_BC* format; 0: RGBA8 (or none of them)
#define CHORD_TEXFMT_NAMES "0 (RGBA8), 1 (BC1_RGB), 2 (BC3), 3 (BC4), 4 (BC5)"
uint32_t tex_levels(const ChordCtx* c, uint32_t t, const ChordTexture& tx, ChordTextureMips& ms);
size_t tex_chain_texels(uint32_t width, uint32_t height, uint32_t levels);

// The compressed levels one upload expands: their bytes go to ONE staging buffer (every chain 16-byte aligned in it), one record
// per level to a small device table, one kernel launch decodes them all; buffer and table are freed after the synchronise.
struct TexDecodeJob {
    struct Copy { const uint8_t* host; uint64_t offset, bytes; };
    std::vector<DTexLevelRec> recs;
    std::vector<Copy> copies;
    uint64_t stagingBytes = 0;
    uint32_t blocks = 0;

    // dst: where level `first` goes (a texel index of dMatTexels / a byte index of dTexAlpha); the levels follow as an RGBA8 chain's
    // do.  Levels below `first` (chordvis_set_texture_first_level) are neither staged nor decoded
    void add(const ChordTexture& tx, uint32_t dst, uint32_t first = 0u);
    int run(ChordCtx* c, const char* who, uint32_t* texels, uint8_t* alpha, bool alphaOnly);
};

// The levels one upload makes: one launch per level step over every texture that has that step, then one launch whose workgroups
// finish the chains from 64 x 64 down, then the coverage passes; the record tables go to ONE device buffer, freed after the
// synchronise.  Runs after the copies and the decode, on the same stream: it reads what they wrote.
struct TexMipJob {
    std::vector<std::vector<DTexMipRec>> steps;     // [k]: the k-th step of every texture that has one
    std::vector<uint32_t> stepUnits;
    std::vector<DTexTailRec> tails;
    std::vector<DTexCovRec> cov;
    uint32_t covGroups = 0, covScaleGroups = 0;
    bool anySrgb = false;

    // base: where level 0 is (a texel index of dMatTexels / a byte index of dTexAlpha); the first `supplied` levels are there
    // when the job runs, levels supplied .. L-1 are made.  coverage: rescale their alpha (not asked for an alpha of 255 throughout)
    void add(uint32_t base, uint32_t width, uint32_t height, uint32_t supplied, uint32_t L, const ChordTextureMips& ms, bool coverage);
    int run(ChordCtx* c, const char* who, uint32_t* texels, uint8_t* alpha, bool alphaOnly);
};

} // namespace chord
