// chordvis — per-pixel attributes of the visible triangle (the visibility buffer's consumers' second step).
// Reference: install/resource/shader/lighting.hlsl:278-371 (per-pixel triangle resolve), nanite_shared.hlsli:111-179
// (getTriangleMiscInfo), material.hlsli:41-64 (uv, uv gradients, motion, positionRS), base.hlsli:457-495
// (calculateTriangleBarycentrics) and nanite_debug.hlsl:30-43,104-130 (the debug colours).
//
//   resolve_attributes_kernel<kLevel>     a wave per 16 x 4 pixels.  Its lanes load their visibility words; a ballot loop
//                               names one leader lane per distinct low word (slot | triangle) of the block; each leader fetches
//                               its triangle (command -> object / meshlet -> index word -> three vertices) and forms the
//                               per-vertex products (clip position, translated-world position, the two motion clip positions,
//                               uv); every pixel reads its leader's values through ds_bpermute and finishes the per-pixel
//                               arithmetic.  Stores: 16 bytes per lane for the float4 images, 256 contiguous bytes per wave and row.
//     <0>                       chordvis_resolve_attributes: the eight images.  Same arithmetic and resources as the
//                               non-template kernel it replaces (108 VGPRs, occupancy 4); its gfx950 code differs from it only
//                               in register assignment and two integer instructions.
//     <1>                       chordvis_resolve_surface: the surface channels compiled in.  The leader also fetches the three
//                               vertices' normals (float3) and tangents (float4) and forms nRS, tRS, bRS
//                               (nanite_shared.hlsli:157-175); the pixels interpolate them (material.hlsli:95-108).  134 VGPRs,
//                               occupancy 3.
//     <2>                       chordvis_resolve_material: the material channels behind them (material.hlsli:66-153).  Once a
//                               pixel's attribute and surface values are final (the leaders' set-up registers are dead), a second
//                               ballot loop walks the distinct MATERIAL ids of the wave: the material's record is read
//                               wave-uniformly (readlane index -> scalar loads), the lanes of that material sample its four
//                               texture slots with the pinned sampler of DESIGN.md 2 item 9 and store their texels of the four
//                               images inside the loop (no accumulators).  1 KB of LDS: the sRGB decode table.
//     <3>                       chordvis_resolve_material after chordvis_set_material_anisotropy with N > 1: <2> whose slots are
//                               sampled by sample_slot_aniso: up to N taps along the longer derivative, each
//                               the whole per-level pipeline, averaged in index order.  A lane loops to its own tap count; the slot's
//                               level records are read once, before the loop.  <2> is not touched: it is what N = 1 launches.
//     <4>, <5>                  the twins of <2> and <3> that chordvis_resolve_material launches while the uploaded store holds a
//                               chain kept as blocks (chordvis_set_material_texture_store, CHORD_TEXSTORE_BLOCKS).  A slot's format
//                               is part of its wave-uniform record: a texel slot runs sample_level as <2> / <3> do, a block slot
//                               sample_level_blocks -- the same wrap arithmetic, then per tap the 8 or 16 bytes of the block that
//                               holds the texel and bc_decode.h's decode of that one texel into the RGBA8 word the upload decoder
//                               would have stored; decode_texel and the filter arithmetic behind it are shared.
//     <2, true> .. <5, true>    chordvis_resolve_gbuffer: the packed twins of <2> .. <5>, the same code up to the store sites, which
//                               pack through gbuffer_pack.h into the reference's G-buffer formats: 4 bytes
//                               per lane (8 for emissive), 64 (128) contiguous bytes per wave and row.  Only motionVector,
//                               vertexNormal and the four material images exist there; the other images' code is compiled out.  A
//                               call that asks for vertexNormal / motionVector alone still launches one of them (the material
//                               loop is skipped at run time): there is no packed <0> or <1>.

//   material_feedback_kernel    chordvis_material_feedback: the same wave block over a LATTICE of pixels, leader loop, set-up and material
//                               loop as above, cut down to what the uv gradients need; instead of sampling, the lanes of a (material,
//                               slot) turn are balloted per finest level and one lane adds the popcount to a workgroup table in LDS,
//                               flushed to the per-(texture, level) counts with one global atomic per entry.
//
// The per-vertex products are the same bits whichever lane forms them (one arithmetic, no reassociation): a pixel's result
// does not depend on its neighbours.  Every + - * / is float32 in source order (-ffp-contract=off, IEEE divide).

#include "device_layer.h"
#include "bc_decode.h"
#include "device_math.h"
#include "gbuffer_pack.h"
#include "material_sampler.h"
#include "material_tables.h"
#include "texel_wrap.h"

namespace chord {

// simpleHash / simpleHashColor -- base.hlsli:112-128
__device__ __forceinline__ uint32_t simple_hash(uint32_t a)
{
    a = (a + 0x7ed55d16u) + (a << 12);
    a = (a ^ 0xc761c23cu) ^ (a >> 19);
    a = (a + 0x165667b1u) + (a << 5);
    a = (a + 0xd3a2646cu) ^ (a << 9);
    a = (a + 0xfd7046c5u) + (a << 3);
    a = (a ^ 0xb55a4f09u) ^ (a >> 16);
    return a;
}
__device__ __forceinline__ f3 simple_hash_color(uint32_t i)
{
    const uint32_t h = simple_hash(i);
    return f3{(float)(h & 255u) / 255.0f, (float)((h >> 8) & 255u) / 255.0f, (float)((h >> 16) & 255u) / 255.0f};
}

// kLODDebugColor -- nanite_debug.hlsl:30-43 (kNaniteMaxLODCount = 12 entries)
__constant__ float kLodDebugColor[12][3] = {
    {1.0f, 0.0f, 0.0f}, {0.7f, 0.3f, 0.0f}, {0.4f, 0.6f, 0.0f}, {0.1f, 0.9f, 0.0f}, {0.0f, 1.0f, 0.2f}, {0.0f, 0.5f, 0.6f},
    {0.0f, 0.1f, 0.8f}, {0.0f, 0.0f, 1.0f}, {0.1f, 0.1f, 0.8f}, {0.2f, 0.2f, 0.6f}, {0.0f, 0.4f, 0.7f}, {0.2f, 0.6f, 0.3f},
};

__device__ __forceinline__ uint32_t pack_unorm8(float c) { return (uint32_t)(saturatef(c) * 255.0f + 0.5f); }

// normalize(v) = v / sqrt(dot(v, v)), each component divided separately.  Departure from the reference: a vector whose dot(v, v)
// is not above 0 gives 0, not NaN (a G-buffer carries no NaN)
__device__ __forceinline__ f3 normalize_or_zero(f3 v)
{
    const float l2 = dot3(v, v);
    if (!(l2 > 0.0f)) return f3{0.0f, 0.0f, 0.0f};
    const float s = sqrtf(l2);
    return f3{v.x / s, v.y / s, v.z / s};
}

// (a0 * b.x + a1 * b.y) + a2 * b.z -- material.hlsli:52-61's interpolation, one component
__device__ __forceinline__ float interp3(float a0, float a1, float a2, f3 b) { return (a0 * b.x + a1 * b.y) + a2 * b.z; }

__device__ __forceinline__ float lane_read(float v, int src) { return __shfl(v, src, 64); }
__device__ __forceinline__ uint32_t lane_read(uint32_t v, int src) { return (uint32_t)__shfl((int)v, src, 64); }

struct ResolveArgs {
    const unsigned long long* vis;
    const ChordDrawCmd* cmds;
    const uint32_t* cmdCount;
    const ChordObject* objects;
    const DObjStatic* objStatic;
    const DPrim* prims;
    const DMeshlet* meshlets;
    const uint8_t* meshletLod;
    const uint32_t* meshletData;
    const float* positions;
    const float* texcoords;            // null: (0, 0)
    const DView* view;
    uint32_t W, H, blocksX, objectCount, meshletCount;
    uint32_t useNoJitter, debugMode;
    uint32_t want;                     // RESOLVE_* bits of the non-null targets
    ChordMat4 vpNoJitter, vpLastNoJitter;
    ChordResolveTargets t;
};
#define RESOLVE_BARY 1u
#define RESOLVE_DDX 2u
#define RESOLVE_DDY 4u
#define RESOLVE_UV 8u
#define RESOLVE_UVGRAD 16u
#define RESOLVE_POS 32u
#define RESOLVE_MOTION 64u
#define RESOLVE_DEBUG 128u

// what the surface variant reads besides ResolveArgs
struct SurfaceArgs {
    const float* normals;              // float3 per vertex (non-null whenever want != 0)
    const float* tangents;             // float4 per vertex (non-null whenever want has SURFACE_TANGENT | SURFACE_BITANGENT)
    uint32_t want;                     // SURFACE_* bits of the non-null targets
    ChordSurfaceTargets t;
};
#define SURFACE_NORMAL 1u
#define SURFACE_TANGENT 2u
#define SURFACE_BITANGENT 4u

// what the material variant reads besides those two
struct MaterialArgs {
    const DMatRecord* records;         // per material (chordvis_upload_material_textures)
    const uint32_t* texels;            // RGBA8 words, R in the low byte
    uint32_t want;                     // MATERIAL_* bits of the non-null targets
    uint32_t needSurface;              // SURFACE_* bits pixelNormal needs formed whether or not their images are asked for
    ChordMaterialTargets t;
};
#define MATERIAL_BASECOLOR 1u
#define MATERIAL_EMISSIVE 2u
#define MATERIAL_NORMAL 4u
#define MATERIAL_RMA 8u

// resolve_attributes_kernel<0> takes ResolveArgs alone; <1> carries SurfaceArgs after it, <2> MaterialArgs after that
template <int kLevel> struct KernelArgs : ResolveArgs {};
template <> struct KernelArgs<1> : ResolveArgs { SurfaceArgs e; };
template <> struct KernelArgs<2> : ResolveArgs { SurfaceArgs e; MaterialArgs m; };
template <> struct KernelArgs<3> : KernelArgs<2> { uint32_t kmax; };   // log2 of the context's maximum anisotropy (1 .. 4)
template <> struct KernelArgs<4> : KernelArgs<2> { const uint2* blocks; };   // dMatBlocks: the chains kept as blocks, 8-byte units
template <> struct KernelArgs<5> : KernelArgs<3> { const uint2* blocks; };

// ---- the pinned sampler ------------------------------------------------------------------------------
__device__ const uint32_t kSrgbBits[256] = {CHORD_SRGB_TABLE_BITS};
__device__ const uint32_t kSrgb2Ap1Bits[9] = {CHORD_SRGB_2_AP1_BITS};

// level of detail in 1/256 steps from the bit pattern of the squared footprint: the exponent and the top 8 mantissa bits are the
// piecewise-linear log2 of rho2 in Q8, halved for the square.  A footprint that is not finite or not above 0 gives 0.
__device__ __forceinline__ int32_t footprint_lodq(float4 g, float fW, float fH)
{
    const float ax = g.x * fW, ay = g.y * fH, bx = g.z * fW, by = g.w * fH;
    const float ra = ax * ax + ay * ay, rb = bx * bx + by * by;
    const float rho2 = fmaxf(ra, rb);
    if (!(ra < __builtin_inff()) || !(rb < __builtin_inff()) || !(rho2 > 0.0f)) return 0;
    return ((int32_t)(__float_as_uint(rho2) >> 15) - (127 << 8)) >> 1;
}

// S: a slot with mips > 0, read wave-uniformly; u, v, g (du/dx, dv/dx, du/dy, dv/dy) per lane
template <bool kSrgb, bool kBlocks>
__device__ __forceinline__ float4 sample_slot(const TexelStores<kBlocks>& texels, const DMatSlot& S, float u, float v, float4 g, const float* srgb)
{
    const uint32_t d0 = S.levels[0].dims;
    const int32_t lodq = footprint_lodq(g, (float)((d0 & 0xFFFFu) + 1u), (float)((d0 >> 16) + 1u));
    return sample_slot_lod<kSrgb, kBlocks>(texels, S, u, v, lodq, srgb);
}

// The anisotropic sampler, kmax = log2 N >= 1.  ra, rb, lmaj as footprint_lodq forms them.  The two
// derivative lengths are the axes (no ellipse fit): k = min(kmax, ceil(lmaj - lmin), ceil(lmaj)) in whole octaves, n = 1 << k taps
// at u + dmaj * t_i, t_i = (2i + 1 - n) / (2n), on level(s) lodq' = max(lmaj - (k << 8), 0); d = 0, d += c_i - c_0 in index order
// (i >= 1), c_0 + d * (1 / n): equal taps give c_0 exactly, which a running sum of the taps does not (3c is not c's neighbour).
// Powers of two make t_i, 1 / n and the level shift exact.  k = 0 (isotropic, magnified, not finite): sample_slot's path, no offset
// formed, c_0 returned as it is.
template <bool kSrgb, bool kBlocks>
__device__ __forceinline__ float4 sample_slot_aniso(const TexelStores<kBlocks>& texels, const DMatSlot& S, float u, float v, float4 g, uint32_t kmax,
                                                    const float* srgb)
{
    const uint32_t d0 = S.levels[0].dims;
    const float fW = (float)((d0 & 0xFFFFu) + 1u), fH = (float)((d0 >> 16) + 1u);
    const float ax = g.x * fW, ay = g.y * fH, bx = g.z * fW, by = g.w * fH;
    const float ra = ax * ax + ay * ay, rb = bx * bx + by * by;
    const bool xMajor = ra >= rb;                                        // (a tie goes to x)
    const float rmaj2 = fmaxf(ra, rb), rmin2 = fminf(ra, rb);
    int32_t lmaj = 0, k = 0;
    if (ra < __builtin_inff() && rb < __builtin_inff() && rmaj2 > 0.0f) {
        lmaj = ((int32_t)(__float_as_uint(rmaj2) >> 15) - (127 << 8)) >> 1;
        if (lmaj > 0) {
            int32_t spread = (int32_t)kmax;
            if (rmin2 > 0.0f) spread = (max(lmaj - (((int32_t)(__float_as_uint(rmin2) >> 15) - (127 << 8)) >> 1), 0) + 255) >> 8;
            k = min(min((int32_t)kmax, spread), (lmaj + 255) >> 8);
        }
    }
    const int32_t lodq = max(lmaj - (k << 8), 0);
    const uint32_t filter = S.filter, last = S.mips - 1u;
    uint32_t l0 = 0u, l1 = 0u;
    bool linear = (filter & CHORD_MATSLOT_MAG_LINEAR) != 0u;
    if (lmaj > 0) {
        linear = (filter & CHORD_MATSLOT_MIN_LINEAR) != 0u;
        if (filter & CHORD_MATSLOT_MIP_NEAREST) l0 = l1 = min((uint32_t)(lodq + 128) >> 8, last);
        else if (filter & CHORD_MATSLOT_MIP_LINEAR) { l0 = min((uint32_t)lodq >> 8, last); l1 = min(l0 + 1u, last); }
    }
    // the level records depend on lodq', not on the tap
    const DMatLevel L0 = S.levels[l0], L1 = S.levels[l1];
    const float f = (float)(lodq & 255) * (1.0f / 256.0f);
    const uint32_t wrapS = S.wrapS, wrapT = S.wrapT;
    const float du = xMajor ? g.x : g.z, dv = xMajor ? g.y : g.w;
    const int32_t n = 1 << k;
    const float inv2n = __uint_as_float((uint32_t)(126 - k) << 23);      // 1 / (2n)
    float4 c0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), d = c0;
    for (int32_t i = 0; i < n; i++) {
        float ui = u, vi = v;
        if (k) { const float t = (float)(2 * i + 1 - n) * inv2n; ui = u + du * t; vi = v + dv * t; }
        float4 c = sample_level<kSrgb, kBlocks>(texels, L0, wrapS, wrapT, linear, ui, vi, srgb);
        if (l1 != l0) {
            const float4 c1 = sample_level<kSrgb, kBlocks>(texels, L1, wrapS, wrapT, linear, ui, vi, srgb);
            c = make_float4(c.x + (c1.x - c.x) * f, c.y + (c1.y - c.y) * f, c.z + (c1.z - c.z) * f, c.w + (c1.w - c.w) * f);
        }
        if (i == 0) c0 = c;
        else d = make_float4(d.x + (c.x - c0.x), d.y + (c.y - c0.y), d.z + (c.z - c0.z), d.w + (c.w - c0.w));
    }
    if (k) { const float s = __uint_as_float((uint32_t)(127 - k) << 23); c0 = make_float4(c0.x + d.x * s, c0.y + d.y * s, c0.z + d.z * s, c0.w + d.w * s); }
    return c0;
}

// a slot of the material loop: <2> and <4> sample it with sample_slot, <3> and <5> with sample_slot_aniso; <4> and <5> look at its format
template <int kLevel, bool kSrgb>
__device__ __forceinline__ float4 sample_material_slot(const uint32_t* __restrict__ texels, const DMatSlot& S, float u, float v, float4 g,
                                                       const KernelArgs<kLevel>& a, const float* srgb)
{
    constexpr bool kBlocks = kLevel >= 4;
    TexelStores<kBlocks> T;
    T.texels = texels;
    if constexpr (kBlocks) { T.blocks = a.blocks; T.format = S.format; }
    if constexpr (kLevel == 3 || kLevel == 5) return sample_slot_aniso<kSrgb, kBlocks>(T, S, u, v, g, a.kmax, srgb);
    else return sample_slot<kSrgb, kBlocks>(T, S, u, v, g, srgb);
}

// kPacked (kLevel >= 2 only): the store policy of chordvis_resolve_gbuffer.  The six target pointers the packed images have a float
// twin for -- a.t.motionVector, a.e.t.vertexNormal and the four of a.m.t -- are the ChordGBufferTargets' (4 bytes a texel, 8 for
// emissive), carried in the same fields; the store sites pack through gbuffer_pack.h, and the images nobody can ask a packed launch for
// are compiled out (their want bits are masked at compile time).  Nothing upstream of the stores differs.
template <int kLevel, bool kPacked = false>
__global__ __launch_bounds__(256) void resolve_attributes_kernel(const KernelArgs<kLevel> a)
{
    static_assert(!kPacked || kLevel >= 2, "the packed store policy exists for the material levels");
    constexpr bool kSurface = kLevel >= 1;
    const uint32_t want = kPacked ? a.want & RESOLVE_MOTION : a.want;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t block = blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t bx = block % a.blocksX, by = block / a.blocksX;
    const uint32_t x = bx * 16u + (lane & 15u), y = by * 4u + (lane >> 4);
    const bool inside = x < a.W && y < a.H;                          // (the grid's last workgroup may hold waves past the image)
    const size_t pix = (size_t)y * a.W + x;
    const uint32_t n = *a.cmdCount;
    const uint32_t low = inside ? (uint32_t)a.vis[pix] : 0u;
    const uint32_t slot = ((low >> 8) & CHORD_MAX_INSTANCE_ID) - 1u;   // base.hlsli:443-447
    const bool covered = low != 0u && slot < n;

    // one leader per distinct (slot, triangle) of the wave
    int leader = (int)lane;
    uint64_t pending = __ballot(covered);
    while (pending) {
        const int l = __ffsll((unsigned long long)pending) - 1;
        const uint32_t key = (uint32_t)__builtin_amdgcn_readlane((int)low, l);
        const bool mine = covered && low == key;
        if (mine) leader = l;
        pending &= ~__ballot(mine);
    }
    const bool isLeader = covered && leader == (int)lane;

    // ---- per-triangle set-up (leaders): getTriangleMiscInfo, nanite_shared.hlsli:111-179 --------------------------------
    bool ok = false;
    float phs[3][4] = {}, prs[3][3] = {}, cur[3][3] = {}, last[3][3] = {}, uvv[3][2] = {};
    uint32_t meshletHashId = 0u, triWord = 0u, lod = 0u;
    float nrs[3][3] = {}, trs[3][3] = {}, brs[3][3] = {};                 // (surface variant only)
    uint32_t matId = 0u;                                                  // (material variant only)
    uint32_t surfNeed = 0u;                                               // SURFACE_* bits the leaders form
    uint32_t surfWant = 0u;                                               // SURFACE_* bits of the images stored
    if constexpr (kSurface) surfWant = kPacked ? a.e.want & SURFACE_NORMAL : a.e.want;
    surfNeed = surfWant;
    if constexpr (kLevel >= 2) surfNeed |= a.m.needSurface;
    if (isLeader) {
        const ChordDrawCmd cmd = a.cmds[slot];
        const uint32_t tri = low & 0xFFu;
        if (cmd.objectId < a.objectCount && cmd.meshletId < a.meshletCount) {
            const DMeshlet& m = a.meshlets[cmd.meshletId];
            const uint32_t V = m.vertexTriangleCount & 0xFFu, T = (m.vertexTriangleCount >> 8) & 0xFFu;
            if (tri < T) {
                ok = true;
                const ChordObject& obj = a.objects[cmd.objectId];
                const DView& dv = *a.view;
                const Mat4 M = load_mat(obj.basicData.localToTranslatedWorld);
                const Mat4 Ml = load_mat(obj.basicData.localToTranslatedWorldLastFrame);
                const Mat4 mvp = mul_mm(load_mat(dv.iv.translatedWorldToClip), M);          // the raster's matrix (kernels_cull.hip obj_mvp)
                const Mat4 mCur = a.useNoJitter ? mul_mm(load_mat(a.vpNoJitter), M) : mvp;
                const Mat4 mLast = a.useNoJitter ? mul_mm(load_mat(a.vpLastNoJitter), Ml)
                                                 : mul_mm(load_mat(dv.view.translatedWorldToClipLastFrame), Ml);   // obj_mvp_last
                triWord = a.meshletData[m.dataOffset + V + tri];
                meshletHashId = cmd.meshletId - a.prims[a.objStatic[cmd.objectId].prim].assetMeshletBase;   // the reference's cmd.y
                lod = a.meshletLod[cmd.meshletId];
                Mat4 Mi = {};
                if constexpr (kSurface) Mi = load_mat(obj.basicData.translatedWorldToLocal);
                if constexpr (kLevel >= 2) matId = CHORD_MATFLAG_MATERIAL(a.objStatic[cmd.objectId].matFlags);
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    const uint32_t vi = a.meshletData[m.dataOffset + ((triWord >> (8 * i)) & 0xFFu)] + m.vertexBase;
                    const float px = a.positions[(size_t)vi * 3], py = a.positions[(size_t)vi * 3 + 1], pz = a.positions[(size_t)vi * 3 + 2];
                    const f4 h = mul_mv(mvp, px, py, pz, 1.0f);
                    phs[i][0] = h.x; phs[i][1] = h.y; phs[i][2] = h.z; phs[i][3] = h.w;
                    const f4 r = mul_mv(M, px, py, pz, 1.0f);
                    prs[i][0] = r.x; prs[i][1] = r.y; prs[i][2] = r.z;
                    const f4 cc = mul_mv(mCur, px, py, pz, 1.0f);
                    cur[i][0] = cc.x; cur[i][1] = cc.y; cur[i][2] = cc.w;
                    const f4 ll = mul_mv(mLast, px, py, pz, 1.0f);
                    last[i][0] = ll.x; last[i][1] = ll.y; last[i][2] = ll.w;
                    if (a.texcoords) { uvv[i][0] = a.texcoords[(size_t)vi * 2]; uvv[i][1] = a.texcoords[(size_t)vi * 2 + 1]; }
                    if constexpr (kSurface) {
                        if (surfNeed) {
                            // nRS = normalize(mul(float4(nLS, 0), translatedWorldToLocal).xyz): the row-vector product, component j
                            // = (x * m0j + y * m1j) + z * m2j
                            const float nx = a.e.normals[(size_t)vi * 3], ny = a.e.normals[(size_t)vi * 3 + 1], nz = a.e.normals[(size_t)vi * 3 + 2];
                            const f3 nw = {(nx * Mi.r[0][0] + ny * Mi.r[1][0]) + nz * Mi.r[2][0],
                                           (nx * Mi.r[0][1] + ny * Mi.r[1][1]) + nz * Mi.r[2][1],
                                           (nx * Mi.r[0][2] + ny * Mi.r[1][2]) + nz * Mi.r[2][2]};
                            const f3 n = normalize_or_zero(nw);
                            nrs[i][0] = n.x; nrs[i][1] = n.y; nrs[i][2] = n.z;
                            if (surfNeed & (SURFACE_TANGENT | SURFACE_BITANGENT)) {
                                const float4 tl = reinterpret_cast<const float4*>(a.e.tangents)[vi];
                                // t = mul(localToTranslatedWorld, float4(tLS.xyz, 0)).xyz; tRS = normalize(t - dot(t, nRS) * nRS)
                                const f3 tw = {(M.r[0][0] * tl.x + M.r[0][1] * tl.y) + M.r[0][2] * tl.z,
                                               (M.r[1][0] * tl.x + M.r[1][1] * tl.y) + M.r[1][2] * tl.z,
                                               (M.r[2][0] * tl.x + M.r[2][1] * tl.y) + M.r[2][2] * tl.z};
                                const float d = dot3(tw, n);
                                const f3 t = normalize_or_zero(f3{tw.x - d * n.x, tw.y - d * n.y, tw.z - d * n.z});
                                trs[i][0] = t.x; trs[i][1] = t.y; trs[i][2] = t.z;
                                // bRS = cross(nRS, tRS) * tLS.w
                                brs[i][0] = (n.y * t.z - n.z * t.y) * tl.w;
                                brs[i][1] = (n.z * t.x - n.x * t.z) * tl.w;
                                brs[i][2] = (n.x * t.y - n.y * t.x) * tl.w;
                            }
                        }
                    }
                }
            }
        }
    }

    // ---- per pixel ------------------------------------------------------------------------------------------------------
    const bool hit = covered && lane_read((uint32_t)ok, leader) != 0u;
    float P[3][4];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 4; k++) P[i][k] = lane_read(phs[i][k], leader);

    // screenUvToNdcUv((dispatchPos + 0.5) * texelSize) -- material.hlsli:38, base.hlsli:137-143
    const DView& dv = *a.view;
    const float invW = dv.view.renderDimension[2], invH = dv.view.renderDimension[3];
    const float su = ((float)x + 0.5f) * invW, sv = ((float)y + 0.5f) * invH;
    const float pcx = 2.0f * (su - 0.5f), pcy = 2.0f * (0.5f - sv);

    // calculateTriangleBarycentrics -- base.hlsli:457-495, statement by statement
    const f3 rcpW = {1.0f / P[0][3], 1.0f / P[1][3], 1.0f / P[2][3]};
    const float p0x = P[0][0] * rcpW.x, p0y = P[0][1] * rcpW.x;
    const float p1x = P[1][0] * rcpW.y, p1y = P[1][1] * rcpW.y;
    const float p2x = P[2][0] * rcpW.z, p2y = P[2][1] * rcpW.z;
    const f3 p120x = {p1x, p2x, p0x}, p120y = {p1y, p2y, p0y}, p201x = {p2x, p0x, p1x}, p201y = {p2y, p0y, p1y};
    const f3 cdx = {p201y.x - p120y.x, p201y.y - p120y.y, p201y.z - p120y.z};
    const f3 cdy = {p120x.x - p201x.x, p120x.y - p201x.y, p120x.z - p201x.z};
    const f3 C = {cdx.x * (pcx - p120x.x) + cdy.x * (pcy - p120y.x),
                  cdx.y * (pcx - p120x.y) + cdy.y * (pcy - p120y.y),
                  cdx.z * (pcx - p120x.z) + cdy.z * (pcy - p120y.z)};
    const f3 G = {C.x * rcpW.x, C.y * rcpW.y, C.z * rcpW.z};
    const float Hs = dot3(C, rcpW);
    const float rcpH = 1.0f / Hs;
    const f3 bary = {G.x * rcpH, G.y * rcpH, G.z * rcpH};
    const f3 gdx = {cdx.x * rcpW.x, cdx.y * rcpW.y, cdx.z * rcpW.z};
    const f3 gdy = {cdy.x * rcpW.x, cdy.y * rcpW.y, cdy.z * rcpW.z};
    const float hdx = dot3(cdx, rcpW), hdy = dot3(cdy, rcpW);
    const float rcpH2 = rcpH * rcpH, sx = 2.0f * invW, sy = -2.0f * invH;
    const f3 ddx = {((gdx.x * Hs - G.x * hdx) * rcpH2) * sx, ((gdx.y * Hs - G.y * hdx) * rcpH2) * sx, ((gdx.z * Hs - G.z * hdx) * rcpH2) * sx};
    const f3 ddy = {((gdy.x * Hs - G.x * hdy) * rcpH2) * sy, ((gdy.y * Hs - G.y * hdy) * rcpH2) * sy, ((gdy.z * Hs - G.z * hdy) * rcpH2) * sy};

    if (want & RESOLVE_BARY)
        if (inside) reinterpret_cast<float4*>(a.t.barycentrics)[pix] = hit ? make_float4(bary.x, bary.y, bary.z, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (want & RESOLVE_DDX)
        if (inside) reinterpret_cast<float4*>(a.t.baryDdx)[pix] = hit ? make_float4(ddx.x, ddx.y, ddx.z, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (want & RESOLVE_DDY)
        if (inside) reinterpret_cast<float4*>(a.t.baryDdy)[pix] = hit ? make_float4(ddy.x, ddy.y, ddy.z, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (want & (RESOLVE_UV | RESOLVE_UVGRAD)) {
        float U[3][2];
#pragma unroll
        for (int i = 0; i < 3; i++) { U[i][0] = lane_read(uvv[i][0], leader); U[i][1] = lane_read(uvv[i][1], leader); }
        if (want & RESOLVE_UV) {
            const float u = interp3(U[0][0], U[1][0], U[2][0], bary), v = interp3(U[0][1], U[1][1], U[2][1], bary);
            if (inside) reinterpret_cast<float2*>(a.t.uv)[pix] = hit ? make_float2(u, v) : make_float2(0.0f, 0.0f);
        }
        if (want & RESOLVE_UVGRAD) {
            const float4 g = make_float4(interp3(U[0][0], U[1][0], U[2][0], ddx), interp3(U[0][1], U[1][1], U[2][1], ddx),
                                         interp3(U[0][0], U[1][0], U[2][0], ddy), interp3(U[0][1], U[1][1], U[2][1], ddy));
            if (inside) reinterpret_cast<float4*>(a.t.uvGrad)[pix] = hit ? g : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
    if (want & RESOLVE_POS) {
        float R[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) R[i][k] = lane_read(prs[i][k], leader);
        const float4 p = make_float4(interp3(R[0][0], R[1][0], R[2][0], bary), interp3(R[0][1], R[1][1], R[2][1], bary),
                                     interp3(R[0][2], R[1][2], R[2][2], bary), 1.0f);
        if (inside) reinterpret_cast<float4*>(a.t.positionRS)[pix] = hit ? p : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    if (want & RESOLVE_MOTION) {
        float Cc[3][3], Ll[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) { Cc[i][k] = lane_read(cur[i][k], leader); Ll[i][k] = lane_read(last[i][k], leader); }
        const float cx = interp3(Cc[0][0], Cc[1][0], Cc[2][0], bary), cy = interp3(Cc[0][1], Cc[1][1], Cc[2][1], bary);
        const float cz = interp3(Cc[0][2], Cc[1][2], Cc[2][2], bary);
        const float lx = interp3(Ll[0][0], Ll[1][0], Ll[2][0], bary), ly = interp3(Ll[0][1], Ll[1][1], Ll[2][1], bary);
        const float lz = interp3(Ll[0][2], Ll[1][2], Ll[2][2], bary);
        // material.hlsli:59
        const float mx = (lx / lz - cx / cz) * 0.5f, my = (ly / lz - cy / cz) * -0.5f;
        if (inside) {
            if constexpr (kPacked) reinterpret_cast<uint32_t*>(a.t.motionVector)[pix] = hit ? gbuffer_pack_motion(mx, my) : 0u;
            else reinterpret_cast<float2*>(a.t.motionVector)[pix] = hit ? make_float2(mx, my) : make_float2(0.0f, 0.0f);
        }
    }
    if (want & RESOLVE_DEBUG) {
        const uint32_t mId = lane_read(meshletHashId, leader), tw = lane_read(triWord, leader);
        const uint32_t lv = min(lane_read(lod, leader), 11u);
        // nanite_debug.hlsl:104-130
        const f3 lodColor = {kLodDebugColor[lv][0], kLodDebugColor[lv][1], kLodDebugColor[lv][2]};
        f3 c;
        if (a.debugMode == CHORD_NANITE_DEBUG_MESHLET) c = simple_hash_color(mId);
        else if (a.debugMode == CHORD_NANITE_DEBUG_TRIANGLE) c = simple_hash_color(tw);
        else if (a.debugMode == CHORD_NANITE_DEBUG_LOD) c = lodColor;
        else if (a.debugMode == CHORD_NANITE_DEBUG_LOD_MESHLET) {
            const f3 mc = simple_hash_color(mId);
            c = f3{powf(mc.x, 0.5f) * lodColor.x, powf(mc.y, 0.5f) * lodColor.y, powf(mc.z, 0.5f) * lodColor.z};
        } else c = bary;
        const uint32_t rgba = pack_unorm8(c.x) | pack_unorm8(c.y) << 8 | pack_unorm8(c.z) << 16 | 0xFF000000u;
        if (inside) a.t.debugRGBA8[pix] = hit ? rgba : 0xFF000000u;
    }
    f3 Npx = {0.0f, 0.0f, 0.0f}, Tpx = {0.0f, 0.0f, 0.0f}, Bpx = {0.0f, 0.0f, 0.0f};   // (material variant: the pixel's frame)
    if constexpr (kSurface) {
        // vertexNormal / tangent / bitangent = (v0 * b.x + v1 * b.y) + v2 * b.z, not renormalised (material.hlsli:98-99)
        auto put = [&](const float (&V)[3][3], float* dst, bool store) {
            float Q[3][3];
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int k = 0; k < 3; k++) Q[i][k] = lane_read(V[i][k], leader);
            const float4 v = make_float4(interp3(Q[0][0], Q[1][0], Q[2][0], bary), interp3(Q[0][1], Q[1][1], Q[2][1], bary),
                                         interp3(Q[0][2], Q[1][2], Q[2][2], bary), 0.0f);
            if (store)
                if (inside) {
                    if constexpr (kPacked) reinterpret_cast<uint32_t*>(dst)[pix] = hit ? gbuffer_pack_normal(v.x, v.y, v.z) : 0u;
                    else reinterpret_cast<float4*>(dst)[pix] = hit ? v : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                }
            return f3{v.x, v.y, v.z};
        };
        if (surfNeed & SURFACE_NORMAL) Npx = put(nrs, a.e.t.vertexNormal, (surfWant & SURFACE_NORMAL) != 0u);
        if (surfNeed & SURFACE_TANGENT) Tpx = put(trs, a.e.t.tangent, (surfWant & SURFACE_TANGENT) != 0u);
        if (surfNeed & SURFACE_BITANGENT) Bpx = put(brs, a.e.t.bitangent, (surfWant & SURFACE_BITANGENT) != 0u);
    }
    if constexpr (kLevel >= 2) {
        // ---- loadGLTFMetallicRoughnessPBRMaterial, material.hlsli:66-153 ---------------------------------------------------
        __shared__ float sSrgb[256];
        sSrgb[threadIdx.x] = __uint_as_float(kSrgbBits[threadIdx.x]);
        __syncthreads();
        if (a.m.want) {
            float U[3][2];
#pragma unroll
            for (int i = 0; i < 3; i++) { U[i][0] = lane_read(uvv[i][0], leader); U[i][1] = lane_read(uvv[i][1], leader); }
            const float u = interp3(U[0][0], U[1][0], U[2][0], bary), v = interp3(U[0][1], U[1][1], U[2][1], bary);
            const float4 g = make_float4(interp3(U[0][0], U[1][0], U[2][0], ddx), interp3(U[0][1], U[1][1], U[2][1], ddx),
                                         interp3(U[0][0], U[1][0], U[2][0], ddy), interp3(U[0][1], U[1][1], U[2][1], ddy));
            const uint32_t mId = lane_read(matId, leader);
            const uint32_t* __restrict__ texels = a.m.texels;
            bool written = false;
            // one turn per distinct material of the wave; its record is wave-uniform
            uint64_t left = __ballot(hit);
            while (left) {
                const int l = __ffsll((unsigned long long)left) - 1;
                const uint32_t mat = (uint32_t)__builtin_amdgcn_readlane((int)mId, l);
                const bool mine = hit && mId == mat;
                left &= ~__ballot(mine);
                const DMatRecord& M = a.m.records[mat];
                if (!M.pbr) continue;                                   // (lighting.hlsl:369: other shading types leave 0)
                if (!mine) continue;
                written = true;
                if (a.m.want & MATERIAL_BASECOLOR) {
                    float4 c = make_float4(1.0f, 1.0f, 1.0f, 1.0f);    // the white fallback (asset_gltf.cpp:323-326)
                    if (M.slot[CHORD_MATSLOT_BASECOLOR].mips) c = sample_material_slot<kLevel, true>(texels, M.slot[CHORD_MATSLOT_BASECOLOR], u, v, g, a, sSrgb);
                    const float r = c.x * M.baseColorFactor[0], gg = c.y * M.baseColorFactor[1], b = c.z * M.baseColorFactor[2];
                    const float al = c.w * M.baseColorFactor[3];
                    float m[9];
#pragma unroll
                    for (int i = 0; i < 9; i++) m[i] = __uint_as_float(kSrgb2Ap1Bits[i]);
                    const float4 o = make_float4((m[0] * r + m[1] * gg) + m[2] * b, (m[3] * r + m[4] * gg) + m[5] * b, (m[6] * r + m[7] * gg) + m[8] * b, al);
                    if constexpr (kPacked) reinterpret_cast<uint32_t*>(a.m.t.baseColor)[pix] = gbuffer_pack_rgb10(o.x, o.y, o.z);
                    else reinterpret_cast<float4*>(a.m.t.baseColor)[pix] = o;
                }
                if (a.m.want & MATERIAL_EMISSIVE) {
                    float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);    // the transparent-black fallback
                    if (M.slot[CHORD_MATSLOT_EMISSIVE].mips) c = sample_material_slot<kLevel, true>(texels, M.slot[CHORD_MATSLOT_EMISSIVE], u, v, g, a, sSrgb);
                    const float4 o = make_float4(c.x * M.emissiveFactor[0], c.y * M.emissiveFactor[1], c.z * M.emissiveFactor[2], 0.0f);
                    if constexpr (kPacked) reinterpret_cast<uint2*>(a.m.t.emissive)[pix] = gbuffer_pack_emissive(o.x, o.y, o.z);
                    else reinterpret_cast<float4*>(a.m.t.emissive)[pix] = o;
                }
                if (a.m.want & MATERIAL_NORMAL) {
                    f3 nrm = Npx;
                    if (M.slot[CHORD_MATSLOT_NORMAL].mips) {
                        const float4 c = sample_material_slot<kLevel, false>(texels, M.slot[CHORD_MATSLOT_NORMAL], u, v, g, a, sSrgb);
                        float tx = c.x * 2.0f - 1.0f, ty = c.y * 2.0f - 1.0f;
                        const float tz = sqrtf(fmaxf(0.0f, 1.0f - (tx * tx + ty * ty)));    // (departure: no NaN from a filtered xy beyond the unit disc)
                        tx *= M.normalFactorScale; ty *= M.normalFactorScale;
                        const f3 n = normalize_or_zero(f3{tx, ty, tz});
                        // mul(n, float3x3(T, B, N)): component j = (n.x * T.j + n.y * B.j) + n.z * N.j
                        nrm = f3{(n.x * Tpx.x + n.y * Bpx.x) + n.z * Npx.x, (n.x * Tpx.y + n.y * Bpx.y) + n.z * Npx.y, (n.x * Tpx.z + n.y * Bpx.z) + n.z * Npx.z};
                    }
                    if constexpr (kPacked) reinterpret_cast<uint32_t*>(a.m.t.pixelNormal)[pix] = gbuffer_pack_normal(nrm.x, nrm.y, nrm.z);
                    else reinterpret_cast<float4*>(a.m.t.pixelNormal)[pix] = make_float4(nrm.x, nrm.y, nrm.z, 0.0f);
                }
                if (a.m.want & MATERIAL_RMA) {
                    float rough = M.roughnessFactor, metal = M.metallicFactor >= 1.0f ? 0.0f : M.metallicFactor, ao = 1.0f;   // gltf.h:53-58
                    if (M.slot[CHORD_MATSLOT_METALROUGH].mips) {
                        const float4 c = sample_material_slot<kLevel, false>(texels, M.slot[CHORD_MATSLOT_METALROUGH], u, v, g, a, sSrgb);
                        rough = c.y; metal = c.z;
                        ao = M.bExistOcclusion ? M.occlusionTextureStrength * c.x : 1.0f;
                    }
                    if constexpr (kPacked) reinterpret_cast<uint32_t*>(a.m.t.roughMetalAO)[pix] = gbuffer_pack_arm(rough, metal, ao);
                    else reinterpret_cast<float4*>(a.m.t.roughMetalAO)[pix] = make_float4(rough, metal, ao, 0.0f);
                }
            }
            if constexpr (kPacked) {                                    // the reference's cleared state: all bits 0
                if (inside && !written) {
                    if (a.m.want & MATERIAL_BASECOLOR) reinterpret_cast<uint32_t*>(a.m.t.baseColor)[pix] = 0u;
                    if (a.m.want & MATERIAL_EMISSIVE) reinterpret_cast<uint2*>(a.m.t.emissive)[pix] = make_uint2(0u, 0u);
                    if (a.m.want & MATERIAL_NORMAL) reinterpret_cast<uint32_t*>(a.m.t.pixelNormal)[pix] = 0u;
                    if (a.m.want & MATERIAL_RMA) reinterpret_cast<uint32_t*>(a.m.t.roughMetalAO)[pix] = 0u;
                }
            } else if (inside && !written) {
                const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (a.m.want & MATERIAL_BASECOLOR) reinterpret_cast<float4*>(a.m.t.baseColor)[pix] = z;
                if (a.m.want & MATERIAL_EMISSIVE) reinterpret_cast<float4*>(a.m.t.emissive)[pix] = z;
                if (a.m.want & MATERIAL_NORMAL) reinterpret_cast<float4*>(a.m.t.pixelNormal)[pix] = z;
                if (a.m.want & MATERIAL_RMA) reinterpret_cast<float4*>(a.m.t.roughMetalAO)[pix] = z;
            }
        }
    }
}


// ---- material feedback (chordvis_material_feedback) ------------------------------------------------------------
// Which level of which texture the pinned sampler's finest tap lands on, counted per (texture, level) over a lattice of pixels.
// The level of sample_slot / sample_slot_aniso without their fetches: the same footprint arithmetic statement by statement, the same
// integer rule (a twin: the sampling kernels stay as they are).  kmax 0: sample_slot's l0; kmax = log2 N >= 1: sample_slot_aniso's.
struct FeedbackArgs {
    const unsigned long long* vis;
    const ChordDrawCmd* cmds;
    const uint32_t* cmdCount;
    const ChordObject* objects;
    const DObjStatic* objStatic;
    const DMeshlet* meshlets;
    const uint32_t* meshletData;
    const float* positions;
    const float* texcoords;            // null: (0, 0)
    const DView* view;
    const DMatRecord* records;
    uint32_t* taps;                    // [textureCount][CHORD_FEEDBACK_LEVELS]
    uint32_t W, H, blocksX, waveBlocks;   // the image; wave blocks (16 x 4 lattice pixels) per lattice row, and in all
    uint32_t blocksPerGroup;           // the strip of wave blocks a workgroup walks
    uint32_t objectCount, meshletCount;
    uint32_t stride, offX, offY, slotMask, kmax, tapWords;
    uint32_t tableMask;                // entries of the workgroup's table in use - 1: FEEDBACK_TABLE - 1 (chordvis_set_debug 4194304: 1)
};
#define FEEDBACK_TABLE 512u            // entries of a workgroup's table of (texture * 16 + level) -> count
#define FEEDBACK_PROBES 32u            // slots a key looks at before it gives up on the table
#define FEEDBACK_EMPTY 0xFFFFFFFFu

__device__ __forceinline__ uint32_t feedback_level(const DMatSlot& S, float4 g, uint32_t kmax)
{
    const uint32_t d0 = S.levels[0].dims;
    const float fW = (float)((d0 & 0xFFFFu) + 1u), fH = (float)((d0 >> 16) + 1u);
    int32_t lodq, lmaj;
    if (kmax == 0u) lodq = lmaj = footprint_lodq(g, fW, fH);
    else {
        const float ax = g.x * fW, ay = g.y * fH, bx = g.z * fW, by = g.w * fH;
        const float ra = ax * ax + ay * ay, rb = bx * bx + by * by;
        const float rmaj2 = fmaxf(ra, rb), rmin2 = fminf(ra, rb);
        int32_t k = 0;
        lmaj = 0;
        if (ra < __builtin_inff() && rb < __builtin_inff() && rmaj2 > 0.0f) {
            lmaj = ((int32_t)(__float_as_uint(rmaj2) >> 15) - (127 << 8)) >> 1;
            if (lmaj > 0) {
                int32_t spread = (int32_t)kmax;
                if (rmin2 > 0.0f) spread = (max(lmaj - (((int32_t)(__float_as_uint(rmin2) >> 15) - (127 << 8)) >> 1), 0) + 255) >> 8;
                k = min(min((int32_t)kmax, spread), (lmaj + 255) >> 8);
            }
        }
        lodq = max(lmaj - (k << 8), 0);
    }
    const uint32_t filter = S.filter, last = S.mips - 1u;
    uint32_t l0 = 0u;
    if (lmaj > 0) {
        if (filter & CHORD_MATSLOT_MIP_NEAREST) l0 = min((uint32_t)(lodq + 128) >> 8, last);
        else if (filter & CHORD_MATSLOT_MIP_LINEAR) l0 = min((uint32_t)lodq >> 8, last);
    }
    return l0;
}

// count more taps of `key`: the workgroup's table, open addressing from a multiplicative hash; a key that finds neither itself nor
// a free slot in FEEDBACK_PROBES steps goes to global memory
__device__ __forceinline__ void feedback_add(uint32_t* sKeys, uint32_t* sVals, uint32_t* __restrict__ taps, uint32_t tableMask, uint32_t key,
                                             uint32_t count)
{
    uint32_t h = ((key * 0x9E3779B1u) >> 23) & tableMask;               // 9 bits
    const uint32_t probes = min(FEEDBACK_PROBES, tableMask + 1u);
    for (uint32_t p = 0; p < probes; p++) {
        const uint32_t was = atomicCAS(&sKeys[h], FEEDBACK_EMPTY, key);
        if (was == FEEDBACK_EMPTY || was == key) { atomicAdd(&sVals[h], count); return; }
        h = (h + 1u) & tableMask;
    }
    atomicAdd(&taps[key], count);
}

// A wave per 16 x 4 LATTICE pixels, x = (bx * 16 + (lane & 15)) * stride + offX and y likewise: resolve_attributes_kernel's leader
// loop, the part of its per-triangle set-up and per-pixel arithmetic the uv gradients need (the same statements), and its
// wave-uniform material loop with the level rule in place of the sampler.  No texel is fetched, no image stored.  Inside a
// (material, slot) turn the lanes are balloted per distinct level and one lane adds the popcount to the workgroup's LDS table; a
// workgroup walks a strip of wave blocks and at its end adds every entry it filled to `taps` with one global atomic.
__global__ __launch_bounds__(256) void material_feedback_kernel(const FeedbackArgs a)
{
    static_assert(FEEDBACK_TABLE == 512u, "feedback_add's hash keeps 9 bits");
    __shared__ uint32_t sKeys[FEEDBACK_TABLE], sVals[FEEDBACK_TABLE];
    for (uint32_t i = threadIdx.x; i < FEEDBACK_TABLE; i += 256u) { sKeys[i] = FEEDBACK_EMPTY; sVals[i] = 0u; }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n = *a.cmdCount;
    const DView& dv = *a.view;
    const float invW = dv.view.renderDimension[2], invH = dv.view.renderDimension[3];
    const uint32_t first = blockIdx.x * a.blocksPerGroup, end = min(first + a.blocksPerGroup, a.waveBlocks);
    for (uint32_t block = first + (threadIdx.x >> 6); block < end; block += 4u) {
        const uint32_t bx = block % a.blocksX, by = block / a.blocksX;
        const uint32_t x = (bx * 16u + (lane & 15u)) * a.stride + a.offX, y = (by * 4u + (lane >> 4)) * a.stride + a.offY;
        const bool inside = x < a.W && y < a.H;
        const uint32_t low = inside ? (uint32_t)a.vis[(size_t)y * a.W + x] : 0u;
        const uint32_t slot = ((low >> 8) & CHORD_MAX_INSTANCE_ID) - 1u;   // base.hlsli:443-447
        const bool covered = low != 0u && slot < n;

        // one leader per distinct (slot, triangle) of the wave
        int leader = (int)lane;
        uint64_t pending = __ballot(covered);
        while (pending) {
            const int l = __ffsll((unsigned long long)pending) - 1;
            const uint32_t key = (uint32_t)__builtin_amdgcn_readlane((int)low, l);
            const bool mine = covered && low == key;
            if (mine) leader = l;
            pending &= ~__ballot(mine);
        }
        const bool isLeader = covered && leader == (int)lane;

        bool ok = false;
        float phs[3][4] = {}, uvv[3][2] = {};
        uint32_t matId = 0u;
        if (isLeader) {
            const ChordDrawCmd cmd = a.cmds[slot];
            const uint32_t tri = low & 0xFFu;
            if (cmd.objectId < a.objectCount && cmd.meshletId < a.meshletCount) {
                const DMeshlet& m = a.meshlets[cmd.meshletId];
                const uint32_t V = m.vertexTriangleCount & 0xFFu, T = (m.vertexTriangleCount >> 8) & 0xFFu;
                if (tri < T) {
                    ok = true;
                    const Mat4 M = load_mat(a.objects[cmd.objectId].basicData.localToTranslatedWorld);
                    const Mat4 mvp = mul_mm(load_mat(dv.iv.translatedWorldToClip), M);
                    const uint32_t triWord = a.meshletData[m.dataOffset + V + tri];
                    matId = CHORD_MATFLAG_MATERIAL(a.objStatic[cmd.objectId].matFlags);
#pragma unroll
                    for (int i = 0; i < 3; i++) {
                        const uint32_t vi = a.meshletData[m.dataOffset + ((triWord >> (8 * i)) & 0xFFu)] + m.vertexBase;
                        const float px = a.positions[(size_t)vi * 3], py = a.positions[(size_t)vi * 3 + 1], pz = a.positions[(size_t)vi * 3 + 2];
                        const f4 h = mul_mv(mvp, px, py, pz, 1.0f);
                        phs[i][0] = h.x; phs[i][1] = h.y; phs[i][2] = h.z; phs[i][3] = h.w;
                        if (a.texcoords) { uvv[i][0] = a.texcoords[(size_t)vi * 2]; uvv[i][1] = a.texcoords[(size_t)vi * 2 + 1]; }
                    }
                }
            }
        }

        const bool hit = covered && lane_read((uint32_t)ok, leader) != 0u;
        float P[3][4], U[3][2];
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int k = 0; k < 4; k++) P[i][k] = lane_read(phs[i][k], leader);
            U[i][0] = lane_read(uvv[i][0], leader); U[i][1] = lane_read(uvv[i][1], leader);
        }
        const float su = ((float)x + 0.5f) * invW, sv = ((float)y + 0.5f) * invH;
        const float pcx = 2.0f * (su - 0.5f), pcy = 2.0f * (0.5f - sv);
        // calculateTriangleBarycentrics -- base.hlsli:457-495: the derivative half
        const f3 rcpW = {1.0f / P[0][3], 1.0f / P[1][3], 1.0f / P[2][3]};
        const float p0x = P[0][0] * rcpW.x, p0y = P[0][1] * rcpW.x;
        const float p1x = P[1][0] * rcpW.y, p1y = P[1][1] * rcpW.y;
        const float p2x = P[2][0] * rcpW.z, p2y = P[2][1] * rcpW.z;
        const f3 p120x = {p1x, p2x, p0x}, p120y = {p1y, p2y, p0y}, p201x = {p2x, p0x, p1x}, p201y = {p2y, p0y, p1y};
        const f3 cdx = {p201y.x - p120y.x, p201y.y - p120y.y, p201y.z - p120y.z};
        const f3 cdy = {p120x.x - p201x.x, p120x.y - p201x.y, p120x.z - p201x.z};
        const f3 C = {cdx.x * (pcx - p120x.x) + cdy.x * (pcy - p120y.x),
                      cdx.y * (pcx - p120x.y) + cdy.y * (pcy - p120y.y),
                      cdx.z * (pcx - p120x.z) + cdy.z * (pcy - p120y.z)};
        const f3 G = {C.x * rcpW.x, C.y * rcpW.y, C.z * rcpW.z};
        const float Hs = dot3(C, rcpW);
        const float rcpH = 1.0f / Hs;
        const f3 gdx = {cdx.x * rcpW.x, cdx.y * rcpW.y, cdx.z * rcpW.z};
        const f3 gdy = {cdy.x * rcpW.x, cdy.y * rcpW.y, cdy.z * rcpW.z};
        const float hdx = dot3(cdx, rcpW), hdy = dot3(cdy, rcpW);
        const float rcpH2 = rcpH * rcpH, sx = 2.0f * invW, sy = -2.0f * invH;
        const f3 ddx = {((gdx.x * Hs - G.x * hdx) * rcpH2) * sx, ((gdx.y * Hs - G.y * hdx) * rcpH2) * sx, ((gdx.z * Hs - G.z * hdx) * rcpH2) * sx};
        const f3 ddy = {((gdy.x * Hs - G.x * hdy) * rcpH2) * sy, ((gdy.y * Hs - G.y * hdy) * rcpH2) * sy, ((gdy.z * Hs - G.z * hdy) * rcpH2) * sy};
        const float4 g = make_float4(interp3(U[0][0], U[1][0], U[2][0], ddx), interp3(U[0][1], U[1][1], U[2][1], ddx),
                                     interp3(U[0][0], U[1][0], U[2][0], ddy), interp3(U[0][1], U[1][1], U[2][1], ddy));
        const uint32_t mId = lane_read(matId, leader);

        // one turn per distinct material of the wave; its record is wave-uniform
        uint64_t left = __ballot(hit);
        while (left) {
            const int l = __ffsll((unsigned long long)left) - 1;
            const uint32_t mat = (uint32_t)__builtin_amdgcn_readlane((int)mId, l);
            const bool mine = hit && mId == mat;
            const uint64_t lanes = __ballot(mine);
            left &= ~lanes;
            const DMatRecord& M = a.records[mat];
            if (!M.pbr) continue;
            for (uint32_t s = 0; s < 4u; s++) {
                if (!((a.slotMask >> s) & 1u) || !M.slot[s].mips) continue;
                const DMatSlot& S = M.slot[s];
                const uint32_t l0 = mine ? feedback_level(S, g, a.kmax) : 0u;
                const uint32_t row = S.texture * CHORD_FEEDBACK_LEVELS;
                uint64_t rest = lanes;
                while (rest) {                                          // one turn per distinct level of the slot's lanes
                    const int q = __ffsll((unsigned long long)rest) - 1;
                    const uint32_t level = (uint32_t)__builtin_amdgcn_readlane((int)l0, q);
                    const uint64_t same = __ballot(mine && l0 == level);
                    rest &= ~same;
                    const uint32_t key = row + level;
                    if ((int)lane == q && key < a.tapWords) feedback_add(sKeys, sVals, a.taps, a.tableMask, key, (uint32_t)__popcll((unsigned long long)same));
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < FEEDBACK_TABLE; i += 256u)
        if (sKeys[i] != FEEDBACK_EMPTY && sVals[i]) atomicAdd(&a.taps[sKeys[i]], sVals[i]);
}

static ResolveArgs resolve_args(ChordCtx* c, const unsigned long long* vis, const ChordDrawCmd* cmds, const uint32_t* cmdCount,
                                const ChordResolveDesc& desc, const ChordResolveTargets& t)
{
    ResolveArgs a;
    a.vis = vis; a.cmds = cmds; a.cmdCount = cmdCount;
    a.objects = c->dObjects; a.objStatic = c->dObjStatic; a.prims = c->dPrims; a.meshlets = c->dMeshlets; a.meshletLod = c->dMeshletLod;
    a.meshletData = c->dMeshletData; a.positions = c->dPositions; a.texcoords = c->dTexcoords; a.view = c->dView;
    a.W = c->width; a.H = c->height; a.blocksX = (c->width + 15u) / 16u;
    a.objectCount = c->objectCount; a.meshletCount = c->meshletCount;
    a.useNoJitter = desc.useNoJitter; a.debugMode = desc.debugMode;
    a.want = (t.barycentrics ? RESOLVE_BARY : 0u) | (t.baryDdx ? RESOLVE_DDX : 0u) | (t.baryDdy ? RESOLVE_DDY : 0u) | (t.uv ? RESOLVE_UV : 0u) |
             (t.uvGrad ? RESOLVE_UVGRAD : 0u) | (t.positionRS ? RESOLVE_POS : 0u) | (t.motionVector ? RESOLVE_MOTION : 0u) |
             (t.debugRGBA8 ? RESOLVE_DEBUG : 0u);
    a.vpNoJitter = desc.translatedWorldToClipNoJitter; a.vpLastNoJitter = desc.translatedWorldToClipLastFrameNoJitter;
    a.t = t;
    return a;
}

void launch_resolve_attributes(ChordCtx* c, const unsigned long long* vis, const ChordDrawCmd* cmds, const uint32_t* cmdCount,
                               const ChordResolveDesc& desc, const ChordResolveTargets& t)
{
    KernelArgs<0> a;
    static_cast<ResolveArgs&>(a) = resolve_args(c, vis, cmds, cmdCount, desc, t);
    const uint32_t waves = a.blocksX * ((c->height + 3u) / 4u);
    CHORD_LAUNCH(c, resolve_attributes_kernel<0>, dim3((waves + 3u) / 4u), dim3(256), 0, c->stream, a);
}

void launch_resolve_surface(ChordCtx* c, const unsigned long long* vis, const ChordDrawCmd* cmds, const uint32_t* cmdCount,
                            const ChordResolveDesc& desc, const ChordResolveTargets& t, const ChordSurfaceTargets& s)
{
    KernelArgs<1> a;
    static_cast<ResolveArgs&>(a) = resolve_args(c, vis, cmds, cmdCount, desc, t);
    a.e.normals = c->dNormals; a.e.tangents = c->dTangents; a.e.t = s;
    a.e.want = (s.vertexNormal ? SURFACE_NORMAL : 0u) | (s.tangent ? SURFACE_TANGENT : 0u) | (s.bitangent ? SURFACE_BITANGENT : 0u);
    const uint32_t waves = a.blocksX * ((c->height + 3u) / 4u);
    CHORD_LAUNCH(c, resolve_attributes_kernel<1>, dim3((waves + 3u) / 4u), dim3(256), 0, c->stream, a);
}

// chordvis_resolve_material's launch (kPacked false) and chordvis_resolve_gbuffer's (true: the packed twin of the same level)
template <bool kPacked>
static void launch_material_level(ChordCtx* c, const unsigned long long* vis, const ChordDrawCmd* cmds, const uint32_t* cmdCount,
                                  const ChordResolveDesc& desc, const ChordResolveTargets& t, const MaterialLaunch& ml)
{
    KernelArgs<3> a;                                                     // (its KernelArgs<2> base is what N = 1 launches)
    static_cast<ResolveArgs&>(a) = resolve_args(c, vis, cmds, cmdCount, desc, t);
    const ChordSurfaceTargets& s = ml.surface;
    const ChordMaterialTargets& m = ml.material;
    a.e.normals = c->dNormals; a.e.tangents = c->dTangents; a.e.t = s;
    a.e.want = (s.vertexNormal ? SURFACE_NORMAL : 0u) | (s.tangent ? SURFACE_TANGENT : 0u) | (s.bitangent ? SURFACE_BITANGENT : 0u);
    a.m.records = c->dMatRecords; a.m.texels = c->dMatTexels; a.m.t = m;
    a.m.want = (m.baseColor ? MATERIAL_BASECOLOR : 0u) | (m.emissive ? MATERIAL_EMISSIVE : 0u) | (m.pixelNormal ? MATERIAL_NORMAL : 0u) |
               (m.roughMetalAO ? MATERIAL_RMA : 0u);
    // pixelNormal reads the pixel's vertex normal, and its tangent and bitangent when some material has a normal texture
    a.m.needSurface = m.pixelNormal ? (SURFACE_NORMAL | (c->matAnyNormalTexture ? SURFACE_TANGENT | SURFACE_BITANGENT : 0u)) : 0u;
    const uint32_t waves = a.blocksX * ((c->height + 3u) / 4u);
    const dim3 grid((waves + 3u) / 4u), block(256);
    const uint2* blocks = reinterpret_cast<const uint2*>(c->dMatBlocks);
    // (named here: a template-id with two arguments does not pass through the launch macro)
    constexpr auto kernel2 = resolve_attributes_kernel<2, kPacked>;
    constexpr auto kernel3 = resolve_attributes_kernel<3, kPacked>;
    constexpr auto kernel4 = resolve_attributes_kernel<4, kPacked>;
    constexpr auto kernel5 = resolve_attributes_kernel<5, kPacked>;
    if (c->matAnisotropy > 1u) {                                         // chordvis_set_material_anisotropy: 2, 4, 8 or 16
        a.kmax = (uint32_t)__builtin_ctz(c->matAnisotropy);
        if (c->matBlockUnits) {                                          // a chain kept as blocks (CHORD_TEXSTORE_BLOCKS): the twin that reads both stores
            KernelArgs<5> b;
            static_cast<KernelArgs<3>&>(b) = a; b.blocks = blocks;
            CHORD_LAUNCH(c, kernel5, grid, block, 0, c->stream, b);
        } else CHORD_LAUNCH(c, kernel3, grid, block, 0, c->stream, a);
    } else if (c->matBlockUnits) {
        KernelArgs<4> b;
        static_cast<KernelArgs<2>&>(b) = a; b.blocks = blocks;
        CHORD_LAUNCH(c, kernel4, grid, block, 0, c->stream, b);
    } else {
        CHORD_LAUNCH(c, kernel2, grid, block, 0, c->stream, static_cast<const KernelArgs<2>&>(a));
    }
}

void launch_resolve_material(ChordCtx* c, const unsigned long long* vis, const ChordDrawCmd* cmds, const uint32_t* cmdCount,
                             const ChordResolveDesc& desc, const ChordResolveTargets& t, const MaterialLaunch& ml)
{
    launch_material_level<false>(c, vis, cmds, cmdCount, desc, t, ml);
}

// The packed images travel in the fields of their float twins (resolve_attributes_kernel's kPacked comment)
void launch_resolve_gbuffer(ChordCtx* c, const unsigned long long* vis, const ChordDrawCmd* cmds, const uint32_t* cmdCount,
                            const ChordResolveDesc& desc, const ChordGBufferTargets& g)
{
    ChordResolveTargets t = {};
    MaterialLaunch ml = {};
    t.motionVector = reinterpret_cast<float*>(g.motionVector);
    ml.surface.vertexNormal = reinterpret_cast<float*>(g.vertexNormal);
    ml.material.baseColor = reinterpret_cast<float*>(g.baseColor);
    ml.material.emissive = reinterpret_cast<float*>(g.emissive);
    ml.material.pixelNormal = reinterpret_cast<float*>(g.pixelNormal);
    ml.material.roughMetalAO = reinterpret_cast<float*>(g.aoRoughnessMetallic);
    launch_material_level<true>(c, vis, cmds, cmdCount, desc, t, ml);
}

void launch_material_feedback(ChordCtx* c, const unsigned long long* vis, const ChordDrawCmd* cmds, const uint32_t* cmdCount,
                              const ChordFeedbackDesc& desc, uint32_t* taps, uint32_t textureCount)
{
    FeedbackArgs a;
    a.vis = vis; a.cmds = cmds; a.cmdCount = cmdCount;
    a.objects = c->dObjects; a.objStatic = c->dObjStatic; a.meshlets = c->dMeshlets; a.meshletData = c->dMeshletData;
    a.positions = c->dPositions; a.texcoords = c->dTexcoords; a.view = c->dView; a.records = c->dMatRecords; a.taps = taps;
    a.W = c->width; a.H = c->height;
    a.stride = desc.stride; a.offX = desc.offset[0]; a.offY = desc.offset[1]; a.slotMask = desc.slotMask;
    // lattice pixels per row / column: those x = i * stride + offset below the size (none when the offset is not)
    const uint32_t latW = a.offX < a.W ? (a.W - a.offX + a.stride - 1u) / a.stride : 0u, latH = a.offY < a.H ? (a.H - a.offY + a.stride - 1u) / a.stride : 0u;
    a.blocksX = (latW + 15u) / 16u;
    a.waveBlocks = a.blocksX * ((latH + 3u) / 4u);
    if (!a.waveBlocks) return;
    // strips: at most four workgroups per CU, each at least its four waves' one block
    const uint32_t groups = min((a.waveBlocks + 3u) / 4u, (uint32_t)c->numCUs * 4u);
    a.blocksPerGroup = (a.waveBlocks + groups - 1u) / groups;
    a.objectCount = c->objectCount; a.meshletCount = c->meshletCount;
    a.kmax = c->matAnisotropy > 1u ? (uint32_t)__builtin_ctz(c->matAnisotropy) : 0u;
    a.tapWords = textureCount * CHORD_FEEDBACK_LEVELS;
    a.tableMask = (c->debugFlags & 4194304u) ? 1u : FEEDBACK_TABLE - 1u;   // (the debug switch: two entries, so that most adds find the table full)
    CHORD_LAUNCH(c, material_feedback_kernel, dim3((a.waveBlocks + a.blocksPerGroup - 1u) / a.blocksPerGroup), dim3(256), 0, c->stream, a);
}

} // namespace chord
