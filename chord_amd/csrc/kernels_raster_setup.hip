// Set-up stage of the software rasterizer (overview: kernels_raster.hip): raster_setup_kernel, raster_setup_wide_kernel,
// raster_setup_blocks_kernel and, for A/B runs, raster_clip_and_bin_large_kernel; the constants only they read; their launches.

#include "raster_device.h"

#include <algorithm>

namespace chord {

#define LDS_VERTS 256

// clip triangles a set-up wave clips at once: one per lane, the polygons of CLIP_SETUP_LANES lanes in the wave's slice of sVert
// (ClipLds: 80 floats of vertices per lane in one 256-float array, 20 + 20 of texture coordinates in the next, 3 x 10 in the third)
#define CLIP_SETUP_LANES 3u
#define CLIP_RANGES 255u           // clusters with clip triangles a set-up wave keeps for its end (more: overflow bit 2, as a full clip list)
static_assert(2u * CLIP_MAXV * CLIP_SETUP_LANES * 4u <= LDS_VERTS && 4u * CLIP_MAXV * CLIP_SETUP_LANES <= LDS_VERTS && 3u * CLIP_MAXV * CLIP_SETUP_LANES <= LDS_VERTS,
              "a set-up wave's clip polygons fit its slices of sVert");

// ---- the per-cluster setup kernel -------------------------------------------------------------
// phase clocks of the wave-per-cluster bodies (profile builds: RASTER_PROFILE and DBG_SETUP_CLOCKS; their locals sprof, sph, stp)
#define SPHASE(i) do { if (sprof) { const unsigned long long tn = wall_clock64(); sph[i] += tn - stp; stp = tn; } } while (0)
#define WIN CHORD_BLOCK_WIN

// cmds / count: the list this launch sets up (the input list, or what the block kernel left over: raster_setup_kernel).
// firstCmd: the three words of THIS wave's first command (index blockIdx.x * 4 + wave), requested by the caller together with the count
// -- one round trip instead of two in front of everything else a wave does (a short list is one cluster per wave: the kernel is the
// chain count -> command -> records -> indices -> positions -> matrix -> reservations, seven dependent round trips until round 6).
template <bool MASKED>
__device__ __forceinline__ void raster_setup_body(const RasterParams& p, const ChordDrawCmd* __restrict__ cmds, const uint32_t count, float (*sVert)[4][LDS_VERTS], uint32_t* sClip,
                                                  const uint32_t firstCmd0, const uint32_t firstCmd1, const uint32_t firstCmd2, const bool firstCmdValid)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    float* lX = sVert[0][wave]; float* lY = sVert[1][wave]; float* lW = sVert[2][wave];
    float* lU = sVert[3][wave]; float* lV = sVert[4][wave]; float* lD = sVert[5][wave];

    const uint32_t listShard = (blockIdx.x * 4u + wave) % CHORD_LIST_SHARDS;

    // The chain command -> meshlet / object records -> index stream -> positions is four dependent memory round trips per cluster;
    // the header of the NEXT cluster is fetched while the current one is processed (command at the top of the iteration, records
    // after the vertex phase), which takes two of them off the critical path.
    // (scene pointers: read from the kernel-argument segment where they are used, not held across the loop)
    auto header_of = [&](uint32_t objectId, uint32_t meshletId, uint32_t slot) -> SetupHeader {
        const RasterParams* q = kernel_args();
        return load_setup_header(scalar_load(&q->meshlets), scalar_load(&q->objStatic), objectId, meshletId, slot);
    };
    auto load_header = [&](uint32_t i) -> SetupHeader {
        const ChordDrawCmd cmd = load_command(cmds, count, i);
        return header_of(cmd.objectId, cmd.meshletId, cmd.slot);
    };
    // (the object's matrix is fetched where the cluster's vertex phase starts, not an iteration ahead with the header: sixteen
    // more scalars alive across a whole cluster are lane spills -- a v_readlane each -- in a loop that sits at its 102 SGPRs)
    auto mvp_of = [&](uint32_t objectId) -> Mat4 { return load_mvp(scalar_load(&kernel_args()->objFrame), objectId); };
    // Software pipeline over clusters (a wave's clusters k, k+1, ... are `stride` apart in the list).  While cluster k is
    // processed, k+1's header is resident, its vertex indices + triangle words are fetched after k's vertex phase, its
    // positions after k's triangle arithmetic, and k+2's header at the end -- so that at the top of an iteration the
    // positions of its first 128 vertices are already in registers (or on their way) and the chain of four dependent
    // round trips command -> records -> indices -> positions is off the critical path.
    const uint32_t stride = gridDim.x * 4u;
    uint32_t c = blockIdx.x * 4u + wave;
    if (c >= count) return;
    SetupHeader hdr = firstCmdValid ? header_of(firstCmd0, firstCmd1, firstCmd2) : load_header(c);
    SetupHeader hdrN = load_header(c + stride);
    // (the first cluster's matrix travels with its index stream: behind it, a cluster's matrix is asked for while the cluster before it
    // stores its records -- see the end of the loop)
    Mat4 mvpNext = mvp_of(hdr.objectId);
    // geometry of the current cluster: vertices lane and lane + 64 (indices, then positions), triangle words
    uint32_t t0 = 0, t1 = 0;
    float pax, pay, paz, pbx, pby, pbz;
    {
        const uint32_t* __restrict__ md = scalar_load(&kernel_args()->meshletData);
        const float* __restrict__ ps = scalar_load(&kernel_args()->positions);
        const uint32_t ia = md[hdr.dataOffset + min(lane, max(hdr.V, 1u) - 1u)] + hdr.vertexBase;
        const uint32_t ib = md[hdr.dataOffset + min(lane + 64u, max(hdr.V, 1u) - 1u)] + hdr.vertexBase;
        if (lane < hdr.T) t0 = md[hdr.dataOffset + hdr.V + lane];
        if (lane + 64u < hdr.T) t1 = md[hdr.dataOffset + hdr.V + 64u + lane];
        const float* __restrict__ pa = ps + (size_t)(ia * 3u);      // (32-bit: chordvis_upload_scene refuses scenes whose vertex index x 3 would not fit)
        const float* __restrict__ pb = ps + (size_t)(ib * 3u);
        pax = pa[0]; pay = pa[1]; paz = pa[2]; pbx = pb[0]; pby = pb[1]; pbz = pb[2];
    }
    const bool sprof = RASTER_PROFILE && (p.debug & DBG_SETUP_CLOCKS) != 0;
    unsigned long long sph[5] = {0, 0, 0, 0, 0}, stp = sprof ? wall_clock64() : 0ull;
    const uint32_t laneTop = lane;
    if (lane == 0u) sClip[0] = 0u;
    for (; c < count; c += stride) {
        // (the lane index of this cluster goes through an empty asm: what the body derives from it is invariant over the cluster
        // loop and would otherwise be hoisted out of it and held in registers across the whole kernel -- raster_tile_kernel: 25 VGPRs)
        uint32_t lane = laneTop;
        asm volatile("" : "+v"(lane));
        const uint32_t slot = hdr.slot, V = hdr.V, T = hdr.T, dataOffset = hdr.dataOffset, vertexBase = hdr.vertexBase;
        const bool twoSided = (hdr.matFlags & CHORD_MATFLAG_TWO_SIDED) != 0u || p.depthOnly != 0u;                       // depth passes: cull mode NONE (mesh_raster.cpp:188-190)
        const bool masked = MASKED && CHORD_MATFLAG_ALPHA(hdr.matFlags) == CHORD_ALPHA_MASK;      // (wave-uniform)
        const Mat4 mvp = mvpNext;
        const uint32_t triWord[2] = {t0, t1};

        if (sprof) { volatile uint32_t sink = V + T; (void)sink; }
        SPHASE(0);
        // ---- vertex phase: position stream -> clip space -> LDS (mesh_raster.hlsl:84-105) ----------------
        bool notFast = false;
        auto vertex = [&](uint32_t i, float x, float y, float z) {
            const f4 h = mul_mv(mvp, x, y, z, 1.0f);                             // mesh_raster.hlsl:99
            const float aw = fabsf(h.w);
            lX[i] = h.x; lY[i] = h.y; lW[i] = h.w;
            lU[i] = h.x / aw * 0.5f + 0.5f;                                      // :159-161
            lV[i] = h.y / aw * -0.5f + 0.5f;
            const bool fast = p.depthClamp ? in_fast_volume_xy(h) : in_fast_volume(h);
            lD[i] = fast ? h.z / h.w : __builtin_nanf("");
            notFast = notFast || !fast;
        };
        if (lane < V) vertex(lane, pax, pay, paz);
        if (lane + 64u < V) vertex(lane + 64u, pbx, pby, pbz);
        for (uint32_t i = lane + 128u; i < V; i += 64u) {                        // (meshlets with more than 128 vertices)
            const float* __restrict__ pp = scalar_load(&kernel_args()->positions) + (size_t)(scalar_load(&kernel_args()->meshletData)[dataOffset + i] + vertexBase) * 3;
            vertex(i, pp[0], pp[1], pp[2]);
        }
        const bool allFast = __ballot(notFast) == 0ull;
        WAVE_LDS_SYNC();
        SPHASE(1);
        // next cluster: indices and triangle words now (its header has been resident for an iteration)
        const uint32_t* __restrict__ mdN = scalar_load(&kernel_args()->meshletData);
        const uint32_t nia = mdN[hdrN.dataOffset + min(lane, max(hdrN.V, 1u) - 1u)] + hdrN.vertexBase;
        const uint32_t nib = mdN[hdrN.dataOffset + min(lane + 64u, max(hdrN.V, 1u) - 1u)] + hdrN.vertexBase;
        const uint32_t nt0 = lane < hdrN.T ? mdN[hdrN.dataOffset + hdrN.V + lane] : 0u;
        const uint32_t nt1 = lane + 64u < hdrN.T ? mdN[hdrN.dataOffset + hdrN.V + 64u + lane] : 0u;

        // ---- triangle phase: the (up to) two triangles of a lane are evaluated first, then emitted together so
        //      that every round of list / bin reservations costs ONE atomic round trip for both ------------------
        // (masked clusters: the texture coordinates of each lane's two triangles are fetched now -- vertex index, then uv: two
        // dependent gathers -- so that they arrive behind the culls and the set-up instead of being waited for in the emission)
        float uvA[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, uvB[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (MASKED && masked && scalar_load(&kernel_args()->texcoords) != nullptr) {
            const float* __restrict__ tc = scalar_load(&kernel_args()->texcoords);
            const uint32_t* __restrict__ mdT = scalar_load(&kernel_args()->meshletData);
#pragma unroll
            for (int i = 0; i < 3; i++) {
                if (lane < T) { const size_t vi = (size_t)(mdT[dataOffset + ((t0 >> (8 * i)) & 0xFFu)] + vertexBase) * 2; uvA[2 * i] = tc[vi]; uvA[2 * i + 1] = tc[vi + 1]; }
                if (lane + 64u < T) { const size_t vi = (size_t)(mdT[dataOffset + ((t1 >> (8 * i)) & 0xFFu)] + vertexBase) * 2; uvB[2 * i] = tc[vi]; uvB[2 * i + 1] = tc[vi + 1]; }
            }
        }
        int kindA = K_NONE, kindB = K_NONE;
        TriSetup tsA, tsB;
        float dA[3] = {0.0f, 0.0f, 0.0f}, dB[3] = {0.0f, 0.0f, 0.0f};
        tsA.px0 = tsA.py0 = tsA.px1 = tsA.py1 = 0; tsB.px0 = tsB.py0 = tsB.px1 = tsB.py1 = 0;
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const uint32_t t = (uint32_t)half * 64u + lane;
            int kind = K_NONE;
            TriSetup ts;
            ts.px0 = ts.py0 = ts.px1 = ts.py1 = 0;
            float d[3] = {0.0f, 0.0f, 0.0f};
            if (t < T) {
                const uint32_t packedIdx = triWord[half];
                const uint32_t i0 = packedIdx & 0xFFu, i1 = (packedIdx >> 8) & 0xFFu, i2 = (packedIdx >> 16) & 0xFFu;
                const float x0 = lX[i0], y0 = lY[i0], w0 = lW[i0];
                const float x1 = lX[i1], y1 = lY[i1], w1 = lW[i1];
                const float x2 = lX[i2], y2 = lY[i2], w2 = lW[i2];
                bool culled = false;
                if (!twoSided) {                                                  // #0 mesh_raster.hlsl:143-149
                    const float det = (x0 * (y1 * w2 - w1 * y2) - y0 * (x1 * w2 - w1 * x2)) + w0 * (x1 * y2 - y1 * x2);
                    culled = det <= 0.0f;
                }
                culled = culled || (w0 <= 0.0f && w1 <= 0.0f && w2 <= 0.0f);     // #1 :152-155
                const float u0 = lU[i0], v0 = lV[i0], u1 = lU[i1], v1 = lV[i1], u2 = lU[i2], v2 = lV[i2];
                const float maxU = fmaxf(u0, fmaxf(u1, u2)), maxV = fmaxf(v0, fmaxf(v1, v2));
                const float minU = fminf(u0, fminf(u1, u2)), minV = fminf(v0, fminf(v1, v2));
                culled = culled || ((minU >= 1.0f || minV >= 1.0f) || (maxU <= 0.0f || maxV <= 0.0f));   // #2 :168-171
                culled = culled || (rintf(minU * p.W) == rintf(maxU * p.W) || rintf(minV * p.H) == rintf(maxV * p.H)); // #3 :174-179
                if (!culled) {
                    d[0] = lD[i0]; d[1] = lD[i1]; d[2] = lD[i2];
                    ts.payload = p.depthOnly ? 0u : encode_triangle_instance(t, slot);   // PASS_TYPE_DEPTH writes no id
                    if (!allFast && (d[0] != d[0] || d[1] != d[1] || d[2] != d[2])) {
                        kind = K_CLIP;
                    } else {
                        // (snapped per use: keeping the snapped pair per vertex in LDS, as the block kernel does, makes the workgroup
                        // 32 KB -- this kernel holds 256 vertices per wave -- and costs it its fifth wave per SIMD: config 4's set-up
                        // 154 -> 227 us per frame, measured)
                        ts.X[0] = snap(u0, p.W); ts.Y[0] = snap(v0, p.H);
                        ts.X[1] = snap(u1, p.W); ts.Y[1] = snap(v1, p.H);
                        ts.X[2] = snap(u2, p.W); ts.Y[2] = snap(v2, p.H);
                        if (tri_setup(ts, twoSided, p.Wi, p.Hi) && owns_rect(p.shard, ts.px0, ts.py0, ts.px1, ts.py1)) {
                            kind = K_EMIT;
                            if (p.biasConst != 0.0f || p.biasSlope != 0.0f) { const float o = depth_bias(ts, d, p.biasConst, p.biasSlope); d[0] += o; d[1] += o; d[2] += o; }
                        }
                    }
                }
            }
            if (ABL(p, DBG_NO_BIN)) kind = K_NONE;
            if (half == 0) { kindA = kind; tsA = ts; dA[0] = d[0]; dA[1] = d[1]; dA[2] = d[2]; }
            else           { kindB = kind; tsB = ts; dB[0] = d[0]; dB[1] = d[1]; dB[2] = d[2]; }
        }
        SPHASE(2);
        // next cluster: its positions now (the indices have arrived behind the triangle arithmetic)
        const float* __restrict__ psN = scalar_load(&kernel_args()->positions);
        const float* __restrict__ npa = psN + (size_t)(nia * 3u);
        const float* __restrict__ npb = psN + (size_t)(nib * 3u);
        const float nax = npa[0], nay = npa[1], naz = npa[2], nbx = npb[0], nby = npb[1], nbz = npb[2];
        {
            const unsigned long long lt = (1ull << lane) - 1ull;
            const unsigned long long cmA = __ballot(kindA == K_CLIP), cmB = __ballot(kindB == K_CLIP);
            const unsigned long long emA = __ballot(kindA == K_EMIT), emB = __ballot(kindB == K_EMIT);
            // the 32-byte record form takes every triangle whose vertices are at most 64 px apart; the rest go wide
            // (a masked triangle takes a 48-byte record and its extension: three slots of the wide list)
            const bool cpA = kindA == K_EMIT && !masked && fits_compact(tsA), cpB = kindB == K_EMIT && !masked && fits_compact(tsB);
            const uint32_t wSlots = masked ? 1u + CHORD_MASK_EXT_SLOTS : 1u;
            const unsigned long long ecA = __ballot(cpA), ecB = __ballot(cpB);
            const unsigned long long ewA = emA & ~ecA, ewB = emB & ~ecB;
            const bool lgA = kindA == K_EMIT && touches_many_tiles(tsA), lgB = kindB == K_EMIT && touches_many_tiles(tsB);
            const unsigned long long lmA = __ballot(lgA), lmB = __ballot(lgB);
            const uint32_t nClip = (uint32_t)(__popcll(cmA) + __popcll(cmB));
            const uint32_t nEc = (uint32_t)(__popcll(ecA) + __popcll(ecB)), nEw = (uint32_t)(__popcll(ewA) + __popcll(ewB));
            const uint32_t nLg = (uint32_t)(__popcll(lmA) + __popcll(lmB));
            {
            const RecordEmitParams e = load_record_emit_params();
            // every reservation of the cluster travels together: the list reservations (lane 0) and the bin
            // reservations; nothing is stored before they are back
            uint32_t cbase = 0, ebaseC = 0, ebaseW = 0, lbase = 0;
            if (lane == 0) {
                if (nClip) cbase = atomicAdd(&e.counters->clipTriCount[p.pass], nClip);
                if (nEc) ebaseC = atomicAdd(&e.counters->triCountC[listShard * CHORD_SHARD_STRIDE], nEc);
                if (nEw) ebaseW = atomicAdd(&e.counters->triCount[listShard * CHORD_SHARD_STRIDE], nEw * wSlots);
                if (nLg) lbase = atomicAdd(&e.counters->largeCount[p.pass][listShard * CHORD_SHARD_STRIDE], nLg);
            }
            BinTicket ticket;
            if (emA | emB) wave_bin_issue(e, kindA == K_EMIT && !lgA, tsA, kindB == K_EMIT && !lgB, tsB, lane, ticket, MASKED && masked);
            cbase = bcast(cbase, 0); ebaseC = bcast(ebaseC, 0); ebaseW = bcast(ebaseW, 0); lbase = bcast(lbase, 0);
            if (e.binInSetup && (lmA | lmB)) {
                const LargeLds LL = {{lX, lY, lU, lV, lD}};
                if (lgA) large_put(LL, lane, tsA);
                if (lgB) large_put(LL, 64u + lane, tsB);
            }
            SPHASE(3);
            mvpNext = mvp_of(hdrN.objectId);              // (the next cluster's matrix: on its way while this one's records are stored)
            if (e.binInSetup && nClip && lane == 0u) {
                // (the wave clips its clip triangles itself once its clusters are done: their ranges of the clip list wait in LDS)
                const uint32_t r = sClip[0];
                if (r < CLIP_RANGES) { sClip[1u + r] = cbase | (nClip - 1u) << 25; sClip[0] = r + 1u; } else atomicOr(&e.counters->overflow, 2u);
            }
            if (kindA == K_CLIP) {
                const uint32_t k = cbase + (uint32_t)__popcll(cmA & lt);
                if (k < e.clipTriCap) { ClipTri ct; ct.objectId = hdr.objectId; ct.meshletId = hdr.meshletId; ct.slot = hdr.slot; ct.tri = lane; e.clipTris[k] = ct; }
                else atomicOr(&e.counters->overflow, 2u);
            }
            if (kindB == K_CLIP) {
                const uint32_t k = cbase + (uint32_t)__popcll(cmA) + (uint32_t)__popcll(cmB & lt);
                if (k < e.clipTriCap) { ClipTri ct; ct.objectId = hdr.objectId; ct.meshletId = hdr.meshletId; ct.slot = hdr.slot; ct.tri = lane + 64u; e.clipTris[k] = ct; }
                else atomicOr(&e.counters->overflow, 2u);
            }
            // giX names the record in a bin: compact index, or CHORD_REC_WIDE | wide index
            uint32_t giA = 0, giB = 0;
            bool okA = false, okB = false;
            if (cpA) {
                const uint32_t li = ebaseC + (uint32_t)__popcll(ecA & lt);
                if (li < e.triCapC) { giA = listShard * e.triCapC + li; write_record_c(&e.trisC[giA], tsA, dA); okA = true; }
                else atomicOr(&e.counters->overflow, 1u);
            } else if (kindA == K_EMIT) {
                const uint32_t li = ebaseW + wSlots * (uint32_t)__popcll(ewA & lt);
                if (li + wSlots <= e.triCap) {
                    giA = listShard * e.triCap + li; write_record(&e.tris[giA], tsA, dA, twoSided, masked);
                    if (MASKED && masked) setup_emit_mask_ext(p, &e.tris[giA + 1u], triWord[0], uvA, lW, CHORD_MATFLAG_MATERIAL(hdr.matFlags), tsA.area);
                    giA |= (MASKED && masked) ? CHORD_REC_MASKED : CHORD_REC_WIDE; okA = true;
                } else atomicOr(&e.counters->overflow, 1u);
            }
            if (cpB) {
                const uint32_t li = ebaseC + (uint32_t)__popcll(ecA) + (uint32_t)__popcll(ecB & lt);
                if (li < e.triCapC) { giB = listShard * e.triCapC + li; write_record_c(&e.trisC[giB], tsB, dB); okB = true; }
                else atomicOr(&e.counters->overflow, 1u);
            } else if (kindB == K_EMIT) {
                const uint32_t li = ebaseW + wSlots * ((uint32_t)__popcll(ewA) + (uint32_t)__popcll(ewB & lt));
                if (li + wSlots <= e.triCap) {
                    giB = listShard * e.triCap + li; write_record(&e.tris[giB], tsB, dB, twoSided, masked);
                    if (MASKED && masked) setup_emit_mask_ext(p, &e.tris[giB + 1u], triWord[1], uvB, lW, CHORD_MATFLAG_MATERIAL(hdr.matFlags), tsB.area);
                    giB |= (MASKED && masked) ? CHORD_REC_MASKED : CHORD_REC_WIDE; okB = true;
                } else atomicOr(&e.counters->overflow, 1u);
            }
            // <= 2x2 tiles: straight into the bins; more: a round of their own below (or the large list)
            const LargeLds LL = {{lX, lY, lU, lV, lD}};
            if (e.binInSetup && (lmA | lmB)) {
                if (lgA && okA) LL.at(LG_GI, lane) = giA;
                if (lgB && okB) LL.at(LG_GI, 64u + lane) = giB;
            }
            if (emA | emB) wave_bin_commit(e, ticket, okA, giA, okB, giB);
            if (e.binInSetup) {
                if (lmA | lmB) wave_bin_large(e, LL, lgA && okA, lgB && okB, lane);
            } else if (lgA && okA) {
                const uint32_t k = lbase + (uint32_t)__popcll(lmA & lt);
                if (k < e.largeCap) e.largeList[(size_t)listShard * e.largeCap + k] = giA & CHORD_REC_WIDE_INDEX; else atomicOr(&e.counters->overflow, 1u);
            }
            if (lgB && okB && !e.binInSetup) {
                const uint32_t k = lbase + (uint32_t)__popcll(lmA) + (uint32_t)__popcll(lmB & lt);
                if (k < e.largeCap) e.largeList[(size_t)listShard * e.largeCap + k] = giB & CHORD_REC_WIDE_INDEX; else atomicOr(&e.counters->overflow, 1u);
            }
            }
        }
        // LDS of this wave is rewritten by the next cluster: order the reads above before those writes
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // rotate the pipeline; the header after next is fetched now and first used after the next vertex phase
        hdr = hdrN;
        hdrN = load_header(c + 2u * stride);
        t0 = nt0; t1 = nt1;
        pax = nax; pay = nay; paz = naz; pbx = nbx; pby = nby; pbz = nbz;
        SPHASE(4);
    }
    // the clip triangles of the wave's clusters: clipped, emitted and binned now, CLIP_SETUP_LANES at a time in the wave's slice of sVert
    // (in the loop, the clipper's registers came on top of the pipeline's: the kernel spilled)
    WAVE_LDS_SYNC();
    if (const uint32_t ranges = __builtin_amdgcn_readfirstlane(sClip[0])) {
        const SetupClipParams q = load_setup_clip_params();
        const ClipLds<CLIP_SETUP_LANES> L = {reinterpret_cast<float4*>(lX), lY, lY + 2u * CLIP_MAXV * CLIP_SETUP_LANES,
                                             reinterpret_cast<int32_t*>(lW), reinterpret_cast<int32_t*>(lW) + CLIP_MAXV * CLIP_SETUP_LANES,
                                             lW + 2u * CLIP_MAXV * CLIP_SETUP_LANES, lane};
        for (uint32_t i = 0; i < ranges; i++) {
            const uint32_t w = __builtin_amdgcn_readfirstlane(sClip[1u + i]), base = w & 0x1FFFFFFu, n = (w >> 25) + 1u;
            for (uint32_t k0 = 0; k0 < n; k0 += CLIP_SETUP_LANES)
                if (lane < CLIP_SETUP_LANES && k0 + lane < n && base + k0 + lane < q.clipTriCap) clip_entry<MASKED>(q, L, q.clipTris[base + k0 + lane], listShard);
        }
    }
    if (sprof && lane == 0u) {
        const uint32_t w = blockIdx.x * 4u + wave;
        if (w < CHORD_MAX_TILES * 8u / 5u) for (int i = 0; i < 5; i++) p.tilePhase[(size_t)w * 5u + i] = sph[i];
    }
}

// ---- the BLOCKS body, round 3: the same clusters -> the same blocks, organised around registers --------------------------
// Round 2's BLOCKS instantiation of raster_setup_body wanted 159 VGPRs and ran at the kernel's 128 with 22 of them in scratch
// (92 bytes per lane, re-read per cluster: the 21 GB of WRITE_SIZE the round-2 profile of BASELINE config 5 could not account
// for -- tools/microbench/write_size_calib shows the block stores themselves are counted at face value).  What it kept alive
// across the block code was the whole set-up of BOTH triangles of a lane (snapped vertices, depths, areas, bounds: 2 x 19
// registers) next to the software pipeline of the next cluster.  This body keeps, per triangle, a 2-bit kind and its pixel
// bounds (two packed registers) between the classification and the resolve, and sets a triangle up again from the wave's LDS
// copy of the vertices right before it is scan-converted, one triangle at a time.  The price is the snapping and the area of
// an emitted triangle twice (~45 VALU instructions per triangle of ~600); the division moves, it is not repeated.
// Wave-uniform records (draw command, meshlet header, object matrix) come through the scalar cache (constant address space:
// s_load instead of a vector load + v_readfirstlane per dword), and a block leaves the wave as 16-byte stores of consecutive
// word pairs (header | word 0, word 1 | word 2, ...): half the store instructions, whole 16-byte granules.

// What the block kernel needs only when a cluster's blocks are written (a few lanes, once per cluster).  Kept in scalar
// registers across the whole loop these 22 dwords push the kernel past its 102 SGPRs, and every scalar the compiler parks in a
// VGPR lane costs a VALU instruction each way (~300 v_readlane / v_writelane in the loop body: 15 % of its VALU work).  They
// are re-read from the kernel-argument segment (scalar cache) right where they are used instead; the pointer goes through an
// empty asm so that the loads cannot be hoisted back out of the loop.
struct BlockEmitParams {
    uint32_t* tileCount; uint32_t* tileBins; uint32_t binCap;
    uint32_t* binPool; uint32_t binPoolChunks; uint32_t* binPoolCount;
    unsigned long long* binChunkTab; uint32_t binStamp; uint32_t binMaxChunks;
    unsigned long long* blockPool; uint32_t blockCap;
    DeviceCounters* counters;
    uint32_t* tileTouched;
};
__device__ __forceinline__ BlockEmitParams load_block_emit_params()
{
    const RasterParams* q = kernel_args();
    BlockEmitParams e;
    e.tileCount = scalar_load(&q->tileCount); e.tileBins = scalar_load(&q->tileBins); e.binCap = scalar_load(&q->binCap);
    e.binPool = scalar_load(&q->binPool); e.binPoolChunks = scalar_load(&q->binPoolChunks); e.binPoolCount = scalar_load(&q->binPoolCount);
    e.binChunkTab = scalar_load(&q->binChunkTab); e.binStamp = scalar_load(&q->binStamp); e.binMaxChunks = scalar_load(&q->binMaxChunks);
    e.blockPool = scalar_load(&q->blockPool); e.blockCap = scalar_load(&q->blockCap);
    e.counters = scalar_load(&q->counters);
    e.tileTouched = scalar_load(&q->tileTouched);
    return e;
}

// classification of one triangle of the cluster in LDS: kind, and for K_EMIT its pixel bounds (x0 | x1 << 16, y0 | y1 << 16)
// and whether it is narrow (fits_compact).  The same culls and the same integers as raster_setup_body.
__device__ __forceinline__ int classify_triangle(const RasterParams& p, uint32_t t, uint32_t T, uint32_t packedIdx, bool twoSided, bool allFast,
                                                 const float* lX, const float* lY, const float* lW, const float* lU, const float* lV, const float* lD,
                                                 const int32_t* lSX, const int32_t* lSY, uint32_t& boxX, uint32_t& boxY, bool& narrow)
{
    boxX = 0u; boxY = 0u; narrow = false;
    if (t >= T) return K_NONE;
    const uint32_t i0 = packedIdx & 0xFFu, i1 = (packedIdx >> 8) & 0xFFu, i2 = (packedIdx >> 16) & 0xFFu;
    const float w0 = lW[i0], w1 = lW[i1], w2 = lW[i2];
    bool culled = false;
    if (!twoSided) {                                                  // #0 mesh_raster.hlsl:143-149
        const float x0 = lX[i0], y0 = lY[i0], x1 = lX[i1], y1 = lY[i1], x2 = lX[i2], y2 = lY[i2];
        const float det = (x0 * (y1 * w2 - w1 * y2) - y0 * (x1 * w2 - w1 * x2)) + w0 * (x1 * y2 - y1 * x2);
        culled = det <= 0.0f;
    }
    culled = culled || (w0 <= 0.0f && w1 <= 0.0f && w2 <= 0.0f);     // #1 :152-155
    const float u0 = lU[i0], v0 = lV[i0], u1 = lU[i1], v1 = lV[i1], u2 = lU[i2], v2 = lV[i2];
    const float maxU = fmaxf(u0, fmaxf(u1, u2)), maxV = fmaxf(v0, fmaxf(v1, v2));
    const float minU = fminf(u0, fminf(u1, u2)), minV = fminf(v0, fminf(v1, v2));
    culled = culled || ((minU >= 1.0f || minV >= 1.0f) || (maxU <= 0.0f || maxV <= 0.0f));   // #2 :168-171
    culled = culled || (rintf(minU * p.W) == rintf(maxU * p.W) || rintf(minV * p.H) == rintf(maxV * p.H)); // #3 :174-179
    if (culled) return K_NONE;
    if (!allFast) { const float d0 = lD[i0], d1 = lD[i1], d2 = lD[i2]; if (d0 != d0 || d1 != d1 || d2 != d2) return K_CLIP; }
    // (the snapped 24.8 coordinates are per-vertex values: computed once per vertex in the vertex phase, not once per use --
    // a cluster's 128 triangles name its 81 vertices 384 times, here and again in the resolve)
    const int32_t X0 = lSX[i0], Y0 = lSY[i0], X1 = lSX[i1], Y1 = lSY[i1], X2 = lSX[i2], Y2 = lSY[i2];
    const int32_t minX = min(X0, min(X1, X2)), maxX = max(X0, max(X1, X2));
    const int32_t minY = min(Y0, min(Y1, Y2)), maxY = max(Y0, max(Y1, Y2));
    // a triangle wider than 64 px is nothing a block holds: the cluster goes to the record kernel whatever else is true of
    // it (emitted and not narrow; the record kernel culls it or sets it up) -- and what is left here has deltas below 2^15:
    // the area is two full-rate 24-bit multiplies (the general 64-bit form is four quarter-rate ones, evaluated for every
    // triangle when it sits behind a select)
    if (maxX - minX > (1 << 14) || maxY - minY > (1 << 14)) return K_EMIT;
    narrow = true;
    const int32_t area2 = __mul24(X1 - X0, Y2 - Y0) - __mul24(X2 - X0, Y1 - Y0);
    if (area2 == 0 || (!twoSided && area2 > 0)) return K_NONE;
    // (sharded frames: ownership is decided per window part, below -- a cluster that straddles two ranks' tiles is small)
    const int32_t px0 = max(0, (minX + 127) >> 8), py0 = max(0, (minY + 127) >> 8);
    const int32_t px1 = min(p.Wi - 1, (maxX - 128) >> 8), py1 = min(p.Hi - 1, (maxY - 128) >> 8);
    if (px1 < px0 || py1 < py0) return K_NONE;
    boxX = (uint32_t)px0 | ((uint32_t)px1 << 16); boxY = (uint32_t)py0 | ((uint32_t)py1 << 16);
    return K_EMIT;
}

// set-up of an emitted, narrow triangle again from LDS and its scan conversion into the wave's pixel window.  `entry` is a word
// of the cluster's compacted list of emitted triangles (vertex indices in the low 24 bits, triangle number above), boxX / boxY
// the pixel bounds its classification found: the emitted triangles of a cluster -- 59 of 128 on BASELINE config 5 -- are
// resolved one per lane in one pass (a second one only when there are more than 64), not in two passes of a lane's own two
// triangles with half the lanes idle in each.  The classification accepted exactly these integers, and only narrow triangles
// reach a block: deltas below 2^15, the area from two 24-bit multiplies, its float an int32 conversion.
__device__ __forceinline__ void resolve_entry(const RasterParams& p, uint32_t entry, uint32_t boxX, uint32_t boxY, uint32_t slot,
                                              const int32_t* lSX, const int32_t* lSY, const float* lD, unsigned long long* win,
                                              int32_t bx0, int32_t by0)
{
    const uint32_t i0 = entry & 0xFFu, i1 = (entry >> 8) & 0xFFu, i2 = (entry >> 16) & 0xFFu, t = entry >> 24;
    TriSetup ts;
    ts.X[0] = lSX[i0]; ts.Y[0] = lSY[i0];
    ts.X[1] = lSX[i1]; ts.Y[1] = lSY[i1];
    ts.X[2] = lSX[i2]; ts.Y[2] = lSY[i2];
    const int32_t dx1 = ts.X[1] - ts.X[0], dy1 = ts.Y[1] - ts.Y[0], dx2 = ts.X[2] - ts.X[0], dy2 = ts.Y[2] - ts.Y[0];
    const int32_t area2 = __mul24(dx1, dy2) - __mul24(dx2, dy1);
    const int32_t area = area2 < 0 ? -area2 : area2;
    ts.s = area2 < 0 ? -1 : 1;
    ts.area = (int64_t)area;
    ts.invA = 1.0f / (float)area;
    ts.px0 = (int32_t)(boxX & 0xFFFFu); ts.px1 = (int32_t)(boxX >> 16);
    ts.py0 = (int32_t)(boxY & 0xFFFFu); ts.py1 = (int32_t)(boxY >> 16);
    float d[3] = {lD[i0], lD[i1], lD[i2]};
    if (p.biasConst != 0.0f || p.biasSlope != 0.0f) { const float o = depth_bias(ts, d, p.biasConst, p.biasSlope); d[0] += o; d[1] += o; d[2] += o; }
    ts.payload = p.depthOnly ? 0u : encode_triangle_instance(t, slot);
    ts.d0 = d[0]; ts.e1 = d[1] - d[0]; ts.e2 = d[2] - d[0];
    // (two copies of the pixel loop rather than a clamp + select per pixel that main-view frames never need)
    if (p.depthClamp != 0u) tile_raster_narrow<WIN>(win, ts, bx0, by0, ts.px0, ts.py0, ts.px1, ts.py1, false, true);
    else tile_raster_narrow<WIN>(win, ts, bx0, by0, ts.px0, ts.py0, ts.px1, ts.py1, false, false);
}

// Hot tiles (BASELINE config 5, variant "hotspot": one screen tile receives 12 % of the frame's 10 M blocks): every bin slot
// is a returning atomic on the tile's counter line, and a line retires ~88 of them per microsecond -- 1.26 M slots of the
// hottest tile are 14 ms of a 17.5-ms kernel spent in one queue.  Once a tile's bin holds SLOT_HOT entries, a wave that draws
// from it takes SLOT_AHEAD slots with one atomic and serves its next clusters in that tile from the reserve (a per-wave,
// direct-mapped table in LDS); what is left of a reserve when the wave ends is filled with the "no entry" word the tile
// kernel skips.  Tiles below the threshold -- every tile of every other workload -- never enter the table.
// (SLOT_HOT: raster_params.h -- launch_raster reads it too; SLOT_VERY_HOT: raster_device.h -- the tile schedule reads it too)
#define SLOT_CACHE 32u
#ifndef SLOT_AHEAD
#define SLOT_AHEAD 8u
#endif
// ... and four times as many once the bin is a quarter of a million entries long: a rank of a sharded frame that owns such a tile
// owns little else, every one of its waves draws from that one counter line, and the queue on the line is what the kernel
// waits for (BASELINE config 5's hotspot at 8 ranks, the rank with the 1.34 M-entry tile: 7.6 -> 6.6 ms per frame; drawing 32
// ahead everywhere costs the one-GPU frame 4 %: every wave leaves up to 31 unused slots in each of the ~40 hot tiles it touched)
#ifndef SLOT_AHEAD_VERY_HOT
#define SLOT_AHEAD_VERY_HOT 32u
#endif
struct SlotCache { uint32_t key[SLOT_CACHE], next[SLOT_CACHE], end[SLOT_CACHE]; uint32_t pend; };   // key = tile + 1 (0: free), slots [next, end) in reserve; pend: lane 0's draw in flight

#ifndef BLOCKS_LDS_VERTS
#define BLOCKS_LDS_VERTS 128    // vertices per cluster the block kernel takes (larger clusters are left to the record kernel): 12 + 8 KB of LDS per workgroup
#endif
template <bool HOT>
__device__ __forceinline__ void raster_setup_blocks_body(const RasterParams& p, const uint32_t count, float (*sVert)[4][BLOCKS_LDS_VERTS], int32_t (*sSnap)[4][BLOCKS_LDS_VERTS],
                                                         unsigned long long (*sWin)[WIN * WIN], SlotCache* slotCaches)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    SlotCache& sc = slotCaches[HOT ? wave : 0u];
    if (HOT && lane < SLOT_CACHE) { sc.key[lane] = 0u; sc.next[lane] = 0u; sc.end[lane] = 0u; }
    if (HOT) {
        // the tiles that were hot in the last frame are hot from this launch's first cluster on: a tile used to become hot only once its
        // bin held SLOT_HOT entries IN THIS LAUNCH, i.e. every frame began with 65 536 single draws from one counter line (~0.75 ms
        // at the ~88 returning atomics per microsecond a line sustains) and 24 k draws of eight before the draws of 32 -- with every wave of
        // the rank that owns the tile queued on it.  An entry with an empty reserve at position p draws ahead on its first use, 32
        // slots when p >= SLOT_VERY_HOT; a tile that has cooled down since costs a few "no entry" words at the end of the launch.
        const uint32_t* __restrict__ hl = scalar_load(&kernel_args()->hotTiles);
        WAVE_LDS_SYNC();
        if (hl) {
            const uint32_t nHot = min(hl[0], (uint32_t)CHORD_HOT_TILES);
            if (lane < nHot) {
                const uint32_t e = hl[1u + lane], tile = e & 0xFFFu, ci = tile & (SLOT_CACHE - 1u);
                const uint32_t pos = (e >> 31) ? SLOT_VERY_HOT : 0u;
                sc.key[ci] = tile + 1u; sc.next[ci] = pos; sc.end[ci] = pos;           // (two hot tiles on one entry: either wins)
            }
        }
        WAVE_LDS_SYNC();
    }
    float* lX = sVert[0][wave]; float* lY = sVert[1][wave]; float* lW = sVert[2][wave];
    float* lU = sVert[3][wave]; float* lV = sVert[4][wave]; float* lD = sVert[5][wave];
    int32_t* lSX = sSnap[0][wave]; int32_t* lSY = sSnap[1][wave];
    unsigned long long* win = sWin[wave];
    const uint32_t listShard = (blockIdx.x * 4u + wave) % CHORD_LIST_SHARDS;

    // the scene pointers are re-read from the kernel-argument segment where they are used (kernel_args; keeping them in
    // registers -- the "hot parameters" variant of profiles/r03_block_kernel_variants.txt -- cost 3 %)
    auto kq = [&]() -> const RasterParams* { return kernel_args(); };
    auto header_at = [&](uint32_t i) -> SetupHeader {
        const RasterParams* q = kq();
        const ChordDrawCmd cmd = load_command(scalar_load(&q->cmds), count, i);
        return load_setup_header(scalar_load(&q->meshlets), scalar_load(&q->objStatic), cmd.objectId, cmd.meshletId, cmd.slot);
    };
    const uint32_t stride = gridDim.x * 4u;
    uint32_t c = blockIdx.x * 4u + wave;
    if (c >= count) return;
    SetupHeader hdr = header_at(c);
    SetupHeader hdrN = header_at(c + stride);
    uint32_t t0 = 0, t1 = 0;
    float pax, pay, paz, pbx, pby, pbz;
    {
        const uint32_t* __restrict__ md = scalar_load(&kq()->meshletData);
        const float* __restrict__ ps = scalar_load(&kq()->positions);
        const uint32_t ia = md[hdr.dataOffset + min(lane, max(hdr.V, 1u) - 1u)] + hdr.vertexBase;
        const uint32_t ib = md[hdr.dataOffset + min(lane + 64u, max(hdr.V, 1u) - 1u)] + hdr.vertexBase;
        if (lane < hdr.T) t0 = md[hdr.dataOffset + hdr.V + lane];
        if (lane + 64u < hdr.T) t1 = md[hdr.dataOffset + hdr.V + 64u + lane];
        const float* __restrict__ pa = ps + (size_t)(ia * 3u);      // (32-bit: chordvis_upload_scene refuses scenes whose vertex index x 3 would not fit)
        const float* __restrict__ pb = ps + (size_t)(ib * 3u);
        pax = pa[0]; pay = pa[1]; paz = pa[2]; pbx = pb[0]; pby = pb[1]; pbz = pb[2];
    }
    const bool sprof = RASTER_PROFILE && (p.debug & DBG_SETUP_CLOCKS) != 0;
    unsigned long long sph[5] = {0, 0, 0, 0, 0}, stp = sprof ? wall_clock64() : 0ull;
    // (the per-cluster opaque lane index of raster_setup_body was measured here too: 78 -> 76 VGPRs, but 928 -> 946 VALU wave-instructions
    // per cluster -- this kernel is bound by VALU issue, and what was hoisted out of its loop was arithmetic it now repeats; not kept)
    for (; c < count; c += stride) {
        const uint32_t V = hdr.V, T = hdr.T, dataOffset = hdr.dataOffset, vertexBase = hdr.vertexBase;
        const bool twoSided = (hdr.matFlags & CHORD_MATFLAG_TWO_SIDED) != 0u || p.depthOnly != 0u;
        const bool masked = CHORD_MATFLAG_ALPHA(hdr.matFlags) == CHORD_ALPHA_MASK;
        if (sprof) { volatile uint32_t sink = V + T; (void)sink; }
        SPHASE(0);
        const bool tooBig = V > (uint32_t)BLOCKS_LDS_VERTS;                  // (wave-uniform) more vertices than the wave's LDS arrays hold
        (void)dataOffset; (void)vertexBase;
        // ---- vertex phase (mesh_raster.hlsl:84-105), as raster_setup_body -------------------------------------------------
        bool notFast = false;
        if (!tooBig) {
            // (fetched here, not an iteration ahead: sixteen more scalar registers alive across the whole cluster cost more
            // lane spills than the other resident waves cover of this one scalar-cache round trip)
            const Mat4 mvp = load_mvp(scalar_load(&kq()->objFrame), hdr.objectId);
            auto vertex = [&](uint32_t i, float x, float y, float z) {
                const f4 h = mul_mv(mvp, x, y, z, 1.0f);
                const float aw = fabsf(h.w);
                lX[i] = h.x; lY[i] = h.y; lW[i] = h.w;
                const float u = h.x / aw * 0.5f + 0.5f, v = h.y / aw * -0.5f + 0.5f;
                lU[i] = u; lV[i] = v;
                // snapped 24.8 coordinates of the vertex (mesh_raster setup: the values every triangle on it uses; a vertex outside
                // the guard band may overflow the conversion -- its triangles take the clipper and never read them)
                lSX[i] = snap(u, p.W); lSY[i] = snap(v, p.H);
                const bool fast = p.depthClamp ? in_fast_volume_xy(h) : in_fast_volume(h);
                lD[i] = fast ? h.z / h.w : __builtin_nanf("");
                notFast = notFast || !fast;
            };
            if (lane < V) vertex(lane, pax, pay, paz);
            if (lane + 64u < V) vertex(lane + 64u, pbx, pby, pbz);
#if BLOCKS_LDS_VERTS > 128
            for (uint32_t i = lane + 128u; i < V; i += 64u) {
                const float* __restrict__ pp = scalar_load(&kq()->positions) + (size_t)(scalar_load(&kq()->meshletData)[dataOffset + i] + vertexBase) * 3;
                vertex(i, pp[0], pp[1], pp[2]);
            }
#endif
        }
        const bool allFast = __ballot(notFast) == 0ull;
        WAVE_LDS_SYNC();
        SPHASE(1);
        // next cluster: vertex indices and triangle words
        const uint32_t* __restrict__ md = scalar_load(&kq()->meshletData);
        const uint32_t nia = md[hdrN.dataOffset + min(lane, max(hdrN.V, 1u) - 1u)] + hdrN.vertexBase;
        const uint32_t nib = md[hdrN.dataOffset + min(lane + 64u, max(hdrN.V, 1u) - 1u)] + hdrN.vertexBase;
        const uint32_t nt0 = lane < hdrN.T ? md[hdrN.dataOffset + hdrN.V + lane] : 0u;
        const uint32_t nt1 = lane + 64u < hdrN.T ? md[hdrN.dataOffset + hdrN.V + 64u + lane] : 0u;

        // ---- classification: kind + pixel bounds per triangle, nothing else survives it ----------------------------------
        uint32_t bxA, byA, bxB, byB;
        bool nwA, nwB;
        int kindA = classify_triangle(p, lane, tooBig ? 0u : T, t0, twoSided, allFast, lX, lY, lW, lU, lV, lD, lSX, lSY, bxA, byA, nwA);
        int kindB = classify_triangle(p, lane + 64u, tooBig ? 0u : T, t1, twoSided, allFast, lX, lY, lW, lU, lV, lD, lSX, lSY, bxB, byB, nwB);
        if (ABL(p, DBG_NO_BIN)) { kindA = K_NONE; kindB = K_NONE; }
        SPHASE(2);
        // next cluster: its positions (the indices have arrived behind the classification)
        const float* __restrict__ ps = scalar_load(&kq()->positions);
        const float* __restrict__ npa = ps + (size_t)(nia * 3u);
        const float* __restrict__ npb = ps + (size_t)(nib * 3u);
        const float nax = npa[0], nay = npa[1], naz = npa[2], nbx = npb[0], nby = npb[1], nbz = npb[2];

        const bool eA = kindA == K_EMIT, eB = kindB == K_EMIT;
        const unsigned long long emA = __ballot(eA), emB = __ballot(eB);
        const unsigned long long bad = __ballot(kindA == K_CLIP || kindB == K_CLIP || (eA && !nwA) || (eB && !nwB)) | (tooBig && T != 0u ? 1ull : 0ull);
        bool blocksDone = false;
        if (!masked && (emA | emB) != 0ull && bad == 0ull) {
            int32_t bx0 = min(eA ? (int32_t)(bxA & 0xFFFFu) : 0x7FFF, eB ? (int32_t)(bxB & 0xFFFFu) : 0x7FFF);
            int32_t by0 = min(eA ? (int32_t)(byA & 0xFFFFu) : 0x7FFF, eB ? (int32_t)(byB & 0xFFFFu) : 0x7FFF);
            int32_t bx1 = max(eA ? (int32_t)(bxA >> 16) : -1, eB ? (int32_t)(bxB >> 16) : -1);
            int32_t by1 = max(eA ? (int32_t)(byA >> 16) : -1, eB ? (int32_t)(byB >> 16) : -1);
            if (__ballot(bx1 - bx0 >= WIN || by1 - by0 >= WIN) == 0ull) {            // (no single lane is already too wide)
                wave_min2_max2(bx0, by0, bx1, by1);
                const int32_t bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
                const uint32_t nE = (uint32_t)(__popcll(emA) + __popcll(emB));
                if (bw <= WIN && bh <= WIN && (uint32_t)(bw * bh + 8) * 8u <= nE * 36u) {
                    blocksDone = true;
                    // the window's parts per tile (<= 2 x 2): lane r < 4 owns the part in tile (r & 1 ? tx1 : tx0, r & 2 ? ty1 : ty0)
                    const int32_t tx0 = bx0 >> TILE_SHIFT, tx1 = bx1 >> TILE_SHIFT, ty0 = by0 >> TILE_SHIFT, ty1 = by1 >> TILE_SHIFT;
                    const uint32_t r = lane & 3u;
                    const bool sx = (r & 1u) != 0u, sy = (r & 2u) != 0u;
                    const int32_t rx0 = sx ? tx1 << TILE_SHIFT : bx0, rx1 = (sx || tx1 == tx0) ? bx1 : (tx0 << TILE_SHIFT) + TILE - 1;
                    const int32_t ry0 = sy ? ty1 << TILE_SHIFT : by0, ry1 = (sy || ty1 == ty0) ? by1 : (ty0 << TILE_SHIFT) + TILE - 1;
                    const uint32_t rw = (uint32_t)(rx1 - rx0 + 1), rh = (uint32_t)(ry1 - ry0 + 1);
                    const bool has = lane < 4u && !(sx && tx1 == tx0) && !(sy && ty1 == ty0) && owns_tile(p.shard, sx ? tx1 : tx0, sy ? ty1 : ty0);
                    const uint32_t hasMask = (uint32_t)__ballot(has) & 15u;
                    const uint32_t gran = has ? (rw * rh + 2u) >> 1 : 0u;              // header + w x h words, in 16-byte granules
                    const uint32_t g0 = bcast(gran, 0), g1 = bcast(gran, 1), g2 = bcast(gran, 2), g3 = bcast(gran, 3);
                    const uint32_t before = (r > 0u ? g0 : 0u) + (r > 1u ? g1 : 0u) + (r > 2u ? g2 : 0u), G = g0 + g1 + g2 + g3;
                    const uint32_t tile = __umul24((uint32_t)(sy ? ty1 : ty0), p.tilesX) + (uint32_t)(sx ? tx1 : tx0);
                    // one round trip: pool space (lane 0) and, per touched tile, ONE 64-bit add on the tile's counter pair
                    // (low word: bin slot, high word: the tile's block count) ...
                    uint32_t gbase = 0, slot = 0;
                    const BlockEmitParams e = load_block_emit_params();
                    // (lane 0's part -- the tile of the window's first pixel -- may be served from this wave's reserve on a hot tile)
                    // (what lane 0 drew -- 0: from the reserve, else the number of slots -- waits in LDS, not in a register, for the
                    // resolve to finish)
                    {
                        uint32_t ahead = 1u;
                        if (HOT) {
                            const uint32_t ci = tile & (SLOT_CACHE - 1u);
                            if (lane == 0u && has && sc.key[ci] == tile + 1u) {
                                const uint32_t nx = sc.next[ci];
                                if (nx < sc.end[ci]) { slot = nx; sc.next[ci] = nx + 1u; ahead = 0u; }
                                else ahead = nx >= SLOT_VERY_HOT ? SLOT_AHEAD_VERY_HOT : SLOT_AHEAD;   // a hot tile whose reserve is used up: draw ahead again
                            }
                            if (lane == 0u) sc.pend = ahead;
                        }
                        if (lane == 0u && G) gbase = atomicAdd(&e.counters->blockGranules[listShard * CHORD_SHARD_STRIDE], G);
                        if (has && ahead) slot = (uint32_t)atomicAdd(reinterpret_cast<unsigned long long*>(&e.tileCount[(size_t)tile * TC_STRIDE]), (unsigned long long)ahead * 0x100000001ull);
                    }
                    // ... and the cluster is resolved while they are in flight.  The emitted triangles are compacted first (the
                    // clip-space arrays x, y, w are dead behind the classification: the list and the two bound words take their place)
                    uint32_t* lList = reinterpret_cast<uint32_t*>(lX);
                    uint32_t* lBoxX = reinterpret_cast<uint32_t*>(lY);
                    uint32_t* lBoxY = reinterpret_cast<uint32_t*>(lW);
                    const uint32_t nA = (uint32_t)__popcll(emA);
                    WAVE_LDS_SYNC();                                             // (every lane's classification has read them)
                    if (eA) { const uint32_t k = mbcnt64(emA); lList[k] = (t0 & 0xFFFFFFu) | lane << 24; lBoxX[k] = bxA; lBoxY[k] = byA; }
                    if (eB) { const uint32_t k = nA + mbcnt64(emB); lList[k] = (t1 & 0xFFFFFFu) | (lane + 64u) << 24; lBoxX[k] = bxB; lBoxY[k] = byB; }
#pragma unroll
                    for (int k = 0; k < WIN * WIN / 64; k++) win[lane + 64u * k] = 0ull;
                    WAVE_LDS_SYNC();
                    // (a sharded frame's cluster none of whose window parts is this rank's: the conservative cluster test let it through)
                    const bool anyPart = hasMask != 0u;
                    if (anyPart) {
                        if (lane < nE) resolve_entry(p, lList[lane], lBoxX[lane], lBoxY[lane], hdr.slot, lSX, lSY, lD, win, bx0, by0);
                        if (nE > 64u) {                                          // (wave-uniform; one triangle's set-up alive at a time)
                            __builtin_amdgcn_sched_barrier(0);
                            if (lane + 64u < nE) resolve_entry(p, lList[lane + 64u], lBoxX[lane + 64u], lBoxY[lane + 64u], hdr.slot, lSX, lSY, lD, win, bx0, by0);
                        }
                    }
                    WAVE_LDS_SYNC();
                    SPHASE(3);
                    gbase = bcast(gbase, 0);
                    const bool fits = gbase + G <= e.blockCap;
                    if (!fits && lane == 0u) atomicOr(&e.counters->overflow, 1u);
                    const uint32_t off = listShard * e.blockCap + gbase + before;              // granule offset of lane r's block
                    uint32_t drew = 1u;
                    if (HOT) {
                        if (lane == 0u) drew = sc.pend;
                        if (lane == 0u && has && drew) {
                            const uint32_t ci = tile & (SLOT_CACHE - 1u);
                            if (drew > 1u) {
                                sc.next[ci] = slot + 1u; sc.end[ci] = slot + drew;
                                for (uint32_t k = 1u; k < drew; k++) bin_alloc(e, tile, slot + k);   // (every drawn slot, before the first store)
                            } else if (slot >= scalar_load(&kq()->slotHot) && (sc.key[ci] == 0u || sc.next[ci] >= sc.end[ci])) {
                                sc.key[ci] = tile + 1u; sc.next[ci] = 0u; sc.end[ci] = 0u;           // hot from now on (an entry with a live reserve is never replaced)
                            }
                        }
                    }
                    if (has && drew) bin_alloc(e, tile, slot);
                    if (has && fits) bin_put(e, tile, slot, CHORD_REC_BLOCK | off);
                    if (fits) {
                        for (uint32_t q = 0; q < 4u; q++) {                      // (wave-uniform: the parts that exist, one in 4 of 5 clusters)
                            if (!((hasMask >> q) & 1u)) continue;
                            const uint32_t qoff = bcast(off, (int)q), qw = bcast(rw, (int)q), qh = bcast(rh, (int)q);
                            const uint32_t qx = (uint32_t)bcast(rx0 - bx0, (int)q), qy = (uint32_t)bcast(ry0 - by0, (int)q);
                            const uint32_t qlx = (uint32_t)bcast(rx0 & (TILE - 1), (int)q), qly = (uint32_t)bcast(ry0 & (TILE - 1), (int)q);
                            const uint32_t n = qw * qh, gq = (n + 2u) >> 1;
                            // ceil(65536 / w), w <= 16: exact from the 1-ulp reciprocal (the quotient is an integer only for powers of two, where
                            // the reciprocal is exact, and otherwise at least 1/16 away from one)
                            const uint32_t rcp = (uint32_t)ceilf(65536.0f * __builtin_amdgcn_rcpf((float)qw));
                            const unsigned long long header = (unsigned long long)(qlx | qly << 6 | (qw - 1u) << 12 | (qh - 1u) << 16) | ((unsigned long long)rcp << 32);
                            ulonglong2* dst = reinterpret_cast<ulonglong2*>(e.blockPool + (size_t)qoff * 2u);
                            for (uint32_t g = lane; g < gq; g += 64u) {
                                // granule g = words 2g - 1, 2g of the block (word -1: the header)
                                const uint32_t j1 = 2u * g, j0 = g == 0u ? 0u : j1 - 1u;
                                // (24-bit multiplies, full rate: j < 512, rcp <= 65536, row < 16, w <= 16)
                                const uint32_t row0 = __umul24(j0, rcp) >> 16, row1 = __umul24(j1, rcp) >> 16;   // exact for j < 256, w <= 16
                                const unsigned long long w0 = g == 0u ? header : win[(qy + row0) * WIN + qx + (j0 - __umul24(row0, qw))];
                                const unsigned long long w1 = j1 < n ? win[(qy + row1) * WIN + qx + (j1 - __umul24(row1, qw))] : 0ull;
                                dst[g] = make_ulonglong2(w0, w1);
                            }
                        }
                    }
                }
            }
        }
        if (!blocksDone && ((emA | emB) != 0ull || bad != 0ull)) {
            // not a block (large, clipped, masked, wide window, too few triangles for its window): the cluster goes to the
            // record kernel that follows this one (raster_setup_kernel reads the leftover list of a dense launch)
            if (lane == 0u) {
                const uint32_t k = atomicAdd(scalar_load(&kq()->leftCount), 1u);
                ChordDrawCmd cmd; cmd.objectId = hdr.objectId; cmd.meshletId = hdr.meshletId; cmd.slot = hdr.slot;
                scalar_load(&kq()->leftCmds)[k] = cmd;                                      // (capacity = the input list's: never full)
            }
            SPHASE(3);
        }
        // LDS of this wave is rewritten by the next cluster: order the reads above before those writes
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        hdr = hdrN;
        hdrN = header_at(c + 2u * stride);
        t0 = nt0; t1 = nt1;
        pax = nax; pay = nay; paz = naz; pbx = nbx; pby = nby; pbz = nbz;
        SPHASE(4);
    }
    // what is left of the reserves: "no entry" words (the tile kernel skips them; the slots are counted in the bin's length)
    if (HOT) WAVE_LDS_SYNC();
    if (HOT && lane < SLOT_CACHE && sc.key[lane] != 0u && sc.next[lane] < sc.end[lane]) {
        const BlockEmitParams e = load_block_emit_params();
        for (uint32_t k = sc.next[lane]; k < sc.end[lane]; k++) bin_put(e, sc.key[lane] - 1u, k, 0xFFFFFFFFu);
    }
    if (sprof && lane == 0u) {
        const uint32_t w = blockIdx.x * 4u + wave;
        if (w < CHORD_MAX_TILES * 8u / 5u) for (int i = 0; i < 5; i++) p.tilePhase[(size_t)w * 5u + i] = sph[i];
    }
#undef SPHASE
}

// Which clusters a launch of the record kernel sets up.  Pixel blocks pay when clusters are small, and then there are many of
// them: a launch is DENSE when its clusters have fewer than 16 pixels of this rank's screen each on average (BASELINE config
// 5: one pixel per cluster; config 4: 32; config 3: 2 000).  A dense launch runs raster_setup_blocks_kernel first, which turns
// every cluster it can into pixel blocks and leaves the others in the leftover list; the record kernel then sets up the
// leftover list instead of the input list.  Either way the image is the same.  (Both kernels evaluate this from the same
// device-side count; the host only knows whether a list COULD be dense, from its capacity, and skips the block kernel
// when it cannot.)
__device__ __forceinline__ bool launch_is_dense(const RasterParams& p, uint32_t count)
{
    const unsigned long long pixels = (unsigned long long)p.Wi * (unsigned long long)p.Hi / (p.shard.ranks > 1u ? p.shard.ranks : 1u);
    return p.blockCap != 0u && p.leftCmds != nullptr && (p.blockForce != 0u || (unsigned long long)count * 16ull >= pixels);
}

#ifndef SETUP_MIN_WAVES
#define SETUP_MIN_WAVES 5       // waves per SIMD the register allocation of the record kernel aims at (94 VGPRs since the area form is chosen per wave; 4 -> 5: config 4 0.420 -> 0.411 ms)
#endif
#ifndef BLOCKS_MIN_WAVES
#define BLOCKS_MIN_WAVES 6      // ... of the block kernel (80 VGPRs, 20 KB of LDS per 256 threads, 106 SGPRs: 6 workgroups per CU)
#endif
// MASKED: the scene has alpha-tested materials (their clusters emit 48-byte records with a texture-coordinate extension);
// scenes without any -- every benchmark configuration -- run the instantiation that knows nothing of them.
#ifndef SETUP_MASKED_WAVES
#define SETUP_MASKED_WAVES 4
#endif
template <bool MASKED>
__global__ __launch_bounds__(256, MASKED ? SETUP_MASKED_WAVES : SETUP_MIN_WAVES) void raster_setup_kernel(RasterParams p)   // (masked: twelve more live registers, see uvA)
{
    __shared__ __attribute__((aligned(16))) float sVert[6][4][LDS_VERTS];   // x, y, w, u, v, depth of a wave's cluster (24 KB; 16-byte aligned: ClipLds)
    __shared__ uint32_t sClip[4][1 + CLIP_RANGES];             // a wave's ranges of the clip list (binInSetup: count, then base | (n - 1) << 25)
    // the wave's first command is asked for TOGETHER with the count (the list has room for the index whatever the count turns out to be)
    const uint32_t c0 = __builtin_amdgcn_readfirstlane(min(blockIdx.x * 4u + (threadIdx.x >> 6), p.cmdCap - 1u));
    const uint32_t* __restrict__ cw = reinterpret_cast<const uint32_t*>(p.cmds + c0);
    const uint32_t f0 = scalar_load(cw), f1 = scalar_load(cw + 1), f2 = scalar_load(cw + 2);
    uint32_t count = *p.count;
    const ChordDrawCmd* cmds = p.cmds;
    bool firstValid = true;
    if (launch_is_dense(p, count)) { count = *p.leftCount; cmds = p.leftCmds; firstValid = false; }   // (what the block kernel left over: another list)
    raster_setup_body<MASKED>(p, cmds, count, sVert, sClip[threadIdx.x >> 6], f0, f1, f2, firstValid);
}

// ---- the wide set-up kernel: one 256-thread workgroup per cluster (light later passes) ------------------------------------
// A light later pass (config 3's second pass: 205 clusters) fills a fifth of the device with raster_setup_kernel's one wave per
// cluster, and that launch lasts as long as one wave's chain: two rounds of the vertex phase, two triangles per lane, then its large
// records and clip triangles one after another.  Here the four waves of a workgroup share one cluster: vertex i on thread i (one
// pass over up to 256 vertices), triangle t on lane t % 32 of wave t / 32, the (record, candidate tile) pairs of the cluster's large
// records dealt over all 256 threads, and the clip triangles CLIP_SETUP_LANES per wave.  Same arithmetic, same records, bin entries
// and counters as raster_setup_body (only the order of slots inside lists and bins differs, as it does from run to run).
// Reservations: one memory round trip per cluster as in the wave form.  Every primary tile of the cluster's records goes into an LDS
// table (tile -> count; the LDS atomic's return is the thread's rank); after a barrier one thread per distinct tile issues the bin
// reservation while thread 0 issues the list reservations, the bases come back through the same table, and only then is anything
// stored.  A slot is allocated for (bin_alloc) by the thread that stores it, right after that barrier and before any wait.
// launch_raster takes it for light later passes only (RasterParams::orderKept == 2); it needs binInSetup.  The host's choice rests on
// a report of a frame long past: a list longer than RasterParams::wideMax (a camera cut, a path across the light / heavy edge) is set
// up by the same launch one wave per cluster (raster_setup_body), so a long list costs what it costs raster_setup_kernel.
#define WIDE_HASH 1024u                // table entries: more than the 4 x 128 primary tiles a cluster can have, so a probe always ends
#define WIDE_EMPTY 0xFFFFFFFFu
#ifndef SETUP_WIDE_WAVES
#define SETUP_WIDE_WAVES 4              // waves per SIMD (workgroups per CU) the wide kernel's registers aim at; the host's grid is numCUs x this
#endif
template <bool MASKED>
__global__ __launch_bounds__(256, SETUP_WIDE_WAVES) void raster_setup_wide_kernel(RasterParams p)
{
    // The LDS of raster_setup_kernel (the form a long list falls back to); the wide form carves its arrays out of sVert.
    __shared__ __attribute__((aligned(16))) float sVert[6][4][LDS_VERTS];
    __shared__ uint32_t sClipW[4][1 + CLIP_RANGES];
    float* const sBuf = &sVert[0][0][0];
    // 0..5: x, y, w, u, v, depth of the cluster's vertices; 6..10: its large records (LargeLds, record k = triangle k);
    // after the cluster loop: the clip polygons, arrays 3w .. 3w + 2 for wave w (ClipLds)
    float (*const sV)[LDS_VERTS] = reinterpret_cast<float (*)[LDS_VERTS]>(sBuf);
    uint32_t* const sKey = reinterpret_cast<uint32_t*>(sBuf + 12u * LDS_VERTS);          // primary tile -> records binned there
    uint32_t* const sCnt = sKey + WIDE_HASH;                                               // ... (then: the bin's base)
    uint32_t* const sIncl = sCnt + WIDE_HASH;              // [128] large records: inclusive prefix of their candidate tile counts
    uint32_t (*const sWave)[4] = reinterpret_cast<uint32_t (*)[4]>(sIncl + 128);   // per wave: clip triangles, compact, wide, large records
    uint32_t* const sBase = sIncl + 128 + 16;              // [3] list bases of the cluster: clip, compact, wide
    static_assert(12u * LDS_VERTS + 2u * WIDE_HASH + 128u + 16u + 3u <= 6u * 4u * LDS_VERTS, "the wide form's arrays fit sVert");
    uint32_t* const sClip = sClipW[0];                     // the workgroup's ranges of the clip list (count, then base | (n - 1) << 25)
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // the workgroup's first command is asked for together with the count (the list has room for the index whatever the count is)
    const uint32_t c0 = __builtin_amdgcn_readfirstlane(min(blockIdx.x, p.cmdCap - 1u));
    const uint32_t* __restrict__ cw0 = reinterpret_cast<const uint32_t*>(p.cmds + c0);
    const uint32_t f0 = scalar_load(cw0), f1 = scalar_load(cw0 + 1), f2 = scalar_load(cw0 + 2);
    uint32_t count = *p.count;
    const ChordDrawCmd* cmds = p.cmds;
    bool firstValid = true;
    if (launch_is_dense(p, count)) { count = *p.leftCount; cmds = p.leftCmds; firstValid = false; }
    count = __builtin_amdgcn_readfirstlane(count);
    // A list longer than a light pass's (the host chose this kernel from a report of a frame long past: a camera cut, or a path that
    // crosses the light / heavy edge) is set up one wave per cluster, as raster_setup_kernel does -- a workgroup per cluster, four or
    // five barriers each, is the slower form once the list fills the device.  (The wave's first command is then read in the body.)
    if (count > p.wideMax) {
        raster_setup_body<MASKED>(p, cmds, count, sVert, sClipW[wave], 0u, 0u, 0u, false);
        return;
    }
    if (blockIdx.x >= count) return;

    auto load_header = [&](uint32_t i) -> SetupHeader {
        const ChordDrawCmd cmd = load_command(cmds, count, i);
        return load_setup_header(p.meshlets, p.objStatic, cmd.objectId, cmd.meshletId, cmd.slot);
    };
    float* lX = sV[0]; float* lY = sV[1]; float* lW = sV[2]; float* lU = sV[3]; float* lV = sV[4]; float* lD = sV[5];
    const LargeLds LL = {{sV[6], sV[7], sV[8], sV[9], sV[10]}};
    const uint32_t listShard = blockIdx.x % CHORD_LIST_SHARDS;
    const uint32_t t = wave * 32u + lane;                                        // this thread's triangle (lanes 0..31 of each wave)
    SetupHeader hdr = firstValid ? load_setup_header(p.meshlets, p.objStatic, f0, f1, f2) : load_header(blockIdx.x);
    if (tid == 0u) sClip[0] = 0u;
    for (uint32_t c = blockIdx.x; c < count; c += gridDim.x) {
        // the next cluster's header is on its way while this one is processed
        const SetupHeader hdrN = load_header(c + gridDim.x);
        const uint32_t V = hdr.V, T = min(hdr.T, 128u), dataOffset = hdr.dataOffset, vertexBase = hdr.vertexBase;
        const bool twoSided = (hdr.matFlags & CHORD_MATFLAG_TWO_SIDED) != 0u || p.depthOnly != 0u;
        const bool masked = MASKED && CHORD_MATFLAG_ALPHA(hdr.matFlags) == CHORD_ALPHA_MASK;
        const uint32_t* __restrict__ md = p.meshletData;
        const bool hasTri = lane < 32u && t < T;
        const uint32_t triWord = hasTri ? md[dataOffset + V + t] : 0u;
        // (not load_mvp: through the helper the compiler commutes and reorders nine instructions of this kernel's vertex transform;
        // the loop is left as it was so that the kernel stays the program that was measured)
        Mat4 mvp;
        {
            const float* __restrict__ mv = p.objFrame[hdr.objectId].mvp;
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int cc = 0; cc < 4; cc++) mvp.r[r][cc] = scalar_load(mv + r * 4 + cc);
        }
        // (the table of the cluster before was last read ahead of the barrier that ended its iteration)
        for (uint32_t h = tid; h < WIDE_HASH; h += 256u) { sKey[h] = WIDE_EMPTY; sCnt[h] = 0u; }
        // ---- vertex phase: one vertex per thread ----------------------------------------------------------------------------
        if (tid < V) {
            const float* __restrict__ pp = p.positions + (size_t)((md[dataOffset + tid] + vertexBase) * 3u);
            const f4 h = mul_mv(mvp, pp[0], pp[1], pp[2], 1.0f);
            const float aw = fabsf(h.w);
            lX[tid] = h.x; lY[tid] = h.y; lW[tid] = h.w;
            lU[tid] = h.x / aw * 0.5f + 0.5f;
            lV[tid] = h.y / aw * -0.5f + 0.5f;
            const bool fast = p.depthClamp ? in_fast_volume_xy(h) : in_fast_volume(h);
            lD[tid] = fast ? h.z / h.w : __builtin_nanf("");
        }
        float uv[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (MASKED && masked && hasTri && p.texcoords != nullptr) {
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const size_t vi = (size_t)(md[dataOffset + ((triWord >> (8 * i)) & 0xFFu)] + vertexBase) * 2;
                uv[2 * i] = p.texcoords[vi]; uv[2 * i + 1] = p.texcoords[vi + 1];
            }
        }
        __syncthreads();
        // ---- triangle phase: one triangle per lane, the culls and set-up of raster_setup_body ---------------------------------
        int kind = K_NONE;
        TriSetup ts;
        ts.px0 = ts.py0 = ts.px1 = ts.py1 = 0;
        float d[3] = {0.0f, 0.0f, 0.0f};
        if (hasTri) {
            const uint32_t i0 = triWord & 0xFFu, i1 = (triWord >> 8) & 0xFFu, i2 = (triWord >> 16) & 0xFFu;
            const float x0 = lX[i0], y0 = lY[i0], w0 = lW[i0];
            const float x1 = lX[i1], y1 = lY[i1], w1 = lW[i1];
            const float x2 = lX[i2], y2 = lY[i2], w2 = lW[i2];
            bool culled = false;
            if (!twoSided) {
                const float det = (x0 * (y1 * w2 - w1 * y2) - y0 * (x1 * w2 - w1 * x2)) + w0 * (x1 * y2 - y1 * x2);
                culled = det <= 0.0f;
            }
            culled = culled || (w0 <= 0.0f && w1 <= 0.0f && w2 <= 0.0f);
            const float u0 = lU[i0], v0 = lV[i0], u1 = lU[i1], v1 = lV[i1], u2 = lU[i2], v2 = lV[i2];
            const float maxU = fmaxf(u0, fmaxf(u1, u2)), maxV = fmaxf(v0, fmaxf(v1, v2));
            const float minU = fminf(u0, fminf(u1, u2)), minV = fminf(v0, fminf(v1, v2));
            culled = culled || ((minU >= 1.0f || minV >= 1.0f) || (maxU <= 0.0f || maxV <= 0.0f));
            culled = culled || (rintf(minU * p.W) == rintf(maxU * p.W) || rintf(minV * p.H) == rintf(maxV * p.H));
            if (!culled) {
                d[0] = lD[i0]; d[1] = lD[i1]; d[2] = lD[i2];
                ts.payload = p.depthOnly ? 0u : encode_triangle_instance(t, hdr.slot);
                if (d[0] != d[0] || d[1] != d[1] || d[2] != d[2]) {          // (NaN: a vertex outside the fast volume)
                    kind = K_CLIP;
                } else {
                    ts.X[0] = snap(u0, p.W); ts.Y[0] = snap(v0, p.H);
                    ts.X[1] = snap(u1, p.W); ts.Y[1] = snap(v1, p.H);
                    ts.X[2] = snap(u2, p.W); ts.Y[2] = snap(v2, p.H);
                    if (tri_setup(ts, twoSided, p.Wi, p.Hi) && owns_rect(p.shard, ts.px0, ts.py0, ts.px1, ts.py1)) {
                        kind = K_EMIT;
                        if (p.biasConst != 0.0f || p.biasSlope != 0.0f) { const float o = depth_bias(ts, d, p.biasConst, p.biasSlope); d[0] += o; d[1] += o; d[2] += o; }
                    }
                }
            }
        }
        if (ABL(p, DBG_NO_BIN)) kind = K_NONE;
        const unsigned long long lt = (1ull << lane) - 1ull;
        const bool cp = kind == K_EMIT && !masked && fits_compact(ts);
        const bool lg = kind == K_EMIT && touches_many_tiles(ts);
        const unsigned long long cm = __ballot(kind == K_CLIP), ec = __ballot(cp), ew = __ballot(kind == K_EMIT && !cp), lm = __ballot(lg);
        if (lane == 0u) {
            sWave[wave][0] = (uint32_t)__popcll(cm); sWave[wave][1] = (uint32_t)__popcll(ec);
            sWave[wave][2] = (uint32_t)__popcll(ew); sWave[wave][3] = (uint32_t)__popcll(lm);
        }
        // primary tiles (records of at most 2x2 tiles) into the table: the LDS atomic's return is the record's rank in the tile
        uint32_t tileR[4], hR[4], rankR[4], has = 0u;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int32_t tx0 = ts.px0 >> TILE_SHIFT, tx1 = ts.px1 >> TILE_SHIFT, ty0 = ts.py0 >> TILE_SHIFT, ty1 = ts.py1 >> TILE_SHIFT;
            const int32_t tx = (r & 1) ? tx1 : tx0, ty = (r & 2) ? ty1 : ty0;
            bool in = kind == K_EMIT && !lg && !((r & 1) && tx1 == tx0) && !((r & 2) && ty1 == ty0);
            if (in) in = owns_tile(p.shard, tx, ty);
            tileR[r] = in ? __umul24((uint32_t)ty, p.tilesX) + (uint32_t)tx : 0u;
            hR[r] = 0u; rankR[r] = 0u;
            if (in) {
                has |= 1u << r;
                uint32_t h = tileR[r] & (WIDE_HASH - 1u);
                for (;;) {
                    const uint32_t o = atomicCAS(&sKey[h], WIDE_EMPTY, tileR[r]);
                    if (o == WIDE_EMPTY || o == tileR[r]) break;
                    h = (h + 1u) & (WIDE_HASH - 1u);
                }
                hR[r] = h;
                rankR[r] = atomicAdd(&sCnt[h], 1u);
            }
        }
        __syncthreads();
        // ---- reservations: every list and bin atomic of the cluster in one round trip -------------------------------------
        const uint32_t nClip = sWave[0][0] + sWave[1][0] + sWave[2][0] + sWave[3][0];
        const uint32_t nLg = sWave[0][3] + sWave[1][3] + sWave[2][3] + sWave[3][3];
        {
            uint32_t n[4], key[4], base[4];
#pragma unroll
            for (int i = 0; i < 4; i++) { n[i] = sCnt[tid + 256u * i]; key[i] = sKey[tid + 256u * i]; }
            uint32_t cbase = 0u, ebaseC = 0u, ebaseW = 0u;
            if (tid == 0u) {
                const uint32_t nEc = sWave[0][1] + sWave[1][1] + sWave[2][1] + sWave[3][1];
                const uint32_t nEw = sWave[0][2] + sWave[1][2] + sWave[2][2] + sWave[3][2];
                if (nClip) cbase = atomicAdd(&p.counters->clipTriCount[p.pass], nClip);
                if (nEc) ebaseC = atomicAdd(&p.counters->triCountC[listShard * CHORD_SHARD_STRIDE], nEc);
                if (nEw) ebaseW = atomicAdd(&p.counters->triCount[listShard * CHORD_SHARD_STRIDE], nEw * (masked ? 1u + CHORD_MASK_EXT_SLOTS : 1u));
                if (nLg) atomicAdd(&p.counters->largeCount[p.pass][listShard * CHORD_SHARD_STRIDE], nLg);
            }
#pragma unroll
            for (int i = 0; i < 4; i++) base[i] = n[i] ? atomicAdd(&p.tileCount[(size_t)key[i] * TC_STRIDE], n[i]) : 0u;
            if (MASKED && masked) {
#pragma unroll
                for (int i = 0; i < 4; i++) if (n[i]) p.tileCount[(size_t)key[i] * TC_STRIDE + TC_MASKED] = 1u;
            }
#pragma unroll
            for (int i = 0; i < 4; i++) if (n[i]) sCnt[tid + 256u * i] = base[i];
            if (tid == 0u) {
                sBase[0] = cbase; sBase[1] = ebaseC; sBase[2] = ebaseW;
                // (the clip triangles are clipped once the workgroup's clusters are done: their ranges of the clip list wait in LDS)
                if (nClip) {
                    const uint32_t r = sClip[0];
                    if (r < CLIP_RANGES) { sClip[1u + r] = cbase | (nClip - 1u) << 25; sClip[0] = r + 1u; } else atomicOr(&p.counters->overflow, 2u);
                }
            }
        }
        __syncthreads();
        // ---- emission: records, clip list entries, bin entries -------------------------------------------------------------
        {
            uint32_t offClip = 0u, offC = 0u, offW = 0u;
            for (uint32_t w = 0; w < wave; w++) { offClip += sWave[w][0]; offC += sWave[w][1]; offW += sWave[w][2]; }
            const uint32_t wSlots = masked ? 1u + CHORD_MASK_EXT_SLOTS : 1u;
            uint32_t slotR[4];
#pragma unroll
            for (int r = 0; r < 4; r++) slotR[r] = (has & (1u << r)) ? sCnt[hR[r]] + rankR[r] : 0u;
            if (kind == K_CLIP) {
                const uint32_t k = sBase[0] + offClip + (uint32_t)__popcll(cm & lt);
                if (k < p.clipTriCap) { ClipTri ct; ct.objectId = hdr.objectId; ct.meshletId = hdr.meshletId; ct.slot = hdr.slot; ct.tri = t; p.clipTris[k] = ct; }
                else atomicOr(&p.counters->overflow, 2u);
            }
            uint32_t gi = 0u;
            bool ok = false;
            if (cp) {
                const uint32_t li = sBase[1] + offC + (uint32_t)__popcll(ec & lt);
                if (li < p.triCapC) { gi = listShard * p.triCapC + li; write_record_c(&p.trisC[gi], ts, d); ok = true; }
                else atomicOr(&p.counters->overflow, 1u);
            } else if (kind == K_EMIT) {
                const uint32_t li = sBase[2] + wSlots * (offW + (uint32_t)__popcll(ew & lt));
                if (li + wSlots <= p.triCap) {
                    gi = listShard * p.triCap + li; write_record(&p.tris[gi], ts, d, twoSided, masked);
                    if (MASKED && masked) setup_emit_mask_ext(p, &p.tris[gi + 1u], triWord, uv, lW, CHORD_MATFLAG_MATERIAL(hdr.matFlags), ts.area);
                    gi |= (MASKED && masked) ? CHORD_REC_MASKED : CHORD_REC_WIDE; ok = true;
                } else atomicOr(&p.counters->overflow, 1u);
            }
            // every slot this thread drew is allocated for before its first store (bin_put's contract; a record that did not fit its
            // list still allocates: other threads may wait for the chunk)
#pragma unroll
            for (int r = 0; r < 4; r++) if (has & (1u << r)) bin_alloc(p, tileR[r], slotR[r]);
            if (ok) {
#pragma unroll
                for (int r = 0; r < 4; r++) if (has & (1u << r)) bin_put(p, tileR[r], slotR[r], gi);
            }
            // records of more than 2x2 tiles: into LDS for the round below, with their candidate tile counts
            if (nLg) {
                uint32_t nt = 0u;
                if (lg && ok) {
                    large_put(LL, t, ts);
                    LL.at(LG_GI, t) = gi;
                    nt = large_tiles(LL.at(LG_BX, t), LL.at(LG_BY, t));
                }
                if (lane < 32u) sIncl[t] = nt;
            }
        }
        if (nLg) {
            // ---- large records: the (record, candidate tile) pairs of the cluster dealt over the workgroup, 256 per round -------
            __syncthreads();
            if (wave == 0u) {
                const uint32_t a = sIncl[2u * lane], b = sIncl[2u * lane + 1u];
                uint32_t incl = a + b;
#pragma unroll
                for (int dd = 1; dd < 64; dd <<= 1) { const uint32_t nb = (uint32_t)__shfl_up((int)incl, dd, 64); if (lane >= (uint32_t)dd) incl += nb; }
                sIncl[2u * lane] = incl - b; sIncl[2u * lane + 1u] = incl;
            }
            __syncthreads();
            const uint32_t total = sIncl[127];
            for (uint32_t j = tid; j < total; j += 256u) {
                uint32_t k = 0u;                                                // the first record whose inclusive count exceeds j
#pragma unroll
                for (uint32_t st = 64u; st > 0u; st >>= 1) if (sIncl[k + st - 1u] <= j) k += st;
                const uint32_t tt = j - (k ? sIncl[k - 1u] : 0u);
                TriSetup lr;
#pragma unroll
                for (int i = 0; i < 3; i++) { lr.X[i] = (int32_t)LL.at(LG_X0 + i, k); lr.Y[i] = (int32_t)LL.at(LG_Y0 + i, k); }
                lr.s = (int32_t)LL.at(LG_S, k);
                const uint32_t bx = LL.at(LG_BX, k), by = LL.at(LG_BY, k), lgi = LL.at(LG_GI, k);
                lr.px0 = (int32_t)(bx & 0xFFFFu); lr.px1 = (int32_t)(bx >> 16); lr.py0 = (int32_t)(by & 0xFFFFu); lr.py1 = (int32_t)(by >> 16);
                const int32_t tx0 = lr.px0 >> TILE_SHIFT, ty0 = lr.py0 >> TILE_SHIFT;
                const uint32_t tw = (uint32_t)((lr.px1 >> TILE_SHIFT) - tx0 + 1);
                const int32_t tx = tx0 + (int32_t)(tt % tw), ty = ty0 + (int32_t)(tt / tw);
                // pixel rectangle of this tile clipped to the triangle's bbox; conservative edge test at its corners (bin_record_tiles)
                const int32_t rx0 = max(lr.px0, tx << TILE_SHIFT), rx1 = min(lr.px1, (tx << TILE_SHIFT) + TILE - 1);
                const int32_t ry0 = max(lr.py0, ty << TILE_SHIFT), ry1 = min(lr.py1, (ty << TILE_SHIFT) + TILE - 1);
                const int ea[3] = {1, 2, 0}, eb[3] = {2, 0, 1};
                bool hit = owns_tile(p.shard, tx, ty);
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    const int64_t dxe = (int64_t)(lr.X[eb[i]] - lr.X[ea[i]]), dye = (int64_t)(lr.Y[eb[i]] - lr.Y[ea[i]]);
                    const int64_t a = -(int64_t)lr.s * dye, b = (int64_t)lr.s * dxe;
                    const int64_t bias = (a > 0 || (a == 0 && b > 0)) ? 0 : -1;
                    const int64_t cx = (int64_t)(a > 0 ? rx1 : rx0) * 256 + 128, cy = (int64_t)(b > 0 ? ry1 : ry0) * 256 + 128;
                    hit = hit && !((int64_t)lr.s * (dxe * (cy - lr.Y[ea[i]]) - dye * (cx - lr.X[ea[i]])) + bias < 0);
                }
                if (!hit) continue;
                const uint32_t tile = (uint32_t)ty * p.tilesX + (uint32_t)tx;
                bin_store(p, tile, atomicAdd(&p.tileCount[(size_t)tile * TC_STRIDE], 1u), lgi);
                if ((lgi & 0xE0000000u) == CHORD_REC_MASKED) p.tileCount[(size_t)tile * TC_STRIDE + TC_MASKED] = 1u;
            }
        }
        // the LDS of this cluster is rewritten by the next one
        __syncthreads();
        hdr = hdrN;
    }
    // ---- the clip triangles of the workgroup's clusters: CLIP_SETUP_LANES per wave at a time, in the wave's three arrays of sV --
    __syncthreads();
    if (const uint32_t ranges = sClip[0]) {
        float* a = sV[3u * wave]; float* b = sV[3u * wave + 1u]; float* cc = sV[3u * wave + 2u];
        const ClipLds<CLIP_SETUP_LANES> L = {reinterpret_cast<float4*>(a), b, b + 2u * CLIP_MAXV * CLIP_SETUP_LANES,
                                             reinterpret_cast<int32_t*>(cc), reinterpret_cast<int32_t*>(cc) + CLIP_MAXV * CLIP_SETUP_LANES,
                                             cc + 2u * CLIP_MAXV * CLIP_SETUP_LANES, lane};
        for (uint32_t i = 0; i < ranges; i++) {
            const uint32_t w = sClip[1u + i], base = w & 0x1FFFFFFu, n = (w >> 25) + 1u;
            for (uint32_t k0 = 0; k0 < n; k0 += 4u * CLIP_SETUP_LANES) {
                const uint32_t k = k0 + wave * CLIP_SETUP_LANES + lane;
                if (lane < CLIP_SETUP_LANES && k < n && base + k < p.clipTriCap) clip_entry<MASKED>(p, L, p.clipTris[base + k], listShard);
            }
        }
    }
}

// HOT: the variant that draws bin slots ahead on hot tiles (above).  It costs the plain kernel's loop 3 % (registers: the loop
// is at its SGPR limit), so the host launches it only when the previous frames' longest bin says a hot tile exists
// (RasterParams::binHint, written by the tile order kernel) -- a choice of speed, both variants fill the same bins.
template <bool HOT>
__global__ __launch_bounds__(256, BLOCKS_MIN_WAVES) void raster_setup_blocks_kernel(RasterParams p)
{
    __shared__ float sVert[6][4][BLOCKS_LDS_VERTS];            // x, y, w, u, v, depth of a wave's cluster (12 KB)
    __shared__ int32_t sSnap[2][4][BLOCKS_LDS_VERTS];          // ... and its snapped 24.8 screen coordinates (4 KB)
    __shared__ unsigned long long sWin[4][WIN * WIN];          // a small cluster's pixel window (8 KB)
    __shared__ SlotCache sSlots[HOT ? 4 : 1];                  // bin slots drawn ahead on hot tiles (1.5 KB)
    const uint32_t count = *p.count;
    if (!launch_is_dense(p, count)) return;
    raster_setup_blocks_body<HOT>(p, count, sVert, sSnap, sWin, sSlots);
}

__device__ void raster_clip_part(const RasterParams& p, uint32_t block, uint32_t blocks)
{
    __shared__ float4 sPoly[2 * CLIP_MAXV * CLIP_THREADS];
    __shared__ float sPU[2 * CLIP_MAXV * CLIP_THREADS], sPV[2 * CLIP_MAXV * CLIP_THREADS];     // texture coordinates ride along (masked materials only)
    __shared__ int32_t sPX[CLIP_MAXV * CLIP_THREADS], sPY[CLIP_MAXV * CLIP_THREADS];
    __shared__ float sPD[CLIP_MAXV * CLIP_THREADS];
    if (threadIdx.x >= CLIP_THREADS) return;
    const ClipLds<CLIP_THREADS> L = {sPoly, sPU, sPV, sPX, sPY, sPD, threadIdx.x};
    const uint32_t n = min(p.counters->clipTriCount[p.pass], p.clipTriCap);
    const uint32_t listShard = block % CHORD_LIST_SHARDS;
    for (uint32_t k = block * CLIP_THREADS + threadIdx.x; k < n; k += blocks * CLIP_THREADS) {
        clip_entry<true>(p, L, p.clipTris[k], listShard);
    }
}

// ---- large triangles: one wave per record, one lane per candidate tile -------------------------
// One launch, two independent roles: the first CLIP_BLOCKS blocks run the clipper, the rest bin the large records.
#define CLIP_BLOCKS 64u
__device__ void raster_bin_large_part(const RasterParams& p, uint32_t block, uint32_t blocks)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // the list is cut into CHORD_LIST_SHARDS sub-lists (one reservation counter each: a single word sustains only
    // ~88 returning atomics per microsecond); a flat index is mapped to (shard, entry) through their prefix sums
    __shared__ uint32_t sStart[CHORD_LIST_SHARDS + 1];
    if (threadIdx.x < 64u) {
        const uint32_t cnt = min(p.counters->largeCount[p.pass][threadIdx.x * CHORD_SHARD_STRIDE], p.largeCap);
        uint32_t incl = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t nb = (uint32_t)__shfl_up((int)incl, d, 64); if (lane >= (uint32_t)d) incl += nb; }
        sStart[threadIdx.x + 1u] = incl;
        if (threadIdx.x == 0u) sStart[0] = 0u;
    }
    __syncthreads();
    const uint32_t n = sStart[CHORD_LIST_SHARDS];
    for (uint32_t k = block * 4u + wave; k < n; k += blocks * 4u) {
        uint32_t sh = 0;
#pragma unroll
        for (uint32_t st = 32u; st > 0u; st >>= 1) if (sStart[sh + st] <= k) sh += st;
        const uint32_t gi = __builtin_amdgcn_readfirstlane(p.largeList[(size_t)sh * p.largeCap + (k - sStart[sh])]);
        const TriRec* __restrict__ r = &p.tris[gi];
        TriSetup ts;
#pragma unroll
        for (int i = 0; i < 3; i++) { ts.X[i] = r->X[i]; ts.Y[i] = r->Y[i]; }
        ts.payload = 0;
        if (!tri_setup(ts, (r->twoSided & 1u) != 0, p.Wi, p.Hi)) continue;
        const bool maskedRec = (r->twoSided & 4u) != 0u;                 // (wave-uniform: one record per wave)
        const int ea[3] = {1, 2, 0}, eb[3] = {2, 0, 1};
        int64_t a[3], b[3], bias[3], dxe[3], dye[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            dxe[i] = (int64_t)(ts.X[eb[i]] - ts.X[ea[i]]); dye[i] = (int64_t)(ts.Y[eb[i]] - ts.Y[ea[i]]);
            a[i] = -(int64_t)ts.s * dye[i]; b[i] = (int64_t)ts.s * dxe[i];
            bias[i] = (a[i] > 0 || (a[i] == 0 && b[i] > 0)) ? 0 : -1;
        }
        const int32_t tx0 = ts.px0 >> TILE_SHIFT, tx1 = ts.px1 >> TILE_SHIFT;
        const int32_t ty0 = ts.py0 >> TILE_SHIFT, ty1 = ts.py1 >> TILE_SHIFT;
        const uint32_t tw = (uint32_t)(tx1 - tx0 + 1), nt = tw * (uint32_t)(ty1 - ty0 + 1);
        for (uint32_t tb = 0; tb < nt; tb += 64u) {
            const uint32_t t = tb + lane;
            if (t >= nt) continue;
            const int32_t tx = tx0 + (int32_t)(t % tw), ty = ty0 + (int32_t)(t / tw);
            // pixel rectangle of this tile clipped to the triangle's bbox; conservative edge test at its corners
            const int32_t rx0 = max(ts.px0, tx << TILE_SHIFT), rx1 = min(ts.px1, (tx << TILE_SHIFT) + TILE - 1);
            const int32_t ry0 = max(ts.py0, ty << TILE_SHIFT), ry1 = min(ts.py1, (ty << TILE_SHIFT) + TILE - 1);
            bool hit = owns_tile(p.shard, tx, ty);
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const int64_t cx = (int64_t)(a[i] > 0 ? rx1 : rx0) * 256 + 128, cy = (int64_t)(b[i] > 0 ? ry1 : ry0) * 256 + 128;
                const int64_t E = (int64_t)ts.s * (dxe[i] * (cy - ts.Y[ea[i]]) - dye[i] * (cx - ts.X[ea[i]]));
                hit = hit && !(E + bias[i] < 0);
            }
            if (hit) {
                const uint32_t tile = (uint32_t)ty * p.tilesX + (uint32_t)tx;
                const uint32_t slot = atomicAdd(&p.tileCount[(size_t)tile * TC_STRIDE], 1u);   // distinct tiles per lane
                bin_store(p, tile, slot, gi | (maskedRec ? CHORD_REC_MASKED : CHORD_REC_WIDE));   // (the large list holds 48-byte records)
                if (maskedRec) p.tileCount[(size_t)tile * TC_STRIDE + TC_MASKED] = 1u;
            }
        }
    }
}

__global__ __launch_bounds__(256) void raster_clip_and_bin_large_kernel(RasterParams p)
{
    if (blockIdx.x < CLIP_BLOCKS) raster_clip_part(p, blockIdx.x, CLIP_BLOCKS);
    else raster_bin_large_part(p, blockIdx.x - CLIP_BLOCKS, gridDim.x - CLIP_BLOCKS);
}

// ---- launches of the set-up stage ---------------------------------------------------------------
#ifndef SETUP_GRID_MULT
#define SETUP_GRID_MULT 1u
#endif
void launch_raster_setup(ChordCtx* c, const RasterParams& p, uint32_t capacity, bool masked, bool blocks, bool hot, bool wide)
{
    stamp(c, S_HZBCULL);      // closes whatever preceded the raster (HZB cull / list reset)
    if (blocks) {
        const uint32_t bb = std::max(1u, std::min((capacity + 3u) / 4u, (uint32_t)c->numCUs * BLOCKS_MIN_WAVES));
        if (hot) CHORD_LAUNCH(c, raster_setup_blocks_kernel<true>, dim3(bb), dim3(256), 0, c->stream, p);
        else     CHORD_LAUNCH(c, raster_setup_blocks_kernel<false>, dim3(bb), dim3(256), 0, c->stream, p);
    }
    if (wide) {
        // one wave of workgroups of the device
        const uint32_t wideBlocks = std::max(1u, std::min(std::max(capacity, 1u), (uint32_t)c->numCUs * SETUP_WIDE_WAVES));
        if (masked) CHORD_LAUNCH(c, raster_setup_wide_kernel<true>, dim3(wideBlocks), dim3(256), 0, c->stream, p);
        else        CHORD_LAUNCH(c, raster_setup_wide_kernel<false>, dim3(wideBlocks), dim3(256), 0, c->stream, p);
    } else {
        const uint32_t maxBlocks = (uint32_t)c->numCUs * SETUP_MIN_WAVES * SETUP_GRID_MULT;    // what is resident at SETUP_MIN_WAVES waves per SIMD
        const uint32_t recBlocks = std::max(1u, std::min((capacity + 3u) / 4u, maxBlocks));
        if (masked) CHORD_LAUNCH(c, raster_setup_kernel<true>, dim3(recBlocks), dim3(256), 0, c->stream, p);
        else        CHORD_LAUNCH(c, raster_setup_kernel<false>, dim3(recBlocks), dim3(256), 0, c->stream, p);
    }
    stamp(c, S_R_CLUSTER);
    if (!p.binInSetup) CHORD_LAUNCH(c, raster_clip_and_bin_large_kernel, dim3(CLIP_BLOCKS + (uint32_t)c->numCUs * 4u), dim3(256), 0, c->stream, p);
}

} // namespace chord
