// chordvis -- object records built on the device from resident f64 world transforms (chordvis_upload_world_transforms,
// chordvis_scatter_world_transforms, chordvis_build_objects), and the flattened (object, group) table built on the
// device for chordvis_set_object_list (group_refs_build_kernel, further down).
//
//   scatter_world_transforms_kernel   a lane per 16-byte vector of the given matrices (8 per matrix): consecutive lanes read consecutive
//                                     addresses of `matrices` and write 128 contiguous bytes of cur per matrix.  An index at or beyond
//                                     objectCount writes nothing.
//   build_objects_kernel              a workgroup of ONE wave per 64 objects.  The 64 x 128 bytes of cur and of prev are one contiguous
//                                     8 KB run each: lane t loads the 16-byte vectors t, t + 64, ... (consecutive lanes on consecutive
//                                     addresses) into LDS rows padded to 144 bytes, then owns object t of the block: it reads its two
//                                     rows back (ds_read_b128; sixteen consecutive lanes start on sixteen different 4-bank slots), does SceneNode::getObjectBasicData in the
//                                     host function's operation order, and leaves the 208 bytes in LDS; the wave then stores the block's
//                                     64 x 13 vectors, lane t the vectors t, t + 64, ..., skipping the id quad behind every record -- those
//                                     16 bytes are neither read nor written.  prev = cur goes out from the registers of the load phase.
//
// The arithmetic is chordvis_object_basic_data's (host_camera.cpp), bit for bit for finite inputs: the translation minus the camera in
// binary64, one conversion per element, inverse4<float> in its source order, no contraction (-ffp-contract=off), correctly rounded divide
// and square root (HIP's default), subnormals kept.  tests/test_gpu_object_build.py holds the kernel to the host function byte by byte.

#include "device_layer.h"

namespace chord {

namespace {

constexpr uint32_t kBuildObjects = 64u;     // objects per workgroup = lanes of its one wave
constexpr uint32_t kRowVectors = 9u;        // 8 vectors of a 4x4 f64 matrix + 1 of padding: 144-byte rows

struct BuildArgs {
    const double2* cur;
    double2* prev;
    float4* objects;        // ChordObject as 14 vectors: 13 of basicData, 1 of ids
    uint32_t* status;       // {singular count, first singular index} of this build
    uint32_t* clearNext;    // the words the NEXT build adds into
    double cam[3], camLast[3];
    uint32_t count;
};

// inverse4<float> of host_camera.cpp, statement for statement.  false: det == 0 (out untouched)
__device__ __forceinline__ bool inverse4_f32(const float* m, float* out)
{
    float inv[16];
    inv[0]  =  m[5]*m[10]*m[15] - m[5]*m[11]*m[14] - m[9]*m[6]*m[15] + m[9]*m[7]*m[14] + m[13]*m[6]*m[11] - m[13]*m[7]*m[10];
    inv[4]  = -m[4]*m[10]*m[15] + m[4]*m[11]*m[14] + m[8]*m[6]*m[15] - m[8]*m[7]*m[14] - m[12]*m[6]*m[11] + m[12]*m[7]*m[10];
    inv[8]  =  m[4]*m[9]*m[15]  - m[4]*m[11]*m[13] - m[8]*m[5]*m[15] + m[8]*m[7]*m[13] + m[12]*m[5]*m[11] - m[12]*m[7]*m[9];
    inv[12] = -m[4]*m[9]*m[14]  + m[4]*m[10]*m[13] + m[8]*m[5]*m[14] - m[8]*m[6]*m[13] - m[12]*m[5]*m[10] + m[12]*m[6]*m[9];
    inv[1]  = -m[1]*m[10]*m[15] + m[1]*m[11]*m[14] + m[9]*m[2]*m[15] - m[9]*m[3]*m[14] - m[13]*m[2]*m[11] + m[13]*m[3]*m[10];
    inv[5]  =  m[0]*m[10]*m[15] - m[0]*m[11]*m[14] - m[8]*m[2]*m[15] + m[8]*m[3]*m[14] + m[12]*m[2]*m[11] - m[12]*m[3]*m[10];
    inv[9]  = -m[0]*m[9]*m[15]  + m[0]*m[11]*m[13] + m[8]*m[1]*m[15] - m[8]*m[3]*m[13] - m[12]*m[1]*m[11] + m[12]*m[3]*m[9];
    inv[13] =  m[0]*m[9]*m[14]  - m[0]*m[10]*m[13] - m[8]*m[1]*m[14] + m[8]*m[2]*m[13] + m[12]*m[1]*m[10] - m[12]*m[2]*m[9];
    inv[2]  =  m[1]*m[6]*m[15]  - m[1]*m[7]*m[14]  - m[5]*m[2]*m[15] + m[5]*m[3]*m[14] + m[13]*m[2]*m[7]  - m[13]*m[3]*m[6];
    inv[6]  = -m[0]*m[6]*m[15]  + m[0]*m[7]*m[14]  + m[4]*m[2]*m[15] - m[4]*m[3]*m[14] - m[12]*m[2]*m[7]  + m[12]*m[3]*m[6];
    inv[10] =  m[0]*m[5]*m[15]  - m[0]*m[7]*m[13]  - m[4]*m[1]*m[15] + m[4]*m[3]*m[13] + m[12]*m[1]*m[7]  - m[12]*m[3]*m[5];
    inv[14] = -m[0]*m[5]*m[14]  + m[0]*m[6]*m[13]  + m[4]*m[1]*m[14] - m[4]*m[2]*m[13] - m[12]*m[1]*m[6]  + m[12]*m[2]*m[5];
    inv[3]  = -m[1]*m[6]*m[11]  + m[1]*m[7]*m[10]  + m[5]*m[2]*m[11] - m[5]*m[3]*m[10] - m[9]*m[2]*m[7]   + m[9]*m[3]*m[6];
    inv[7]  =  m[0]*m[6]*m[11]  - m[0]*m[7]*m[10]  - m[4]*m[2]*m[11] + m[4]*m[3]*m[10] + m[8]*m[2]*m[7]   - m[8]*m[3]*m[6];
    inv[11] = -m[0]*m[5]*m[11]  + m[0]*m[7]*m[9]   + m[4]*m[1]*m[11] - m[4]*m[3]*m[9]  - m[8]*m[1]*m[7]   + m[8]*m[3]*m[5];
    inv[15] =  m[0]*m[5]*m[10]  - m[0]*m[6]*m[9]   - m[4]*m[1]*m[10] + m[4]*m[2]*m[9]  + m[8]*m[1]*m[6]   - m[8]*m[2]*m[5];
    const float det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
    if (det == 0.0f) return false;
    const float inv_det = 1.0f / det;
#pragma unroll
    for (int i = 0; i < 16; i++) out[i] = inv[i] * inv_det;
    return true;
}

// one LDS row (a 4x4 f64 matrix) -> the camera-relative f32 matrix: scene_node.cpp:51-55 / :80-84
__device__ __forceinline__ void relative_f32(const double2* row, const double cam[3], float* L)
{
    double m[16];
#pragma unroll
    for (int q = 0; q < 8; q++) { const double2 v = row[q]; m[2 * q] = v.x; m[2 * q + 1] = v.y; }
    m[12] -= cam[0]; m[13] -= cam[1]; m[14] -= cam[2];
#pragma unroll
    for (int i = 0; i < 16; i++) L[i] = (float)m[i];
}

} // namespace

__global__ __launch_bounds__(256) void scatter_world_transforms_kernel(const uint32_t* __restrict__ indices, const double2* __restrict__ matrices,
                                                                       double2* __restrict__ cur, uint32_t n, uint32_t count)
{
    const uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t k = v >> 3;
    if (k >= n) return;
    const uint32_t o = indices[k];
    if (o >= count) return;
    cur[(uint64_t)o * 8u + (v & 7u)] = matrices[v];
}

__global__ __launch_bounds__(64) void build_objects_kernel(const BuildArgs a)
{
    __shared__ double2 sIn[2][kBuildObjects][kRowVectors];
    __shared__ float4 sOut[kBuildObjects][13];
    const uint32_t t = threadIdx.x, base = blockIdx.x * kBuildObjects;
    const uint32_t here = a.count - base < kBuildObjects ? a.count - base : kBuildObjects;     // objects of this block
    const uint64_t in0 = (uint64_t)base * 8u;

    if (blockIdx.x == 0 && t == 0) { a.clearNext[0] = 0u; a.clearNext[1] = 0xFFFFFFFFu; }

    double2 c[8], p[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {                 // (all sixteen loads are issued before the first LDS write waits for one)
        const uint32_t v = t + 64u * k;
        const bool in = (v >> 3) < here;
        c[k] = in ? a.cur[in0 + v] : make_double2(0.0, 0.0);
        p[k] = in ? a.prev[in0 + v] : make_double2(0.0, 0.0);
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t v = t + 64u * k;
        if ((v >> 3) < here) { sIn[0][v >> 3][v & 7u] = c[k]; sIn[1][v >> 3][v & 7u] = p[k]; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; k++) {                 // prev = cur (this lane read these very vectors of prev above)
        const uint32_t v = t + 64u * k;
        if ((v >> 3) < here) a.prev[in0 + v] = c[k];
    }

    if (t < here) {
        float L[16], P[16], I[16], s[4];
        relative_f32(sIn[0][t], a.cam, L);
        relative_f32(sIn[1][t], a.camLast, P);
        if (inverse4_f32(L, I)) {
            // (Finite inputs can still end in a NaN here: a determinant in the subnormal range has 1 / det = inf, and inf times the
            // zeros of an affine inverse's last row is invalid.  This hardware makes 0xFFC00000 for an invalid multiply or add, the
            // pattern an x86 host makes, so those bytes equal the host function's too: the 2^-45 object of the tests' input set.)
            s[0] = sqrtf(L[0] * L[0] + L[1] * L[1] + L[2] * L[2]);             // scene_node.cpp:60-64
            s[1] = sqrtf(L[4] * L[4] + L[5] * L[5] + L[6] * L[6]);
            s[2] = sqrtf(L[8] * L[8] + L[9] * L[9] + L[10] * L[10]);
            s[3] = fmaxf(fmaxf(fabsf(s[0]), fabsf(s[1])), fabsf(s[2]));
        } else {
            // the host function returns here with the inverse and the scale still zero
#pragma unroll
            for (int i = 0; i < 16; i++) I[i] = 0.0f;
            s[0] = s[1] = s[2] = s[3] = 0.0f;
            atomicAdd(&a.status[0], 1u);
            atomicMin(&a.status[1], base + t);
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            sOut[t][q] = make_float4(L[4 * q], L[4 * q + 1], L[4 * q + 2], L[4 * q + 3]);
            sOut[t][4 + q] = make_float4(I[4 * q], I[4 * q + 1], I[4 * q + 2], I[4 * q + 3]);
            sOut[t][8 + q] = make_float4(P[4 * q], P[4 * q + 1], P[4 * q + 2], P[4 * q + 3]);
        }
        sOut[t][12] = make_float4(s[0], s[1], s[2], s[3]);
    }
    __syncthreads();

    const float4* flat = &sOut[0][0];
#pragma unroll
    for (int k = 0; k < 13; k++) {
        const uint32_t v = t + 64u * k, o = v / 13u;
        if (o < here) a.objects[(uint64_t)(base + o) * 14u + (v - o * 13u)] = flat[v];
    }
}

// ---- the flattened (object, group) table of chordvis_set_object_list ----
//
//   group_refs_build_kernel   a lane per group instance i.  Its owner is the last object whose groupBase is <= i (objects of no groups
//                             share their successor's base and own nothing): a bisection over DObjStatic::groupBase, whose probes are
//                             the same few lines for every lane of a wave.  Then the walk chordvis_upload_scene does on the host --
//                             object -> primitive -> group -> group indices -- and the 24-byte record as three 8-byte stores: a wave
//                             writes 1536 contiguous bytes in three instructions, every byte of every line it touches.  The work per
//                             lane is the same whatever the objects' sizes; a grid-stride loop takes lists longer than the grid.
//                             (A form that gathered a workgroup's records in LDS and stored them as 16-byte vectors took the same
//                             time -- the kernel waits for its chain of dependent loads, not for its stores -- and was dropped.)
constexpr uint32_t kRefsThreads = 256u;

__global__ __launch_bounds__(kRefsThreads) void group_refs_build_kernel(const DObjStatic* __restrict__ objStatic, const DPrim* __restrict__ prims,
                                                                         const DGroup* __restrict__ groups, const uint32_t* __restrict__ groupIndices,
                                                                         DGroupRef* __restrict__ refs, uint32_t objectCount, uint32_t groupInstances)
{
    // (groupInstances <= 2^31 - 1 and the grid is at most 2^19 lanes: neither i nor the stride wraps)
    for (uint32_t i = blockIdx.x * kRefsThreads + threadIdx.x; i < groupInstances; i += gridDim.x * kRefsThreads) {
        uint32_t lo = 0u, hi = objectCount;                   // the first object whose groupBase is > i, in [lo, hi]
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (objStatic[mid].groupBase <= i) lo = mid + 1u; else hi = mid;
        }
        const uint32_t o = lo - 1u;                           // (object 0's base is 0 <= i: lo >= 1)
        const DObjStatic& d = objStatic[o];
        const DPrim& pr = prims[d.prim];
        const uint32_t g = pr.groupBase + (i - d.groupBase);
        const uint32_t meshletOffset = groups[g].meshletOffset, meshletCount = groups[g].meshletCount;
        const uint32_t cnt = meshletCount < (uint32_t)CHORD_GROUP_MAX_MESHLETS ? meshletCount : (uint32_t)CHORD_GROUP_MAX_MESHLETS;
        uint32_t m[CHORD_GROUP_MAX_MESHLETS];
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)CHORD_GROUP_MAX_MESHLETS; k++)
            m[k] = cnt ? pr.meshletBase + groupIndices[pr.groupIndicesBase + meshletOffset + (k < cnt ? k : 0u)] : 0u;
        uint2* out = reinterpret_cast<uint2*>(refs + i);
        out[0] = make_uint2(o, g | (cnt << 28)); out[1] = make_uint2(m[0], m[1]); out[2] = make_uint2(m[2], m[3]);
    }
}

void launch_group_refs_build(ChordCtx* c)
{
    if (c->groupInstances == 0u) return;
    const uint32_t blocks = (c->groupInstances + kRefsThreads - 1u) / kRefsThreads;
    const uint32_t grid = blocks < (uint32_t)c->numCUs * 8u ? blocks : (uint32_t)c->numCUs * 8u;
    CHORD_LAUNCH(c, group_refs_build_kernel, dim3(grid), dim3(kRefsThreads), 0, c->stream, c->dObjStatic, c->dPrims, c->dGroups, c->dGroupIndices,
                 c->dGroupRefs, c->objectCount, c->groupInstances);
}

void launch_scatter_world_transforms(ChordCtx* c, const uint32_t* indices, const double* matrices, uint32_t n)
{
    const uint64_t vectors = (uint64_t)n * 8u;
    CHORD_LAUNCH(c, scatter_world_transforms_kernel, dim3((uint32_t)((vectors + 255u) / 256u)), dim3(256), 0, c->stream, indices,
                 reinterpret_cast<const double2*>(matrices), reinterpret_cast<double2*>(c->dWorldCur), n, c->objectCount);
}

void launch_build_objects(ChordCtx* c, const double cameraPos[3], const double cameraPosLast[3], uint32_t* status, uint32_t* clearNext)
{
    BuildArgs a;
    a.cur = reinterpret_cast<const double2*>(c->dWorldCur); a.prev = reinterpret_cast<double2*>(c->dWorldPrev);
    a.objects = reinterpret_cast<float4*>(c->dObjectsOwned);
    a.status = status; a.clearNext = clearNext;
    for (int i = 0; i < 3; i++) { a.cam[i] = cameraPos[i]; a.camLast[i] = cameraPosLast[i]; }
    a.count = c->objectCount;
    CHORD_LAUNCH(c, build_objects_kernel, dim3((c->objectCount + kBuildObjects - 1u) / kBuildObjects), dim3(kBuildObjects), 0, c->stream, a);
}

} // namespace chord
