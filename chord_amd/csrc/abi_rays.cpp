// C ABI, ray queries on the resident scene (include/chordvis.h RAY QUERIES; ray_scene.cpp; kernels_rays.hip): the BLASes
// and the TLAS built on the host and uploaded, the refit, and the launches that trace rays and shade their hits.

#include "host_layer.h"

using namespace chord;

namespace chord {

// The ray scene (chordvis_build_ray_scene).  The TLAS belongs to an object list: chordvis_set_object_list parks its buffers without
// waiting; the BLASes belong to a scene upload, which has let the stream run empty before it frees them.
void drop_ray_tlas(ChordCtx* c, bool park)
{
    // (a rebuilt TLAS lives in the rebuild's own buffers, which stay for the next rebuild: abi_raytlas.cpp)
    if (c->rayTlasRebuilt) { c->dRayTlas = nullptr; c->dRayLeafRef = nullptr; c->dRayCounters = nullptr; c->dRayLeafBox = nullptr; c->dRayRoot = nullptr; c->rayTlasRebuilt = false; }
    if (park) { retire(c, c->dRayTlas); retire(c, c->dRayLeafRef); retire(c, c->dRayCounters); retire(c, c->dRayLeafBox); retire(c, c->dRayRoot); }
    else { dfree(c->dRayTlas); dfree(c->dRayLeafRef); dfree(c->dRayCounters); dfree(c->dRayLeafBox); dfree(c->dRayRoot); }
    c->rayTlasBuilt = false; c->rayRefitDue = false; c->rayTlasNodes = c->rayTlasDepth = 0; c->rayTlasBytes = 0;
}

void drop_ray_scene(ChordCtx* c)          // (the caller has let the stream run empty)
{
    drop_ray_tlas(c, false);
    drop_ray_rebuild_buffers(c);
    dfree(c->dRayBlas); dfree(c->dRayTriangles); dfree(c->dRayBlasRoot); dfree(c->dRayCounts);
    c->rayBlasBuilt = false; c->rayBlasNodes = c->rayBlasTriangles = c->rayBlasDepth = 0; c->rayBlasBytes = 0;
}

} // namespace chord

namespace {

int ray_checks(ChordCtx* c, const char* fn, bool needTlas)
{
    if (c->sharedScene) return refuse(c, CHORDVIS_E_INVALID, fn, "not on a depth-view context");
    if (!c->sceneLoaded) return refuse(c, CHORDVIS_E_INVALID, fn, "no scene (call chordvis_upload_scene first)");
    if (needTlas && !(c->rayBlasBuilt && c->rayTlasBuilt))
        return refuse(c, CHORDVIS_E_INVALID, fn, "no ray scene, or it was dropped by chordvis_upload_scene / chordvis_set_object_list (call chordvis_build_ray_scene, or chordvis_rebuild_ray_tlas)");
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

extern "C" {

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

    DeviceTemp<ray::Node> fBlas, fTlas;
    DeviceTemp<ray::Triangle> fTris;
    DeviceTemp<uint32_t> fRoots, fLeafRef, fCounters;
    DeviceTemp<float> fLeafBox, fRoot;
    uint64_t blasBytes = 0, tlasBytes = 0;
    int rc = CHORDVIS_OK;
    if (buildBlas) {
        if (!rc) rc = ray_upload(c, fBlas.p, blas.nodes.data(), blas.nodes.size(), blasBytes);
        if (!rc) rc = ray_upload(c, fTris.p, blas.triangles.data(), blas.triangles.size(), blasBytes);
        if (!rc) rc = ray_upload(c, fRoots.p, blas.roots.data(), blas.roots.size(), blasBytes);
    }
    if (!rc) rc = ray_upload(c, fTlas.p, tlas.nodes.data(), tlas.nodes.size(), tlasBytes);
    if (!rc) rc = ray_upload(c, fLeafRef.p, tlas.leafRef.data(), tlas.leafRef.size(), tlasBytes);
    if (!rc) rc = ray_upload(c, fCounters.p, nullptr, tlas.nodes.size(), tlasBytes);
    if (!rc) rc = ray_upload(c, fLeafBox.p, nullptr, (size_t)c->objectCount * 8u, tlasBytes);
    if (!rc) rc = ray_upload(c, fRoot.p, nullptr, 8u, tlasBytes);
    if (rc) return rc;

    // commit (the stream is empty: nothing reads the old buffers)
    if (buildBlas) {
        dfree(c->dRayBlas); dfree(c->dRayTriangles); dfree(c->dRayBlasRoot);
        c->dRayBlas = fBlas.release(); c->dRayTriangles = fTris.release(); c->dRayBlasRoot = fRoots.release();
        c->rayBlasNodes = (uint32_t)blas.nodes.size(); c->rayBlasTriangles = (uint32_t)blas.triangles.size(); c->rayBlasDepth = blas.depth;
        c->rayBlasBytes = blasBytes; c->rayBlasBuilt = true;
    }
    drop_ray_tlas(c, false);
    c->dRayTlas = fTlas.release(); c->dRayLeafRef = fLeafRef.release(); c->dRayCounters = fCounters.release(); c->dRayLeafBox = fLeafBox.release(); c->dRayRoot = fRoot.release();
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

} // extern "C"
