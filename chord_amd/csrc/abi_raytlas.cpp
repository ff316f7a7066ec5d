// C ABI, the ray scene's TLAS rebuilt on the device and read back (include/chordvis.h RAY QUERIES, "rebuilding the TLAS";
// ray_tlas_shape.h; kernels_raytlas.hip).  The shape of the tree follows from the object count, so everything the
// host decides -- node count, buffer sizes, launches -- it decides without reading the device.

#include "host_layer.h"
#include "ray_tlas_shape.h"

using namespace chord;

static_assert(sizeof(ChordRayNode) == sizeof(ray::Node), "ChordRayNode mirrors ray::Node");
static_assert(CHORD_RAY_TLAS_NODE == ray::kTlasNode && CHORD_RAY_TLAS_LEAF == ray::kTlasLeaf && CHORD_RAY_NO_CHILD == ray::kNoChild, "child words");

namespace chord {

void drop_ray_rebuild_buffers(ChordCtx* c)
{
    dfree(c->dRayRebuildNodes); dfree(c->dRayRebuildLeafRef); dfree(c->dRayRebuildCounters); dfree(c->dRayRebuildLeafBox);
    dfree(c->dRayRebuildRoot); dfree(c->dRayRebuildScratch);
    c->rayRebuildCapacity = 0; c->rayRebuildBytes = 0;
}

} // namespace chord

namespace {

// Buffers for `cap` objects: every new one first, then the old ones are parked (a launch in flight may still read them; whichever call
// waits next frees them).  A refusal leaves what was there.
int grow_rebuild_buffers(ChordCtx* c, uint64_t cap)
{
    const uint64_t nodes = ray::tlas_node_count(cap);
    const ray::TlasScratch lay = ray::tlas_scratch(cap);
    DeviceTemp<ray::Node> fNodes;
    DeviceTemp<uint32_t> fLeafRef, fCounters, fScratch;
    DeviceTemp<float> fLeafBox, fRoot;
    uint64_t bytes = 0;
    auto make = [&](auto& t, uint64_t count) -> int {
        const size_t n = (size_t)count * sizeof(*t.p);
        const hipError_t e = hipMalloc((void**)&t.p, n);
        if (e != hipSuccess) { t.p = nullptr; return fail(c, CHORDVIS_E_HIP, "rebuild_ray_tlas: hipMalloc of a buffer the longer list needs", e); }
        bytes += n;
        return CHORDVIS_OK;
    };
    int rc;
    if ((rc = make(fNodes, nodes)) || (rc = make(fLeafRef, cap)) || (rc = make(fCounters, nodes)) || (rc = make(fLeafBox, cap * 8u)) ||
        (rc = make(fRoot, 8u)) || (rc = make(fScratch, lay.words))) return rc;
    // the bounds words as every rebuild leaves them (ray_tlas_nodes_kernel): minima at the top of the order, maxima at the bottom
    const uint32_t cleared[8] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u, 0u, 0u};
    CHORD_HIP(c, hipMemcpy(fScratch.p + lay.bounds, cleared, sizeof(cleared), hipMemcpyHostToDevice));
    CHORD_HIP(c, hipMemset(fRoot.p, 0, 8u * sizeof(float)));

    if (c->rayTlasRebuilt) drop_ray_tlas(c, true);        // (it lives in the buffers that go: unlinked, and no TLAS until the commit)
    retire(c, c->dRayRebuildNodes); retire(c, c->dRayRebuildLeafRef); retire(c, c->dRayRebuildCounters); retire(c, c->dRayRebuildLeafBox);
    retire(c, c->dRayRebuildRoot); retire(c, c->dRayRebuildScratch);
    c->dRayRebuildNodes = fNodes.release(); c->dRayRebuildLeafRef = fLeafRef.release(); c->dRayRebuildCounters = fCounters.release();
    c->dRayRebuildLeafBox = fLeafBox.release(); c->dRayRebuildRoot = fRoot.release(); c->dRayRebuildScratch = fScratch.release();
    c->rayRebuildCapacity = cap; c->rayRebuildBytes = bytes;
    return CHORDVIS_OK;
}

} // namespace

extern "C" {

// Refusals first, then the buffers (only a list longer than every earlier one allocates), then the commit and the launches.
int chordvis_rebuild_ray_tlas(ChordCtx* c)
{
    if (!c) return CHORDVIS_E_INVALID;
    if (c->sharedScene) return refuse(c, CHORDVIS_E_INVALID, "rebuild_ray_tlas", "not on a depth-view context");
    if (!c->sceneLoaded) return refuse(c, CHORDVIS_E_INVALID, "rebuild_ray_tlas", "no scene (call chordvis_upload_scene first)");
    if (!c->rayBlasBuilt)
        return refuse(c, CHORDVIS_E_INVALID, "rebuild_ray_tlas", "no BLASes since the last chordvis_upload_scene (call chordvis_build_ray_scene once first)");
    ray::TlasShape shape;
    if (ray::tlas_shape(c->objectCount, shape))
        return refuse(c, CHORDVIS_E_CAPACITY, "rebuild_ray_tlas", "the TLAS is deeper than CHORD_RAY_MAX_DEPTH levels (more than 4^12 objects)");
    (void)hipSetDevice(c->device);
    if (c->objectCount > c->rayRebuildCapacity) {
        // (a host that grows and never calls anything that waits: the parked memory is bounded, as in chordvis_set_object_list)
        if (c->retired.size() >= 32u) { CHORD_HIP(c, hipStreamSynchronize(c->stream)); free_retired(c); }
        const int rc = grow_rebuild_buffers(c, c->objectCount);
        if (rc) return rc;
    }

    // commit: a host-built TLAS is parked (traces in flight read it), the rebuild's buffers become the TLAS
    if (!c->rayTlasRebuilt) drop_ray_tlas(c, true);
    c->dRayTlas = c->dRayRebuildNodes; c->dRayLeafRef = c->dRayRebuildLeafRef; c->dRayCounters = c->dRayRebuildCounters;
    c->dRayLeafBox = c->dRayRebuildLeafBox; c->dRayRoot = c->dRayRebuildRoot;
    c->rayTlasRebuilt = true; c->rayTlasBuilt = true;
    c->rayTlasNodes = shape.nodes; c->rayTlasDepth = shape.depth; c->rayTlasBytes = c->rayRebuildBytes;
    chord::launch_ray_tlas_rebuild(c, shape);
    chord::launch_ray_refit(c);
    CHORD_HIP(c, hipGetLastError());
    c->rayRefitDue = false;
    return CHORDVIS_OK;
}

int chordvis_readback_ray_tlas(ChordCtx* c, ChordRayNode* hostNodes, uint32_t nodeCapacity, uint32_t* hostLeafRef, uint32_t objectCapacity)
{
    if (!c) return CHORDVIS_E_INVALID;
    if (c->sharedScene) return refuse(c, CHORDVIS_E_INVALID, "readback_ray_tlas", "not on a depth-view context");
    if (!c->sceneLoaded) return refuse(c, CHORDVIS_E_INVALID, "readback_ray_tlas", "no scene (call chordvis_upload_scene first)");
    if (!(c->rayBlasBuilt && c->rayTlasBuilt))
        return refuse(c, CHORDVIS_E_INVALID, "readback_ray_tlas", "no ray scene, or it was dropped by chordvis_upload_scene / chordvis_set_object_list (call chordvis_build_ray_scene, or chordvis_rebuild_ray_tlas)");
    if ((hostNodes && nodeCapacity < c->rayTlasNodes) || (hostLeafRef && objectCapacity < c->objectCount))
        return refuse(c, CHORDVIS_E_INVALID, "readback_ray_tlas", "nodeCapacity / objectCapacity below the TLAS's node count (chordvis_ray_scene_info) / the object count");
    (void)hipSetDevice(c->device);
    CHORD_HIP(c, hipStreamSynchronize(c->stream));
    if (hostNodes) CHORD_HIP(c, hipMemcpy(hostNodes, c->dRayTlas, sizeof(ray::Node) * (size_t)c->rayTlasNodes, hipMemcpyDeviceToHost));
    if (hostLeafRef) CHORD_HIP(c, hipMemcpy(hostLeafRef, c->dRayLeafRef, sizeof(uint32_t) * (size_t)c->objectCount, hipMemcpyDeviceToHost));
    return CHORDVIS_OK;
}

} // extern "C"
