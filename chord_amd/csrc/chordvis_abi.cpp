// C ABI, the scene: chordvis_upload_scene, the object list of a resident scene, object records and world transforms, and the work
// buffers sized by the scene's counts.  The other entry points are in abi_*.cpp, one file per feature; this one, the largest piece,
// keeps the name the whole host layer once had.

#include "host_layer.h"

using namespace chord;

namespace {

// The per-object static table and the totals every launch is sized by, from an object list and the resident scene's tables (hPrims,
// hPrimMeshlets, hPrimTriangles, hMatFlags, hMatType), in O(count): what chordvis_upload_scene and chordvis_set_object_list share.
// Nothing of the context is written but `out` (the caller's) and, on a refusal, the error text.
struct ObjectListTotals { uint64_t groupInst = 0, cmdCap = 0, instTriangles = 0; };

int derive_object_list(ChordCtx* c, const char* fn, const ChordObject* objects, uint32_t count, std::vector<DObjStatic>& out, ObjectListTotals& t)
{
    const size_t primCount = c->hPrims.size(), materialCount = c->hMatFlags.size();
    out.assign(count, DObjStatic{});
    t = ObjectListTotals{};
    for (uint32_t o = 0; o < count; o++) {
        const ChordObject& ob = objects[o];
        if (ob.GLTFPrimitiveDetail >= primCount || ob.GLTFMaterialData >= materialCount)
            return refuse(c, CHORDVIS_E_INVALID, fn, "object primitive/material id out of range");
        if (ob.GLTFMaterialData >= (1u << 24)) return refuse(c, CHORDVIS_E_CAPACITY, fn, "more than 2^24 materials");
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
        return refuse(c, CHORDVIS_E_CAPACITY, fn, "more than 2^24-2 cluster instances do not fit the 24-bit visibility id (base.h:412)");
    return CHORDVIS_OK;
}

} // namespace

namespace chord {

// what chordvis_upload_world_transforms keeps (hipFree waits for the device: a build in flight finishes on memory that is still its own)
void drop_world_transforms(ChordCtx* c)
{
    dfree(c->dWorldCur); dfree(c->dWorldPrev); dfree(c->dBuildStatus);
    c->buildCount = 0;
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

} // namespace chord

extern "C" {

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
            for (uint32_t l = 0; l < d.texMips && l < CHORD_MAX_TEX_LEVELS; l++) {
                const uint32_t w = std::max(1u, d.texWidth >> l), h = std::max(1u, d.texHeight >> l);
                chord::DMatLevel& L = d.levels[l];
                L.base = off; L.dims = (w - 1u) | (h - 1u) << 16;
                tex_wrap_constants(w, d.wrapS, L.magicS, L.biasS);
                tex_wrap_constants(h, d.wrapT, L.magicT, L.biasT);
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

} // extern "C"
