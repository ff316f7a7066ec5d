// C ABI, the consumers of a rendered frame's visibility image: the tile marker and shading tiles, the attribute / surface / material /
// G-buffer resolves, material and geometry feedback, and the bounds queries.

#include "host_layer.h"

using namespace chord;

extern "C" {

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

// ---------------------------------------------------------------- per-pixel attributes of the visible triangle --

// The preconditions chordvis_resolve_attributes and chordvis_resolve_surface share, in this order: a scene and gbuffer, a frame
// since, no update_objects / set_view after it, a command list, a target, debugMode within range.  `fn` names the entry point in
// the messages.
static int resolve_checks(ChordCtx* c, const char* fn, ChordCountAndCmd drawed, bool anyTarget, bool wantDebug, const ChordResolveDesc& d)
{
    const int E = CHORDVIS_E_INVALID;
    if (!c || !c->dVis || !c->sceneLoaded) return refuse(c, E, fn, "no scene / gbuffer");
    if (!c->resolveFrame) return refuse(c, E, fn, "no frame rendered yet");
    if (c->resolveStale) return refuse(c, E, fn, "chordvis_update_objects / chordvis_bind_objects / chordvis_set_view came after the frame (the image's matrices are gone)");
    if (!drawed.count || !drawed.cmds) return refuse(c, E, fn, "null command list");
    if (!anyTarget) return refuse(c, E, fn, "no target");
    if (wantDebug && d.debugMode > CHORD_NANITE_DEBUG_BARYCENTRICS) return refuse(c, E, fn, "debugMode beyond 4");
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
    const int E = CHORDVIS_E_INVALID;
    const bool anySurface = ss.vertexNormal || ss.tangent || ss.bitangent;
    const bool anyMaterial = mm.baseColor || mm.emissive || mm.pixelNormal || mm.roughMetalAO;
    if (ss.pad) return refuse(c, E, fn, "ChordSurfaceTargets::pad must be NULL");
    if ((ss.tangent || ss.bitangent) && !c->dTangents) return refuse(c, E, fn, "the scene was uploaded without tangents (ChordAssetDesc::tangents)");
    if (anySurface && !c->dNormals) return refuse(c, E, fn, "the scene was uploaded without normals (ChordAssetDesc::normals)");
    if (anyMaterial && !c->matTexturesLoaded) return refuse(c, E, fn, "no chordvis_upload_material_textures since the last chordvis_upload_scene");
    if (mm.pixelNormal && !c->dNormals) return refuse(c, E, fn, "pixelNormal needs a scene uploaded with normals (ChordAssetDesc::normals)");
    if (mm.pixelNormal && c->matAnyNormalTexture && !c->dTangents)
        return refuse(c, E, fn, "pixelNormal with a normal texture needs a scene uploaded with tangents (ChordAssetDesc::tangents)");
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

} // extern "C"
