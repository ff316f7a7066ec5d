// C ABI, measurement and debugging aids: chordvis_set_debug and every chordvis_debug_* entry point.

#include "host_layer.h"

using namespace chord;

extern "C" {

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

} // extern "C"
