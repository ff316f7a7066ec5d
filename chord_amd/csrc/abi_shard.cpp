// C ABI, sharded contexts: chordvis_set_shard, the tile map and its device tables, the exchange buffers of a sharded frame and their
// accessors, and the second pair of visibility buffers of pipelined frames.

#include "host_layer.h"

using namespace chord;

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

} // namespace chord

extern "C" {

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

uint64_t chordvis_hzb_exchange_chunk_halves(ChordCtx* c) { return c ? c->hzbExchangeChunkHalves : 0; }

} // extern "C"
