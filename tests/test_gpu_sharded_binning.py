"""Sharded frames through the set-up kernels' own binners: large records (wave_bin_large) and clip triangles (the clip pass)
filter by the rank's tiles (owns_tile / owns_rect) like the primary bins.

Each case is rendered as a sharded frame on one device (helpers.sharded_contexts / sharded_frame: a context per rank, the
all-gathers as device-to-device copies), two frames (no history, then the two-pass HZB), under NO_BLOCKS and FORCE_BLOCKS on
every context:
  * floor / masked_floor: a camera just above a coarse floor (opaque / alpha-tested), 3 ranks on the checker map;
  * near_layers: scenes.stacked_layers("near"), every triangle clipped at the near plane, 2 ranks;
  * ground: config 3's street at 1280 x 720 from a hand above the ground, 4 ranks (large records across many tiles).
Every rank's image is the oracle's; the case's clip triangles / large records occur on some rank (the guard); and,
in the record form, every rank's per-tile bin counts of both passes are 0 on the tiles it does not own and equal the
single-GPU context's on the tiles it owns -- a binner that binned another rank's tile, or dropped one of its own, fails."""
import numpy as np
import pytest

import helpers as H
import orc
from chord_amd import scenes

pytestmark = pytest.mark.gpu

NO_BLOCKS, FORCE_BLOCKS = 32768, 65536


def _ground():
    scene, _ = scenes.config3_street(1280, 720)
    return scene, scenes.Camera((-62.0, 0.25, 3.0), (1.0, -0.02, -0.04), 1280, 720)


# (name, builder, ranks, tile map, what the frames must have: "clip" triangles, "large" records)
CASES = [
    ("floor", lambda: scenes.floor_under_camera(width=256, height=192), 3, "checker", ("clip", "large")),
    ("masked_floor", lambda: scenes.masked_floor_under_camera(width=320, height=192), 3, "checker", ("clip", "large")),
    ("near_layers", lambda: scenes.stacked_layers("near"), 2, "default", ("clip",)),
    # (this still camera sees no triangle that straddles the near plane -- the oracle clips none --: large records only)
    ("ground", _ground, 4, "default", ("large",)),
]


def _counts(r, tiles, p):
    from chord_amd import lib as L
    ticks = np.zeros(tiles * 9, np.uint64)
    cnt = np.zeros(tiles, np.uint32)
    assert L.lib.chordvis_debug_tile_profile(r._ctx, p, ticks.ctypes.data, cnt.ctypes.data, tiles * 9) == 0
    return cnt.astype(np.int64)


@pytest.mark.parametrize("mode", [NO_BLOCKS, FORCE_BLOCKS], ids=["records", "blocks"])
@pytest.mark.parametrize("name,builder,ranks,tile_map,needs", CASES, ids=[c[0] for c in CASES])
def test_sharded_set_up_binners_bin_only_the_ranks_tiles(gpu, name, builder, ranks, tile_map, needs, mode):
    from chord_amd.renderer import VisibilityRenderer
    scene, cam, view, iv = H.setup_scene(builder)
    w, h, flags = cam.width, cam.height, H.ALL_FLAGS
    tiles = ((w + 63) // 64) * ((h + 63) // 64)
    single = VisibilityRenderer(0)
    single.upload_scene(scene)
    single.allocate_gbuffer(w, h)
    single.set_view(view, iv, flags)
    single.set_debug(mode)
    ctxs = H.sharded_contexts(scene, view, iv, w, h, flags, ranks, tile_map, debug_of_rank=lambda rk: mode)
    owners = ctxs[0].tile_owners()
    assert all(np.array_equal(r.tile_owners(), owners) for r in ctxs) and len(set(owners.tolist())) == ranks
    prev = None
    clipped = larges = 0
    for frame in range(2):
        want = orc.frame_mt(scene, view, iv, flags, prev, 16)
        prev = want["hzb_min"]
        single.render_frame()
        H.assert_vis_equal(single.read_visibility(), want["vis"], w, h, "%s frame %d, single GPU" % (name, frame))
        H.sharded_frame(ctxs)
        sts = [r.stats() for r in ctxs]
        for rk, r in enumerate(ctxs):
            H.assert_vis_equal(r.read_visibility(), want["vis"], w, h, "%s frame %d, rank %d" % (name, frame, rk))
            assert sts[rk]["overflow"] == 0, (name, frame, rk)
        clipped += sum(sum(st["clipTriangles"]) for st in sts)
        larges += sum(sum(st["largeRecords"]) for st in sts)
        if mode != NO_BLOCKS:
            continue
        for p in (0, 1):
            ref = _counts(single, tiles, p)
            for rk, r in enumerate(ctxs):
                got = _counts(r, tiles, p)
                mine = owners == rk
                assert not got[~mine].any(), (name, frame, p, rk, "binned tiles of other ranks", np.nonzero(got * ~mine)[0][:8].tolist())
                assert np.array_equal(got[mine], ref[mine]), (name, frame, p, rk, np.nonzero((got != ref) & mine)[0][:8].tolist())
    # the guard: the set-up binners had the clip triangles / large records the case is there for to bin on some rank
    assert (clipped > 0 or "clip" not in needs) and (larges > 0 or "large" not in needs), (name, clipped, larges)
    for r in ctxs + [single]:
        r.close()
