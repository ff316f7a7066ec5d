"""Inputs for chordvis_bin_bounds: hand-made ChordBoundsResult records aimed at the edges of the pair test, and the boxes of the
rendered-frame case.  TEST INFRASTRUCTURE, shared by tests/test_bounds_tiles_spec.py (CPU) and tests/test_gpu_bounds_tiles.py."""
import numpy as np

from chord_amd import records as R

import bounds_scenes as B
import spec_bounds_tiles_np as S

F32_ONE = 0x3F800000

# the rendered-frame case: small_test_scene under bounds_scenes.two_frames' cameras, boxes of bounds_scenes.make_boxes under a seed of
# their own, binned into RENDERED_TILE-pixel tiles with room for RENDERED_MAX_PER_TILE boxes per tile (chosen on the CPU so that every
# way the pair test can go occurs and some tile overflows: tests/test_bounds_tiles_spec.py asserts it)
RENDERED_SIZE = (160, 96)
RENDERED_BOXES = 600
RENDERED_SEED = 29
RENDERED_TILE = 16
RENDERED_MAX_PER_TILE = 96            # (the boxes that reach the near plane, about 80 of the 600, are in every tile's list)


def rendered_boxes():
    """(scene, cam_last, cam, (view_last, iv_last), (view, iv), queries) of the rendered-frame case."""
    scene, cam_last, cam, first, second = B.two_frames(*RENDERED_SIZE)
    queries, _ = B.make_boxes(cam, cam_last, RENDERED_BOXES, seed=RENDERED_SEED)
    return scene, cam_last, cam, first, second, queries


CHUNK, CHUNK_DEBUG, CANDIDATE_SLOTS = 256, 64, 512      # kernels_tiles.hip: records per step (debug bit 33554432: 64), BOUNDS_TILES_CAND


def midstream_flushes(results, w, h, chunk):
    """The tile kernel's flush rule replayed per 64 x 64-pixel block: how often the block whose candidate list fills most often
    flushes it BEFORE its last chunk -- because the next chunk might not fit --, carrying the tiles' counts and the ascending order
    over to the next fill.  (The flush after the last chunk is not counted.)"""
    part = np.flatnonzero(S.participates(results))
    rect = results["rect"][part].astype(np.int64)
    most = 0
    for by0 in range(0, h, 64):
        for bx0 in range(0, w, 64):
            bx1, by1 = min(w, bx0 + 64) - 1, min(h, by0 + 64) - 1
            hit = (rect[:, 0] <= bx1) & (rect[:, 2] >= bx0) & (rect[:, 1] <= by1) & (rect[:, 3] >= by0)
            held = flushes = 0
            for base in range(0, len(part), chunk):
                held += int(hit[base:base + chunk].sum())
                assert held <= CANDIDATE_SLOTS
                last = base + chunk >= len(part)
                if last or held + chunk > CANDIDATE_SLOTS:
                    flushes += 0 if last else 1
                    held = 0
            most = max(most, flushes)
    return most


def piled_results(w, h, T, depth, count, seed):
    """handmade_results in which every record takes part and three of four cover the whole screen: every block collects three
    quarters of the records as candidates, so its list fills and is flushed mid-stream (midstream_flushes says how often)."""
    out = handmade_results(w, h, T, depth, count, seed)
    out["status"] |= R.BOUNDS_IN_FRUSTUM | R.BOUNDS_UNOCCLUDED
    whole = np.arange(count) % 4 != 3
    out["rect"][whole] = (0, 0, w - 1, h - 1)
    return out


def handmade_results(w, h, T, depth, count, seed):
    """`count` records.BOUNDS_RESULT made by hand against the tiles of a w x h image whose depth bounds are `depth`
    (spec_bounds_tiles_np.tile_depth).  Record i takes its rectangle from case i % 8, its nearestZ from case i % 5 and its status from
    the rule below, each around a tile picked at random:
      rectangles  0 exactly the tile: ends on the tile's last pixel        1 one pixel further: ends on the next tiles' first pixels
                  2 a single pixel (every other one a tile's first or last) 3 the whole screen
                  4 from the tile to beyond the right and bottom edges      5 wholly beyond the right or the bottom edge
                  6 any rectangle                                           7 from the tile's last pixel on: the neighbours' first
      nearestZ    the tile's far bits, one ulp below, one ulp above, a random depth, 1.0
      status      two records of three take part (IN_FRUSTUM | UNOCCLUDED, with random further bits and a level); every third walks
                  through all 32 combinations of the five status bits."""
    rng = np.random.default_rng([int(seed), int(w), int(h), int(T), int(count)])
    tiles, tx, _ = S.tile_count(w, h, T)
    out = np.zeros(count, dtype=R.BOUNDS_RESULT)
    for i in range(count):
        t = int(rng.integers(tiles))
        x0, y0 = (t % tx) * T, (t // tx) * T
        x1, y1 = min(w, x0 + T) - 1, min(h, y0 + T) - 1
        a, b = (int(v) for v in rng.integers(1, 100, size=2))
        kind = i % 8
        if kind == 0:
            rect = (x0, y0, x1, y1)
        elif kind == 1:
            rect = (x0, y0, x1 + 1, y1 + 1)
        elif kind == 2:
            px, py = int(rng.integers(w)), int(rng.integers(h))
            if (i // 8) % 2:
                px, py = (x0, y1) if (i // 16) % 2 else (x1, y0)
            rect = (px, py, px, py)
        elif kind == 3:
            rect = (0, 0, w - 1, h - 1)
        elif kind == 4:
            rect = (x0, y0, w - 1 + a, h - 1 + b)
        elif kind == 5:
            rect = (w + a, y0, w + a + b, y1) if (i // 8) % 2 else (x0, h + a, x1, h + a + b)
        elif kind == 6:
            xs, ys = np.sort(rng.integers(0, w, size=2)), np.sort(rng.integers(0, h, size=2))
            rect = (int(xs[0]), int(ys[0]), int(xs[1]), int(ys[1]))
        else:
            rect = (x1, y1, x1 + a % (2 * T), y1 + b % (2 * T))
        far = int(depth[t, 0])
        z = (far, max(far - 1, 0), far + 1, int(np.float32(rng.random()).view(np.uint32)), F32_ONE)[i % 5]
        if i % 3 == 0:
            status = (i // 3) % 32
        else:
            status = R.BOUNDS_IN_FRUSTUM | R.BOUNDS_UNOCCLUDED | (int(rng.integers(8)) << 2) | (int(rng.integers(12)) << R.BOUNDS_LEVEL_SHIFT)
        out["status"][i] = status
        out["nearestZ"][i] = np.uint32(z).view(np.float32)
        out["rect"][i] = rect
    return out
