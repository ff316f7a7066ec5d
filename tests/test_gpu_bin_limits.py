"""Tile bins at the limits of their pool (chordvis_set_limits: binPoolChunks, binMaxChunksPerTile), through each binner that
reaches the pool chunks.

A tile's bin holds binCap entries in its fixed part; entries past that live in 1 024-entry chunks drawn from a per-pass pool,
at most binMaxChunksPerTile per tile.  A slot past either limit is dropped and sets overflow bit 1 (chordvis_stats then says
CHORDVIS_E_CAPACITY); bit 4 would mean that a bin_put waited for a chunk that was never allocated (a binner that broke the
bin_alloc-before-bin_put contract).  Per-tile, per-pass slot counts (chordvis_debug_tile_profile) are raw: not clamped.

Each case names the binner whose bins reach the chunks, and a guard proves it did:
  * config4: config 4 at 640 x 360 in the record form (NO_BLOCKS) -- raster_setup_kernel's primary / straddle bins;
  * large: scenes.stacked_layers("large") -- every triangle a large record, binned by the set-up kernel itself;
  * near: scenes.stacked_layers("near") -- every triangle clipped at the near plane and binned by the set-up kernel's clip pass;
  * hotspot: config 5's hotspot variant, reduced, as pixel blocks (FORCE_BLOCKS) -- raster_setup_blocks_kernel;
  * wide: the large layers as a camera cut in a light later pass (every object 'was' 500 m further down the view), so that
    raster_setup_wide_kernel sets up and bins all of them in pass 1.
For every case, with n_t the slot counts of the pass at generous limits, k = max_t ceil((n_t - binCap) / 1024) and
P = sum_t ceil(max(0, n_t - binCap) / 1024):
  1. generous limits: exact against the oracle, overflow 0;
  2. bin_max_chunks_per_tile = k: exact, overflow 0, the same counts; k - 1: CHORDVIS_E_CAPACITY with overflow exactly 1;
  3. bin_pool_chunks = P: exact; P - 1: the same as k - 1;
  4. (single-pass cases) the overflowed frames drop entries and never invent any: tiles within the capacity in force are exact,
     and no pixel word is above the oracle's;
  5. the same context then renders a frame of the scene with some objects moved out of view, whose bins still reach the pool
     but fit the limits: exact, overflow 0 (no chunk-table entry or pool count of the overflowed frame is used again).
The hot-tile block variant (FORCE_HOT) draws bin slots ahead and leaves some empty, so its slot counts are not a property of
the scene; it is not one of the cases."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import orc
from chord_amd import records as R
from chord_amd import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_BLOCKS, FORCE_BLOCKS = 32768, 65536
ONE_PASS = R.FLAG_FRUSTUM_CULL | R.FLAG_CONE_CULL
GENEROUS = dict(bin_pool_chunks=16384, bin_max_chunks_per_tile=2048)
E_CAPACITY = -4


def _layout():
    """CHORD_BIN_CAP / CHORD_TILE / CHORD_BIN_CHUNK of the 64-pixel tile build, as device_layer.h defines them (its block of
    bin and tile macros, compiled into a probe that prints them)."""
    import tempfile
    src = open(os.path.join(ROOT, "chord_amd", "csrc", "device_layer.h")).read()
    block = src[src.index("#define CHORD_BIN_CHUNK_SHIFT"):src.index("static_assert(CHORD_BIN_CAP")]
    probe = ('#include <stdio.h>\n%s\nint main(void){printf("%%u %%u %%u\\n", (unsigned)(CHORD_BIN_CAP), (unsigned)(CHORD_TILE), '
             '(unsigned)(CHORD_BIN_CHUNK)); return 0;}\n' % block)
    with tempfile.TemporaryDirectory() as td:
        cpath, exe = os.path.join(td, "layout.c"), os.path.join(td, "layout")
        open(cpath, "w").write(probe)
        cc = subprocess.run(["gcc", "-std=c11", cpath, "-o", exe], capture_output=True, text=True)
        assert cc.returncode == 0, cc.stderr[-1500:]
        cap, tile, chunk = (int(x) for x in subprocess.check_output([exe]).split())
    return {"BIN_CAP": cap, "TILE": tile, "CHUNK": chunk}


LAYOUT = _layout()
BIN_CAP, CHUNK = LAYOUT["BIN_CAP"], LAYOUT["CHUNK"]


def test_layout_is_the_64_pixel_tile_build():
    assert LAYOUT == {"BIN_CAP": 16384, "TILE": 64, "CHUNK": 1024}, LAYOUT


# ------------------------------------------------------------------------------------------------------------------ cases --

def _case(name):
    """(scene, camera, flags, debug, objects that may be moved out of view)."""
    if name == "config4":
        scene, cam = scenes.config4_street_x64(640, 360)
        return scene, cam, ONE_PASS, NO_BLOCKS, len(scene.objects)
    if name in ("large", "wide"):
        scene, cam = scenes.stacked_layers("large")
        return scene, cam, (H.ALL_FLAGS if name == "wide" else ONE_PASS), NO_BLOCKS, len(scene.objects) - 1   # (not the backdrop)
    if name == "near":
        scene, cam = scenes.stacked_layers("near")
        return scene, cam, ONE_PASS, NO_BLOCKS, len(scene.objects)
    if name == "hotspot":
        scene, cam = scenes.config5_subpixel(960, 540, prims=32, patches_per_prim=256, instances=8, hotspot_sigma_px=32.0)
        return scene, cam, ONE_PASS, FORCE_BLOCKS, len(scene.objects)
    raise ValueError(name)


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _case(name)
    return _CASES[name]


def moved_out(scene, movable, part):
    """local_to_world of the scene with a share of its first `movable` objects 1 000 km to the side: part 1 = every fourth, 2 =
    every second, 3 = three of four (interleaved, so that every crowded tile loses about that share)."""
    l2w = scene.local_to_world.copy()
    idx = np.arange(movable)
    sel = idx[(idx % 4) < part]
    l2w[sel, 12] += 1.0e6                                  # glm column-major: the translation column
    return l2w


def frames(name, part):
    """[(scene with its object records, view, iv, camera)] of the frames a case renders in order on one context, with the
    objects of the reduced frames moved out by `part` (0: none).  Single-pass cases: one frame.  wide: frames 0 and 1 of the
    reduced scene, frame 2 the whole scene as a camera cut (objects 'were' 500 m further down the view: a history HZB behind
    the backdrop rejects them all in stage 0, and the host still announces the second pass light), frame 3 the reduced scene
    as a cut again."""
    from chord_amd import lib as L
    scene, cam, flags, debug, movable = case(name)
    full = scene.local_to_world
    red = moved_out(scene, movable, part) if part else full
    if name != "wide":
        plan = [(red, None)]
    else:
        f = np.asarray(cam.front, np.float64)
        f /= np.linalg.norm(f)

        def cut(m):
            last = m.copy()
            last[:, 12:15] += 500.0 * f
            return last
        plan = [(red, None), (red, None), (full, cut(full)), (red, cut(red))]
    out = []
    view0, _ = L.make_views(cam)
    for l2w, last in plan:
        view, iv = L.make_views(cam, view0)
        sc = scene.with_objects(scene.objects.copy())
        sc.local_to_world = np.ascontiguousarray(l2w)
        L.fill_objects(sc, cam, cam, last)
        out.append((sc, view, iv, cam))
    return out


_ORACLE = {}


def oracle(name, part):
    """The oracle's frames of frames(name, part), each with the history of the one before."""
    key = (name, part)
    if key not in _ORACLE:
        _, _, flags, _, _ = case(name)
        prev, res = None, []
        for sc, view, iv, cam in frames(name, part):
            want = orc.frame_mt(sc, view, iv, flags, prev, 16)
            res.append(want)
            prev = want["hzb_min"]
        _ORACLE[key] = res
    return _ORACLE[key]


# --------------------------------------------------------------------------------------------------------------- running --

def _raw_stats(r):
    from chord_amd import lib as L
    st = L.Stats()
    rc = L.lib.chordvis_stats(r._ctx, C.byref(st))
    return rc, st.as_dict()


def _tile_counts(r, tiles, p):
    from chord_amd import lib as L
    ticks = np.zeros(tiles * 9, np.uint64)
    cnt = np.zeros(tiles, np.uint32)
    assert L.lib.chordvis_debug_tile_profile(r._ctx, p, ticks.ctypes.data, cnt.ctypes.data, tiles * 9) == 0
    return cnt.astype(np.int64)


def render(gpu, name, limits, parts=(0,)):
    """Render the frames of `name` for every entry of parts in turn on ONE context with the given limits: per frame a dict of the
    image, the raw chordvis_stats return code and stats, both passes' tile counts and the set-up kernels of both passes."""
    from chord_amd import lib as L
    from chord_amd.renderer import VisibilityRenderer
    scene, cam, flags, debug, _ = case(name)
    tiles = ((cam.width + 63) // 64) * ((cam.height + 63) // 64)
    r = VisibilityRenderer(0)
    r.set_limits(**limits)
    r.upload_scene(scene)
    r.allocate_gbuffer(cam.width, cam.height)
    r.set_debug(debug)
    out = []
    for part in parts:
        seq = []
        for sc, view, iv, _ in frames(name, part):
            r.update_objects(sc.objects)
            r.set_view(view, iv, flags)
            r.render_frame()
            rc, st = _raw_stats(r)
            wide = (C.c_uint32 * 2)()
            assert L.lib.chordvis_debug_setup_kernels(r._ctx, wide) == 0
            seq.append(dict(vis=r.read_visibility(), rc=rc, st=st, counts=[_tile_counts(r, tiles, p) for p in (0, 1)], wide=list(wide)))
        out.append(seq)
    r.close()
    return out


def chunks_needed(counts):
    """(k, P): the most chunks one tile takes, and the chunks of all tiles together."""
    over = np.maximum(counts - BIN_CAP, 0)
    per = (over + CHUNK - 1) // CHUNK
    return int(per.max()), int(per.sum())


def _pass(name):
    return 1 if name == "wide" else 0


def _frame_of_interest(name):
    return 2 if name == "wide" else 0


def guard(name, got, want):
    """The case took the binner it is there for, and that binner's bins reached the pool chunks."""
    i, p = _frame_of_interest(name), _pass(name)
    g = got[i]
    st, n = g["st"], g["counts"][p]
    assert int(n.max()) > BIN_CAP + 2 * CHUNK, (name, int(n.max()))
    if name in ("large", "near", "wide"):
        # (CHORDVIS_BIN_IN_SETUP, read once per process: 0 would bin these records with the separate binner launch instead)
        assert os.environ.get("CHORDVIS_BIN_IN_SETUP", "1") != "0", "the in-setup binners are switched off in this process"
    if name == "config4":
        assert st["pixelBlocks"] == 0 and g["wide"] == [0, 0], (name, st["pixelBlocks"], g["wide"])
    elif name == "large":
        # every layer triangle is a large record; the backdrop's 128 small triangles are the only other entries of a tile
        assert st["clipTriangles"] == [0, 0] and st["largeRecords"][0] >= int(n.max()) - 128, (st["largeRecords"], int(n.max()))
        assert want[i]["stats"].trianglesClipped == 0
    elif name == "near":
        assert st["clipTriangles"][0] == want[i]["stats"].trianglesSubmitted == want[i]["stats"].trianglesClipped, st["clipTriangles"]
        assert st["pixelBlocks"] == 0
    elif name == "hotspot":
        assert st["pixelBlocks"] >= int(n.max()) and st["pixelBlockBytes"] > 0, (st["pixelBlocks"], int(n.max()))
    elif name == "wide":
        assert g["wide"][1] == 1, g["wide"]                                   # pass 1 set up by the wide kernel
        assert st["countStage1Visible"] == len(case(name)[0].meshlets) <= 1024, st["countStage1Visible"]
        assert st["largeRecords"][1] >= int(n.max()) - 128 and int(g["counts"][0].max()) == 0, (st["largeRecords"], g["counts"][0].max())


def assert_exact(name, got, want, what, submitted=True):
    cam = case(name)[1]
    for i, (g, w) in enumerate(zip(got, want)):
        H.assert_vis_equal(g["vis"], w["vis"], cam.width, cam.height, "%s frame %d, %s" % (name, i, what))
        assert g["rc"] == 0 and g["st"]["overflow"] == 0, (name, i, what, g["rc"], g["st"]["overflow"])
        if submitted:
            assert g["st"]["trianglesSubmitted"] == w["stats"].trianglesSubmitted, (name, i, what)


def assert_dropped_not_invented(name, g, want, cap, counts):
    """An overflowed single-pass frame: tiles whose count fits the capacity in force are exact, and no word is above the
    oracle's (entries may be lost, none may come from a stale or invalid chunk)."""
    cam = case(name)[1]
    w, h = cam.width, cam.height
    got = np.asarray(g["vis"], np.uint64).reshape(h, w)
    ref = np.asarray(want["vis"], np.uint64).reshape(h, w)
    assert (got <= ref).all(), (name, int((got > ref).sum()))
    tx = (w + 63) // 64
    for t in np.nonzero(counts <= cap)[0]:
        x, y = int(t % tx) * 64, int(t // tx) * 64
        assert np.array_equal(got[y:y + 64, x:x + 64], ref[y:y + 64, x:x + 64]), (name, "tile", int(t), int(counts[t]))


def assert_capacity_error(name, g, what):
    assert g["rc"] == E_CAPACITY and g["st"]["overflow"] == 1, (name, what, g["rc"], g["st"]["overflow"])


def _limits(tag, k, P, short=False):
    if tag == "k":
        return dict(bin_pool_chunks=16384, bin_max_chunks_per_tile=k - (1 if short else 0))
    return dict(bin_pool_chunks=P - (1 if short else 0), bin_max_chunks_per_tile=2048)


SINGLE = ("config4", "large", "near", "hotspot")


@pytest.mark.parametrize("name", SINGLE)
def test_single_pass_bins_at_the_pool_and_per_tile_chunk_limits(gpu, name):
    want = oracle(name, 0)
    # 1. generous limits
    (gen,) = render(gpu, name, GENEROUS)
    assert_exact(name, gen, want, "generous limits")
    guard(name, gen, want)
    n = gen[0]["counts"][0]
    k, P = chunks_needed(n)
    assert k >= 2 and P >= k, (name, k, P)
    # the recovery frame of step 5: the first share of objects moved out whose bins still reach the pool but fit k - 1 and P - 1
    part, tries = None, render(gpu, name, GENEROUS, parts=(1, 2, 3))
    for pt, (fr,) in zip((1, 2, 3), tries):
        kk, pp = chunks_needed(fr["counts"][0])
        if int(fr["counts"][0].max()) > BIN_CAP and kk <= k - 1 and pp <= P - 1:
            part = pt
            break
    assert part is not None, (name, k, P, [chunks_needed(fr["counts"][0]) for (fr,) in tries])
    want_red = oracle(name, part)
    assert_exact(name, tries[part - 1], want_red, "reduced frame, generous limits")
    for tag in ("k", "P"):
        # 2. / 3. at the limit: exact, with the same counts
        (at,) = render(gpu, name, _limits(tag, k, P))
        assert_exact(name, at, want, "%s at %s" % (tag, _limits(tag, k, P)))
        assert np.array_equal(at[0]["counts"][0], n), (name, tag)
        # one chunk short: CHORDVIS_E_CAPACITY with overflow bit 1 alone, entries dropped and none invented (4.), then the
        # reduced frame on the same context (5.)
        over, rec = render(gpu, name, _limits(tag, k, P, short=True), parts=(0, part))
        assert_capacity_error(name, over[0], "%s - 1" % tag)
        assert_dropped_not_invented(name, over[0], want[0], BIN_CAP + (k - 1) * CHUNK if tag == "k" else BIN_CAP, n)
        assert_exact(name, rec, want_red, "%s - 1, the frame after the overflowed one" % tag)
        assert int(rec[0]["counts"][0].max()) > BIN_CAP, name


WIDE_PART = 1


def test_wide_setup_bins_at_the_pool_and_per_tile_chunk_limits(gpu):
    """The wide case: frames 0, 1 (reduced: a quarter of the layers out of view), 2 (all layers, a cut: pass 1 set up by
    raster_setup_wide_kernel), 3 (reduced, a cut again) on one context.  k and P are those of frame 2's pass 1; at k - 1 / P - 1
    frames 0 and 1 fit, frame 2 overflows, and frame 3 on the same context is exact again."""
    name = "wide"
    want = oracle(name, WIDE_PART)
    (gen,) = render(gpu, name, GENEROUS, parts=(WIDE_PART,))
    assert_exact(name, gen, want, "generous limits")
    guard(name, gen, want)
    k, P = chunks_needed(gen[2]["counts"][1])
    assert k >= 2 and P >= k, (k, P)
    # the reduced frames fit one chunk less, and frame 3's pass 1 still reaches the pool
    for i, q in ((0, 0), (1, 0), (1, 1), (3, 0), (3, 1)):
        kk, pp = chunks_needed(gen[i]["counts"][q])
        assert kk <= k - 1 and pp <= P - 1, (i, q, kk, pp, k, P)
    assert int(gen[3]["counts"][1].max()) > BIN_CAP
    for tag in ("k", "P"):
        (at,) = render(gpu, name, _limits(tag, k, P), parts=(WIDE_PART,))
        assert_exact(name, at, want, "%s at %s" % (tag, _limits(tag, k, P)))
        assert at[2]["wide"][1] == 1
        for i in range(4):
            for q in (0, 1):
                assert np.array_equal(at[i]["counts"][q], gen[i]["counts"][q]), (tag, i, q)
        (seq,) = render(gpu, name, _limits(tag, k, P, short=True), parts=(WIDE_PART,))
        assert_exact(name, seq[:2], want[:2], "%s - 1, frames before the cut" % tag)
        assert seq[2]["wide"][1] == 1, seq[2]["wide"]
        assert_capacity_error(name, seq[2], "%s - 1" % tag)
        # (frame 3's history HZB is that of the overflowed frame: the image must be exact, how its clusters split over the two
        # passes need not be the oracle's)
        assert_exact(name, seq[3:], want[3:], "%s - 1, the frame after the overflowed one" % tag, submitted=False)
