"""Frames enqueued ahead of the device on a caller-owned stream (tests/inflight.py has the harness: the gate, the stream-ordered
snapshots, the measured gate length).  Every other GPU test creates the context on its own stream and reads back -- synchronises --
after every frame; bench.py and a real host hand a stream over and enqueue tens of frames without waiting.  Here every scenario
runs on a torch.cuda.Stream of the test's own (or on hipStreamLegacy), behind a gate that keeps the device from starting any of it
until the last call has returned, and every frame is compared exactly with the oracle's chain -- image, list 0, the four stage
counts, the history HZB -- (tests/test_frames_in_flight_spec.py shows, without a GPU, that the states a misordered call would see
give other results).

  A  reports of every age: launch_raster picks kernels from host-mapped words the device writes when a pass finishes.  The
     sequences cut / sky / masked_floor of tests/test_gpu_setup_wide.py with the gate at several frames: before it the frames are
     synchronised one by one, from it on all are enqueued under the report the host held at the gate ('none yet' at position 0).
  B  stale density and hot-tile reports: dense hotspot frames under an empty view's report (no block kernel: the record kernel sets
     up a dense list), the reverse (the block kernel launched onto empty lists), and the block kernel's hot variant launched onto
     empty lists and onto the hotspot under a hot-tile report that is frames old.
  C  caller state in flight: the host buffer of update_objects, set_view twice around pass-by-pass frames (the view as a kernel
     argument, and through flush_view's copy from the context's host record), a bound array rewritten
     on the stream, the caller-owned image, resolves between frames, the state changes that wait, hipStreamLegacy, close().
     test_the_gate_exposes_a_write_that_is_not_ordered is the harness's own sensitivity proof.
  D  depth views: render_shadow ticks between main frames.

WAITS below is what each call did behind the gate on an MI355X -- returned with the gate closed, or waited for the stream -- and is
asserted both ways for every call a scenario makes.

MEASURED DRY RUNS (host seconds of the un-gated call sequence on the throw-away context; the gate is four times that, at least
20 ms), from a run on an MI355X:
  cut, gate at 0 / 3 / 5 (28 / 16 / 8 calls)                    4.8 (first test of the process) .. 1.0 / 0.5 / 0.3 ms
  sky, gate at 0 / 2 (20 / 12 calls)                            3.8 (first) .. 0.9 / 0.4 ms
  masked_floor, gate at 0 / 2 (16 / 8 calls)                    0.5 / 0.2 ms
  (cut, sky, masked_floor: the same to 0.5 ms with the chain snapshotted every frame or after the last, keep default or 0)
  hotspot dense_then_sparse / sparse_then_dense / hot_then_sparse (12 / 20 / 16 calls)   0.2 / 0.3 / 0.4 ms
  24 frames, gate at 0 / 9 (96 / 60 calls)                      1.7 / 1.1 ms
  update_objects, host buffer overwritten / dropped (16 calls)  3.2 (first) / 0.7 ms
  update_objects, 5 MB array overwritten (12 calls)             4.6 .. 34.5 ms between runs (every update_objects waits: WAITS)
  pageable copies, 4 KB .. 16 MB (8 calls)                      under 20 ms (the copies of 2 MB and more wait)
  pass-by-pass frames, one set_view per frame / the view set again (36 / 40 calls)   1.1 / 0.7 ms
  bound objects (17 calls)                                      3.5 ms (first)
  caller-owned image (20 calls)                                 0.9 ms
  resolves in flight (12 calls)                                 1.1 ms
  state changes: upload_history_hzb / reset_history / allocate_gbuffer / upload_scene / upload_material_textures
                 (13 / 13 / 18 / 13 / 13 calls)                 0.5 / 0.4 / 1.6 / 2.7 / 0.7 ms
  hipStreamLegacy (12 calls)                                    0.4 ms
  close() in flight (13 calls)                                  2.2 ms
  misordered write (3 calls)                                    0.4 ms
  render_shadow in flight (10 calls)                            3.4 ms
Every gate but the 5 MB scenario's (up to 138 ms) was therefore at its floor of 20 ms; no dry run needed a second take."""
import time

import numpy as np
import pytest

import helpers as H
import inflight as F

pytestmark = pytest.mark.gpu

# call kind -> whether it waits for the context's stream (True) or is enqueued and returns at once (False)
WAITS = {
    "update_objects": False,  "set_view": False, "render_frame": False, "snapshot": False, "bind_objects": False,
    "clear_gbuffer": False, "instance_culling": False, "visibility_stage0": False, "build_hzb": False, "visibility_stage1": False,
    "resolve_attributes": False, "resolve_gbuffer": False, "render_shadow": False, "reset_history": False,
    "caller_copy": False, "caller_zero": False, "side_stream_copy": False,
    # (22 528 objects, 5 MB: the HIP runtime's copy from pageable memory of that size waits for the stream; 79 KB -- config 3 -- does not)
    "update_objects_5MB": True,
    "upload_history_hzb": True, "allocate_gbuffer": True, "upload_scene": True, "upload_material_textures": True, "close": True,
}


def _entry(name, fn):
    return (name, fn, WAITS[F.kind_of(name)])


def _observe(log, what):
    for kind, waited in F.waits(log).items():
        assert WAITS[kind] == waited, "%s: %s %s" % (what, kind, "waited for the stream" if waited else "did not wait for the stream")


def _frame_entries(ctx, k, hzb=True):
    return [(n, fn, WAITS[F.kind_of(n)]) for n, fn, _ in ctx.frame_calls(k, hzb=hzb)]


# ---------------------------------------------------------------------------------------------- A and B: reports of every age --

def _run_frames(sc, keep, gate_at, what, hzb="each"):
    """The scenario's frames on one context: frames before gate_at synchronised one by one, the rest behind one gate (and, on the
    harness's throw-away context, with no gate and no synchronise: checked too).  hzb: 'each'
    (a snapshot of the chain after every frame), 'last' (after the last frame only: the tail of every other chain rides on the next
    frame's first kernel) or None.  Returns (chordvis_debug_setup_kernels after every render_frame, stats() of the last frame)."""
    n = len(sc.frames)

    def wants_hzb(k):
        return hzb == "each" or (hzb == "last" and k == n - 1)

    def prepare():
        ctx = F.Context(sc, keep=keep)
        for k in range(gate_at):
            F.run_calls(ctx.frame_calls(k, hzb=wants_hzb(k)))
            ctx.synchronize()
        return ctx

    def script(ctx):
        return [e for k in range(gate_at, n) for e in _frame_entries(ctx, k, wants_hzb(k))]

    def check(ctx, what=what):
        for k, f in enumerate(sc.frames):
            F.check_frame(ctx.snaps[k], f.want, "%s, frame %d" % (what, k), hzb=wants_hzb(k),
                          counts=k > 0 and bool(sc.flags & H.R.FLAG_HZB_CULL))
        F.check_stats(ctx, sc.frames[-1].want, what, counts=bool(sc.flags & H.R.FLAG_HZB_CULL))

    if gate_at < n:
        # (the dry run is held to the oracle as well: the same calls with the device free to run, its reports landing between them)
        ctx, log, _ = F.run_behind_gate(prepare, script, what, check_dry=lambda c: check(c, what + ", un-gated"))
    else:
        ctx, log = prepare(), []
    check(ctx)
    words, stats = ctx.words, ctx.r.stats()
    ctx.close()
    _observe(log, what)
    return words, stats


_SYNC_WORDS = {}


def _synchronised_words(name, keep):
    """The set-up kernels of a run that synchronises after every frame, as the rest of the suite does."""
    if (name, keep) not in _SYNC_WORDS:
        sc = F.wide_sequence(name)
        _SYNC_WORDS[name, keep] = _run_frames(sc, keep, len(sc.frames), "%s synchronised, keep %r" % (name, keep))[0]
    return _SYNC_WORDS[name, keep]


# what launch_raster decides for cut's second passes (wide[1] per frame) from the report the host holds:
#   synchronised: frame 1's pass reports light -> frame 2 wide; frame 3 (heavy) still announced light -> wide; frames 4 and 5 under a
#                 heavy report -> not; frame 6 under frame 5's light report -> wide
#   gate at 0:    'none yet' lasts the whole sequence -> never wide
#   gate at 3:    the host has seen frame 2's light report -> frames 3 .. 6 all wide, the heavy frame 4 included
#   gate at 5:    the host has seen frame 4's heavy report -> frames 5 and 6 not wide, though they are light
CUT_WIDE = {"synchronised": [0, 0, 1, 1, 0, 0, 1], 0: [0, 0, 0, 0, 0, 0, 0], 3: [0, 0, 1, 1, 1, 1, 1], 5: [0, 0, 1, 1, 0, 0, 0]}


HZB_MODES = pytest.mark.parametrize("hzb", ["each", "last"], ids=["hzb_each_frame", "hzb_last_frame"])
KEEPS = pytest.mark.parametrize("keep", [None, 0], ids=["keep_default", "keep_0"])


@HZB_MODES
@KEEPS
@pytest.mark.parametrize("gate_at", [0, 3, 5])
def test_cut_under_reports_of_every_age(gpu, gate_at, keep, hzb):
    """cut: light second passes, two heavy ones (frames 3, 4), light again.  Gate at 0: no report ever arrives.  At 3: the host has
    seen 'light' and enqueues both heavy frames and the light ones behind them under it -- frame 4 takes the wide kernel with a list of
    several thousand clusters, which the synchronised run never does.  At 5: the host has seen 'heavy' and enqueues light frames
    under it.  hzb_each_frame snapshots the history chain -- min, max, valid range -- after every frame (history_hzb() launches the
    chain's tail in flight), hzb_last_frame after the last frame only (every other tail rides on the next frame's first kernel)."""
    what = "cut, gate at %d, keep %r, hzb %s" % (gate_at, keep, hzb)
    words, _ = _run_frames(F.wide_sequence("cut"), keep, gate_at, what, hzb=hzb)
    sync = _synchronised_words("cut", keep)
    assert [w[0] for w in words] == [0] * 7 and [w[0] for w in sync] == [0] * 7, (what, words)          # first passes never
    assert [w[1] for w in sync] == CUT_WIDE["synchronised"], sync
    assert words != sync, "%s: the host decided as in the synchronised run: %r" % (what, words)
    if gate_at == 3:
        assert words[4][1] == 1 and sync[4][1] == 0, (what, words)
    assert [w[1] for w in words] == CUT_WIDE[gate_at], (what, words)


@HZB_MODES
@KEEPS
@pytest.mark.parametrize("name,gate_at", [("sky", 0), ("sky", 2), ("masked_floor", 0), ("masked_floor", 2)])
def test_sky_and_floor_under_reports_of_every_age(gpu, name, gate_at, keep, hzb):
    """sky: an empty second pass and the street's long one behind it, enqueued under the light report of frame 1 (or none);
    masked_floor: the clip triangles of an alpha-tested floor through a second pass set up under a stale report."""
    what = "%s, gate at %d, keep %r, hzb %s" % (name, gate_at, keep, hzb)
    sc = F.wide_sequence(name)
    words, _ = _run_frames(sc, keep, gate_at, what, hzb=hzb)
    if gate_at == 0:
        assert all(w == [0, 0] for w in words), (what, words)                 # 'none yet': never the direct form
        assert any(w[1] for w in _synchronised_words(name, keep)), what
    else:
        assert all(w[1] == 1 for w in words[gate_at:]), (what, words)         # the light report of frame 1 holds to the end


@pytest.mark.parametrize("order", ["dense_then_sparse", "sparse_then_dense"])
def test_stale_density_reports(gpu, order):
    """sparse_then_dense: the host holds an empty view's report (0 clusters: no block kernel) and enqueues hotspot frames -- the
    record kernel sets up a dense list by itself -- an empty one and the hotspot twice.  dense_then_sparse: it holds the hotspot's
    (dense) and enqueues the block kernel onto empty lists, then the hotspot (no bin of this scene is long enough for a hot-tile
    report: test_hot_variant_under_a_stale_hot_tile_report).
    That the host decided from the stale report shows in the last frame's counters, the hotspot in both orders: without the block
    kernel every triangle is a record and no pixel block is written; with it blocks are written and fewer records.  A run that
    synchronises after every frame does the opposite in that frame (it follows a dense frame in the first order, an empty one in the
    second)."""
    sc = F.hotspot(order)
    n = len(sc.frames)
    want = sc.frames[-1].want
    probe = F.Context(sc)
    capacity = probe.r.last_frame_cmds().capacity
    probe.close()
    assert capacity * 16 >= sc.w * sc.h, "launch_raster never considers the block kernel for this scene at this size"
    _, st = _run_frames(sc, None, F.HOTSPOT_GATE[order], "hotspot " + order, hzb=None)
    _, st_sync = _run_frames(sc, None, n, "hotspot %s synchronised" % order, hzb=None)
    for stats, blocks in ((st, order == "dense_then_sparse"), (st_sync, order == "sparse_then_dense")):
        if blocks:
            assert stats["pixelBlockBytes"] > 0 and stats["triangleRecords"] < want["stats"].trianglesRastered, (order, stats)
        else:
            assert stats["pixelBlockBytes"] == 0 and stats["triangleRecords"] == want["stats"].trianglesRastered, (order, stats)


def test_hot_variant_under_a_stale_hot_tile_report(gpu):
    """The block kernel's hot variant (raster_setup_blocks_kernel<true>) is launched when the longest bin of the last report holds
    SLOT_HOT entries, and draws bin slots ahead for the tiles of the device-side hot list, which the tile schedule of the frame
    before wrote.  The scene (inflight.HOTSPOT_SCENES) puts more than 65 536 clusters into one tile, so its block-form frames report
    a hot tile by themselves: frame 0 (no report yet) runs the plain variant, frame 1, synchronised, the hot one -- more pixel
    blocks than frame 0's, the unused remainders of the slots drawn ahead (test_config5_hotspot_quarter_size_4k_matches_oracle's
    sign).  Behind the gate the host holds that report -- dense, hot -- for two empty frames and two hotspot frames: the hot variant
    runs on empty lists, then on the hotspot with the hot list the EMPTY frame before it left (none), then with the list of the
    hotspot frame before it -- the host's decision and the device's list come from reports of different ages.  Every image and list
    against the oracle; the last frame's pixel blocks above the plain variant's show that the hot variant ran there.
    (The un-gated dry run may see the empty frames' report, elide the block kernel and send the hotspot through the record form,
    which this scene overflows -- detected on the device, tests/test_gpu_bin_limits.py --: its results are not looked at.)"""
    order = "hot_then_sparse"
    sc = F.hotspot(order)
    n, gate_at = len(sc.frames), F.HOTSPOT_GATE[order]
    what = "hotspot " + order

    def prepare():
        ctx = F.Context(sc)
        ctx.blocks = []
        for k in range(gate_at):
            F.run_calls(ctx.frame_calls(k, hzb=False))
            ctx.synchronize()
            st = ctx.r.stats()
            assert st["overflow"] == 0, (what, k)
            ctx.blocks.append(st["pixelBlocks"])
        return ctx

    ctx, log, _ = F.run_behind_gate(prepare, lambda ctx: [e for k in range(gate_at, n) for e in _frame_entries(ctx, k, False)], what)
    for k, f in enumerate(sc.frames):
        F.check_frame(ctx.snaps[k], f.want, "%s, frame %d" % (what, k), hzb=False)
    F.check_stats(ctx, sc.frames[-1].want, what, counts=False)
    plain, hot = ctx.blocks
    assert plain > 65536, "frame 0 wrote %d pixel blocks: no bin of it can have reported a hot tile" % plain
    assert hot > plain, "frame 1 did not run the hot variant: the report of frame 0 names no hot tile (%d, %d)" % (plain, hot)
    last = ctx.r.stats()["pixelBlocks"]
    assert last > plain, "the last frame did not run the hot variant behind the gate (%d, %d)" % (plain, last)
    ctx.close()
    _observe(log, what)


@pytest.mark.parametrize("gate_at", [0, 9])
def test_many_frames_enqueued_ahead(gpu, gate_at):
    """Two dozen frames behind one gate, as a benchmark loop enqueues them: the history slots, the kept schedules' two buffers and
    the pending chain tails alternate many times with nothing finished in between -- from a context that has never finished a frame
    (gate at 0) and from one in its steady state (gate at 9).  The chain is snapshotted after the last frame only."""
    sc = F.moving("small", 24)
    _run_frames(sc, None, gate_at, "24 frames, gate at %d" % gate_at, hzb="last")


# ------------------------------------------------------------------------------------------------ C: caller state in flight --

def _moving_context(kind="small", frames_before=0, **kw):
    sc = F.moving(kind)

    def prepare():
        ctx = F.Context(sc, **kw)
        for k in range(frames_before):
            F.run_calls(ctx.frame_calls(k))
            ctx.synchronize()
        return ctx
    return sc, prepare


def _check_all(ctx, sc, what, frames=None, hzb=True):
    for k in (range(len(sc.frames)) if frames is None else frames):
        F.check_frame(ctx.snaps[k], sc.frames[k].want, "%s, frame %d" % (what, k), hzb=hzb, counts=k > 0)


@pytest.mark.parametrize("kind,temporary", [("small", False), ("small", True), ("street_x64", False)],
                         ids=["overwritten", "temporary", "overwritten_5MB"])
def test_host_buffer_is_the_callers_again_when_update_objects_returns(gpu, kind, temporary):
    """chordvis_update_objects from a numpy buffer that is overwritten with the NEXT pose's objects as soon as the call returns -- or
    from a temporary that is dropped there, its memory taken at once by arrays holding the next pose (renderer.update_objects'
    np.ascontiguousarray makes such temporaries): frame k must show pose k.  overwritten_5MB: BASELINE config 4's scene (22 528
    objects, 5 MB of records, at 640 x 360) -- the HIP runtime moves a pageable array of that size otherwise than a small one, and a
    benchmark loop hands one over every frame.  (No temporary at that size: its pages go back to the system, and reading them late
    would be a host fault, not a mismatch.)"""
    from chord_amd import lib as L
    sc = F.moving(kind) if kind == "small" else F.moving(kind, 3, 640, 360)
    prepare = lambda: F.Context(sc)
    n = len(sc.frames)
    what = "update_objects, %s, host buffer %s" % (kind, "dropped" if temporary else "overwritten")
    update_name = "update_objects" if kind == "small" else "update_objects_5MB"

    def script(ctx):
        buf = np.zeros_like(sc.frames[0].objs)
        ctx.keep_alive = []
        calls = []
        for k in range(n):
            def update(k=k):
                cur, nxt = sc.frames[k].objs, sc.frames[(k + 1) % n].objs
                if temporary:
                    tmp = cur.copy()
                    rc = L.lib.chordvis_update_objects(ctx.r._ctx, tmp.ctypes.data, len(tmp))
                    del tmp
                    ctx.keep_alive.append([nxt.copy() for _ in range(8)])    # (the allocator hands the freed block out again)
                else:
                    buf[...] = cur
                    rc = L.lib.chordvis_update_objects(ctx.r._ctx, buf.ctypes.data, len(buf))
                    buf[...] = nxt
                assert rc == 0
            entries = _frame_entries(ctx, k)
            calls += [_entry("%s[%d]" % (update_name, k), update)] + entries[1:]
        return calls

    ctx, log, _ = F.run_behind_gate(prepare, script, what)
    _check_all(ctx, sc, what)
    F.check_stats(ctx, sc.frames[-1].want, what)
    ctx.close()
    _observe(log, what)


# bytes -> whether hipMemcpyAsync from pageable host memory waited for the stream (measured on an MI355X, HIP 7.0)
PAGEABLE_COPY_WAITS = {4 << 10: False, 78848: False, 256 << 10: False, 1 << 20: False,
                       2 << 20: True, 4 << 20: True, 5046272: True, 16 << 20: True}
PAGEABLE_COPY_SIZES = [4 << 10, 78848, 256 << 10, 1 << 20, 2 << 20, 4 << 20, 5046272, 16 << 20]


def test_pageable_copies_of_every_size_read_the_host_array_before_they_return(gpu):
    """What chordvis_update_objects promises about hostObjects is a property of the HIP runtime's hipMemcpyAsync from pageable
    memory, which the scenes above hold at two sizes (352 objects, 22 528 objects).  Here the same call -- pageable numpy array to
    device memory, on a caller's stream behind the gate -- at sizes from 4 KB to 16 MB, the two scenes' among them: the array is
    overwritten with other bytes as soon as the call returns, and the device must hold the bytes of before.  Which sizes wait for
    the stream is recorded in PAGEABLE_COPY_WAITS and asserted both ways."""
    import ctypes as C
    import torch
    from chord_amd import lib as L
    hip = L._preload_hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    rng = np.random.default_rng(5)
    first = {n: rng.integers(0, 256, n, dtype=np.uint8) for n in PAGEABLE_COPY_SIZES}
    with torch.cuda.stream(stream):
        dst = {n: torch.zeros(n, dtype=torch.uint8, device=dev) for n in PAGEABLE_COPY_SIZES}
    stream.synchronize()
    bufs = {n: np.empty(n, dtype=np.uint8) for n in PAGEABLE_COPY_SIZES}

    def copy(n):
        bufs[n][...] = first[n]
        assert hip.hipMemcpyAsync(dst[n].data_ptr(), bufs[n].ctypes.data, n, 1, stream.cuda_stream) == 0
        bufs[n][...] = ~first[n]                                             # (every byte another one)

    calls = [("pageable_copy[%d]" % n, lambda n=n: copy(n), True) for n in PAGEABLE_COPY_SIZES]
    t0 = time.perf_counter()
    F.run_calls(calls)                                                        # the dry run: un-gated, and the process's one-time costs
    dry = time.perf_counter() - t0
    stream.synchronize()
    for n in PAGEABLE_COPY_SIZES:
        assert np.array_equal(dst[n].cpu().numpy(), first[n]), "un-gated, %d bytes: the device holds bytes written after the call returned" % n
        dst[n].zero_()
    torch.cuda.synchronize()
    assert F.GATE_FACTOR * dry <= F.GATE_CEILING_S, dry
    log = F.enqueue(stream, max(F.GATE_FLOOR_S, F.GATE_FACTOR * dry), calls, "pageable copies")
    stream.synchronize()
    print("dry run of pageable copies: %.1f ms host time for %d calls" % (dry * 1e3, len(calls)))
    for n in PAGEABLE_COPY_SIZES:
        assert np.array_equal(dst[n].cpu().numpy(), first[n]), "%d bytes: the device holds bytes written after the call returned" % n
    observed = {int(name.split("[")[1][:-1]): waited for name, waited in log}
    print("pageable copies that waited:", observed)
    assert observed == PAGEABLE_COPY_WAITS, observed


def _pass_by_pass_entries(ctx, k, state):
    """The frame recorded pass by pass (test_individual_passes_compose_to_the_frame), the caller carrying the history handle."""
    r = ctx.r

    def cull():
        state["post"] = r.instance_culling()

    def stage0():
        state["stage1"], state["rejected"] = r.visibility_stage0(state.get("hist"), state["post"])
        assert state["stage1"] == (state.get("hist") is not None)

    def mid_hzb():
        if state["stage1"]:
            state["tmp"] = r.build_hzb(True, False, False, slot=0)

    def stage1():
        if state["stage1"]:
            r.visibility_stage1(state["tmp"], state["rejected"])

    def final_hzb():
        state["hist"] = r.build_hzb(True, True, True, slot=1 + (k & 1))

    def snapshot():
        s = ctx.snapshot(hzb=False, cmd=state["post"])
        s.update(ctx.snapshot_hzb(state["hist"]))
        ctx.snaps[k] = s

    return [_entry("clear_gbuffer[%d]" % k, r.clear_gbuffer), _entry("instance_culling[%d]" % k, cull),
            _entry("visibility_stage0[%d]" % k, stage0), _entry("build_hzb[%d]" % k, mid_hzb),
            _entry("visibility_stage1[%d]" % k, stage1), _entry("build_hzb[%d]" % k, final_hzb), _entry("snapshot[%d]" % k, snapshot)]


def _check_pass_by_pass(s, want, what):
    H.assert_vis_equal(F.host(s["vis"], np.uint64), want["vis"], s["w"], s["h"], what)
    n, cmds = F.list_of(s)
    assert n == len(want["cmds"]) and np.array_equal(H.sort_cmds(cmds), H.sort_cmds(want["cmds"])), what + ": culled list"
    d = want["desc"]
    for got, ref in ((F.host(s["hzb_min"], np.uint16), want["hzb_min"]), (F.host(s["hzb_max"], np.uint16), want["hzb_max"])):
        for lv, (a, b) in enumerate(zip(H.hzb_levels(d, got), H.hzb_levels(d, ref.view(np.uint16)))):
            assert np.array_equal(a, b), "%s: HZB level %d" % (what, lv)         # (only the sampled extent of a level is defined)
    assert np.array_equal(F.host(s["valid_range"], np.uint32), want["valid_range"].view(np.uint32)), what + ": valid range"


@pytest.mark.parametrize("republish", [False, True], ids=["view_as_kernel_argument", "view_through_flush_view"])
def test_set_view_twice_around_pass_by_pass_frames(gpu, republish):
    """Every pass-by-pass frame is followed AT ONCE by the next frame's update_objects and set_view and its passes, all behind one
    gate, and must still be rendered with its own view.  How the view reaches the device:
      view_as_kernel_argument   chordvis_instance_culling hands the host record to the cull kernel by value (launch_group_cull), the
                                kernel publishes it for the later passes and the record is clean: no copy is made at all;
      view_through_flush_view   the caller sets the view AGAIN -- the same valid view -- between instance_culling and
                                visibility_stage0, so the record is dirty when stage 0's first pass (chordvis_hzb_culling, or
                                chordvis_render_mesh in the frame without history) calls flush_view: a hipMemcpyAsync from the
                                context's own pageable record c->hView, which the next frame's set_view overwrites a few
                                microseconds later, with the copy still behind the gate.  Were the record read when the copy
                                runs and not when it is enqueued, stage 0 and all behind it would run under the NEXT frame's view."""
    sc, prepare = _moving_context("small")
    what = "pass-by-pass frames, " + ("the view set again before stage 0" if republish else "one set_view per frame")

    def script(ctx):
        state, calls = {}, []
        for k in range(len(sc.frames)):
            head, passes = _frame_entries(ctx, k)[:2], _pass_by_pass_entries(ctx, k, state)
            if republish:
                again = _entry("set_view[%d again]" % k, head[1][1])
                passes = passes[:2] + [again] + passes[2:]                   # clear, instance_culling | set_view | stage 0 ...
                assert F.kind_of(passes[1][0]) == "instance_culling" and F.kind_of(passes[3][0]) == "visibility_stage0"
            calls += head + passes
        return calls

    ctx, log, _ = F.run_behind_gate(prepare, script, what)
    for k, f in enumerate(sc.frames):
        _check_pass_by_pass(ctx.snaps[k], f.want, "%s, frame %d" % (what, k))
    assert ctx.r.stats()["overflow"] == 0
    ctx.close()
    _observe(log, what)


def _pinned_objects(sc):
    import torch
    return [torch.from_numpy(f.objs.view(np.uint8).reshape(-1).copy()).pin_memory() for f in sc.frames]


def test_bound_objects_rewritten_on_the_stream(gpu):
    """chordvis_bind_objects of a torch tensor the caller rewrites between frames with copy_(pinned, non_blocking=True) on the
    context's stream -- 'ordered behind the context's stream', include/chordvis.h --: each frame sees its own objects."""
    import torch
    sc, prepare = _moving_context("small")
    what = "bound objects"

    def script(ctx):
        pinned = _pinned_objects(sc)
        with torch.cuda.stream(ctx.stream):
            ctx.objects = torch.zeros(pinned[0].numel(), dtype=torch.uint8, device=torch.device("cuda", ctx.device))
        calls = []
        for k in range(len(sc.frames)):
            def copy(k=k):
                with torch.cuda.stream(ctx.stream):
                    ctx.objects.copy_(pinned[k], non_blocking=True)
            calls.append(_entry("caller_copy[%d]" % k, copy))
            if k == 0:
                calls.append(_entry("bind_objects", lambda: ctx.r.bind_objects(ctx.objects.data_ptr(), len(sc.frames[0].objs))))
            calls += _frame_entries(ctx, k)[1:]
        ctx.pinned = pinned
        return calls

    ctx, log, _ = F.run_behind_gate(prepare, script, what)
    _check_all(ctx, sc, what)
    F.check_stats(ctx, sc.frames[-1].want, what)
    ctx.close()
    _observe(log, what)


def test_caller_owned_image_zeroed_rendered_and_cloned_in_flight(gpu):
    """The caller zeroes its image on the stream, renders, clones, zeroes and renders again: the clones hold their own frames."""
    import torch
    sc, prepare = _moving_context("masked")
    what = "caller-owned image"

    def script(ctx):
        def zero():
            with torch.cuda.stream(ctx.stream):
                ctx.vis.zero_()
        calls = []
        for k in range(len(sc.frames)):
            calls += [_entry("caller_zero[%d]" % k, zero)] + _frame_entries(ctx, k)
        return calls

    ctx, log, _ = F.run_behind_gate(prepare, script, what)
    _check_all(ctx, sc, what)
    F.check_stats(ctx, sc.frames[-1].want, what)
    ctx.close()
    _observe(log, what)


def test_resolves_between_frames_in_flight(gpu):
    """Frame A, resolve_attributes and resolve_gbuffer into caller tensors, update_objects(B) + set_view(B), frame B, the resolves
    again -- one gate.  Both sets equal the numpy specs (spec_resolve_np, spec_gbuffer_np's packing) for their own frame."""
    import torch
    import spec_gbuffer_np as SG
    import spec_resolve_np as SR
    import test_gpu_gbuffer as GB
    import test_gpu_resolve as TR
    from chord_amd import lib as L
    sc = F.moving("masked_attributes")
    what = "resolves in flight"
    pair = (1, 2)

    def prepare():
        ctx = F.Context(sc)
        ctx.r.upload_material_textures()
        ctx.resolved = {}
        F.run_calls(ctx.frame_calls(0))
        ctx.synchronize()
        return ctx

    def script(ctx):
        dev = torch.device("cuda", ctx.device)
        calls = []
        for k in pair:
            with torch.cuda.stream(ctx.stream):
                attrs = {n: torch.zeros((sc.h, sc.w) if ch == 1 else (sc.h, sc.w, ch), dtype=torch.int32 if n == "debugRGBA8" else torch.float32,
                                        device=dev) for n, ch in L.RESOLVE_CHANNELS.items()}
                packed = ctx.r._gbuffer_images(None, None, sc.w, sc.h, "test")
                for t in packed.values():
                    t.zero_()
            ctx.resolved[k] = (attrs, packed)

            def resolve_attributes(attrs=attrs):
                with torch.cuda.stream(ctx.stream):
                    ctx.r.resolve_attributes(out=attrs)

            def resolve_gbuffer(packed=packed):
                with torch.cuda.stream(ctx.stream):
                    ctx.r.resolve_gbuffer(out=packed)
            calls += _frame_entries(ctx, k) + [_entry("resolve_attributes[%d]" % k, resolve_attributes),
                                               _entry("resolve_gbuffer[%d]" % k, resolve_gbuffer)]
        return calls

    ctx, log, _ = F.run_behind_gate(prepare, script, what)
    _check_all(ctx, sc, what, frames=(0,) + pair)
    for k in pair:
        f = sc.frames[k]
        scene = sc.scene.with_objects(f.objs)
        attrs, packed = ctx.resolved[k]
        want = SR.resolve(scene, f.want["vis"], f.want["cmds"], f.view, f.iv, sc.w, sc.h, names=SR.NAMES)
        TR._assert_same({n: t.cpu().numpy().view(np.uint32) for n, t in attrs.items()}, want, "%s, frame %d" % (what, k))
        want_packed, written, _ = GB._spec(scene, f.want["vis"], f.want["cmds"], f.view, f.iv, sc.w, sc.h)
        GB._same({n: SG.words_of(t.cpu().numpy()) for n, t in packed.items()}, want_packed, "%s, frame %d" % (what, k))
        assert written["baseColor"].any() and written["vertexNormal"].any()
    a, b = (ctx.resolved[k][0]["positionRS"].cpu().numpy() for k in pair)
    assert not np.array_equal(a, b), "the two frames resolve to the same positions: the comparison shows nothing"
    ctx.close()
    _observe(log, what)


CHANGES = ["upload_history_hzb", "reset_history", "allocate_gbuffer", "upload_scene", "upload_material_textures"]


@pytest.mark.parametrize("change", CHANGES)
def test_state_changes_with_unfinished_frames_in_front(gpu, change):
    """Frames 0 and 1 sit behind the gate with their snapshots when the state change is called; it may wait (WAITS says which do).
    The snapshots taken before it are exact, and the frame after it is the oracle's for the new state:
      upload_history_hzb       frame 2 against frame 0's chain (its stage counts differ from those against frame 1's)
      reset_history            frame 2 without history (no second pass)
      allocate_gbuffer         a frame of another size, then back: frame 2 without history
      upload_scene             the other scene's frame 0
      upload_material_textures frame 2 as it would have been (the raster reads nothing of the material store)"""
    import orc
    sc = F.moving("masked_attributes" if change == "upload_material_textures" else "small")
    other, small = F.moving("masked"), F.moving("small", 2, 256, 160)
    what = "state change " + change
    f2 = sc.frames[2]
    scene2 = sc.scene.with_objects(f2.objs)

    def prepare():
        ctx = F.Context(sc)
        return ctx

    def frame_of(ctx, f, key, flags, hzb=True):
        """update_objects -> set_view -> render_frame -> snapshot of a Frame that need not be the context's scenario's"""
        return [_entry("update_objects[%s]" % key, lambda: ctx.r.update_objects(f.objs)),
                _entry("set_view[%s]" % key, lambda: ctx.r.set_view(f.view, f.iv, flags)),
                _entry("render_frame[%s]" % key, ctx.render_frame),
                _entry("snapshot[%s]" % key, lambda: ctx.snaps.__setitem__(key, ctx.snapshot(hzb=hzb)))]

    def script(ctx):
        calls = _frame_entries(ctx, 0) + _frame_entries(ctx, 1)
        if change == "upload_history_hzb":
            calls.append(_entry(change, lambda: ctx.r.upload_history_hzb(sc.frames[0].want["hzb_min"])))
        elif change == "reset_history":
            calls.append(_entry(change, ctx.r.reset_history))
        elif change == "allocate_gbuffer":
            calls.append(_entry("allocate_gbuffer[to %dx%d]" % (small.w, small.h), lambda: ctx.attach(small.w, small.h)))
            calls += frame_of(ctx, small.frames[0], "small", small.flags)
            calls.append(_entry("allocate_gbuffer[back]", lambda: ctx.attach(sc.w, sc.h)))
        elif change == "upload_scene":
            calls.append(_entry(change, lambda: ctx.r.upload_scene(other.scene)))
            return calls + frame_of(ctx, other.frames[0], "other", other.flags)
        elif change == "upload_material_textures":
            calls.append(_entry(change, ctx.r.upload_material_textures))
        return calls + frame_of(ctx, f2, 2, sc.flags)

    ctx, log, _ = F.run_behind_gate(prepare, script, what)
    _check_all(ctx, sc, what, frames=(0, 1))
    if change == "upload_scene":
        F.check_frame(ctx.snaps["other"], other.frames[0].want, what + ", the other scene's frame")
        F.check_stats(ctx, other.frames[0].want, what, counts=False)
    else:
        prev = {"upload_history_hzb": sc.frames[0].want["hzb_min"], "upload_material_textures": sc.frames[1].want["hzb_min"]}.get(change)
        want = f2.want if change == "upload_material_textures" else orc.frame(scene2, f2.view, f2.iv, sc.flags, prev_hzb_min=prev)
        if change == "allocate_gbuffer":
            F.check_frame(ctx.snaps["small"], small.frames[0].want, what + ", the frame of another size")
        F.check_frame(ctx.snaps[2], want, what + ", the frame after it", counts=prev is not None)
        F.check_stats(ctx, want, what, counts=prev is not None)
    ctx.close()
    _observe(log, what)
    assert F.waits(log)[F.kind_of(change)] == WAITS[change]


def test_three_frames_on_the_legacy_stream_handle(gpu):
    """chordvis_create(0, (void*)1, ...): hipStreamLegacy 'goes through' (include/chordvis.h); the caller's own work -- the gate,
    the snapshots -- is on torch's default stream, the same queue."""
    sc = F.moving("small")
    what = "hipStreamLegacy"

    def prepare():
        ctx = F.Context(sc, handle=1)
        return ctx

    ctx, log, _ = F.run_behind_gate(prepare, lambda ctx: [e for k in range(3) for e in _frame_entries(ctx, k)], what)
    assert ctx.r.stream() == 1
    _check_all(ctx, sc, what, frames=range(3))
    F.check_stats(ctx, sc.frames[2].want, what)
    ctx.close()
    _observe(log, what)


def test_close_with_frames_in_flight(gpu):
    """chordvis_destroy synchronises the stream before it frees anything: frames still behind the gate run to their end on memory
    that is still theirs, the snapshots cloned before the close are exact, and the device is clean afterwards."""
    import torch
    sc, prepare = _moving_context("small")
    what = "close() in flight"
    ctx, log, _ = F.run_behind_gate(prepare, lambda ctx: [e for k in range(3) for e in _frame_entries(ctx, k)] + [_entry("close", ctx.close)], what)
    torch.cuda.synchronize()
    _check_all(ctx, sc, what, frames=range(3))
    _observe(log, what)
    assert F.waits(log)["close"] is True


def test_the_gate_exposes_a_write_that_is_not_ordered(gpu):
    """The harness's own sensitivity proof.  Pose A is in an array bound with bind_objects and frame A sits behind the gate when the
    test -- a caller's error, made on purpose; both states are valid -- copies pose B into the array from a side stream.  The
    snapshot of frame A must then NOT be the oracle's frame A, and must be exactly the oracle's image for (objects B, view A): the
    gate really holds the frame back until the last call has returned.  If it did not, the other tests would prove nothing."""
    import torch
    sc, _ = _moving_context("small")
    what = "misordered write"
    pinned = _pinned_objects(sc)

    def prepare():
        ctx = F.Context(sc)
        with torch.cuda.stream(ctx.stream):
            ctx.objects = torch.zeros(pinned[0].numel(), dtype=torch.uint8, device=torch.device("cuda", ctx.device))
            ctx.objects.copy_(pinned[0], non_blocking=True)
        ctx.r.bind_objects(ctx.objects.data_ptr(), len(sc.frames[0].objs))
        ctx.r.set_view(sc.frames[0].view, sc.frames[0].iv, sc.flags)
        ctx.synchronize()
        return ctx

    def script(ctx):
        side = torch.cuda.Stream(device=torch.device("cuda", ctx.device))

        def misordered():
            with torch.cuda.stream(side):
                ctx.objects.copy_(pinned[1], non_blocking=True)
            side.synchronize()                                              # (the side stream's copy alone: the gate stays closed)
        return [_entry("render_frame[0]", ctx.render_frame),
                _entry("snapshot[0]", lambda: ctx.snaps.__setitem__(0, ctx.snapshot(hzb=False))),
                _entry("side_stream_copy", misordered)]

    ctx, log, _ = F.run_behind_gate(prepare, script, what)
    got = F.host(ctx.snaps[0]["vis"], np.uint64)
    assert not np.array_equal(got, sc.frames[0].want["vis"]), "frame A shows pose A: the gate did not hold it back behind the write"
    F.check_frame(ctx.snaps[0], F.crossed(sc, 1, 0), what + ": (objects B, view A)", hzb=False)
    ctx.close()
    _observe(log, what)


# -------------------------------------------------------------------------------------------------------- D: depth views --

def test_render_shadow_ticks_between_main_frames_in_flight(gpu):
    """The cascade scene of test_render_shadow_with_cascade_cache_matches_the_replay at dim 256: main frame, render_shadow tick 0
    (every cascade), main frame, tick 1 (the far cascades but one come from the cache) behind one gate, every cascade's image
    snapshotted per tick: the values of that test's oracle replay, and the main frames the oracle's."""
    import test_depth_views as DV
    from chord_amd import lib as L
    from chord_amd import records as R
    from chord_amd import scenes
    scene, cam = scenes.masked_test_scene(320, 200)
    cfg = R.default_cascade_config(cascadeCount=5, realtimeCascadeCount=2, cascadeDim=256, cascadeEndDistance=12.0, farCascadeEndDistance=60.0,
                                   shadowBiasConst=-8.0, shadowBiasSlope=-0.5)
    objs = L.fill_objects(scene, cam).copy()
    view, iv = L.make_views(cam)
    sc = F._chain("cascades", scene, 320, 200, H.ALL_FLAGS, [(view, iv, objs)] * 2)
    what = "render_shadow in flight"

    def prepare():
        ctx = F.Context(sc)
        ctx.r.allocate_depth_views(256, 5)
        ctx.ticks = {}
        ctx.synchronize()
        return ctx

    def script(ctx):
        calls = []
        for tick in range(2):
            def shadow(tick=tick):
                depths, views, mask = ctx.r.render_shadow(cfg, DV.LIGHT, tick)
                ctx.ticks[tick] = ([ctx.snapshot_depth(d) for d in depths], views, mask)
            calls += _frame_entries(ctx, tick) + [_entry("render_shadow[%d]" % tick, shadow)]
        return calls

    ctx, log, _ = F.run_behind_gate(prepare, script, what)
    _check_all(ctx, sc, what)
    hist = None
    for tick in range(2):
        hist, want_mask = DV._replay_shadow(scene.with_objects(objs), view, iv, cfg, tick, hist, H.ALL_FLAGS)
        depths, views, mask = ctx.ticks[tick]
        assert mask == want_mask == (0b11111 if tick == 0 else 0b01011), (tick, bin(mask), bin(want_mask))
        assert np.array_equal(views.view(np.uint8), hist["views"].view(np.uint8)), "tick %d: cascade views" % tick
        for k in range(5):
            assert np.array_equal(F.host(depths[k], np.uint32), hist["depths"][k].view(np.uint32)), "tick %d cascade %d" % (tick, k)
    assert ctx.r.depth_view_stats()["overflow"] == 0
    F.check_stats(ctx, sc.frames[1].want, what)
    ctx.close()
    _observe(log, what)
