"""Frames enqueued ahead of the device on a caller-owned stream: the harness of tests/test_gpu_frames_in_flight.py and the
scenario builders it shares with tests/test_frames_in_flight_spec.py.  A plain helper module: no fixture, no pytest setting.

THE GATE.  Gate(stream, seconds) enqueues torch.cuda._sleep -- a kernel that spins for a number of device clock ticks, calibrated
once per process against two events -- and an event behind it.  While the event has not completed, nothing enqueued behind the
gate on that stream has started: a host call that returns with the gate still closed was enqueued ahead of the device, and a
call that returns with the gate open has waited for the stream (or for the device).  The gate is a bounded spin on the device
and is never waited for on the host, so nothing can hang on it.  Its length is measured: run_behind_gate runs the same calls
un-gated on a throw-away context first (which also pays one-time process costs such as code-object loading), takes their host
time with time.perf_counter and closes the gate for four times that, at least 20 ms.  A dry run whose fourfold exceeds 1 s is
taken once more (the first carried the one-time costs); if it still does, the scenario is too long and the harness says so.

ENQUEUE.  enqueue() runs (name, callable, may_wait) entries behind a gate.  An entry with may_wait False that returns with the
gate open, when it was closed before, fails the test under its name.  An entry with may_wait True may open the gate; the harness
notes that it waited and closes a new gate before the next entry, so that what follows is again ahead of the device.  After the
last entry the gate must still be closed -- or the last entry was a may_wait one entered with the gate closed (close() at the end of
a scenario: everything before it was enqueued ahead of the device, and waiting is its contract).  Only then is the stream
synchronised and are the snapshots read.

SNAPSHOTS are stream-ordered device copies, never read-backs: the visibility image is a caller-owned int64 tensor handed to
allocate_gbuffer(device_visibility=...) and cloned under torch.cuda.stream(stream); the library's own arrays -- count / cmds of
last_frame_cmds(), minTexels / maxTexels / validRange of history_hzb(), a ChordDepthTarget's image -- are wrapped by an object
with __cuda_array_interface__ (typestr <i4 / <i2), made a tensor with torch.as_tensor(obj, device=...) and cloned the same way;
the host reinterprets the words after the final synchronise.  MECHANISM IN USE: the interface (torch 2.10 for ROCm accepts it for
raw hipMalloc pointers); the prefix-run fallback is not needed and not implemented.
history_hzb() launches the tail of the chain (levels 6.. and the valid range) that otherwise rides on the next frame's first
kernel, so a scenario that snapshots the chain every frame tests that launch in flight and one that snapshots it after the last
frame only tests the riding tail in flight; Context.snapshot(hzb=...) chooses."""
import ctypes
import functools
import time

import numpy as np

import helpers as H

GATE_FLOOR_S = 0.020
GATE_CEILING_S = 1.0
GATE_FACTOR = 4.0


# ------------------------------------------------------------------------------------------------------------- scenarios --

class Frame:
    """One frame's inputs and the oracle's result for them (want: orc.frame's dict, chained through prev_hzb_min)."""

    def __init__(self, view, iv, objs, want):
        self.view, self.iv, self.objs, self.want = view, iv, objs, want


class Scenario:
    def __init__(self, name, scene, w, h, flags, frames, limits=None):
        self.name, self.scene, self.w, self.h, self.flags, self.frames, self.limits = name, scene, w, h, flags, frames, limits


def _chain(name, scene, w, h, flags, inputs, limits=None):
    """Scenario of [(view, iv, objs)]: every frame's oracle result against the oracle's chain of the frame before."""
    import orc
    frames, prev = [], None
    for view, iv, objs in inputs:
        want = orc.frame(scene.with_objects(objs), view, iv, flags, prev_hzb_min=prev)
        frames.append(Frame(view, iv, objs, want))
        prev = want["hzb_min"]
    return Scenario(name, scene, w, h, flags, frames, limits)


@functools.lru_cache(maxsize=None)
def wide_sequence(name):
    """A sequence of tests/test_gpu_setup_wide.py (cut, sky, masked_floor, ...) at that file's size."""
    import test_gpu_setup_wide as SW
    scene, cam0 = SW._scene(name)
    inputs = [SW._frame_inputs(scene, cam, last_cam, last) for cam, last_cam, last in SW.sequence(name, scene, cam0)]
    return _chain(name, scene, cam0.width, cam0.height, H.ALL_FLAGS, inputs)


HOTSPOT_LIMITS = dict(max_triangle_records=8 << 20, bin_pool_chunks=16384, bin_max_chunks_per_tile=2048)
# a: the view that looks away, h: the hotspot
HOTSPOT_ORDERS = {"sparse_then_dense": "aahhahh", "dense_then_sparse": "hhaah", "hot_then_sparse": "hhaahh"}
HOTSPOT_GATE = {"sparse_then_dense": 2, "dense_then_sparse": 2, "hot_then_sparse": 2}
# hot_then_sparse: 81 920 clusters (10.5 M triangles) with sigma = 8 px round the middle of the tile in the middle of a 704 x 448 target:
# in block form -- an entry per cluster and tile -- that tile's bin is longer than SLOT_HOT (65 536), so a block-form frame reports a
# hot tile by itself.  The scene is for block-form frames only: one record per triangle is more than a tile's bin can hold under any
# limits (16 384 + 3 072 x 1 024 entries).
HOTSPOT_SCENES = {"hot_then_sparse": dict(w=704, h=448, instances=20, sigma=8.0,
                                          limits=dict(max_triangle_records=24 << 20, bin_pool_chunks=16384, bin_max_chunks_per_tile=2048))}


@functools.lru_cache(maxsize=None)
def hotspot(order):
    """The reduced config-5 hotspot scene of test_config5_hotspot_reduced_matches_oracle, under its limits and flags, seen from the
    hotspot camera ('h': a dense list) and from one that looks away ('a': an empty list).  At 640 x 360, not that test's 960 x 540:
    launch_raster considers the block kernel only where the list's capacity allows a cluster per 16 pixels, and the device takes
    the list for dense from a cluster per 16 pixels on -- the scene's 16 384 clusters are that many on 230 400 pixels and not on
    518 400, where neither a fresh nor a stale report could change a launch.  hot_then_sparse: HOTSPOT_SCENES."""
    import orc
    from chord_amd import lib as L
    from chord_amd import records as R
    from chord_amd import scenes
    spec = HOTSPOT_SCENES.get(order, dict(w=640, h=360, instances=4, sigma=64.0, limits=HOTSPOT_LIMITS))
    w, h = spec["w"], spec["h"]
    scene, hot = scenes.config5_subpixel(w, h, prims=16, patches_per_prim=256, instances=spec["instances"], hotspot_sigma_px=spec["sigma"])
    away = scenes.Camera((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), w, h)
    cams = [hot if ch == "h" else away for ch in HOTSPOT_ORDERS[order]]
    flags = R.FLAG_FRUSTUM_CULL | R.FLAG_CONE_CULL
    frames, memo = [], {}
    for i, cam in enumerate(cams):
        last = cams[i - 1] if i else cam
        view0, _ = L.make_views(last)
        view, iv = L.make_views(cam, view0)
        objs = L.fill_objects(scene, cam, last).copy()
        key = (view.tobytes(), iv.tobytes(), objs.tobytes())                  # (no HZB culling: a frame is a function of its inputs alone)
        if key not in memo:
            memo[key] = orc.frame(scene.with_objects(objs), view, iv, flags)
        frames.append(Frame(view, iv, objs, memo[key]))
    return Scenario("hotspot_" + order, scene, w, h, flags, frames, spec["limits"])


def _moving_scene(kind, w, h):
    from chord_amd import scenes
    if kind == "small":
        scene, cam0 = scenes.small_test_scene(w, h)
    elif kind == "street_x64":                                                # BASELINE config 4's scene: 22 528 objects, 5 MB of records
        scene, cam0 = scenes.config4_street_x64(w, h, grid=8)
    else:                                                                     # masked / masked_attributes (normals, tangents: the G-buffer resolve)
        scene, cam0 = scenes.masked_test_scene(w, h, attributes=(kind == "masked_attributes"))
    f = np.array(cam0.front, dtype=np.float64)
    f /= np.linalg.norm(f)
    static = scene.local_to_world.copy()
    scene.local_to_world_at = lambda k: static                             # (H.moving_sequence: the objects stand, the camera moves)
    return scene, cam0, f


@functools.lru_cache(maxsize=None)
def moving(kind, frames=4, w=320, h=200):
    """small_test_scene(w, h) / masked_test_scene(w, h) / config4_street_x64(w, h) under a camera that moves forward and upward and turns, through
    H.moving_sequence: every frame has object records (camera-relative transforms, this frame's and the last one's) and a view of
    its own."""
    scene, cam0, f = _moving_scene(kind, w, h)
    from chord_amd import scenes
    side = np.cross(f, np.array([0.0, 1.0, 0.0]))
    cams = [scenes.Camera(tuple(np.array(cam0.position) + 0.35 * k * f + np.array([0.0, 0.02 * k, 0.0])), tuple(f + 0.04 * k * side), w, h,
                          cam0.fovy, cam0.z_near, cam0.z_far, cam0.world_up) for k in range(frames)]                                           # (it turns too: the view record changes, not only the position)
    out = [Frame(view, iv, scene.objects.copy(), want) for _, view, iv, want in H.moving_sequence(scene, cams)]
    return Scenario("moving_%s_%dx%d" % (kind, w, h), scene, w, h, H.ALL_FLAGS, out)


def crossed(sc, k_objs, k_view, prev_hzb=None):
    """The oracle's frame for frame k_objs's object records under frame k_view's view: what a misordered write shows."""
    import orc
    f = sc.frames[k_view]
    return orc.frame(sc.scene.with_objects(sc.frames[k_objs].objs), f.view, f.iv, sc.flags, prev_hzb_min=prev_hzb)


# ------------------------------------------------------------------------------------------------------------------ gate --

@functools.lru_cache(maxsize=None)
def cycles_per_second(device=0):
    """Ticks of torch.cuda._sleep's clock per second: one fixed sleep between two events, once per process."""
    import torch
    with torch.cuda.device(device):
        torch.cuda._sleep(1000)                                               # (loads the kernel)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 20_000_000
        a.record()
        torch.cuda._sleep(n)
        b.record()
        b.synchronize()
        return n / (a.elapsed_time(b) * 1e-3)


class Gate:
    def __init__(self, stream, seconds):
        import torch
        self.seconds = seconds
        cycles = int(seconds * cycles_per_second(stream.device.index))
        with torch.cuda.stream(stream):
            torch.cuda._sleep(cycles)
            self.event = torch.cuda.Event()
            self.event.record(stream)

    def closed(self):
        return not self.event.query()


def enqueue(stream, seconds, calls, what=""):
    """Runs calls [(name, callable, may_wait)] behind a gate of `seconds` (see the module docstring); returns [(name, waited)]."""
    gate = Gate(stream, seconds)
    assert gate.closed(), "%s: the gate was open before the first call" % what
    log = []
    regate = False
    was_closed = True
    may_wait = False
    for name, fn, may_wait in calls:
        if regate:
            gate = Gate(stream, seconds)
            regate = False
        was_closed = gate.closed()
        assert was_closed, "%s: the gate ran out before %s: the calls before it were not all enqueued ahead of the device" % (what, name)
        fn()
        waited = not gate.closed()
        if waited and not may_wait:
            raise AssertionError("%s: %s returned with the gate open: it waited for the stream" % (what, name))
        log.append((name, waited))
        regate = waited
    assert gate.closed() or (may_wait and was_closed), "%s: the gate was open after the last call" % what
    return log


def kind_of(name):
    """'update_objects[3]' -> 'update_objects'"""
    return name.split("[")[0]


def waits(log):
    """{call kind: waited} of an enqueue log; a kind that waited in one place and not in another is an error of its own."""
    out = {}
    for name, waited in log:
        k = kind_of(name)
        assert out.setdefault(k, waited) == waited, "%s waited in one call and not in another: %r" % (k, log)
    return out


# --------------------------------------------------------------------------------------------------------------- context --

class _DeviceArray:
    def __init__(self, ptr, count, typestr):
        self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": typestr, "data": (int(ptr), False), "version": 2,
                                         "strides": None}


def device_view(ptr, count, typestr, device=0):
    """A tensor over `count` words of library-owned device memory at `ptr` (typestr '<i4' or '<i2'); no copy, no synchronise."""
    import torch
    return torch.as_tensor(_DeviceArray(ptr, count, typestr), device=torch.device("cuda", device))


class Context:
    """A VisibilityRenderer on a caller's stream with a caller-owned visibility image.  handle None: a torch.cuda.Stream of the
    test's own, handed over as its hipStream_t; handle 1: hipStreamLegacy, the caller working on torch's default stream."""

    def __init__(self, sc, device=0, handle=None, keep=None):
        self.sc, self.device = sc, device
        self.snaps = {}                                                        # {frame: snapshot}, filled by frame_calls
        self.r, self.stream = caller_stream_renderer(device, handle)
        if sc.limits:
            self.r.set_limits(**sc.limits)
        self.r.upload_scene(sc.scene)
        if keep is not None:
            self.r.set_tile_schedule_keep(keep)
        self.vis = None
        self.attach(sc.w, sc.h)
        self.words = []                                                        # chordvis_debug_setup_kernels after every render_frame
        self.synchronize()

    def attach(self, w, h):
        """A caller-owned image of w x h words becomes the context's target."""
        import torch
        old = self.vis                                                        # (kept until the library has let go of it)
        with torch.cuda.stream(self.stream):
            self.vis = torch.zeros(w * h, dtype=torch.int64, device=torch.device("cuda", self.device))
        self.r.allocate_gbuffer(w, h, device_visibility=self.vis.data_ptr())
        self.w, self.h = w, h
        del old

    def synchronize(self):
        self.stream.synchronize()

    def setup_words(self):
        from chord_amd import lib as L
        wide = (ctypes.c_uint32 * 2)()
        assert L.lib.chordvis_debug_setup_kernels(self.r._ctx, wide) == 0
        return [int(wide[0]), int(wide[1])]

    def render_frame(self):
        self.r.render_frame()
        self.words.append(self.setup_words())

    def snapshot(self, hzb=True, cmd=None):
        """Device copies, in stream order, of the image, the frame's list 0 (or `cmd`) with the four stage counts and -- hzb -- the
        history chain."""
        import torch
        s = {"w": self.w, "h": self.h}
        with torch.cuda.stream(self.stream):
            s["vis"] = self.vis.clone()
            if cmd is None:
                # the frame's list 0; its count word is the first of the context's eight list counts (FrameState::listCounts,
                # device_layer.h), of which [0..3] are what chordvis_stats reports as the four stage counts
                cmd = self.r.last_frame_cmds()
                s["counts"] = device_view(cmd.count, 4, "<i4", self.device).clone()
            s["count"] = device_view(cmd.count, 1, "<i4", self.device).clone()
            s["cmds"] = device_view(cmd.cmds, 3 * max(1, cmd.capacity), "<i4", self.device).clone()
            if hzb:
                s.update(self.snapshot_hzb(self.r.history_hzb()))
        return s

    def snapshot_hzb(self, hz):
        import torch
        n = hz.desc.totalTexels
        with torch.cuda.stream(self.stream):
            return {"hzb_min": device_view(hz.minTexels, n, "<i2", self.device).clone(),
                    "hzb_max": device_view(hz.maxTexels, n, "<i2", self.device).clone(),
                    "valid_range": device_view(hz.validRange, 2, "<i4", self.device).clone()}

    def snapshot_depth(self, target):
        import torch
        with torch.cuda.stream(self.stream):
            return device_view(target.depth, target.width * target.height, "<i4", self.device).clone()

    def frame_calls(self, k, hzb=True):
        """update_objects -> set_view -> render_frame -> snapshot of frame k, as enqueue() entries; the snapshot lands in self.snaps[k]."""
        f, sc, snaps = self.sc.frames[k], self.sc, self.snaps
        return [("update_objects[%d]" % k, lambda: self.r.update_objects(f.objs), False),
                ("set_view[%d]" % k, lambda: self.r.set_view(f.view, f.iv, sc.flags), False),
                ("render_frame[%d]" % k, self.render_frame, False),
                ("snapshot[%d]" % k, lambda: snaps.__setitem__(k, self.snapshot(hzb=hzb)), False)]

    def close(self):
        self.r.close()


def caller_stream_renderer(device=0, handle=None):
    """(VisibilityRenderer, torch stream): the renderer enqueues on a torch.cuda.Stream made here -- or, handle 1, on
    hipStreamLegacy, with torch's default stream (the same queue) for the caller's own work."""
    import torch
    from chord_amd.renderer import VisibilityRenderer
    dev = torch.device("cuda", device)
    if handle is None:
        stream = torch.cuda.Stream(device=dev)
        return VisibilityRenderer(device, stream=stream.cuda_stream), stream
    assert handle == 1, "caller_stream_renderer: handle None (a stream of its own) or 1 (hipStreamLegacy)"
    return VisibilityRenderer(device, stream=ctypes.c_void_p(1)), torch.cuda.default_stream(dev)


def run_calls(calls):
    for _, fn, _ in calls:
        fn()


def run_behind_gate(prepare, script, what, check_dry=None):
    """prepare() -> a fresh Context brought to the gate position and synchronised; script(ctx) -> the enqueue() entries.  Runs
    the entries un-gated on a throw-away context (closed afterwards) to measure their host time, then on a second context behind
    a gate of four times that, and synchronises.  Returns (ctx, log, dry-run seconds); the caller closes ctx.
    check_dry(ctx): called on the throw-away context after its synchronise.  The dry run is the free-running case -- the device
    works while the host enqueues, and its reports land between any two calls -- so a scenario may hold its snapshots to the
    oracle too."""
    def dry_run():
        ctx = prepare()
        calls = script(ctx)
        t0 = time.perf_counter()
        run_calls(calls)
        dt = time.perf_counter() - t0
        ctx.synchronize()
        if check_dry is not None:
            check_dry(ctx)
        ctx.close()
        return dt
    dry = dry_run()
    if GATE_FACTOR * dry > GATE_CEILING_S:
        dry = dry_run()                                                       # (the first run paid the process's one-time costs)
    assert GATE_FACTOR * dry <= GATE_CEILING_S, "%s: a dry run of %.3f s: shorten the scenario, not lengthen the gate" % (what, dry)
    ctx = prepare()
    calls = script(ctx)
    log = enqueue(ctx.stream, max(GATE_FLOOR_S, GATE_FACTOR * dry), calls, what)
    ctx.synchronize()
    DRY_RUNS[what] = dry
    print("dry run of %s: %.1f ms host time for %d calls" % (what, dry * 1e3, len(calls)))
    return ctx, log, dry


DRY_RUNS = {}                                                                  # {scenario: measured dry-run seconds} of this process


# ---------------------------------------------------------------------------------------------------------------- checks --

def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def list_of(s):
    from chord_amd import records as R
    n = int(host(s["count"], np.uint32)[0])
    return n, host(s["cmds"], np.uint32)[:3 * n].copy().view(R.DRAW_CMD)


def check_frame(s, want, what, hzb=True, counts=False):
    """A snapshot against the oracle's frame: image, list 0 and its count, -- counts: a frame with a history, whose four stage counts
    are defined -- the stage counts, and -- hzb -- the chain's min / max / valid range."""
    H.assert_vis_equal(host(s["vis"], np.uint64), want["vis"], s["w"], s["h"], what)
    n, cmds = list_of(s)
    assert n == len(want["cmds"]), "%s: list 0 holds %d commands, the oracle's %d" % (what, n, len(want["cmds"]))
    assert np.array_equal(cmds, want["cmds"]), what + ": list 0"
    if counts:
        got = host(s["counts"], np.uint32).tolist()
        assert got == want["counts"].tolist(), "%s: stage counts %r, the oracle's %r" % (what, got, want["counts"].tolist())
    if hzb:
        check_hzb(s, want, what)


def check_hzb(s, want, what):
    assert np.array_equal(host(s["hzb_min"], np.uint16), want["hzb_min"].view(np.uint16)), what + ": history HZB min"
    assert np.array_equal(host(s["hzb_max"], np.uint16), want["hzb_max"].view(np.uint16)), what + ": history HZB max"
    assert np.array_equal(host(s["valid_range"], np.uint32), want["valid_range"].view(np.uint32)), what + ": valid range"


def check_stats(ctx, want, what, counts=True):
    """After the final synchronise: no overflow, the last frame's triangles and -- a frame with history -- its four stage counts."""
    st = ctx.r.stats()
    assert st["overflow"] == 0, what
    assert st["trianglesSubmitted"] == want["stats"].trianglesSubmitted, (what, st["trianglesSubmitted"])
    if counts:
        got = [st["countInstanceCulled"], st["countStage0Visible"], st["countStage0Rejected"], st["countStage1Visible"]]
        assert got == want["counts"].tolist(), (what, got, want["counts"].tolist())
