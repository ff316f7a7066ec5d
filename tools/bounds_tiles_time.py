"""chordvis_bin_bounds beside its yardstick, chordvis_visibility_mark, on the BASELINE config 3 frame at 3840 x 2160.

The frame is config 3's second frame.  The boxes are built as tools/bounds_query_time.py builds them -- the first n commands of an
instance cull's list, n the length of the list the second frame's phase-1 cull was given, each command's object matrices and meshlet
bounds -- from config 3 (5 072 boxes) and from config 4 (about 216 000; config 4 is rendered in a context of its own only to make
that list, and its boxes are then asked about under config 3's view and chain: to the calls they are boxes like any others).
chordvis_query_bounds(history chain, phase 1) makes the results once; then, timed in turn, ROUNDS times in the one process, for
T = 16 and T = 64:
    bin_bounds        chordvis_bin_bounds(NEAR | FAR): counts, items (room for MAX_PER_TILE), depth and totals (four launches)
    depth_only        count == 0, tileDepth only: the depth reduction alone (one launch); its GB/s are the image's 8 W H bytes over it
    visibility_mark   chordvis_visibility_mark on the same image: a pass that reads the same words (one launch)
Every figure is the time between two events on the context's stream around N calls, after WARMUP calls; a line reports the median,
the minimum and every run.  After the timed calls config 3's four outputs are compared with tests/spec_bounds_tiles_np.py (exact
equality).  Config 4's pair matrix would not fit in memory: only its depth bounds are compared with the spec, and its totals are
checked for agreeing with its own counts -- its lists are NOT checked here.  Writes
profiles/bounds_tiles_time.txt.

    python tools/bounds_tiles_time.py [N] [WARMUP] [ROUNDS]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from chord_amd import lib as L, records as R, scenes  # noqa: E402
from chord_amd.renderer import VisibilityRenderer  # noqa: E402

FLAGS = R.FLAG_FRUSTUM_CULL | R.FLAG_CONE_CULL | R.FLAG_HZB_CULL
MAX_PER_TILE = 128
W, H = 3840, 2160


def boxes_of(builder, stream):
    """(renderer, scene, view, iv, queries): two frames of the config, and the boxes of the first n commands of an instance cull."""
    scene, cam = builder()
    L.fill_objects(scene, cam)
    view, iv = L.make_views(cam)
    r = VisibilityRenderer(0, stream=stream.cuda_stream)
    r.upload_scene(scene)
    r.allocate_gbuffer(cam.width, cam.height)
    r.set_view(view, iv, FLAGS)
    r.render_frame()
    r.render_frame()
    count = int(r.stats()["countStage0Rejected"])                  # what the frame's phase-1 cull was given
    cmds = r.read_cmds(r.instance_culling())[:count]
    q = np.zeros(count, dtype=R.BOUNDS_QUERY)
    q["localToTranslatedWorld"] = scene.objects["localToTranslatedWorld"][cmds["objectId"]]
    q["localToTranslatedWorldLastFrame"] = scene.objects["localToTranslatedWorldLastFrame"][cmds["objectId"]]
    q["posMin"], q["posMax"] = scene.meshlets["posMin"][cmds["meshletId"]], scene.meshlets["posMax"][cmds["meshletId"]]
    q["user"] = cmds["slot"]
    return r, scene, view, iv, q


def timed(stream, passes, n, warm, rounds):
    times = {p: [] for p, _ in passes}
    for _ in range(rounds):
        for p, call in passes:
            for _ in range(warm):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(n):
                call()
            e1.record(stream)
            e1.synchronize()
            times[p].append(e0.elapsed_time(e1) / n)
    return times


def measure(name, r, view, iv, hzb, queries, stream, n, warm, rounds, check, out):
    import spec_bounds_tiles_np as S
    dev = torch.device("cuda", 0)
    count = len(queries)
    dq = torch.from_numpy(queries.view(np.uint8).copy()).to(dev)
    res = torch.zeros(4 * count, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert L.lib.chordvis_query_bounds(r._ctx, L.C.byref(hzb), 1, dq.data_ptr(), count, res.data_ptr(), None, None, 0) == L.OK, r.last_error()
    r.sync()
    results = res.cpu().numpy().view(R.BOUNDS_RESULT)
    handle = r.last_frame_cmds()
    report = []
    for T in (16, 64):
        tiles = S.tile_count(W, H, T)[0]
        cnt = torch.zeros(tiles, dtype=torch.int32, device=dev)
        items = torch.full((tiles * MAX_PER_TILE,), -1, dtype=torch.int32, device=dev)
        depth = torch.zeros(2 * tiles, dtype=torch.int32, device=dev)
        totals = torch.zeros(4, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        desc = L.BoundsTilesDesc(T, MAX_PER_TILE, 1, R.BOUNDS_TILES_NEAR | R.BOUNDS_TILES_FAR)
        full = L.BoundsTiles(cnt.data_ptr(), items.data_ptr(), depth.data_ptr(), totals.data_ptr())
        bare = L.BoundsTiles(None, None, depth.data_ptr(), None)
        d, f, b = L.C.byref(desc), L.C.byref(full), L.C.byref(bare)
        passes = [("bin_bounds", lambda: L.lib.chordvis_bin_bounds(r._ctx, d, res.data_ptr(), dq.data_ptr(), count, f)),
                  ("depth_only", lambda: L.lib.chordvis_bin_bounds(r._ctx, d, None, dq.data_ptr(), 0, b)),
                  ("visibility_mark", lambda: r.visibility_mark(handle))]
        times = timed(stream, passes, n, warm, rounds)
        assert passes[0][1]() == L.OK, r.last_error()
        r.sync()
        got = dict(counts=cnt.cpu().numpy().view(np.uint32), items=items.cpu().numpy().view(np.uint32).reshape(tiles, MAX_PER_TILE),
                   depth=depth.cpu().numpy().view(np.uint32).reshape(tiles, 2), totals=totals.cpu().numpy().view(np.uint32))
        words = r.read_visibility()
        equal = bool(np.array_equal(got["depth"], S.tile_depth(words, W, H, T)) and got["totals"][1] == got["counts"].astype(np.int64).sum() & 0xFFFFFFFF
                     and got["totals"][3] == got["counts"].max() and got["totals"][2] == (got["counts"] > MAX_PER_TILE).sum())
        if check:
            want = S.bin_bounds(words, W, H, results, T, MAX_PER_TILE, desc.flags, S.far_z(view, iv, queries, 1, results["status"]))
            equal = equal and all(np.array_equal(got[k], want[k]) for k in ("counts", "items", "depth", "totals"))
        med = {}
        for p, _ in passes:
            t = sorted(times[p])
            med[p] = t[len(t) // 2]
            report.append(dict(boxes=name, tile=T, call=p, ms_median=round(med[p], 4), ms_min=round(t[0], 4), runs_ms=[round(v, 4) for v in times[p]]))
            print("%-8s T %-3d %-16s median %7.4f ms  min %7.4f ms   runs %s" % (name, T, p, med[p], t[0], report[-1]["runs_ms"]), file=out)
        gbs = W * H * 8 / (med["depth_only"] * 1e-3) / 1e9
        mark_gbs = W * H * 8 / (med["visibility_mark"] * 1e-3) / 1e9
        print("%-8s T %-3d %d boxes, %d take part; kept pairs %d, tiles beyond %d: %d, longest list %d; bin_bounds / visibility_mark %.2f; depth_only / "
              "visibility_mark %.2f; depth_only %.0f GB/s of visibility words, visibility_mark %.0f GB/s; equal to the spec (%s): %s"
              % (name, T, count, got["totals"][0], got["totals"][1], MAX_PER_TILE, got["totals"][2], got["totals"][3], med["bin_bounds"] / med["visibility_mark"],
                 med["depth_only"] / med["visibility_mark"], gbs, mark_gbs, "all four outputs" if check else "depth bounds only; totals agree with the call's own counts", equal), file=out)
        report.append(dict(boxes=name, tile=T, count=count, take_part=int(got["totals"][0]), kept_pairs=int(got["totals"][1]), overflowing=int(got["totals"][2]),
                           longest=int(got["totals"][3]), depth_only_gbs=round(gbs, 1), visibility_mark_gbs=round(mark_gbs, 1), equal=equal))
        del cnt, items, depth, totals
    del dq, res
    torch.cuda.synchronize()
    return report


def main():
    pos = [int(a) for a in sys.argv[1:] if a.isdigit()]
    n, warm, rounds = (pos + [500, 20, 5][len(pos):])[:3]
    path = os.path.join(ROOT, "profiles", "bounds_tiles_time.txt")
    stream = torch.cuda.Stream()
    results = []
    with open(path, "w") as fh, torch.cuda.stream(stream):
        class Tee:
            def write(self, s):
                sys.stdout.write(s); fh.write(s)

            def flush(self):
                sys.stdout.flush(); fh.flush()
        out = Tee()
        print("tools/bounds_tiles_time.py %d %d %d on %s: ms per call between two events around %d calls, %d rounds in turn; config 3 at %d x %d, NEAR | FAR, "
              "maxPerTile %d" % (n, warm, rounds, torch.cuda.get_device_name(0), n, rounds, W, H, MAX_PER_TILE), file=out)
        other, _, _, _, many = boxes_of(lambda: scenes.config4_street_x64(W, H), stream)
        other.close()
        r, _, view, iv, few = boxes_of(lambda: scenes.config3_street(W, H), stream)
        hzb = r.history_hzb()
        results += measure("config3", r, view, iv, hzb, few, stream, n, warm, rounds, True, out)
        results += measure("config4", r, view, iv, hzb, many, stream, n, warm, rounds, False, out)
        r.close()
        print(json.dumps(dict(calls=n, warmup=warm, rounds=rounds, device=torch.cuda.get_device_name(0), results=results)), file=out)
    if not all(c.get("equal", True) for c in results):
        raise SystemExit("the outputs differ from the spec")


if __name__ == "__main__":
    main()
