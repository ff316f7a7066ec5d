"""chordvis_query_bounds beside its yardstick, the phase-1 occlusion cull, on BASELINE config 3 and config 4 at 3840 x 2160.

Per config: two frames are rendered; n is the length of the list the second frame's phase-1 cull was given (countStage0Rejected); the
first n commands of an instance cull's list -- a mix of hidden and visible clusters, where the frame's own rejected list tested again
against the chain that rejected it would keep nothing -- are the cull's input, and the same n commands become n queries: each
command's object matrices and meshlet bounds, so the query call projects the same boxes and taps the same texels as the cull.
Timed in turn, ROUNDS times in the one process:
    query_bounds      chordvis_query_bounds(history chain, phase 1, n queries): results, visible list and count (two launches)
    query_results     the same with the list and the count not asked for (one launch)
    hzb_culling       chordvis_hzb_culling(history chain, second stage, the n-command list) (a 4-byte memset and one launch)
Every figure is the time between two events on the context's stream around N calls, after WARMUP calls; a line reports the median, the
minimum and every run.  After the timed calls the query results are compared with tests/spec_bounds_query_np.py and the visible
queries with the commands the cull kept (exact equality).  Writes profiles/bounds_query_time.txt.

    python tools/bounds_query_time.py [N] [WARMUP] [ROUNDS]
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


def measure(name, builder, n, warm, rounds, out):
    import spec_bounds_query_np as S
    flags = R.FLAG_FRUSTUM_CULL | R.FLAG_CONE_CULL | R.FLAG_HZB_CULL
    scene, cam = builder()
    L.fill_objects(scene, cam)
    view, iv = L.make_views(cam)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        r = VisibilityRenderer(0, stream=stream.cuda_stream)
        r.upload_scene(scene)
        r.allocate_gbuffer(cam.width, cam.height)
        r.set_view(view, iv, flags)
        r.render_frame()
        r.render_frame()
        hzb = r.history_hzb()
        count = int(r.stats()["countStage0Rejected"])              # what the frame's phase-1 cull was given
        full = r.instance_culling()
        cmds = r.read_cmds(full)[:count]
        length = torch.full((1,), count, dtype=torch.int32, device=dev)
        given = L.CountAndCmd(length.data_ptr(), full.cmds, full.capacity)     # the list's first `count` commands
        q = np.zeros(count, dtype=R.BOUNDS_QUERY)
        q["localToTranslatedWorld"] = scene.objects["localToTranslatedWorld"][cmds["objectId"]]
        q["localToTranslatedWorldLastFrame"] = scene.objects["localToTranslatedWorldLastFrame"][cmds["objectId"]]
        q["posMin"], q["posMax"] = scene.meshlets["posMin"][cmds["meshletId"]], scene.meshlets["posMax"][cmds["meshletId"]]
        q["user"] = cmds["slot"]
        dq = torch.from_numpy(q.view(np.uint8).copy()).to(dev)
        res = torch.zeros(4 * count, dtype=torch.int32, device=dev)
        vis = torch.zeros(count + 1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        h = L.C.byref(hzb)
        passes = [("query_bounds", lambda: L.lib.chordvis_query_bounds(r._ctx, h, 1, dq.data_ptr(), count, res.data_ptr(), vis.data_ptr() + 4, vis.data_ptr(), count)),
                  ("query_results", lambda: L.lib.chordvis_query_bounds(r._ctx, h, 1, dq.data_ptr(), count, res.data_ptr(), None, None, 0)),
                  ("hzb_culling", lambda: r.hzb_culling(hzb, False, given))]
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
        # what was timed, checked: the spec on the chain read back, and the cull's own answer for the same commands
        assert passes[0][1]() == L.OK, r.last_error()
        kept, _ = r.hzb_culling(hzb, False, given)
        kept = r.read_cmds(kept)
        r.sync()
        got = res.cpu().numpy().view(R.BOUNDS_RESULT)
        listed = vis.cpu().numpy().view(np.uint32)
        want, wvis, wn = S.query_bounds(view, iv, q, 1, hzb.desc, r.read_hzb(hzb)[0])
        unoccluded = np.flatnonzero((got["status"] & R.BOUNDS_UNOCCLUDED) != 0)
        equal = bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)) and listed[0] == wn and np.array_equal(listed[1:1 + wn], wvis))
        as_cull = bool(np.array_equal(np.sort(cmds["slot"][unoccluded]), np.sort(kept["slot"])))
        r.close()
    long_cull, long_query = given.capacity > 65536, count > 65536
    lines = []
    for p, _ in passes:
        t = sorted(times[p])
        lines.append(dict(call=p, ms_median=round(t[len(t) // 2], 4), ms_min=round(t[0], 4), ns_per_item_median=round(1e6 * t[len(t) // 2] / max(count, 1), 2),
                          runs_ms=[round(v, 4) for v in times[p]]))
        print("%-10s %-14s median %7.4f ms  min %7.4f ms  %7.2f ns/item   runs %s" % (name, p, lines[-1]["ms_median"], lines[-1]["ms_min"],
                                                                                  lines[-1]["ns_per_item_median"], lines[-1]["runs_ms"]), file=out)
    print("%-10s %d commands = %d queries (list capacity %d): the cull runs its %s form, the query its %s form; %d visible, %d kept by the cull; "
          "results equal to the spec: %s; unoccluded queries are the commands the cull kept: %s"
          % (name, count, count, given.capacity, "one-per-thread" if long_cull else "eight-lane", "one-per-thread" if long_query else "eight-lane",
             wn, len(kept), equal, as_cull), file=out)
    return dict(config=name, items=count, list_capacity=int(given.capacity), results=lines, equal_to_spec=equal, unoccluded_equal_cull_kept=as_cull)


def main():
    pos = [int(a) for a in sys.argv[1:] if a.isdigit()]
    n, warm, rounds = (pos + [500, 20, 5][len(pos):])[:3]
    path = os.path.join(ROOT, "profiles", "bounds_query_time.txt")
    results = []
    with open(path, "w") as fh:
        class Tee:
            def write(self, s):
                sys.stdout.write(s); fh.write(s)

            def flush(self):
                sys.stdout.flush(); fh.flush()
        out = Tee()
        print("tools/bounds_query_time.py %d %d %d on %s: ms per call between two events around %d calls, %d rounds in turn"
              % (n, warm, rounds, torch.cuda.get_device_name(0), n, rounds), file=out)
        for name, builder in (("config3", lambda: scenes.config3_street(3840, 2160)), ("config4", lambda: scenes.config4_street_x64(3840, 2160))):
            results.append(measure(name, builder, n, warm, rounds, out))
        print(json.dumps(dict(calls=n, warmup=warm, rounds=rounds, device=torch.cuda.get_device_name(0), results=results)), file=out)
    if not all(c["equal_to_spec"] and c["unoccluded_equal_cull_kept"] for c in results):
        raise SystemExit("the query results differ from the spec or from the cull")


if __name__ == "__main__":
    main()
