"""chordvis_geometry_feedback and chordvis_visible_clusters on the config 3 frame (BASELINE config 3 under the textured materials) at
3840 x 2160, after a two-pass frame: ms per call at strides 1 and 4, and ms per chordvis_visible_clusters call, beside two yardsticks
that read the same image in the same run: chordvis_visibility_mark (stride 1 only: it has no lattice) and chordvis_material_feedback
at slotMask 15 and the same strides.  Every figure is the time between two events on the context's stream around N calls, after
WARMUP calls; the passes are timed ROUNDS times in turn (a, b, c, a, b, c, ...) in the one process and a line reports the median,
the minimum and every run.  After the timed calls the counts, the bitmap and the visible list are read back and compared with
tests/spec_geometry_feedback_np.py (exact equality; the counts of N calls are N times the spec's).

    python tools/geometry_feedback_time.py [N] [WARMUP] [ROUNDS]
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


def main():
    import spec_geometry_feedback_np as SG
    pos = [int(a) for a in sys.argv[1:] if a.isdigit()]
    n, warm, rounds = (pos + [50, 5, 5][len(pos):])[:3]
    flags = R.FLAG_FRUSTUM_CULL | R.FLAG_CONE_CULL | R.FLAG_HZB_CULL
    w, h = 3840, 2160
    scene, cam = scenes.config3_street(w, h, materials=True)
    L.fill_objects(scene, cam)
    view, iv = L.make_views(cam)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        r = VisibilityRenderer(0, stream=stream.cuda_stream)
        r.upload_scene(scene)
        r.upload_material_textures()
        r.allocate_gbuffer(w, h)
        r.set_view(view, iv, flags)
        r.render_frame()
        r.render_frame()
        r.sync()
        handle = r.last_frame_cmds()
        cmds = r.read_cmds(handle)
        words = r.read_visibility()
        out = torch.zeros(3 * handle.capacity + 1, dtype=torch.int32, device=torch.device("cuda", r.device))
        passes = [("geometry_feedback/1", lambda: r.geometry_feedback(1, (0, 0), handle)),
                  ("geometry_feedback/4", lambda: r.geometry_feedback(4, (0, 0), handle)),
                  ("visible_clusters", lambda: L.lib.chordvis_visible_clusters(r._ctx, handle, out.data_ptr(), out.data_ptr() + 12 * handle.capacity, handle.capacity)),
                  ("visibility_mark", lambda: r.visibility_mark(handle)),
                  ("material_feedback/1", lambda: r.material_feedback(15, 1, (0, 0), handle)),
                  ("material_feedback/4", lambda: r.material_feedback(15, 4, (0, 0), handle))]
        r.reset_geometry_feedback()
        r.reset_material_feedback()
        r.geometry_feedback(1, (0, 0), handle)                              # (visible_clusters wants a feedback call before it)
        times = {name: [] for name, _ in passes}
        for _ in range(rounds):
            for name, call in passes:
                for _ in range(warm):
                    call()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(n):
                    call()
                e1.record(stream)
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) / n)
        # the results of what was timed: stride 1 and stride 4, n calls each after a reset, against the spec
        cap = handle.capacity
        checked = {}
        for stride in (1, 4):
            r.reset_geometry_feedback()
            for _ in range(n):
                r.geometry_feedback(stride, (0, 0), handle)
            got = r.read_geometry_feedback()
            seen = r.read_geometry_feedback_seen()
            recs, total = r.visible_clusters(drawed_meshlet_cmd=handle, out=out)
            want = SG.geometry_feedback(scene, words, cmds, len(cmds), w, h, cap, stride, (0, 0))
            ok = all(np.array_equal(got[k], want[k] * np.uint32(n)) for k in SG.ARRAYS) and np.array_equal(seen, want["seen"]) and \
                total == len(want["visible"]) and np.array_equal(recs, want["visible"])
            checked[stride] = dict(equal_to_spec=bool(ok), totals_per_call=[int(v) for v in want["totals"]], commands=len(cmds),
                                   visible=len(want["visible"]), objects_with_pixels=int((want["objectPixels"] > 0).sum()), objects=len(scene.objects),
                                   lod_submitted=[int(v) for v in want["lodSubmitted"].sum(axis=0)[:4]], lod_visible=[int(v) for v in want["lodVisible"].sum(axis=0)[:4]])
    lines = []
    for name, _ in passes:
        t = sorted(times[name])
        lines.append(dict(call=name, ms_median=round(t[len(t) // 2], 4), ms_min=round(t[0], 4), runs_ms=[round(v, 4) for v in times[name]]))
        print("%-22s median %7.4f ms  min %7.4f ms   runs %s" % (name, lines[-1]["ms_median"], lines[-1]["ms_min"], lines[-1]["runs_ms"]))
    for stride, c in checked.items():
        print("stride %d: equal to the spec: %s; per call: %d lattice pixels, %d contributing, %d rejected; %d of %d commands seen; %d of %d objects own a pixel; "
              "submitted / visible per LOD 0..3: %s / %s" % (stride, c["equal_to_spec"], c["totals_per_call"][0], c["totals_per_call"][1], c["totals_per_call"][2],
                                                             c["visible"], c["commands"], c["objects_with_pixels"], c["objects"], c["lod_submitted"], c["lod_visible"]))
    print(json.dumps(dict(workload="config3_materials_3840x2160_two_pass", calls=n, warmup=warm, rounds=rounds, device=torch.cuda.get_device_name(0),
                          results=lines, checked=checked)))
    r.close()
    if not all(c["equal_to_spec"] for c in checked.values()):
        raise SystemExit("the counts differ from tests/spec_geometry_feedback_np.py")


if __name__ == "__main__":
    main()
