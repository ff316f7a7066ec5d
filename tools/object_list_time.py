"""What a change of the object LIST costs on BASELINE config 4 (64 street instances of 352 objects: 22 528 objects) at 3840 x 2160.
Eight of the 64 instances leave the list and come back, by the two routes a host has, alternated in one process:

    a  set_object_list   chordvis_set_object_list of the other list, set_view, render_frame: the geometry stays, the history HZB stays
    b  upload_scene      chordvis_upload_scene of the scene under the other list (and chordvis_upload_material_textures where the scene
                         has material textures: config 4 has none), set_view, render_frame: the only way before -- every vertex and
                         meshlet copied again, a frame without history

A repeat is one change + one frame between two synchronisations, timed with the host clock; the routes take turns REPEATS times (the list
shrinks on even repeats and grows back on odd ones), after two untimed repeats each.  Before and after the changes, the steady frame time (FRAMES
frames between two synchronisations) of a context that never called chordvis_set_object_list, and between its blocks that of the
context that did, on the same full list: the frame path gains no launch and no byte, so the touched context's blocks lie among the
untouched one's.  The build kernel's own time comes from a `rocprofv3 --kernel-trace --stats` run of this script's --kernel-only mode
(a child process; LAUNCHES calls, no frames), with the bytes it writes per second (24 bytes per group instance).  Last, what was timed is
checked: after chordvis_reset_history route a's frame of either list is route b's, pixel for pixel.  Writes profiles/object_list_time.txt (or --out PATH).

    python tools/object_list_time.py [REPEATS] [FRAMES] [LAUNCHES] [--out PATH] [--no-rocprof]
"""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from chord_amd import lib as L, records as R, scenes  # noqa: E402
from chord_amd.renderer import VisibilityRenderer  # noqa: E402

INSTANCE_OBJECTS = 352
KERNEL = "group_refs_build_kernel"


def lists():
    """(scene under the full list, scene without every eighth street instance, camera)"""
    scene, cam = scenes.config4_street_x64(3840, 2160)
    L.fill_objects(scene, cam)
    n = len(scene.objects)
    assert n == 64 * INSTANCE_OBJECTS
    keep = np.flatnonzero((np.arange(n) // INSTANCE_OBJECTS) % 8 != 3)
    short = scene.with_objects(scene.objects[keep].copy())
    short.local_to_world = np.ascontiguousarray(scene.local_to_world[keep])
    return scene, short, cam


def kernel_only(launches):
    """The child under rocprofv3: `launches` list changes on a context without a target, nothing else."""
    full, short, _ = lists()
    r = VisibilityRenderer(0)
    r.upload_scene(full)
    for k in range(launches):
        r.set_object_list((short, full)[k & 1].objects)
    r.sync()
    r.close()
    print(json.dumps(dict(group_instances=[short.group_instances, full.group_instances])))


def rocprof_kernel(launches):
    """{calls, avg_us, min_us, max_us} of the build kernel from rocprofv3's stats, or {"error": ...}."""
    exe = shutil.which("rocprofv3") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "rocprofv3")
    if not os.path.exists(exe):
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="object_list_time_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "r", "--",
               sys.executable, os.path.abspath(__file__), "--kernel-only", str(launches)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            return {"error": "rocprofv3 exited with %d: %s" % (p.returncode, p.stderr[-400:])}
        for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as fh:
                for row in csv.DictReader(fh):
                    if KERNEL in row["Name"]:
                        return dict(calls=int(row["Calls"]), avg_us=float(row["AverageNs"]) / 1e3, min_us=float(row["MinNs"]) / 1e3,
                                    max_us=float(row["MaxNs"]) / 1e3, name=row["Name"])
        return {"error": "no row of %s in rocprofv3's kernel stats" % KERNEL}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    argv = sys.argv[1:]
    if "--kernel-only" in argv:
        return kernel_only(int(argv[argv.index("--kernel-only") + 1]))
    path = os.path.join(ROOT, "profiles", "object_list_time.txt")
    if "--out" in argv:
        path = argv[argv.index("--out") + 1]
        argv = [a for k, a in enumerate(argv) if k not in (argv.index("--out"), argv.index("--out") + 1)]
    pos = [int(a) for a in argv if a.isdigit()]
    repeats, frames, launches = (pos + [50, 100, 200][len(pos):])[:3]
    repeats = max(repeats, 50)
    repeats += repeats & 1                                                    # (even: the last repeat puts the full list back)
    import torch
    flags = R.FLAG_FRUSTUM_CULL | R.FLAG_CONE_CULL | R.FLAG_HZB_CULL
    full, short, cam = lists()
    view, iv = L.make_views(cam)
    w, h = cam.width, cam.height

    def context():
        r = VisibilityRenderer(0)
        r.upload_scene(full)
        r.allocate_gbuffer(w, h)
        r.set_view(view, iv, flags)
        r.render_frame()
        r.sync()
        return r

    untouched, a, b = context(), context(), context()

    def steady(r):
        for _ in range(10):
            r.render_frame()
        r.sync()
        t0 = time.perf_counter()
        for _ in range(frames):
            r.render_frame()
        r.sync()
        return (time.perf_counter() - t0) * 1e3 / frames

    def route_a(scene):
        a.set_object_list(scene.objects)
        a.set_view(view, iv, flags)
        a.render_frame()

    def route_b(scene):
        b.upload_scene(scene)
        b.set_view(view, iv, flags)
        b.render_frame()

    def timed(route, r, scene):
        r.sync()
        t0 = time.perf_counter()
        route(scene)
        r.sync()
        return (time.perf_counter() - t0) * 1e3

    first = steady(untouched)
    times = {"a set_object_list": [], "b upload_scene": []}
    for k in range(-2, repeats):                                              # (two untimed repeats each)
        scene = (short, full)[k & 1]
        ta, tb = timed(route_a, a, scene), timed(route_b, b, scene)
        if k >= 0:
            times["a set_object_list"].append(ta)
            times["b upload_scene"].append(tb)
    assert scene is full
    # the steady frame of the full list: the untouched context on either side of the touched one, three rounds
    blocks = {"untouched": [first], "touched": []}
    for _ in range(3):
        blocks["untouched"].append(steady(untouched))
        blocks["touched"].append(steady(a))
        blocks["untouched"].append(steady(untouched))
    launches_per_frame = (untouched.stats()["kernelLaunches"], a.stats()["kernelLaunches"])
    same_steady = bool(np.array_equal(a.read_visibility(), untouched.read_visibility()))
    # what was timed, checked.  Route a's frame ran against the history of the list before and route b's without one, and the two-pass
    # occlusion cull is the reference's: far away its image depends on the chain it culls against in a few pixels (the oracle's does
    # too).  The equivalence the header states is that of one frame after chordvis_reset_history, so that is what is compared.
    same_image = True
    for scene in (short, full):
        a.set_object_list(scene.objects)
        a.reset_history()
        a.set_view(view, iv, flags)
        a.render_frame()
        route_b(scene)
        same_image = bool(same_image and np.array_equal(a.read_visibility(), b.read_visibility()) and np.any(a.read_visibility()))
    for r in (untouched, a, b):
        r.close()
    kern = {"error": "skipped (--no-rocprof)"} if "--no-rocprof" in argv else rocprof_kernel(launches)

    def spread(v):
        s = sorted(v)
        return dict(ms_median=round(s[len(s) // 2], 4), ms_min=round(s[0], 4), ms_max=round(s[-1], 4))

    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        def out(s):
            print(s)
            fh.write(s + "\n")
        name_dev = torch.cuda.get_device_name(0)
        out("tools/object_list_time.py %d %d %d on %s: config 4 at %d x %d; the list is %d objects (%d group instances) or %d (%d)"
            % (repeats, frames, launches, name_dev, w, h, len(full.objects), full.group_instances, len(short.objects), short.group_instances))
        out("wall ms per change + one frame, host clock around work that ends in a synchronise, the routes in turn, %d repeats" % repeats)
        res = {}
        for name in times:
            res[name] = spread(times[name])
            out("  %-20s median %9.4f  min %9.4f  max %9.4f" % (name, res[name]["ms_median"], res[name]["ms_min"], res[name]["ms_max"]))
        ra, rb = res["a set_object_list"]["ms_median"], res["b upload_scene"]["ms_median"]
        out("  route a is %s route b: %.4f ms against %.4f ms (b / a = %.1f)" % ("below" if ra < rb else "NOT below", ra, rb, rb / ra))
        out("steady ms per frame, %d frames between two synchronisations, the full list" % frames)
        fmt = lambda v: "[" + ", ".join("%.4f" % x for x in v) + "]"
        out("  a context that never called chordvis_set_object_list: blocks %s (the first one before the changes)" % fmt(blocks["untouched"]))
        out("  the context after %d chordvis_set_object_list calls:  blocks %s (each between two of the untouched context's)" % (repeats + 2, fmt(blocks["touched"])))
        lo, hi = min(blocks["untouched"]), max(blocks["untouched"])
        touched = sorted(blocks["touched"])[len(blocks["touched"]) // 2]
        out("  the touched context's median block, %.4f, is %s the untouched context's blocks, %.4f .. %.4f (spread %.4f); kernel launches per frame: %d and %d"
            % (touched, "within" if lo <= touched <= hi else "NOT within", lo, hi, hi - lo, launches_per_frame[0], launches_per_frame[1]))
        if "error" in kern:
            out("build kernel: %s" % kern["error"])
        else:
            # (the child alternates the two lists: the mean launch writes the mean of their tables)
            mean_bytes = 24 * (full.group_instances + short.group_instances) / 2
            out("build kernel (rocprofv3 --kernel-trace --stats, %d calls): average %.2f us, min %.2f us, max %.2f us; %.2f MB written per call on"
                " average: %.2f TB/s" % (kern["calls"], kern["avg_us"], kern["min_us"], kern["max_us"], mean_bytes / 1e6, mean_bytes / 1e12 / (kern["avg_us"] * 1e-6)))
        out("after reset_history route a's frame of either list equals route b's: %s; the steady frames of the touched and the untouched context are equal: %s" % (same_image, same_steady))
        out(json.dumps(dict(repeats=repeats, frames=frames, launches=launches, device=name_dev, objects=[len(full.objects), len(short.objects)],
                            group_instances=[full.group_instances, short.group_instances], wall_ms=res,
                            steady_ms={k: [round(x, 4) for x in v] for k, v in blocks.items()}, launches_per_frame=launches_per_frame,
                            kernel=kern, same_image=same_image, same_steady=same_steady)))
    if not (same_image and same_steady):
        raise SystemExit("the images differ between the routes")


if __name__ == "__main__":
    main()
