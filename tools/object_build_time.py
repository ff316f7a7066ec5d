"""What a moving camera costs per frame on BASELINE config 4 (22 528 objects) at 3840 x 2160, three ways to get the object records of
the frame to the device, alternated in one process:

    A  host_fill_update   lib.fill_objects on the host (chordvis_object_basic_data_batch), chordvis_update_objects (224 B per object
                          from pageable memory), set_view, render_frame: the only way before chordvis_build_objects
    B  build_objects      chordvis_build_objects from the resident world transforms (nothing scattered: the objects stand), set_view,
                          render_frame
    C  bound_prebuilt     chordvis_bind_objects of a device array filled and uploaded before the timed region, set_view, render_frame:
                          bench.py's moving_path form, the floor for B (a real host cannot pre-build the arrays)

The camera walks a closed path of POSES views, 0.5 m per frame there and back, so every frame's camera differs from the one before.
A block is FRAMES frames of one form between two synchronisations, timed with the host clock (wall ms per frame); the three forms are
run in turn ROUNDS times after one untimed block each; a line reports the median, the minimum and every block.  Then the device time
of the kernels alone, between two events around LAUNCHES launches: chordvis_build_objects, and chordvis_scatter_world_transforms of 5 %
and of 100 % of the objects.  Last, what was timed is checked: the built records equal the host-filled ones byte for byte, and the three
forms leave the same image.  Writes profiles/object_build_time.txt (or --out PATH).

    python tools/object_build_time.py [FRAMES] [ROUNDS] [LAUNCHES] [--out PATH]
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from chord_amd import lib as L, records as R, scenes  # noqa: E402
from chord_amd.renderer import VisibilityRenderer  # noqa: E402

POSES = 8


def main():
    argv = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "object_build_time.txt")
    if "--out" in argv:
        path = argv[argv.index("--out") + 1]
    pos = [int(a) for a in argv if a.isdigit()]
    frames, rounds, launches = (pos + [200, 5, 200][len(pos):])[:3]
    flags = R.FLAG_FRUSTUM_CULL | R.FLAG_CONE_CULL | R.FLAG_HZB_CULL
    scene, cam0 = scenes.config4_street_x64(3840, 2160)
    n = len(scene.objects)
    f = np.array(cam0.front, dtype=np.float64)
    f /= np.linalg.norm(f)
    steps = list(range(POSES // 2 + 1)) + list(range(POSES // 2 - 1, 0, -1))            # 0 1 2 3 4 3 2 1
    cams = [cam0.moved(tuple(0.5 * s * f)) for s in steps]
    base = [L.make_views(c)[0] for c in cams]
    views = [L.make_views(c, base[k - 1]) for k, c in enumerate(cams)]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        r = VisibilityRenderer(0, stream=stream.cuda_stream)
        r.upload_scene(scene)
        r.allocate_gbuffer(cam0.width, cam0.height)
        r.upload_world_transforms(scene.local_to_world)
        filled = [L.fill_objects(scene, c, cams[k - 1]).copy() for k, c in enumerate(cams)]
        bound = [torch.from_numpy(o.view(np.uint8).reshape(-1).copy()).to(dev) for o in filled]
        position = [(C.c_double * 3)(*c.position) for c in cams]
        torch.cuda.synchronize()

        def frame_a(k):
            r.update_objects(L.fill_objects(scene, cams[k], cams[k - 1]))
            r.set_view(views[k][0], views[k][1], flags)
            r.render_frame()

        def frame_b(k):
            L.lib.chordvis_build_objects(r._ctx, position[k], position[k - 1])
            r.set_view(views[k][0], views[k][1], flags)
            r.render_frame()

        def frame_c(k):
            r.bind_objects(bound[k].data_ptr(), n)
            r.set_view(views[k][0], views[k][1], flags)
            r.render_frame()

        forms = [("A host_fill_update", frame_a), ("B build_objects", frame_b), ("C bound_prebuilt", frame_c)]

        def block(frame):
            r.sync()
            t0 = time.perf_counter()
            for i in range(frames):
                frame(i % POSES)
            r.sync()
            return (time.perf_counter() - t0) * 1e3 / frames

        times = {name: [] for name, _ in forms}
        for name, frame in forms:                                                      # warm-up: one untimed block each
            block(frame)
        for _ in range(rounds):
            for name, frame in forms:
                times[name].append(block(frame))
        # the host's share of A, by itself
        t0 = time.perf_counter()
        for i in range(20):
            L.fill_objects(scene, cams[i % POSES], cams[i % POSES - 1])
        fill_ms = (time.perf_counter() - t0) * 1e3 / 20

        # the kernels alone
        def device_ms(call):
            for _ in range(20):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(launches):
                call()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / launches

        rng = np.random.default_rng(4)
        kernels = {}
        for _ in range(rounds):
            kernels.setdefault("build_objects", []).append(device_ms(lambda: L.lib.chordvis_build_objects(r._ctx, position[1], position[0])))
        for share in (5, 100):
            m = n * share // 100
            idx = np.sort(rng.permutation(n)[:m]).astype(np.int32)
            ti = torch.from_numpy(idx).to(dev)
            tm = torch.from_numpy(np.ascontiguousarray(scene.local_to_world[idx])).to(dev)
            torch.cuda.synchronize()
            for _ in range(rounds):
                kernels.setdefault("scatter_%d%%" % share, []).append(
                    device_ms(lambda: L.lib.chordvis_scatter_world_transforms(r._ctx, ti.data_ptr(), tm.data_ptr(), m)))
            kernels["scatter_%d%%_objects" % share] = m

        # what was timed, checked
        images = []
        for name, frame in forms:
            for k in range(POSES):
                frame(k)
            images.append(r.read_visibility().copy())
        same_image = bool(np.array_equal(images[0], images[1]) and np.array_equal(images[0], images[2]) and np.any(images[0]))
        r.build_objects(cams[3].position, cams[2].position)
        same_records = r.read_objects().tobytes() == filled[3].tobytes()
        cur, _ = r.read_world_transforms()
        same_records = bool(same_records and np.array_equal(cur, scene.local_to_world))
        r.close()

    def spread(v):
        s = sorted(v)
        return dict(ms_median=round(s[len(s) // 2], 4), ms_min=round(s[0], 4), ms_max=round(s[-1], 4), runs_ms=[round(x, 4) for x in v])

    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        def out(s):
            print(s)
            fh.write(s + "\n")
        name_dev = torch.cuda.get_device_name(0)
        out("tools/object_build_time.py %d %d %d on %s: config 4 (%d objects) at 3840 x 2160, a camera that moves every frame (%d poses)"
            % (frames, rounds, launches, name_dev, n, POSES))
        out("wall ms per frame, host clock around blocks of %d frames that end in a synchronise, the three forms in turn, %d rounds" % (frames, rounds))
        res = {}
        for name, _ in forms:
            res[name] = spread(times[name])
            out("  %-20s median %7.4f  min %7.4f  max %7.4f   blocks %s" % (name, res[name]["ms_median"], res[name]["ms_min"], res[name]["ms_max"], res[name]["runs_ms"]))
        a, b, c = (res[name]["ms_median"] for name, _ in forms)
        noise = max(res[name]["ms_max"] - res[name]["ms_min"] for name, _ in forms)
        out("  A - B = %.4f ms per frame, B - C = %.4f ms per frame; widest spread of one form over its blocks: %.4f ms" % (a - b, b - c, noise))
        out("  B is %s A by more than that spread" % ("below" if a - b > noise else "NOT below"))
        out("  the host's share of A by itself: lib.fill_objects %.4f ms per call (%d objects); the records are %.2f MB per frame" % (fill_ms, n, n * 224 / 1e6))
        out("device ms per launch between two events around %d launches, %d rounds" % (launches, rounds))
        kres = {}
        for kname in ("build_objects", "scatter_5%", "scatter_100%"):
            kres[kname] = spread(kernels[kname])
            extra = "" if kname == "build_objects" else "  (%d matrices)" % kernels[kname + "_objects"]
            out("  %-20s median %7.4f  min %7.4f  max %7.4f   runs %s%s" % (kname, kres[kname]["ms_median"], kres[kname]["ms_min"], kres[kname]["ms_max"],
                                                                       kres[kname]["runs_ms"], extra))
        out("  the build moves %d x 592 B = %.1f MB: %.2f TB/s at the median" % (n, n * 592 / 1e6, n * 592 / 1e12 / (kres["build_objects"]["ms_median"] * 1e-3)))
        out("built records equal the host-filled ones byte for byte, cur unchanged: %s; the three forms leave the same image: %s" % (same_records, same_image))
        out(json.dumps(dict(frames=frames, rounds=rounds, launches=launches, device=name_dev, objects=n, wall_ms_per_frame=res, fill_objects_ms=round(fill_ms, 4),
                            device_ms_per_launch=kres, same_records=same_records, same_image=same_image)))
    if not (same_records and same_image):
        raise SystemExit("the built records or the images differ between the forms")


if __name__ == "__main__":
    main()
