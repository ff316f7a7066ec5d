"""What rebuilding the ray scene's TLAS on the device costs, and what its tree costs the walk, on BASELINE config 3 (352 objects) and
config 4 (22 528 objects) at 3840 x 2160 -- recorded, not gated.

    rebuild   chordvis_rebuild_ray_tlas, event-timed on the context's stream (the refit included), beside chordvis_build_ray_scene's
              TLAS-only rebuild of the same list as HOST WALL TIME: its wait, its read-back of the object array, the host build, the
              uploads and the refit
    trace     one closest-hit pixel-centre ray per pixel in pixel order, and the AO configuration of tools/pixel_rays_time.py
              (HEMISPHERE, closest hit, START_FROM_DEPTH), on the host-built tree and on the rebuilt tree of the same list; the hit
              buffers of the two trees are compared
    counters  TLAS nodes and objects entered per ray for both trees, from the -DCHORD_RAY_COUNTERS=1 build (chord_amd/build.py --tag
              raycount; built here if it is missing) in a child process of its own (this script with --counters)

Each device figure: ray_query_time.blocks -- untimed warm-up launches, then REPEATS blocks of LAUNCHES launches between two events;
the median block and the spread (min .. max), per launch.  Writes profiles/ray_tlas_time.txt (or --out PATH).

    python tools/ray_tlas_time.py [REPEATS] [LAUNCHES] [--out PATH]
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from chord_amd import lib as L, scenes  # noqa: E402
from chord_amd.renderer import VisibilityRenderer  # noqa: E402
from chord_amd import records as R  # noqa: E402
from pixel_rays_time import fused_call, hemisphere_table  # noqa: E402
from ray_query_time import COUNTER_NAMES, pixel_rays  # noqa: E402
from ray_shade_time import blocks  # noqa: E402

W, H = 3840, 2160
CONFIGS = (("config3", lambda w, h: scenes.config3_street(w, h, attributes=True)), ("config4", scenes.config4_street_x64))


def frame_images(r, scene, cam, dev):
    """(position, normal, visibility image) of two frames' second, on the current stream.  The normal image is the resolved vertex
    normal where the scene carries normals (config 3 with attributes); config 4's builder makes none, so its AO rays leave along a
    hemisphere about +y for every pixel."""
    view, iv = L.make_views(cam)
    vis = torch.zeros(W * H, dtype=torch.int64, device=dev)
    r.allocate_gbuffer(W, H, device_visibility=vis.data_ptr())
    r.set_view(view, iv, R.FLAG_FRUSTUM_CULL | R.FLAG_CONE_CULL | R.FLAG_HZB_CULL)
    r.render_frame()
    r.render_frame()
    if scene.normals is not None:
        res = r.resolve_attributes(names=["positionRS", "vertexNormal"])
        return res["positionRS"], res["vertexNormal"], vis
    pos = r.resolve_attributes(names=["positionRS"])["positionRS"]
    nrm = torch.zeros_like(pos)
    nrm[:, :, 1] = 1.0
    return pos, nrm, vis


def counters_child():
    """--counters: under the measuring library, the pixel-order closest-hit set once per config and tree; one JSON line of the sums."""
    dev = torch.device("cuda", 0)
    out = {}
    for name, make in CONFIGS:
        scene, cam = make(W, H)
        L.fill_objects(scene, cam)
        view, _ = L.make_views(cam)
        r = VisibilityRenderer(0)
        r.upload_scene(scene)
        r.build_ray_scene()
        rays = pixel_rays(view, W, H, dev)
        hits = torch.empty((W * H, 8), dtype=torch.int32, device=dev)

        def sums():
            words = np.zeros(40, dtype=np.uint64)
            r.sync()
            r._check(L.lib.chordvis_debug_read(r._ctx, 10, 0, words.nbytes, words.ctypes.data), "debug_read 10 (is this the -DCHORD_RAY_COUNTERS=1 library?)")
            return words[::8].astype(np.int64)

        for tree in ("host", "rebuilt"):
            if tree == "rebuilt":
                r.rebuild_ray_tlas()
            before = sums()
            r.trace_rays(rays, out=hits)
            out["%s_%s" % (name, tree)] = dict(zip(COUNTER_NAMES, (int(v) for v in sums() - before)))
        del rays, hits
        torch.cuda.synchronize(dev)
        torch.cuda.empty_cache()
        r.close()
    print("RAY_COUNTERS " + json.dumps(out))


def measure_counters():
    from chord_amd import build as B
    lib = os.path.join(B.OUT_DIR, "libchordvis_raycount.so")
    if not os.path.exists(lib):
        B.build(verbose=False, defines=("-DCHORD_RAY_COUNTERS=1",), tag="raycount")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--counters"], env=dict(os.environ, CHORDVIS_LIB=lib), capture_output=True, text=True, timeout=500)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RAY_COUNTERS ")]
    if p.returncode != 0 or not line:
        raise RuntimeError("the counting run failed (%d): %s" % (p.returncode, (p.stdout + p.stderr)[-2000:]))
    return json.loads(line[-1][len("RAY_COUNTERS "):])


def spread(samples):
    s = sorted(samples)
    return {"ms_median": round(s[len(s) // 2], 5), "ms_min": round(s[0], 5), "ms_max": round(s[-1], 5)}


def fmt(b):
    return "median %.4f ms (min %.4f, max %.4f)" % (b["ms_median"], b["ms_min"], b["ms_max"])


def main():
    argv = sys.argv[1:]
    if "--counters" in argv:
        return counters_child()
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "ray_tlas_time.txt")
    nums = [int(a) for a in argv if a.isdigit()]
    repeats, launches = (nums + [9, 5])[:2] if len(nums) < 2 else nums[:2]
    dev = torch.device("cuda", 0)
    res = {"repeats": repeats, "launches": launches, "device": torch.cuda.get_device_name(0)}
    lines = ["tools/ray_tlas_time.py %d %d on %s at %d x %d" % (repeats, launches, res["device"], W, H)]
    for name, make in CONFIGS:
        scene, cam = make(W, H)
        L.fill_objects(scene, cam)
        view, _ = L.make_views(cam)
        stream = torch.cuda.Stream()
        torch.cuda.set_stream(stream)
        r = VisibilityRenderer(0, stream=stream.cuda_stream)
        r.upload_scene(scene)
        r.build_ray_scene()
        e = {"objects": len(scene.objects), "real_normals": scene.normals is not None}
        # the host's TLAS-only rebuild, as wall time with its wait
        wall = []
        for _ in range(repeats):
            r.sync()
            t0 = time.perf_counter()
            info = r.build_ray_scene()
            r.sync()
            wall.append((time.perf_counter() - t0) * 1e3)
        e["host_tlas_wall"] = spread(wall)
        e["host_tree"] = {"nodes": info.tlasNodes, "depth": info.tlasDepth}
        pos, nrm, vis = frame_images(r, scene, cam, dev)
        table = hemisphere_table(dev)
        rays = pixel_rays(view, W, H, dev)
        ao = torch.empty((H, W), dtype=torch.float32, device=dev)
        hits = {t: torch.empty((W * H, 8), dtype=torch.int32, device=dev) for t in ("host", "rebuilt")}
        r.sync()
        for tree in ("host", "rebuilt"):
            if tree == "rebuilt":
                e["rebuild"] = blocks(stream, r.rebuild_ray_tlas, repeats, 4 * launches)
                e["rebuild"]["launches"] = 2 if len(scene.objects) <= L.RAY_TLAS_GROUP_MAX else 15
                info = r.ray_scene_info()
                e["rebuilt_tree"] = {"nodes": info.tlasNodes, "depth": info.tlasDepth}
            e["closest_" + tree] = blocks(stream, lambda: r.trace_rays(rays, out=hits[tree]), repeats, launches)
            e["ao_" + tree] = blocks(stream, fused_call(r, "ao", pos, nrm, vis, table, cam.z_near, ao), repeats, launches)
        r.sync()
        e["hits_equal"] = bool(torch.equal(hits["host"], hits["rebuilt"]))
        e["hit_fraction"] = round(float((hits["host"][:, 7] & 1).float().mean()), 4)
        res[name] = e
        del pos, nrm, vis, table, rays, ao, hits
        torch.cuda.synchronize(dev)
        torch.cuda.empty_cache()
        r.close()
        torch.cuda.set_stream(torch.cuda.default_stream(dev))
        lines.append("%s, %d objects%s:" % (name, e["objects"], "" if e["real_normals"] else " (no vertex normals in this scene: the AO normal image is +y everywhere)"))
        lines.append("  chordvis_rebuild_ray_tlas (%d launches, the refit included): %s; tree %d nodes, %d levels"
                     % (e["rebuild"]["launches"], fmt(e["rebuild"]), e["rebuilt_tree"]["nodes"], e["rebuilt_tree"]["depth"]))
        lines.append("  chordvis_build_ray_scene, TLAS only, host wall with its wait and read-back: %s; tree %d nodes, %d levels"
                     % (fmt(e["host_tlas_wall"]), e["host_tree"]["nodes"], e["host_tree"]["depth"]))
        for k, what in (("closest", "closest hit, a ray per pixel in pixel order"), ("ao", "AO (HEMISPHERE, closest, START_FROM_DEPTH)")):
            a, b = e[k + "_host"], e[k + "_rebuilt"]
            lines.append("  %s: host-built tree %s; rebuilt tree %s; rebuilt / host %.3f" % (what, fmt(a), fmt(b), b["ms_median"] / a["ms_median"]))
        lines.append("  the two trees' hit buffers are equal: %s (hit fraction %.3f)" % (e["hits_equal"], e["hit_fraction"]))
    res["counters"] = measure_counters()
    lines.append("entered per ray, means over the pixel-order closest-hit set (a -DCHORD_RAY_COUNTERS=1 build, one launch per tree, a process of its own):")
    for name, _ in CONFIGS:
        for tree in ("host", "rebuilt"):
            c = res["counters"]["%s_%s" % (name, tree)]
            n = float(c["rays"])
            lines.append("  %s, %s tree: TLAS nodes %.2f, objects entered %.2f, BLAS nodes %.2f, triangles %.2f"
                         % (name, tree, c["tlas_nodes"] / n, c["tlas_leaves"] / n, c["blas_nodes"] / n, c["triangles"] / n))
    lines.append(json.dumps(res))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
