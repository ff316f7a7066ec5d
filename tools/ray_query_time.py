"""What ray queries cost on BASELINE config 3 (the street, 352 objects) at 3840 x 2160 -- recorded, not gated: there is no earlier figure
for a capability that did not exist.

    build     host wall time of chordvis_build_ray_scene (BLASes + TLAS + refit, one synchronise), and of a second call (TLAS only);
              the ray scene's device bytes beside the bytes of the scene's own arrays
    refit     chordvis_refit_ray_scene for config 3, and for config 4's 22 528 objects (a context of its own)
    closest   one pixel-centre ray per pixel (formed in binary64 from the view), in pixel order and in a fixed shuffled order
    any-hit   from those hit points towards one sun direction, tMin 1e-2

Each device figure: WARMUP untimed launches, then REPEATS blocks of LAUNCHES launches between two events on the context's stream; the
median block, and the spread (min .. max), per launch.

    counters  beside the times, per ray set: the mean TLAS nodes, objects entered (TLAS leaves), BLAS nodes and triangles tested per ray.
              The product kernel carries no counters: they come from a measuring build of the library, -DCHORD_RAY_COUNTERS=1
              (chord_amd/build.py --tag raycount; built here if it is missing), loaded through CHORDVIS_LIB by a child process of its
              own (this script with --counters) that launches each ray set once and reads the sums (chordvis_debug_read 10).  The
              child's hits are compared with nothing here; the traversal is the product's, the sums ride along.

Writes profiles/ray_query_time.txt (or --out PATH).

    python tools/ray_query_time.py [REPEATS] [LAUNCHES] [--out PATH]
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from chord_amd import lib as L, records as R, scenes  # noqa: E402
from chord_amd.renderer import VisibilityRenderer  # noqa: E402

WARMUP = 3
SUN = (0.35, 0.8, 0.45)


def scene_bytes(scene):
    return sum(a.nbytes for a in (scene.objects, scene.primitives, scene.materials, scene.meshlets, scene.groups, scene.group_indices,
                                  scene.meshlet_data, scene.positions))


def blocks(r, call, repeats, launches):
    """ms per launch: the blocks' median, min and max."""
    stream = torch.cuda.ExternalStream(r.stream(), device=torch.device("cuda", 0))
    for _ in range(WARMUP):
        call()
    r.sync()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(launches):
            call()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b) / launches)
    out.sort()
    return {"ms_median": round(out[len(out) // 2], 5), "ms_min": round(out[0], 5), "ms_max": round(out[-1], 5)}


def pixel_rays(view, w, h, dev):
    m = torch.from_numpy(view["translatedWorldToClip"][0].astype(np.float64).reshape(4, 4).T.copy())
    inv = torch.linalg.inv(m).to(dev)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64, device=dev), torch.arange(w, dtype=torch.float64, device=dev), indexing="ij")
    ndc = torch.stack([(xs + 0.5) / w * 2.0 - 1.0, 1.0 - (ys + 0.5) / h * 2.0, torch.full_like(xs, 0.5), torch.ones_like(xs)], dim=-1).reshape(-1, 4)
    p = ndc @ inv.T
    p = p[:, :3] / p[:, 3:4]
    d = (p / p.norm(dim=1, keepdim=True)).to(torch.float32)
    rays = torch.zeros((w * h, 8), dtype=torch.float32, device=dev)
    rays[:, 3], rays[:, 4:7], rays[:, 7] = 1e-2, d, 1e9
    return rays


COUNTER_NAMES = ("rays", "tlas_nodes", "tlas_leaves", "blas_nodes", "triangles")


def ray_sets(r, view, w, h, dev, run):
    """The three ray sets in turn: run(name, rays, any_hit, hits) launches (and times or counts) one; hits is written by it."""
    n = w * h
    rays = pixel_rays(view, w, h, dev)
    hits = torch.empty((n, 8), dtype=torch.int32, device=dev)
    run("closest_pixel_order", rays, False, hits)
    first = hits.clone()
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(dev)
    shuffled = rays[perm].contiguous()
    run("closest_shuffled", shuffled, False, hits)
    same = bool(torch.equal(hits, first[perm]))
    del shuffled
    # shadow rays from the hit points towards the sun
    t = first[:, 0].view(torch.float32)
    sun = torch.tensor(SUN, dtype=torch.float32, device=dev)
    sun = sun / sun.norm()
    shadow = torch.zeros_like(rays)
    shadow[:, :3] = rays[:, :3] + rays[:, 4:7] * t[:, None]
    shadow[:, 3], shadow[:, 4:7], shadow[:, 7] = 1e-2, sun, 1e9
    shadow = shadow[(first[:, 7] & 1) != 0].contiguous()
    hits = torch.empty((len(shadow), 8), dtype=torch.int32, device=dev)
    run("any_hit_sun", shadow, True, hits)
    # trace_rays records its tensors on the context's stream: they go back to the allocator before close() destroys that stream
    del rays, hits, first, perm, shadow, t, sun
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    return same


def counters_child():
    """--counters: under the measuring library, each ray set once; one JSON line of the sums per set."""
    dev = torch.device("cuda", 0)
    w, h = 3840, 2160
    scene, cam = scenes.config3_street(w, h)
    L.fill_objects(scene, cam)
    view, _ = L.make_views(cam)
    r = VisibilityRenderer(0)
    r.upload_scene(scene)
    r.build_ray_scene()
    out = {}

    def sums():
        words = np.zeros(40, dtype=np.uint64)
        r.sync()
        r._check(L.lib.chordvis_debug_read(r._ctx, 10, 0, words.nbytes, words.ctypes.data), "debug_read 10 (is this the -DCHORD_RAY_COUNTERS=1 library?)")
        return words[::8].astype(np.int64)

    def run(name, rays, any_hit, hits):
        before = sums()
        r.trace_rays(rays, any_hit=any_hit, out=hits)
        d = sums() - before
        assert d[0] == len(hits), (name, d[0], len(hits))
        out[name] = dict(zip(COUNTER_NAMES, (int(v) for v in d)))

    ray_sets(r, view, w, h, dev, run)
    r.close()
    print("RAY_COUNTERS " + json.dumps(out))


def measure_counters():
    """The child process under the measuring library; {set: {counter: sum}}."""
    from chord_amd import build as B
    lib = os.path.join(B.OUT_DIR, "libchordvis_raycount.so")
    if not os.path.exists(lib):
        B.build(verbose=False, defines=("-DCHORD_RAY_COUNTERS=1",), tag="raycount")
    env = dict(os.environ, CHORDVIS_LIB=lib)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--counters"], env=env, capture_output=True, text=True, timeout=400)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RAY_COUNTERS ")]
    if p.returncode != 0 or not line:
        raise RuntimeError("the counting run failed (%d): %s" % (p.returncode, (p.stdout + p.stderr)[-2000:]))
    return json.loads(line[-1][len("RAY_COUNTERS "):])


def main():
    argv = sys.argv[1:]
    if "--counters" in argv:
        return counters_child()
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "ray_query_time.txt")
    nums = [int(a) for a in argv if a.isdigit()]
    repeats, launches = (nums + [9, 5])[:2] if len(nums) < 2 else nums[:2]
    dev = torch.device("cuda", 0)
    w, h = 3840, 2160
    res = {"repeats": repeats, "launches": launches, "device": torch.cuda.get_device_name(0)}

    scene, cam = scenes.config3_street(w, h)
    L.fill_objects(scene, cam)
    view, iv = L.make_views(cam)
    r = VisibilityRenderer(0)
    r.upload_scene(scene)
    t0 = time.perf_counter(); info = r.build_ray_scene(); t1 = time.perf_counter(); r.build_ray_scene(); t2 = time.perf_counter()
    res["build"] = {"first_s": round(t1 - t0, 3), "second_tlas_only_s": round(t2 - t1, 4), "info": info.as_dict(), "scene_bytes": scene_bytes(scene)}
    res["refit_config3"] = dict(blocks(r, r.refit_ray_scene, repeats, 20 * launches), objects=len(scene.objects))

    def timed(name, rr, any_hit, hits):
        b = blocks(r, lambda: r.trace_rays(rr, any_hit=any_hit, out=hits), repeats, launches)
        r.sync()
        b["rays"] = len(hits)
        b["grays_per_s"] = round(len(hits) / (b["ms_median"] * 1e-3) / 1e9, 4)
        b["hit_fraction"] = round(float((hits[:, 7] & 1).float().mean()), 4)
        res[name] = b

    res["shuffled_equals_ordered"] = ray_sets(r, view, w, h, dev, timed)
    r.close()

    scene4, cam4 = scenes.config4_street_x64(w, h)
    L.fill_objects(scene4, cam4)
    r = VisibilityRenderer(0)
    r.upload_scene(scene4)
    t0 = time.perf_counter(); info4 = r.build_ray_scene(); t1 = time.perf_counter()
    res["refit_config4"] = dict(blocks(r, r.refit_ray_scene, repeats, 20 * launches), objects=len(scene4.objects), build_s=round(t1 - t0, 3),
                                tlas_nodes=info4.tlasNodes, tlas_depth=info4.tlasDepth)
    r.close()

    lines = ["tools/ray_query_time.py %d %d on %s: config 3 at %d x %d" % (repeats, launches, res["device"], w, h)]
    b = res["build"]
    lines.append("build: %.3f s host wall for %d BLASes (%d nodes, %d triangles, deepest %d levels) + TLAS (%d nodes, %d levels) + refit; a second call (TLAS only) %.4f s"
                 % (b["first_s"], b["info"]["blasCount"], b["info"]["blasNodes"], b["info"]["blasTriangles"], b["info"]["blasMaxDepth"], b["info"]["tlasNodes"],
                    b["info"]["tlasDepth"], b["second_tlas_only_s"]))
    lines.append("device bytes: ray scene %.1f MB, the scene's own arrays %.1f MB" % (b["info"]["deviceBytes"] / 1e6, b["scene_bytes"] / 1e6))
    for k in ("refit_config3", "refit_config4"):
        lines.append("%s (%d objects): median %.2f us per launch (min %.2f, max %.2f)" % (k, res[k]["objects"], res[k]["ms_median"] * 1e3, res[k]["ms_min"] * 1e3, res[k]["ms_max"] * 1e3))
    for k in ("closest_pixel_order", "closest_shuffled", "any_hit_sun"):
        lines.append("%s: %d rays, median %.3f ms (min %.3f, max %.3f): %.3f G rays/s; hit fraction %.3f"
                     % (k, res[k]["rays"], res[k]["ms_median"], res[k]["ms_min"], res[k]["ms_max"], res[k]["grays_per_s"], res[k]["hit_fraction"]))
    lines.append("the shuffled launch's hits are the ordered launch's, permuted: %s" % res["shuffled_equals_ordered"])
    res["counters"] = measure_counters()
    lines.append("tested per ray, means over the set (a -DCHORD_RAY_COUNTERS=1 build of the same kernel, one launch per set, a process of its own):")
    for k in ("closest_pixel_order", "closest_shuffled", "any_hit_sun"):
        c = res["counters"][k]
        n = float(c["rays"])
        lines.append("  %s: TLAS nodes %.2f, objects entered %.2f, BLAS nodes %.2f, triangles %.2f"
                     % (k, c["tlas_nodes"] / n, c["tlas_leaves"] / n, c["blas_nodes"] / n, c["triangles"] / n))
    lines.append(json.dumps(res))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
