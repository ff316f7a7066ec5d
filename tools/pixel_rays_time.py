"""What pixel rays cost (chordvis_pixel_rays) on BASELINE config 3 under the textured materials
(scenes.config3_street(materials=True)) at 3840 x 2160 and at 1920 x 1080, the half-resolution buffer an AO pass commonly runs at --
recorded, not gated: there is no earlier figure for a capability that did not exist.  Per size, from the frame's own positionRS,
vertexNormal and the depth halves of its visibility image (deviceZStride 2), two passes:

    ao        HEMISPHERE, closest hit, START_FROM_DEPTH, a 128 x 128 table made here (uniformSampleHemisphere of a seeded generator)
    shadow    DIRECTION towards the sun of tools/ray_query_time.py, ANY_HIT | FRONT_ONLY, START_FROM_DEPTH

each measured four ways in the same session:

    fused         chordvis_pixel_rays, one launch, under the library's pixel-to-lane mapping (8 x 8 blocks)
    fused_rows    the same under 64 x 1 row segments: a -DCHORD_PIXEL_RAYS_ROWS=1 build (chord_amd/build.py --tag pixelrows; built
                  here if it is missing) in a child process through CHORDVIS_LIB; the child's images are compared with the parent's
    three_step    what the entry point replaces: a ray-generation step written with torch ops, chordvis_trace_rays, a torch reduction
                  of the hits to the float image
    trace_alone   chordvis_trace_rays on those rays, materialised beforehand in pixel order: the trace the fused kernel cannot beat
                  by much

Each figure: WARMUP untimed runs, then REPEATS blocks of LAUNCHES runs between two events on the context's stream; the median block
and the spread (min .. max), per run.  Everything runs on a caller-owned stream.  The torch ray generation is float32 but not the
specification's arithmetic word for word (torch fuses nothing here, but its normalize and cross differ in order): its images are
compared with the fused ones and the fraction of equal pixels is reported, not asserted.

    python tools/pixel_rays_time.py [REPEATS] [LAUNCHES] [--out PATH]
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from chord_amd import lib as L, records as R, scenes  # noqa: E402
from chord_amd.renderer import VisibilityRenderer  # noqa: E402
from ray_query_time import SUN  # noqa: E402
from ray_shade_time import blocks  # noqa: E402

SIZES = ((3840, 2160), (1920, 1080))
AO_LENGTH = 2.0                                                                # metres: a street's AO radius
SHADOW_LENGTH = 1e9
TABLE = 128


def hemisphere_table(dev):
    rng = np.random.default_rng(7)
    z = rng.random(TABLE * TABLE)
    phi = rng.random(TABLE * TABLE) * 2.0 * np.pi
    r = np.sqrt(1.0 - z * z)
    t = np.stack([r * np.cos(phi), r * np.sin(phi), z, np.zeros_like(z)], axis=1).astype(np.float32)
    return torch.from_numpy(t.reshape(TABLE, TABLE, 4)).to(dev)


def start_offset(z, z_near):
    s = (z_near / z) * 0.01
    return 5e-3 + (s / (s + 1.0)) * (1e-1 - 5e-3)


def torch_rays(pos, nrm, z, table, z_near, mode, rays):
    """The ray-generation step of the three-step path, written with torch ops into `rays` (n, 8) float32."""
    h, w = pos.shape[0], pos.shape[1]
    p = pos.reshape(-1, 4)
    n = torch.nn.functional.normalize(nrm.reshape(-1, 4)[:, :3], dim=1, eps=0.0).nan_to_num(0.0)
    valid = z > 0
    if mode == "ao":
        ys, xs = torch.meshgrid(torch.arange(h, device=pos.device), torch.arange(w, device=pos.device), indexing="ij")
        dT = table[ys.reshape(-1) & (TABLE - 1), xs.reshape(-1) & (TABLE - 1), :3]
        zb = n[:, 2].abs() > 0
        kz = torch.sqrt(n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
        kx = torch.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1])
        zero = torch.zeros_like(kz)
        u = torch.where(zb[:, None], torch.stack([zero, -n[:, 2] / kz, n[:, 1] / kz], 1), torch.stack([n[:, 1] / kx, -n[:, 0] / kx, zero], 1))
        b = torch.linalg.cross(n, u)
        d = dT[:, 0:1] * u + dT[:, 1:2] * b + dT[:, 2:3] * n
        length = AO_LENGTH
    else:
        sun = torch.tensor(SUN, dtype=torch.float32, device=pos.device)
        d = sun.expand(len(p), 3)
        valid = valid & ((n * sun).sum(1) > 0)
        length = SHADOW_LENGTH
    rays[:, :3] = p[:, :3]
    rays[:, 3] = start_offset(z, z_near)
    rays[:, 4:7] = d
    rays[:, 7] = length
    rays[~valid] = 0.0                                                          # (a zero ray is a miss)
    return valid


def torch_reduce(hits, valid, z, mode, out):
    hit = (hits[:, 7] & 1) != 0
    if mode == "ao":
        out.copy_(torch.where(hit, (hits[:, 0].view(torch.float32) / AO_LENGTH).clamp(0.0, 1.0), torch.ones_like(out)))
    else:
        # 0 in shadow -- a hit, or a covered pixel that faces away and was not traced -- and 1 otherwise
        out.copy_(torch.where(hit | ((z > 0) & ~valid), torch.zeros_like(out), torch.ones_like(out)))
    return out


def frame_images(r, scene, cam, w, h, dev):
    """(position, normal, visibility image) of two frames' second at w x h, on the current stream"""
    view, iv = L.make_views(scenes.Camera(cam.position, cam.front, w, h, fovy=cam.fovy, z_near=cam.z_near, z_far=cam.z_far, world_up=cam.world_up))
    vis = torch.zeros(w * h, dtype=torch.int64, device=dev)
    r.allocate_gbuffer(w, h, device_visibility=vis.data_ptr())
    r.set_view(view, iv, R.FLAG_FRUSTUM_CULL | R.FLAG_CONE_CULL | R.FLAG_HZB_CULL)
    r.render_frame()
    r.render_frame()
    res = r.resolve_attributes(names=["positionRS", "vertexNormal"])
    return res["positionRS"], res["vertexNormal"], vis


def fused_call(r, mode, pos, nrm, vis, table, z_near, out):
    if mode == "ao":
        return lambda: r.pixel_rays(pos, nrm, mode=L.PIXEL_RAYS_HEMISPHERE, table=table, ray_length=AO_LENGTH, z_near=z_near,
                                    depth=vis.data_ptr() + 4, depth_stride=2, start_from_depth=True, out=out)
    return lambda: r.pixel_rays(pos, nrm, mode=L.PIXEL_RAYS_DIRECTION, direction=SUN, ray_length=SHADOW_LENGTH, z_near=z_near,
                                depth=vis.data_ptr() + 4, depth_stride=2, start_from_depth=True, any_hit=True, front_only=True, out=out)


def measure(repeats, launches, child):
    dev = torch.device("cuda", 0)
    res = {"library": os.path.basename(L.LIB_PATH), "repeats": repeats, "launches": launches, "device": torch.cuda.get_device_name(0), "sizes": {}}
    scene, cam = scenes.config3_street(SIZES[0][0], SIZES[0][1], materials=True)
    L.fill_objects(scene, cam)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        r = VisibilityRenderer(0, stream=stream.cuda_stream)
        r.upload_scene(scene)
        r.build_ray_scene()
        table = hemisphere_table(dev)
        for w, h in SIZES:
            pos, nrm, vis = frame_images(r, scene, cam, w, h, dev)
            n = w * h
            z = vis.view(torch.float32)[1::2]
            out = torch.empty((h, w), dtype=torch.float32, device=dev)
            entry = {"covered": round(float((z > 0).float().mean()), 4)}
            for mode in ("ao", "shadow"):
                e = {}
                call = fused_call(r, mode, pos, nrm, vis, table, cam.z_near, out)
                e["fused"] = blocks(stream, call, repeats, launches)
                stream.synchronize()
                image = out.clone()
                e["sum_of_words"] = int(image.view(torch.int32).to(torch.int64).sum())
                e["mean"] = round(float(image.mean()), 5)
                if not child:
                    rays = torch.zeros((n, 8), dtype=torch.float32, device=dev)
                    hits = torch.empty((n, 8), dtype=torch.int32, device=dev)
                    flat = torch.empty(n, dtype=torch.float32, device=dev)
                    any_hit = mode == "shadow"

                    def three_step():
                        valid = torch_rays(pos, nrm, z, table, cam.z_near, mode, rays)
                        r.trace_rays(rays, any_hit=any_hit, out=hits)
                        torch_reduce(hits, valid, z, mode, flat)
                    e["three_step"] = blocks(stream, three_step, repeats, launches)
                    e["ray_generation_torch"] = blocks(stream, lambda: torch_rays(pos, nrm, z, table, cam.z_near, mode, rays), repeats, launches)
                    valid = torch_rays(pos, nrm, z, table, cam.z_near, mode, rays)
                    e["trace_alone"] = blocks(stream, lambda: r.trace_rays(rays, any_hit=any_hit, out=hits), repeats, launches)
                    e["reduction_torch"] = blocks(stream, lambda: torch_reduce(hits, valid, z, mode, flat), repeats, launches)
                    stream.synchronize()
                    e["traced_fraction"] = round(float(valid.float().mean()), 4)
                    e["hit_fraction_of_traced"] = round(float(((hits[:, 7] & 1) != 0).float().sum() / valid.float().sum().clamp(min=1)), 4)
                    e["three_step_equals_fused"] = round(float((flat.view(torch.int32) == image.reshape(-1).view(torch.int32)).float().mean()), 5)
                    del rays, hits, flat, valid
                entry[mode] = e
                del image
            res["sizes"]["%dx%d" % (w, h)] = entry
            del pos, nrm, vis, z, out
        del table
        stream.synchronize()
    r.close()
    return res


def measure_rows(repeats, launches):
    from chord_amd import build as B
    lib = os.path.join(B.OUT_DIR, "libchordvis_pixelrows.so")
    if not os.path.exists(lib):
        B.build(verbose=False, defines=("-DCHORD_PIXEL_RAYS_ROWS=1",), tag="pixelrows")
    env = dict(os.environ, CHORDVIS_LIB=lib)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(repeats), str(launches), "--child"], env=env, capture_output=True, text=True, timeout=900)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("PIXEL_RAYS_CHILD ")]
    if p.returncode != 0 or not line:
        raise RuntimeError("the row-mapping run failed (%d): %s" % (p.returncode, (p.stdout + p.stderr)[-2000:]))
    return json.loads(line[-1][len("PIXEL_RAYS_CHILD "):])


def fmt(b):
    return "%.3f ms (min %.3f, max %.3f)" % (b["ms_median"], b["ms_min"], b["ms_max"])


def main():
    argv = sys.argv[1:]
    nums = [int(a) for i, a in enumerate(argv) if a.isdigit() and (i == 0 or not argv[i - 1].startswith("--"))]
    repeats, launches = (nums + [9, 5][len(nums):])[:2]
    if "--child" in argv:
        print("PIXEL_RAYS_CHILD " + json.dumps(measure(repeats, launches, True)))
        return
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "pixel_rays_time.txt")
    res = measure(repeats, launches, False)
    rows = measure_rows(repeats, launches)
    res["rows_library"] = rows["library"]
    lines = ["tools/pixel_rays_time.py %d %d on %s: config 3 with materials, library %s; rows: %s" % (repeats, launches, res["device"], res["library"], rows["library"])]
    lines.append("ao: HEMISPHERE closest, rayLength %.1f, START_FROM_DEPTH, %d x %d table; shadow: DIRECTION %r, ANY_HIT | FRONT_ONLY, START_FROM_DEPTH; "
                 "position, normal and depth (deviceZStride 2) from the frame" % (AO_LENGTH, TABLE, TABLE, SUN))
    for size, entry in res["sizes"].items():
        lines.append("%s: %.1f %% of the pixels covered" % (size, 100.0 * entry["covered"]))
        for mode in ("ao", "shadow"):
            e, er = entry[mode], rows["sizes"][size][mode]
            e["fused_rows"] = er["fused"]
            e["rows_image_equal"] = er["sum_of_words"] == e["sum_of_words"] and er["mean"] == e["mean"]
            lines.append("  %-6s traced %.1f %% of the pixels, %.1f %% of them hit; mean of out %.4f" % (mode, 100.0 * e["traced_fraction"], 100.0 * e["hit_fraction_of_traced"], e["mean"]))
            lines.append("    fused, 8 x 8 blocks      %s" % fmt(e["fused"]))
            lines.append("    fused, 64 x 1 rows       %s; the two mappings' images agree (sum of words, mean): %s" % (fmt(e["fused_rows"]), e["rows_image_equal"]))
            lines.append("    three steps              %s = torch ray generation %s + trace + torch reduction %s" % (fmt(e["three_step"]), fmt(e["ray_generation_torch"]), fmt(e["reduction_torch"])))
            lines.append("    chordvis_trace_rays alone %s; %.3f %% of the three-step image's words equal the fused image's" % (fmt(e["trace_alone"]), 100.0 * e["three_step_equals_fused"]))
    lines.append("bytes per pixel: fused 16 position + 16 normal + 4 depth + 16 table (ao) in, 4 out; the trace alone 32 ray in, 32 hit out; "
                 "the three steps move the fused inputs, 32 + 32 of ray, 32 + 32 of hit and 4 out, and torch's temporaries")
    lines.append(json.dumps(res))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
