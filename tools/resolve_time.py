"""chordvis_resolve_attributes on the config 3 frame (masked twin: texture coordinates exist; with normals and tangents) at
3840 x 2160, after a two-pass frame: ms per resolve for all targets, for barycentrics + uvGrad + motion, and for the three surface
targets of chordvis_resolve_surface (vertexNormal, tangent, bitangent), bytes moved, share of 8 TB/s (MI355X peak HBM) and of
6.3 TB/s (achievable).  Times N resolves between two events on the context's stream (a torch stream handed to the context).

    python tools/resolve_time.py [N] [WARMUP]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from chord_amd import lib as L, records as R, scenes  # noqa: E402
from chord_amd.renderer import VisibilityRenderer  # noqa: E402

PEAK, ACHIEVABLE = 8.0e12, 6.3e12
SETS = {"all": list(L.RESOLVE_CHANNELS), "bary+uvGrad+motion": ["barycentrics", "uvGrad", "motionVector"], "surface": list(L.SURFACE_CHANNELS)}
CHANNELS = dict(L.RESOLVE_CHANNELS, **L.SURFACE_CHANNELS)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    warm = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    flags = R.FLAG_FRUSTUM_CULL | R.FLAG_CONE_CULL | R.FLAG_HZB_CULL
    scene, cam = scenes.config3_street(3840, 2160, masked=True, attributes=True)
    L.fill_objects(scene, cam)
    view, iv = L.make_views(cam)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        r = VisibilityRenderer(0, stream=stream.cuda_stream)
        r.upload_scene(scene)
        r.allocate_gbuffer(cam.width, cam.height)
        r.set_view(view, iv, flags)
        r.render_frame()
        r.render_frame()
        r.sync()
        covered = int(((r.read_visibility() & 0xFFFFFFFF) != 0).sum())
        lines = []
        for name, names in SETS.items():
            out = r.resolve_attributes(names=names)                  # the targets, allocated once
            for _ in range(warm):
                r.resolve_attributes(names=names, out=out)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(n):
                r.resolve_attributes(names=names, out=out)
            e1.record(stream)
            e1.synchronize()
            ms = e0.elapsed_time(e1) / n
            written = sum(4 * CHANNELS[k] for k in names)
            moved = cam.width * cam.height * (written + 8)             # every target texel written once + every visibility word read once
            lines.append(dict(targets=name, ms=round(ms, 4), bytes_per_pixel=written + 8, bytes=moved,
                              bytes_bound_ms_8tbs=round(moved / PEAK * 1e3, 4), bytes_bound_ms_6p3tbs=round(moved / ACHIEVABLE * 1e3, 4),
                              share_of_8tbs=round(moved / (ms * 1e-3) / PEAK, 3), share_of_6p3tbs=round(moved / (ms * 1e-3) / ACHIEVABLE, 3)))
    info = dict(workload="config3_masked_attributes_3840x2160_two_pass", pixels=cam.width * cam.height, covered=covered, resolves=n, warmup=warm,
                device=torch.cuda.get_device_name(0))
    for ln in lines:
        print("%-20s %8.4f ms  %3d B/px  %6.1f MB  bound %.4f ms @8 TB/s, %.4f ms @6.3 TB/s  -> %.1f %% of 8 TB/s" % (
            ln["targets"], ln["ms"], ln["bytes_per_pixel"], ln["bytes"] / 1e6, ln["bytes_bound_ms_8tbs"], ln["bytes_bound_ms_6p3tbs"],
            100.0 * ln["share_of_8tbs"]))
    print(json.dumps(dict(info, results=lines)))
    r.close()


if __name__ == "__main__":
    main()
