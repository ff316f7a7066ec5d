"""chordvis_resolve_attributes on the config 3 frame (masked twin: texture coordinates exist; with normals and tangents) at
3840 x 2160, after a two-pass frame: ms per resolve for all targets, for barycentrics + uvGrad + motion, and for the three surface
targets of chordvis_resolve_surface (vertexNormal, tangent, bitangent), bytes moved, share of 8 TB/s (MI355X peak HBM) and of
6.3 TB/s (achievable).  Times N resolves between two events on the context's stream (a torch stream handed to the context).

    python tools/resolve_time.py [N] [WARMUP]
    python tools/resolve_time.py [N] [WARMUP] --materials [--sets a,b] [--compare OTHER_LIB [ROUNDS]]

--materials: config 3 under the textured materials (scenes.config3_street(materials=True)) and two more sets: `material` (the four
images of chordvis_resolve_material) and `everything` (all fifteen).  Their bytes column counts the image bytes only (the texels
fetched come on top: a gather, see profiles/resolve_material_config3_4k_time.txt).
--compare OTHER_LIB: the sets `all` and `surface` measured in fresh processes that alternate this library, OTHER_LIB and OTHER_LIB
again (ROUNDS times, default 3): this library against the other one, and the other one against itself (the spread of the run).
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
MATERIAL = dict(getattr(L, "MATERIAL_CHANNELS", {}))
MATERIAL_SETS = {"material": list(MATERIAL), "everything": list(L.RESOLVE_CHANNELS) + list(L.SURFACE_CHANNELS) + list(MATERIAL)}
CHANNELS = dict(L.RESOLVE_CHANNELS, **L.SURFACE_CHANNELS, **MATERIAL)


def compare(argv, other, rounds):
    """alternating fresh processes: (this, other, other) x rounds over the existing sets"""
    import subprocess
    libs = [("this", L.LIB_PATH), ("otherA", other), ("otherB", other)]
    ms = {k: {"all": [], "surface": []} for k, _ in libs}
    for _ in range(rounds):
        for key, path in libs:
            env = dict(os.environ, CHORDVIS_LIB=path, CHORDVIS_AB_OLD_LIB="1")
            out = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv + ["--materials", "--sets", "all,surface"], env=env,
                                 capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise SystemExit("child failed (%s): %s" % (key, out.stderr[-2000:]))
            for ln in json.loads(out.stdout.strip().splitlines()[-1])["results"]:
                ms[key][ln["targets"]].append(ln["ms"])
    med = lambda v: sorted(v)[len(v) // 2]
    for name in ("all", "surface"):
        a, b, t = med(ms["otherA"][name]), med(ms["otherB"][name]), med(ms["this"][name])
        print("%-8s this %.4f ms | other %.4f / %.4f ms (itself against itself: %+.2f %%) | this against other %+.2f %%   runs this %s other %s" % (
            name, t, a, b, 100.0 * (b - a) / a, 100.0 * (t - min(a, b)) / min(a, b), ms["this"][name], ms["otherA"][name] + ms["otherB"][name]))
    print(json.dumps(dict(compare=ms, other=os.path.basename(other), rounds=rounds)))


def main():
    argv = sys.argv[1:]
    pos = [a for a in argv if a.isdigit()]
    n = int(pos[0]) if len(pos) > 0 else 50
    warm = int(pos[1]) if len(pos) > 1 else 5
    materials = "--materials" in argv
    sets = dict(SETS, **MATERIAL_SETS) if materials else SETS
    if "--sets" in argv:
        sets = {k: sets[k] for k in argv[argv.index("--sets") + 1].split(",")}
    if "--compare" in argv:
        i = argv.index("--compare")
        rounds = int(argv[i + 2]) if len(argv) > i + 2 and argv[i + 2].isdigit() else 3
        sets = {k: v for k, v in sets.items() if k in MATERIAL_SETS}
    flags = R.FLAG_FRUSTUM_CULL | R.FLAG_CONE_CULL | R.FLAG_HZB_CULL
    scene, cam = scenes.config3_street(3840, 2160, materials=True) if materials else scenes.config3_street(3840, 2160, masked=True, attributes=True)
    L.fill_objects(scene, cam)
    view, iv = L.make_views(cam)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        r = VisibilityRenderer(0, stream=stream.cuda_stream)
        r.upload_scene(scene)
        if any(k in MATERIAL for names in sets.values() for k in names):
            r.upload_material_textures()
        r.allocate_gbuffer(cam.width, cam.height)
        r.set_view(view, iv, flags)
        r.render_frame()
        r.render_frame()
        r.sync()
        covered = int(((r.read_visibility() & 0xFFFFFFFF) != 0).sum())
        lines = []
        for name, names in sets.items():
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
    info = dict(workload="config3_materials_3840x2160_two_pass" if materials else "config3_masked_attributes_3840x2160_two_pass", pixels=cam.width * cam.height, covered=covered, resolves=n, warmup=warm,
                device=torch.cuda.get_device_name(0))
    for ln in lines:
        print("%-20s %8.4f ms  %3d B/px  %6.1f MB  bound %.4f ms @8 TB/s, %.4f ms @6.3 TB/s  -> %.1f %% of 8 TB/s" % (
            ln["targets"], ln["ms"], ln["bytes_per_pixel"], ln["bytes"] / 1e6, ln["bytes_bound_ms_8tbs"], ln["bytes_bound_ms_6p3tbs"],
            100.0 * ln["share_of_8tbs"]))
    print(json.dumps(dict(info, results=lines)))
    r.close()
    if "--compare" in argv:
        compare([str(n), str(warm)], argv[argv.index("--compare") + 1], rounds)


if __name__ == "__main__":
    main()
