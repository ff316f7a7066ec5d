"""chordvis_resolve_attributes on the config 3 frame (masked twin: texture coordinates exist; with normals and tangents) at
3840 x 2160, after a two-pass frame: ms per resolve for all targets, for barycentrics + uvGrad + motion, and for the three surface
targets of chordvis_resolve_surface (vertexNormal, tangent, bitangent), bytes moved, share of 8 TB/s (MI355X peak HBM) and of
6.3 TB/s (achievable).  Times N resolves between two events on the context's stream (a torch stream handed to the context).

    python tools/resolve_time.py [N] [WARMUP]
    python tools/resolve_time.py [N] [WARMUP] --materials [--sets a,b] [--compare OTHER_LIB [ROUNDS]] [--compare-sets a,b]
    python tools/resolve_time.py [N] [WARMUP] --materials --sets material --anisotropy 1,8,16 [--taps]
    python tools/resolve_time.py [N] [WARMUP] --materials --sets gbuffer,gbuffer_float --alternate 5
    python tools/resolve_time.py [N] [WARMUP] --materials --sets material --feedback 1,2,4

--materials: config 3 under the textured materials (scenes.config3_street(materials=True)) and two more sets: `material` (the four
images of chordvis_resolve_material) and `everything` (all fifteen).  Their bytes column counts the image bytes only (the texels
fetched come on top: a gather, see profiles/resolve_material_config3_4k_time.txt).
Two more sets under --materials: `gbuffer` (the six packed images of chordvis_resolve_gbuffer, 28 bytes per pixel) and `gbuffer_float`
(the same six as float images through chordvis_resolve_material, 88 bytes per pixel).
--alternate R: the chosen sets are timed R times in turn (a, b, a, b, ...) in the one process; a set's line reports the median and
lists every run.
--compare OTHER_LIB: the sets `all` and `surface` measured in fresh processes that alternate this library, OTHER_LIB and OTHER_LIB
again (ROUNDS times, default 3): this library against the other one, and the other one against itself (the spread of the run).
--compare-sets a,b: the sets compared (default all,surface), e.g. `material` at the default anisotropy of 1.
--anisotropy A,B,...: every chosen set that holds a material image is timed once per value, under
chordvis_set_material_anisotropy (its line is named set@value); the other sets are timed once.
--taps: per value, the sampler taps and the texel fetches the pinned sampler requests per PBR pixel of the frame, counted on the
host by tests/spec_material_aniso_np.py's tap_plan from the uv gradients the device resolved (no texel is read).
--feedback S,T,...: after the sets, chordvis_material_feedback at slotMask 15 is timed once per stride (offset 0, 0), the same way
(its line is named feedback/stride; the buffer is reset before each timed run), and the counts of the first stride are printed.
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
GBUFFER = dict(getattr(L, "GBUFFER_IMAGES", {}))
MATERIAL_SETS.update({"gbuffer": list(GBUFFER), "gbuffer_float": [src for src, _ in GBUFFER.values()]})
CHANNELS = dict(L.RESOLVE_CHANNELS, **L.SURFACE_CHANNELS, **MATERIAL)


def count_taps(r, scene, values):
    """{value: (sampler taps, texel fetches) per PBR pixel} over the textured slots of the frame r holds"""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import spec_material_aniso_np as SA
    import spec_material_np as SM
    g = r.resolve_attributes(names=["uvGrad"])["uvGrad"]
    torch.cuda.synchronize()
    grad = g.cpu().numpy().reshape(-1, 4)
    mat = SM.material_of_pixels(scene, r.read_visibility(), r.read_cmds(r.last_frame_cmds()))
    out = {}
    for n in values:
        taps = fetches = pbr = 0
        for m in np.unique(mat[mat >= 0]):
            M = scene.materials[m]
            if int(M["materialType"]) != SM.PBR_TYPE:
                continue
            pix = np.nonzero(mat == m)[0]
            pbr += len(pix)
            for slot in SM.SLOTS:
                levels, smp = SM.slot_texture(scene, M, slot)
                if levels is None:
                    continue
                p = SA.tap_plan(grad[pix], levels[0].shape[1], levels[0].shape[0], n)
                minified, last = p["lmaj"] > 0, len(levels) - 1
                lin = lambda f: f in (SM.LINEAR, SM.LINEAR_MIPMAP_NEAREST, SM.LINEAR_MIPMAP_LINEAR)
                per_level = np.where(minified, 4 if lin(smp[0]) else 1, 4 if lin(smp[1]) else 1)
                two = minified & (smp[0] in (SM.NEAREST_MIPMAP_LINEAR, SM.LINEAR_MIPMAP_LINEAR)) & ((p["lodq"] >> 8) < last)
                n_taps = np.int64(1) << p["k"]
                taps += int(n_taps.sum())
                fetches += int((n_taps * per_level * np.where(two, 2, 1)).sum())
        out[n] = (taps / max(pbr, 1), fetches / max(pbr, 1), pbr)
    return out


def compare(argv, other, rounds, names):
    """alternating fresh processes: (this, other, other) x rounds over `names`"""
    import subprocess
    libs = [("this", L.LIB_PATH), ("otherA", other), ("otherB", other)]
    ms = {k: {n: [] for n in names} for k, _ in libs}
    for _ in range(rounds):
        for key, path in libs:
            env = dict(os.environ, CHORDVIS_LIB=path, CHORDVIS_AB_OLD_LIB="1")
            out = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv + ["--materials", "--sets", ",".join(names)], env=env,
                                 capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise SystemExit("child failed (%s): %s" % (key, out.stderr[-2000:]))
            for ln in json.loads(out.stdout.strip().splitlines()[-1])["results"]:
                ms[key][ln["targets"]].append(ln["ms"])
                print("  %s %s %.4f ms" % (key, ln["targets"], ln["ms"]), file=sys.stderr, flush=True)      # (progress of a long run)
    med = lambda v: sorted(v)[len(v) // 2]
    for name in names:
        a, b, t = med(ms["otherA"][name]), med(ms["otherB"][name]), med(ms["this"][name])
        print("%-8s this %.4f ms | other %.4f / %.4f ms (itself against itself: %+.2f %%) | this against other %+.2f %%   runs this %s other %s" % (
            name, t, a, b, 100.0 * (b - a) / a, 100.0 * (t - min(a, b)) / min(a, b), ms["this"][name], ms["otherA"][name] + ms["otherB"][name]))
    print(json.dumps(dict(compare=ms, other=os.path.basename(other), rounds=rounds)))


def main():
    argv = sys.argv[1:]
    pos = [a for i, a in enumerate(argv) if a.isdigit() and (i == 0 or argv[i - 1] not in ("--anisotropy", "--alternate"))]
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
    aniso = [int(x) for x in argv[argv.index("--anisotropy") + 1].split(",")] if "--anisotropy" in argv else [None]
    flags = R.FLAG_FRUSTUM_CULL | R.FLAG_CONE_CULL | R.FLAG_HZB_CULL
    scene, cam = scenes.config3_street(3840, 2160, materials=True) if materials else scenes.config3_street(3840, 2160, masked=True, attributes=True)
    L.fill_objects(scene, cam)
    view, iv = L.make_views(cam)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        r = VisibilityRenderer(0, stream=stream.cuda_stream)
        r.upload_scene(scene)
        if any(k in MATERIAL for names in sets.values() for k in names) or "gbuffer" in sets:
            r.upload_material_textures()
        r.allocate_gbuffer(cam.width, cam.height)
        r.set_view(view, iv, flags)
        r.render_frame()
        r.render_frame()
        r.sync()
        covered = int(((r.read_visibility() & 0xFFFFFFFF) != 0).sum())
        lines = []
        runs = [(name, names, a) for name, names in sets.items() for a in (aniso if any(k in MATERIAL for k in names) else [None])]
        alternate = int(argv[argv.index("--alternate") + 1]) if "--alternate" in argv else 1
        times, outs = {}, {}
        for _ in range(alternate):
            for name, names, a in runs:
                packed = name == "gbuffer"                              # (the one set that goes through chordvis_resolve_gbuffer)
                resolve = r.resolve_gbuffer if packed else r.resolve_attributes
                if a is not None:
                    r.set_material_anisotropy(a)
                    name = "%s@%d" % (name, a)
                if name not in outs:
                    outs[name] = resolve(names=names)                # the targets, allocated once
                out = outs[name]
                for _ in range(warm):
                    resolve(names=names, out=out)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(n):
                    resolve(names=names, out=out)
                e1.record(stream)
                e1.synchronize()
                times.setdefault(name, []).append(e0.elapsed_time(e1) / n)
        for name, names, a in runs:
            packed = name == "gbuffer"
            if a is not None:
                name = "%s@%d" % (name, a)
            ms = sorted(times[name])[len(times[name]) // 2]
            written = sum((2 * GBUFFER[k][1] or 4) if packed else 4 * CHANNELS[k] for k in names)
            moved = cam.width * cam.height * (written + 8)             # every target texel written once + every visibility word read once
            lines.append(dict(targets=name, ms=round(ms, 4), bytes_per_pixel=written + 8, bytes=moved,
                              bytes_bound_ms_8tbs=round(moved / PEAK * 1e3, 4), bytes_bound_ms_6p3tbs=round(moved / ACHIEVABLE * 1e3, 4),
                              share_of_8tbs=round(moved / (ms * 1e-3) / PEAK, 3), share_of_6p3tbs=round(moved / (ms * 1e-3) / ACHIEVABLE, 3),
                              **({"runs_ms": [round(t, 4) for t in times[name]]} if alternate > 1 else {})))
    info = dict(workload="config3_materials_3840x2160_two_pass" if materials else "config3_masked_attributes_3840x2160_two_pass", pixels=cam.width * cam.height, covered=covered, resolves=n, warmup=warm,
                device=torch.cuda.get_device_name(0))
    for ln in [ln for ln in lines if "bytes" in ln]:
        print("%-20s %8.4f ms  %3d B/px  %6.1f MB  bound %.4f ms @8 TB/s, %.4f ms @6.3 TB/s  -> %.1f %% of 8 TB/s" % (
            ln["targets"], ln["ms"], ln["bytes_per_pixel"], ln["bytes"] / 1e6, ln["bytes_bound_ms_8tbs"], ln["bytes_bound_ms_6p3tbs"],
            100.0 * ln["share_of_8tbs"]) + ("   runs %s" % ln["runs_ms"] if "runs_ms" in ln else ""))
    if "--feedback" in argv:
        for stride in [int(x) for x in argv[argv.index("--feedback") + 1].split(",")]:
            with torch.cuda.stream(stream):
                r.reset_material_feedback()
                for _ in range(warm):
                    r.material_feedback(15, stride)
                r.reset_material_feedback()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(n):
                    r.material_feedback(15, stride)
                e1.record(stream)
                e1.synchronize()
            taps = r.read_material_feedback()
            ms = e0.elapsed_time(e1) / n
            lines.append(dict(targets="feedback/%d" % stride, ms=round(ms, 4), lattice_pixels=((cam.width + stride - 1) // stride) * ((cam.height + stride - 1) // stride),
                              taps_per_call=int(taps.sum()) // n, rows=[[int(v) // n for v in row[:12]] for row in taps]))
            print("%-20s %8.4f ms  %9d lattice pixels  %9d taps per call" % (lines[-1]["targets"], ms, lines[-1]["lattice_pixels"], lines[-1]["taps_per_call"]))
    if "--taps" in argv:
        info["taps"] = {}
        for a, (taps, fetches, pbr) in count_taps(r, scene, [1 if a is None else a for a in aniso]).items():
            print("anisotropy %2d: %.2f sampler taps, %.2f texel fetches per PBR pixel (%d PBR pixels)" % (a, taps, fetches, pbr))
            info["taps"][a] = dict(sampler_taps_per_pbr_pixel=round(taps, 3), texel_fetches_per_pbr_pixel=round(fetches, 3), pbr_pixels=pbr)
    print(json.dumps(dict(info, results=lines)))
    r.close()
    if "--compare" in argv:
        names = argv[argv.index("--compare-sets") + 1].split(",") if "--compare-sets" in argv else ["all", "surface"]
        compare([str(n), str(warm)], argv[argv.index("--compare") + 1], rounds, names)


if __name__ == "__main__":
    main()
