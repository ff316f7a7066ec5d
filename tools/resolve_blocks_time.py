"""chordvis_resolve_material's four images at 3840 x 2160 with block-compressed textures in both texture stores
(chordvis_set_material_texture_store): CHORD_TEXSTORE_EXPANDED (RGBA8 texels, the default) against CHORD_TEXSTORE_BLOCKS (the
blocks, decoded per tap), at anisotropy 1 and 8, on two scenes:

    (a) config 3 with materials (scenes.config3_street(materials=True)), its five textures block-compressed (BC3 albedo, noise and
        emissive, BC5 normal, BC1_RGB occlusion / roughness / metallic).  Their texels are under 64 KB: every tap hits a cache, so
        the difference between the stores is the instructions the decode adds.
    (b) the same frame with each texture replaced by a 2048 x 2048 full chain of the same format (random blocks): taps miss the
        near caches, which is the case the block store is for.

One context per store lives side by side on the same frame; their timings alternate, ROUNDS times (median printed, every run
listed).  Beside each time: the store's texelBytes / blockBytes (chordvis_material_texture_memory) and the sampler taps and texel
fetches per PBR pixel (tools/resolve_time.py's count on the host).

    python tools/resolve_blocks_time.py [N] [WARMUP] [ROUNDS] [--scenes a,b] [--anisotropy 1,8]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from chord_amd import lib as L, records as R, scenes  # noqa: E402
from chord_amd.renderer import VisibilityRenderer  # noqa: E402
from resolve_time import count_taps  # noqa: E402

FORMATS = [R.TEXFMT_BC3, R.TEXFMT_BC3, R.TEXFMT_BC5, R.TEXFMT_BC1_RGB, R.TEXFMT_BC3]       # albedo, noise, normal, ORM, emissive
NAMES = list(L.MATERIAL_CHANNELS)
STORES = [("expanded", L.TEXSTORE_EXPANDED), ("blocks", L.TEXSTORE_BLOCKS)]


def scene_textures(scene, which):
    if which == "a":
        return [R.bc_chain(t, f) for t, f in zip(scene.texture_images, FORMATS)]
    rng = np.random.default_rng(7)
    return [R.TextureChain(rng.integers(0, 256, size=L.texture_chain_bytes(f, 2048, 2048, 12), dtype=np.uint8), 2048, 2048, 12, f) for f in FORMATS]


def main():
    argv = sys.argv[1:]
    pos = [int(a) for i, a in enumerate(argv) if a.isdigit() and (i == 0 or not argv[i - 1].startswith("--"))]
    n, warm, rounds = (pos + [30, 5, 5][len(pos):])[:3]
    which = argv[argv.index("--scenes") + 1].split(",") if "--scenes" in argv else ["a", "b"]
    aniso = [int(x) for x in argv[argv.index("--anisotropy") + 1].split(",")] if "--anisotropy" in argv else [1, 8]
    flags = R.FLAG_FRUSTUM_CULL | R.FLAG_CONE_CULL | R.FLAG_HZB_CULL
    base, cam = scenes.config3_street(3840, 2160, materials=True)
    L.fill_objects(base, cam)
    view, iv = L.make_views(cam)
    stream = torch.cuda.Stream()
    results = []
    with torch.cuda.stream(stream):
        for s in which:
            scene = scenes.with_textures(base, scene_textures(base, s))
            rs, outs, mem = {}, {}, {}
            for name, store in STORES:
                r = VisibilityRenderer(0, stream=stream.cuda_stream)
                r.set_material_texture_store(store)
                r.upload_scene(scene)
                r.upload_material_textures()
                r.allocate_gbuffer(cam.width, cam.height)
                r.set_view(view, iv, flags)
                r.render_frame()
                r.render_frame()
                r.sync()
                rs[name], mem[name] = r, r.material_texture_memory()
                outs[name] = r.resolve_attributes(names=NAMES)           # the targets, allocated once
            # the two stores give the same words
            for a in aniso:
                for r in rs.values():
                    r.set_material_anisotropy(a)
                x = rs["expanded"].resolve_attributes(names=NAMES, out=outs["expanded"])
                y = rs["blocks"].resolve_attributes(names=NAMES, out=outs["blocks"])
                torch.cuda.synchronize()
                assert all(torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)) for k in NAMES), (s, a)
            # (the count looks at level sizes and samplers only: a scene of the same shapes with empty RGBA8 chains)
            shapes = scenes.with_textures(base, [R.TextureChain(np.zeros(L.texture_chain_bytes(R.TEXFMT_RGBA8, t.width, t.height, t.mips), np.uint8),
                                                                t.width, t.height, t.mips) for t in scene.texture_images])
            taps = count_taps(rs["expanded"], shapes, aniso)
            ms = {(name, a): [] for name, _ in STORES for a in aniso}
            for _ in range(rounds):
                for a in aniso:
                    for name, _ in STORES:
                        r = rs[name]
                        r.set_material_anisotropy(a)
                        for _ in range(warm):
                            r.resolve_attributes(names=NAMES, out=outs[name])
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        for _ in range(n):
                            r.resolve_attributes(names=NAMES, out=outs[name])
                        e1.record(stream)
                        e1.synchronize()
                        ms[(name, a)].append(round(e0.elapsed_time(e1) / n, 4))
            med = lambda v: sorted(v)[len(v) // 2]
            for a in aniso:
                e, b = med(ms[("expanded", a)]), med(ms[("blocks", a)])
                for name, _ in STORES:
                    t = med(ms[(name, a)])
                    print("scene (%s) material@%-2d %-8s %8.4f ms   texelBytes %11d blockBytes %10d   %.2f taps, %.2f texel fetches per PBR pixel   runs %s" % (
                        s, a, name, t, mem[name][0], mem[name][1], taps[a][0], taps[a][1], ms[(name, a)]))
                    results.append(dict(scene=s, anisotropy=a, store=name, ms=t, runs=ms[(name, a)], texelBytes=mem[name][0], blockBytes=mem[name][1],
                                        sampler_taps_per_pbr_pixel=round(taps[a][0], 3), texel_fetches_per_pbr_pixel=round(taps[a][1], 3)))
                print("scene (%s) material@%-2d blocks against expanded: %+.1f %%   device bytes %.2fx smaller" % (
                    s, a, 100.0 * (b - e) / e, sum(mem["expanded"]) / max(1, sum(mem["blocks"]))))
            for r in rs.values():
                r.close()
    print(json.dumps(dict(workload="config3_materials_3840x2160_two_pass_bc", resolves=n, warmup=warm, rounds=rounds, lib=os.path.basename(L.LIB_PATH),
                          device=torch.cuda.get_device_name(0), results=results)))


if __name__ == "__main__":
    main()
