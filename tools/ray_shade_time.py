"""What shading ray hits costs (chordvis_shade_ray_hits) on BASELINE config 3 under the textured materials
(scenes.config3_street(materials=True)) at 3840 x 2160 -- recorded, not gated: there is no earlier figure for a capability that did
not exist.  Three hit sets:

    pixel_order   the hits of one pixel-centre ray per pixel (chordvis_trace_rays), in pixel order
    shuffled      the same hits in the fixed shuffled order tools/ray_query_time.py uses
    alternating   the valid hits arranged so that neighbouring lanes name different materials: hit k of material m sits at k x M + m

each shaded in both texture stores (the five textures block-compressed as in tools/resolve_blocks_time.py scene (a), kept as
blocks or expanded at upload), at one level for every hit (LOD) and at a level per hit, log2 of the hit's t (a ray cone's
footprint).  Each figure: WARMUP untimed launches, then REPEATS blocks of LAUNCHES launches between two events on the context's
stream; the median block, and the spread (min .. max), per launch.  Beside them the yardsticks of the same scene, measured the same
way in the same run: the primary trace and the 4K material resolve (chordvis_resolve_material, four images).

The two stores' records are compared word for word on every set.  Everything runs on a caller-owned stream.  The library is the one
chord_amd loads (CHORDVIS_LIB names another build); --label NAME goes into the report.

    python tools/ray_shade_time.py [REPEATS] [LAUNCHES] [--label NAME] [--out PATH]
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
from ray_query_time import pixel_rays  # noqa: E402

WARMUP = 3
LOD = 1.5
FORMATS = [R.TEXFMT_BC3, R.TEXFMT_BC3, R.TEXFMT_BC5, R.TEXFMT_BC1_RGB, R.TEXFMT_BC3]       # albedo, noise, normal, ORM, emissive
STORES = [("expanded", L.TEXSTORE_EXPANDED), ("blocks", L.TEXSTORE_BLOCKS)]


def blocks(stream, call, repeats, launches):
    """ms per launch: the blocks' median, min and max."""
    for _ in range(WARMUP):
        call()
    stream.synchronize()
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


def alternating(hits, materials_of_object):
    """The valid hits, hit k of the m-th distinct material at position k x M + m (the tail holds the materials with more hits)."""
    valid = torch.nonzero((hits[:, 7] & 1) != 0).reshape(-1)
    mat = materials_of_object[hits[valid, 3].long()]
    ids, inverse = torch.unique(mat, return_inverse=True)
    order = torch.argsort(inverse, stable=True)
    counts = torch.bincount(inverse, minlength=len(ids))
    starts = torch.cumsum(counts, 0) - counts
    rank = torch.arange(len(order), device=hits.device) - starts[inverse[order]]
    key = rank * len(ids) + inverse[order]
    return hits[valid[order[torch.argsort(key)]]].contiguous(), len(ids)


def main():
    argv = sys.argv[1:]
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "ray_shade_time.txt")
    label = argv[argv.index("--label") + 1] if "--label" in argv else "product"
    nums = [int(a) for i, a in enumerate(argv) if a.isdigit() and (i == 0 or not argv[i - 1].startswith("--"))]
    repeats, launches = (nums + [9, 5][len(nums):])[:2]
    dev = torch.device("cuda", 0)
    w, h = 3840, 2160
    flags = R.FLAG_FRUSTUM_CULL | R.FLAG_CONE_CULL | R.FLAG_HZB_CULL
    res = {"label": label, "library": os.path.basename(L.LIB_PATH), "repeats": repeats, "launches": launches, "device": torch.cuda.get_device_name(0), "lod": LOD}

    base, cam = scenes.config3_street(w, h, materials=True)
    L.fill_objects(base, cam)
    view, iv = L.make_views(cam)
    scene = scenes.with_textures(base, [R.bc_chain(t, f) for t, f in zip(base.texture_images, FORMATS)])
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        rs = {}
        for name, store in STORES:
            r = VisibilityRenderer(0, stream=stream.cuda_stream)
            r.set_material_texture_store(store)
            r.upload_scene(scene)
            r.upload_material_textures()
            rs[name] = r
        r = rs["expanded"]
        r.build_ray_scene()
        rays = pixel_rays(view, w, h, dev)
        n = w * h
        hits = torch.empty((n, 8), dtype=torch.int32, device=dev)
        res["trace_pixel_order"] = blocks(stream, lambda: r.trace_rays(rays, out=hits), repeats, launches)
        del rays
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(dev)
        objmat = torch.from_numpy(scene.objects["GLTFMaterialData"].astype(np.int64)).to(dev)
        alt, distinct = alternating(hits, objmat)
        sets = [("pixel_order", hits), ("shuffled", hits[perm].contiguous()), ("alternating", alt)]
        res["hit_fraction"] = round(float((hits[:, 7] & 1).float().mean()), 4)
        res["materials_met"] = distinct
        del perm
        surf = {name: torch.empty((n, 16), dtype=torch.int32, device=dev) for name, _ in STORES}
        res["sets"] = {}
        for sname, hh in sets:
            m = len(hh)
            lods = torch.log2(torch.clamp(hh[:, 0].view(torch.float32), min=1e-3)).contiguous()
            entry = {"hits": m}
            for mode, kw in (("uniform", dict(lod=LOD)), ("per_hit", dict(lods=lods))):
                for name, _ in STORES:
                    b = blocks(stream, lambda: rs[name].shade_ray_hits(hh, out=surf[name][:m], **kw), repeats, launches)
                    b["ghits_per_s"] = round(m / (b["ms_median"] * 1e-3) / 1e9, 4)
                    # the streams every hit moves whatever it names: its record in, its level in, the surface record out
                    b["stream_bytes_per_hit"] = 32 + (4 if mode == "per_hit" else 0) + 64
                    b["stream_gb_per_s"] = round(b["stream_bytes_per_hit"] * m / (b["ms_median"] * 1e-3) / 1e9, 1)
                    entry["%s_%s" % (mode, name)] = b
                stream.synchronize()
                entry["%s_stores_agree" % mode] = bool(torch.equal(surf["expanded"][:m], surf["blocks"][:m]))
            flags_word = surf["expanded"][:m, 15]
            entry["valid_fraction"] = round(float((flags_word & 1).float().mean()), 4)
            entry["pbr_fraction"] = round(float(((flags_word & 8) != 0).float().mean()), 4)
            res["sets"][sname] = entry
            del lods
        del sets, alt, surf
        # the second yardstick: the four material images of a frame of the same scene
        r.allocate_gbuffer(w, h)
        r.set_view(view, iv, flags)
        r.render_frame()
        r.render_frame()
        names = list(L.MATERIAL_CHANNELS)
        images = r.resolve_attributes(names=names)
        res["resolve_material_4_images"] = blocks(stream, lambda: r.resolve_attributes(names=names, out=images), repeats, launches)
        res["texture_memory"] = {name: list(rs[name].material_texture_memory()) for name, _ in STORES}
        del images, hits, objmat
        stream.synchronize()
    for r in rs.values():
        r.close()

    lines = ["tools/ray_shade_time.py %d %d on %s: config 3 with materials at %d x %d, library %s (%s)"
             % (repeats, launches, res["device"], w, h, res["library"], label)]
    t, m4 = res["trace_pixel_order"], res["resolve_material_4_images"]
    lines.append("yardsticks, same run: primary trace %.3f ms (min %.3f, max %.3f); material resolve, four images %.3f ms (min %.3f, max %.3f)"
                 % (t["ms_median"], t["ms_min"], t["ms_max"], m4["ms_median"], m4["ms_min"], m4["ms_max"]))
    lines.append("hit fraction %.3f; %d distinct materials met; uniform level %.2f, per-hit level log2(t)" % (res["hit_fraction"], res["materials_met"], LOD))
    for sname, e in res["sets"].items():
        lines.append("%s: %d hits, valid %.3f, PBR %.3f; the two stores agree word for word: uniform %s, per-hit %s"
                     % (sname, e["hits"], e["valid_fraction"], e["pbr_fraction"], e["uniform_stores_agree"], e["per_hit_stores_agree"]))
        for mode in ("uniform", "per_hit"):
            for name, _ in STORES:
                b = e["%s_%s" % (mode, name)]
                lines.append("  %-8s %-8s median %.3f ms (min %.3f, max %.3f): %.2f G hits/s; %d stream bytes per hit in + out: %.0f GB/s"
                             % (mode, name, b["ms_median"], b["ms_min"], b["ms_max"], b["ghits_per_s"], b["stream_bytes_per_hit"], b["stream_gb_per_s"]))
    lines.append("gathered per valid hit beside the streams: 72 bytes of its object record, 8 of its meshlet, four meshlet-data words, three vertices' "
                 "uv and normal (60 bytes), the material's factors and the words of up to three slots, and 1 to 8 texels (or their blocks) per slot")
    lines.append(json.dumps(res))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
