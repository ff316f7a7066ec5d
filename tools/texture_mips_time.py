"""chordvis_upload_material_textures on TEXTURES 2048 x 2048 RGBA8 textures (default 16): host milliseconds per call (the call is
synchronous), median of N calls after WARMUP, for

    level0        level 0 alone, nothing generated (mipCount 1 downstream)
    generated     level 0 alone, levels = FULL under flags 0: the other 11 levels made on the device
    generated_sc  the same under SRGB | COVERAGE (cutoff 128)
    host_chain    the full 12-level chain built on the host (records.mip_chain_rgba8) and copied

    python tools/texture_mips_time.py [TEXTURES] [N] [WARMUP]

The textures share one random host image (and one host chain): the copies and the kernels do the work of TEXTURES textures.  After
the timed calls the last level of the last texture of the generated sets is read back and compared with the numpy spec."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

SIZE = 2048


def scene_of(textures):
    from chord_amd import records as R, scenes
    count = len(textures)
    base, _ = scenes.small_test_scene(64, 48, lods=1)
    mats = np.zeros(count, dtype=R.MATERIAL)
    mats[:] = base.materials[0]
    mats["alphaMode"] = R.ALPHA_OPAQUE
    mats["baseColorId"] = np.arange(count)
    for s in ("emissiveTexture", "normalTexture", "metallicRoughnessTexture"):
        mats[s] = 0xFFFFFFFF
    objs = base.objects.copy()
    objs["GLTFMaterialData"] = 0
    return R.Scene(objs, base.primitives, mats, base.meshlets, base.groups, base.group_indices, base.meshlet_data, base.positions,
                   textures=textures, bvh_nodes=base.bvh_nodes)


def main():
    from chord_amd import lib as L, records as R
    from chord_amd.renderer import VisibilityRenderer
    import spec_texture_mips_np as M
    pos = [int(a) for a in sys.argv[1:] if a.isdigit()]
    count, n, warm = (pos + [16, 7, 2][len(pos):])[:3]
    img = np.random.default_rng(3).integers(0, 256, size=(SIZE, SIZE, 4), dtype=np.uint8)
    chain, mips = R.mip_chain_rgba8(img)
    alone = scene_of([R.TextureChain(img.reshape(-1), SIZE, SIZE, 1)] * count)
    whole = scene_of([R.TextureChain(chain, SIZE, SIZE, mips)] * count)
    sets = [("level0", alone, None, 0, 0), ("generated", alone, [(L.TEXMIPS_FULL, 0, 0)] * count, 0, 0),
            ("generated_sc", alone, [(L.TEXMIPS_FULL, 3, 128)] * count, 3, 128), ("host_chain", whole, None, 0, 0)]
    for name, scene, settings, flags, cutoff in sets:
        r = VisibilityRenderer(0)
        r.set_texture_mips(settings)
        r.upload_scene(scene)
        ms = []
        for k in range(warm + n):
            t0 = time.perf_counter()
            r.upload_material_textures()
            t1 = time.perf_counter()
            if k >= warm:
                ms.append((t1 - t0) * 1e3)
        checked = None
        if settings:
            want = M.build_chain([img], M.FULL, flags, cutoff)
            checked = all(bool(np.array_equal(r.readback_material_texture(count - 1, l), want[l])) for l in (1, 5, mips - 1))
            if not checked:
                raise SystemExit("%s: a generated level differs from the spec" % name)
        r.close()
        ms.sort()
        print(json.dumps(dict(set=name, textures=count, size=SIZE, calls=n, ms_median=round(ms[len(ms) // 2], 3), ms_min=round(ms[0], 3),
                              ms_max=round(ms[-1], 3), levels_equal_spec=checked)), flush=True)


if __name__ == "__main__":
    main()
