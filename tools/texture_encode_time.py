"""chordvis_upload_material_textures on TEXTURES 2048 x 2048 RGBA8 level-0 textures (default 16) with levels = FULL: host
milliseconds per call (the call is synchronous), median of N calls after WARMUP, and chordvis_material_texture_memory, for

    expanded      mode EXPANDED, nothing encoded: the 12-level chains stay RGBA8 texels
    blocks_bc3    mode BLOCKS with BC3 targets (chordvis_set_texture_compress): made, then encoded on the device
    blocks_bc1    mode BLOCKS with BC1_RGB targets
    supplied_bc3  mode BLOCKS, the same chains compressed beforehand on the host (tests/spec_texture_encode_np.py) and supplied as BC3

    python tools/texture_encode_time.py [TEXTURES] [N] [WARMUP]

The textures share one random host image: the copies and the kernels do the work of TEXTURES textures.  After the timed calls one
level of the last texture of the encoded sets is read back as blocks and compared with the numpy spec.  The kernel's own time:
rocprofv3 --kernel-trace --stats -- python tools/texture_encode_time.py 16 1 0, in a run of its own."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from texture_mips_time import SIZE, scene_of  # noqa: E402

CHECK_LEVEL = 3


def encode_level(E, img, format, chunk=1 << 15):
    blocks = E.fill_blocks(img)
    return np.concatenate([E.encode_blocks(blocks[i:i + chunk], format).reshape(-1) for i in range(0, len(blocks), chunk)])


def main():
    from chord_amd import lib as L, records as R
    from chord_amd.renderer import VisibilityRenderer
    import spec_texture_encode_np as E
    import spec_texture_mips_np as M
    pos = [int(a) for a in sys.argv[1:] if a.isdigit()]
    count, n, warm = (pos + [16, 7, 2][len(pos):])[:3]
    img = np.random.default_rng(3).integers(0, 256, size=(SIZE, SIZE, 4), dtype=np.uint8)
    levels = M.build_chain([img], M.FULL)
    mips = len(levels)
    bc3 = np.concatenate([encode_level(E, l, E.BC3) for l in levels])
    alone = scene_of([R.TextureChain(img.reshape(-1), SIZE, SIZE, 1)] * count)
    supplied = scene_of([R.TextureChain(bc3, SIZE, SIZE, mips, E.BC3)] * count)
    full = [(L.TEXMIPS_FULL, 0, 0)] * count
    sets = [("expanded", alone, L.TEXSTORE_EXPANDED, full, None), ("blocks_bc3", alone, L.TEXSTORE_BLOCKS, full, E.BC3),
            ("blocks_bc1", alone, L.TEXSTORE_BLOCKS, full, E.BC1_RGB), ("supplied_bc3", supplied, L.TEXSTORE_BLOCKS, None, None)]
    for name, scene, store, settings, target in sets:
        r = VisibilityRenderer(0)
        r.set_material_texture_store(store)
        r.set_texture_mips(settings)
        r.set_texture_compress([target] * count if target else None)
        r.upload_scene(scene)
        ms = []
        for k in range(warm + n):
            t0 = time.perf_counter()
            r.upload_material_textures()
            t1 = time.perf_counter()
            if k >= warm:
                ms.append((t1 - t0) * 1e3)
        texel_bytes, block_bytes = r.material_texture_memory()
        checked = None
        if target or name == "supplied_bc3":
            f = target or E.BC3
            got = r.readback_material_blocks(count - 1, f, mips)
            at = sum(L.texture_chain_bytes(f, max(1, SIZE >> l), max(1, SIZE >> l), 1) for l in range(CHECK_LEVEL))
            want = encode_level(E, levels[CHECK_LEVEL], f)
            checked = bool(np.array_equal(got[at:at + len(want)], want))
            if not checked:
                raise SystemExit("%s: level %d of the last texture differs from the spec" % (name, CHECK_LEVEL))
        r.close()
        ms.sort()
        print(json.dumps(dict(set=name, textures=count, size=SIZE, calls=n, ms_median=round(ms[len(ms) // 2], 3), ms_min=round(ms[0], 3),
                              ms_max=round(ms[-1], 3), texel_bytes=texel_bytes, block_bytes=block_bytes, level_equals_spec=checked)), flush=True)


if __name__ == "__main__":
    main()
