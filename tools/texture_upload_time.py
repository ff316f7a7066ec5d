"""chordvis_upload_material_textures on a set of 2048 x 2048 full-chain textures (12 levels each), given as block-compressed
chains (BC3, BC1_RGB, BC5, BC4 in turn; random block bytes: every byte pattern is a valid block) and as their spec-decoded RGBA8
twin: host milliseconds per call (the call is synchronous), median of N calls after WARMUP.

    python tools/texture_upload_time.py [TEXTURES] [N] [WARMUP]
    python tools/texture_upload_time.py [TEXTURES] [N] [WARMUP] --compare OTHER_LIB [ROUNDS]
    python tools/texture_upload_time.py [TEXTURES] [N] [WARMUP] --set bc|rgba8        (one set, one JSON line: what --compare runs)

--compare OTHER_LIB: fresh processes alternate this library on the BC set, this library on the RGBA8 twin, OTHER_LIB on the RGBA8
twin and OTHER_LIB on it again (ROUNDS times, default 3): the BC upload against an earlier library's RGBA8 upload of the same
content, and that library against itself (the spread of the run).  An earlier library reads ChordTexture::format as padding, so
it is only ever given the RGBA8 twin.
The decode kernel's own time is not in these numbers' resolution: take it from `rocprofv3 --kernel-trace --stats -- python
tools/texture_upload_time.py 8 3 1 --set bc` (texture_decode_kernel); the tool prints the bytes it stores per call.
After the timed calls every --set run reads level 0 of the last texture back and compares it with the spec's decode (--no-check: not).
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

SIZE, FORMATS = 2048, (2, 1, 4, 3)


def build(count, which):
    import spec_texture_bc_np as BC
    from chord_amd import records as R, scenes
    rng = np.random.default_rng(17)
    mips = SIZE.bit_length()
    textures, compressed, texels = [], 0, 0
    for i in range(count):
        f = FORMATS[i % len(FORMATS)]
        data = rng.integers(0, 256, size=BC.chain_bytes(SIZE, SIZE, mips, f), dtype=np.uint8)
        compressed += len(data)
        texels += BC.chain_bytes(SIZE, SIZE, mips, BC.RGBA8) // 4
        if which == "rgba8":
            textures.append(R.TextureChain(BC.chain_rgba8(data, SIZE, SIZE, mips, f), SIZE, SIZE, mips, BC.RGBA8))
        else:
            textures.append(R.TextureChain(data, SIZE, SIZE, mips, f))
    base, _ = scenes.small_test_scene(64, 48, lods=1)
    mats = np.zeros(count, dtype=R.MATERIAL)
    mats[:] = base.materials[0]
    mats["alphaMode"] = R.ALPHA_OPAQUE
    mats["baseColorId"] = np.arange(count)
    for s in ("emissiveTexture", "normalTexture", "metallicRoughnessTexture"):
        mats[s] = 0xFFFFFFFF
    objs = base.objects.copy()
    objs["GLTFMaterialData"] = 0
    scene = R.Scene(objs, base.primitives, mats, base.meshlets, base.groups, base.group_indices, base.meshlet_data, base.positions,
                    textures=textures, bvh_nodes=base.bvh_nodes)
    return scene, compressed, texels


def one_set(count, n, warm, which):
    from chord_amd.renderer import VisibilityRenderer
    scene, compressed, texels = build(count, which)
    r = VisibilityRenderer(0)
    r.upload_scene(scene)
    ms = []
    for k in range(warm + n):
        t0 = time.perf_counter()
        r.upload_material_textures()
        t1 = time.perf_counter()
        if k >= warm:
            ms.append((t1 - t0) * 1e3)
    # the texels the timed calls left behind, at the size timed: level 0 of the last texture against the spec's decode
    checked = None
    if hasattr(r, "readback_material_texture") and "--no-check" not in sys.argv:
        import spec_texture_bc_np as BC
        t = scene.texture_images[-1]
        n0 = BC.level_bytes(t.width, t.height, t.format)
        want = t.data[:n0].reshape(t.height, t.width, 4) if t.format == BC.RGBA8 else BC.decode_level(t.data[:n0], t.width, t.height, t.format)
        try:
            checked = bool(np.array_equal(r.readback_material_texture(len(scene.texture_images) - 1, 0), want))
        except AttributeError:
            checked = None                                # an earlier library: no read-back entry point
        if checked is False:
            raise SystemExit("texture %d level 0 differs from the spec's decode" % (len(scene.texture_images) - 1))
    r.close()
    ms.sort()
    return dict(level0_equals_spec=checked, set=which, textures=count, size=SIZE, calls=n, ms_median=round(ms[len(ms) // 2], 3), ms_min=round(ms[0], 3), ms_max=round(ms[-1], 3),
                host_bytes=compressed if which == "bc" else texels * 4, texel_bytes_stored=texels * 4)


def compare(count, n, warm, other, rounds):
    from chord_amd import lib as L
    runs = [("this_bc", L.LIB_PATH, "bc"), ("this_rgba8", L.LIB_PATH, "rgba8"), ("otherA_rgba8", other, "rgba8"), ("otherB_rgba8", other, "rgba8")]
    ms = {k: [] for k, _, _ in runs}
    info = {}
    for _ in range(rounds):
        for key, path, which in runs:
            env = dict(os.environ, CHORDVIS_LIB=path, CHORDVIS_AB_OLD_LIB="1")
            out = subprocess.run([sys.executable, os.path.abspath(__file__), str(count), str(n), str(warm), "--set", which], env=env,
                                 capture_output=True, text=True, timeout=900)
            if out.returncode != 0:
                raise SystemExit("child failed (%s): %s" % (key, out.stderr[-2000:]))
            line = json.loads(out.stdout.strip().splitlines()[-1])
            ms[key].append(line["ms_median"])
            info[key] = line
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    a, b = med["otherA_rgba8"], med["otherB_rgba8"]
    print("%d textures of %d x %d, full chains: host bytes BC %.1f MB, RGBA8 %.1f MB" % (
        count, SIZE, SIZE, info["this_bc"]["host_bytes"] / 1e6, info["this_rgba8"]["host_bytes"] / 1e6))
    print("this, BC          %9.3f ms   runs %s" % (med["this_bc"], ms["this_bc"]))
    print("this, RGBA8 twin  %9.3f ms   runs %s" % (med["this_rgba8"], ms["this_rgba8"]))
    print("other, RGBA8 twin %9.3f / %.3f ms (itself against itself: %+.2f %%)   runs %s" % (a, b, 100.0 * (b - a) / a, ms["otherA_rgba8"] + ms["otherB_rgba8"]))
    print("this BC against other RGBA8: %+.2f %%; this RGBA8 against other RGBA8: %+.2f %%" % (
        100.0 * (med["this_bc"] - min(a, b)) / min(a, b), 100.0 * (med["this_rgba8"] - min(a, b)) / min(a, b)))
    print(json.dumps(dict(compare=ms, medians=med, other=os.path.basename(other), rounds=rounds, textures=count, size=SIZE)))


def main():
    argv = sys.argv[1:]
    pos = []
    for a in argv:
        if not a.isdigit():
            break
        pos.append(int(a))
    count, n, warm = (pos + [8, 5, 1][len(pos):])[:3]
    if "--compare" in argv:
        i = argv.index("--compare")
        rounds = int(argv[i + 2]) if len(argv) > i + 2 and argv[i + 2].isdigit() else 3
        compare(count, n, warm, argv[i + 1], rounds)
        return
    sets = [argv[argv.index("--set") + 1]] if "--set" in argv else ["bc", "rgba8"]
    for which in sets:
        print(json.dumps(one_set(count, n, warm, which)))


if __name__ == "__main__":
    main()
