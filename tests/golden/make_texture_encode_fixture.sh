#!/bin/sh
# Regenerates texture_encode.npz with the reference's vendored stb_dxt.h (only present in the build container): the header is
# compiled where it lies, nothing of it is copied.  The input blocks come from make_texture_encode_fixture.py's classes; the
# outputs are what the reference's importer would have written for them (BC1, BC3 at HIGHQUAL; BC4 of .r; BC5 of .rg).
# The float parts of the encoder must not be contracted: the pinned build is -O2 -ffp-contract=off, and nothing is written
# unless an -O0 build gives the same bytes.
set -e
cd "$(dirname "$0")"
REF=/root/reference/external/include/stb
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
g++ -O2 -ffp-contract=off -std=c++17 -I $REF make_texture_encode_fixture.cpp -o "$TMP/enc_o2"
g++ -O0 -std=c++17 -I $REF make_texture_encode_fixture.cpp -o "$TMP/enc_o0"
python3 - "$TMP/blocks.bin" "$TMP/classes.txt" <<'PY'
import sys, numpy as np
sys.path.insert(0, "../..")
sys.path.insert(0, "..")
import spec_texture_encode_np as E
from chord_amd import scenes

rng = np.random.default_rng(20260519)
classes = []                                                    # (name, (n, 16, 4) uint8)


def add(name, blocks):
    classes.append((name, np.asarray(blocks, dtype=np.uint8).reshape(-1, 16, 4)))


def noise(n, lo=0, hi=256):
    return rng.integers(lo, hi, size=(n, 16, 4), dtype=np.uint8)


# constant blocks: every value 0..255 in each of r, g and b
v = np.arange(256)
c = np.stack([v, (v + 85) % 256, (v + 170) % 256, np.where(v % 3 == 0, 255, v)], axis=1)
add("constant", np.repeat(c[:, None, :], 16, axis=1))
# constant colour, varying alpha
b = np.repeat(noise(32)[:, :1, :], 16, axis=1)
b[:, :, 3] = rng.integers(0, 256, size=(32, 16))
add("constant_colour_varying_alpha", b)
# two colours
two = noise(128)[:, :2, :]
pick = rng.integers(0, 2, size=(128, 16))
pick[:, 0], pick[:, 1] = 0, 1
add("two_colour", two[np.arange(128)[:, None], pick])
# +-1 and +-2 noise around a base
base = rng.integers(2, 254, size=(128, 1, 4))
amp = np.where(np.arange(128) < 64, 1, 2)[:, None, None]
add("small_noise", base + rng.integers(-1, 2, size=(128, 16, 4)) * amp)
# ramps: along x, along y, along the diagonals, per channel slopes of either sign
x, y = np.tile(np.arange(4), 4), np.repeat(np.arange(4), 4)
ramps = []
for k in range(128):
    t = [x, y, x + y, x - y + 3][k % 4] / [3.0, 3.0, 6.0, 6.0][k % 4]
    a, e = rng.integers(0, 256, size=4), rng.integers(0, 256, size=4)
    ramps.append(np.rint(a[None, :] + (e - a)[None, :] * t[:, None]))
add("ramp", np.array(ramps))
add("full_noise", noise(256))
# channel ranges: dist = 0, 1..7, 8, 255 in r, g and alpha
ch = []
for dist in [0, 1, 2, 3, 4, 5, 6, 7, 8, 255] * 6:
    lo = 0 if dist == 255 else int(rng.integers(0, 256 - dist))
    blk = rng.integers(lo, lo + dist + 1, size=(16, 4))
    blk[0], blk[1] = lo, lo + dist
    ch.append(blk)
add("channel_ranges", np.array(ch))
# 0 / 255 masks
m = rng.integers(0, 2, size=(32, 16, 4)) * 255
m[:, 0], m[:, 1] = 0, 255
add("masks", m)
# cut from the project's own material_test_scene textures
scene, _ = scenes.material_test_scene(320, 200)
cut = []
for k in range(64):
    img = np.asarray(scene.texture_images[k % len(scene.texture_images)], dtype=np.uint8)
    by, bx = int(rng.integers(0, img.shape[0] // 4)), int(rng.integers(0, img.shape[1] // 4))
    cut.append(img[4 * by:4 * by + 4, 4 * bx:4 * bx + 4].reshape(16, 4))
add("scene", np.array(cut))
# chosen by what the encoder does with them: a refinement round that finds one index in all 16 texels, and blocks that end
# with max16 < min16.  Candidates: low-contrast noise (the first) and all of the above kinds (the second)
cand = np.concatenate([noise(4096)] + [(rng.integers(0, 256 - k, size=(2048, 1, 4)) + rng.integers(0, k + 1, size=(2048, 16, 4))).astype(np.uint8) for k in (1, 2, 3, 5, 9)])
info = {}
E.encode_colour(cand, info)
sing = cand[info["singular"]][::7][:64]
swap = cand[info["swapped"] & ~info["constant"]][:64]
assert len(sing) == 64 and len(swap) == 64, (len(sing), len(swap))
add("singular", sing)
add("swapped", swap)

blocks = np.concatenate([b for _, b in classes])
assert len(blocks) <= 2048
blocks.tofile(sys.argv[1])
with open(sys.argv[2], "w") as f:
    for name, b in classes:
        f.write("%s %d\n" % (name, len(b)))
PY
"$TMP/enc_o2" "$TMP/blocks.bin" "$TMP/out_o2.bin"
"$TMP/enc_o0" "$TMP/blocks.bin" "$TMP/out_o0.bin"
cmp "$TMP/out_o2.bin" "$TMP/out_o0.bin" || { echo "the -O0 build disagrees with the pinned one: nothing written" >&2; exit 1; }
python3 - "$TMP/blocks.bin" "$TMP/classes.txt" "$TMP/out_o2.bin" <<'PY'
import sys, os, numpy as np
blocks = np.fromfile(sys.argv[1], dtype=np.uint8).reshape(-1, 16, 4)
out = np.fromfile(sys.argv[3], dtype=np.uint8).reshape(len(blocks), 48)
names, counts = zip(*[(l.split()[0], int(l.split()[1])) for l in open(sys.argv[2])])
assert sum(counts) == len(blocks)
np.savez_compressed("texture_encode.npz", blocks=blocks, bc1=out[:, :8], bc3=out[:, 8:24], bc4=out[:, 24:32], bc5=out[:, 32:48],
                    class_names=np.array(names), class_counts=np.array(counts, dtype=np.uint32))
size = os.path.getsize("texture_encode.npz")
assert size < 256 * 1024, size
print("wrote texture_encode.npz: %d blocks, %d bytes" % (len(blocks), size), dict(zip(names, counts)))
PY
