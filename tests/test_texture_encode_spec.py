"""tests/spec_texture_encode_np.py (the block compression of chordvis_set_texture_compress) against the
reference's bytes: tests/golden/texture_encode.npz holds what the reference importer's compressor wrote for the fixture's blocks
(make_texture_encode_fixture.sh).  No GPU."""
import os

import numpy as np
import pytest

from chord_amd import records as R

import spec_texture_bc_np as BC
import spec_texture_encode_np as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "texture_encode.npz")
FORMATS = [(E.BC1_RGB, "bc1"), (E.BC3, "bc3"), (E.BC4, "bc4"), (E.BC5, "bc5")]
CLASSES = ["constant", "constant_colour_varying_alpha", "two_colour", "small_noise", "ramp", "full_noise", "channel_ranges", "masks",
           "scene", "singular", "swapped"]


@pytest.fixture(scope="module")
def golden():
    d = np.load(GOLDEN)
    names = [str(n) for n in d["class_names"]]
    counts = [int(n) for n in d["class_counts"]]
    start = np.concatenate([[0], np.cumsum(counts)])
    classes = {n: slice(int(start[i]), int(start[i + 1])) for i, n in enumerate(names)}
    return d, classes


def test_fixture_holds_every_class(golden):
    d, classes = golden
    blocks = d["blocks"]
    assert os.path.getsize(GOLDEN) < 256 * 1024 and len(blocks) <= 2048 and blocks.shape[1:] == (16, 4)
    assert sorted(classes) == sorted(CLASSES) and all(s.stop > s.start for s in classes.values())
    info = {}
    E.encode_colour(blocks, info)
    const = blocks[classes["constant"]]
    assert (const == const[:, :1]).all()
    for ch in range(3):                                                    # every entry of both pair tables
        assert sorted(set(const[:, 0, ch].tolist())) == list(range(256))
    cva = classes["constant_colour_varying_alpha"]
    assert (blocks[cva][:, :, :3] == blocks[cva][:, :1, :3]).all() and not info["constant"][cva].any()      # BC1: the general path
    opaque = blocks[cva].copy()
    opaque[:, :, 3] = 255
    info3 = {}
    E.encode_colour(opaque, info3)
    assert info3["constant"].all()                                         # BC3: constant once the alpha is forced
    two = blocks[classes["two_colour"]][:, :, :3]
    assert all(len(np.unique(b, axis=0)) == 2 for b in two)
    assert info["luminance"][classes["small_noise"]].any() and not info["luminance"][classes["full_noise"]].all()
    assert info["singular"][classes["singular"]].all()
    assert info["swapped"][classes["swapped"]].all() and not info["constant"][classes["swapped"]].any()
    cr = blocks[classes["channel_ranges"]].astype(int)
    for ch in (0, 1, 3):
        dist = cr[:, :, ch].max(axis=1) - cr[:, :, ch].min(axis=1)
        assert set(dist.tolist()) == {0, 1, 2, 3, 4, 5, 6, 7, 8, 255}
    assert set(np.unique(blocks[classes["masks"]]).tolist()) == {0, 255}
    assert classes["scene"].stop - classes["scene"].start == 64


@pytest.mark.parametrize("format,key", FORMATS, ids=[k for _, k in FORMATS])
def test_spec_encodes_the_fixture_to_the_reference_bytes(golden, format, key):
    d, classes = golden
    got, want = E.encode_blocks(d["blocks"], format), d[key]
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.nonzero((got != want).any(axis=1))[0]
    if len(bad):
        cls = [n for n, s in classes.items() if s.start <= bad[0] < s.stop]
        raise AssertionError("%s: %d blocks differ; first %d (%s): got %s want %s" % (key, len(bad), bad[0], cls, got[bad[0]], want[bad[0]]))


@pytest.mark.parametrize("w,h", [(1, 1), (2, 2), (3, 5), (4, 4), (5, 7), (8, 8)])
def test_level_encoder_is_the_block_encoder_on_the_stated_fill(w, h):
    rng = np.random.default_rng(100 * w + h)
    img = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    bw, bh = (w + 3) // 4, (h + 3) // 4
    blocks = np.zeros((bh * bw, 16, 4), np.uint8)
    for by in range(bh):
        for bx in range(bw):
            for y in range(4):
                for x in range(4):
                    blocks[by * bw + bx, 4 * y + x] = img[(4 * by + y) % h, (4 * bx + x) % w]
    assert np.array_equal(E.fill_blocks(img), blocks)
    for format, _ in FORMATS:
        got = E.encode_level(img, format)
        assert len(got) == BC.level_bytes(w, h, format)
        assert np.array_equal(got, E.encode_blocks(blocks, format).reshape(-1))
    chain = E.encode_chain([img, img[:max(1, h // 2), :max(1, w // 2)]], E.BC3)
    assert np.array_equal(chain[:bw * bh * 16], E.encode_level(img, E.BC3))


def colour_mse(golden):
    """{class: (spec, trivial)} mean squared colour error of the BC1 blocks over the fixture's non-constant blocks, and "all"."""
    d, classes = golden
    blocks = d["blocks"]
    rgb = blocks[:, :, :3].astype(np.int64)
    varying = ~(rgb == rgb[:, :1]).all(axis=(1, 2))
    err = lambda enc: ((BC.decode_blocks(enc, BC.BC1_RGB)[:, :, :3].astype(np.int64) - rgb) ** 2).mean(axis=(1, 2))
    spec, trivial = err(E.encode_blocks(blocks, E.BC1_RGB)), err(R._encode_colour(rgb))
    out = {}
    for n, s in classes.items():
        k = np.nonzero(varying[s])[0] + s.start
        if len(k):
            out[n] = (float(spec[k].mean()), float(trivial[k].mean()))
    out["all"] = (float(spec[varying].mean()), float(trivial[varying].mean()))
    return out


def test_better_not_just_different(golden):
    """Against the trivial encoder (endpoints = the per-channel minimum and maximum, every texel the nearest palette entry): the
    spec's BC1 blocks are no worse on any class and strictly better over all classes together.  The figures are in DESIGN.md
    2 item 9(j)."""
    mse = colour_mse(golden)
    for n, (spec, trivial) in sorted(mse.items()):
        print("%-32s spec %9.3f trivial %9.3f" % (n, spec, trivial))
    for n, (spec, trivial) in mse.items():
        assert spec <= trivial, (n, spec, trivial)
    assert mse["all"][0] < mse["all"][1]
