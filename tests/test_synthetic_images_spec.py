"""The references of tests/test_gpu_synthetic_images.py, pinned before the GPU is held to them: on the adversarial depth images of
helpers.synthetic_depth the two CPU statements of the HZB chain (spec_np.hzb_build, vectorised numpy; orc.hzb_build, scalar C)
agree bit for bit with each other and with helpers.valid_range_of, the generator really contains every class of value it
promises, and every image size has the layout property it was chosen for."""
import numpy as np
import pytest

import helpers as H
import orc
import spec_np as S

SIZES = H.HZB_SIZES + [(d, d) for d in H.DEPTH_VIEW_DIMS if (d, d) not in H.HZB_SIZES]
ids = lambda s: "%dx%d" % s


@pytest.mark.parametrize("size", SIZES, ids=ids)
def test_both_cpu_chains_and_the_range_agree_on_synthetic_depth(size):
    w, h = size
    for seed in (1, 2):
        depth = H.synthetic_depth(w, h, seed)
        counts = H.depth_classes(depth)
        assert all(v > 0 for v in counts.values()), counts
        assert 0.05 < counts["zero"] / (w * h) < 0.2 and 0.02 < counts["one"] / (w * h) < 0.1, counts
        words = H.synthetic_words(depth, np.zeros(w * h, dtype=np.uint32))
        assert np.array_equal((words >> np.uint64(32)).astype(np.uint32), depth.ravel().view(np.uint32))
        desc, mn, mx, rng = orc.hzb_build(words, w, h, want_max=True, want_range=True)
        dims, offs, levels = S.hzb_build(depth, w, h, want_max=True)
        assert [desc.mip_dims(l) for l in range(desc.mipCount)] == dims
        assert [int(desc.mipOffset[l]) for l in range(desc.mipCount)] == offs[:-1].tolist() and desc.totalTexels == offs[-1]
        got_min, got_max = H.hzb_levels(desc, mn), H.hzb_levels(desc, mx)
        for l, (smn, smx) in enumerate(levels):
            assert smn.shape == desc.valid_dims(l)[::-1]
            assert np.array_equal(got_min[l], smn), "%dx%d seed %d: min level %d" % (w, h, seed, l)
            assert np.array_equal(got_max[l], smx), "%dx%d seed %d: max level %d" % (w, h, seed, l)
        assert np.array_equal(rng, H.valid_range_of(depth)), (rng, H.valid_range_of(depth))
        # the image does what it is for: up to the level whose texels are as large as a cell of the generator's 4 x 4 grid the
        # chains hold many values, not min 0.0 / max 1.0 throughout; and the range is not the trivial one
        for l in range(2, max(4, int(np.log2(min(w, h) / 4)))):
            assert len(np.unique(got_min[l])) > 2 and len(np.unique(got_max[l])) > 2, (l, size)
        assert rng[0] != 0xFFFFFFFF and rng[1] == H.F32_ONE


def test_the_range_of_degenerate_images():
    z, o = np.zeros((67, 129), dtype=np.float32), np.ones((67, 129), dtype=np.float32)
    assert H.valid_range_of(z).tolist() == [0xFFFFFFFF, 0]
    assert H.valid_range_of(o).tolist() == [0xFFFFFFFF, H.F32_ONE]
    for d in (z, o):
        _, _, _, rng = orc.hzb_build(H.synthetic_words(d, np.zeros(d.size, dtype=np.uint32)), 129, 67, want_max=True, want_range=True)
        assert np.array_equal(rng, H.valid_range_of(d))


def test_rounding_classes_separate_the_rounding_modes():
    """On the generator's ties and their neighbours round-to-nearest-even, truncation and round-half-up give three different
    binary16 images: a kernel with either wrong mode cannot pass an exact comparison."""
    depth = H.synthetic_depth(129, 67, 1).ravel()
    b = depth.view(np.uint32)
    rne = S.f16_bits(depth)
    normal = (depth >= np.float32(2.0 ** -14)) & (depth < 1)
    trunc = (((b >> 23) - 112) << 10 | (b >> 13) & 0x3FF).astype(np.uint16)
    half_up = ((((b + 0x1000) >> 23) - 112) << 10 | ((b + 0x1000) >> 13) & 0x3FF).astype(np.uint16)
    assert (rne[normal] != trunc[normal]).any() and (rne[normal] != half_up[normal]).any()
    assert np.array_equal(orc_f16(depth), rne)


def orc_f16(depth):
    return np.array([orc.lib.orc_f32_to_f16(float(v)) for v in depth], dtype=np.uint16)


LAYOUT = {
    (64, 64): lambda d: d.mipCount == 6,                                             # no tail level: the tail runs for the range alone
    (65, 64): lambda d: d.mipCount == 7 and d.mip_dims(6) == (1, 1) and d.valid_dims(6) == (1, 1),
    (64, 127): lambda d: d.valid_dims(0) == d.mip_dims(0) == (32, 64) and 2 * 63 + 1 > 126,   # the last mip-0 row clamps its second source row
    (129, 67): lambda d: d.valid_dims(0) == (65, 34) and d.mip_dims(0) == (128, 64),
    (257, 64): lambda d: d.mip_dims(0)[0] == 256 and all(d.valid_dims(l)[0] == (128 >> l) + 1 < d.mip_dims(l)[0] for l in range(7)),
    (66, 2049): lambda d: d.mipCount == 12 and d.mip_dims(6) == (1, 32) and d.valid_dims(6) == (1, 17),
    (2049, 65): lambda d: d.mipCount == 12 and d.mip_dims(6) == (32, 1) and d.valid_dims(6) == (17, 1),
    (1237, 701): lambda d: H.range_partial_count(1237, 701) == 880 > 3 * 256,       # the tail's 256-thread partial loop: four trips
    (4096, 4096): lambda d: d.mipCount == 12 and d.valid_dims(6) == d.mip_dims(6) == (32, 32),   # 1024 texels: all of sMinA / sMaxA
}


@pytest.mark.parametrize("size", H.HZB_SIZES + [H.HZB_FULL_TAIL_SIZE], ids=ids)
def test_every_size_has_the_layout_it_was_chosen_for(size):
    d = orc.hzb_desc(*size)
    assert (d.srcWidth, d.srcHeight) == size
    assert LAYOUT[size](d), [(d.mip_dims(l), d.valid_dims(l)) for l in range(d.mipCount)]
    for l in range(d.mipCount):
        assert all(1 <= v <= m for v, m in zip(d.valid_dims(l), d.mip_dims(l)))


def test_the_full_tail_needs_nearly_4096_pixels_per_axis():
    """Level 6 holds 32 x 32 valid texels -- every float of the tail's first LDS buffer -- only from 3969 pixels per axis; the
    suite's 3840 x 2160 frames reach 30 x 17."""
    assert orc.hzb_desc(3840, 2160).valid_dims(6) == (30, 17)
    assert orc.hzb_desc(3968, 3968).valid_dims(6) == (31, 31) and orc.hzb_desc(3969, 3969).valid_dims(6) == (32, 32)
