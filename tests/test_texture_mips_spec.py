"""The numpy spec of the upload-time mip chains (tests/spec_texture_mips_np.py) against the properties DESIGN.md 2 item 9(i) states:
flags 0 is records.mip_chain_rgba8, the linear-light average keeps flat images and differs from the code average, and the alpha
rescale reaches level 0's coverage on every generated level, is exact at the cutoff, and is idle where it has nothing to do."""
import numpy as np
import pytest

from chord_amd import records as R

import spec_texture_mips_np as M

SIZES = [(1, 1), (2, 2), (5, 3), (7, 9), (64, 64), (260, 4), (4, 260), (37, 21)]           # (width, height)


def _random(rng, w, h):
    return rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)


@pytest.mark.parametrize("w,h", SIZES)
def test_flags_0_is_mip_chain_rgba8(w, h):
    img = _random(np.random.default_rng(w * 1000 + h), w, h)
    want, mips = R.mip_chain_rgba8(img)
    got = M.build_chain([img], M.FULL)
    assert len(got) == mips == M.full_levels(w, h)
    assert [l.shape for l in got] == [(lh, lw, 4) for lw, lh in R.level_dims(w, h, mips)]
    assert np.array_equal(M.chain_bytes(got), want)
    # a chain supplied with some levels goes on from the last of them
    if mips > 2:
        assert np.array_equal(M.chain_bytes(M.build_chain(got[:2], M.FULL)), want)
    assert len(M.build_chain([img], 0)) == 1 and len(M.build_chain([img], 2)) == min(2, mips)


def test_tables_are_strictly_increasing():
    assert (np.diff(M.T) > 0).all() and (np.diff(M.MID[1:]) > 0).all()
    assert (M.T[:-1] < M.MID[1:]).all() and (M.MID[1:] < M.T[1:]).all()
    from chord_amd import lib as L
    assert np.array_equal(L.material_constants()[0].view(np.uint32), M.T.view(np.uint32))


def test_srgb_keeps_flat_images_and_differs_from_codes():
    for code in range(256):
        img = np.full((4, 6, 4), code, dtype=np.uint8)
        for l in M.build_chain([img], M.FULL, M.SRGB):
            assert (l == code).all(), code
    img = _random(np.random.default_rng(5), 64, 64)
    a, b = M.build_chain([img], M.FULL), M.build_chain([img], M.FULL, M.SRGB)
    differ = sum(int((x[..., :3] != y[..., :3]).sum()) for x, y in zip(a, b))
    assert differ > 1000, differ
    for x, y in zip(a, b):
        assert np.array_equal(x[..., 3], y[..., 3])                  # alpha is averaged as a code under either
        assert (y[..., :3].astype(int) >= x[..., :3].astype(int) - 1).all()     # the linear mean is never darker (up to the code rounding)


def _mask(rng, share=0.3, n=128):
    img = _random(rng, n, n)
    img[..., 3] = np.where(rng.random((n, n)) < share, 255, 0)
    return img


def _check_coverage(img, cutoff, flags=M.COVERAGE):
    """The properties of every generated level; returns [(level, t')]."""
    plain = M.build_chain([img], M.FULL, flags & ~M.COVERAGE)
    ts = []
    got = M.build_chain([img], M.FULL, flags, cutoff, ts)
    n0, p0 = img[..., 3].size, int((img[..., 3] >= cutoff).sum())
    assert np.array_equal(got[0], img)
    assert [l for l, _ in ts] == list(range(1, len(got)))
    for (l, tp), a, b in zip(ts, plain[1:], got[1:]):
        assert np.array_equal(a[..., :3], b[..., :3])
        cnt = M.counts(a[..., 3])
        n = a[..., 3].size
        assert 1 <= tp <= 255
        assert int((b[..., 3] >= cutoff).sum()) == cnt[tp], (l, tp)
        if cnt[1] * n0 >= p0 * n:
            assert int((b[..., 3] >= cutoff).sum()) >= -(-p0 * n // n0), (l, tp)
        if tp == cutoff:
            assert np.array_equal(a, b)
    return ts


def test_coverage_on_masks():
    img = _mask(np.random.default_rng(11))
    t128 = dict(_check_coverage(img, 128))
    assert any(t < 128 for t in t128.values()), t128                 # the box thins the mask: the threshold comes down
    t64 = dict(_check_coverage(img, 64))
    assert any(t > 64 for t in t64.values()), t64                    # ... and at a low cutoff it fattens it: the threshold goes up
    assert any(t != 64 for l, t in t64.items() if l <= 3)
    rnd = _random(np.random.default_rng(12), 128, 128)
    t200 = dict(_check_coverage(rnd, 200, M.SRGB | M.COVERAGE))
    assert all(t < 200 for l, t in t200.items() if l <= 4), t200
    # the rescale is not idle: the rescaled alpha differs from the plain chain's
    plain, scaled = M.build_chain([rnd], M.FULL), M.build_chain([rnd], M.FULL, M.COVERAGE, 200)
    assert any(not np.array_equal(a, b) for a, b in zip(plain[1:], scaled[1:]))


@pytest.mark.parametrize("cutoff", [1, 64, 128, 255])
def test_coverage_leaves_what_it_cannot_improve(cutoff):
    rng = np.random.default_rng(13)
    opaque = _random(rng, 37, 21)
    opaque[..., 3] = 255
    none = _random(rng, 37, 21)
    none[..., 3] = rng.integers(0, cutoff, size=(21, 37))            # no texel passes
    for img in (opaque, none):
        ts = _check_coverage(img, cutoff)
        assert all(t == cutoff for _, t in ts), ts
        assert np.array_equal(M.chain_bytes(M.build_chain([img], M.FULL, M.COVERAGE, cutoff)), M.chain_bytes(M.build_chain([img], M.FULL)))


def test_supplied_levels_are_never_rescaled():
    img = _mask(np.random.default_rng(14), n=64)
    plain = M.build_chain([img], M.FULL)
    got = M.build_chain(plain[:3], M.FULL, M.COVERAGE, 128)
    for l in range(3):
        assert np.array_equal(got[l], plain[l])
    assert any(not np.array_equal(a, b) for a, b in zip(plain[3:], got[3:]))
    assert len(M.build_chain(plain[:3], 5, M.COVERAGE, 128)) == 5 and len(M.build_chain(plain[:3], 2)) == 3
