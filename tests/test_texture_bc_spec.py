"""The pinned decode of block-compressed textures (tests/spec_texture_bc_np.py): hand-computed blocks, the
vectorised restatement against a per-texel one, bit order, edge blocks, chain sizes against chordvis_texture_chain_bytes, the test
encoder's round trip, and the guard that keeps tests/test_gpu_texture_bc.py's masked scene from being vacuous.  CPU only."""
import numpy as np
import pytest

import helpers as H
import spec_texture_bc_np as BC
from chord_amd import records as R

FORMATS = [BC.BC1_RGB, BC.BC3, BC.BC4, BC.BC5]
RED, BLUE = (0x00, 0xF8), (0x1F, 0x00)                    # c = 0xF800 (255, 0, 0) and c = 0x001F (0, 0, 255), little-endian


def _u32(v):
    return [v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0xFF, (v >> 24) & 0xFF]


def _idx48(idx):
    bits = sum(k << (3 * i) for i, k in enumerate(idx))
    return [(bits >> (8 * j)) & 0xFF for j in range(6)]


def _first(blocks, format, n):
    return [tuple(int(v) for v in t) for t in BC.decode_blocks(np.array(blocks, np.uint8), format)[0, :n]]


def test_known_answers():
    # BC1, c0 > c1: four colours, thirds with floor division; alpha always 255
    four = list(RED) + list(BLUE) + _u32(0xE4)           # texels 0..3 take indices 0..3
    assert _first(four, BC.BC1_RGB, 4) == [(255, 0, 0, 255), (0, 0, 255, 255), (170, 0, 85, 255), (85, 0, 170, 255)]
    # BC1, c0 < c1: three colours, the floor of the half, and black (still alpha 255: the _RGB_ format)
    three = list(BLUE) + list(RED) + _u32(0xE4)
    assert _first(three, BC.BC1_RGB, 4) == [(0, 0, 255, 255), (255, 0, 0, 255), (127, 0, 127, 255), (0, 0, 0, 255)]
    # BC1, c0 == c1: three-colour mode too
    same = list(RED) + list(RED) + _u32(0xE4)
    assert _first(same, BC.BC1_RGB, 4) == [(255, 0, 0, 255), (255, 0, 0, 255), (255, 0, 0, 255), (0, 0, 0, 255)]
    # BC3: the SAME colour bytes with c0 < c1 stay in four-colour mode; alpha eight-value mode (a0 > a1), sevenths floored
    alpha8 = [200, 100] + _idx48(list(range(8)) + [0] * 8)
    got = _first(alpha8 + three, BC.BC3, 8)
    assert [t[:3] for t in got[:4]] == [(0, 0, 255), (255, 0, 0), (85, 0, 170), (170, 0, 85)]
    assert [t[3] for t in got] == [200, 100, 185, 171, 157, 142, 128, 114]
    # BC4: six-value mode (a0 <= a1) with its 0 and 255
    six = [50, 250] + _idx48(list(range(8)) + [0] * 8)
    assert _first(six, BC.BC4, 8) == [(v, 0, 0, 255) for v in (50, 250, 90, 130, 170, 210, 0, 255)]
    assert _first([7, 7] + _idx48([0, 1, 2, 5, 6, 7] + [0] * 10), BC.BC4, 6) == [(v, 0, 0, 255) for v in (7, 7, 7, 7, 0, 255)]
    # BC5: red from the first block (eight values), green from the second (six values)
    assert _first(alpha8 + six, BC.BC5, 8) == [(r, g, 0, 255) for r, g in zip((200, 100, 185, 171, 157, 142, 128, 114), (50, 250, 90, 130, 170, 210, 0, 255))]
    # endpoint expansion by bit replication: r5 = 16 -> 132, g6 = 32 -> 130, b5 = 1 -> 8; g6 = 63 -> 255
    c = (16 << 11) | (32 << 5) | 1
    assert _first([c & 0xFF, c >> 8, 0, 0] + _u32(0), BC.BC1_RGB, 1) == [(132, 130, 8, 255)]
    assert _first([0xE0, 0x07, 0, 0] + _u32(0), BC.BC1_RGB, 1) == [(0, 255, 0, 255)]


@pytest.mark.parametrize("format", FORMATS)
def test_per_texel_restatement_equals_the_vectorised_one(format):
    rng = np.random.default_rng(100 + format)
    blocks = rng.integers(0, 256, size=(48, BC.BLOCK_BYTES[format]), dtype=np.uint8)
    blocks[0, :] = 0
    blocks[1, :] = 255
    got = BC.decode_blocks(blocks, format)
    for n, b in enumerate(blocks):
        for y in range(4):
            for x in range(4):
                assert tuple(int(v) for v in got[n, 4 * y + x]) == BC.texel(b, x, y, format), (format, n, x, y)


def test_a_solid_block_returns_the_expanded_endpoint():
    rng = np.random.default_rng(5)
    for _ in range(64):
        c = int(rng.integers(0, 65536))
        r5, g6, b5 = c >> 11, (c >> 5) & 63, c & 31
        want = ((r5 << 3) | (r5 >> 2), (g6 << 2) | (g6 >> 4), (b5 << 3) | (b5 >> 2))
        a = int(rng.integers(0, 256))
        for word in (0, 0x55555555):                     # every texel on index 0, every texel on index 1
            colour = [c & 0xFF, c >> 8, c & 0xFF, c >> 8] + _u32(word)
            assert all(t == want + (255,) for t in _first(colour, BC.BC1_RGB, 16))
            assert all(t == want + (a,) for t in _first([a, a] + _idx48([0] * 16) + colour, BC.BC3, 16))
        assert all(t == (a, 0, 0, 255) for t in _first([a, a] + _idx48([1] * 16), BC.BC4, 16))


def test_index_bit_order():
    """Texel (x, y) of a block reads bits 2i, 2i + 1 (colour) / 3i .. 3i + 2 (channel), i = 4y + x, least significant first."""
    for i in range(16):
        colour = list(RED) + list(BLUE) + _u32(1 << (2 * i))             # index 1 (blue) at texel i alone
        img = BC.decode_level(np.array(colour, np.uint8), 4, 4, BC.BC1_RGB)
        blue = np.argwhere(img[..., 2] == 255)
        assert blue.tolist() == [[i // 4, i % 4]]
        chan = [10, 20] + _idx48([1 if j == i else 0 for j in range(16)])
        img = BC.decode_level(np.array(chan, np.uint8), 4, 4, BC.BC4)
        assert np.argwhere(img[..., 0] == 20).tolist() == [[i // 4, i % 4]]
    # an index that straddles a byte: texel 5 uses bits 15..17 of the 48
    chan = [10, 20] + _idx48([7 if j == 5 else 0 for j in range(16)])
    assert BC.decode_level(np.array(chan, np.uint8), 4, 4, BC.BC4)[1, 1, 0] == 255


@pytest.mark.parametrize("format", FORMATS)
def test_edge_blocks_are_cropped(format):
    rng = np.random.default_rng(7 + format)
    bb = BC.BLOCK_BYTES[format]
    blocks = rng.integers(0, 256, size=(2, bb), dtype=np.uint8)          # 5 x 3: two blocks in a row, one row
    full = BC.decode_blocks(blocks, format).reshape(2, 4, 4, 4)
    img = BC.decode_level(blocks, 5, 3, format)
    assert img.shape == (3, 5, 4)
    assert np.array_equal(img[:, :4], full[0, :3]) and np.array_equal(img[:, 4], full[1, :3, 0])
    one = BC.decode_level(blocks[:1], 1, 1, format)
    assert one.shape == (1, 1, 4) and np.array_equal(one[0, 0], full[0, 0, 0])
    # rows of blocks: 7 x 9 is 2 x 3 blocks, row-major
    blocks = rng.integers(0, 256, size=(6, bb), dtype=np.uint8)
    full = BC.decode_blocks(blocks, format).reshape(3, 2, 4, 4, 4)
    img = BC.decode_level(blocks, 7, 9, format)
    assert np.array_equal(img[8, 4:7], full[2, 1, 0, :3]) and np.array_equal(img[4:8, 0:4], full[1, 0])


def test_chain_sizes_match_the_library(built_lib):
    L = built_lib
    for w, h in [(4, 4), (1, 1), (2, 2), (5, 3), (7, 9), (64, 64), (260, 4), (4, 260), (37, 21), (2048, 2048), (16384, 16384)]:
        full = max(w, h).bit_length()
        for mips in sorted({1, 2, full} & set(range(1, full + 1))):
            for f in [BC.RGBA8] + FORMATS:
                assert L.texture_chain_bytes(f, w, h, mips) == BC.chain_bytes(w, h, mips, f), (w, h, mips, f)
    import ctypes as C
    n = C.c_uint64(77)
    for args in [(5, 4, 4, 1), (999, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 1), (0, 4, 4, 0)]:
        assert L.lib.chordvis_texture_chain_bytes(*args, C.byref(n)) == L.E_INVALID and n.value == 77
    assert L.lib.chordvis_texture_chain_bytes(1, 4, 4, 1, None) == L.E_INVALID
    # level offsets: the chain of the encoder is the levels back to back
    img = np.random.default_rng(3).integers(0, 256, size=(21, 37, 4), dtype=np.uint8)
    for f in FORMATS:
        ch = R.bc_chain(img, f)
        assert ch.mips == 6 and len(ch.data) == L.texture_chain_bytes(f, 37, 21, 6)
        chain, _ = R.mip_chain_rgba8(img)
        off = boff = 0
        for lw, lh in BC.level_dims(37, 21, 6):
            nb = BC.level_bytes(lw, lh, f)
            assert np.array_equal(ch.data[boff:boff + nb], R.encode_bc(chain[off:off + lw * lh * 4].reshape(lh, lw, 4), f))
            off += lw * lh * 4
            boff += nb


def test_encoder_round_trip():
    rng = np.random.default_rng(21)
    # a constant image whose codes are representable (5:6:5 expanded) decodes to itself, in every format's channels
    for _ in range(8):
        c = int(rng.integers(0, 65536))
        r5, g6, b5 = c >> 11, (c >> 5) & 63, c & 31
        px = np.array([(r5 << 3) | (r5 >> 2), (g6 << 2) | (g6 >> 4), (b5 << 3) | (b5 >> 2), int(rng.integers(0, 256))], np.uint8)
        img = np.broadcast_to(px, (6, 9, 4)).copy()
        want = {BC.BC1_RGB: [px[0], px[1], px[2], 255], BC.BC3: list(px), BC.BC4: [px[0], 0, 0, 255], BC.BC5: [px[0], px[1], 0, 255]}
        for f in FORMATS:
            got = BC.decode_level(R.encode_bc(img, f), 9, 6, f)
            assert (got == np.array(want[f], np.uint8)).all(), (f, px)
    # black and white are representable too (the encoder keeps c0 > c1 on solid blocks)
    for v in (0, 255):
        img = np.full((4, 4, 4), v, np.uint8)
        assert (BC.decode_level(R.encode_bc(img, BC.BC3), 4, 4, BC.BC3) == v).all()
    # well-formed on anything: right sizes, never the three-colour mode, both orders of a0 / a1 in BC3's alpha, and a decode
    # that stays near the image (bounding-box endpoints: within the block's range per channel)
    img = rng.integers(0, 256, size=(21, 37, 4), dtype=np.uint8)
    for f in FORMATS:
        blocks = R.encode_bc(img, f).reshape(-1, BC.BLOCK_BYTES[f])
        assert len(blocks) == 10 * 6
        if f in (BC.BC1_RGB, BC.BC3):
            c0, c1 = BC.colour_endpoints(blocks[:, -8:])
            assert (c0 > c1).all()
        if f != BC.BC1_RGB:
            a0, a1 = blocks[:, 0].astype(int), blocks[:, 1].astype(int)
            assert (a0 > a1).sum() >= len(blocks) // 4 and (a0 <= a1).sum() >= len(blocks) // 4
    smooth = np.zeros((16, 16, 4), np.uint8)
    smooth[..., 0] = np.arange(16)[None, :] * 16
    smooth[..., 1] = np.arange(16)[:, None] * 16
    smooth[..., 2] = 90
    smooth[..., 3] = np.arange(16)[None, :] * 8 + np.arange(16)[:, None] * 8
    got = BC.decode_level(R.encode_bc(smooth, BC.BC3), 16, 16, BC.BC3).astype(int)
    # (every palette entry lies between the block's truncated minimum and its maximum per channel: a texel is off by at most the
    # block's range, 3 steps of 16 here, plus the 7 codes truncation to 5 bits can take)
    assert np.abs(got - smooth.astype(int)).max() <= 3 * 16 + 7


def test_the_masked_scene_of_the_gpu_tests_depends_on_its_alpha():
    """tests/test_gpu_texture_bc.py compares frames of masked_test_scene(320, 200) under BC3 base colours with the oracle's; that
    would show nothing if the decoded alpha did not matter.  On the oracle, the frame under the BC3 textures' decoded twin differs
    from the frame under the BC1_RGB twins (alpha 255 throughout) in 28976 of 64000 pixels."""
    import orc
    bc3, bc1, cam, view, iv = BC.masked_scenes(320, 200)
    a = orc.frame(BC.decoded_twin(bc3), view, iv, H.ALL_FLAGS)["vis"]
    b = orc.frame(BC.decoded_twin(bc1), view, iv, H.ALL_FLAGS)["vis"]
    differ = int((a != b).sum())
    print("pixels that differ between the BC3 and the BC1_RGB twin:", differ)
    assert differ > 0
    # ... and the decoded BC3 alpha is not trivially that of the source either way: it holds both opaque and cut-out texels
    for t in bc3.texture_images:
        alpha = BC.decode_chain(t.data, t.width, t.height, t.mips, t.format)[0][..., 3]
        assert (alpha > 128).any() and (alpha < 64).any()
