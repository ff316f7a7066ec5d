"""The pinned decode of block-compressed textures restated in numpy: what chordvis_upload_scene and
chordvis_upload_material_textures expand CHORD_TEXFMT_BC1_RGB / BC3 / BC4 / BC5 chains to.  Integers only, floor divisions.

    decode_level(blocks, w, h, format)  -> (h, w, 4) uint8
    decode_chain(data, width, height, mips, format) -> [level 0, level 1, ...]
    texel(block_bytes, x, y, format)    -> (r, g, b, a): the same, one texel at a time in plain Python
"""
import numpy as np

RGBA8, BC1_RGB, BC3, BC4, BC5 = 0, 1, 2, 3, 4
BLOCK_BYTES = {BC1_RGB: 8, BC3: 16, BC4: 8, BC5: 16}


def level_dims(width, height, mips):
    return [(max(1, width >> l), max(1, height >> l)) for l in range(mips)]


def level_bytes(w, h, format):
    return w * h * 4 if format == RGBA8 else ((w + 3) // 4) * ((h + 3) // 4) * BLOCK_BYTES[format]


def chain_bytes(width, height, mips, format):
    return sum(level_bytes(w, h, format) for w, h in level_dims(width, height, mips))


def colour_endpoints(blocks8):
    """(c0, c1) of (n, 8) colour blocks."""
    b = blocks8.astype(np.int64)
    return b[:, 0] | (b[:, 1] << 8), b[:, 2] | (b[:, 3] << 8)


def colour_block(blocks8, always_four):
    """(n, 8) uint8 colour blocks -> (n, 16, 3): texel (x, y) of the block at index 4 * y + x."""
    b = blocks8.astype(np.int64)
    c0, c1 = colour_endpoints(blocks8)
    idx_word = b[:, 4] | (b[:, 5] << 8) | (b[:, 6] << 16) | (b[:, 7] << 24)

    def expand(c):
        r5, g6, b5 = c >> 11, (c >> 5) & 63, c & 31
        return np.stack([(r5 << 3) | (r5 >> 2), (g6 << 2) | (g6 >> 4), (b5 << 3) | (b5 >> 2)], axis=1)
    p0, p1 = expand(c0), expand(c1)
    four = np.ones(len(b), dtype=bool) if always_four else c0 > c1
    p2 = np.where(four[:, None], (2 * p0 + p1) // 3, (p0 + p1) // 2)
    p3 = np.where(four[:, None], (p0 + 2 * p1) // 3, 0)
    pal = np.stack([p0, p1, p2, p3], axis=1)                                     # (n, 4, 3)
    idx = (idx_word[:, None] >> (2 * np.arange(16))[None, :]) & 3               # (n, 16)
    return np.take_along_axis(pal, idx[:, :, None].repeat(3, axis=2), axis=1)


def channel_block(blocks8):
    """(n, 8) uint8 alpha / single-channel blocks -> (n, 16)."""
    b = blocks8.astype(np.int64)
    a0, a1 = b[:, 0], b[:, 1]
    bits = np.zeros(len(b), dtype=np.int64)
    for j in range(6):
        bits |= b[:, 2 + j] << (8 * j)
    pal = np.zeros((len(b), 8), dtype=np.int64)
    pal[:, 0], pal[:, 1] = a0, a1
    for k in range(2, 8):
        eight = ((8 - k) * a0 + (k - 1) * a1) // 7
        six = ((6 - k) * a0 + (k - 1) * a1) // 5 if k < 6 else np.full_like(a0, 0 if k == 6 else 255)
        pal[:, k] = np.where(a0 > a1, eight, six)
    idx = (bits[:, None] >> (3 * np.arange(16))[None, :]) & 7
    return np.take_along_axis(pal, idx, axis=1)


def decode_blocks(blocks, format):
    """(n, block bytes) uint8 -> (n, 16, 4) uint8."""
    blocks = np.asarray(blocks, dtype=np.uint8).reshape(-1, BLOCK_BYTES[format])
    out = np.zeros((len(blocks), 16, 4), dtype=np.int64)
    out[:, :, 3] = 255
    if format == BC1_RGB:
        out[:, :, :3] = colour_block(blocks, False)
    elif format == BC3:
        out[:, :, 3] = channel_block(blocks[:, :8])
        out[:, :, :3] = colour_block(blocks[:, 8:], True)
    elif format == BC4:
        out[:, :, 0] = channel_block(blocks)
    elif format == BC5:
        out[:, :, 0] = channel_block(blocks[:, :8])
        out[:, :, 1] = channel_block(blocks[:, 8:])
    else:
        raise ValueError(format)
    return out.astype(np.uint8)


def decode_level(blocks, w, h, format):
    """The ceil(w / 4) x ceil(h / 4) row-major blocks of one level -> (h, w, 4) uint8 (texels outside the level are dropped)."""
    bw, bh = (w + 3) // 4, (h + 3) // 4
    t = decode_blocks(blocks, format)
    assert len(t) == bw * bh
    img = t.reshape(bh, bw, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(bh * 4, bw * 4, 4)
    return np.ascontiguousarray(img[:h, :w])


def decode_chain(data, width, height, mips, format):
    data = np.asarray(data, dtype=np.uint8).reshape(-1)
    assert len(data) == chain_bytes(width, height, mips, format)
    out, off = [], 0
    for w, h in level_dims(width, height, mips):
        n = level_bytes(w, h, format)
        out.append(data[off:off + n].reshape(h, w, 4).copy() if format == RGBA8 else decode_level(data[off:off + n], w, h, format))
        off += n
    return out


def chain_rgba8(data, width, height, mips, format):
    """The decoded levels back to back: the RGBA8 chain a host would have had to make."""
    return np.concatenate([l.reshape(-1) for l in decode_chain(data, width, height, mips, format)])


# ---- one texel at a time, plain Python -------------------------------------------------------------------------------------------

def _channel_texel(b, x, y):
    a0, a1 = int(b[0]), int(b[1])
    bits = sum(int(b[2 + j]) << (8 * j) for j in range(6))
    k = (bits >> (3 * (4 * (y & 3) + (x & 3)))) & 7
    if k == 0:
        return a0
    if k == 1:
        return a1
    if a0 > a1:
        return ((8 - k) * a0 + (k - 1) * a1) // 7
    if k < 6:
        return ((6 - k) * a0 + (k - 1) * a1) // 5
    return 0 if k == 6 else 255


def _colour_texel(b, x, y, always_four):
    c0, c1 = int(b[0]) | int(b[1]) << 8, int(b[2]) | int(b[3]) << 8
    word = int(b[4]) | int(b[5]) << 8 | int(b[6]) << 16 | int(b[7]) << 24
    i = 4 * (y & 3) + (x & 3)
    k = (word >> (2 * i)) & 3

    def expand(c):
        r5, g6, b5 = c >> 11, (c >> 5) & 63, c & 31
        return ((r5 << 3) | (r5 >> 2), (g6 << 2) | (g6 >> 4), (b5 << 3) | (b5 >> 2))
    p0, p1 = expand(c0), expand(c1)
    if k == 0:
        return p0
    if k == 1:
        return p1
    if always_four or c0 > c1:
        return tuple((2 * a + b_) // 3 for a, b_ in zip(p0, p1)) if k == 2 else tuple((a + 2 * b_) // 3 for a, b_ in zip(p0, p1))
    return tuple((a + b_) // 2 for a, b_ in zip(p0, p1)) if k == 2 else (0, 0, 0)


def texel(block, x, y, format):
    b = [int(v) for v in block]
    if format == BC1_RGB:
        return _colour_texel(b, x, y, False) + (255,)
    if format == BC3:
        return _colour_texel(b[8:], x, y, True) + (_channel_texel(b[:8], x, y),)
    if format == BC4:
        return (_channel_texel(b, x, y), 0, 0, 255)
    if format == BC5:
        return (_channel_texel(b[:8], x, y), _channel_texel(b[8:], x, y), 0, 255)
    raise ValueError(format)


# ---- scenes of the tests: a scene under block-compressed textures, and its decoded RGBA8 twin -------------------------------------

def bc_scene(scene, formats):
    """`scene` with texture i encoded to formats[i] by records.bc_chain (RGBA8: kept as an image)."""
    from chord_amd import records as R, scenes
    return scenes.with_textures(scene, [t if f == RGBA8 else R.bc_chain(t, f) for t, f in zip(scene.texture_images, formats)])


def decoded_twin(scene):
    """The same scene with every block-compressed texture handed over as the RGBA8 chain this file decodes it to."""
    from chord_amd import records as R, scenes
    out = []
    for t in scene.texture_images:
        if isinstance(t, R.TextureChain) and t.format != RGBA8:
            t = R.TextureChain(chain_rgba8(t.data, t.width, t.height, t.mips, t.format), t.width, t.height, t.mips, RGBA8)
        out.append(t)
    return scenes.with_textures(scene, out)


def masked_scenes(width=320, height=200):
    """masked_test_scene with BC3 base colours and with BC1_RGB ones (alpha 255): (bc3 scene, bc1 scene, cam, view, iv)."""
    import helpers as H
    from chord_amd import scenes
    scene, cam, view, iv = H.setup_scene(scenes.masked_test_scene, width, height)
    n = len(scene.texture_images)
    return bc_scene(scene, [BC3] * n), bc_scene(scene, [BC1_RGB] * n), cam, view, iv
