"""Shared helpers for the parity tests: scene/view setup and GPU-vs-oracle comparisons."""
import numpy as np

from chord_amd import records as R
from chord_amd import scenes

ALL_FLAGS = R.FLAG_FRUSTUM_CULL | R.FLAG_CONE_CULL | R.FLAG_HZB_CULL


def setup_scene(builder, *args, **kw):
    """(scene, camera, view, iv) with object records filled for the camera (static scene, no history)."""
    from chord_amd import lib as L
    scene, cam = builder(*args, **kw)
    L.fill_objects(scene, cam)
    view, iv = L.make_views(cam)
    return scene, cam, view, iv


def views_for(cam, last_view=None):
    from chord_amd import lib as L
    return L.make_views(cam, last_view)


def sort_cmds(cmds):
    return np.sort(np.asarray(cmds, dtype=R.DRAW_CMD), order=["slot", "objectId", "meshletId"])


def assert_vis_equal(got, want, w, h, what=""):
    got = np.asarray(got, dtype=np.uint64).reshape(h, w)
    want = np.asarray(want, dtype=np.uint64).reshape(h, w)
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    y, x = bad[0]
    raise AssertionError("%s visibility mismatch at %d pixels; first (x=%d, y=%d): got %#018x want %#018x"
                         % (what, len(bad), x, y, int(got[y, x]), int(want[y, x])))


def with_shading_types(scene, types=(1, 37, 100, 64, 127)):
    """A copy of `scene` in which object i has its own material of shading type types[i % len(types)]
    (the procedural scenes use type 1 throughout; the tile marker wants variety)."""
    mats = scene.materials[scene.objects["GLTFMaterialData"]].copy()
    mats["materialType"] = np.asarray(types, dtype=np.uint32)[np.arange(len(mats)) % len(types)]
    objs = scene.objects.copy()
    objs["GLTFMaterialData"] = np.arange(len(objs), dtype=np.uint32)
    out = scene.with_objects(objs, mats)
    out.name = scene.name + "+types"
    return out


def brute_force_marker(scene, vis, w, h, cmds):
    """Per 8x8 pixels the set of shading types present (empty pixel = type 0), straight from the definition."""
    low = (np.asarray(vis, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32).reshape(h, w)
    slot = ((low >> 8) & 0xFFFFFF).astype(np.int64) - 1
    obj = np.asarray(cmds["objectId"], dtype=np.int64)
    typ = np.zeros((h, w), dtype=np.uint32)
    hit = low != 0
    typ[hit] = scene.materials["materialType"][scene.objects["GLTFMaterialData"][obj[slot[hit]]]]
    mw, mh = (w + 7) // 8, (h + 7) // 8
    marker = np.zeros((mh, mw, 4), dtype=np.uint32)
    for y in range(h):
        for x in range(w):
            t = int(typ[y, x])
            marker[y // 8, x // 8, t // 32] |= np.uint32(1 << (t % 32))
    return marker


def tiles_with_type(marker, t):
    ys, xs = np.nonzero(marker[:, :, t // 32] & np.uint32(1 << (t % 32)))
    return sorted((int(x) * 8, int(y) * 8) for x, y in zip(xs, ys))


def assert_rank_counts(rank_stats, single):
    """Counts of a sharded frame against the single-GPU frame's.  The instance cull is replicated (identical list, identical
    slots: the visibility ids agree); the occlusion culls of a rank run over the clusters that touch ITS screen tiles only, so
    per stage every rank counts at most the frame's clusters and together they count every one of them at least once
    (a cluster that touches tiles of two ranks is culled -- identically -- by both owners)."""
    assert all(st["overflow"] == 0 for st in rank_stats)
    assert all(st["countInstanceCulled"] == single["countInstanceCulled"] for st in rank_stats)
    for k in ("countStage0Visible", "countStage0Rejected", "countStage1Visible"):
        vals = [st[k] for st in rank_stats]
        assert max(vals) <= single[k], (k, vals, single[k])
        assert sum(vals) >= single[k], (k, vals, single[k])


def without_groups(scene):
    """The same assets and objects with every primitive's meshletGroupCount set to 0: a scene of no group instances (and no BVH,
    whose leaves would name groups the primitives no longer have)."""
    from chord_amd import records as R_
    prims = scene.primitives.copy()
    prims["meshletGroupCount"] = 0
    out = R_.Scene(scene.objects, prims, scene.materials, scene.meshlets, scene.groups, scene.group_indices, scene.meshlet_data,
                   scene.positions, name=scene.name + "+no_groups", texcoord0=scene.texcoord0, textures=scene.texture_images,
                   samplers=scene.samplers, bvh_nodes=None)
    out.local_to_world = scene.local_to_world
    return out


def hzb_levels(desc, chain):
    """The min chain as one float16-bit array per level, cut to the level's valid extent (spec_np.hzb_visible's layout)."""
    out = []
    for l in range(desc.mipCount):
        mw, mh = desc.mip_dims(l)
        vw, vh = desc.valid_dims(l)
        o = int(desc.mipOffset[l])
        out.append(np.asarray(chain[o: o + mw * mh]).reshape(mh, mw)[:vh, :vw].copy())
    return out


def hzb_with_upper_levels(desc, chain, value=None, first=6):
    """A copy of a min chain whose levels `first`.. hold `value` (binary16 bits), or -- value None -- the 2x2 min of the level
    below, edges clamped (what a chain built by the library holds there).  Only the valid extent of a level is written: texels
    past it are no pixel's, nothing samples them and no build writes them."""
    out = np.array(chain, dtype=np.uint16, copy=True)
    for l in range(first, desc.mipCount):
        mw, mh = desc.mip_dims(l)
        vw, vh = desc.valid_dims(l)
        lv = out[int(desc.mipOffset[l]): int(desc.mipOffset[l]) + mw * mh].reshape(mh, mw)
        if value is not None:
            lv[:vh, :vw] = value
            continue
        pw, ph = desc.mip_dims(l - 1)
        pvw, pvh = desc.valid_dims(l - 1)
        po = int(desc.mipOffset[l - 1])
        prev = out[po: po + pw * ph].view(np.float16).reshape(ph, pw)
        ys = np.minimum(np.arange(vh)[:, None] * 2 + np.arange(2)[None, :], pvh - 1)
        xs = np.minimum(np.arange(vw)[:, None] * 2 + np.arange(2)[None, :], pvw - 1)
        lv[:vh, :vw] = prev[ys[:, None, :, None], xs[None, :, None, :]].min(axis=(2, 3)).view(np.uint16)
    return out


def close_view_chain(scene, flags=ALL_FLAGS):
    """For scenes.group_count_scene at 640x360: the history chain of a view 0.4 m in front of the scene's first tile -- its clusters
    span hundreds of pixels, so a phase-0 cull from it tests them on HZB levels 6.. -- and the view of a frame a step further in
    that has it as its last frame: (chain, view, iv).  Leaves the object records filled for that frame."""
    import orc
    from chord_amd import lib as L
    occ = scenes.Camera((-3.3, -1.3, 0.4), (0.05, 0.03, -1.0), 640, 360)
    L.fill_objects(scene, occ)
    view_o, iv_o = L.make_views(occ)
    chain = orc.frame(scene, view_o, iv_o, flags)["hzb_min"]
    cam = occ.moved((0.02, 0.01, -0.03))
    L.fill_objects(scene, cam, occ)
    view, iv = L.make_views(cam, view_o)
    return chain, view, iv


# ---- sharded frames on one device: every rank a context of its own, the all-gathers replaced by device-to-device copies ----

def sharded_contexts(scene, view, iv, w, h, flags, ranks, tile_map="default", limits=None, debug_of_rank=None):
    """One context per rank of a `ranks`-rank frame on device 0, each with the scene, its rank and the view.  tile_map
    "checker" makes every tile border a rank border (chordvis_set_tile_owners); any other value keeps the library's compact
    regions.  debug_of_rank(rank) -> chordvis_set_debug flags (0 / None: none)."""
    from chord_amd.renderer import VisibilityRenderer
    from chord_amd.sharding import TileLayout
    lay = TileLayout(w, h, ranks)
    ctxs = []
    for rk in range(ranks):
        r = VisibilityRenderer(0)
        if limits:
            r.set_limits(**limits)
        r.upload_scene(scene)
        r.set_shard(ranks, rk)
        r.allocate_gbuffer(w, h)
        assert np.array_equal(r.tile_owners(), lay.owners)
        if tile_map == "checker":
            r.set_tile_owners([(t % lay.tiles_x + t // lay.tiles_x) % ranks for t in range(lay.tiles)])
        r.set_view(view, iv, flags)
        dbg = debug_of_rank(rk) if debug_of_rank else 0
        if dbg:
            r.set_debug(dbg)
        ctxs.append(r)
    return ctxs


def sharded_gather(ctxs, ptrs, chunk_bytes):
    """The all-gather of rank chunks: rank src's chunk src of each buffer is copied into every other rank's buffer."""
    import ctypes as C
    from chord_amd import lib as L
    hip = L._preload_hip_runtime()
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    for r in ctxs:
        r.sync()
    ranks = len(ctxs)
    for dst in range(ranks):
        for src in range(ranks):
            if src != dst:
                assert hip.hipMemcpy(ptrs[dst] + src * chunk_bytes, ptrs[src] + src * chunk_bytes, chunk_bytes, 3) == 0
    # a device-to-device hipMemcpy is ordered on the null stream only; the contexts run on non-blocking streams
    assert hip.hipDeviceSynchronize() == 0


def sharded_frame(ctxs, sharded_cull=True):
    """One frame on every rank: [phase cull, gather of the rank masks,] phase a, gather of the mid-frame HZB texels, phase b,
    gathers of the end-of-frame HZB texels and of the visibility words, phase c.  Without sharded_cull the frame starts at
    phase a (the replicated group cull)."""
    if sharded_cull:
        for r in ctxs:
            r.frame_phase_cull()
        cx = [r.cull_exchange() for r in ctxs]
        assert all(c[0] and c[1] == cx[0][1] for c in cx)
        sharded_gather(ctxs, [c[0] for c in cx], cx[0][1])
    for r in ctxs:
        r.frame_phase_a()
    ex = [r.hzb_exchange() for r in ctxs]
    sharded_gather(ctxs, [e[0] for e in ex], ex[0][2] * 2)
    for r in ctxs:
        r.frame_phase_b()
    fin = [r.hzb_final_exchange() for r in ctxs]
    sharded_gather(ctxs, [f[0] for f in fin], fin[0][1])
    sharded_gather(ctxs, [r.visibility_ptr() for r in ctxs], ctxs[0].visibility_chunk_words() * 8)
    for r in ctxs:
        r.frame_phase_c()


# ---- moving scenes (scenes.general_transform_scene and its kin): objects at local_to_world_at(k) under cams[k] in frame k ----

def moving_frame(scene, cams, k, prev_view=None):
    """Fills the object records for frame k of a moving sequence (this frame's transforms and camera, and the frame before's for
    the last-frame matrices; frame 0 has no frame before) and returns (view, iv).  prev_view: frame k - 1's view record.
    Side effect: scene.local_to_world is left at frame k's transforms (and scene.objects filled for frame k), so whoever sets the
    same scene object up afterwards starts from that frame, not from the builder's."""
    from chord_amd import lib as L
    scene.local_to_world = scene.local_to_world_at(k)
    L.fill_objects(scene, cams[k], cams[k - 1] if k else None, scene.local_to_world_at(k - 1) if k else None)
    return L.make_views(cams[k], prev_view)


def moving_sequence(scene, cams, flags=ALL_FLAGS, frames=None):
    """Generator over the frames of a moving sequence: yields (k, view, iv, want) with the object records filled for frame k and
    want = the oracle's frame against the oracle's chain of frame k - 1."""
    import orc
    prev_view, prev_hzb = None, None
    for k in range(len(cams) if frames is None else frames):
        view, iv = moving_frame(scene, cams, k, prev_view)
        want = orc.frame(scene, view, iv, flags, prev_hzb_min=prev_hzb)
        yield k, view, iv, want
        prev_view, prev_hzb = view, want["hzb_min"]


# ---- synthetic, caller-owned visibility images: what the image-reading kernels are never shown by a rasterised frame ----

F32_ONE = 0x3F800000
# per region kind, the weights of the value classes (zero, one, wide, normal, tie, subnormal, tiny) of synthetic_depth
_DEPTH_KINDS = np.array([[0.40, 0.08, 0.12, 0.10, 0.15, 0.08, 0.07],      # 1: the full mix
                         [0.00, 0.00, 0.00, 0.55, 0.45, 0.00, 0.00],      # 2: binary16 normals, no 0.0 and no 1.0
                         [0.00, 0.00, 0.00, 0.20, 0.20, 0.60, 0.00],      # 3: mostly binary16 subnormals, nothing that rounds to 0 but a tie
                         [0.00, 0.13, 0.00, 0.45, 0.42, 0.00, 0.00]])     # 4: just under 1.0, and 1.0


def synthetic_depth(w, h, seed):
    """float32[(h, w)] depths in [0, 1], seeded.  Every pixel draws its value from one of seven classes:
      zero       exactly 0.0                                         one   exactly 1.0
      wide       random mantissa, exponent 2^-57 .. 2^-1 (far below the binary16 subnormal range up to just under 1.0)
      normal     random mantissa, exponent inside the binary16 normal range, between the floor and the top of the pixel's 64-pixel
                 block and region kind
      tie        a binary16 normal's float bits with bit 12 set and the lower bits clear -- exactly half way to the next binary16 --
                 or the float one ulp below or above it: round-to-nearest-even differs from truncation on the tie and above, and
                 from round-half-up on the tie after an even binary16
      subnormal  2^-24 .. 2^-14 with a random mantissa, or the tie (k + 1/2) 2^-24 between two binary16 subnormals (k = 0: between
                 0 and the smallest) and its two float neighbours
      tiny       2^-87 .. 2^-25: below half of the smallest binary16 subnormal
    The class weights are not the same everywhere: about 10 % of all pixels are 0.0 and about 5 % are 1.0, but they sit in some
    regions only (a 4 x 4 grid of cells of different kinds, one kind a patchwork of 16-pixel blocks), and the normals of a 64-pixel
    block share an exponent range.  With the same weights at every pixel every texel from level 2 up would be min 0.0 / max 1.0
    and the upper levels of a chain would be checked on one value."""
    rng = np.random.default_rng([int(seed), int(w), int(h)])
    ys, xs = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]
    coarse = rng.permutation(np.arange(16) % 5).reshape(4, 4)               # every kind in at least three cells
    fine = rng.integers(1, 5, ((h + 15) // 16, (w + 15) // 16))
    kind = coarse[ys * 4 // h, xs * 4 // w]
    kind = np.where(kind == 0, fine[ys // 16, xs // 16], kind).ravel()
    floor = rng.integers(113, 126, ((h + 63) // 64, (w + 63) // 64))[ys // 64, xs // 64].ravel().astype(np.uint32)
    top = np.minimum(floor + np.uint32(3), np.uint32(126))                  # kind 2: a block's normals span four exponents
    top[kind == 1] = 126
    floor[kind == 3], top[kind == 3] = 113, 115
    floor[kind == 4], top[kind == 4] = 125, 126
    n = w * h
    u = rng.random(n, dtype=np.float32)
    cls = np.zeros(n, dtype=np.uint8)
    for k in range(1, 5):
        at = np.flatnonzero(kind == k)
        cls[at] = np.minimum(np.searchsorted(np.cumsum(_DEPTH_KINDS[k - 1]).astype(np.float32), u[at], side="right"), 6)
    r1 = rng.integers(0, 1 << 32, n, dtype=np.uint32)
    r2 = rng.integers(0, 1 << 32, n, dtype=np.uint32)
    mant, step = r1 & np.uint32(0x7FFFFF), ((r2 >> np.uint32(16)) % np.uint32(3)).astype(np.int64) - 1
    span = top + np.uint32(1) - floor
    exp_n = floor + (r2 & np.uint32(0xFFFF)) % span                          # float exponent field, floor .. top
    tie_n = (exp_n << np.uint32(23) | (r1 & np.uint32(0x3FF)) << np.uint32(13) | np.uint32(0x1000)).astype(np.int64) + step
    sub_tie = ((2 * (r1 & np.uint32(0x3FF)).astype(np.float64) + 1) * 2.0 ** -25).astype(np.float32).view(np.uint32).astype(np.int64) + step
    sub_rnd = (np.uint32(103) + (r2 & np.uint32(0xFFFF)) % np.uint32(10)) << np.uint32(23) | mant
    bits = np.select(
        [cls == 0, cls == 1, cls == 2, cls == 3, cls == 4, cls == 5],
        [0, F32_ONE, ((np.uint32(70) + (r2 & np.uint32(0xFFFF)) % np.uint32(57)) << np.uint32(23) | mant).astype(np.int64),
         (exp_n << np.uint32(23) | mant).astype(np.int64), tie_n,
         np.where((r2 >> np.uint32(31)) != 0, sub_tie, sub_rnd.astype(np.int64))],
        ((np.uint32(40) + (r2 & np.uint32(0xFFFF)) % np.uint32(62)) << np.uint32(23) | mant).astype(np.int64))
    depth = bits.astype(np.uint32).view(np.float32).reshape(h, w)
    assert (depth >= 0).all() and (depth <= 1).all()
    return depth


def depth_classes(depth):
    """How many pixels of a depth image are (exact binary16-normal ties after an even / after an odd binary16, in the binary16
    subnormal range, below half of the smallest subnormal, 0.0, 1.0): what synthetic_depth promises to contain."""
    d = np.asarray(depth, dtype=np.float32).ravel()
    b = d.view(np.uint32)
    tie = (d >= np.float32(2.0 ** -14)) & (d < 1) & ((b & np.uint32(0x1FFF)) == np.uint32(0x1000))
    odd = (b & np.uint32(0x2000)) != 0
    return dict(tie_even=int((tie & ~odd).sum()), tie_odd=int((tie & odd).sum()),
                subnormal=int(((d >= np.float32(2.0 ** -24)) & (d < np.float32(2.0 ** -14))).sum()),
                tiny=int(((d > 0) & (d < np.float32(2.0 ** -25))).sum()), zero=int((b == 0).sum()), one=int((b == F32_ONE).sum()))


def synthetic_words(depth, low):
    """Visibility words depth_bits << 32 | low, flattened row-major."""
    bits = np.ascontiguousarray(depth, dtype=np.float32).ravel().view(np.uint32).astype(np.uint64)
    return (bits << np.uint64(32)) | (np.asarray(low, dtype=np.uint64).ravel() & np.uint64(0xFFFFFFFF))


def valid_range_of(depth):
    """{min bits, max bits} of hzb_mip0_kernel's valid range, from its definition: the smallest bit pattern among 0 < d < 1, the
    largest among d > 0; {0xFFFFFFFF, 0} where no pixel qualifies."""
    d = np.ascontiguousarray(depth, dtype=np.float32).ravel()
    b = d.view(np.uint32)
    inner, pos = b[(d > 0) & (d < 1)], b[d > 0]
    return np.array([inner.min() if len(inner) else 0xFFFFFFFF, pos.max() if len(pos) else 0], dtype=np.uint32)


class CallerVisibility:
    """A visibility image the caller owns: a torch int64 tensor of w * h words on the renderer's device, handed to
    chordvis_allocate_gbuffer as deviceVisibility.  The context runs on a stream of its own, so every write into the tensor is
    followed by a device-wide synchronise before the library may be called, and the context is synchronised before the tensor is
    read.  The renderer keeps the tensor alive (the library holds only its address)."""

    def __init__(self, r, w, h):
        import torch
        self.r, self.w, self.h = r, w, h
        self.tensor = torch.zeros(w * h, dtype=torch.int64, device=torch.device("cuda", r.device))
        torch.cuda.synchronize()
        self.attach()
        r._caller_visibility = self.tensor

    def attach(self):
        self.r.allocate_gbuffer(self.w, self.h, device_visibility=self.tensor.data_ptr())

    def write(self, words):
        import torch
        words = np.ascontiguousarray(words, dtype=np.uint64)
        assert words.size == self.w * self.h
        self.r.sync()                                      # (nothing of the context's still reads the old image)
        self.tensor.copy_(torch.from_numpy(words.view(np.int64)))
        torch.cuda.synchronize()

    def read(self):
        self.r.sync()
        return self.tensor.cpu().numpy().view(np.uint64)


def marker_from_definition(scene, vis, w, h, cmds):
    """Per 8 x 8 pixels the set of shading types present, from the definition and for ANY low word: 0 -> type 0; an id field of 0
    or an id past the command list -> type 0 (no cluster); else the material type of the id's command's object."""
    low = (np.asarray(vis, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32).reshape(h, w)
    ident = ((low >> 8) & 0xFFFFFF).astype(np.int64)
    hit = (ident >= 1) & (ident <= len(cmds))
    typ = np.zeros((h, w), dtype=np.uint32)
    obj = np.asarray(cmds["objectId"], dtype=np.int64)
    typ[hit] = scene.materials["materialType"][scene.objects["GLTFMaterialData"][obj[ident[hit] - 1]]]
    marker = np.zeros(((h + 7) // 8, (w + 7) // 8, 4), dtype=np.uint32)
    ys, xs = np.nonzero(np.ones((h, w), dtype=bool))
    np.bitwise_or.at(marker, (ys // 8, xs // 8, (typ.ravel() // 32).astype(np.int64)), np.uint32(1) << (typ.ravel() % 32))
    return marker


# image sizes of the synthetic-image tests, chosen for what they do to the chain's layout (tests/test_synthetic_images_spec.py
# asserts each property from the descriptor)
HZB_SIZES = [(64, 64), (65, 64), (64, 127), (129, 67), (257, 64), (66, 2049), (2049, 65), (1237, 701)]
HZB_FULL_TAIL_SIZE = (4096, 4096)
DEPTH_VIEW_DIMS = [64, 96, 160]


def range_partial_count(w, h):
    """Blocks of hzb_mip0_kernel (64 x 4 mip-0 texels each) = valid-range partials the tail reduces."""
    vw, vh = ((w - 1) >> 1) + 1, ((h - 1) >> 1) + 1
    return ((vw + 63) // 64) * ((vh + 3) // 4)


# ---- hand-made screen-space triangles (tests/test_gpu_span_bounds.py, tests/alpha_chart.py) ----

def _unproject(view, iv, tris, w, h, dist0=5.0):
    """World positions (float32) whose projections are the given pixel positions, triangle k on the plane of view depth
    dist0 + k / 64 (no two triangles tie in depth)."""
    m = view["translatedWorldToClip"][0].reshape(4, 4).T.astype(np.float64)
    inv = np.linalg.inv(m)
    campos = np.frombuffer(iv["cameraWorldPos"][0].tobytes(), dtype=np.float64)[:3]
    out = []
    for k, tri in enumerate(tris):
        for (x, y) in tri:
            ndc = np.array([x / w * 2.0 - 1.0, 1.0 - y / h * 2.0])
            a = inv @ np.array([ndc[0], ndc[1], 0.5, 1.0]); a = a[:3] / a[3]
            b = inv @ np.array([ndc[0], ndc[1], 0.25, 1.0]); b = b[:3] / b[3]
            wa, wb = m[3] @ np.append(a, 1.0), m[3] @ np.append(b, 1.0)
            t = (dist0 + k / 64.0 - wa) / (wb - wa)
            out.append(campos + a + t * (b - a))
    pos = np.asarray(out, dtype=np.float32)
    # back through the matrix: the float32 positions land on the intended sub-pixels
    clip = m @ np.concatenate([pos.astype(np.float64) - campos, np.ones((len(pos), 1))], axis=1).T
    px, py = (clip[0] / clip[3] * 0.5 + 0.5) * w, (0.5 - clip[1] / clip[3] * 0.5) * h
    want = np.asarray([v for tri in tris for v in tri], dtype=np.float64)
    near = (np.abs(want) < 1000.0).all(axis=1)          # (the far vertices of GUARD only have to be far)
    assert np.abs(px - want[:, 0])[near].max() * 256 < 0.25 and np.abs(py - want[:, 1])[near].max() * 256 < 0.25, "a vertex misses its sub-pixel"
    return pos
