"""tests/meshlet_shapes.py against the oracle alone: what the scenes promise, so that tests/test_gpu_meshlet_shapes.py cannot pass
without running the shape-dependent code it is there for.  No GPU."""
import numpy as np
import pytest

import helpers as H
import meshlet_shapes as MS
import orc
from chord_amd import lib as L
from chord_amd import records as R

_CACHE = {}


def setup(variant):
    """(scene with its object records filled, camera, view, iv, the oracle's frame 0), made once."""
    if variant not in _CACHE:
        sc, cam = MS.scene(variant)
        L.fill_objects(sc, cam)
        view, iv = L.make_views(cam)
        _CACHE[variant] = (sc, cam, view, iv, orc.frame(sc, view, iv, H.ALL_FLAGS))
    return _CACHE[variant]


def _low(vis):
    return (np.asarray(vis, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def test_the_scene_holds_the_shape_list():
    sc, cam, _, _, want = setup("plain")
    tab = MS.meshlet_table(sc)
    shapes = [(V, T) for _, _, V, T, _ in tab]
    assert sorted(s for s in shapes if s != MS.EMPTY) == sorted(MS.SHAPES) and shapes.count(MS.EMPTY) == 1
    assert all(3 <= V <= 3 * T and V <= 255 and T <= 128 for V, T in MS.SHAPES)
    # the meshlet without triangles lies inside the stream, with words of other meshlets before and behind it
    (e_off,) = [off for _, _, V, T, off in tab if (V, T) == MS.EMPTY]
    assert 0 < e_off and e_off + MS.EMPTY[0] < len(sc.meshlet_data) - 3
    assert {off % 2 for _, _, _, _, off in tab} == {0, 1}, "odd and even dataOffsets"
    assert len(tab) == sum(V + T > 0 for V, T in shapes) and sum(V + T for V, T in shapes) == len(sc.meshlet_data)
    assert len(sc.primitives) >= 2 and (sc.primitives["vertexOffset"][1:] != 0).all()
    # groups: un-parented LOD-0 groups of 1, 2, 3 and 4 meshlets, every meshlet in exactly one
    assert set(sc.groups["meshletCount"].tolist()) == {1, 2, 3, 4}
    assert (sc.groups["parentError"] > 3.0e38).all() and (sc.groups["error"] < 0).all() and (sc.meshlets["lod"] == 0).all()
    assert int(sc.groups["meshletCount"].sum()) == len(sc.meshlets) and sc.bvh_nodes is not None and len(sc.bvh_nodes) == len(sc.primitives)
    not_ascending, shared = 0, 0
    for p, m, V, T, off in tab:
        base = int(sc.primitives[p]["vertexOffset"])
        ids = sc.meshlet_data[off: off + V].astype(np.int64)
        assert len(set(ids.tolist())) == V and ids.max() < int(sc.primitives[p]["vertexCount"])
        not_ascending += bool((np.diff(ids) < 0).any())
        tl = MS.triangle_locals(sc, m)
        assert tl.size == 0 or tl.max() < V
        if T:
            assert set(tl.ravel().tolist()) == set(range(V)), ("every local index is used", V, T)
            pos = sc.positions[base + ids].astype(np.float64)
            a, b, c = pos[tl[:, 0]], pos[tl[:, 1]], pos[tl[:, 2]]
            n = np.cross(b - a, c - a)
            assert (n[:, 2] > 0).all() and (np.linalg.norm(n, axis=1) > 1e-6).all(), "front-facing, not degenerate"
            zc = (a[:, 2] + b[:, 2] + c[:, 2]) / 3.0
            assert len(set(zc.tolist())) == T, "a depth of its own per triangle"
            assert len({tuple(sorted(t)) for t in tl.tolist()}) == T
            # the cone holds every triangle normal (or never culls)
            mm = sc.meshlets[m]
            if mm["coneCutOff"] < 1.0:
                dots = (n / np.linalg.norm(n, axis=1, keepdims=True)) @ mm["coneAxis"].astype(np.float64)
                assert (dots >= np.sqrt(1.0 - float(mm["coneCutOff"]) ** 2) - 1e-5).all()
        else:
            assert sc.meshlets[m]["coneCutOff"] == 1.0
        pos32 = sc.positions[base + ids]
        assert np.array_equal(sc.meshlets[m]["posMin"], pos32.min(axis=0)) and np.array_equal(sc.meshlets[m]["posMax"], pos32.max(axis=0))
        assert len({tuple(t) for t in sc.texcoord0[base + ids].tolist()}) == V, "a texture coordinate of its own per vertex"
    for p in range(len(sc.primitives)):
        sets = [set(sc.meshlet_data[off: off + V].tolist()) for q, _, V, _, off in tab if q == p]
        shared += sum(len(a & b) > 0 for a, b in zip(sets, sets[1:]))
    assert 2 * not_ascending >= len(MS.SHAPES), not_ascending
    assert shared >= 2, "meshlets of one primitive share global vertices"
    uv = sc.texcoord0
    assert uv is not None and len(uv) == len(sc.positions) and len({tuple(x) for x in uv.tolist()}) > 0.99 * len(uv)


def _owned(sc, want):
    """{meshlet id: (pixels, {band: pixels of triangles that use a vertex of the band})} of an oracle frame of one-instance scenes."""
    low = _low(want["vis"])
    hit = low != 0
    slot = ((low >> 8) & 0xFFFFFF).astype(np.int64) - 1
    tri = (low & 0xFF).astype(np.int64)
    meshlet_of_slot = np.full(int(want["cmds"]["slot"].max()) + 1, -1, dtype=np.int64)
    meshlet_of_slot[want["cmds"]["slot"]] = want["cmds"]["meshletId"]
    out = {}
    for _, m, V, T, _ in MS.meshlet_table(sc):
        px = hit & (meshlet_of_slot[np.where(hit, slot, 0)] == m)
        tl = MS.triangle_locals(sc, m)
        bands = {}
        for t, n in zip(*np.unique(tri[px], return_counts=True)):
            for b in set((tl[t] // 64).tolist()):
                bands[b] = bands.get(b, 0) + int(n)
        out[m] = (int(px.sum()), bands)
    return out


def test_plain_every_shape_and_every_band_owns_pixels():
    sc, cam, _, iv, want = setup("plain")
    assert (cam.width, cam.height) == (320, 200) and len(want["cmds"]) == len(sc.meshlets)        # nothing is culled
    owned = _owned(sc, want)
    for _, m, V, T, _ in MS.meshlet_table(sc):
        if T == 0:
            assert owned[m][0] == 0
            continue
        assert owned[m][0] >= 8, ((V, T), owned[m])
        for b in MS.bands_of(V):
            assert owned[m][1].get(b, 0) >= 1, ((V, T), "band", b, owned[m])
        x, y, w = MS.project(sc, iv, int(np.nonzero(sc.objects["GLTFPrimitiveDetail"] == _prim_of(sc, m))[0][0]), m)
        assert 10 <= max(x.max() - x.min(), y.max() - y.min()) <= 120 and (w > 0).all(), "tens of pixels across"
    assert want["stats"].trianglesClipped == 0 and want["stats"].trianglesSubmitted == sum(T for _, T in MS.SHAPES)


def _prim_of(sc, m):
    return int(np.searchsorted(sc.primitives["meshletOffset"], m, side="right") - 1)


@pytest.mark.parametrize("band", range(4))
def test_plain_image_depends_on_the_vertices_of_every_band(band):
    """Moving only what the clusters of more than 128 vertices hold at the band's local indices by about 2 pixels changes the
    oracle's image: a kernel that fetched or transformed that band wrongly cannot produce it."""
    sc, cam, view, iv, want = setup("plain")
    px = 2.0 * np.tan(0.5 * cam.fovy) * 6.6 / cam.height                     # a pixel in the primitives' space
    moved, n = MS.displaced(sc, band, (2.0 * px, 1.5 * px))
    assert n >= 9
    L.fill_objects(moved, cam)
    got = orc.frame(moved, view, iv, H.ALL_FLAGS)
    assert not np.array_equal(got["vis"], want["vis"])
    assert (got["vis"] != want["vis"]).sum() >= 8


def test_near_clips_triangles_of_the_large_clusters_only():
    sc, cam, view, iv, want = setup("near")
    assert want["stats"].trianglesClipped > 0
    large = np.nonzero(sc.objects["GLTFPrimitiveDetail"] == 2)[0]
    small = np.nonzero(sc.objects["GLTFPrimitiveDetail"] != 2)[0]
    assert all(V > 128 for p, _, V, _, _ in MS.meshlet_table(sc) if p == 2) and all(V <= 128 for p, _, V, _, _ in MS.meshlet_table(sc) if p != 2)
    alone = orc.frame(MS.only_objects(sc, large), view, iv, H.ALL_FLAGS)["stats"]
    others = orc.frame(MS.only_objects(sc, small), view, iv, H.ALL_FLAGS)["stats"]
    assert alone.trianglesClipped == want["stats"].trianglesClipped and others.trianglesClipped == 0 and others.trianglesSubmitted > 0
    # triangles that straddle the camera plane, per band of the local indices they use, among the clusters the oracle draws
    bands, shapes = set(), set()
    for c in want["cmds"]:
        m = int(c["meshletId"])
        _, _, w = MS.project(sc, iv, int(c["objectId"]), m)
        tl = MS.triangle_locals(sc, m)
        tw = w[tl]
        cross = ((tw > 0).any(axis=1) & (tw <= 0).any(axis=1)) if len(tl) else np.zeros(0, bool)
        if cross.any():
            assert len(w) > 128
            shapes.add(len(w))
            bands.update((tl[cross] // 64).ravel().tolist())
    assert bands == {0, 1, 2, 3} and max(shapes) > 192 and len(shapes) >= 4, (bands, shapes)


def test_masked_clips_fragments_and_differs_from_the_opaque_image():
    sc, cam, _, _, want = setup("masked")
    plain = setup("plain")[4]
    assert want["stats"].fragmentsClipped > 0 and want["stats"].trianglesSubmitted == plain["stats"].trianglesSubmitted
    assert not np.array_equal(want["vis"], plain["vis"])
    assert (sc.materials["alphaMode"][sc.objects["GLTFMaterialData"]] == R.ALPHA_MASK).all()
    # every masked shape keeps some pixels and loses some
    kept, full = _owned(sc, want), _owned(setup("plain")[0], plain)
    for _, m, V, T, _ in MS.meshlet_table(sc):
        if T >= 32:
            assert 0 < kept[m][0], ((V, T), kept[m][0], full[m][0])


def test_tiny_clusters_are_small_enough_for_pixel_blocks():
    sc, cam, view, iv, want = setup("tiny")
    assert want["stats"].trianglesClipped == 0
    small = tiles_ok = window_ok = large = 0
    for c in want["cmds"]:
        m = int(c["meshletId"])
        x, y, w = MS.project(sc, iv, int(c["objectId"]), m)
        assert (w > 0).all()
        if len(w) > 128:
            large += 1
            continue
        if (int(sc.meshlets[m]["vertexTriangleCount"]) >> 8) == 0:
            continue
        small += 1
        tiles_ok += (int(x.max()) // 64 - int(x.min()) // 64 <= 1) and (int(y.max()) // 64 - int(y.min()) // 64 <= 1)
        window_ok += max(x.max() - x.min(), y.max() - y.min()) <= 14.0            # (inside a 16-pixel block window, with room for snapping)
    assert small > 500 and large > 300, (small, large)
    assert 2 * tiles_ok > small and 2 * window_ok > small, (small, tiles_ok, window_ok)
    assert (_low(want["vis"]) != 0).sum() > 1000


@pytest.mark.parametrize("variant", ["plain", "masked", "near"])
def test_a_cut_sends_every_cluster_through_the_second_pass(variant):
    """meshlet_shapes.cut_last: after two still frames, the frame whose objects 'were' beside the screen has no cluster in its first
    pass and every one -- the 255-vertex clusters included, and for near the clipped triangles -- in its second."""
    sc, cam = MS.scene(variant)
    view0, _ = L.make_views(cam)
    view, iv = L.make_views(cam, view0)
    still = L.fill_objects(sc, cam, cam).copy()
    cut = L.fill_objects(sc.with_objects(sc.objects.copy()), cam, cam, MS.cut_last(sc, cam)).copy()
    prev = None
    for objs in (still, still, cut):
        want = orc.frame(sc.with_objects(objs), view, iv, H.ALL_FLAGS, prev_hzb_min=prev)
        prev = want["hzb_min"]
    n = len(want["cmds"])
    assert want["counts"].tolist() == [n, 0, n, n] and n >= len(MS.SHAPES)
    assert max(int(sc.meshlets[c["meshletId"]]["vertexTriangleCount"]) & 0xFF for c in want["cmds"]) == 255
    assert (want["stats"].trianglesClipped > 0) == (variant == "near")
