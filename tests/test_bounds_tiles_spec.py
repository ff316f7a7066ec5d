"""chordvis_bin_bounds on the CPU: the records of the header, records.py and lib.py agree; the vectorised numpy restatement of the
contract (spec_bounds_tiles_np) equals a plain loop over every (query, tile) pair; chordvis_bounds_tile_count counts as the contract
says; and the rendered-frame input of tests/test_gpu_bounds_tiles.py reaches every way the pair test can go.  Runs without a GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import bounds_scenes as B
import bounds_tiles_cases as K
import helpers as H
import spec_bounds_query_np as Q
import spec_bounds_tiles_np as S
from chord_amd import records as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile_records_match_the_header_and_the_calls_are_exported(built_lib):
    L = built_lib
    numpy_mirrors = {"ChordBoundsTilesDesc": R.BOUNDS_TILES_DESC, "ChordBoundsTiles": R.BOUNDS_TILES}
    ctypes_mirrors = {"ChordBoundsTilesDesc": L.BoundsTilesDesc, "ChordBoundsTiles": L.BoundsTiles}
    lines = []
    for cname, dt in numpy_mirrors.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in dt.names:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    for name in ("NEAR", "FAR"):
        lines.append('printf("%s %%u\\n", (unsigned)CHORD_BOUNDS_TILES_%s);' % (name, name))
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "chordvis.h"\nint main(void){\n%s\nreturn 0;}\n' % "\n".join(lines)
    with tempfile.TemporaryDirectory() as td:
        cpath, exe = os.path.join(td, "l.c"), os.path.join(td, "l")
        open(cpath, "w").write(src)
        cc = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), cpath, "-o", exe], capture_output=True, text=True)
        assert cc.returncode == 0, cc.stderr[-1500:]
        out = dict(l.split() for l in subprocess.check_output([exe]).decode().splitlines())
    assert [int(out["ChordBoundsTilesDesc"]), int(out["ChordBoundsTiles"])] == [16, 32]
    for cname, dt in numpy_mirrors.items():
        ct = ctypes_mirrors[cname]
        assert int(out[cname]) == dt.itemsize == C.sizeof(ct), cname
        assert [f for f, _ in ct._fields_] == list(dt.names), cname
        for f in dt.names:
            assert int(out["%s.%s" % (cname, f)]) == dt.fields[f][1] == getattr(ct, f).offset, (cname, f)
    assert (int(out["NEAR"]), int(out["FAR"])) == (R.BOUNDS_TILES_NEAR, R.BOUNDS_TILES_FAR) == (1, 2)
    assert "chordvis_bin_bounds" in L.EXPORTED and "chordvis_bounds_tile_count" in L.EXPORTED


@pytest.mark.parametrize("size", [(64, 64), (160, 96), (641, 377), (3840, 2160), (4096, 4096), (65, 129)], ids=lambda s: "%dx%d" % s)
def test_tile_count_for_exact_and_partial_sizes(built_lib, size):
    w, h = size
    for T in (8, 16, 32, 64):
        tx, ty = C.c_uint32(77), C.c_uint32(77)
        n = built_lib.lib.chordvis_bounds_tile_count(w, h, T, C.byref(tx), C.byref(ty))
        assert (n, tx.value, ty.value) == S.tile_count(w, h, T) == ((w + T - 1) // T * ((h + T - 1) // T), (w + T - 1) // T, (h + T - 1) // T)
        assert built_lib.lib.chordvis_bounds_tile_count(w, h, T, None, None) == n
    for T in (0, 1, 4, 12, 24, 128, 65):
        tx, ty = C.c_uint32(77), C.c_uint32(77)
        assert built_lib.lib.chordvis_bounds_tile_count(w, h, T, C.byref(tx), C.byref(ty)) == 0 == S.tile_count(w, h, T)[0]
        assert (tx.value, ty.value) == (0, 0)


def _loop(words, w, h, results, T, max_per_tile, flags, farz):
    """The contract, one (query, tile) pair at a time."""
    d = (np.asarray(words, dtype=np.uint64) >> np.uint64(32)).astype(np.uint32).reshape(h, w)
    tx, ty = (w + T - 1) // T, (h + T - 1) // T
    counts = np.zeros(tx * ty, dtype=np.uint32)
    items = np.full((tx * ty, max_per_tile), S.FILL, dtype=np.uint32)
    depth = np.zeros((tx * ty, 2), dtype=np.uint32)
    taking_part = 0
    for i, r in enumerate(results):
        if (int(r["status"]) & 3) == 3:
            taking_part += 1
    for t in range(tx * ty):
        x0, y0 = (t % tx) * T, (t // tx) * T
        x1, y1 = min(w, x0 + T) - 1, min(h, y0 + T) - 1
        tile = d[y0:y1 + 1, x0:x1 + 1]
        depth[t] = (tile.min(), tile.max())
        zfar, znear = np.uint32(depth[t, 0]).view(np.float32), np.uint32(depth[t, 1]).view(np.float32)
        for i, r in enumerate(results):
            if (int(r["status"]) & 3) != 3:
                continue
            rect = [int(v) for v in r["rect"]]
            if not (rect[0] <= x1 and rect[2] >= x0 and rect[1] <= y1 and rect[3] >= y0):
                continue
            if (flags & 1) and np.float32(r["nearestZ"]) < zfar:
                continue
            if (flags & 2) and np.float32(farz[i]) > znear:
                continue
            if counts[t] < max_per_tile:
                items[t, counts[t]] = i
            counts[t] += 1
    totals = np.array([taking_part, int(counts.astype(np.int64).sum()) & 0xFFFFFFFF, int((counts > max_per_tile).sum()), int(counts.max())], dtype=np.uint32)
    return dict(counts=counts, items=items, depth=depth, totals=totals)


@pytest.mark.parametrize("flags", (0, 1, 2, 3))
def test_vectorised_spec_equals_the_pair_loop(flags):
    w, h, T, n, cap = 70, 45, 16, 120, 20
    depth_img = H.synthetic_depth(w, h, 5)
    words = H.synthetic_words(depth_img, np.arange(w * h))
    results = K.handmade_results(w, h, T, S.tile_depth(words, w, h, T), n, seed=3)
    rng = np.random.default_rng(8)
    farz = np.where(rng.random(n) < 0.3, 0.0, rng.random(n) * depth_img.max()).astype(np.float32)
    want = _loop(words, w, h, results, T, cap, flags, farz)
    got = S.bin_bounds(words, w, h, results, T, cap, flags, farz)
    for k in ("counts", "items", "depth", "totals"):
        assert np.array_equal(got[k], want[k]), k
    if flags == 0:
        assert want["totals"][2] > 0 and (want["counts"] < cap).any(), "the tiny case has tiles beyond and below maxPerTile"
    if flags:
        assert not np.array_equal(want["counts"], _loop(words, w, h, results, T, cap, 0, farz)["counts"]), "the depth sides reject something"


@pytest.fixture(scope="module")
def rendered(built_lib):
    """The rendered-frame case on the oracle: its image of the second of two frames, the spec's results for the boxes against the
    chain that frame left."""
    import orc
    scene, cam_last, cam, (view_last, iv_last), (view, iv), queries = K.rendered_boxes()
    B.fill_for(scene, cam_last)
    first = orc.frame(scene, view_last, iv_last, H.ALL_FLAGS)
    B.fill_for(scene, cam, cam_last)
    second = orc.frame(scene, view, iv, H.ALL_FLAGS, prev_hzb_min=first["hzb_min"])
    return dict(view=view, iv=iv, queries=queries, words=second["vis"], desc=second["desc"], chain=second["hzb_min"])


@pytest.mark.parametrize("phase", (1, 0))
def test_the_rendered_frame_input_reaches_every_class(rendered, phase):
    w, h = K.RENDERED_SIZE
    T, cap = K.RENDERED_TILE, K.RENDERED_MAX_PER_TILE
    r = rendered
    results, _, visible = Q.query_bounds(r["view"], r["iv"], r["queries"], phase, r["desc"], r["chain"])
    farz = S.far_z(r["view"], r["iv"], r["queries"], phase, results["status"])
    flags = R.BOUNDS_TILES_NEAR | R.BOUNDS_TILES_FAR
    overlap, near_rej, far_rej, idx = S.pair_classes(r["words"], w, h, results, T, flags, farz)
    assert len(idx) == visible > 0
    classes = dict(rectangle_miss=int((~overlap).sum()), near_rejected=int((overlap & near_rej).sum()),
                   far_rejected=int((overlap & ~near_rej & far_rej).sum()), kept=int((overlap & ~near_rej & ~far_rej).sum()))
    out = S.bin_bounds(r["words"], w, h, results, T, cap, flags, farz)
    print("phase %d: %d of %d boxes take part; pairs %s; totals %s" % (phase, visible, len(results), classes, out["totals"].tolist()))
    assert all(v > 0 for v in classes.values()), classes
    assert out["totals"][2] > 0 and out["totals"][3] > cap, "no tile overflows maxPerTile"
    assert (out["counts"] < cap).any(), "every tile overflows"
    assert out["totals"][1] == classes["kept"] == int(out["counts"].sum()) and out["totals"][0] == visible
    # a tile of empty pixels under FAR keeps only the NEAR records
    empty = out["depth"][:, 1] == 0
    assert empty.any() and not empty.all(), "the frame has empty tiles and covered ones"
    near_records = (results["status"][idx] & R.BOUNDS_NEAR) != 0
    keep = overlap & ~near_rej & ~far_rej
    assert near_records.any() and not keep[~near_records][:, empty].any()


@pytest.mark.parametrize("T", (8, 16, 32, 64))
def test_the_piled_input_fills_the_candidate_list_mid_stream(T):
    """tests/test_gpu_bounds_tiles.py's piled records make the tile kernel flush a full candidate list before its last chunk, at
    both chunk sizes and more than once -- and none of the suite's other hand-made inputs does, which is why the case exists."""
    w, h = 160, 96
    words = H.synthetic_words(H.synthetic_depth(w, h, 6), np.zeros(w * h))
    depth = S.tile_depth(words, w, h, T)
    piled = K.piled_results(w, h, T, depth, 2000, seed=5)
    assert S.participates(piled).all()
    assert K.midstream_flushes(piled, w, h, K.CHUNK) >= 2 and K.midstream_flushes(piled, w, h, K.CHUNK_DEBUG) >= 2
    plain = K.handmade_results(w, h, T, depth, 1000, seed=2)
    assert K.midstream_flushes(plain, w, h, K.CHUNK) == 0 and K.midstream_flushes(plain, w, h, K.CHUNK_DEBUG) == 0
