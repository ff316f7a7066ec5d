"""tests/spec_ray_tlas_np.py -- the TLAS of chordvis_rebuild_ray_tlas as a function of the object boxes -- held to a scalar evaluation
written with loops (one float32 operation per statement, struct-packed bit casts), on random lists and on the lists where the
statements have edges; and the shape's invariants from the offsets arithmetic alone, up to the 4^12 objects the depth allows.  CPU only."""
import struct

import numpy as np
import pytest

from chord_amd import records as R

import ray_tlas_cases as TC
import spec_ray_tlas_np as T

F = np.float32
U = np.uint32
SIZES = (1, 2, 4, 5, 16, 17, 64, 65, 257)


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def _mono(x):
    u = _bits(x)
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def _unmono(k):
    u = (k & 0x7FFFFFFF) if k & 0x80000000 else (~k & 0xFFFFFFFF)
    return F(struct.unpack("<f", struct.pack("<I", u))[0])


def scalar_tree(lo, hi):
    """(nodes as a list of dictionaries, leafRef list, depth) by loops."""
    n = len(lo)
    with np.errstate(all="ignore"):
        c = [[F(F(lo[i][a]) * F(0.5)) + F(F(hi[i][a]) * F(0.5)) for a in range(3)] for i in range(n)]
        blo = [_unmono(min(_mono(c[i][a]) for i in range(n))) for a in range(3)]
        bhi = [_unmono(max(_mono(c[i][a]) for i in range(n))) for a in range(3)]
        key = []
        for i in range(n):
            m = 0
            for a in range(3):
                extent = F(bhi[a] - blo[a])
                q = 0
                if (extent > F(0.0)) and (extent < F(3.0e38)):
                    scale = F(F(1024.0) / extent)
                    f = F(F(c[i][a] - blo[a]) * scale)
                    q = (int(f) if f < F(1024.0) else 1023) if f > F(0.0) else 0
                for k in range(10):
                    m |= ((q >> k) & 1) << (3 * k + a)
            key.append(m)
    order = sorted(range(n), key=lambda i: (key[i], i))
    cnt = [n]
    while True:
        cnt.append(-(-cnt[-1] // 4))
        if cnt[-1] == 1:
            break
    depth = len(cnt) - 1
    base = {depth: 0}
    for j in range(depth, 1, -1):
        base[j - 1] = base[j] + cnt[j]
    nodes = [None] * sum(cnt[1:])
    leaf_ref = [0] * n
    for p, o in enumerate(order):
        leaf_ref[o] = (base[1] + (p >> 2)) * 4 + (p & 3)
    boxes = [(list(map(F, lo[o])), list(map(F, hi[o]))) for o in order]
    for j in range(1, depth + 1):
        above = []
        for i in range(cnt[j]):
            children = min(4, cnt[j - 1] - 4 * i)
            nd = dict(lo=[[F(np.inf)] * 4 for _ in range(3)], hi=[[F(-np.inf)] * 4 for _ in range(3)], child=[T.NO_CHILD] * 4,
                      parentRef=T.NO_CHILD if j == depth else (base[j + 1] + (i >> 2)) * 4 + (i & 3), childCount=children)
            ulo = uhi = None
            for k in range(children):
                item = 4 * i + k
                nd["child"][k] = (T.LEAF << 30 | order[item]) if j == 1 else (T.NODE << 30 | (base[j - 1] + item))
                blo_k, bhi_k = boxes[item]
                for a in range(3):
                    nd["lo"][a][k], nd["hi"][a][k] = blo_k[a], bhi_k[a]
                if k == 0:
                    ulo, uhi = list(blo_k), list(bhi_k)
                else:
                    ulo = [ulo[a] if ulo[a] < blo_k[a] else blo_k[a] for a in range(3)]
                    uhi = [uhi[a] if uhi[a] > bhi_k[a] else bhi_k[a] for a in range(3)]
            above.append((ulo, uhi))
            nodes[base[j] + i] = nd
        boxes = above
    return nodes, leaf_ref, depth


def _hold(lo, hi, what):
    nodes, leaf_ref, s = T.tree(lo, hi)
    want, want_ref, depth = scalar_tree(lo, hi)
    assert s.depth == depth and s.nodes == len(want) == len(nodes), what
    assert leaf_ref.tolist() == want_ref, what
    for g, w in enumerate(want):
        nd = nodes[g]
        assert nd["child"].tolist() == w["child"] and int(nd["parentRef"]) == w["parentRef"] and int(nd["childCount"]) == w["childCount"], (what, g)
        assert nd["pad"].tolist() == [0, 0]
        assert nd["lo"].tobytes() == np.array(w["lo"], dtype=F).tobytes() and nd["hi"].tobytes() == np.array(w["hi"], dtype=F).tobytes(), (what, g)
    return nodes, leaf_ref, s


@pytest.mark.parametrize("n", SIZES)
def test_random_lists(n):
    lo, hi = TC.random_boxes(n, 7 + n)
    nodes, leaf_ref, s = _hold(lo, hi, "%d random boxes" % n)
    assert len(np.unique(T.keys(lo, hi))) > 1 or n == 1


def test_all_centres_equal():
    """Every key ties: the order is the index order."""
    lo, hi = TC.equal_centre_boxes(37)
    assert (T.keys(lo, hi) == 0).all() and T.order(lo, hi).tolist() == list(range(37))
    nodes, leaf_ref, s = _hold(lo, hi, "equal centres")
    assert leaf_ref.tolist() == [(s.base[1] + (p >> 2)) * 4 + (p & 3) for p in range(37)]


def test_centres_in_one_plane():
    """One axis without an extent: its ten bits are zero, the other two sort."""
    lo, hi = TC.plane_boxes(41, axis=1)
    q = T.quantise(T.centres(lo, hi), *T.centre_bounds(T.centres(lo, hi)))
    assert (q[:, 1] == 0).all() and q[:, 0].max() == 1023 and q[:, 2].max() == 1023
    _hold(lo, hi, "one plane")


def test_signed_zero_pair():
    """-0 and +0 are two values of the order: a list whose centres on an axis are only -0 and +0 has Blo = -0, Bhi = +0, an extent of
    0 and so no bits from that axis."""
    lo, hi = TC.signed_zero_boxes()
    c = T.centres(lo, hi)
    blo, bhi = T.centre_bounds(c)
    assert np.signbit(blo[0]) and blo[0] == 0 and not np.signbit(bhi[0]) and bhi[0] == 0
    assert T.mono(F(-0.0)) < T.mono(F(0.0))
    assert (T.quantise(c, blo, bhi)[:, 0] == 0).all()
    _hold(lo, hi, "signed zeros")


def test_one_nan_box():
    """A NaN centre goes to an end of the order, the extent is then a NaN and every q of the list is 0: the index order."""
    lo, hi = TC.random_boxes(19, 5)
    lo[7], hi[7] = np.nan, np.nan
    assert (T.keys(lo, hi) == 0).all() and T.order(lo, hi).tolist() == list(range(19))
    _hold(lo, hi, "a NaN box")


@pytest.mark.parametrize("n", SIZES + (4 ** 11 + 1, 4 ** 12))
def test_shape_invariants(n):
    """From the offsets arithmetic alone (no node table is made): every object in exactly one leaf slot, parentRef and the child words
    agree, every node but the root named once, at most 12 levels."""
    s = T.Shape(n)
    assert 1 <= s.depth <= T.MAX_DEPTH and s.cnt[0] == n and s.cnt[s.depth] == 1 and s.base[s.depth] == 0
    assert s.nodes == sum(s.cnt[1:]) and all(s.cnt[j] > 1 for j in range(1, s.depth))
    # the levels tile the node numbers 0 .. nodes - 1, the root first
    spans = sorted((s.base[j], s.base[j] + s.cnt[j]) for j in range(1, s.depth + 1))
    assert spans[0][0] == 0 and spans[-1][1] == s.nodes and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    # leaf slots: position p sits in node base[1] + p // 4, slot p % 4, which that node uses; the slots used at level 1 are n
    p = np.arange(n, dtype=np.int64)
    ref = (s.base[1] + (p >> 2)) * 4 + (p & 3)
    node, slot = ref >> 2, ref & 3
    assert len(np.unique(ref)) == n and (node >= s.base[1]).all() and (node < s.base[1] + s.cnt[1]).all()
    assert (slot < np.minimum(4, n - 4 * (node - s.base[1]))).all()
    for j in range(1, s.depth + 1):
        i = np.arange(s.cnt[j], dtype=np.int64)
        children = np.minimum(4, s.cnt[j - 1] - 4 * i)
        assert (children >= 1).all() and int(children.sum()) == s.cnt[j - 1]           # every item below is named once
        if j < s.depth:
            parent = (s.base[j + 1] + (i >> 2)) * 4 + (i & 3)
            pn, ps = parent >> 2, parent & 3
            pi = pn - s.base[j + 1]
            assert (pi >= 0).all() and (pi < s.cnt[j + 1]).all()
            assert (ps < np.minimum(4, s.cnt[j] - 4 * pi)).all()
            # ... and the parent's child word in that slot names this node
            assert ((s.base[j] + 4 * pi + ps) == s.base[j] + i).all()


def test_too_many_objects_are_refused():
    with pytest.raises(ValueError):
        T.Shape(4 ** 12 + 1)
    with pytest.raises(ValueError):
        T.Shape(0)
    assert T.Shape(4 ** 12).depth == 12 and T.Shape(4 ** 11 + 1).depth == 12 and T.Shape(4 ** 11).depth == 11
