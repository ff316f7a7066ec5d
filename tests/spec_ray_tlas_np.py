"""The specification of chordvis_rebuild_ray_tlas in numpy: the TLAS as a pure function of the object boxes (include/chordvis.h RAY
QUERIES, "rebuilding the TLAS"; chord_amd/csrc/ray_tlas_shape.h is the library's code of the same statements).

Arithmetic: binary32, one rounding per operation (numpy float32 arrays never contract), correctly rounded divide.  min / max of node
boxes are the selects of tests/spec_rays_np.py (rmin, rmax), folded over a node's children in slot order as the refit folds them.

    box        of object i: spec_rays_np.object_boxes
    centre     c[a] = lo[a] * 0.5 + hi[a] * 0.5
    bounds     Blo[a], Bhi[a]: min and max of c[a] under the total order of mono(c) = u & 0x80000000 ? ~u : u | 0x80000000 of the bits
               u: -0 below +0, a NaN at an end
    quantised  extent = Bhi[a] - Blo[a]; not (extent > 0) or not (extent < 3.0e38): q[a] = 0; else scale = 1024 / extent,
               f = (c[a] - Blo[a]) * scale, q[a] = f > 0 ? (f < 1024 ? (uint32) f : 1023) : 0 (a NaN f gives 0)
    key        bit 3 k + a of the 30-bit m is bit k of q[a]
    order      ascending (m, i)
    levels     cnt[0] = n, cnt[j] = ceil(cnt[j-1] / 4) up to the first j >= 1 with cnt[j] == 1: the depth D; D > 12 (n > 4^12) is refused
    numbering  base[D] = 0, base[j-1] = base[j] + cnt[j]; node (j, i) is base[j] + i
    words      childCount = min(4, cnt[j-1] - 4 i); child k = LEAF << 30 | order[4 i + k] for j == 1, else NODE << 30 | (base[j-1] + 4 i
               + k); unused slots: child 0xFFFFFFFF, lo = +inf, hi = -inf; parentRef = 0xFFFFFFFF for the root, else (base[j+1] +
               (i >> 2)) * 4 + (i & 3); pad = 0
    leafRef    leafRef[order[p]] = (base[1] + (p >> 2)) * 4 + (p & 3)
    boxes      a level-1 slot holds its object's box; a higher slot the fold of the child node's used slots
"""
import numpy as np

from chord_amd import records as R

import spec_rays_np as S

F = np.float32
U = np.uint32
MAX_DEPTH = 12
MAX_OBJECTS = 4 ** MAX_DEPTH
NODE, LEAF, NO_CHILD = 0, 1, 0xFFFFFFFF


class Shape:
    """depth D, cnt[0 .. D], base[1 .. D] (base[0] is None), nodes."""
    def __init__(self, n):
        n = int(n)
        if n < 1 or n > MAX_OBJECTS:
            raise ValueError("a TLAS over %d objects: 1 .. 4^12 objects" % n)
        cnt = [n]
        while True:
            cnt.append((cnt[-1] + 3) // 4)
            if cnt[-1] == 1:
                break
        self.depth = len(cnt) - 1
        assert self.depth <= MAX_DEPTH
        base = [None] * (self.depth + 1)
        base[self.depth] = 0
        for j in range(self.depth, 1, -1):
            base[j - 1] = base[j] + cnt[j]
        self.cnt, self.base, self.nodes = cnt, base, sum(cnt[1:])


def mono(x):
    u = np.asarray(x, dtype=F).view(U)
    return np.where(u & U(0x80000000), ~u, u | U(0x80000000)).astype(U)


def unmono(k):
    k = np.asarray(k, dtype=U)
    return np.where(k & U(0x80000000), k & U(0x7FFFFFFF), ~k).astype(U).view(F)


def centres(lo, hi):
    with np.errstate(all="ignore"):
        return (np.asarray(lo, dtype=F) * F(0.5) + np.asarray(hi, dtype=F) * F(0.5)).astype(F)


def centre_bounds(c):
    k = mono(c)
    return unmono(k.min(axis=0)), unmono(k.max(axis=0))


def quantise(c, blo, bhi):
    """uint32 (n, 3)"""
    with np.errstate(all="ignore"):
        extent = (bhi - blo).astype(F)
        usable = (extent > F(0.0)) & (extent < F(3.0e38))
        scale = (F(1024.0) / extent).astype(F)
        f = ((c - blo).astype(F) * scale).astype(F)
        inside = usable[None, :] & (f > F(0.0)) & (f < F(1024.0))
        q = np.where(inside, f, F(0.0)).astype(np.int64)                  # (truncation of a value in (0, 1024))
        q = np.where(usable[None, :] & (f >= F(1024.0)), 1023, q)          # (f > 0 and not f < 1024, f not a NaN)
    return q.astype(U)


def morton(q):
    m = np.zeros(len(q), dtype=U)
    for k in range(10):
        for a in range(3):
            m |= ((q[:, a] >> U(k)) & U(1)) << U(3 * k + a)
    return m


def keys(lo, hi):
    c = centres(lo, hi)
    blo, bhi = centre_bounds(c)
    return morton(quantise(c, blo, bhi))


def order(lo, hi):
    m = keys(lo, hi)
    return np.lexsort((np.arange(len(m)), m)).astype(U)


def tree(lo, hi):
    """(records.RAY_NODE nodes with every box, uint32 leafRef, Shape) over the boxes lo, hi float32 (n, 3)."""
    lo, hi = np.asarray(lo, dtype=F), np.asarray(hi, dtype=F)
    n = len(lo)
    s = Shape(n)
    od = order(lo, hi)
    nodes = np.zeros(s.nodes, dtype=R.RAY_NODE)
    nodes["lo"], nodes["hi"], nodes["child"] = np.inf, -np.inf, NO_CHILD
    leaf_ref = np.zeros(n, dtype=U)
    p = np.arange(n)
    leaf_ref[od] = (s.base[1] + (p >> 2)) * 4 + (p & 3)
    below_lo, below_hi = lo[od], hi[od]                                    # the boxes of level j - 1's items, in their order
    for j in range(1, s.depth + 1):
        cnt, below = s.cnt[j], s.cnt[j - 1]
        i = np.arange(cnt)
        lv = nodes[s.base[j]: s.base[j] + cnt]                             # (a view)
        children = np.minimum(4, below - 4 * i)
        lv["childCount"] = children
        lv["parentRef"] = NO_CHILD if j == s.depth else (s.base[j + 1] + (i >> 2)) * 4 + (i & 3)
        union_lo = union_hi = None
        for k in range(4):
            used = k < children
            item = np.minimum(4 * i + k, below - 1)
            word = (LEAF << 30 | od[item].astype(np.int64)) if j == 1 else (NODE << 30 | (s.base[j - 1] + item))
            lv["child"][:, k] = np.where(used, word, NO_CHILD)
            blo_k, bhi_k = below_lo[item], below_hi[item]
            lv["lo"][:, :, k] = np.where(used[:, None], blo_k, F(np.inf))
            lv["hi"][:, :, k] = np.where(used[:, None], bhi_k, F(-np.inf))
            if k == 0:
                union_lo, union_hi = blo_k, bhi_k
            else:
                union_lo = np.where(used[:, None], S.rmin(union_lo, blo_k), union_lo)
                union_hi = np.where(used[:, None], S.rmax(union_hi, bhi_k), union_hi)
        below_lo, below_hi = union_lo.astype(F), union_hi.astype(F)
    return nodes, leaf_ref, s


def root_box(nodes):
    """(lo, hi) float32 (3,): the fold of the root's used slots, what chordvis_ray_scene_info reports."""
    nd = nodes[0]
    lo, hi = nd["lo"][:, 0], nd["hi"][:, 0]
    for k in range(1, int(nd["childCount"])):
        lo, hi = S.rmin(lo, nd["lo"][:, k]), S.rmax(hi, nd["hi"][:, k])
    return lo.astype(F), hi.astype(F)


def tree_of_objects(objects, primitives):
    lo, hi = S.object_boxes(np.ascontiguousarray(objects, dtype=R.OBJECT), primitives)
    return tree(lo, hi)
