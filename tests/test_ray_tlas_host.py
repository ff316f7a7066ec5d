"""chord_amd/csrc/ray_tlas_shape.h -- the functions chordvis_rebuild_ray_tlas's kernels call per object and per node -- compiled by the
host compiler with -fsanitize=address,undefined into a program of its own (tests/ray_tlas_main.cpp: its own main, no Python in the
process) and held word for word to tests/spec_ray_tlas_np.py.  The program keeps the node table and the leaf references in heap
allocations of exactly their size, so a node or an object index one past the shape's counts ends it with a sanitizer report; the bare
shape at 4^12 objects, the most the depth allows, is written whole and summed.  Built with -ffp-contract=off as the kernels are.  CPU
only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from chord_amd import records as R

import ray_tlas_cases as TC
import spec_ray_tlas_np as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U = np.float32, np.uint32


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("ray_tlas") / "ray_tlas_check")
    cc = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "chord_amd", "csrc"),
                         os.path.join(ROOT, "tests", "ray_tlas_main.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, cc      # (a build that fails is every test's failure, asserted where the program is run)


def _run(program, tmp_path, mode, n, boxes=None, expect=0):
    parts = [np.array([mode, n, 0, 0, 0, 0, 0, 0], dtype=U)]
    if boxes is not None:
        parts.append(np.ascontiguousarray(np.concatenate([boxes[0], boxes[1]], axis=1), dtype=F).view(U).reshape(-1))
    req, ans = os.path.join(str(tmp_path), "request.bin"), os.path.join(str(tmp_path), "answer.bin")
    np.concatenate(parts).tofile(req)
    exe, cc = program
    assert cc.returncode == 0, "tests/ray_tlas_main.cpp does not build against chord_amd/csrc/ray_tlas_shape.h:\n" + cc.stderr[-3000:]
    p = subprocess.run([exe, req, ans], capture_output=True, text=True, timeout=300)
    assert p.returncode == expect, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
    return np.fromfile(ans, dtype=U) if expect == 0 else None


def _hold(program, tmp_path, lo, hi, what):
    want, want_ref, s = T.tree(lo, hi)
    out = _run(program, tmp_path, 0, len(lo), (lo, hi))
    assert (int(out[0]), int(out[1])) == (s.depth, s.nodes), what
    nodes = out[8: 8 + 32 * s.nodes].view(R.RAY_NODE)
    leaf_ref = out[8 + 32 * s.nodes:]
    assert np.array_equal(leaf_ref, want_ref), what
    for f in ("child", "parentRef", "childCount", "pad"):
        assert np.array_equal(nodes[f], want[f]), (what, f)
    assert nodes.tobytes() == want.tobytes(), (what, "boxes")


@pytest.mark.parametrize("n", (1, 2, 4, 5, 16, 17, 64, 65, 257, 4097))
def test_random_lists(program, tmp_path, n):
    lo, hi = TC.random_boxes(n, 7 + n)
    _hold(program, tmp_path, lo, hi, "%d random boxes" % n)


def test_edge_lists(program, tmp_path):
    _hold(program, tmp_path, *TC.equal_centre_boxes(37), "equal centres")
    _hold(program, tmp_path, *TC.plane_boxes(41, axis=1), "one plane")
    _hold(program, tmp_path, *TC.signed_zero_boxes(), "signed zeros")
    lo, hi = TC.random_boxes(19, 5)
    lo[7], hi[7] = np.nan, np.nan
    want, want_ref, s = T.tree(lo, hi)
    out = _run(program, tmp_path, 0, 19, (lo, hi))                          # (a NaN box: the words, not the boxes, are compared bytewise too)
    assert out[8: 8 + 32 * s.nodes].view(R.RAY_NODE).tobytes() == want.tobytes() and np.array_equal(out[8 + 32 * s.nodes:], want_ref)
    lo, hi = TC.random_boxes(23, 9)
    lo[:, 2], hi[:, 2] = -3.0e38, -3.0e38                                   # centres 6e38 apart: the extent overflows, no bits from that axis
    lo[5, 2], hi[5, 2] = 3.0e38, 3.0e38
    assert (T.quantise(T.centres(lo, hi), *T.centre_bounds(T.centres(lo, hi)))[:, 2] == 0).all()
    _hold(program, tmp_path, lo, hi, "an extent beyond 3e38")


def _sums(n):
    """The four sums of tests/ray_tlas_main.cpp's mode 1 from the offsets arithmetic alone, modulo 2^64."""
    s = T.Shape(n)
    u64 = np.uint64
    child = parent = count = u64(0)
    with np.errstate(over="ignore"):
        for j in range(1, s.depth + 1):
            i = np.arange(s.cnt[j], dtype=u64)
            g = u64(s.base[j]) + i
            children = np.minimum(u64(4), u64(s.cnt[j - 1]) - u64(4) * i)
            for k in range(4):
                item = u64(4) * i + u64(k)
                word = (u64(T.LEAF << 30) | item) if j == 1 else (u64(T.NODE << 30) | (u64(s.base[j - 1]) + item))
                word = np.where(u64(k) < children, word, u64(T.NO_CHILD))
                child = child + (word * (u64(4) * g + u64(k + 1))).sum(dtype=u64)
            ref = u64(T.NO_CHILD) if j == s.depth else (u64(s.base[j + 1]) + (i >> u64(2))) * u64(4) + (i & u64(3))
            parent = parent + (ref * (g + u64(1))).sum(dtype=u64)
            count = count + children.sum(dtype=u64)
        p = np.arange(n, dtype=u64)
        leaf = (((u64(s.base[1]) + (p >> u64(2))) * u64(4) + (p & u64(3))) * (p + u64(1))).sum(dtype=u64)
    return s, [int(child), int(parent), int(count), int(leaf)]


@pytest.mark.parametrize("n", (1, 5, 4 ** 6 + 1, 4 ** 12))
def test_bare_shape(program, tmp_path, n):
    """Every node and every leaf reference of the shape over n objects written into allocations of exactly their size: at 4^12 objects
    the twelve levels the traversal stack is sized for."""
    s, want = _sums(n)
    out = _run(program, tmp_path, 1, n)
    assert (int(out[0]), int(out[1])) == (s.depth, s.nodes)
    got = [int(out[2 + 2 * i]) | int(out[3 + 2 * i]) << 32 for i in range(4)]
    assert got == want
    if n == 4 ** 12:
        assert s.depth == 12 and want[2] == s.nodes - 1 + n


def test_refused_counts(program, tmp_path):
    _run(program, tmp_path, 1, 4 ** 12 + 1, expect=3)
    _run(program, tmp_path, 1, 0, expect=3)
