"""The select form of the row-span bounds (chord_amd/csrc/span_bounds.h) against the if / else-if ladder it replaced, and the
form that takes ready-made reciprocals against the one that computes them: tests/span_bounds_equal_main.cpp is built with the
host compiler as a program of its own and run, as tests/test_span_bounds.py does; it holds a frozen copy of the ladder and the
sweeps, and asks for the same (k0, k1) on every input."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CLASSES = ("empty", "on_centre", "zero_neg", "zero_zero", "zero_pos", "assign_below", "nan_q", "far_left", "far_right", "clamp_lo", "clamp_hi",
           "n0", "n63")


def _compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if cxx and shutil.which(cxx):
            return cxx
    return None


def _run(tmp_path, *defines):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = os.path.join(str(tmp_path), "span_bounds_equal")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "chord_amd", "csrc"), *defines,
                           os.path.join(ROOT, "tests", "span_bounds_equal_main.cpp"), "-o", exe, "-lm"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr)
    m = re.search(r"kinds (\d+) (\d+) (\d+)", p.stdout)
    counts = {k: int(v) for k, v in re.findall(r"([a-z_]\w*) (-?\d+)", p.stdout)}
    counts["per_kind"] = [int(v) for v in m.groups()] if m else [0, 0, 0]
    return p, counts


@pytest.mark.parametrize("defines", [("-DSPAN_STRAIGHT=1",), ("-DSPAN_STRAIGHT=1", "-DSPAN_SLACK_LEGACY=1"), ()], ids=["selects", "selects_legacy_slack", "product"])
def test_select_form_and_reciprocal_form_return_the_ladders_bounds(tmp_path, defines):
    """Zero differences over the lattice of int32-kind triangles in a 64-px box, seeded triangles of all three kinds, raw edge
    values and steps up to 2^62 / 2^40, zero steps with E <, ==, > 0 (the constant-and-outside case also behind an edge that had
    left the right bound below -1: assign_below), crossings on pixel centres, both clamp values, n = 0 and 63, three reciprocals
    (exact, +-1 ulp); span_bounds() and span_bounds_rcp() with float and with integer steps.  Every case class occurred."""
    p, c = _run(tmp_path, *defines)
    assert p.returncode == 0, p.stdout + p.stderr
    assert c["differences"] == 0
    assert c["rows"] > 1000000 and c["compared"] == 9 * c["rows"]
    assert all(v > 10000 for v in c["per_kind"]), c["per_kind"]
    for k in CLASSES:
        assert c[k] > 0, k


