"""The row-span bounds of the tile kernel's scan loops (chord_amd/csrc/span_bounds.h) on the host: tests/span_bounds_main.cpp is
built with the host compiler as a program of its own and run; it holds the sweeps, the exact integer reference and both
conditions (no covered step cut; at most one step of excess at either end)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if cxx and shutil.which(cxx):
            return cxx
    return None


def _run(tmp_path, *defines):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = os.path.join(str(tmp_path), "span_bounds_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "chord_amd", "csrc"), *defines,
                           os.path.join(ROOT, "tests", "span_bounds_main.cpp"), "-o", exe, "-lm"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr)
    counts = {k: int(v) for k, v in re.findall(r"([a-z_]\w*) (-?\d+)", p.stdout)}
    return p, counts


def test_span_bounds_cut_no_covered_pixel_and_scan_at_most_two_more(tmp_path):
    """Exhaustive over a lattice of int32-kind triangles in a 64-px box, seeded random triangles of all three kinds, and edge
    values / steps straight from their ranges (up to 2^62 and 2^40) with crossings on pixel centres, at the clamp values and far off
    the row; three reciprocals (exact, +-1 ulp).  The program exits 0 only if no bound cut a covered step, no loop was more than
    2 steps longer than the covered interval (1 at either end), and every case class occurred."""
    p, c = _run(tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    assert c["violations"] == 0 and c["loose"] == 0 and c["max_excess"] <= 2
    assert c["rows"] > 1000000 and c["covered"] > 100000
    for k in ("on_centre_biased", "on_centre_unbiased", "zero_neg", "zero_zero", "zero_pos", "zero_at_start", "far_left", "far_right",
              "clamp_lo", "clamp_hi", "n0", "n63"):
        assert c[k] > 0, k


def test_legacy_bounds_of_the_measurement_variant_cut_no_covered_pixel(tmp_path):
    """-DSPAN_SLACK_LEGACY=1 (the variant the change is measured against) returns the earlier, wider bounds: safe as well."""
    p, c = _run(tmp_path, "-DSPAN_SLACK_LEGACY=1")
    assert p.returncode == 0, p.stdout + p.stderr
    assert c["violations"] == 0
