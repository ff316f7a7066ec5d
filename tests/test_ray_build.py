"""The host builder of the ray scene's trees (chord_amd/csrc/ray_scene.cpp) on the CPU: tests/ray_build_main.cpp and the builder are
compiled together by the host compiler with -fsanitize=address,undefined into a program of its own, and run.  The program builds
BLAS-shaped trees for a one-triangle primitive, 1 024 coincident triangles, a 255-vertex meshlet's 85 triangles, a random mesh,
exponentially spaced boxes and the two trees of the deep ray scene (exactly 12 levels each), refuses an empty input, builds TLAS-shaped trees for 1, 2, 9 and 600 boxes, and checks leaf membership,
exact union boxes, the depth bound and byte-identical rebuilds (see its header comment)."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cxx and shutil.which(cxx):
            return cxx
    return None


def test_ray_tree_builder_under_sanitizers(tmp_path):
    cxx = _compiler()
    assert cxx is not None, "no host C++ compiler"
    csrc = os.path.join(ROOT, "chord_amd", "csrc")
    exe = os.path.join(str(tmp_path), "ray_build_check")
    cc = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-I", csrc, os.path.join(csrc, "ray_scene.cpp"), os.path.join(ROOT, "tests", "ray_build_main.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    c = {k: int(v) for k, v in re.findall(r"^([a-z_]\w*) (-?\d+)$", p.stdout, flags=re.M)}
    assert c["failures"] == 0 and c["no_triangle_refused"] == 1
    assert c["one_triangle_nodes"] == 1 and c["one_triangle_leaves"] == 1 and c["one_triangle_depth"] == 1
    # coincident triangles: equal-count splits all the way, so the depth IS the balanced bound
    assert c["coincident_items"] == 1024 and c["coincident_depth"] == c["coincident_balanced_levels"] == 4
    assert c["meshlet255_items"] == 85
    assert c["random_mesh_items"] == 5000
    # the trees are within the stack's bound; surface-area splits may go deeper than the balanced tree, never beyond 12 levels
    for name in ("coincident", "meshlet255", "random_mesh", "exponential", "non_finite", "tlas1", "tlas2", "tlas9", "tlas600", "tlas600_same"):
        assert 1 <= c[name + "_depth"] <= 12, name
    assert c["exponential_depth"] > c["exponential_balanced_levels"]     # (surface-area splits peel these off one by one, until the bound acts)
    # the deep scene of tests/ray_deep_cases.py: both of its trees are exactly as deep as the bound allows (the node counts are what
    # tests/test_ray_walk_host.py's program builds from the scene itself)
    assert c["deep_blas_items"] == 128 and c["deep_blas_depth"] == 12 and c["deep_blas_nodes"] == 25
    assert c["deep_tlas_items"] == 120 and c["deep_tlas_depth"] == 12 and c["deep_tlas_nodes"] == 57
    assert c["tlas1_nodes"] == 1 and c["tlas1_leaves"] == 1
    assert c["tlas2_leaves"] == 2 and c["tlas9_leaves"] == 9 and c["tlas600_leaves"] == 600 and c["tlas600_same_leaves"] == 600
