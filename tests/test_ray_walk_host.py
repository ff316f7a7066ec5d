"""chord_amd/csrc/ray_walk.h -- the whole per-ray function of chordvis_trace_rays, the statements kernels_rays.hip runs a ray per lane,
and the box arithmetic of chordvis_refit_ray_scene -- compiled by the host compiler with -fsanitize=address,undefined into a program of
its own (tests/ray_walk_main.cpp with chord_amd/csrc/ray_scene.cpp: its own main, no Python in the process) and held word for word
(uint32 views, no tolerance, no ray left out) to tests/spec_rays_np.trace.  The program builds the trees as the library does and keeps
every array -- the traversal stack too -- in a heap allocation of exactly its size, so an index that passes its check and still
touches one element past an array ends the program with a sanitizer report.  Built with -ffp-contract=off as the kernels are.

The deep scenes of tests/ray_deep_cases.py are proved here to be what they claim: both trees exactly ray::kMaxDepth = 12 levels, no
push refused on any ray, and a stack high-water mark of at least 71 of the 73 words two 12-level trees can ask for.  CPU only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from chord_amd import lib as L, records as R

import ray_deep_cases as D
import spec_rays_np as S
import test_gpu_rays as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("ray_walk") / "ray_walk_check")
    csrc = os.path.join(ROOT, "chord_amd", "csrc")
    cc = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"),
                         "-I", os.path.join(ROOT, "include"), "-I", csrc,
                         os.path.join(ROOT, "tests", "ray_walk_main.cpp"), os.path.join(csrc, "ray_scene.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, cc      # (a build that fails is every test's failure, asserted where the program is run)


def _run(program, tmp_path, scene, objects, tris, rays, any_hit=False):
    """(hits as records.RAY_HIT, stack high-water mark per ray, refused pushes per ray, info dictionary) of the program."""
    objects = np.ascontiguousarray(objects, dtype=R.OBJECT)
    rays = np.ascontiguousarray(rays, dtype=R.RAY).reshape(-1)
    parts = [np.array([len(objects), len(scene.primitives), len(rays), int(any_hit), 0, 0, 0, 0], dtype=u32), objects.view(u32).reshape(-1)]
    for p, (verts, mids, tids) in zip(scene.primitives, tris):
        parts += [p["posMin"].astype(f32).view(u32), p["posMax"].astype(f32).view(u32), np.array([len(verts)], dtype=u32)]
        rec = np.concatenate([np.ascontiguousarray(verts, dtype=f32).reshape(-1, 9).view(u32), mids.astype(u32)[:, None], tids.astype(u32)[:, None]], axis=1)
        parts.append(rec.reshape(-1))
    parts.append(rays.view(u32).reshape(-1))
    req, ans = os.path.join(str(tmp_path), "request.bin"), os.path.join(str(tmp_path), "answer.bin")
    np.concatenate([np.ascontiguousarray(p, dtype=u32).reshape(-1) for p in parts]).tofile(req)
    exe, cc = program
    assert cc.returncode == 0, "tests/ray_walk_main.cpp does not build against chord_amd/csrc/ray_walk.h:\n" + cc.stderr[-3000:]
    p = subprocess.run([exe, req, ans], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
    out = np.fromfile(ans, dtype=u32)
    head, body = out[:8], out[8:].reshape(-1, 10)
    assert len(body) == len(rays)
    info = dict(blasMaxDepth=int(head[0]), tlasDepth=int(head[1]), blasNodes=int(head[2]), tlasNodes=int(head[3]), blasTriangles=int(head[4]))
    return np.ascontiguousarray(body[:, :8]).view(R.RAY_HIT).reshape(-1), body[:, 8].copy(), body[:, 9].copy(), info


def _both_modes(program, tmp_path, scene, objects, tris, rays, want, want_any, what):
    got, high, refused, info = _run(program, tmp_path, scene, objects, tris, rays)
    assert not refused.any(), (what, "the stack refused a push", np.flatnonzero(refused)[:10])
    G._same(got, want, rays, what + ", closest")
    got_any, _, refused_any, _ = _run(program, tmp_path, scene, objects, tris, rays, any_hit=True)
    assert not refused_any.any(), (what, "the stack refused a push (any-hit)")
    G._same(got_any, want_any, rays, what + ", any-hit")
    return high, info


@pytest.mark.parametrize("name", sorted(G.SCENES))
def test_walk_equals_the_specification(program, tmp_path, name):
    scene, cam, view, iv, tris, rays, want, want_any = G._case(name)
    high, info = _both_modes(program, tmp_path, scene, scene.objects, tris, rays, want, want_any, name)
    assert info["blasTriangles"] == sum(len(t[0]) for t in tris)
    assert 1 <= info["blasMaxDepth"] <= L.RAY_MAX_DEPTH and 1 <= info["tlasDepth"] <= L.RAY_MAX_DEPTH
    assert high.max() <= D.STACK_ENTRIES and (high[S.live_rays(rays)] >= 1).all() and not high[~S.live_rays(rays)].any()


def test_ties_go_to_the_lowest_ids(program, tmp_path):
    scene, cam = G.tie_scene()
    L.fill_objects(scene, cam)
    tris = S.lod0_triangles(scene)
    o = [(0.7, 0.3, 3.0), (0.6, 0.2, -2.0), (2.2, 0.3, 3.0), (2.5, 0.25, 1.0), (2.1, 0.1, -1.0), (2.3, 0.6, 2.0)]
    d = [(0, 0, -1), (0, 0, 1), (0, 0, -1), (0, 0, -1), (0, 0, 1), (0.01, 0.0, -1.0)]
    rays = S.make_rays(np.array(o, dtype=f32) - np.array(cam.position, dtype=f32), np.array(d, dtype=f32), 0.0, 1e9)
    want = S.trace(scene, scene.objects, rays, triangles=tris)
    assert (want["status"] != 0).all() and (want["triangle"] == 0).all()
    want_any = np.zeros(len(rays), dtype=R.RAY_HIT)
    want_any["status"] = 1
    _, info = _both_modes(program, tmp_path, scene, scene.objects, tris, rays, want, want_any, "ties")
    assert info["blasTriangles"] == 3 + 1024


@pytest.mark.parametrize("name", sorted(D.SCENES))
def test_deep_scenes(program, tmp_path, name):
    scene, tris, rays, want, want_any = D.case(name)
    if name == "deep":
        assert D.conditions(want) == []
    high, info = _both_modes(program, tmp_path, scene, scene.objects, tris, rays, want, want_any, name)
    print(name, info, "stack high-water: largest %d, ray FILL %d, ray WALK %d" % (high.max(), high[D.FILL], high[D.WALK]))
    if name != "deep_tlas_only":
        assert info["blasMaxDepth"] == D.MAX_DEPTH
    if name != "deep_blas_only":
        assert info["tlasDepth"] == D.MAX_DEPTH
    if name == "deep":
        assert D.STACK_REACHED <= high.max() <= D.STACK_BOUND
        assert high[D.FILL] >= D.STACK_REACHED and (want["status"][D.FILL] & 1) == 1 and want["object"][D.FILL] == 0 and want["triangle"][D.FILL] == 0
        assert want["status"][D.WALK] == 0
    if name == "deep_tlas_only":         # the object without a BLAS is in the way of rays that hit what lies behind it
        empty = np.flatnonzero(scene.objects["GLTFPrimitiveDetail"] == 1)
        assert len(empty) == 1 and len(tris[1][0]) == 0
        lo, hi = S.object_boxes(scene.objects[empty], scene.primitives)
        n, f = S.slab(rays["origin"], rays["direction"], lo[0], hi[0])
        through = ~(n > f) & ((want["status"] & 1) != 0) & (want["t"] > n)
        assert through.sum() >= 10
