"""chord_amd/csrc/pixel_rays.h -- the per-pixel statements of chordvis_pixel_rays, which kernels_pixelrays.hip runs a pixel per lane
-- compiled by the host compiler with -fsanitize=address,undefined into a program of its own (tests/pixel_rays_main.cpp with chord_amd/
csrc/ray_scene.cpp: its own main, no Python in the process) and held word for word (uint32 views, no tolerance, no pixel left out) to
tests/spec_pixel_rays_np.pixel_rays on every case of tests/pixel_rays_cases.py.  The program runs pixel_of_lane -> make_pixel_ray ->
walk_ray -> finish_pixel_ray with every image, table, output and the traversal stack in a heap allocation of exactly its size, so an
index that touches one element past an array ends the program with a sanitizer report; it also proves that the lanes of the waves
visit every pixel exactly once.  Built with -ffp-contract=off as the kernels are, once for each pixel-to-lane mapping.  CPU only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from chord_amd import records as R

import pixel_rays_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32


@pytest.fixture(scope="module", params=[0, 1], ids=["blocks_8x8", "rows_64x1"])
def program(request, tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("pixel_rays") / "pixel_rays_check")
    csrc = os.path.join(ROOT, "chord_amd", "csrc")
    cc = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-D__HIP_PLATFORM_AMD__", "-DCHORD_PIXEL_RAYS_ROWS=%d" % request.param,
                         "-I", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"),
                         "-I", os.path.join(ROOT, "include"), "-I", csrc,
                         os.path.join(ROOT, "tests", "pixel_rays_main.cpp"), os.path.join(csrc, "ray_scene.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, cc      # (a build that fails is every test's failure, asserted where the program is run)


def _run(program, tmp_path, scene, tris, cases):
    """[(out (h, w) float32, hits records.RAY_HIT (h * w,))] of the program for the cases of one scene"""
    objects = np.ascontiguousarray(scene.objects, dtype=R.OBJECT)
    parts = [np.array([len(objects), len(scene.primitives), len(cases), 0, 0, 0, 0, 0], dtype=u32), objects.view(u32).reshape(-1)]
    for p, (verts, mids, tids) in zip(scene.primitives, tris):
        parts += [p["posMin"].astype(f32).view(u32), p["posMax"].astype(f32).view(u32), np.array([len(verts)], dtype=u32)]
        rec = np.concatenate([np.ascontiguousarray(verts, dtype=f32).reshape(-1, 9).view(u32), mids.astype(u32)[:, None], tids.astype(u32)[:, None]], axis=1)
        parts.append(rec.reshape(-1))
    for c in cases:
        desc = np.frombuffer(bytes(c.ctypes_desc()), dtype=u32)
        assert len(desc) == 16
        parts += [desc, np.array([c.z is not None, c.hits], dtype=u32), np.ascontiguousarray(c.position, dtype=f32).view(u32).reshape(-1),
                  np.ascontiguousarray(c.normal, dtype=f32).view(u32).reshape(-1)]
        if c.z is not None:
            parts.append(c.device_z().view(u32))
        if c.table is not None:
            parts.append(np.ascontiguousarray(c.table, dtype=f32).view(u32).reshape(-1))
    req, ans = os.path.join(str(tmp_path), "request.bin"), os.path.join(str(tmp_path), "answer.bin")
    np.concatenate([np.ascontiguousarray(p, dtype=u32).reshape(-1) for p in parts]).tofile(req)
    exe, cc = program
    assert cc.returncode == 0, "tests/pixel_rays_main.cpp does not build against chord_amd/csrc/pixel_rays.h:\n" + cc.stderr[-3000:]
    p = subprocess.run([exe, req, ans], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
    words = np.fromfile(ans, dtype=u32)
    out, at = [], 0
    for c in cases:
        n = c.desc.width * c.desc.height
        o = words[at:at + n].view(f32).reshape(c.desc.height, c.desc.width)
        h = np.ascontiguousarray(words[at + n:at + 9 * n]).view(R.RAY_HIT).reshape(-1)
        assert words[at + 9 * n] == n, (c.name, "pixels visited", int(words[at + 9 * n]), n)
        out.append((o, h))
        at += 9 * n + 1
    assert at == len(words)
    return out


@pytest.mark.parametrize("name", sorted(PC.SCENES))
def test_statements_equal_the_specification(program, tmp_path, name):
    scene, cam, tris = PC.scene(name)
    cases = [c for c in PC.cases() if c.scene == name]
    assert len(cases) == len(PC.MODES) * len(PC.DEPTHS)
    for c, (out, hits) in zip(cases, _run(program, tmp_path, scene, tris, cases)):
        want_out, want_hits, _ = PC.expected(c)
        assert np.array_equal(out.view(u32), want_out.view(u32)), (c.name, np.argwhere(out.view(u32) != want_out.view(u32))[:5])
        if c.hits:
            assert hits.tobytes() == want_hits.tobytes(), (c.name, np.flatnonzero((hits.view(u32).reshape(-1, 8) != want_hits.view(u32).reshape(-1, 8)).any(axis=1))[:5])
        else:
            assert not hits.view(u32).any(), (c.name, "hit records nobody asked for")
