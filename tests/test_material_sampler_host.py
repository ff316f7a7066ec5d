"""chord_amd/csrc/material_sampler.h -- the sampler the material resolve's kernels include, with the level rule taken from an explicit
lodq (sample_slot_lod) -- compiled by the host compiler with -fsanitize=address,undefined into a program of its own
(tests/material_sampler_main.cpp) and held word for word (uint32 views, no tolerance) to tests/spec_ray_shade_np.sample_lod: texel
store and every block format, all six minification filters, the three wrap modes, sRGB and linear decode, power-of-two, odd and
one-texel-wide chains, levels from below 0 to beyond the chain's last, coordinates at texel edges, far outside [0, 1] and not finite.
The header's functions are float32 / integer C++ in source order, built here with -ffp-contract=off as the kernels are, so the host
executes the kernels' statements.  CPU only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from chord_amd import records as R

import spec_material_np as SM
import spec_ray_shade_np as RS
import spec_texture_bc_np as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
FILTERS = (SM.NEAREST, SM.LINEAR, SM.NEAREST_MIPMAP_NEAREST, SM.LINEAR_MIPMAP_NEAREST, SM.NEAREST_MIPMAP_LINEAR, SM.LINEAR_MIPMAP_LINEAR)
WRAPS = (SM.REPEAT, SM.CLAMP_TO_EDGE, SM.MIRRORED_REPEAT)
SIZES = ((16, 8), (5, 3), (37, 21), (8, 64), (1, 1))                       # (width, height)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("material_sampler") / "material_sampler_check")
    cc = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"),
                         "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "chord_amd", "csrc"),
                         os.path.join(ROOT, "tests", "material_sampler_main.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, cc      # (a build that fails is every test's failure, asserted where the program is run)


def _samples(rng, width, height, mips, n=320):
    """(u, v, lodq): random coordinates over several periods, then texel edges and centres of level 0, huge and non-finite ones; lodq
    over the rule's edges: <= 0, the rounding point of *_MIPMAP_NEAREST, whole levels, the last level and beyond it."""
    u = (rng.random(n) * 7.0 - 3.0).astype(f32)
    v = (rng.random(n) * 7.0 - 3.0).astype(f32)
    k = np.arange(40)
    u[:40] = ((k % (width + 2)) - 1).astype(f32) / f32(width) + np.where(k % 3 == 0, f32(0.5) / f32(width), f32(0.0))
    v[:40] = ((k % (height + 2)) - 1).astype(f32) / f32(height)
    u[40:48] = np.array([np.nan, np.inf, -np.inf, 1.0e10, -1.0e10, 9.9e8, -9.9e8, 0.0], dtype=f32)
    v[44:52] = np.array([np.nan, np.inf, -np.inf, 1.0e10, -1.0e10, 9.9e8, -9.9e8, -0.0], dtype=f32)
    last = mips - 1
    edges = np.array([0, 1, -1, -700, 127, 128, 129, 255, 256, 257, 383, 384, 576, 256 * last - 1, 256 * last, 256 * last + 1, 256 * last + 200,
                      256 * (last + 3), 3840], dtype=np.int32)
    lodq = edges[rng.integers(0, len(edges), size=n)]
    lodq[::7] = rng.integers(0, 256 * (last + 2) + 1, size=len(lodq[::7]))
    return u, v, lodq.astype(np.int32)


def _run(program, tmp_path, format, width, height, mips, data, sampler, srgb, u, v, lodq):
    data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    data = np.concatenate([data, np.zeros((-len(data)) % (4 if format == 0 else 8), dtype=np.uint8)])
    head = np.array([format, width, height, mips, sampler[0], sampler[1], sampler[2], sampler[3], int(srgb), len(u)], dtype=np.uint32)
    rec = np.stack([u.view(np.uint32), v.view(np.uint32), lodq.view(np.uint32)], axis=1).reshape(-1)
    req, ans = os.path.join(str(tmp_path), "request.bin"), os.path.join(str(tmp_path), "answer.bin")
    np.concatenate([head, data.view(np.uint32), rec]).tofile(req)
    exe, cc = program
    assert cc.returncode == 0, "tests/material_sampler_main.cpp does not build against chord_amd/csrc/material_sampler.h:\n" + cc.stderr[-3000:]
    p = subprocess.run([exe, req, ans], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
    return np.fromfile(ans, dtype=f32).reshape(-1, 4)


def _compare(got, levels, sampler, srgb, u, v, lodq, what):
    table, _ = SM.tables()
    stats = {}
    want = RS.sample_lod(levels, sampler, u, v, lodq, table if srgb else None, stats)
    g, w = got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    if not np.array_equal(g, w):
        bad = np.flatnonzero((g != w).any(axis=1))
        k = int(bad[0])
        raise AssertionError("%s: %d of %d samples differ; first: u %r v %r lodq %d got %r want %r" % (what, len(bad), len(u), u[k], v[k], lodq[k], got[k], want[k]))
    return stats


def test_texel_store_equals_the_specification(program, tmp_path):
    rng = np.random.default_rng(11)
    levels_seen, blends, case = set(), 0, 0
    for width, height in SIZES:
        image = rng.integers(0, 256, size=(height, width, 4), dtype=np.uint8)
        chain, mips = R.mip_chain_rgba8(image)
        levels = SM.levels_of(chain, width, height, mips)
        for min_f in FILTERS:
            case += 1
            sampler = (min_f, FILTERS[case % 2], WRAPS[case % 3], WRAPS[(case // 3 + 1) % 3])
            srgb = case % 2 == 1
            u, v, lodq = _samples(rng, width, height, mips)
            got = _run(program, tmp_path, 0, width, height, mips, chain, sampler, srgb, u, v, lodq)
            stats = _compare(got, levels, sampler, srgb, u, v, lodq, "%d x %d, sampler %r, srgb %d" % (width, height, sampler, srgb))
            assert not np.isnan(got).any()
            levels_seen |= set(np.unique(stats["l0"]).tolist())
            blends += int((stats["l1"] != stats["l0"]).sum())
    assert case == 30 and levels_seen >= set(range(7)) and blends > 500           # (64 texels: seven levels; *_MIPMAP_LINEAR blends)


@pytest.mark.parametrize("format", [BC.BC1_RGB, BC.BC3, BC.BC4, BC.BC5])
def test_block_store_equals_the_specification_of_the_decoded_texels(program, tmp_path, format):
    rng = np.random.default_rng(100 + format)
    for k, (width, height) in enumerate(((16, 8), (37, 21), (5, 3), (4, 260))):
        mips = max(width, height).bit_length()
        data = rng.integers(0, 256, size=BC.chain_bytes(width, height, mips, format), dtype=np.uint8)      # any bytes are blocks: both modes of every kind
        levels = [np.ascontiguousarray(l).reshape(l.shape[0], l.shape[1], 4).view(np.uint32)[..., 0] for l in BC.decode_chain(data, width, height, mips, format)]
        for min_f in (SM.LINEAR_MIPMAP_LINEAR, SM.NEAREST_MIPMAP_NEAREST, SM.NEAREST):
            sampler = (min_f, FILTERS[(k + min_f) % 2], WRAPS[k % 3], WRAPS[(k + 1) % 3])
            srgb = (k + min_f) % 2 == 0
            u, v, lodq = _samples(rng, width, height, mips)
            got = _run(program, tmp_path, format, width, height, mips, data, sampler, srgb, u, v, lodq)
            _compare(got, levels, sampler, srgb, u, v, lodq, "format %d, %d x %d, sampler %r, srgb %d" % (format, width, height, sampler, srgb))


def test_the_resolve_kernels_take_the_sampler_from_the_header():
    """One definition: kernels_resolve.hip includes material_sampler.h and defines none of its functions itself, and its sample_slot
    forms the footprint's lodq and hands it to sample_slot_lod."""
    src = open(os.path.join(ROOT, "chord_amd", "csrc", "kernels_resolve.hip")).read()
    assert '#include "material_sampler.h"' in src
    for name in ("decode_texel(", "sample_level(", "sample_level_blocks(", "block_texel(", "sample_slot_lod("):
        assert "float4 " + name not in src and "uint32_t " + name not in src, name
    assert "return sample_slot_lod<kSrgb, kBlocks>(texels, S, u, v, lodq, srgb);" in src
