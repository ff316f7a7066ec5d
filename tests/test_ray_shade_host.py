"""chord_amd/csrc/ray_shade.h -- the whole per-hit function of chordvis_shade_ray_hits, the statements kernels_rayshade.hip runs a hit
per lane -- compiled by the host compiler with -fsanitize=address,undefined into a program of its own (tests/ray_shade_main.cpp: its
own main, no Python in the process) and held word for word (uint32 views, no tolerance) to tests/spec_ray_shade_np.shade.  The program
keeps every array in a heap allocation of exactly its size, so an index that passes its check and still reads one element past an
array ends the program with a sanitizer report.  Built with -ffp-contract=off as the kernels are.  CPU only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from chord_amd import records as R

import ray_shade_cases as RC
import spec_rays_np as S
import spec_ray_shade_np as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32
BIG = 0xFFFFFFFF


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("ray_shade") / "ray_shade_check")
    cc = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"),
                         "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "chord_amd", "csrc"),
                         os.path.join(ROOT, "tests", "ray_shade_main.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, cc      # (a build that fails is every test's failure, asserted where the program is run)


def _run(program, tmp_path, scene, objects, hits, lod=0.0, lods=None, texcoords="scene", normals="scene", asset_meshlet_base=None,
         asset_meshlet_count=None):
    """The program's records for `hits` against `objects` over `scene` (texcoords / normals None: a scene uploaded without).
    asset_meshlet_base / asset_meshlet_count: per primitive, its asset's first meshlet and meshlet count (None: one asset)."""
    mbase = np.zeros(len(scene.primitives), dtype=u32) if asset_meshlet_base is None else np.asarray(asset_meshlet_base, dtype=u32)
    mcount = np.full(len(scene.primitives), len(scene.meshlets), dtype=u32) if asset_meshlet_count is None else np.asarray(asset_meshlet_count, dtype=u32)
    hits = np.ascontiguousarray(hits, dtype=R.RAY_HIT).reshape(-1)
    objects = np.ascontiguousarray(objects, dtype=R.OBJECT)
    uv = scene.texcoord0 if isinstance(texcoords, str) else texcoords
    nrm = scene.normals if isinstance(normals, str) else normals
    head = np.zeros(16, dtype=u32)
    head[:12] = [len(objects), len(scene.meshlets), len(scene.primitives), len(scene.materials), len(scene.samplers), len(scene.texture_images),
                 len(scene.meshlet_data), len(scene.positions), uv is not None, nrm is not None, len(hits), lods is not None]
    head[12] = np.array([lod], dtype=f32).view(u32)[0]
    m = np.stack([scene.meshlets["dataOffset"], scene.meshlets["vertexTriangleCount"]], axis=1).astype(u32)
    parts = [head, objects.view(u32).reshape(-1), scene.primitives["vertexOffset"].astype(u32),
             np.stack([mbase, mcount], axis=1).reshape(-1), m.reshape(-1), scene.meshlet_data]
    if uv is not None:
        parts.append(np.ascontiguousarray(uv, dtype=f32).view(u32).reshape(-1))
    if nrm is not None:
        parts.append(np.ascontiguousarray(nrm, dtype=f32).view(u32).reshape(-1))
    parts += [scene.materials.view(u32).reshape(-1), scene.samplers.view(u32).reshape(-1)]
    for t, (chain, mips) in zip(scene.texture_images, scene._tex_chains):
        assert not isinstance(t, R.TextureChain), "RGBA8 images only: the block formats are held by tests/test_material_sampler_host.py"
        parts += [np.array([t.shape[1], t.shape[0], mips], dtype=u32), np.ascontiguousarray(chain, dtype=np.uint8).reshape(-1).view(u32)]
    parts.append(hits.view(u32).reshape(-1))
    if lods is not None:
        parts.append(np.ascontiguousarray(lods, dtype=f32).view(u32).reshape(-1))
    req, ans = os.path.join(str(tmp_path), "request.bin"), os.path.join(str(tmp_path), "answer.bin")
    np.concatenate([np.ascontiguousarray(p, dtype=u32).reshape(-1) for p in parts]).tofile(req)
    exe, cc = program
    assert cc.returncode == 0, "tests/ray_shade_main.cpp does not build against chord_amd/csrc/ray_shade.h:\n" + cc.stderr[-3000:]
    p = subprocess.run([exe, req, ans], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
    return np.fromfile(ans, dtype=u32).reshape(-1, 16)


def _same(got, want, hits, what):
    w = np.ascontiguousarray(want).view(u32).reshape(-1, 16)
    assert got.shape == w.shape, (what, got.shape, w.shape)
    if not np.array_equal(got, w):
        bad = np.flatnonzero((got != w).any(axis=1))
        k = int(bad[0])
        raise AssertionError("%s: %d of %d hits differ from the specification; first: hit %d %r\n got  %r\n want %r"
                             % (what, len(bad), len(w), k, hits[k], got[k].view(RS.RAY_HIT_SURFACE), want[k]))


def _grid_hits(n_objects):
    """A grid of barycentrics -- corners, edges, interior and beyond the triangle -- on every object and both faces."""
    vals = (0.0, 0.125, 1.0 / 3.0, 0.5, 0.875, 1.0, -0.25, 1.5)
    return np.concatenate([RC.hit(o, u, v, status=st, t=1.0 + 0.5 * o) for o in range(n_objects) for st in (1, 3) for u in vals for v in vals])


def test_triangle_scene_every_object_both_faces(program, tmp_path):
    scene, cam = RC.triangle_scene()
    hits = _grid_hits(len(scene.objects))
    for label, lod, lods in RC.lod_runs(hits):
        want = RS.shade(scene, scene.objects, hits, lod=lod, lods=lods)
        assert (want["flags"] & RS.RAYSURF_VALID).all()
        _same(_run(program, tmp_path, scene, scene.objects, hits, lod, lods), want, hits, "triangle scene, " + label)
    fl = want["flags"]
    for bits in (1 | 8, 1 | 2 | 8, 1 | 4 | 8, 1 | 2 | 4 | 8, 1, 1 | 2):                 # one- and two-sided, both faces, and the other materialType
        assert (fl == bits).any(), bits


def _past_the_end(scene):
    """[(what, hit)]: the object, meshlet, triangle and material words each one past their array and at 0xFFFFFFFF (the material word
    lives in the object record: test_invalid_records_give_zero_words rewrites it there)."""
    T = int(scene.meshlets["vertexTriangleCount"][0] >> 8) & 0xFF
    out = []
    for v in (len(scene.objects), BIG):
        out.append(("object %#x" % v, RC.hit(v, 0.25, 0.25)))
    for v in (len(scene.meshlets), BIG):
        out.append(("meshlet %#x" % v, RC.hit(0, 0.25, 0.25, meshlet=v)))
    for v in (T, BIG):
        out.append(("triangle %#x" % v, RC.hit(0, 0.25, 0.25, triangle=v)))
    return out


def test_invalid_records_give_zero_words(program, tmp_path):
    scene, cam = RC.triangle_scene()
    cases = RC.invalid_hits(scene) + _past_the_end(scene)
    good = RC.hit(1, 0.3, 0.3, status=3)
    hits = np.concatenate([h for _, h in cases] + [good])
    want = RS.shade(scene, scene.objects, hits, lod=1.5)
    assert not want[:-1].view(u32).any() and want[-1]["flags"] == 1 | 2 | 4 | 8
    _same(_run(program, tmp_path, scene, scene.objects, hits, 1.5), want, hits, "invalid records")
    # the object's own ids: a primitive or a material one past its array, and 0xFFFFFFFF
    for field, count in (("GLTFPrimitiveDetail", len(scene.primitives)), ("GLTFMaterialData", len(scene.materials))):
        for v in (count, BIG):
            objects = scene.objects.copy()
            objects[field][2] = v
            hits = np.concatenate([RC.hit(o, 0.2, 0.5) for o in range(len(objects))])
            want = RS.shade(scene, objects, hits, lod=0.5)
            assert not want[2:3].view(u32).any() and (want["flags"][[0, 1, 3]] & 1).all()
            _same(_run(program, tmp_path, scene, objects, hits, 0.5), want, hits, "%s %#x" % (field, v))
    # data words and vertex ids that leave their arrays: a meshlet whose data lies at the very end of the stream, and one past it
    for shift, what in ((0, "vertex ids past the positions"), (1, "the triangle word past the data")):
        meshlets = scene.meshlets.copy()
        data = scene.meshlet_data.copy()
        if shift:
            meshlets["dataOffset"][0] += 1                  # the triangle word is now one past the stream
        else:
            data[:3] = [len(scene.positions), BIG, 2]       # vertex ids one past the positions and at 0xFFFFFFFF
        bent = R.Scene(scene.objects, scene.primitives, scene.materials, meshlets, scene.groups, scene.group_indices, data, scene.positions,
                       texcoord0=scene.texcoord0, textures=scene.texture_images, samplers=scene.samplers, normals=scene.normals, tangents=scene.tangents)
        hits = np.concatenate([RC.hit(o, 0.2, 0.5) for o in range(len(scene.objects))])
        want = RS.shade(bent, bent.objects, hits, lod=0.0)
        assert not want.view(u32).any(), what
        _same(_run(program, tmp_path, bent, bent.objects, hits), want, hits, what)


def test_material_scene_traced_hits_every_level_run(program, tmp_path):
    scene, cam, view, iv, rays = RC.case("material")
    hits = S.trace(scene, scene.objects, rays, meshlet_cull=True)
    runs = RC.shade_runs(scene, scene.objects, hits)
    assert RC.vacuity(scene, "material", hits, [(want, stats) for _, _, _, want, stats in runs]) == []
    lods = runs[-1][2]
    assert np.isnan(lods).any() and np.isposinf(lods).any() and np.isneginf(lods).any() and (lods[np.isfinite(lods)] < 0).any()
    for label, lod, lods, want, _ in runs:
        _same(_run(program, tmp_path, scene, scene.objects, hits, lod, lods), want, hits, "material scene, " + label)


def test_meshlets_of_another_primitive_take_the_objects_vertex_offset(program, tmp_path):
    """A host's own hits may pair an object with a meshlet of another primitive: the vertex ids are then offset by the vertexOffset of
    the OBJECT's primitive, as the specification's validate says, and a vertex id that leaves the positions makes the hit invalid."""
    scene, cam, view, iv, rays = RC.case("material")
    assert len(np.unique(scene.primitives["vertexOffset"])) > 2
    hits = S.trace(scene, scene.objects, rays, meshlet_cull=True)
    hits = hits[(hits["status"] & 1) != 0].copy()
    own = RS.shade(scene, scene.objects, hits, lod=1.0)
    prim = scene.objects["GLTFPrimitiveDetail"]
    for step in (1, 3):
        other = hits.copy()
        other["object"] = (hits["object"] + step) % len(scene.objects)
        foreign = scene.primitives["vertexOffset"][prim[other["object"]]] != scene.primitives["vertexOffset"][prim[hits["object"]]]
        want = RS.shade(scene, scene.objects, other, lod=1.0)
        valid = (want["flags"] & 1) != 0
        assert (foreign & valid).sum() > 100 and (foreign & ~valid).sum() > 10, (foreign.sum(), valid.sum())
        assert (want["uv"][foreign & valid] != own["uv"][foreign & valid]).any(axis=1).mean() > 0.9      # other vertices were read
        _same(_run(program, tmp_path, scene, scene.objects, other, 1.0), want, other, "objects %+d: meshlets of another primitive" % step)


def test_scene_without_normals_or_texcoords(program, tmp_path):
    scene, cam = RC.triangle_scene()
    hits = _grid_hits(len(scene.objects))
    lods = RC.per_hit_lods(hits)
    want = RS.shade(scene, scene.objects, hits, lods=lods, normals=None)
    assert not (want["normal"].view(u32) & 0x7FFFFFFF).any() and want["uv"].any()
    _same(_run(program, tmp_path, scene, scene.objects, hits, 0.0, lods, normals=None), want, hits, "no normals")
    bare = R.Scene(scene.objects, scene.primitives, scene.materials, scene.meshlets, scene.groups, scene.group_indices, scene.meshlet_data, scene.positions,
                   texcoord0=None, textures=scene.texture_images, samplers=scene.samplers, normals=scene.normals, tangents=scene.tangents)
    want = RS.shade(bare, bare.objects, hits, lods=lods)
    assert not want["uv"].view(u32).any() and want["normal"].any() and want["baseColor"].any()
    _same(_run(program, tmp_path, bare, bare.objects, hits, 0.0, lods), want, hits, "no texture coordinates")


def test_several_assets_the_hits_meshlet_is_asset_relative(program, tmp_path):
    """tests/multi_asset.py's three assets as one table (per primitive the first meshlet and the meshlet count of its asset): the traced
    hits, whose meshlet is asset-relative, and the edges of that numbering -- the last meshlet of an asset, its count (invalid, though a
    valid index of the concatenated array), a meshlet of another primitive of the same asset."""
    import multi_asset as MA
    ms, cam = MA.three_assets()
    MA.filled(ms, cam)
    rays, _ = MA.ray_set(ms)
    hits = S.trace(ms.spec, ms.objects, rays, meshlet_cull=True, asset_meshlet_base=ms.asset_meshlet_base)
    edges = ms.edge_hits()
    hits = np.concatenate([hits] + [h for _, h, _ in edges])
    kw = dict(asset_meshlet_base=ms.asset_meshlet_base, asset_meshlet_count=ms.asset_meshlet_count)
    lods = RC.per_hit_lods(hits)
    want = RS.shade(ms.spec, ms.objects, hits, lods=lods, **kw)
    valid = (want["flags"] & RS.RAYSURF_VALID) != 0
    on = ms.asset_of_object[np.where(valid, hits["object"], 0)]
    assert all((valid & (on == a)).sum() >= 50 for a in range(3))
    assert [bool(v) for v in valid[-len(edges):]] == [v for _, _, v in edges]
    assert (want.view(u32).reshape(-1, 16) != RS.shade(ms.spec, ms.objects, hits, lods=lods).view(u32).reshape(-1, 16)).any(axis=1).sum() >= 50
    _same(_run(program, tmp_path, ms.spec, ms.objects, hits, 0.0, lods, **kw), want, hits, "three assets")
