"""chordvis_build_ray_scene / chordvis_refit_ray_scene / chordvis_trace_rays on trees of full depth (tests/ray_deep_cases.py): a BLAS and
a TLAS of exactly CHORD_RAY_MAX_DEPTH = 12 levels each, and rays whose stacks reach 71 of the 73 words two such trees can ask for
(tests/test_ray_walk_host.py proves both on the CPU, from a host build of the kernel's own statements).  A push the stack refuses is
silent -- the ray just returns a farther hit or a miss -- so every word of every hit is held to the brute-force specification
(tests/spec_rays_np.py), closest and any-hit, after a build, after refits over all twelve levels, and after a reversed object list."""
import numpy as np
import pytest

import ray_deep_cases as D
import spec_rays_np as S
from chord_amd import lib as L, records as R
from test_gpu_rays import _hits, _renderer, _same

pytestmark = pytest.mark.gpu
F = np.float32


def _any(want):
    out = np.zeros(len(want), dtype=R.RAY_HIT)
    out["status"] = want["status"] & 1
    return out


def _root_is(info, objects, primitives):
    lo, hi = S.object_boxes(objects, primitives)
    assert np.array_equal(np.array(info.rootMin, dtype=F), lo.min(axis=0)) and np.array_equal(np.array(info.rootMax, dtype=F), hi.max(axis=0))


@pytest.mark.parametrize("name", sorted(D.SCENES))
def test_hits_equal_the_specification_at_full_depth(gpu, name):
    scene, tris, rays, want, want_any = D.case(name)
    if name == "deep":
        assert D.conditions(want) == []
    r = _renderer(scene)
    try:
        info = r.build_ray_scene()
        assert info.blasTriangles == sum(len(t[0]) for t in tris)
        if name != "deep_tlas_only":
            assert info.blasMaxDepth == D.MAX_DEPTH == L.RAY_MAX_DEPTH
        if name != "deep_blas_only":
            assert info.tlasDepth == D.MAX_DEPTH == L.RAY_MAX_DEPTH
        _root_is(info, scene.objects, scene.primitives)
        _same(_hits(r, rays), want, rays, name + ", closest")
        _same(_hits(r, rays, any_hit=True), want_any, rays, name + ", any-hit")
    finally:
        r.close()


def test_refit_over_twelve_levels_and_back(gpu):
    """Every third instance moved twice as far (still exact), refit; then moved back, refit again: the second refit works only if the
    first left every arrival counter of all twelve levels at zero."""
    scene, tris, rays, want, want_any = D.case("deep")
    moved = scene.with_objects(scene.objects.copy())
    moved.local_to_world = scene.local_to_world.copy()
    moved.local_to_world[::3, 12] *= 2.0
    L.fill_objects(moved, D.CAMERA)
    want_moved = S.trace(moved, moved.objects, rays, triangles=tris, meshlet_cull=True)
    assert want_moved.tobytes() != want.tobytes()
    r = _renderer(scene)
    try:
        assert r.build_ray_scene().tlasDepth == D.MAX_DEPTH
        r.update_objects(moved.objects)
        r.refit_ray_scene()
        _root_is(r.ray_scene_info(), moved.objects, scene.primitives)
        _same(_hits(r, rays), want_moved, rays, "moved, closest")
        _same(_hits(r, rays, any_hit=True), _any(want_moved), rays, "moved, any-hit")
        r.update_objects(scene.objects)
        r.refit_ray_scene()
        _root_is(r.ray_scene_info(), scene.objects, scene.primitives)
        _same(_hits(r, rays), want, rays, "moved back, closest")
        _same(_hits(r, rays, any_hit=True), want_any, rays, "moved back, any-hit")
    finally:
        r.close()


def test_reversed_object_list(gpu):
    """The same instances in reverse order: the TLAS is as deep again, and the hits name the new object indices."""
    scene, tris, rays, want, _ = D.case("deep")
    rev = scene.with_objects(scene.objects[::-1].copy())
    rev.local_to_world = np.ascontiguousarray(scene.local_to_world[::-1])
    L.fill_objects(rev, D.CAMERA)
    want_rev = S.trace(rev, rev.objects, rays, triangles=tris, meshlet_cull=True)
    hit = (want["status"] & 1) != 0
    assert np.array_equal((want_rev["status"] & 1) != 0, hit) and np.array_equal(want_rev["object"][hit], len(scene.objects) - 1 - want["object"][hit])
    r = _renderer(scene)
    try:
        r.build_ray_scene()
        r.set_object_list(rev)
        info = r.build_ray_scene()
        assert info.blasBuilt == 0 and info.blasMaxDepth == D.MAX_DEPTH and info.tlasDepth == D.MAX_DEPTH
        _same(_hits(r, rays), want_rev, rays, "reversed list, closest")
        _same(_hits(r, rays, any_hit=True), _any(want_rev), rays, "reversed list, any-hit")
    finally:
        r.close()


def test_full_stacks_by_the_wave(gpu):
    """1, 64 and 65 copies of the stack-filling ray alone: a lone lane, a whole wave of maximal stacks in scratch, and one more."""
    scene, tris, rays, want, want_any = D.case("deep")
    r = _renderer(scene)
    try:
        r.build_ray_scene()
        for n in (1, 64, 65):
            idx = np.full(n, D.FILL)
            _same(_hits(r, rays[idx]), want[idx], rays[idx], "%d stack-filling rays" % n)
            _same(_hits(r, rays[idx], any_hit=True), want_any[idx], rays[idx], "%d stack-filling rays, any-hit" % n)
    finally:
        r.close()
