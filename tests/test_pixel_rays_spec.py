"""The specification of chordvis_pixel_rays (tests/spec_pixel_rays_np.py) held to a scalar, loop-written evaluation of the same
statements on every case of tests/pixel_rays_cases.py, and the conditions those cases must meet for the comparisons on the device and
on the host (tests/test_gpu_pixel_rays.py, tests/test_pixel_rays_host.py) to mean something.  CPU only."""
import collections
import warnings

import numpy as np
import pytest

from chord_amd import records as R

import pixel_rays_cases as PC
import spec_pixel_rays_np as PR

F = np.float32
u32 = np.uint32
CASES = PC.cases()


def _scalar_pixel(desc, p, nrm, z, dT):
    """One pixel, one statement after the other on numpy float32 scalars: (disposition, eight ray words, createTBN's branch)"""
    zero8 = [F(0.0)] * 8
    valid = (z > F(0.0)) if z is not None else (p[3] != F(0.0))
    if not valid:
        return PR.FIXED_ONE, zero8, False
    x, y, zc = F(nrm[0]), F(nrm[1]), F(nrm[2])
    l2 = F(F(x * x + y * y) + zc * zc)
    if l2 > F(0.0):
        s = F(np.sqrt(l2))
        n = [F(x / s), F(y / s), F(zc / s)]
    else:
        n = [F(0.0), F(0.0), F(0.0)]
    z_branch = False
    if desc.mode == PR.HEMISPHERE:
        if abs(n[2]) > F(0.0):
            z_branch = True
            k = F(np.sqrt(F(n[1] * n[1] + n[2] * n[2])))
            u = [F(0.0), F(-n[2] / k), F(n[1] / k)]
        else:
            k = F(np.sqrt(F(n[0] * n[0] + n[1] * n[1])))
            u = [F(n[1] / k), F(-n[0] / k), F(0.0)]
        b = [F(F(n[1] * u[2]) - F(n[2] * u[1])), F(F(n[2] * u[0]) - F(n[0] * u[2])), F(F(n[0] * u[1]) - F(n[1] * u[0]))]
        d = [F(F(F(dT[0] * u[k]) + F(dT[1] * b[k])) + F(dT[2] * n[k])) for k in range(3)]
    else:
        d = [F(v) for v in desc.direction]
        if desc.flags & PR.FRONT_ONLY:
            facing = F(F(F(n[0] * d[0]) + F(n[1] * d[1])) + F(n[2] * d[2]))
            if not facing > F(0.0):
                return PR.FIXED_ZERO, zero8, False
    t_min = desc.tMin
    if desc.flags & PR.START_FROM_DEPTH:
        lin = F(desc.zNear / z)
        s = F(lin * F(0.01))
        w = F(s / F(s + F(1.0)))
        t_min = F(F(5e-3) + F(w * F(F(1e-1) - F(5e-3))))
    return PR.TRACE, [F(p[0]), F(p[1]), F(p[2]), t_min, d[0], d[1], d[2], desc.rayLength], z_branch


def _scalar_out(desc, disposition, hit):
    if disposition == PR.FIXED_ZERO:
        return F(0.0)
    if disposition == PR.FIXED_ONE or not (int(hit["status"]) & 1):
        return F(1.0)
    if desc.flags & PR.ANY_HIT:
        return F(0.0)
    q = F(hit["t"] / desc.rayLength)
    q = q if q > F(0.0) else F(0.0)
    return q if q < F(1.0) else F(1.0)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_vectorised_equals_scalar(case):
    out, hits, info = PC.expected(case)
    d = case.desc
    rays = info["rays"].view(u32).reshape(-1, 8)
    sc, cam, tris = PC.scene(case.scene)
    traced = info["disposition"] == PR.TRACE
    all_hits = hits
    if all_hits is None:                                                    # ANY_HIT: the status words, from out
        all_hits = np.zeros(d.width * d.height, dtype=R.RAY_HIT)
        all_hits["status"] = (traced & (out.reshape(-1) == 0)).astype(u32)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for i in range(d.width * d.height):
            y, x = divmod(i, d.width)
            dT = case.table[y & (d.tableH - 1), x & (d.tableW - 1)] if d.mode == PR.HEMISPHERE else None
            disp, words, zb = _scalar_pixel(d, case.position[y, x], case.normal[y, x], None if case.z is None else case.z[y, x], dT)
            assert disp == info["disposition"][i], (case.name, x, y, disp, info["disposition"][i])
            assert np.array_equal(np.array(words, dtype=F).view(u32), rays[i]), (case.name, x, y, words, info["rays"][i])
            if disp == PR.TRACE and d.mode == PR.HEMISPHERE:
                assert zb == bool(info["z_branch"][i])
            want = _scalar_out(d, disp, all_hits[i])
            assert np.array(want, dtype=F).view(u32) == out[y, x].view(u32), (case.name, x, y, want, out[y, x])
            if disp != PR.TRACE and hits is not None:
                assert not hits[i:i + 1].view(u32).any(), "a pixel that is not traced has a zero hit record"
    if d.flags & PR.ANY_HIT:
        assert hits is None and set(np.unique(out)) <= {F(0.0), F(1.0)}


def _stats():
    agg = collections.defaultdict(lambda: dict(valid=0, hit=0, miss=0))
    seen = dict(z_branch=False, x_branch=False, fixed_one=False, fixed_zero=False, beyond=False)
    between = {}
    for c in CASES:
        out, hits, info = PC.expected(c)
        disp, o = info["disposition"], out.reshape(-1)
        traced = disp == PR.TRACE
        hit = traced & (o == 0) if c.desc.flags & PR.ANY_HIT else (hits["status"] & 1) != 0
        a = agg[(c.scene, c.mode_name)]
        a["valid"] += int((disp != PR.FIXED_ONE).sum()); a["hit"] += int(hit.sum()); a["miss"] += int((traced & ~hit).sum())
        seen["fixed_one"] |= bool((disp == PR.FIXED_ONE).any()); seen["fixed_zero"] |= bool((disp == PR.FIXED_ZERO).any())
        if c.desc.mode == PR.HEMISPHERE:
            seen["z_branch"] |= bool((traced & info["z_branch"]).any()); seen["x_branch"] |= bool((traced & ~info["z_branch"]).any())
        if not c.desc.flags & PR.ANY_HIT:
            between[c.name] = int(((o > 0) & (o < 1)).sum())
            # a hit beyond rayLength: the same rays, ten times as long, meet something the case's rays do not reach
            if not seen["beyond"]:
                sc, cam, tris = PC.scene(c.scene)
                longer = PR.Desc(c.desc.width, c.desc.height, c.desc.mode, c.desc.flags, c.desc.tableW, c.desc.tableH, c.desc.direction,
                                 c.desc.rayLength * F(10.0), c.desc.tMin, c.desc.zNear)
                _, far, _ = (*PR.pixel_rays(sc, sc.objects, c.position, c.normal, c.z, c.table, longer, triangles=tris, meshlet_cull=True), None)
                seen["beyond"] |= bool((((far["status"] & 1) != 0) & ~hit & (far["t"] > c.desc.rayLength)).any())
    return agg, seen, between


def test_conditions_on_the_cases():
    agg, seen, between = _stats()
    assert len(agg) == len(PC.SCENES) * len(PC.MODES)
    for key, a in agg.items():
        assert 5 * a["hit"] >= a["valid"] and 5 * a["miss"] >= a["valid"], (key, a)
    assert seen["z_branch"] and seen["x_branch"], "both createTBN branches"
    assert seen["fixed_one"] and seen["fixed_zero"], "every fixed-answer disposition"
    assert seen["beyond"], "a hit beyond rayLength"
    assert between and all(n >= 1 for n in between.values()), [k for k, n in between.items() if n < 1]


def test_every_size_table_mode_and_depth_setting_is_met():
    for sname in PC.SCENES:
        for mname, (mode, flags, hits) in PC.MODES.items():
            mine = [c for c in CASES if c.scene == sname and c.mode_name == mname]
            assert {(c.desc.width, c.desc.height) for c in mine} == set(PC.SIZES)
            assert {c.depth_name for c in mine} == set(PC.DEPTHS)
            assert {(c.z is not None, c.stride, bool(c.desc.flags & PR.START_FROM_DEPTH)) for c in mine} == \
                {(False, 1, False), (True, 1, False), (True, 1, True), (True, 2, False), (True, 2, True)}
            if mode == PR.HEMISPHERE:
                assert {(c.desc.tableW, c.desc.tableH) for c in mine} == set(PC.TABLES)
            assert any(c.kind == "frame" for c in mine) and any(c.kind == "synthetic" for c in mine)
    for tw, th in PC.TABLES:
        t = PC.table(tw, th).reshape(-1, 4)
        assert (t[:, 2] >= 0).all() and np.allclose(np.linalg.norm(t[:, :3].astype(np.float64), axis=1), 1.0, atol=1e-6)
        if tw * th >= 4:
            assert (t[:, 2] == 0).any() and (t[:, 2] == 1).any()


def test_special_values_give_the_stated_answers():
    """A zero normal, (0, 0, 1e-30) and a NaN-free zero-length normal give a NaN direction in HEMISPHERE and so out = 1; a non-finite
    position is a miss; an invalid pixel is 1 with a zero record; tMin > tMax is a miss."""
    sc, cam, tris = PC.scene("triangle")
    pos = np.zeros((1, 6, 4), dtype=F)
    pos[0, :, :3] = (-0.5, 0.3, -3.8)                                       # 0.1 in front of object 0's triangle, whose plane is z = -4 + y / 3
    pos[0, :, :3] -= np.array(cam.position, dtype=F)
    pos[0, :, 3] = 1.0
    nrm = np.zeros((1, 6, 4), dtype=F)
    nrm[0, :, :3] = [(0, 0, -3.0), (0, 0, 0), (0, 0, 1e-30), (0, 0, -3.0), (0, 0, -3.0), (0, 0, -3.0)]
    pos[0, 3, 1] = np.inf
    pos[0, 4, 3] = 0.0
    tab = np.array([[(0.0, 0.0, 1.0, 0.0)]], dtype=F)
    d = PR.Desc(6, 1, PR.HEMISPHERE, 0, 1, 1, rayLength=0.5, tMin=0.0)
    info = {}
    out, hits = PR.pixel_rays(sc, sc.objects, pos, nrm, None, tab, d, triangles=tris, info=info)
    assert 0 < out[0, 0] < 1 and out[0, 5] == out[0, 0] and hits["status"][0] & 1 and hits["object"][0] == 0
    assert out[0, 1] == 1 and out[0, 2] == 1 and np.isnan(info["rays"]["direction"][1]).any() and np.isnan(info["rays"]["direction"][2]).any()
    assert out[0, 3] == 1 and out[0, 4] == 1 and info["disposition"][4] == PR.FIXED_ONE and info["disposition"][3] == PR.TRACE
    assert not hits[1:5].view(u32).any()
    short = PR.Desc(6, 1, PR.HEMISPHERE, 0, 1, 1, rayLength=0.05, tMin=0.0)
    assert (PR.pixel_rays(sc, sc.objects, pos, nrm, None, tab, short, triangles=tris)[0] == 1).all(), "the triangle lies beyond rayLength"
    crossed = PR.Desc(6, 1, PR.HEMISPHERE, 0, 1, 1, rayLength=0.5, tMin=0.75)
    assert (PR.pixel_rays(sc, sc.objects, pos, nrm, None, tab, crossed, triangles=tris)[0] == 1).all(), "tMin > tMax is a miss"
    away = PR.Desc(6, 1, PR.DIRECTION, PR.ANY_HIT | PR.FRONT_ONLY, direction=(0.0, 0.0, 2.0), rayLength=0.5)
    out, none = PR.pixel_rays(sc, sc.objects, pos, nrm, None, None, away, triangles=tris)
    assert none is None and out[0].tolist() == [0, 0, 0, 0, 1, 0], "facing away (and a zero normal) is 0; an invalid pixel stays 1"
    towards = PR.Desc(6, 1, PR.DIRECTION, PR.ANY_HIT | PR.FRONT_ONLY, direction=(0.0, 0.0, -2.0), rayLength=0.5)
    assert PR.pixel_rays(sc, sc.objects, pos, nrm, None, None, towards, triangles=tris)[0][0].tolist() == [0, 0, 0, 1, 1, 0]
