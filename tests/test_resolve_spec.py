"""chordvis_resolve_attributes without a GPU: the layouts of its two structs (header vs ctypes mirrors), and the numpy
restatement of its arithmetic (tests/spec_resolve_np.py) held against the oracle's raster -- the barycentrics of a covered pixel
reproduce the pixel centre and the word's depth, their derivatives the neighbours' differences, the motion vectors a float64
reprojection."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from chord_amd import scenes

import helpers as H
import spec_resolve_np as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_resolve_struct_layouts_match_the_header(built_lib):
    L = built_lib
    mirrors = (("ChordResolveDesc", L.ResolveDesc), ("ChordResolveTargets", L.ResolveTargets))
    lines = []
    for cname, ct in mirrors:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in ct._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines.append('printf("debugModes %u\\n", CHORD_NANITE_DEBUG_BARYCENTRICS);')
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "chordvis.h"\nint main(void){\n%s\nreturn 0;}\n' % "\n".join(lines)
    with tempfile.TemporaryDirectory() as td:
        cpath, exe = os.path.join(td, "l.c"), os.path.join(td, "l")
        open(cpath, "w").write(src)
        cc = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), cpath, "-o", exe], capture_output=True, text=True)
        assert cc.returncode == 0, cc.stderr[-1500:]
        out = dict(l.split() for l in subprocess.check_output([exe]).decode().splitlines())
    for cname, ct in mirrors:
        assert int(out[cname]) == C.sizeof(ct), cname
        for f, _ in ct._fields_:
            assert int(out["%s.%s" % (cname, f)]) == getattr(ct, f).offset, (cname, f)
    assert int(out["ChordResolveDesc"]) == 144 and int(out["ChordResolveTargets"]) == 64
    assert int(out["debugModes"]) == L.DEBUG_BARYCENTRICS == 4
    assert list(L.RESOLVE_CHANNELS) == [f for f, _ in L.ResolveTargets._fields_] == list(SR.NAMES)


SCENES = [("small", lambda: scenes.small_test_scene(160, 96)),
          ("masked", lambda: scenes.masked_test_scene(320, 200)),
          ("built_mesh", lambda: scenes.built_mesh_scene(320, 180, n=48))]


def _frame(scene, view, iv):
    import orc
    return orc.frame(scene, view, iv, H.ALL_FLAGS)


def _depth(vis):
    return (np.asarray(vis, dtype=np.uint64) >> np.uint64(32)).astype(np.uint32).view(f32)


@pytest.mark.parametrize("name,builder", SCENES, ids=[s[0] for s in SCENES])
def test_spec_barycentrics_reproduce_the_oracle_raster(built_lib, name, builder):
    scene, cam, view, iv = H.setup_scene(builder)
    w, h = cam.width, cam.height
    fr = _frame(scene, view, iv)
    got = SR.resolve(scene, fr["vis"], fr["cmds"], view, iv, w, h, extras=True)
    hit = got["hit"]
    assert hit.sum() > 0.2 * w * h, name
    low = (fr["vis"] & np.uint64(0xFFFFFFFF)).astype(np.uint32).reshape(h, w)
    assert np.array_equal(hit, low != 0), "every covered pixel of an oracle frame resolves"
    b = got["barycentrics"][..., :3][hit].astype(np.float64)
    # inside the triangle, up to the raster's vertex snapping: a pixel centre may lie up to one 1/256-pixel step
    # (CHORD_SUBPIXEL_BITS) outside the unsnapped triangle, which moves a barycentric by (|ddx| + |ddy|) / 256
    snap = (np.abs(got["baryDdx"][..., :3][hit]) + np.abs(got["baryDdy"][..., :3][hit])).astype(np.float64) / 256.0
    assert np.all(b >= -1e-4 - snap) and np.all(b <= 1 + 1e-4 + snap), (b.min(), b.max())
    assert np.mean(b < -1e-4) < 0.01, "off-triangle centres are rare"
    assert np.abs(b.sum(-1) - 1.0).max() <= 1e-5
    # the interpolated clip position projects to the pixel centre and to the word's depth
    phs_all = got["phs"][hit].astype(np.float64)
    phs, pdx, pdy = phs_all[:, 0], phs_all[:, 1], phs_all[:, 2]
    ys, xs = np.nonzero(hit)
    sx = (phs[:, 0] / phs[:, 3] * 0.5 + 0.5) * w - (xs + 0.5)
    sy = (0.5 - phs[:, 1] / phs[:, 3] * 0.5) * h - (ys + 0.5)
    assert np.abs(sx).max() <= 1e-3 and np.abs(sy).max() <= 1e-3, (np.abs(sx).max(), np.abs(sy).max())
    # the word's depth: relative 1e-5, plus what one sub-pixel snapping step moves z / w by (its screen gradient / 256)
    z = _depth(fr["vis"]).reshape(h, w)[hit].astype(np.float64)
    zw = phs[:, 2] / phs[:, 3]
    dzw = lambda d: (d[:, 2] * phs[:, 3] - phs[:, 2] * d[:, 3]) / (phs[:, 3] * phs[:, 3])
    tol = 1e-5 * np.abs(z) + (np.abs(dzw(pdx)) + np.abs(dzw(pdy))) / 256.0
    assert np.all(np.abs(zw - z) <= tol), np.max(np.abs(zw - z) / tol)
    assert np.median(np.abs(zw - z) / np.abs(z)) <= 1e-4
    # screen derivatives: the difference to the neighbour on the same triangle (same low word)
    bary = got["barycentrics"][..., :3].astype(np.float64)
    for axis, key in ((1, "baryDdx"), (0, "baryDdy")):
        a = [slice(None), slice(None)]; c = [slice(None), slice(None)]
        a[axis], c[axis] = slice(0, -1), slice(1, None)
        same = hit[tuple(a)] & (low[tuple(a)] == low[tuple(c)])
        assert same.sum() > 0.1 * w * h, key
        diff = (bary[tuple(c)] - bary[tuple(a)])[same]
        dd = got[key][..., :3].astype(np.float64)
        d = 0.5 * (dd[tuple(a)] + dd[tuple(c)])[same]              # (the derivative at both ends: bary is not linear in screen space)
        assert np.abs(diff - d).max() <= 1e-3, (key, np.abs(diff - d).max())
    # static camera and objects: no motion at all; empty pixels are zero everywhere
    assert not np.any(got["motionVector"])
    for n in SR.NAMES:
        if n != "debugRGBA8":
            assert not np.any(got[n][~hit]), n
    assert np.all(got["debugRGBA8"][~hit] == SR.EMPTY_RGBA8)
    assert np.all(got["positionRS"][hit][:, 3] == 1.0)


def _reprojection64(scene, fr, view, iv, got, w, h):
    """float64: the pixel's point from the (spec) barycentrics of its triangle, through VP*M and VP_last*M_last."""
    import spec_np as S
    low = (fr["vis"] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    hit = got["hit"].reshape(-1)
    setup = SR.triangle_setup(scene, fr["cmds"], np.asarray(view).reshape(-1)[0], np.asarray(iv).reshape(-1)[0], low[hit])
    cmd = fr["cmds"][((low[hit] >> 8) & 0xFFFFFF).astype(np.int64) - 1]
    obj = scene.objects[cmd["objectId"]]
    m = scene.meshlets[cmd["meshletId"]]
    tw = scene.meshlet_data[m["dataOffset"].astype(np.int64) + (m["vertexTriangleCount"] & 0xFF) + (low[hit] & 0xFF)]
    vb = scene.primitives["vertexOffset"][obj["GLTFPrimitiveDetail"]].astype(np.int64)
    p = np.stack([scene.positions[scene.meshlet_data[m["dataOffset"].astype(np.int64) + ((tw >> (8 * i)) & 0xFF)].astype(np.int64) + vb]
                  for i in range(3)], 1).astype(np.float64)
    b = got["barycentrics"].reshape(-1, 4)[hit, :3].astype(np.float64)
    ploc = (p * b[..., None]).sum(1)
    ph = np.concatenate([ploc, np.ones((len(ploc), 1))], 1)
    M = S.mat(obj["localToTranslatedWorld"]).astype(np.float64)
    Ml = S.mat(obj["localToTranslatedWorldLastFrame"]).astype(np.float64)
    VP = S.mat(np.asarray(iv["translatedWorldToClip"]).reshape(16)).astype(np.float64)
    VPl = S.mat(np.asarray(view["translatedWorldToClipLastFrame"]).reshape(16)).astype(np.float64)
    cur = np.einsum("ij,njk,nk->ni", VP, M, ph)
    last = np.einsum("ij,njk,nk->ni", VPl, Ml, ph)
    mv = (last[:, :2] / last[:, 3:4] - cur[:, :2] / cur[:, 3:4]) * np.array([0.5, -0.5])
    assert setup["ok"].all()
    return mv, hit


@pytest.mark.parametrize("move", ["camera", "object"])
def test_spec_motion_matches_a_float64_reprojection(built_lib, move):
    from chord_amd import lib as L
    scene, cam = scenes.small_test_scene(160, 96)
    cam0 = cam
    if move == "camera":
        cam1 = cam0.moved((0.15, -0.05, 0.2))
        L.fill_objects(scene, cam1, camera_last=cam0)
        view0, _ = L.make_views(cam0)
        view, iv = L.make_views(cam1, view0)
    else:
        last = scene.local_to_world.copy()
        last[:, 12] -= 0.3                                            # translation x of the previous frame (column-major)
        last[:, 14] += 0.1
        L.fill_objects(scene, cam0, local_to_world_last=last)
        view, iv = L.make_views(cam0)
    w, h = cam0.width, cam0.height
    fr = _frame(scene, view, iv)
    got = SR.resolve(scene, fr["vis"], fr["cmds"], view, iv, w, h, names=("barycentrics", "motionVector"), extras=True)
    mv64, hit = _reprojection64(scene, fr, view, iv, got, w, h)
    mv = got["motionVector"].reshape(-1, 2)[hit].astype(np.float64)
    assert np.abs(mv64).max() > 1e-3, "the move shows in the motion vectors"
    assert np.abs(mv - mv64).max() <= 1e-4, np.abs(mv - mv64).max()


def test_spec_debug_colours():
    c = SR.pack_rgba8(np.array([[0.0, 0.5, 1.0], [np.nan, -1.0, 2.0]], dtype=f32))
    assert list(c) == [0xFF000000 | 0 | 128 << 8 | 255 << 16, 0xFF000000 | 0 | 0 << 8 | 255 << 16]
    col = SR.simple_hash_color(np.arange(1000, dtype=np.uint32))
    h = SR.simple_hash(np.arange(1000, dtype=np.uint32))
    assert np.array_equal(SR.pack_rgba8(col) & 0xFFFFFF, h & 0xFFFFFF), "a hash colour packs back to the hash's low three bytes"
