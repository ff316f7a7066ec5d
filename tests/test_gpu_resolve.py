"""chordvis_resolve_attributes on the GPU, held bit for bit against tests/spec_resolve_np.py (uint32 views: NaN patterns count),
on frames whose visibility words and command lists are read back from the library itself."""
import ctypes as C

import numpy as np
import pytest

from chord_amd import scenes

import helpers as H
import spec_resolve_np as SR

pytestmark = pytest.mark.gpu


def _renderer(scene, view, iv, w, h, flags=H.ALL_FLAGS):
    from chord_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(0)
    r.upload_scene(scene)
    r.allocate_gbuffer(w, h)
    r.set_view(view, iv, flags)
    return r


def _desc(debug_mode=0, vp_nj=None, vp_last_nj=None):
    from chord_amd import lib as L
    d = L.ResolveDesc()
    d.debugMode = debug_mode
    if vp_nj is not None:
        d.useNoJitter = 1
        d.translatedWorldToClipNoJitter[:] = [float(v) for v in np.asarray(vp_nj, dtype=np.float32).reshape(16)]
        d.translatedWorldToClipLastFrameNoJitter[:] = [float(v) for v in np.asarray(vp_last_nj, dtype=np.float32).reshape(16)]
    return d


def _gpu(r, names=None, desc=None):
    out = r.resolve_attributes(names=names, desc=desc)
    import torch
    torch.cuda.synchronize()
    return {n: t.cpu().numpy().view(np.uint32) for n, t in out.items()}


def _spec(r, scene, view, iv, names=SR.NAMES, **kw):
    w, h = r.width, r.height
    return SR.resolve(scene, r.read_visibility(), r.read_cmds(r.last_frame_cmds()), view, iv, w, h, names=names, **kw)


def _assert_same(got, want, what):
    for n, g in got.items():
        wv = np.ascontiguousarray(want[n]).view(np.uint32)
        if n == "debugRGBA8":
            wv = wv.reshape(g.shape)
        if not np.array_equal(g, wv):
            bad = np.argwhere(g.reshape(wv.shape) != wv)
            raise AssertionError("%s %s: %d texels differ; first %s got %r want %r" % (what, n, len(bad), bad[0],
                                 g.reshape(wv.shape)[tuple(bad[0][:2])], wv[tuple(bad[0][:2])]))


def _check(r, scene, view, iv, what, desc=None, **kw):
    got = _gpu(r, desc=desc)
    want = _spec(r, scene, view, iv, **kw)
    _assert_same(got, want, what)
    return got, want


SCENES = [("small", lambda: scenes.small_test_scene(160, 96)),
          ("small_odd", lambda: scenes.small_test_scene(333, 201, seed=8)),
          ("masked", lambda: scenes.masked_test_scene(320, 200)),
          ("built_mesh", lambda: scenes.built_mesh_scene(320, 180, n=48))]


@pytest.mark.parametrize("name,builder", SCENES, ids=[s[0] for s in SCENES])
def test_resolve_equals_the_spec(gpu, name, builder):
    scene, cam, view, iv = H.setup_scene(builder)
    r = _renderer(scene, view, iv, cam.width, cam.height)
    r.render_frame()                                   # frame 0: no history
    got, _ = _check(r, scene, view, iv, name + " frame 0")
    r.render_frame()                                   # frame 1: two-pass HZB
    _check(r, scene, view, iv, name + " frame 1")
    hit = (r.read_visibility() & np.uint64(0xFFFFFFFF)) != 0
    assert hit.sum() > 0.2 * cam.width * cam.height
    if scene.texcoord0 is not None:
        assert np.any(got["uv"].view(np.float32)), "real texture coordinates"
    r.close()


def test_jitter_with_and_without_no_jitter_matrices(gpu):
    from chord_amd import lib as L
    scene, cam = scenes.small_test_scene(200, 120, seed=5)
    jc = scenes.Camera(cam.position, cam.front, cam.width, cam.height, jitter=(0.31, -0.22))
    L.fill_objects(scene, jc)
    view, iv = L.make_views(jc)
    view_nj, _ = L.make_views(cam)                     # chordvis_camera_fill_view with jitter 0
    r = _renderer(scene, view, iv, cam.width, cam.height)
    r.render_frame()
    r.render_frame()
    _check(r, scene, view, iv, "jittered")
    d = _desc(vp_nj=view_nj["translatedWorldToClip"], vp_last_nj=view_nj["translatedWorldToClipLastFrame"])
    _check(r, scene, view, iv, "jittered, no-jitter motion", desc=d, use_no_jitter=True,
                    vp_nj=view_nj["translatedWorldToClip"], vp_last_nj=view_nj["translatedWorldToClipLastFrame"])
    r.close()


def test_moving_camera_and_objects(gpu):
    from chord_amd import lib as L
    scene, cam0 = scenes.small_test_scene(160, 96, seed=11)
    L.fill_objects(scene, cam0)
    v0, iv0 = L.make_views(cam0)
    r = _renderer(scene, v0, iv0, cam0.width, cam0.height)
    r.render_frame()
    cam1 = cam0.moved((0.2, -0.05, 0.3))
    last = scene.local_to_world.copy()
    last[:, 12] -= 0.25
    L.fill_objects(scene, cam1, camera_last=cam0, local_to_world_last=last)
    v1, iv1 = L.make_views(cam1, v0)
    r.update_objects(scene.objects)
    r.set_view(v1, iv1, H.ALL_FLAGS)
    r.render_frame()
    got, _ = _check(r, scene, v1, iv1, "moving")
    assert np.abs(got["motionVector"].view(np.float32)).max() > 1e-3
    r.close()


def test_config3_masked_4k(gpu):
    scene, cam, view, iv = H.setup_scene(scenes.config3_street, 3840, 2160, masked=True)
    r = _renderer(scene, view, iv, cam.width, cam.height)
    r.render_frame()
    r.render_frame()
    _check(r, scene, view, iv, "config 3 masked 4K")
    r.close()


def test_subsets_and_debug_modes(gpu):
    scene, cam, view, iv = H.setup_scene(scenes.masked_test_scene, 320, 200)
    r = _renderer(scene, view, iv, cam.width, cam.height)
    r.render_frame()
    r.render_frame()
    full = _gpu(r)
    for n in SR.NAMES:                                 # every one-target subset equals its plane of the all-targets run
        one = _gpu(r, names=[n])
        assert list(one) == [n] and np.array_equal(one[n], full[n]), n
    pair = _gpu(r, names=["barycentrics", "uvGrad", "motionVector"])
    for n, g in pair.items():
        assert np.array_equal(g, full[n]), n
    for mode in range(5):
        got = _gpu(r, names=["debugRGBA8"], desc=_desc(debug_mode=mode))["debugRGBA8"]
        want = _spec(r, scene, view, iv, names=("debugRGBA8",), debug_mode=mode)["debugRGBA8"]
        if mode <= 2:
            assert np.array_equal(got, want), mode
        else:
            g = got.view(np.uint8).reshape(-1, 4).astype(np.int32)
            wv = want.view(np.uint8).reshape(-1, 4).astype(np.int32)
            assert np.abs(g - wv).max() <= 1, mode
        assert len(np.unique(got)) > 2, mode
    r.close()


def test_nothing_in_view(gpu):
    from chord_amd import lib as L
    scene, cam = scenes.small_test_scene(160, 96)
    away = scenes.Camera((1000.0, 2.0, 1000.0), (1.0, 0.0, 0.0), cam.width, cam.height)   # the scene lies behind the camera
    L.fill_objects(scene, away)
    view, iv = L.make_views(away)
    r = _renderer(scene, view, iv, cam.width, cam.height)
    r.render_frame()
    assert not np.any(r.read_visibility())
    got = _gpu(r)
    for n, g in got.items():
        assert np.all(g == (SR.EMPTY_RGBA8 if n == "debugRGBA8" else 0)), n
    r.close()


def test_sharded_rank_equals_the_single_context(gpu):
    """Two ranks of a sharded frame on one device (the all-gathers replaced by copies, as in test_gpu_parity.py): each rank's
    resolve of the resolved image equals the single context's bit for bit."""
    from chord_amd import lib as L
    from chord_amd.renderer import VisibilityRenderer
    scene, cam, view, iv = H.setup_scene(scenes.masked_test_scene, 320, 200)
    w, h, ranks = cam.width, cam.height, 2
    ref = _renderer(scene, view, iv, w, h)
    ctxs = []
    for rk in range(ranks):
        r = VisibilityRenderer(0)
        r.upload_scene(scene)
        r.set_shard(ranks, rk)
        r.allocate_gbuffer(w, h)
        r.set_view(view, iv, H.ALL_FLAGS)
        ctxs.append(r)
    hip = L._preload_hip_runtime()
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def gather(ptrs, chunk_bytes):
        for r in ctxs:
            r.sync()
        for dst in range(ranks):
            for src in range(ranks):
                if src != dst:
                    assert hip.hipMemcpy(ptrs[dst] + src * chunk_bytes, ptrs[src] + src * chunk_bytes, chunk_bytes, 3) == 0
        assert hip.hipDeviceSynchronize() == 0

    for frame in range(2):
        ref.render_frame()
        if frame > 0:
            for r in ctxs:
                r.frame_phase_cull()
            cx = [r.cull_exchange() for r in ctxs]
            gather([c[0] for c in cx], cx[0][1])
        for r in ctxs:
            r.frame_phase_a()
        ex = [r.hzb_exchange() for r in ctxs]
        gather([e[0] for e in ex], ex[0][2] * 2)
        for r in ctxs:
            r.frame_phase_b()
        fin = [r.hzb_final_exchange() for r in ctxs]
        gather([f[0] for f in fin], fin[0][1])
        gather([r.visibility_ptr() for r in ctxs], ctxs[0].visibility_chunk_words() * 8)
        for r in ctxs:
            r.frame_phase_c()
    want = _gpu(ref)
    _assert_same(want, _spec(ref, scene, view, iv), "single context")
    for rk, r in enumerate(ctxs):
        H.assert_vis_equal(r.read_visibility(), ref.read_visibility(), w, h, "rank %d" % rk)
        got = _gpu(r)
        for n in SR.NAMES:
            assert np.array_equal(got[n], want[n]), (rk, n)
    for r in ctxs + [ref]:
        r.close()


def test_refusals(gpu):
    from chord_amd import lib as L
    scene, cam, view, iv = H.setup_scene(scenes.small_test_scene, 160, 96)
    r = _renderer(scene, view, iv, cam.width, cam.height)
    with pytest.raises(L.ChordvisError, match="no frame"):
        r.resolve_attributes(names=["barycentrics"])
    r.render_frame()
    r.resolve_attributes(names=["barycentrics"])
    none = L.ResolveTargets()
    rc = L.lib.chordvis_resolve_attributes(r._ctx, r.last_frame_cmds(), None, C.byref(none))
    assert rc == L.E_INVALID and b"no target" in L.lib.chordvis_last_error(r._ctx)
    with pytest.raises(L.ChordvisError, match="debugMode"):
        r.resolve_attributes(names=["debugRGBA8"], desc=_desc(debug_mode=5))
    r.resolve_attributes(names=["uv"], desc=_desc(debug_mode=5))      # (the mode is read only for debugRGBA8)
    r.update_objects(scene.objects)
    with pytest.raises(L.ChordvisError, match="came after the frame"):
        r.resolve_attributes(names=["barycentrics"])
    r.render_frame()
    r.resolve_attributes(names=["barycentrics"])
    r.set_view(view, iv, H.ALL_FLAGS)
    with pytest.raises(L.ChordvisError, match="came after the frame"):
        r.resolve_attributes(names=["barycentrics"])
    r.close()


def test_resolving_between_frames_leaves_the_next_frame_alone(gpu):
    scene, cam, view, iv = H.setup_scene(scenes.small_test_scene, 160, 96)
    a = _renderer(scene, view, iv, cam.width, cam.height)
    b = _renderer(scene, view, iv, cam.width, cam.height)
    a.render_frame(); b.render_frame()
    _gpu(a)
    a.render_frame(); b.render_frame()
    H.assert_vis_equal(a.read_visibility(), b.read_visibility(), cam.width, cam.height, "after a resolve")
    a.close(); b.close()
