"""chordvis_resolve_surface on the GPU: the vertex normal, tangent and bitangent images held bit for bit against
tests/spec_surface_np.py, and the eight images of chordvis_resolve_attributes unchanged when written in the same launch."""
import ctypes as C

import numpy as np
import pytest

from chord_amd import records as R, scenes

import helpers as H
import multi_asset as MA
import spec_resolve_np as SR
import spec_surface_np as SS

pytestmark = pytest.mark.gpu


def _renderer(scene, view, iv, w, h, flags=H.ALL_FLAGS):
    from chord_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(0)
    r.upload_scene(scene)
    r.allocate_gbuffer(w, h)
    r.set_view(view, iv, flags)
    return r


def _gpu(r, names):
    out = r.resolve_attributes(names=names)
    import torch
    torch.cuda.synchronize()
    return {n: t.cpu().numpy().view(np.uint32) for n, t in out.items()}


def _check(r, scene, view, iv, what, names=SS.NAMES, spec_scene=None, cmds=None, **kw):
    got = _gpu(r, list(names))
    want = SS.resolve(spec_scene or scene, r.read_visibility(), r.read_cmds(r.last_frame_cmds()) if cmds is None else cmds, view, iv, r.width, r.height,
                      names=names, **kw)
    for n in names:
        wv = np.ascontiguousarray(want[n]).view(np.uint32)
        if not np.array_equal(got[n], wv):
            bad = np.argwhere(got[n] != wv)
            raise AssertionError("%s %s: %d texels differ; first %s got %r want %r" % (what, n, len(bad), bad[0],
                                 got[n][tuple(bad[0][:2])].view(np.float32), wv[tuple(bad[0][:2])].view(np.float32)))
    return got


SCENES = [("small", lambda: scenes.small_test_scene(160, 96, attributes=True)),
          ("small_odd", lambda: scenes.small_test_scene(333, 201, seed=8, attributes=True)),
          ("masked", lambda: scenes.masked_test_scene(320, 200, attributes=True)),
          ("built_mesh", lambda: scenes.built_mesh_scene(320, 180, n=48, attributes=True))]


@pytest.mark.parametrize("name,builder", SCENES, ids=[s[0] for s in SCENES])
def test_surface_equals_the_spec(gpu, name, builder):
    scene, cam, view, iv = H.setup_scene(builder)
    r = _renderer(scene, view, iv, cam.width, cam.height)
    r.render_frame()                                   # frame 0: no history
    _check(r, scene, view, iv, name + " frame 0")
    r.render_frame()                                   # frame 1: two-pass HZB
    got = _check(r, scene, view, iv, name + " frame 1")
    hit = ((r.read_visibility() & np.uint64(0xFFFFFFFF)) != 0).reshape(cam.height, cam.width)
    assert hit.sum() > 0.2 * cam.width * cam.height
    n = got["vertexNormal"].view(np.float32)[hit]
    ln = np.linalg.norm(n[:, :3], axis=1)
    assert np.all((ln > 0.5) & (ln < 1.01)), "interpolated unit normals (shorter between diverging ones)"
    assert np.all(n[:, 3] == 0.0) and not np.any(got["tangent"][~hit])
    r.close()


def test_resolve_attributes_images_are_unchanged_beside_the_surface(gpu):
    """The eight images of chordvis_resolve_attributes equal those of chordvis_resolve_surface asked for all eleven, and every
    subset of the three surface targets equals its plane of the full run."""
    scene, cam, view, iv = H.setup_scene(scenes.masked_test_scene, 320, 200, attributes=True)
    r = _renderer(scene, view, iv, cam.width, cam.height)
    r.render_frame()
    r.render_frame()
    from chord_amd import lib as L
    alone = _gpu(r, list(L.RESOLVE_CHANNELS))
    both = _gpu(r, list(L.RESOLVE_CHANNELS) + list(SS.NAMES))
    for n in L.RESOLVE_CHANNELS:
        assert np.array_equal(alone[n], both[n]), n
    want = SR.resolve(scene, r.read_visibility(), r.read_cmds(r.last_frame_cmds()), view, iv, r.width, r.height)
    for n in L.RESOLVE_CHANNELS:
        assert np.array_equal(both[n], np.ascontiguousarray(want[n]).view(np.uint32).reshape(both[n].shape)), n
    for k in range(1, 8):
        names = [SS.NAMES[i] for i in range(3) if k & (1 << i)]
        sub = _gpu(r, names)
        assert sorted(sub) == sorted(names)
        for n in names:
            assert np.array_equal(sub[n], both[n]), (names, n)
    r.close()


def test_config3_4k(gpu):
    scene, cam, view, iv = H.setup_scene(scenes.config3_street, 3840, 2160, attributes=True)
    r = _renderer(scene, view, iv, cam.width, cam.height)
    r.render_frame()
    r.render_frame()
    _check(r, scene, view, iv, "config 3 4K")
    r.close()


def test_an_asset_without_normals_beside_one_with_them(gpu):
    from chord_amd import lib as L
    a, cam = scenes.small_test_scene(200, 120, attributes=True)
    b, _ = scenes.small_test_scene(200, 120, seed=9)
    b.local_to_world = b.local_to_world.copy()
    b.local_to_world[:, 12] += 1.5                     # (the second asset's objects beside the first's)
    two = MA.MultiAssetScene([a, b])                    # (tests/multi_asset.py: what _TwoAssetScene of this file grew into)
    L.fill_objects(two, cam)
    assert two.spec.objects is two.objects
    view, iv = L.make_views(cam)
    r = _renderer(two, view, iv, cam.width, cam.height)
    r.render_frame()
    r.render_frame()
    cmds = r.read_cmds(r.last_frame_cmds())
    vis = r.read_visibility()
    slot = ((vis & np.uint64(0xFFFFFFFF)) >> np.uint64(8)).astype(np.int64) - 1
    on = slot[(slot >= 0) & (slot < len(cmds))]
    objs = cmds["objectId"][on]
    assert np.any(objs < len(a.objects)) and np.any(objs >= len(a.objects)), "both assets on screen"
    assert np.any(two.asset_of_object[objs] == 0) and np.any(two.asset_of_object[objs] == 1), "both assets on screen (objects are interleaved)"
    cmds = two.to_concatenated(cmds)                   # (the list reads back asset-relative; the twin's meshlets are concatenated)
    got = _check(r, two, view, iv, "two assets", spec_scene=two.spec, cmds=cmds)
    assert np.any(got["vertexNormal"].view(np.float32)[..., :3] != 0.0)
    r.close()


def test_moving_camera_and_objects(gpu):
    """The frame's matrices, not the last frame's, transform the normals and tangents."""
    from chord_amd import lib as L
    scene, cam0 = scenes.small_test_scene(160, 96, seed=11, attributes=True)
    L.fill_objects(scene, cam0)
    v0, iv0 = L.make_views(cam0)
    r = _renderer(scene, v0, iv0, cam0.width, cam0.height)
    r.render_frame()
    cam1 = cam0.moved((0.2, -0.05, 0.3))
    last = scene.local_to_world.copy()
    scene.local_to_world = scene.local_to_world.copy()
    m = scenes.rotate_y(0.4)
    for k in range(1, len(last)):                      # objects turn about their own origin: the normals move with them
        l2w = scene.local_to_world[k].reshape(4, 4).T
        scene.local_to_world[k] = (l2w @ m).T.reshape(16)
    L.fill_objects(scene, cam1, camera_last=cam0, local_to_world_last=last)
    v1, iv1 = L.make_views(cam1, v0)
    r.update_objects(scene.objects)
    r.set_view(v1, iv1, H.ALL_FLAGS)
    r.render_frame()
    _check(r, scene, v1, iv1, "moving")
    r.close()


def test_sharded_rank_equals_the_single_context(gpu):
    """Two ranks of a sharded frame on one device (the all-gathers replaced by copies, as in test_gpu_resolve.py): each rank's
    surface resolve of the resolved image equals the single context's bit for bit."""
    from chord_amd import lib as L
    from chord_amd.renderer import VisibilityRenderer
    scene, cam, view, iv = H.setup_scene(scenes.masked_test_scene, 320, 200, attributes=True)
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
    want = _check(ref, scene, view, iv, "single context")
    for rk, r in enumerate(ctxs):
        H.assert_vis_equal(r.read_visibility(), ref.read_visibility(), w, h, "rank %d" % rk)
        got = _gpu(r, list(SS.NAMES))
        for n in SS.NAMES:
            assert np.array_equal(got[n], want[n]), (rk, n)
    for r in ctxs + [ref]:
        r.close()


def test_refusals(gpu):
    from chord_amd import lib as L
    plain, cam = scenes.small_test_scene(160, 96)
    L.fill_objects(plain, cam)
    view, iv = L.make_views(cam)
    r = _renderer(plain, view, iv, cam.width, cam.height)
    r.render_frame()
    with pytest.raises(L.ChordvisError, match="without normals"):
        r.resolve_attributes(names=["vertexNormal"])
    with pytest.raises(L.ChordvisError, match="without tangents"):
        r.resolve_attributes(names=["tangent"])
    r.resolve_attributes(names=["barycentrics"])                   # (the eight images need neither)
    r.close()
    no_tangents = R.Scene(plain.objects, plain.primitives, plain.materials, plain.meshlets, plain.groups, plain.group_indices,
                          plain.meshlet_data, plain.positions, normals=scenes.small_test_scene(160, 96, attributes=True)[0].normals)
    r = _renderer(no_tangents, view, iv, cam.width, cam.height)
    with pytest.raises(L.ChordvisError, match="no frame"):
        r.resolve_attributes(names=["vertexNormal"])
    r.render_frame()
    r.resolve_attributes(names=["vertexNormal"])
    for n in ("tangent", "bitangent"):
        with pytest.raises(L.ChordvisError, match="without tangents"):
            r.resolve_attributes(names=[n])
    none, surf = L.ResolveTargets(), L.SurfaceTargets()
    rc = L.lib.chordvis_resolve_surface(r._ctx, r.last_frame_cmds(), None, None, C.byref(surf))
    assert rc == L.E_INVALID and b"no target" in L.lib.chordvis_last_error(r._ctx)
    rc = L.lib.chordvis_resolve_surface(r._ctx, r.last_frame_cmds(), None, C.byref(none), None)
    assert rc == L.E_INVALID and b"no target" in L.lib.chordvis_last_error(r._ctx)
    d = L.ResolveDesc()
    d.debugMode = 5
    with pytest.raises(L.ChordvisError, match="debugMode"):
        r.resolve_attributes(names=["debugRGBA8", "vertexNormal"], desc=d)
    r.update_objects(no_tangents.objects)
    with pytest.raises(L.ChordvisError, match="came after the frame"):
        r.resolve_attributes(names=["vertexNormal"])
    r.render_frame()
    r.resolve_attributes(names=["vertexNormal"])
    r.set_view(view, iv, H.ALL_FLAGS)
    with pytest.raises(L.ChordvisError, match="came after the frame"):
        r.resolve_attributes(names=["vertexNormal"])
    r.close()


def test_resolving_between_frames_leaves_the_next_frame_alone(gpu):
    scene, cam, view, iv = H.setup_scene(scenes.small_test_scene, 160, 96, attributes=True)
    a = _renderer(scene, view, iv, cam.width, cam.height)
    b = _renderer(scene, view, iv, cam.width, cam.height)
    a.render_frame(); b.render_frame()
    _gpu(a, list(SS.NAMES) + ["barycentrics"])
    a.render_frame(); b.render_frame()
    H.assert_vis_equal(a.read_visibility(), b.read_visibility(), cam.width, cam.height, "after a surface resolve")
    a.close(); b.close()


def test_group_ranks_carry_the_streams(gpu):
    """chordvis_group_upload_scene uploads the normals and tangents to every rank: each rank of a two-rank group (on one device)
    resolves the surface of the gathered image as the single context does."""
    from chord_amd.renderer import VisibilityGroup
    scene, cam, view, iv = H.setup_scene(scenes.small_test_scene, 160, 96, attributes=True)
    w, h = cam.width, cam.height
    ref = _renderer(scene, view, iv, w, h)
    ref.render_frame()
    ref.render_frame()
    want = _check(ref, scene, view, iv, "single context")
    g = VisibilityGroup([0, 0])
    g.upload_scene(scene)
    g.allocate_gbuffer(w, h)
    g.set_view(view, iv, H.ALL_FLAGS)
    g.render_frame()
    g.render_frame()
    g.sync()
    for rk, r in enumerate(g.ranks):
        H.assert_vis_equal(r.read_visibility(), ref.read_visibility(), w, h, "rank %d" % rk)
        got = _gpu(r, list(SS.NAMES))
        for n in SS.NAMES:
            assert np.array_equal(got[n], want[n]), (rk, n)
    g.close()
    ref.close()
