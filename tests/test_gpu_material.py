"""chordvis_resolve_material on the GPU, through the C ABI: base colour, emissive, pixel normal and roughness / metallic / AO held
bit for bit (uint32 views) against tests/spec_material_np.py; the eleven earlier images unchanged beside them; refusals; frames
untouched by chordvis_upload_material_textures."""
import ctypes as C

import numpy as np
import pytest

from chord_amd import records as R, scenes

import helpers as H
import spec_material_np as SM
import spec_resolve_np as SR
import spec_surface_np as SS

pytestmark = pytest.mark.gpu


def _renderer(scene, view, iv, w, h, flags=H.ALL_FLAGS, textures=True):
    from chord_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(0)
    r.upload_scene(scene)
    if textures:
        r.upload_material_textures()
    r.allocate_gbuffer(w, h)
    r.set_view(view, iv, flags)
    return r


def _gpu(r, names):
    out = r.resolve_attributes(names=names)
    import torch
    torch.cuda.synchronize()
    return {n: t.cpu().numpy().view(np.uint32) for n, t in out.items()}


def _check(r, scene, view, iv, what, names=SM.NAMES):
    got = _gpu(r, list(names))
    want = SM.resolve(scene, r.read_visibility(), r.read_cmds(r.last_frame_cmds()), view, iv, r.width, r.height, names=names)
    for n in names:
        wv = np.ascontiguousarray(want[n]).view(np.uint32)
        if not np.array_equal(got[n], wv):
            bad = np.argwhere(got[n] != wv)
            raise AssertionError("%s %s: %d texels differ; first %s got %r want %r" % (what, n, len(bad), bad[0],
                                 got[n][tuple(bad[0][:2])].view(np.float32), wv[tuple(bad[0][:2])].view(np.float32)))
    return got


SCENES = [("material", lambda: scenes.material_test_scene(320, 200)),
          ("material_odd", lambda: scenes.material_test_scene(333, 201)),
          ("masked", lambda: scenes.masked_test_scene(320, 200, attributes=True)),
          ("built_mesh", lambda: scenes.built_mesh_scene(320, 180, n=48, attributes=True))]


@pytest.mark.parametrize("name,builder", SCENES, ids=[s[0] for s in SCENES])
def test_material_equals_the_spec(gpu, name, builder):
    scene, cam, view, iv = H.setup_scene(builder)
    r = _renderer(scene, view, iv, cam.width, cam.height)
    r.render_frame()                                   # frame 0: no history
    _check(r, scene, view, iv, name + " frame 0")
    r.render_frame()                                   # frame 1: two-pass HZB
    got = _check(r, scene, view, iv, name + " frame 1")
    hit = ((r.read_visibility() & np.uint64(0xFFFFFFFF)) != 0).reshape(cam.height, cam.width)
    assert hit.sum() > 0.2 * cam.width * cam.height
    for n in SM.NAMES:
        assert not np.any(got[n][~hit]), n
        assert not np.any(np.isnan(got[n].view(np.float32))), n
    assert np.any(got["baseColor"][hit]) and np.any(got["pixelNormal"][hit])
    r.close()


def test_general_transforms_over_moving_cameras(gpu):
    """Mirrored and stretched objects (the bitangent's sign through the TBN), camera and objects in motion."""
    scene, cam0, _ = scenes.general_transform_scene(320, 180, materials=True)
    cams = scenes.general_cameras(cam0, 3)
    view, iv = H.moving_frame(scene, cams, 0)
    r = _renderer(scene, view, iv, cam0.width, cam0.height)
    for k in range(len(cams)):
        if k:
            view, iv = H.moving_frame(scene, cams, k, view)
            r.update_objects(scene.objects)
            r.set_view(view, iv, H.ALL_FLAGS)
        r.render_frame()
        _check(r, scene, view, iv, "view %d" % k)
    r.close()


def test_config3_4k(gpu):
    scene, cam, view, iv = H.setup_scene(scenes.config3_street, 3840, 2160, materials=True)
    r = _renderer(scene, view, iv, cam.width, cam.height)
    r.render_frame()
    r.render_frame()
    _check(r, scene, view, iv, "config 3 4K")
    r.close()


def test_earlier_images_are_unchanged_and_subsets_equal_the_full_run(gpu):
    """The eleven earlier images written by chordvis_resolve_material equal those of chordvis_resolve_surface on the same frame,
    and every one of the 15 non-empty subsets of the four material targets equals its plane of the full run."""
    from chord_amd import lib as L
    scene, cam, view, iv = H.setup_scene(scenes.material_test_scene, 320, 200)
    r = _renderer(scene, view, iv, cam.width, cam.height)
    r.render_frame()
    r.render_frame()
    eleven = list(L.RESOLVE_CHANNELS) + list(L.SURFACE_CHANNELS)
    alone = _gpu(r, eleven)
    full = _gpu(r, eleven + list(SM.NAMES))
    for n in eleven:
        assert np.array_equal(alone[n], full[n]), n
    want = SR.resolve(scene, r.read_visibility(), r.read_cmds(r.last_frame_cmds()), view, iv, r.width, r.height)
    for n in L.RESOLVE_CHANNELS:
        assert np.array_equal(full[n], np.ascontiguousarray(want[n]).view(np.uint32).reshape(full[n].shape)), n
    for k in range(1, 16):
        names = [SM.NAMES[i] for i in range(4) if k & (1 << i)]
        sub = _gpu(r, names)
        assert sorted(sub) == sorted(names)
        for n in names:
            assert np.array_equal(sub[n], full[n]), (names, n)
    r.close()


def test_sharded_rank_equals_the_single_context(gpu):
    """Two ranks of a sharded frame on one device (the all-gathers replaced by copies, as in test_gpu_resolve.py): each rank holds
    the textures and records and resolves the four images of the resolved image as the single context does."""
    from chord_amd import lib as L
    from chord_amd.renderer import VisibilityRenderer
    scene, cam, view, iv = H.setup_scene(scenes.material_test_scene, 320, 200)
    w, h, ranks = cam.width, cam.height, 2
    ref = _renderer(scene, view, iv, w, h)
    ctxs = []
    for rk in range(ranks):
        r = VisibilityRenderer(0)
        r.upload_scene(scene)
        r.upload_material_textures()
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
        got = _gpu(r, list(SM.NAMES))
        for n in SM.NAMES:
            assert np.array_equal(got[n], want[n]), (rk, n)
    for r in ctxs + [ref]:
        r.close()


def _without(scene, normals=True, tangents=True):
    out = R.Scene(scene.objects, scene.primitives, scene.materials, scene.meshlets, scene.groups, scene.group_indices,
                  scene.meshlet_data, scene.positions, texcoord0=scene.texcoord0, textures=scene.texture_images,
                  samplers=scene.samplers, bvh_nodes=scene.bvh_nodes, normals=scene.normals if normals else None,
                  tangents=scene.tangents if tangents else None)
    return out


def test_refusals(gpu):
    from chord_amd import lib as L
    scene, cam, view, iv = H.setup_scene(scenes.material_test_scene, 160, 100)
    r = _renderer(scene, view, iv, cam.width, cam.height, textures=False)
    r.render_frame()
    with pytest.raises(L.ChordvisError, match="no chordvis_upload_material_textures"):
        r.resolve_attributes(names=["baseColor"])
    r.resolve_attributes(names=["barycentrics", "vertexNormal"])          # (the earlier images need no textures)
    r.upload_material_textures()
    r.resolve_attributes(names=["baseColor"])                             # (no new frame needed: frames do not read them)
    r.upload_scene(scene)                                                 # a second upload_scene drops them
    r.allocate_gbuffer(cam.width, cam.height)
    r.set_view(view, iv, H.ALL_FLAGS)
    r.render_frame()
    with pytest.raises(L.ChordvisError, match="no chordvis_upload_material_textures"):
        r.resolve_attributes(names=["roughMetalAO"])
    # targets and surface NULL, no material target: "no target"
    rc = L.lib.chordvis_resolve_material(r._ctx, r.last_frame_cmds(), None, None, None, C.byref(L.MaterialTargets()))
    assert rc == L.E_INVALID and b"no target" in L.lib.chordvis_last_error(r._ctx)
    r.close()
    # pixelNormal without normals; without tangents when a normal map exists
    bare = _without(scene, normals=False, tangents=False)
    r = _renderer(bare, view, iv, cam.width, cam.height)
    r.render_frame()
    with pytest.raises(L.ChordvisError, match="pixelNormal needs a scene uploaded with normals"):
        r.resolve_attributes(names=["pixelNormal"])
    r.resolve_attributes(names=["baseColor", "emissive", "roughMetalAO"])
    r.close()
    no_t = _without(scene, tangents=False)
    r = _renderer(no_t, view, iv, cam.width, cam.height)
    r.render_frame()
    with pytest.raises(L.ChordvisError, match="needs a scene uploaded with tangents"):
        r.resolve_attributes(names=["pixelNormal"])
    r.close()
    # ... but a scene whose materials name no normal texture resolves pixelNormal (= vertexNormal) without tangents
    plain, pcam, pview, piv = H.setup_scene(scenes.small_test_scene, 160, 96, attributes=True)
    plain = _without(plain, tangents=False)
    r = _renderer(plain, pview, piv, pcam.width, pcam.height)
    r.render_frame()
    got = _gpu(r, ["pixelNormal", "vertexNormal"])
    assert np.array_equal(got["pixelNormal"], got["vertexNormal"]) and np.any(got["pixelNormal"])
    r.close()


class _NullTextures:
    """`scene` with the pixel data of the chosen textures taken away (ChordTexture::rgba8 = NULL)."""

    def __init__(self, scene, which):
        self._scene = scene
        n = len(scene.texture_images)
        self._textures = (R.Texture * n)()
        for i in range(n):
            t = scene._textures[i]
            self._textures[i] = R.Texture(None if i in which else t.rgba8, t.width, t.height, t.mipCount, 0)
        d = scene.desc
        self.desc = R.SceneDesc(d.objects, d.objectCount, d.primitives, d.primitiveCount, d.materials, d.materialCount,
                                d.assets, d.assetCount, C.cast(self._textures, C.c_void_p), n, d.samplers, d.samplerCount)


def test_a_named_texture_without_data(gpu):
    """upload_scene still accepts NULL data in textures the visibility pass does not sample (unchanged behaviour);
    upload_material_textures refuses a named one, keeps nothing, and the context still renders and resolves the earlier images."""
    from chord_amd import lib as L
    scene, cam, view, iv = H.setup_scene(scenes.material_test_scene, 160, 100, masked=False)
    holes = _NullTextures(scene, which={2, 3, 4})     # normal, metallic-roughness, emissive: no masked material samples them
    r = _renderer(scene, view, iv, cam.width, cam.height, textures=False)
    r.upload_scene(holes)                             # accepted
    r.scene = scene
    r.allocate_gbuffer(cam.width, cam.height)
    r.set_view(view, iv, H.ALL_FLAGS)
    with pytest.raises(L.ChordvisError, match="has no data"):
        r.upload_material_textures(holes)
    r.render_frame()
    with pytest.raises(L.ChordvisError, match="no chordvis_upload_material_textures"):
        r.resolve_attributes(names=["baseColor"])
    got = _gpu(r, list(SS.NAMES) + ["uv"])
    want = SS.resolve(scene, r.read_visibility(), r.read_cmds(r.last_frame_cmds()), view, iv, r.width, r.height)
    for n in SS.NAMES:
        assert np.array_equal(got[n], np.ascontiguousarray(want[n]).view(np.uint32)), n
    r.upload_material_textures(scene)                 # with the data: kept, and the same frame resolves
    _check(r, scene, view, iv, "after the refused upload")
    r.close()


def test_frames_are_untouched(gpu):
    """The visibility words are identical with and without upload_material_textures between upload and frame."""
    scene, cam, view, iv = H.setup_scene(scenes.material_test_scene, 320, 200)
    a = _renderer(scene, view, iv, cam.width, cam.height, textures=True)
    b = _renderer(scene, view, iv, cam.width, cam.height, textures=False)
    for frame in range(2):
        a.render_frame(); b.render_frame()
        H.assert_vis_equal(a.read_visibility(), b.read_visibility(), cam.width, cam.height, "frame %d" % frame)
        _gpu(a, list(SM.NAMES))                       # (a resolve between frames leaves the next frame alone)
    a.close(); b.close()
