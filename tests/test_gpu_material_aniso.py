"""chordvis_resolve_material under chordvis_set_material_anisotropy on the GPU, through the C ABI: the four material images held bit
for bit (uint32 views) against tests/spec_material_aniso_np.py at N = 2, 8 and 16; the setting switched back and forth on one
context; a sharded rank; subsets; refusals; frames and the eleven earlier images untouched by the setting."""
import ctypes as C

import numpy as np
import pytest

from chord_amd import scenes

import helpers as H
import spec_material_aniso_np as SA
import spec_material_np as SM

pytestmark = pytest.mark.gpu


def _renderer(scene, view, iv, w, h, n=None):
    from chord_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(0)
    if n is not None:
        r.set_material_anisotropy(n)                  # (before the uploads: the setting survives them)
    r.upload_scene(scene)
    r.upload_material_textures()
    r.allocate_gbuffer(w, h)
    r.set_view(view, iv, H.ALL_FLAGS)
    return r


def _gpu(r, names):
    out = r.resolve_attributes(names=names)
    import torch
    torch.cuda.synchronize()
    return {n: t.cpu().numpy().view(np.uint32) for n, t in out.items()}


def _equal(got, want, what, names=SM.NAMES):
    for n in names:
        wv = np.ascontiguousarray(want[n]).view(np.uint32)
        if not np.array_equal(got[n], wv):
            bad = np.argwhere(got[n] != wv)
            raise AssertionError("%s %s: %d texels differ; first %s got %r want %r" % (what, n, len(bad), bad[0],
                                 got[n][tuple(bad[0][:2])].view(np.float32), wv[tuple(bad[0][:2])].view(np.float32)))


class _Frame:
    """the spec's inputs of the frame a renderer holds, read back once and shared by the settings compared on it"""

    def __init__(self, r, scene, view, iv):
        self.args = (scene, r.read_visibility(), r.read_cmds(r.last_frame_cmds()), view, iv, r.width, r.height)
        self.surface = SM.SS.resolve(*self.args)

    def want(self, n):
        return SA.resolve(*self.args, surface=self.surface, max_aniso=n)


SCENES = [("material", (320, 200)), ("material_odd", (333, 201))]


@pytest.mark.parametrize("n", [2, 8, 16])
@pytest.mark.parametrize("name,size", SCENES, ids=[s[0] for s in SCENES])
def test_material_equals_the_spec(gpu, name, size, n):
    scene, cam, view, iv = H.setup_scene(scenes.material_test_scene, *size)
    r = _renderer(scene, view, iv, cam.width, cam.height, n=n)
    assert r.material_anisotropy() == n
    for frame in range(2):                               # frame 0: no history; frame 1: two-pass HZB
        r.render_frame()
        fr = _Frame(r, scene, view, iv)
        hit = ((fr.args[1] & np.uint64(0xFFFFFFFF)) != 0).reshape(cam.height, cam.width)
        assert hit.sum() > 0.2 * cam.width * cam.height
        got = _gpu(r, list(SM.NAMES))
        _equal(got, fr.want(n), "%s frame %d N = %d" % (name, frame, n))
        for img in SM.NAMES:
            assert not np.any(got[img][~hit]), img
            assert not np.any(np.isnan(got[img].view(np.float32))), img
        assert np.any(got["baseColor"][hit]) and np.any(got["pixelNormal"][hit])
    r.close()


def test_general_transforms_over_moving_cameras(gpu):
    """Mirrored and stretched objects, camera and objects in motion, at N = 8."""
    scene, cam0, _ = scenes.general_transform_scene(320, 180, materials=True)
    cams = scenes.general_cameras(cam0, 3)
    view, iv = H.moving_frame(scene, cams, 0)
    r = _renderer(scene, view, iv, cam0.width, cam0.height, n=8)
    for k in range(len(cams)):
        if k:
            view, iv = H.moving_frame(scene, cams, k, view)
            r.update_objects(scene.objects)
            r.set_view(view, iv, H.ALL_FLAGS)
        r.render_frame()
        _equal(_gpu(r, list(SM.NAMES)), _Frame(r, scene, view, iv).want(8), "view %d" % k)
    r.close()


def test_switching_the_setting_and_subsets(gpu):
    """One context at N = 8, 1, 8: N = 1 is the isotropic spec (spec_material_np), the two N = 8 runs are equal, the eleven earlier
    images are the same at every N, and a subset of the material targets at N = 8 equals its planes of the full run."""
    from chord_amd import lib as L
    scene, cam, view, iv = H.setup_scene(scenes.material_test_scene, 320, 200)
    r = _renderer(scene, view, iv, cam.width, cam.height)
    assert r.material_anisotropy() == 1
    r.render_frame()
    r.render_frame()
    fr = _Frame(r, scene, view, iv)
    eleven = list(L.RESOLVE_CHANNELS) + list(L.SURFACE_CHANNELS)
    everything = eleven + list(SM.NAMES)
    r.set_material_anisotropy(8)
    first = _gpu(r, everything)
    r.set_material_anisotropy(1)
    one = _gpu(r, everything)
    r.set_material_anisotropy(8)
    second = _gpu(r, everything)
    _equal(one, SM.resolve(*fr.args, surface=fr.surface), "N = 1 after N = 8")
    _equal(first, fr.want(8), "N = 8")
    for n in everything:
        assert np.array_equal(first[n], second[n]), n
    for n in eleven:
        assert np.array_equal(first[n], one[n]), n
    alone = _gpu(r, eleven)                                 # (chordvis_resolve_surface: does not read the setting)
    for n in eleven:
        assert np.array_equal(alone[n], first[n]), n
    assert any(not np.array_equal(first[n], one[n]) for n in SM.NAMES)
    for names in (["baseColor"], ["emissive", "roughMetalAO"], ["pixelNormal"], ["baseColor", "pixelNormal", "roughMetalAO"]):
        sub = _gpu(r, names)
        assert sorted(sub) == sorted(names)
        for n in names:
            assert np.array_equal(sub[n], first[n]), (names, n)
    r.close()


def test_sharded_rank_equals_the_single_context(gpu):
    """Two ranks of a sharded frame on one device (the all-gathers replaced by copies, as in test_gpu_material.py): each rank sets
    N = 8 itself and resolves the four images as the single context does."""
    from chord_amd import lib as L
    from chord_amd.renderer import VisibilityRenderer
    scene, cam, view, iv = H.setup_scene(scenes.material_test_scene, 320, 200)
    w, h, ranks = cam.width, cam.height, 2
    ref = _renderer(scene, view, iv, w, h, n=8)
    ctxs = []
    for rk in range(ranks):
        r = VisibilityRenderer(0)
        r.upload_scene(scene)
        r.upload_material_textures()
        r.set_shard(ranks, rk)
        r.allocate_gbuffer(w, h)
        r.set_view(view, iv, H.ALL_FLAGS)
        r.set_material_anisotropy(8)
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
    want = _gpu(ref, list(SM.NAMES))
    _equal(want, _Frame(ref, scene, view, iv).want(8), "single context")
    for rk, r in enumerate(ctxs):
        H.assert_vis_equal(r.read_visibility(), ref.read_visibility(), w, h, "rank %d" % rk)
        got = _gpu(r, list(SM.NAMES))
        for n in SM.NAMES:
            assert np.array_equal(got[n], want[n]), (rk, n)
    for r in ctxs + [ref]:
        r.close()


def test_refusals_and_untouched_frames(gpu):
    from chord_amd import lib as L
    scene, cam, view, iv = H.setup_scene(scenes.material_test_scene, 320, 200)
    r = _renderer(scene, view, iv, cam.width, cam.height)
    before = []
    for frame in range(2):
        r.render_frame()
        before.append(r.read_visibility().copy())
    r.set_material_anisotropy(4)
    for bad in (0, 3, 32):
        with pytest.raises(L.ChordvisError, match="1 .off., 2, 4, 8 or 16"):
            r.set_material_anisotropy(bad)
        assert L.lib.chordvis_set_material_anisotropy(r._ctx, bad) == L.E_INVALID
        assert b"2, 4, 8 or 16" in L.lib.chordvis_last_error(r._ctx)
        assert r.material_anisotropy() == 4, "the getter returns the last accepted value"
    r.set_material_anisotropy(16)
    assert r.material_anisotropy() == 16
    r.upload_scene(scene)                                 # the setting survives both uploads
    r.upload_material_textures()
    r.allocate_gbuffer(cam.width, cam.height)
    r.set_view(view, iv, H.ALL_FLAGS)
    assert r.material_anisotropy() == 16
    for frame in range(2):
        r.render_frame()
        H.assert_vis_equal(r.read_visibility(), before[frame], cam.width, cam.height, "frame %d at N = 16" % frame)
        _gpu(r, list(SM.NAMES))                           # (a resolve between frames leaves the next frame alone)
    _equal(_gpu(r, list(SM.NAMES)), _Frame(r, scene, view, iv).want(16), "N = 16 after the uploads")
    r.close()
