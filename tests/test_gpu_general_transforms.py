"""Every implementation of the per-object arithmetic under general object and camera transforms, bit for bit against the oracle (and
the numpy resolve specs): objects tilted about three axes, stretched non-uniformly, mirrored, instanced at several sizes, moving
between the frames (rotating, translating, rescaling, coming out from behind an occluder and going behind it, entering the
frustum), under cameras that are rolled, turn between frames and change fovy, near plane and jitter.
tests/test_general_transforms.py holds the anchor (oracle against spec_np on the same inputs) and the conditions that keep these
cases from being vacuous.  No tolerances anywhere."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import orc
import spec_resolve_np as SR
import spec_surface_np as SS
from chord_amd import records as R, scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(640, 360), (1237, 701)]


def _scene(w, h, masked=False, attributes=False):
    scene, cam, _ = scenes.general_transform_scene(w, h, masked=masked, attributes=attributes)
    return scene, scenes.general_cameras(cam)


def _renderer(scene, w, h, cull_mode=0):
    from chord_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(0)
    if cull_mode:
        r.set_cull_mode(cull_mode)
    r.upload_scene(scene)
    r.allocate_gbuffer(w, h)
    return r


def _check_frame(r, want, w, h, what, with_stats=True):
    """test_gpu_cull_paths._check_frame: image, list 0 as an array, the four stage counts, trianglesSubmitted, the three chains."""
    H.assert_vis_equal(r.read_visibility(), want["vis"], w, h, what)
    got = r.read_cmds(r.last_frame_cmds())
    if not np.array_equal(got, want["cmds"]):
        n = min(len(got), len(want["cmds"]))
        bad = np.nonzero(got[:n] != want["cmds"][:n])[0]
        raise AssertionError("%s: list 0 (%d vs %d commands), first difference at %s: got %s want %s" % (
            what, len(got), len(want["cmds"]), bad[:1], got[bad[:1]], want["cmds"][bad[:1]]))
    if not with_stats:
        return None
    st = r.stats()
    counts = [st["countInstanceCulled"], st["countStage0Visible"], st["countStage0Rejected"], st["countStage1Visible"]]
    assert counts == [int(c) for c in want["counts"]], "%s: stage counts %s, oracle %s" % (what, counts, list(want["counts"]))
    assert st["trianglesSubmitted"] == want["stats"].trianglesSubmitted, what
    assert st["overflow"] == 0, what
    mn, mx, rng = r.read_hzb(r.history_hzb())
    assert np.array_equal(mn, want["hzb_min"]), what + ": history HZB min"
    assert np.array_equal(mx, want["hzb_max"]), what + ": history HZB max"
    assert np.array_equal(rng, want["valid_range"]), what + ": history valid range"
    return st


def run_moving_frames(w, h, masked=False, cull_mode=0, scene_cams=None, what="general"):
    """The moving sequence through chordvis_render_frame on a fresh context, every frame against the oracle (frame 0's stats are
    not read: frame 1 is to carry its HZB tail).  Returns {"wide": per frame, whether the second raster pass was set up by the wide
    kernel; "launches": kernelLaunches of frames 1..}."""
    from chord_amd import lib as L
    scene, cams = scene_cams or _scene(w, h, masked)
    r = _renderer(scene, w, h, cull_mode)
    wide, launches = [], []
    try:
        for k, view, iv, want in H.moving_sequence(scene, cams):
            r.update_objects(scene.objects)
            r.set_view(view, iv, H.ALL_FLAGS)
            r.render_frame()
            st = _check_frame(r, want, w, h, "%s %dx%d masked=%s mode %d frame %d" % (what, w, h, masked, cull_mode, k), with_stats=k > 0)
            if st is not None:
                launches.append(st["kernelLaunches"])
            kernels = (C.c_uint32 * 2)()
            assert L.lib.chordvis_debug_setup_kernels(r._ctx, kernels) == 0
            wide.append(int(kernels[1]) if k and want["counts"][3] else 0)
    finally:
        r.close()
    return {"wide": wide, "launches": launches}


# ---- stand-alone instance cull ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_instance_culling_of_every_camera_matches_oracle(gpu, w, h, masked):
    scene, cams = _scene(w, h, masked)
    for mode in (0, 1):                                                    # flat dispatch, hierarchical (BVH) cull
        r = _renderer(scene, w, h, mode)
        prev = None
        for k in range(len(cams)):
            view, iv = H.moving_frame(scene, cams, k, prev)
            prev = view
            r.update_objects(scene.objects)
            for flags in (H.ALL_FLAGS, R.FLAG_FRUSTUM_CULL):
                r.set_view(view, iv, flags)
                got = r.read_cmds(r.instance_culling())
                want = orc.instance_culling(scene, view, iv, flags)
                assert len(want) > 0 and np.array_equal(got, want), "camera %d mode %d flags %d: %d vs %d commands" % (k, mode, flags, len(got), len(want))
        r.close()


# ---- chordvis_render_frame on the moving sequence ---------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_moving_frames_on_the_fused_path_match_oracle(gpu, w, h, masked):
    wide = run_moving_frames(w, h, masked)["wide"]
    # "at least one of the moving frames" is asked of one case only, on purpose: whether a later pass counts as light depends on the
    # size and on the alpha test, and the other cases are not there to pin that threshold (tests/test_gpu_setup_wide.py does)
    if (w, h) == SIZES[0] and not masked:
        assert any(wide), "a moving frame set its second pass up with the wide kernel: %s" % wide


@pytest.mark.parametrize("w,h", SIZES)
def test_moving_frames_with_the_hierarchical_cull_match_oracle(gpu, w, h):
    run_moving_frames(w, h, cull_mode=1)


def _child_main():
    """In a child interpreter (CHORDVIS_CULL_FUSED=0 or CHORDVIS_SETUP_WIDE=0, read once per process): the same sequences."""
    out = {"%dx%d" % s: run_moving_frames(*s) for s in SIZES}
    out["masked"] = run_moving_frames(*SIZES[0], masked=True)
    print(json.dumps(out))


def _run_child(var):
    env = dict(os.environ)
    env[var] = "0"
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_general_transforms as T; T._child_main()" % (ROOT, os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, "child (%s=0) failed:\n%s\n%s" % (var, out.stdout[-2000:], out.stderr[-4000:])
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_moving_frames_on_the_three_launch_path_match_oracle(gpu):
    """CHORDVIS_CULL_FUSED=0 in a fresh interpreter: count + scatter + phase-0 cull, to the same oracle frames.  That the two
    processes really took different paths shows in the launch counts of the frames with a history, as in
    tests/test_gpu_cull_paths.py::test_three_launch_path_on_the_fused_size_scenes: this process fuses them into fewer launches."""
    unfused = _run_child("CHORDVIS_CULL_FUSED")
    for key, size, masked in [("%dx%d" % s, s, False) for s in SIZES] + [("masked", SIZES[0], True)]:
        fused = run_moving_frames(*size, masked=masked)["launches"]
        there = unfused[key]["launches"]
        assert len(fused) == len(there) == 3 and all(a < b for a, b in zip(fused, there)), (key, fused, there)


def test_moving_frames_without_the_wide_setup_match_oracle(gpu):
    got = _run_child("CHORDVIS_SETUP_WIDE")
    assert not any(any(v["wide"]) for v in got.values()), got


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_moving_frames_pass_by_pass_match_oracle(gpu, masked):
    """test_individual_passes_compose_to_the_frame on the moving sequence: the caller carries the history chain."""
    w, h = SIZES[0]
    scene, cams = _scene(w, h, masked)
    r = _renderer(scene, w, h)
    hist = None
    for k, view, iv, want in H.moving_sequence(scene, cams):
        r.update_objects(scene.objects)
        r.set_view(view, iv, H.ALL_FLAGS)
        r.clear_gbuffer()
        post = r.instance_culling()
        stage1, rejected = r.visibility_stage0(hist, post)
        assert stage1 == (hist is not None)
        if stage1:
            r.visibility_stage1(r.build_hzb(True, False, False, slot=0), rejected)
        hist = r.build_hzb(True, True, True, slot=1 + (k & 1))
        H.assert_vis_equal(r.read_visibility(), want["vis"], w, h, "pass-by-pass frame %d" % k)
        mn, mx, rng = r.read_hzb(hist)
        d = want["desc"]
        for l in range(d.mipCount):
            vw, vh = d.valid_dims(l)
            mw, _ = d.mip_dims(l)
            o = d.mipOffset[l]
            for arr, ref in ((mn, want["hzb_min"]), (mx, want["hzb_max"])):
                a = arr[o:o + mw * max(1, d.height >> l)].reshape(-1, mw)[:vh, :vw]
                b = ref[o:o + mw * max(1, d.height >> l)].reshape(-1, mw)[:vh, :vw]
                assert np.array_equal(a, b), (k, l)
        assert np.array_equal(rng, want["valid_range"])
        assert np.array_equal(r.read_cmds(post), want["cmds"])
    assert r.stats()["overflow"] == 0
    r.close()


# ---- the long scene: one thread per group, the stand-alone object cull -----------------------------------------------------------------

def test_long_scene_cull_and_a_moving_two_pass_frame_match_oracle(gpu):
    scene, cam, _ = scenes.general_long_scene()
    assert scene.group_instances > 65536 and -(-scene.group_instances // 256) > 512
    w, h = cam.width, cam.height
    cams = [cam, scenes.general_cameras(cam)[1]]
    r = _renderer(scene, w, h)
    try:
        for k, view, iv, want in H.moving_sequence(scene, cams):
            r.update_objects(scene.objects)
            r.set_view(view, iv, H.ALL_FLAGS)
            got = r.read_cmds(r.instance_culling())
            assert np.array_equal(got, want["cmds"]), "long scene, stand-alone cull %d" % k
            r.render_frame()
            st = _check_frame(r, want, w, h, "long scene frame %d" % k, with_stats=k > 0)
        assert st["countStage0Rejected"] > 0 and st["countStage1Visible"] > 0
    finally:
        r.close()


# ---- sharded frames on one device --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ranks,tile_map,sharded_cull", [(2, "default", True), (3, "checker", False), (3, "rebalance", True),
                                                         (8, "default", True), (8, "rebalance", False)])
def test_sharded_moving_frames_reassemble_to_the_oracle_image(gpu, ranks, tile_map, sharded_cull):
    w, h = SIZES[0]
    scene, cams = _scene(w, h, masked=(ranks == 3))
    view0, iv0 = H.moving_frame(scene, cams, 0)
    ctxs = H.sharded_contexts(scene, view0, iv0, w, h, H.ALL_FLAGS, ranks, tile_map)
    try:
        for k, view, iv, want in H.moving_sequence(scene, cams, frames=3):
            for r in ctxs:
                r.update_objects(scene.objects)
                r.set_view(view, iv, H.ALL_FLAGS)
            H.sharded_frame(ctxs, sharded_cull=sharded_cull)
            for rk, r in enumerate(ctxs):
                H.assert_vis_equal(r.read_visibility(), want["vis"], w, h, "frame %d rank %d of %d" % (k, rk, ranks))
                mn, mx, rng = r.read_hzb(r.history_hzb())
                assert np.array_equal(mn, want["hzb_min"]) and np.array_equal(mx, want["hzb_max"]) and np.array_equal(rng, want["valid_range"])
            single = dict(zip(("countInstanceCulled", "countStage0Visible", "countStage0Rejected", "countStage1Visible"), (int(c) for c in want["counts"])))
            H.assert_rank_counts([r.stats() for r in ctxs], single)
            for r in (ctxs[0], ctxs[-1]):
                assert np.array_equal(r.read_cmds(r.last_frame_cmds()), want["cmds"]), "frame %d: the full command list" % k
            if tile_map == "rebalance":
                before = [r.rebalance() for r in ctxs]
                maps = [r.tile_owners() for r in ctxs]
                assert all(np.array_equal(maps[0], m) for m in maps[1:]) and len(set(before)) == 1
    finally:
        for r in ctxs:
            r.close()


def test_group_of_ranks_renders_the_moving_sequence(gpu):
    """One ChordGroup (every rank a context of device 0) over three moving frames."""
    from chord_amd.renderer import VisibilityGroup
    w, h = SIZES[0]
    scene, cams = _scene(w, h)
    g = VisibilityGroup([0, 0])
    try:
        g.upload_scene(scene)
        g.allocate_gbuffer(w, h)
        for k, view, iv, want in H.moving_sequence(scene, cams, frames=3):
            g.update_objects(scene.objects)
            g.set_view(view, iv, H.ALL_FLAGS)
            g.render_frame()
            g.sync()
            for rk in range(2):
                H.assert_vis_equal(g.ranks[rk].read_visibility(), want["vis"], w, h, "group frame %d rank %d" % (k, rk))
                assert np.array_equal(g.ranks[rk].read_cmds(g.ranks[rk].last_frame_cmds()), want["cmds"])
    finally:
        g.close()


# ---- depth views ---------------------------------------------------------------------------------------------------------------------

def test_depth_views_of_the_moving_general_scene_match_oracle(gpu):
    """Per-view instance cull, the generic HZB cull with the last-frame matrices of moving objects, and the clamp + bias raster of
    cascade views, as tests/test_depth_views.py does on the older scenes."""
    from chord_amd import lib as L
    w, h = SIZES[0]
    scene, cams = _scene(w, h, masked=True)
    view, iv = H.moving_frame(scene, cams, 1, L.make_views(cams[0])[0])
    dim = 256
    cfg = R.default_cascade_config(cascadeCount=3, realtimeCascadeCount=2, cascadeDim=dim, cascadeEndDistance=14.0, farCascadeEndDistance=40.0)
    views = L.cascade_setup(cfg, view, iv, (0.35, -1.0, 0.25))
    campos = np.frombuffer(iv["cameraWorldPos"][0].tobytes(), dtype=np.float64)[:3]
    desc = orc.hzb_desc(dim, dim)
    r = _renderer(scene, w, h)
    try:
        r.update_objects(scene.objects)
        r.set_view(view, iv, H.ALL_FLAGS)
        r.allocate_depth_views(dim, 3)
        r.set_instance_views(views)
        rejected = 0
        for k in range(3):
            post = r.instance_culling_view(k)
            want = orc.instance_culling(scene, view, views[k:k + 1], H.ALL_FLAGS)
            assert len(want) > 0 and np.array_equal(r.read_cmds(post), want), "cascade %d cull" % k
            depth = r.render_mesh_depth(k, post, True, 1.25, 1.75)
            wd, _ = orc.raster_depth(scene, views[k:k + 1], want, dim, dim, True, 1.25, 1.75)
            got = r.read_depth(depth)
            assert np.array_equal(np.asarray(got).view(np.uint32).ravel(), wd.view(np.uint32)), "cascade %d depth" % k
            hzb = r.build_hzb_from_depth(depth)
            _, hmin, _, _ = orc.hzb_build(wd.view(np.uint32).astype(np.uint64) << np.uint64(32), dim, dim)
            for last in (True, False):
                kept = r.read_cmds(r.hzb_culling_generic(hzb, 1.5, k, last, post))
                wk = orc.hzb_culling_generic(scene, views[k:k + 1], campos, H.ALL_FLAGS, 1.5, last, desc, hmin, want)
                assert np.array_equal(H.sort_cmds(kept), H.sort_cmds(wk)), "cascade %d generic cull, last=%s" % (k, last)
                rejected += len(want) - len(wk)
        assert rejected > 0
    finally:
        r.close()


def test_render_shadow_ticks_with_the_cascade_cache_match_the_replay(gpu):
    """chordvis_render_shadow over five ticks of the moving sequence (objects at local_to_world_at(tick), the camera turning every
    tick): the first tick renders every cascade, the later ones the realtime cascades and one far cascade each, first culled against
    the HZB of its own cached depth.  Every cascade's view and depth image against the oracle's replay
    (tests/test_depth_views.py::_replay_shadow), every tick."""
    from test_depth_views import _replay_shadow, LIGHT
    w, h = SIZES[0]
    scene, cam, _ = scenes.general_transform_scene(w, h, masked=True)
    cams = scenes.general_cameras(cam, steps=5)
    cfg = R.default_cascade_config(cascadeCount=5, realtimeCascadeCount=2, cascadeDim=384, cascadeEndDistance=12.0, farCascadeEndDistance=60.0,
                                   shadowBiasConst=-8.0, shadowBiasSlope=-0.5)
    r = _renderer(scene, w, h)
    try:
        hist, prev, masks = None, None, []
        for tick in range(5):
            view, iv = H.moving_frame(scene, cams, tick, prev)
            prev = view
            r.update_objects(scene.objects)
            r.set_view(view, iv, H.ALL_FLAGS)
            depths, views, mask = r.render_shadow(cfg, LIGHT, tick)
            hist, want_mask = _replay_shadow(scene, view, iv, cfg, tick, hist, H.ALL_FLAGS)
            masks.append(mask)
            assert mask == want_mask, "tick %d: rendered cascades %s vs %s" % (tick, bin(mask), bin(want_mask))
            assert np.array_equal(views.view(np.uint8), hist["views"].view(np.uint8)), "tick %d: cascade views" % tick
            for k in range(5):
                got = r.read_depth(depths[k])
                assert np.array_equal(got.view(np.uint32), hist["depths"][k].view(np.uint32)), "tick %d cascade %d" % (tick, k)
                assert np.any(got.view(np.uint32)), "tick %d cascade %d is empty" % (tick, k)
        assert masks[0] == 0b11111 and masks[1:] == [0b00011 | (1 << (2 + t % 3)) for t in range(1, 5)]
    finally:
        r.close()


# ---- resolve ---------------------------------------------------------------------------------------------------------------------------

def _resolved(r, names, desc=None):
    """The targets as numpy arrays.  The tensors are recorded on the context's stream: they are dropped here, before anyone closes
    the context (test_gpu_surface._gpu does the same)."""
    import torch
    out = r.resolve_attributes(names=names, desc=desc)
    torch.cuda.synchronize()
    return {n: t.cpu().numpy().view(np.uint32) for n, t in out.items()}


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_resolve_targets_of_the_moving_frame_equal_the_specs(gpu, masked):
    """Every target of chordvis_resolve_attributes and chordvis_resolve_surface on frames 1 and 2 of the moving sequence (jittered
    views): motion vectors of rotating and rescaling objects, normals under stretch, tangent frames of mirrored objects -- with
    the view's own (jittered) matrices, and with the no-jitter matrices of this frame's camera and of the previous, turned one."""
    from chord_amd import lib as L
    w, h = 333, 201
    scene, cams = _scene(w, h, masked, attributes=True)
    plain = [scenes.Camera(c.position, c.front, c.width, c.height, c.fovy, c.z_near, c.z_far, c.world_up) for c in cams]   # jitter 0
    names = list(L.RESOLVE_CHANNELS) + list(SS.NAMES)

    def same(got, spec, what):
        for n in names:
            wv = np.ascontiguousarray(spec[n]).view(np.uint32).reshape(got[n].shape)
            if not np.array_equal(got[n], wv):
                bad = np.argwhere(got[n] != wv)
                raise AssertionError("%s %s: %d texels differ; first %s got %r want %r" % (
                    what, n, len(bad), bad[0], got[n][tuple(bad[0][:2])].view(np.float32), wv[tuple(bad[0][:2])].view(np.float32)))

    r = _renderer(scene, w, h)
    try:
        view_nj = None
        for k, view, iv, want in H.moving_sequence(scene, cams, frames=3):
            view_nj, _ = L.make_views(plain[k], view_nj)                 # (its last-frame matrix: the previous camera's, without jitter)
            r.update_objects(scene.objects)
            r.set_view(view, iv, H.ALL_FLAGS)
            r.render_frame()
            if not k:
                continue
            H.assert_vis_equal(r.read_visibility(), want["vis"], w, h, "resolve frame %d" % k)
            got = _resolved(r, names)
            spec = SR.resolve(scene, want["vis"], want["cmds"], view, iv, w, h)
            spec.update(SS.resolve(scene, want["vis"], want["cmds"], view, iv, w, h))
            same(got, spec, "frame %d" % k)
            assert np.any(got["motionVector"]) and np.any(got["vertexNormal"])
            vp, vpl = view_nj["translatedWorldToClip"], view_nj["translatedWorldToClipLastFrame"]
            assert not np.array_equal(vp, view["translatedWorldToClip"]) and not np.array_equal(vp, vpl)
            d = L.ResolveDesc()
            d.useNoJitter = 1
            d.translatedWorldToClipNoJitter[:] = [float(v) for v in np.asarray(vp, dtype=np.float32).reshape(16)]
            d.translatedWorldToClipLastFrameNoJitter[:] = [float(v) for v in np.asarray(vpl, dtype=np.float32).reshape(16)]
            got_nj = _resolved(r, names, d)
            spec_nj = SR.resolve(scene, want["vis"], want["cmds"], view, iv, w, h, use_no_jitter=True, vp_nj=vp, vp_last_nj=vpl)
            spec_nj.update({n: spec[n] for n in SS.NAMES})
            same(got_nj, spec_nj, "frame %d, no-jitter matrices" % k)
            assert not np.array_equal(got_nj["motionVector"], got["motionVector"]), "the no-jitter matrices change the motion vectors"
    finally:
        r.close()


# ---- mvp[3][3] == 1.0f under a perspective camera ------------------------------------------------------------------------------------

def test_unit_depth_objects_take_the_oracle_branch(gpu):
    from chord_amd import lib as L
    scene, cam = scenes.unit_depth_scene()
    w, h = cam.width, cam.height
    L.fill_objects(scene, cam)
    view, iv = L.make_views(cam)
    for mode in (0, 1):
        r = _renderer(scene, w, h, mode)
        for flags in (H.ALL_FLAGS, R.FLAG_FRUSTUM_CULL):
            r.set_view(view, iv, flags)
            assert np.array_equal(r.read_cmds(r.instance_culling()), orc.instance_culling(scene, view, iv, flags)), (mode, flags)
        r.set_view(view, iv, H.ALL_FLAGS)
        prev = None
        for k in range(2):
            want = orc.frame(scene, view, iv, H.ALL_FLAGS, prev_hzb_min=prev)
            r.render_frame()
            _check_frame(r, want, w, h, "unit depth mode %d frame %d" % (mode, k), with_stats=k > 0)
            prev = want["hzb_min"]
        r.close()
    ctxs = H.sharded_contexts(scene, view, iv, w, h, H.ALL_FLAGS, 2)
    prev = None
    for k in range(2):
        want = orc.frame(scene, view, iv, H.ALL_FLAGS, prev_hzb_min=prev)
        H.sharded_frame(ctxs, sharded_cull=True)
        for rk, r in enumerate(ctxs):
            H.assert_vis_equal(r.read_visibility(), want["vis"], w, h, "unit depth, 2 ranks, frame %d rank %d" % (k, rk))
            assert np.array_equal(r.read_cmds(r.last_frame_cmds()), want["cmds"])
        prev = want["hzb_min"]
    for r in ctxs:
        r.close()


# ---- the full-size case ----------------------------------------------------------------------------------------------------------------

def test_config3_street_general_4k_two_moving_frames_match_oracle(gpu):
    scene, cam, _ = scenes.config3_street_general()
    w, h = cam.width, cam.height
    cams = [cam, scenes.general_cameras(cam)[1]]
    r = _renderer(scene, w, h)
    try:
        for k, view, iv, want in H.moving_sequence(scene, cams):
            r.update_objects(scene.objects)
            r.set_view(view, iv, H.ALL_FLAGS)
            r.render_frame()
            st = _check_frame(r, want, w, h, "street general 4K frame %d" % k, with_stats=k > 0)
        assert st["countStage0Rejected"] > 0 and st["countStage1Visible"] > 0 and st["countStage0Visible"] > 1000
    finally:
        r.close()
