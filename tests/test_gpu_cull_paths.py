"""Every cull path that can open a frame of chordvis_render_frame, held to the oracle on both sides of the host's thresholds, on
an empty group list, and on history chains the library did not build itself.

launch_group_cull picks the path from the group-instance count: frame_cull_fused_kernel (object pass, group cull, phase-0 HZB cull
and list placement in one launch), the quad group_cull_count_kernel + scatter (+ hzb_cull_kernel<0> in a frame with a history),
or object_cull_kernel + count + self-summing scatter.  Each case runs a short sequence on one context against orc.frame:
frame 0 (no history), frame 1 (camera moved; carries frame 0's pending HZB tail), then -- stats() having flushed frame 1's tail
-- frame 2 (camera moved again; a history and no pending tail)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import orc
from chord_amd import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the host's thresholds, mirrored (chord_amd/csrc/kernels_cull.hip unless said otherwise) ---------------------------------------
FUSED_CULL_THREADS = 256            # :945  threads of a fused workgroup
FUSED_CULL_GROUPS = 64              # :947  FUSED_CULL_THREADS / 4: group instances per fused workgroup
FUSED_CULL_MAX_BLOCKS = 1024        # :948  look-back words
QUAD_CULL_MAX_BLOCKS = 512          # :1620, :1631  past it, object_cull_kernel opens the frame (count + self-summing scatter)
CULL_SELFSUM_MAX_BLOCKS = 4096      # :1187 past it, group_cull_prefix_kernel as well (BASELINE config 5 sits there)
COUNT_BLOCK_GROUPS = 256            # chordvis_abi.cpp upload_scene_impl  cullBlocks = max(1, ceil(groupInstances / 256))
# (the fused path's last condition, the HZB tail in HZB_TAIL_FLOATS (:706), holds for every target of this module)


def cull_blocks(groups):
    return max(1, -(-groups // COUNT_BLOCK_GROUPS))


def takes_fused(groups, objects, num_cus):
    """launch_group_cull's test (:1615-1627) for a flat, unsharded frame of chordvis_render_frame with the library's own history."""
    fblocks = max(1, -(-groups // FUSED_CULL_GROUPS))
    fobj = -(-objects // FUSED_CULL_THREADS)
    return (fblocks + 1 + fobj <= num_cus * (1024 // FUSED_CULL_THREADS) and fblocks <= FUSED_CULL_MAX_BLOCKS
            and cull_blocks(groups) <= QUAD_CULL_MAX_BLOCKS)


def scene_objects(groups, panels=True):
    """Objects of scenes.group_count_scene(groups)."""
    return groups // 64 + groups % 64 if groups > 256 and panels else groups


def num_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def largest_fused(cus):
    g = FUSED_CULL_GROUPS * min(FUSED_CULL_MAX_BLOCKS, cus * (1024 // FUSED_CULL_THREADS))
    while not takes_fused(g, scene_objects(g), cus):
        g -= 1
    return g


MOVES = [(0.15, 0.05, -0.1), (0.1, -0.05, -0.15)]


def _renderer(scene, w, h):
    from chord_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(0)
    r.upload_scene(scene)
    r.allocate_gbuffer(w, h)
    return r


def _check_frame(r, scene, want, w, h, what, with_stats=True):
    """The image and list 0 (as an array: its slot order is deterministic on every path); with_stats: also the four stage counts,
    the triangles, overflow and the history chain -- reading those flushes a pending HZB tail."""
    H.assert_vis_equal(r.read_visibility(), want["vis"], w, h, what)
    got = r.read_cmds(r.last_frame_cmds())
    assert np.array_equal(got, want["cmds"]), "%s: list 0 (%d vs %d commands)" % (what, len(got), len(want["cmds"]))
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


def run_sequence(groups, w=320, h=180, flags=H.ALL_FLAGS, panels=True):
    """Frames 0, 1, 2 of one case on a fresh context, each against the oracle; returns kernelLaunches of frames 1 and 2."""
    from chord_amd import lib as L
    scene, cam = scenes.group_count_scene(groups, w, h, panels=panels)
    assert scene.group_instances == groups
    r = _renderer(scene, w, h)
    try:
        prev_view, prev_cam, prev_hzb, launches = None, None, None, []
        for k in range(3):
            if k:
                cam = cam.moved(MOVES[k - 1])
            L.fill_objects(scene, cam, prev_cam)
            view, iv = L.make_views(cam, prev_view)
            r.update_objects(scene.objects)
            r.set_view(view, iv, flags)
            want = orc.frame(scene, view, iv, flags, prev_hzb_min=prev_hzb)
            r.render_frame()
            # frame 0: its stats and chain are not read, which would flush the HZB tail frame 1 is to carry
            st = _check_frame(r, scene, want, w, h, "%d groups, frame %d" % (groups, k), with_stats=k > 0)
            if st is not None:
                launches.append(st["kernelLaunches"])
            prev_view, prev_cam, prev_hzb = view, cam, want["hzb_min"]
        return launches
    finally:
        r.close()


SMALL = [1, 63, 64, 65]          # one fused workgroup, the first / last lane of it, the second workgroup and its tc clamp


@pytest.mark.parametrize("groups", SMALL)
def test_short_scenes_on_the_fused_path_match_the_oracle(gpu, groups):
    assert takes_fused(groups, scene_objects(groups), num_cus())
    run_sequence(groups)


def test_either_side_of_the_fused_limit(gpu):
    """The largest group-instance count the fused kernel takes (its grid: one look-back slot per workgroup, plus the tail and
    object workgroups, at most four per CU) and one more."""
    cus = num_cus()
    g = largest_fused(cus)
    assert takes_fused(g, scene_objects(g), cus) and not takes_fused(g + 1, scene_objects(g + 1), cus)
    fused = run_sequence(g)
    quad = run_sequence(g + 1)
    # frames 1 and 2: one launch against count + scatter + phase-0 cull -- if a threshold moves, this case lost its point
    assert all(a < b for a, b in zip(fused, quad)), (g, fused, quad)


def test_either_side_of_the_quad_count_limit(gpu):
    """512 count blocks (the quad count kernel, which the fused path's grid limit has long left behind) and 513 (object_cull_kernel
    + count + self-summing scatter)."""
    g = QUAD_CULL_MAX_BLOCKS * COUNT_BLOCK_GROUPS
    assert cull_blocks(g) == QUAD_CULL_MAX_BLOCKS and cull_blocks(g + 1) == QUAD_CULL_MAX_BLOCKS + 1 <= CULL_SELFSUM_MAX_BLOCKS
    assert not takes_fused(g, scene_objects(g), num_cus())
    quad = run_sequence(g)
    selfsum = run_sequence(g + 1)
    assert all(a < b for a, b in zip(quad, selfsum)), (quad, selfsum)       # (object_cull_kernel in front of the count)


def test_empty_group_list_after_a_full_scene(gpu):
    """A scene whose primitives have no cluster groups, uploaded over one that has: the frame still zeroes its counters, publishes
    its view and writes the list counts (all zero) -- also the second frame, which carries the first one's HZB tail -- and the
    non-empty scene uploaded again renders as before."""
    from chord_amd import lib as L
    w, h = 320, 180
    full, cam = scenes.group_count_scene(65, w, h)
    empty = H.without_groups(full)
    assert empty.group_instances == 0
    L.fill_objects(full, cam)
    view, iv = L.make_views(cam)
    want = orc.frame(full, view, iv, H.ALL_FLAGS)
    assert want["counts"][0] > 0
    r = _renderer(full, w, h)
    try:
        r.set_view(view, iv, H.ALL_FLAGS)
        r.render_frame()
        _check_frame(r, full, want, w, h, "full scene")
        L.fill_objects(empty, cam)
        r.upload_scene(empty)
        r.set_view(view, iv, H.ALL_FLAGS)
        nothing = orc.frame(empty, view, iv, H.ALL_FLAGS)
        assert not nothing["vis"].any() and not nothing["counts"].any()
        r.render_frame()
        _check_frame(r, empty, nothing, w, h, "empty scene, frame 0", with_stats=False)
        r.render_frame()                                    # (a history, and frame 0's tail pending)
        nothing1 = orc.frame(empty, view, iv, H.ALL_FLAGS, prev_hzb_min=nothing["hzb_min"])
        st = _check_frame(r, empty, nothing1, w, h, "empty scene, frame 1")
        assert st["trianglesSubmitted"] == 0 and st["countInstanceCulled"] == 0
        r.upload_scene(full)
        r.set_view(view, iv, H.ALL_FLAGS)
        r.render_frame()
        _check_frame(r, full, want, w, h, "full scene again")
        r.render_frame()
        _check_frame(r, full, orc.frame(full, view, iv, H.ALL_FLAGS, prev_hzb_min=want["hzb_min"]), w, h, "full scene again, frame 1")
    finally:
        r.close()


def uploaded_chain_case(groups, panels=True):
    """Chains handed in through chordvis_upload_history_hzb: (i) the oracle's chain of another view, (ii) the same with levels 6..
    all 1.0 -- not the 2x2 min of level 5.  Each is uploaded, a frame rendered against it and held to orc.frame with that chain;
    a frame after it runs on the library's own chain.  Returns kernelLaunches of (frame on (ii), the frame after it)."""
    from chord_amd import lib as L
    w, h = 640, 360
    scene, _ = scenes.group_count_scene(groups, w, h, panels=panels)
    chain_i, view, iv = H.close_view_chain(scene)
    desc = orc.hzb_desc(w, h)
    chain_ii = H.hzb_with_upper_levels(desc, chain_i, 0x3C00)
    # the case has teeth: the oracle tells (ii) from (ii) with levels 6.. recomputed, i.e. from what the fused kernel used to cull against
    a = orc.frame(scene, view, iv, H.ALL_FLAGS, prev_hzb_min=chain_ii)["counts"]
    b = orc.frame(scene, view, iv, H.ALL_FLAGS, prev_hzb_min=H.hzb_with_upper_levels(desc, chain_ii))["counts"]
    assert list(a) != list(b), (a, b)
    r = _renderer(scene, w, h)
    try:
        r.update_objects(scene.objects)
        r.set_view(view, iv, H.ALL_FLAGS)
        launches = []
        for name, chain in (("(i)", chain_i), ("(ii)", chain_ii)):
            r.upload_history_hzb(chain)
            want = orc.frame(scene, view, iv, H.ALL_FLAGS, prev_hzb_min=chain)
            r.render_frame()
            st = _check_frame(r, scene, want, w, h, "%d groups, uploaded chain %s" % (groups, name))
            launches = [st["kernelLaunches"]]
        r.render_frame()                                     # the library's own chain again (same view)
        st = _check_frame(r, scene, orc.frame(scene, view, iv, H.ALL_FLAGS, prev_hzb_min=want["hzb_min"]), w, h,
                          "%d groups, the frame after the uploaded chain" % groups)
        return launches + [st["kernelLaunches"]]
    finally:
        r.close()


def test_uploaded_history_chain_on_the_fused_size_scene(gpu):
    assert takes_fused(64, scene_objects(64), num_cus())
    uploaded, after = uploaded_chain_case(64)
    assert after < uploaded, (uploaded, after)               # the uploaded chain's frame takes the three launches, the next one fuses


def test_uploaded_history_chain_past_the_fused_limit(gpu):
    cus = num_cus()
    g = largest_fused(cus) + 1
    assert not takes_fused(g, g, cus)                        # (one object per group instance: further past the limit still)
    uploaded_chain_case(g, panels=False)


def _child_main():
    """Run in a child interpreter with CHORDVIS_CULL_FUSED=0 (read once per process): the fused-size cases and the uploaded chains on
    the three-launch path, against the oracle.  Prints {"launches": {groups: [frame 1, frame 2]}}; a failure exits non-zero."""
    out = {str(g): run_sequence(g) for g in SMALL}
    uploaded_chain_case(64)
    print(json.dumps({"launches": out}))


def test_three_launch_path_on_the_fused_size_scenes(gpu):
    """CHORDVIS_CULL_FUSED=0 in a fresh interpreter: the same short scenes and uploaded chains take count + scatter + phase-0 cull,
    with the same results (list 0 in the same order); in this process they take the fused kernel, in fewer launches."""
    env = dict(os.environ)
    env["CHORDVIS_CULL_FUSED"] = "0"
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_cull_paths as T; T._child_main()" % (ROOT, os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, "child (CHORDVIS_CULL_FUSED=0) failed:\n%s\n%s" % (out.stdout[-2000:], out.stderr[-4000:])
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    unfused = json.loads(lines[0])["launches"]
    for g in SMALL:
        fused = run_sequence(g)
        assert all(a < b for a, b in zip(fused, unfused[str(g)])), (g, fused, unfused[str(g)])
