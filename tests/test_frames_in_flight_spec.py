"""What makes tests/test_gpu_frames_in_flight.py non-vacuous, from the oracle alone (no GPU): in every scenario the state a
misordered call would see gives ANOTHER expected output than the state it should see -- the comparisons on the GPU are exact, so
'differ' is the whole condition -- and the frames that are there to meet a stale host decision really are what that decision is
about (a heavy second pass, a dense list).  The scenarios come from tests/inflight.py, cached per process, so both files share
one set of oracle frames."""
import numpy as np
import pytest

import inflight as F

TILE_DIRECT_MAX_CLUSTERS = 1024            # chord_amd/csrc/raster_params.h


def _differ(a, b):
    return not np.array_equal(a["vis"], b["vis"])


@pytest.mark.parametrize("name", ["cut", "sky", "masked_floor"])
def test_adjacent_frames_of_the_report_sequences_differ(name):
    sc = F.wide_sequence(name)
    for k in range(len(sc.frames) - 1):
        a, b = sc.frames[k], sc.frames[k + 1]
        if name == "sky" and k == 2:
            # frames 2 and 3 look up from one place: the same image by construction; what a frame skipped or doubled changes is the
            # second pass -- frame 2 culls against a street view's chain, frame 3 against the sky view's own
            assert not _differ(a.want, b.want)
            assert a.want["counts"].tolist() != b.want["counts"].tolist()
            continue
        assert _differ(a.want, b.want), (name, k)
        # (a camera that only translates keeps its view record -- matrices relative to the camera --: position and motion are in the
        # objects' and the instance view's records)
        assert not np.array_equal(a.objs, b.objs) and a.iv.tobytes() != b.iv.tobytes(), (name, k)


def test_cut_has_two_heavy_second_passes_between_light_ones():
    """Frames 3 and 4 send the scene through the second pass (more clusters than the direct form's limit), frames 1, 2, 5 and 6 do
    not: a host that has seen 'light' meets heavy passes, and one that has seen 'heavy' meets light ones."""
    counts = [int(f.want["counts"][3]) for f in F.wide_sequence("cut").frames]
    assert len(counts) == 7
    assert all(counts[k] > TILE_DIRECT_MAX_CLUSTERS for k in (3, 4)), counts
    assert all(counts[k] <= TILE_DIRECT_MAX_CLUSTERS for k in (1, 2, 5, 6)), counts
    assert all(counts[k] > 0 for k in (1, 2, 5, 6)), counts                  # (light, not empty: the wide kernel has clusters to set up)


def test_sky_and_masked_floor_have_a_light_second_pass_after_the_gate():
    sky = [int(f.want["counts"][3]) for f in F.wide_sequence("sky").frames]
    assert sky[3] == 0 and sky[4] > TILE_DIRECT_MAX_CLUSTERS and 0 < sky[1] <= TILE_DIRECT_MAX_CLUSTERS, sky
    floor = [int(f.want["counts"][3]) for f in F.wide_sequence("masked_floor").frames]
    assert 0 < floor[2] <= TILE_DIRECT_MAX_CLUSTERS, floor


@pytest.mark.parametrize("order", sorted(F.HOTSPOT_ORDERS))
def test_hotspot_frames_are_dense_and_the_view_away_is_not(order):
    """launch_raster's rule for eliding the block kernel: the last report's cluster count x 32 below the pixel count; the device's
    rule for a dense list (launch_is_dense): a cluster per 16 pixels."""
    sc = F.hotspot(order)
    pixels = sc.w * sc.h
    letters = F.HOTSPOT_ORDERS[order]
    for k, (ch, f) in enumerate(zip(letters, sc.frames)):
        n = len(f.want["cmds"])
        assert (n * 32 >= pixels) == (ch == "h") and (n * 16 >= pixels) == (ch == "h"), (order, k, n, pixels)
        assert f.want["vis"].any() == (ch == "h"), (order, k)
    if order in F.HOTSPOT_SCENES:
        # the hot-tile scene: more clusters than SLOT_HOT (65 536), all drawn inside the block of 2 x 2 tiles round the target's centre
        # (sigma 8 px round the middle of a tile), and too many triangles for the record form of one tile -- block-form frames only
        hot = next(f for ch, f in zip(letters, sc.frames) if ch == "h")
        assert len(hot.want["cmds"]) > 65536 + 8192
        ys, xs = np.nonzero((hot.want["vis"] & np.uint64(0xFFFFFFFF)).reshape(sc.h, sc.w))
        assert xs.max() - xs.min() < 128 and ys.max() - ys.min() < 128 and (sc.w // 2) % 64 == 32 and (sc.h // 2) % 64 == 32
        assert hot.want["stats"].trianglesRastered > 16384 + 3072 * 1024
    g = F.HOTSPOT_GATE[order]
    assert letters[g - 1] != letters[g], "the first frame behind the gate must contradict the report the host holds"
    assert len(set(letters[g:])) == 2, "both kinds of frame run under the stale report"
    assert len(set(letters[:g])) == 1


@pytest.mark.parametrize("kind", ["small", "masked"])
def test_moving_frames_differ_and_so_do_crossed_states(kind):
    """Frame k+1's objects under frame k's view, and frame k's objects under frame k+1's view, are valid frames with other images
    than frame k's and frame k+1's: a host buffer read late, a bound array rewritten early or a view published late all show."""
    sc = F.moving(kind)
    for k in range(len(sc.frames) - 1):
        a, b = sc.frames[k], sc.frames[k + 1]
        assert _differ(a.want, b.want), (kind, k)
        assert a.view.tobytes() != b.view.tobytes() and a.iv.tobytes() != b.iv.tobytes() and not np.array_equal(a.objs, b.objs)
        late_objs = F.crossed(sc, k + 1, k)
        late_view = F.crossed(sc, k, k + 1)
        for x in (late_objs, late_view):
            assert _differ(x, a.want) and _differ(x, b.want) and x["vis"].any(), (kind, k)
        assert not np.array_equal(late_objs["cmds"], a.want["cmds"]) or _differ(late_objs, a.want)


def test_the_large_object_array_differs_from_pose_to_pose():
    """update_objects at BASELINE config 4's size: 5 MB of records (beyond what the HIP runtime stages for a pageable copy in one piece),
    and the next pose's objects under a frame's view give another image."""
    sc = F.moving("street_x64", 3, 640, 360)
    assert sc.frames[0].objs.nbytes > 4 << 20
    for k in range(2):
        assert _differ(sc.frames[k].want, sc.frames[k + 1].want) and not np.array_equal(sc.frames[k].objs, sc.frames[k + 1].objs)
    late = F.crossed(sc, 1, 0)
    assert _differ(late, sc.frames[0].want) and late["vis"].any()


def test_many_frames_all_differ_from_their_neighbours():
    sc = F.moving("small", 24)
    for k in range(23):
        assert _differ(sc.frames[k].want, sc.frames[k + 1].want), k
    second = [int(f.want["counts"][3]) for f in sc.frames[1:]]
    # (second passes of every kind along the way: none, a handful of clusters, the whole scene when the camera runs into a wall)
    assert 0 in second and any(0 < s < 20 for s in second) and any(s > 200 for s in second), second


def test_state_changes_lead_to_other_frames():
    """The frame after each state change of test_state_changes_that_may_wait is not the frame that would have run without it."""
    import orc
    sc, other, small = F.moving("small"), F.moving("masked"), F.moving("small", 2, 256, 160)
    f2 = sc.frames[2]
    scene2 = sc.scene.with_objects(f2.objs)
    # upload_history_hzb of frame 0's chain where frame 1's was the history: other stage counts
    up = orc.frame(scene2, f2.view, f2.iv, sc.flags, prev_hzb_min=sc.frames[0].want["hzb_min"])
    assert not np.array_equal(sc.frames[0].want["hzb_min"], sc.frames[1].want["hzb_min"])
    assert up["counts"].tolist() != f2.want["counts"].tolist(), up["counts"]
    # reset_history: a frame without a second pass submits other triangles
    reset = orc.frame(scene2, f2.view, f2.iv, sc.flags)
    assert reset["stats"].trianglesSubmitted != f2.want["stats"].trianglesSubmitted
    # another size, another scene
    assert (small.w, small.h) != (sc.w, sc.h) and small.frames[0].want["vis"].any()
    assert len(other.scene.objects) != len(sc.scene.objects) or _differ(other.frames[0].want, sc.frames[0].want)
    assert _differ(other.frames[0].want, sc.frames[2].want)


def test_the_misordered_write_of_the_sensitivity_test_shows():
    """test_the_gate_exposes_a_write_that_is_not_ordered: pose 1's objects under view 0 (no history) is neither frame 0 nor empty."""
    sc = F.moving("small")
    x = F.crossed(sc, 1, 0)
    assert _differ(x, sc.frames[0].want) and x["vis"].any()
