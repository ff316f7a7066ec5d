"""chordvis_query_bounds on the CPU: the numpy restatement of its contract (spec_bounds_query_np) gives, for every generated box,
the two answers the oracle gives for the equivalent one-meshlet scene -- against a chain the oracle built and against a chain whose
every level holds its own constant --, the generator reaches every way the tests can go, and the records of the header, records.py
and lib.py agree.  Runs without a GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import bounds_scenes as B
import spec_bounds_query_np as S
from chord_amd import records as R
from helpers import ALL_FLAGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOXES = 2000
MIN_SHARE = 0.03


@pytest.fixture(scope="module")
def rendered(built_lib):
    """small_test_scene at 160 x 96, two oracle frames with a moved camera: the second frame's views and the chain it left."""
    import orc
    scene, cam_last, cam, (view_last, iv_last), (view, iv) = B.two_frames(160, 96)
    B.fill_for(scene, cam_last)
    first = orc.frame(scene, view_last, iv_last, ALL_FLAGS)
    B.fill_for(scene, cam, cam_last)
    second = orc.frame(scene, view, iv, ALL_FLAGS, prev_hzb_min=first["hzb_min"])
    queries, kinds = B.make_boxes(cam, cam_last, BOXES, seed=11)
    return dict(dims=(160, 96), view=view, iv=iv, desc=second["desc"], chain=second["hzb_min"], queries=queries, kinds=kinds)


@pytest.fixture(scope="module")
def levelled(built_lib):
    """129 x 67 under the same two cameras, and a chain in which every level holds its own constant."""
    import orc
    _, cam_last, cam, (view_last, _), (view, iv) = B.two_frames(129, 67)
    queries, kinds = B.make_boxes(cam, cam_last, BOXES, seed=12)
    desc = orc.hzb_desc(129, 67)
    _, _, nearest, _ = S.tests(view, iv, queries, 1)
    return dict(dims=(129, 67), view=view, iv=iv, desc=desc, chain=B.level_chain(desc, nearest), queries=queries, kinds=kinds)


def check_against_oracle(w, phase):
    inside, status, _, _ = S.tests(w["view"], w["iv"], w["queries"], phase, w["desc"], w["chain"])
    want_inside, want_seen = B.oracle_answers(w["queries"], w["view"], w["iv"], phase, w["desc"], w["chain"])
    bad = np.flatnonzero(inside != want_inside)
    assert len(bad) == 0, "IN_FRUSTUM differs from orc.object_cull for boxes %s" % bad[:8]
    bad = np.flatnonzero(((status & R.BOUNDS_UNOCCLUDED) != 0) != want_seen)
    assert len(bad) == 0, "UNOCCLUDED differs from orc.hzb_culling for boxes %s (status %s)" % (bad[:8], status[bad[:8]])
    return S.classes(want_inside, status, top_from=S.top_level(*w["dims"]) - 1), want_seen


@pytest.mark.parametrize("phase", (1, 0))
def test_spec_equals_the_oracle_on_a_rendered_chain_and_covers_every_class(rendered, phase):
    cls, _ = check_against_oracle(rendered, phase)
    share = {k: float(v.mean()) for k, v in cls.items()}
    print("phase %d shares: %s" % (phase, {k: round(s, 3) for k, s in share.items()}))
    assert set(share) == set(B.CLASSES)
    assert all(s >= MIN_SHARE for s in share.values()), share


@pytest.mark.parametrize("phase", (1, 0))
def test_spec_equals_the_oracle_on_a_chain_of_level_constants(levelled, phase):
    cls, seen = check_against_oracle(levelled, phase)
    share = {k: float(v.mean()) for k, v in cls.items()}
    print("phase %d shares: %s" % (phase, {k: round(s, 3) for k, s in share.items()}))
    assert all(s >= MIN_SHARE for s in share.values()), share
    # the verdict follows the level: the same chain with its levels' constants in the opposite order answers differently
    w = dict(levelled)
    desc = w["desc"]
    flipped = np.array(w["chain"], copy=True)
    for l in range(desc.mipCount):
        mw, mh = desc.mip_dims(l)
        flipped[int(desc.mipOffset[l]): int(desc.mipOffset[l]) + mw * mh] = w["chain"][int(desc.mipOffset[desc.mipCount - 1 - l])]
    w["chain"] = flipped
    _, seen_flipped = check_against_oracle(w, phase)
    # (how many: level l of n holds the depth quantile (n - l - 0.5) / n, and (l + 0.5) / n when flipped; a box tapped on level l
    # answers differently when its depth lies between the two, a band |n - 2 l - 1| / n of the depths wide -- 0.5 on average over the
    # eight levels here.  Neither the levels nor the tapped boxes' depths are spread evenly: half of that is asked for.)
    tapped = cls["occluded"] | cls["visible"]
    assert (seen != seen_flipped)[tapped].mean() >= 0.25
    # ... and every level a rectangle of this screen can reach is tapped by some box
    _, status, _, _ = S.tests(levelled["view"], levelled["iv"], levelled["queries"], phase, desc, levelled["chain"])
    plain = (status & (R.BOUNDS_NEAR | R.BOUNDS_OFFSCREEN | R.BOUNDS_EMPTY_RECT)) == 0
    assert set(((status[plain] >> R.BOUNDS_LEVEL_SHIFT) & R.BOUNDS_LEVEL_MASK).tolist()) == set(range(S.top_level(*levelled["dims"]) + 1))


def test_results_and_list_follow_the_contract(rendered):
    """What the two tests' answers become in the records: a culled box is all zero, the list is the ascending indices of the boxes
    with both bits, and without a chain only the boxes that reach a tap change."""
    w = rendered
    res, vis, n = S.query_bounds(w["view"], w["iv"], w["queries"], 1, w["desc"], w["chain"])
    culled = (res["status"] & R.BOUNDS_IN_FRUSTUM) == 0
    assert culled.any() and not res[culled].view(np.uint8).any()
    both = R.BOUNDS_IN_FRUSTUM | R.BOUNDS_UNOCCLUDED
    assert n == len(vis) and np.array_equal(vis, np.flatnonzero((res["status"] & both) == both)) and (np.diff(vis.astype(np.int64)) > 0).all()
    bare, vis0, _ = S.query_bounds(w["view"], w["iv"], w["queries"], 1)
    rejected = (bare["status"] & (R.BOUNDS_OFFSCREEN | R.BOUNDS_EMPTY_RECT)) != 0
    assert np.array_equal((bare["status"] & R.BOUNDS_UNOCCLUDED) != 0, ~culled & ~rejected)
    assert not ((bare["status"] >> R.BOUNDS_LEVEL_SHIFT) & R.BOUNDS_LEVEL_MASK).any()
    assert np.array_equal(bare["rect"], res["rect"]) and np.array_equal(bare["nearestZ"].view(np.uint32), res["nearestZ"].view(np.uint32))
    assert set(vis.tolist()) <= set(vis0.tolist())
    near = (res["status"] & R.BOUNDS_NEAR) != 0
    assert near.any() and (res["nearestZ"][near] == 1.0).all() and (res["rect"][near] == (0, 0, 159, 95)).all()
    off = (res["status"] & R.BOUNDS_OFFSCREEN) != 0
    assert not res["rect"][off].any()


def test_query_record_layouts_match_the_header(built_lib):
    L = built_lib
    numpy_mirrors = {"ChordBoundsQuery": R.BOUNDS_QUERY, "ChordBoundsResult": R.BOUNDS_RESULT}
    ctypes_mirrors = {"ChordBoundsQuery": L.BoundsQuery, "ChordBoundsResult": L.BoundsResult}
    lines = []
    for cname, dt in numpy_mirrors.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in dt.names:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    for name in ("IN_FRUSTUM", "UNOCCLUDED", "NEAR", "OFFSCREEN", "EMPTY_RECT", "LEVEL_SHIFT", "LEVEL_MASK"):
        lines.append('printf("%s %%u\\n", (unsigned)CHORD_BOUNDS_%s);' % (name, name))
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "chordvis.h"\nint main(void){\n%s\nreturn 0;}\n' % "\n".join(lines)
    with tempfile.TemporaryDirectory() as td:
        cpath, exe = os.path.join(td, "l.c"), os.path.join(td, "l")
        open(cpath, "w").write(src)
        cc = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), cpath, "-o", exe], capture_output=True, text=True)
        assert cc.returncode == 0, cc.stderr[-1500:]
        out = dict(l.split() for l in subprocess.check_output([exe]).decode().splitlines())
    assert [int(out["ChordBoundsQuery"]), int(out["ChordBoundsResult"])] == [160, 16]
    for cname, dt in numpy_mirrors.items():
        ct = ctypes_mirrors[cname]
        assert int(out[cname]) == dt.itemsize == C.sizeof(ct), cname
        assert [f for f, _ in ct._fields_] == list(dt.names), cname
        for f in dt.names:
            assert int(out["%s.%s" % (cname, f)]) == dt.fields[f][1] == getattr(ct, f).offset, (cname, f)
    for name in ("IN_FRUSTUM", "UNOCCLUDED", "NEAR", "OFFSCREEN", "EMPTY_RECT", "LEVEL_SHIFT", "LEVEL_MASK"):
        assert int(out[name]) == getattr(R, "BOUNDS_" + name), name
    assert "chordvis_query_bounds" in L.EXPORTED
