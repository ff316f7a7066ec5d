"""tests/spec_object_list_np.py -- the numpy restatement of the per-object static table and the flattened (object, group) table -- held
against a plain Python loop written from chordvis_upload_scene's (chordvis_abi.cpp "objects"), against the Scene's own aggregate counts,
and under permutation, repetition and omission of objects: the lists tests/test_gpu_object_list.py hands to chordvis_set_object_list."""
import functools

import numpy as np
import pytest

import spec_object_list_np as S
from chord_amd import scenes


@functools.lru_cache(maxsize=None)
def _small():
    return scenes.small_test_scene()[0]


@functools.lru_cache(maxsize=None)
def _groups257():
    return scenes.group_count_scene(257)[0]


def loop_tables(scene):
    """(static records as tuples, group refs as 6-tuples) by the walk object -> primitive -> group -> group indices."""
    stat, refs, base = [], [], 0
    for o, ob in enumerate(scene.objects):
        p = scene.primitives[int(ob["GLTFPrimitiveDetail"])]
        m = scene.materials[int(ob["GLTFMaterialData"])]
        flags = (1 if m["bTwoSided"] else 0) | (min(int(m["alphaMode"]), 2) << 1) | (int(ob["GLTFMaterialData"]) << 8)
        stat.append((int(ob["GLTFPrimitiveDetail"]), flags, base, int(m["materialType"]), tuple(p["posMin"].tolist()), tuple(p["posMax"].tolist())))
        for gl in range(int(p["meshletGroupCount"])):
            gi = int(p["meshletGroupOffset"]) + gl
            g = scene.groups[gi]
            cnt = min(int(g["meshletCount"]), 4)
            ids = [int(p["meshletOffset"]) + int(scene.group_indices[int(p["meshletGroupIndicesOffset"]) + int(g["meshletOffset"]) + (i if i < cnt else 0)])
                   if cnt else 0 for i in range(4)]
            refs.append((o, gi | (cnt << 28), *ids))
        base += int(p["meshletGroupCount"])
    return stat, refs


def assert_matches_loop(scene):
    stat, refs = loop_tables(scene)
    got_s, got_r = S.obj_static(scene), S.group_refs(scene)
    assert len(got_s) == len(stat) and len(got_r) == len(refs)
    for a, b in zip(got_s, stat):
        assert (int(a["prim"]), int(a["matFlags"]), int(a["groupBase"]), int(a["shadingType"]), tuple(a["posMin"].tolist()), tuple(a["posMax"].tolist())) == b
        assert a["pad0"] == 0 and a["pad1"] == 0
    assert [(int(r["object"]), int(r["group"]), *r["meshlet"].tolist()) for r in got_r] == refs


def test_layouts_are_the_device_records():
    assert S.OBJ_STATIC.itemsize == 48 and S.GROUP_REF.itemsize == 24
    assert [S.OBJ_STATIC.fields[n][1] for n in ("prim", "matFlags", "groupBase", "shadingType", "posMin", "pad0", "posMax", "pad1")] == [0, 4, 8, 12, 16, 28, 32, 44]
    assert [S.GROUP_REF.fields[n][1] for n in ("object", "group", "meshlet")] == [0, 4, 8]


def test_spec_matches_a_plain_loop_and_the_scene_counts():
    scene = _small()
    assert_matches_loop(scene)
    groups, clusters, triangles, blocks = S.totals(scene)
    assert groups == scene.group_instances == len(S.group_refs(scene))
    assert clusters == scene.lod0_meshlet_instances
    tri = (scene.meshlets["vertexTriangleCount"] >> 8) & 0xFF
    assert triangles == sum(int(tri[m]) for r in loop_tables(scene)[1] for m in r[2:2 + (r[1] >> 28)])
    assert blocks == max(1, -(-groups // 256))
    # a material's flags: small_test_scene has one two-sided material (index 1) on some objects
    st = S.obj_static(scene)
    two = scene.objects["GLTFMaterialData"] == 1
    assert two.any() and (~two).any()
    assert ((st["matFlags"] & 1) == two).all() and ((st["matFlags"] >> 8) == scene.objects["GLTFMaterialData"]).all()


def test_count_blocks_of_the_group_count_scene():
    scene = _groups257()
    assert_matches_loop(scene)
    assert S.totals(scene)[0] == 257 and S.totals(scene)[3] == 2
    # the 64-group panel ahead of one-group tiles: bases step by 64, then by 1
    st = S.obj_static(scene)
    assert st["groupBase"].tolist() == [0, 64, 128, 192, 256]


LISTS = {
    "reversed": lambda n: list(range(n))[::-1],
    "subset": lambda n: [k for k in range(n) if k % 3 != 1],
    "repeated": lambda n: [0, 2, 2, 1, 2] + list(range(3, n)),
    "single": lambda n: [n - 1],
}


@pytest.mark.parametrize("name", sorted(LISTS))
@pytest.mark.parametrize("which", ["small", "groups257"])
def test_spec_under_permutation_repetition_and_omission(which, name):
    scene = _small() if which == "small" else _groups257()
    order = LISTS[name](len(scene.objects))
    new = S.relist(scene, order)
    assert_matches_loop(new)
    # every object's block of the table is its source object's block with the owner renamed, wherever it now stands
    old_s, old_r = S.obj_static(scene), S.group_refs(scene)
    new_s, new_r = S.obj_static(new), S.group_refs(new)
    assert new.group_instances == len(new_r) == sum(int(scene.primitives["meshletGroupCount"][scene.objects["GLTFPrimitiveDetail"][k]]) for k in order)
    for o, k in enumerate(order):
        n = int(scene.primitives["meshletGroupCount"][scene.objects["GLTFPrimitiveDetail"][k]])
        a, b = int(new_s["groupBase"][o]), int(old_s["groupBase"][k])
        assert (new_r["object"][a:a + n] == o).all()
        assert np.array_equal(new_r["group"][a:a + n], old_r["group"][b:b + n]) and np.array_equal(new_r["meshlet"][a:a + n], old_r["meshlet"][b:b + n])
        for f in ("prim", "matFlags", "shadingType", "posMin", "posMax"):
            assert np.array_equal(new_s[f][o], old_s[f][k])


def test_rematerialed_objects_change_flags_only():
    scene = _small()
    n = len(scene.objects)
    mats = scene.objects["GLTFMaterialData"].copy()
    mats[0] = 1 - mats[0]                                    # one-sided <-> two-sided
    new = S.relist(scene, range(n), mats)
    a, b = S.obj_static(scene), S.obj_static(new)
    assert (a["matFlags"][0] ^ b["matFlags"][0]) == (1 | (1 << 8))
    assert np.array_equal(a["matFlags"][1:], b["matFlags"][1:]) and np.array_equal(a["groupBase"], b["groupBase"])
    assert np.array_equal(S.group_refs(scene), S.group_refs(new))


def test_a_primitive_no_object_named():
    """A list may name a primitive that no object of the uploaded list named: group_count_scene(64) is 64 one-group tiles, and the
    64-group panel primitive is in the scene's tables with no object of its own."""
    scene = scenes.group_count_scene(64)[0]
    assert len(scene.primitives) == 2 and set(scene.objects["GLTFPrimitiveDetail"].tolist()) == {1}
    objs = scene.objects[:3].copy()
    objs["GLTFPrimitiveDetail"][1] = 0
    new = scene.with_objects(objs)
    assert_matches_loop(new)
    assert S.obj_static(new)["groupBase"].tolist() == [0, 1, 65] and new.group_instances == 66
