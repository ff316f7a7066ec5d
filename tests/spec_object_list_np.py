"""The two tables chordvis_upload_scene and chordvis_set_object_list derive from an object list, restated in numpy for a
records.Scene (one asset: every asset base is 0): the per-object static table (DObjStatic, 48 bytes) and the flattened
(object, group) table (DGroupRef, 24 bytes), as chord_amd/csrc/device_layer.h lays them out and chordvis_debug_read 9 / 8 hands
them back.  Vectorised over the group instances; tests/test_object_list_spec.py holds it against a plain loop."""
import numpy as np

u32, f32 = np.uint32, np.float32

OBJ_STATIC = np.dtype([("prim", u32), ("matFlags", u32), ("groupBase", u32), ("shadingType", u32),
                       ("posMin", f32, 3), ("pad0", u32), ("posMax", f32, 3), ("pad1", u32)])
GROUP_REF = np.dtype([("object", u32), ("group", u32), ("meshlet", u32, 4)])
assert OBJ_STATIC.itemsize == 48 and GROUP_REF.itemsize == 24

GROUP_MAX_MESHLETS = 4            # CHORD_GROUP_MAX_MESHLETS (nanite_builder.cpp:411-415)
MAX_INSTANCE_ID = (1 << 24) - 2   # CHORD_MAX_INSTANCE_ID: a list of this many cluster instances or more is refused
MAX_GROUP_INSTANCES = (1 << 31) - 1


def relist(scene, order, materials=None):
    """The scene under the object list [scene.objects[k] for k in order] (material ids replaced where `materials` gives them): the
    same assets, primitives and materials, the objects' records and world transforms picked by `order`."""
    order = np.asarray(list(order), dtype=np.int64)
    objs = scene.objects[order].copy()
    if materials is not None:
        objs["GLTFMaterialData"] = np.asarray(materials, dtype=np.uint32)
    out = scene.with_objects(objs)
    out.local_to_world = np.ascontiguousarray(scene.local_to_world[order])
    return out


def obj_static(scene):
    """OBJ_STATIC[len(scene.objects)]."""
    prim = scene.objects["GLTFPrimitiveDetail"].astype(np.int64)
    mat_id = scene.objects["GLTFMaterialData"].astype(np.int64)
    assert (prim < len(scene.primitives)).all() and (mat_id < len(scene.materials)).all()
    mat = scene.materials[mat_id]
    out = np.zeros(len(prim), dtype=OBJ_STATIC)
    out["prim"] = prim
    # bit 0 bTwoSided, bits 1-2 alphaMode (anything past blend draws nothing, like blend), bits 8.. the material's index
    out["matFlags"] = (mat["bTwoSided"] != 0).astype(u32) | (np.minimum(mat["alphaMode"], 2).astype(u32) << u32(1)) | (mat_id.astype(u32) << u32(8))
    counts = scene.primitives["meshletGroupCount"][prim].astype(np.int64)
    out["groupBase"] = np.concatenate([[0], np.cumsum(counts)[:-1]]) if len(prim) else []
    out["shadingType"] = mat["materialType"]
    out["posMin"] = scene.primitives["posMin"][prim]
    out["posMax"] = scene.primitives["posMax"][prim]
    return out


def group_refs(scene):
    """GROUP_REF[scene.group_instances]: object o's groups at [groupBase(o), groupBase(o) + its primitive's group count), in the
    primitive's order.  Unused meshlet slots repeat the first; all four are 0 for a group of no meshlets."""
    prim = scene.objects["GLTFPrimitiveDetail"].astype(np.int64)
    P = scene.primitives
    counts = P["meshletGroupCount"][prim].astype(np.int64)
    total = int(counts.sum())
    out = np.zeros(total, dtype=GROUP_REF)
    if total == 0:
        return out
    owner = np.repeat(np.arange(len(prim), dtype=np.int64), counts)
    base = np.concatenate([[0], np.cumsum(counts)[:-1]])
    p = prim[owner]
    g = P["meshletGroupOffset"][p].astype(np.int64) + (np.arange(total, dtype=np.int64) - base[owner])
    cnt = np.minimum(scene.groups["meshletCount"][g].astype(np.int64), GROUP_MAX_MESHLETS)
    k = np.arange(GROUP_MAX_MESHLETS, dtype=np.int64)[None, :]
    at = (P["meshletGroupIndicesOffset"][p].astype(np.int64) + scene.groups["meshletOffset"][g].astype(np.int64))[:, None] + np.where(k < cnt[:, None], k, 0)
    at = np.where(cnt[:, None] > 0, at, 0)                      # (a group of no meshlets reads no index)
    ids = P["meshletOffset"][p].astype(np.int64)[:, None] + scene.group_indices[at].astype(np.int64)
    out["object"] = owner
    out["group"] = g.astype(u32) | (cnt.astype(u32) << u32(28))
    out["meshlet"] = np.where(cnt[:, None] > 0, ids, 0)
    return out


def totals(scene):
    """(group instances, cluster instances, triangles of every cluster instance, count blocks) of the list: what the launches and the
    capacities of a context are sized by."""
    prim = scene.objects["GLTFPrimitiveDetail"].astype(np.int64)
    refs = group_refs(scene)
    cnt = (refs["group"] >> u32(28)).astype(np.int64)
    tri = ((scene.meshlets["vertexTriangleCount"] >> u32(8)) & u32(0xFF)).astype(np.int64)
    used = np.arange(GROUP_MAX_MESHLETS)[None, :] < cnt[:, None]
    triangles = int(tri[refs["meshlet"].astype(np.int64)][used].sum()) if len(refs) else 0
    groups = int(scene.primitives["meshletGroupCount"][prim].sum())
    return groups, int(cnt.sum()), triangles, max(1, -(-groups // 256))
