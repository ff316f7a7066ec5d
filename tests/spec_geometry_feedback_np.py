"""chordvis_geometry_feedback and chordvis_visible_clusters (include/chordvis.h) restated in numpy from their definitions: which
lattice pixels contribute, what one call adds to the seven count arrays, the seen bitmap and the visible-cluster list.  Integers
throughout.  TEST INFRASTRUCTURE: never imported by chord_amd/.

Scenes are records.Scene (one asset): a command's meshletId indexes scene.meshlets directly, an object's GLTFPrimitiveDetail is the
row of scene.primitives."""
import numpy as np

LODS = 16
ARRAYS = ("objectPixels", "objectSubmitted", "objectVisible", "lodPixels", "lodSubmitted", "lodVisible", "totals")
PIXEL_ARRAYS = ("objectPixels", "lodPixels")


def command_keys(scene, cmds):
    """Per command: (valid, object, prim, lod) -- valid: objectId and meshletId in range; the others 0 where it is not."""
    cmds = np.asarray(cmds)
    obj = cmds["objectId"].astype(np.int64)
    mid = cmds["meshletId"].astype(np.int64)
    valid = (obj < len(scene.objects)) & (mid < len(scene.meshlets))
    obj, mid = np.where(valid, obj, 0), np.where(valid, mid, 0)
    prim = scene.objects["GLTFPrimitiveDetail"][obj].astype(np.int64)
    lod = np.minimum(scene.meshlets["lod"][mid].astype(np.int64), LODS - 1)
    return valid, obj, np.where(valid, prim, 0), np.where(valid, lod, 0)


def geometry_feedback(scene, words, cmds, count, w, h, capacity, stride=1, offset=(0, 0)):
    """What ONE call adds: {the seven arrays of ARRAYS (uint32), "seen": the bitmap's ceil(capacity / 32) words, "visible": the seen
    commands in list order (records verbatim), "n": min(count, capacity), "contributing": (h, w) bool over the whole image with the
    off-lattice pixels False}.  cmds: at least n records."""
    cmds = np.asarray(cmds)
    n = min(int(count), int(capacity))
    assert len(cmds) >= n
    n_obj, n_prim = len(scene.objects), len(scene.primitives)
    low = (np.asarray(words, dtype=np.uint64).reshape(h, w) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    lattice = np.zeros((h, w), dtype=bool)
    lattice[offset[1]::stride, offset[0]::stride] = True
    slot = ((low >> 8) & 0xFFFFFF) - 1                                 # (-1: an id field of 0, which names no command)
    tri = low & 0xFF
    named = lattice & (low != 0) & (slot >= 0) & (slot < n)
    valid, obj, prim, lod = command_keys(scene, cmds[:n])
    at = np.where(named, slot, 0)
    if n:
        tri_count = (scene.meshlets["vertexTriangleCount"][np.where(valid, cmds["meshletId"][:n], 0).astype(np.int64)].astype(np.int64) >> 8) & 0xFF
        contributing = named & valid[at] & (tri < tri_count[at])
    else:
        contributing = np.zeros((h, w), dtype=bool)
    hit = at[contributing]
    per_cmd = np.bincount(hit, minlength=max(n, 1))[:n]                # contributing pixels per command
    seen = per_cmd > 0
    out = {
        "objectPixels": np.bincount(obj[hit], minlength=n_obj) if n else np.zeros(n_obj, np.int64),
        "objectSubmitted": np.bincount(obj[valid], minlength=n_obj),
        "objectVisible": np.bincount(obj[seen], minlength=n_obj),
        "lodPixels": (np.bincount(prim[hit] * LODS + lod[hit], minlength=n_prim * LODS) if n else np.zeros(n_prim * LODS, np.int64)).reshape(n_prim, LODS),
        "lodSubmitted": np.bincount(prim[valid] * LODS + lod[valid], minlength=n_prim * LODS).reshape(n_prim, LODS),
        "lodVisible": np.bincount(prim[seen] * LODS + lod[seen], minlength=n_prim * LODS).reshape(n_prim, LODS),
        "totals": np.array([lattice.sum(), contributing.sum(), (lattice & (low != 0) & ~contributing).sum(), seen.sum()]),
    }
    out = {k: (v & 0xFFFFFFFF).astype(np.uint32) for k, v in out.items()}
    bitmap = np.zeros((int(capacity) + 31) // 32, dtype=np.uint32)
    idx = np.flatnonzero(seen)
    np.bitwise_or.at(bitmap, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    out["seen"] = bitmap
    out["visible"] = cmds[:n][seen].copy()
    out["n"] = n
    out["contributing"] = contributing
    return out


def identities(fb):
    """The identities the header states, as a list of the ones that FAIL (empty: all hold)."""
    bad = []
    if not (int(fb["objectPixels"].sum()) == int(fb["lodPixels"].sum()) == int(fb["totals"][1])): bad.append("sum(objectPixels) == sum(lodPixels) == totals[1]")
    if not (int(fb["objectVisible"].sum()) == int(fb["lodVisible"].sum()) == int(fb["totals"][3])): bad.append("sum(objectVisible) == sum(lodVisible) == totals[3]")
    if not (fb["objectVisible"] <= fb["objectSubmitted"]).all(): bad.append("objectVisible <= objectSubmitted")
    if not (fb["lodVisible"] <= fb["lodSubmitted"]).all(): bad.append("lodVisible <= lodSubmitted")
    if not np.array_equal(fb["objectPixels"] > 0, fb["objectVisible"] > 0): bad.append("objectPixels > 0 exactly when objectVisible > 0")
    if not int(fb["totals"][1]) + int(fb["totals"][2]) <= int(fb["totals"][0]): bad.append("contributing + rejected <= looked at")
    return bad
