"""Boxes for chordvis_query_bounds and the scene the oracle answers them with.  TEST INFRASTRUCTURE.

A box is a one-object, one-primitive, one-meshlet scene whose primitive and meshlet bounds are the box: orc.object_cull then gives
IN_FRUSTUM and orc.hzb_culling -- asked with cmds[i] = (i, i, i) -- gives UNOCCLUDED.  make_boxes places seeded boxes in the space of
a camera so that every way the two tests can go occurs: outside the frustum, hidden, visible, reaching the near plane, behind the
camera, beside the screen, smaller than a pixel, and wide enough to be tested on the top levels of the chain.  Transforms carry a
rotation, a non-uniform scale and (every third box) a mirror; every fourth box moved since the last frame."""
import math

import numpy as np

from chord_amd import records as R
from chord_amd import scenes

KINDS = ("outside", "field", "buried", "near", "behind", "edge", "subpixel", "wide")
CLASSES = ("frustum_culled", "occluded", "visible", "near", "offscreen", "empty_rect", "top_levels")


def _basis(cam):
    f = np.asarray(cam.front, dtype=np.float64)
    f = f / np.linalg.norm(f)
    r = np.cross(f, np.asarray(cam.world_up, dtype=np.float64))
    r = r / np.linalg.norm(r)
    return f, r, np.cross(r, f)


def _rotation(axis, angle):
    a = axis / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def make_boxes(cam, cam_last, count, seed):
    """(queries records.BOUNDS_QUERY[count], kinds int[count] indexing KINDS) for the camera of this frame and of the last one."""
    from chord_amd import lib as L
    import ctypes as C
    rng = np.random.default_rng(seed)
    f, r, u = _basis(cam)
    pos = np.asarray(cam.position, dtype=np.float64)
    ty = math.tan(0.5 * cam.fovy)
    tx = ty * cam.width / cam.height
    px = 2.0 * ty / cam.height                     # a pixel's size at depth 1
    kinds = rng.integers(0, len(KINDS), size=count)
    l2w = np.zeros((count, 4, 4)); l2w_last = np.zeros((count, 4, 4))
    pmin = np.zeros((count, 3), dtype=np.float32); pmax = np.zeros((count, 3), dtype=np.float32)
    for i in range(count):
        k = KINDS[kinds[i]]
        x, y = rng.uniform(-0.9, 0.9, size=2)      # centre in normalised device coordinates, depth along the view direction
        d = math.exp(rng.uniform(math.log(2.0), math.log(30.0)))
        half = np.exp(rng.uniform(math.log(0.05), math.log(0.6), size=3))
        if k == "outside":
            side = rng.integers(0, 4)
            x, y = [(rng.uniform(1.4, 3.0), y), (-rng.uniform(1.4, 3.0), y), (x, rng.uniform(1.4, 3.0)), (x, -rng.uniform(1.4, 3.0))][side]
            half *= 0.3
        elif k == "buried":                         # below the ground plane of small_test_scene, or far behind what stands on it
            d = rng.uniform(6.0, 16.0)
            half *= 0.25
        elif k == "near":                           # reaches the near plane: the camera is inside or next to it
            d = rng.uniform(-0.3, 0.6)
            x, y = rng.uniform(-0.3, 0.3, size=2)
            half = rng.uniform(0.7, 1.5, size=3)
        elif k == "behind":
            d = -rng.uniform(1.0, 20.0)
        elif k == "edge":                           # at the border of the screen: inside one frame's frustum, beside the other's screen
            side = rng.integers(0, 4)
            e = rng.uniform(0.97, 1.12)
            x, y = [(e, y), (-e, y), (x, e), (x, -e)][side]
            half = np.exp(rng.uniform(math.log(0.01), math.log(0.06), size=3)) * d * 0.1
        elif k == "subpixel":
            half = rng.uniform(0.05, 0.45, size=3) * px * d
        elif k == "wide":                           # a slab across the view, thin along it, in front of everything
            d = rng.uniform(1.5, 6.0)
            x, y = rng.uniform(-0.3, 0.3, size=2)
            half = np.array([rng.uniform(0.3, 1.2) * tx * d, rng.uniform(0.3, 1.2) * ty * d, 0.01])
        centre = pos + f * d + r * (x * tx * abs(d)) + u * (y * ty * abs(d))
        if k == "buried" and i % 2 == 0:
            centre[1] = -rng.uniform(0.8, 3.0)
        # local box: off-centre; transform: rotation (none for the wide slabs, which face the camera), non-uniform scale, a mirror
        lo = -rng.uniform(0.5, 1.5, size=3); hi = rng.uniform(0.5, 1.5, size=3)
        sc = 2.0 * half / (hi - lo)
        if i % 3 == 0:
            sc[(i // 3) % 3 if k != "wide" else 0] *= -1.0
        rot = np.stack([r, u, -f], axis=1) if k == "wide" else _rotation(rng.normal(size=3), rng.uniform(0, 2 * math.pi))
        A = rot @ np.diag(sc)
        m = np.eye(4); m[:3, :3] = A; m[:3, 3] = centre - A @ (0.5 * (lo + hi))
        ml = m.copy()
        if i % 4 == 0:                              # it moved: last frame it was somewhere else, turned a little
            step = _rotation(rng.normal(size=3), rng.uniform(-0.2, 0.2))
            ml[:3, :3] = step @ A
            ml[:3, 3] = m[:3, 3] + (r * rng.uniform(-0.5, 0.5) + u * rng.uniform(-0.3, 0.3) + f * rng.uniform(-0.5, 0.5)) * 0.1 * abs(d)
        l2w[i], l2w_last[i] = m, ml
        pmin[i], pmax[i] = lo, hi
    # the library's own conversion to camera-relative float matrices (chordvis_object_basic_data_batch)
    objects = np.zeros(count, dtype=R.OBJECT)
    cols = np.ascontiguousarray(np.stack([m.T.reshape(16) for m in l2w]), dtype=np.float64)
    cols_last = np.ascontiguousarray(np.stack([m.T.reshape(16) for m in l2w_last]), dtype=np.float64)
    rc = L.lib.chordvis_object_basic_data_batch(count, cols.ctypes.data, cols_last.ctypes.data, (C.c_double * 3)(*cam.position),
                                                (C.c_double * 3)(*cam_last.position), objects.ctypes.data)
    assert rc == L.OK
    q = np.zeros(count, dtype=R.BOUNDS_QUERY)
    q["localToTranslatedWorld"] = objects["localToTranslatedWorld"]
    q["localToTranslatedWorldLastFrame"] = objects["localToTranslatedWorldLastFrame"]
    q["posMin"], q["posMax"] = pmin, pmax
    q["user"] = (np.arange(count, dtype=np.uint64) * 2654435761 & 0xFFFFFFFF).astype(np.uint32)
    return q, kinds


def oracle_scene(queries):
    """records.Scene the oracle answers the queries with: object i -> primitive i -> meshlet i, both bounds the box."""
    n = len(queries)
    objects = np.zeros(n, dtype=R.OBJECT)
    objects["localToTranslatedWorld"] = queries["localToTranslatedWorld"]
    objects["localToTranslatedWorldLastFrame"] = queries["localToTranslatedWorldLastFrame"]
    objects["GLTFPrimitiveDetail"] = np.arange(n)
    prims = np.zeros(n, dtype=R.PRIMITIVE)
    prims["posMin"], prims["posMax"] = queries["posMin"], queries["posMax"]
    prims["meshletOffset"] = np.arange(n)
    meshlets = np.zeros(n, dtype=R.MESHLET)
    meshlets["posMin"], meshlets["posMax"] = queries["posMin"], queries["posMax"]
    return R.Scene(objects, prims, np.zeros(1, dtype=R.MATERIAL), meshlets, np.zeros(0, dtype=R.MESHLET_GROUP), np.zeros(0, dtype=np.uint32),
                   np.zeros(0, dtype=np.uint32), np.zeros((0, 3), dtype=np.float32), name="bounds_queries")


def oracle_answers(queries, view, iv, phase, desc, hzb_min):
    """(in_frustum bool[n], unoccluded bool[n]) from the oracle.  The frustum answer of phase 0 is the object stage's on last
    frame's matrix."""
    import orc
    n = len(queries)
    flags = R.FLAG_FRUSTUM_CULL | R.FLAG_HZB_CULL
    scene = oracle_scene(queries)
    if phase == 0:
        frustum_scene = oracle_scene(queries)
        frustum_scene.objects["localToTranslatedWorld"] = queries["localToTranslatedWorldLastFrame"]
    else:
        frustum_scene = scene
    in_frustum = orc.object_cull(frustum_scene, iv, flags).astype(bool)
    cmds = np.zeros(n, dtype=R.DRAW_CMD)
    cmds["objectId"] = cmds["meshletId"] = cmds["slot"] = np.arange(n)
    vis, _ = orc.hzb_culling(scene, view, flags, phase, desc, np.ascontiguousarray(hzb_min, dtype=np.uint16), cmds)
    unoccluded = np.zeros(n, dtype=bool)
    unoccluded[vis["slot"]] = True
    return in_frustum, unoccluded


def two_frames(width, height):
    """small_test_scene under a camera that moved and turned between its two frames: (scene, cam_last, cam, (view_last, iv_last),
    (view, iv)).  The scene's object records are left filled for the second frame.  (The turn is what lets phase 0 find a box inside
    this frame's frustum and beside last frame's screen: last frame's matrices are relative to last frame's camera position, so a
    camera that only moved would test the same box against the same planes.)"""
    from chord_amd import lib as L
    scene, cam_last = scenes.small_test_scene(width, height)
    cam = cam_last.moved((0.35, 0.1, -0.25))
    cam.front = (0.74, -0.09, -0.66)
    view_last, iv_last = L.make_views(cam_last)
    view, iv = L.make_views(cam, view_last)
    L.fill_objects(scene, cam, cam_last)
    return scene, cam_last, cam, (view_last, iv_last), (view, iv)


def fill_for(scene, cam, cam_last=None):
    from chord_amd import lib as L
    L.fill_objects(scene, cam, cam_last)


def level_chain(desc, depths):
    """A min chain in which every level holds its own constant (binary16 bits): the constants are spread over `depths` (projected
    nearest depths of the boxes under test), falling with the level -- reverse Z: a finer level is nearer --, so that a box of a given
    depth is hidden on the fine levels and seen on the coarse ones: the verdict says which level was tapped."""
    z = np.sort(np.asarray(depths, dtype=np.float32))
    z = z[(z > 0) & (z < 1)]
    chain = np.zeros(desc.totalTexels, dtype=np.uint16)
    n = desc.mipCount
    for l in range(n):
        c = np.float16(z[int((len(z) - 1) * (n - l - 0.5) / n)])
        mw, mh = desc.mip_dims(l)
        chain[int(desc.mipOffset[l]): int(desc.mipOffset[l]) + mw * mh] = c.view(np.uint16)
    return chain
