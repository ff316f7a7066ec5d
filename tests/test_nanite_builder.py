"""chordvis_nanite_build: the invariants the runtime relies on (nanite_builder.cpp's own checks and the shape of
its output), the container, and -- gpu -- frames of built meshes against the oracle in both cull modes."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import helpers as H
import orc
from chord_amd import lib as L, records as R
from chord_amd import scenes


def _tris_of(a, m):
    V, T = int(m["vertexTriangleCount"]) & 0xFF, (int(m["vertexTriangleCount"]) >> 8) & 0xFF
    d = a.meshlet_data[m["dataOffset"]: m["dataOffset"] + V + T]
    verts, words = d[:V], d[V:]
    loc = np.stack([words & 0xFF, (words >> 8) & 0xFF, (words >> 16) & 0xFF], -1)
    assert (loc < V).all()
    return verts[loc]                                                           # (T, 3) global vertex ids


def test_built_asset_invariants():
    pos, idx, uv = scenes.bumpy_sphere_mesh(96, 1)
    a = L.nanite_build(pos, idx, uv)
    V = a.meshlets["vertexTriangleCount"] & 0xFF
    T = (a.meshlets["vertexTriangleCount"] >> 8) & 0xFF
    assert V.max() <= 255 and T.max() <= 128 and T.min() >= 1                      # base.h:428-430
    assert a.lod_count >= 4 and set(np.unique(a.meshlets["lod"])) == set(range(a.lod_count))
    # LOD 0 is the input: every triangle exactly once (as vertex triples up to rotation)
    def canon(t):
        t = np.asarray(t, dtype=np.int64)
        r = np.argmin(t, axis=1)
        return np.stack([np.take_along_axis(t, ((r + k) % 3)[:, None], 1)[:, 0] for k in range(3)], -1)
    lod0 = np.concatenate([_tris_of(a, m) for m in a.meshlets[a.meshlets["lod"] == 0]])
    want = canon(idx.reshape(-1, 3)); got = canon(lod0)
    order = lambda x: x[np.lexsort(x.T[::-1])]
    assert np.array_equal(order(got), order(want))
    # every level roughly halves the triangles (kGroupSimplifyThreshold 0.5, accepted only below 0.8: nanite_builder.cpp:18-21,838)
    per_lod = [int(T[a.meshlets["lod"] == l].sum()) for l in range(a.lod_count)]
    assert all(b < 0.8 * c for c, b in zip(per_lod, per_lod[1:]))
    # groups: at most 4 meshlets, each meshlet in exactly one, members share the group's spheres
    g = a.groups
    assert g["meshletCount"].max() <= 4 and g["meshletCount"].min() >= 1        # nanite_builder.cpp:411-414
    members = np.concatenate([a.group_indices[x["meshletOffset"]: x["meshletOffset"] + x["meshletCount"]] for x in g])
    assert np.array_equal(np.sort(members), np.arange(len(a.meshlets)))
    lod_of_group = np.array([a.meshlets["lod"][a.group_indices[x["meshletOffset"]]] for x in g])
    assert ((g["error"] == -1.0) == (lod_of_group == 0)).all()                   # :891
    assert (g["parentError"][g["parentError"] < 3e38] >= np.maximum(g["error"], 0)[g["parentError"] < 3e38]).all()   # error only grows up the DAG (:853)
    assert (g["parentError"] >= 3e38).any()                                      # the coarsest level is un-parented
    # a child group's parent sphere IS some coarser group's own sphere (the hand-over of :857-868)
    own = {(tuple(x["clusterPosCenter"]), float(x["error"])) for x in g if x["error"] >= 0}
    for x in g[g["parentError"] < 3e38]:
        assert (tuple(x["parentPosCenter"]), float(x["parentError"])) in own
    # cones: a camera far along the axis sees the front of every triangle of the cluster, so the test must not cull it;
    # one far behind the apex along -axis must be culled (meshlet_visible: dot(normalize(apex - cam), axis) >= cutoff culls)
    for m in a.meshlets[::7]:
        if m["coneCutOff"] >= 1.0:
            continue
        axis, apex = m["coneAxis"].astype(np.float64), m["coneApex"].astype(np.float64)
        front, back = apex + 50.0 * axis, apex - 50.0 * axis
        for cam, culled in ((front, False), (back, True)):
            v = apex - cam
            assert (np.dot(v / np.linalg.norm(v), axis) >= m["coneCutOff"]) == culled
    # BVH: shape of the reference builder + what chordvis_upload_scene checks (spheres contain the parent spheres beneath)
    nodes = a.bvh_nodes
    assert nodes[0]["bvhNodeCount"] == len(nodes)
    listed = np.concatenate([np.arange(n["leafMeshletGroupOffset"], n["leafMeshletGroupOffset"] + n["leafMeshletGroupCount"]) for n in nodes])
    assert np.array_equal(listed, np.arange(len(g)))


def test_degenerate_inputs_and_container(tmp_path):
    h = C.c_void_p()
    pos = np.zeros((3, 3), np.float32); idx = np.array([0, 1, 5], np.uint32)
    assert L.lib.chordvis_nanite_build(pos.ctypes.data, 3, idx.ctypes.data, 3, None, C.byref(h)) == L.E_INVALID      # index out of range
    assert L.lib.chordvis_nanite_build(pos.ctypes.data, 3, idx.ctypes.data, 2, None, C.byref(h)) == L.E_INVALID      # not a triangle list
    # one triangle: one meshlet, one un-parented LOD-0 group, a root-only tree
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    a = L.nanite_build(pos, [0, 1, 2])
    assert len(a.meshlets) == 1 and len(a.groups) == 1 and a.groups["error"][0] == -1.0 and a.groups["parentError"][0] > 3e38 and len(a.bvh_nodes) == 1
    # container round trip
    p, i, uv = scenes.bumpy_sphere_mesh(48, 2)
    h = L.nanite_build(p, i, uv, keep_handle=True)
    path = str(tmp_path / "sphere.chordasset").encode()
    assert L.lib.chordvis_save_asset(h, path) == L.OK
    h2 = C.c_void_p()
    assert L.lib.chordvis_load_asset(path, C.byref(h2)) == L.OK
    a1, a2 = L.BuiltAsset(h), L.BuiltAsset(h2)
    for f in ("meshlets", "groups", "group_indices", "meshlet_data", "positions", "texcoord0", "bvh_nodes", "primitive"):
        assert np.array_equal(getattr(a1, f).view(np.uint8), getattr(a2, f).view(np.uint8)), f
    L.lib.chordvis_free_built_asset(h); L.lib.chordvis_free_built_asset(h2)
    open(path.decode(), "wb").write(b"not an asset")
    assert L.lib.chordvis_load_asset(path, C.byref(h2)) == L.E_INVALID


def test_lod_selection_uses_every_level_and_covers_the_silhouette():
    scene, cam, view, iv = H.setup_scene(scenes.built_mesh_scene)
    cmds = orc.instance_culling(scene, view, iv, H.ALL_FLAGS)
    lods = scene.meshlets["lod"][cmds["meshletId"]]
    per_obj = [set(lods[cmds["objectId"] == o].tolist()) for o in range(len(scene.objects))]
    mean_lod = [float(lods[cmds["objectId"] == o].mean()) for o in range(len(scene.objects))]
    assert all(per_obj) and mean_lod[0] < mean_lod[3] < mean_lod[-1]              # coarser with distance (regions whose simplification stalled stay finer)
    assert max(per_obj[-1]) >= 4 and len(set().union(*per_obj)) >= 4              # ... and most levels of the DAG are in use somewhere
    tri = ((scene.meshlets["vertexTriangleCount"] >> 8) & 0xFF)[cmds["meshletId"]]
    per_obj_tris = [int(tri[cmds["objectId"] == o].sum()) for o in range(len(scene.objects))]
    assert per_obj_tris[-1] < 0.5 * per_obj_tris[0]                               # the far instance costs a fraction of the near one (locked group borders bound how far a level reduces)
    # the LOD cut does not open holes: what the selected clusters cover is (nearly) what LOD 0 alone covers
    fr = orc.frame(scene, view, iv, H.ALL_FLAGS)
    lod0 = scene.groups.copy()
    keep = lod0["error"] < -0.5
    lod0["parentError"][keep] = 3.4e38                                            # LOD 0 groups un-parented ...
    lod0["error"][~keep] = 1e30; lod0["parentError"][~keep] = 1e-30               # ... everything else never selected
    only0 = R.Scene(scene.objects, scene.primitives, scene.materials, scene.meshlets, lod0, scene.group_indices, scene.meshlet_data,
                    scene.positions)
    f0 = orc.frame(only0, view, iv, H.ALL_FLAGS)
    a, b = fr["vis"] != 0, f0["vis"] != 0
    assert (a != b).sum() <= 0.01 * b.sum() + 16


@pytest.mark.gpu
@pytest.mark.parametrize("hier", [0, 1], ids=["flat", "hierarchical"])
def test_built_meshes_render_like_the_oracle(gpu, hier):
    from chord_amd.renderer import VisibilityRenderer
    scene, cam, view, iv = H.setup_scene(scenes.built_mesh_scene)
    r = VisibilityRenderer(0)
    r.set_cull_mode(hier)
    r.upload_scene(scene)                                                         # (validates the builder's BVH)
    r.allocate_gbuffer(cam.width, cam.height)
    r.set_view(view, iv, H.ALL_FLAGS)
    assert np.array_equal(r.read_cmds(r.instance_culling()), orc.instance_culling(scene, view, iv, H.ALL_FLAGS))
    prev = None
    for frame in range(2):
        r.render_frame()
        want = orc.frame(scene, view, iv, H.ALL_FLAGS, prev_hzb_min=prev)
        H.assert_vis_equal(r.read_visibility(), want["vis"], cam.width, cam.height, "built meshes, frame %d" % frame)
        prev = want["hzb_min"]
    r.close()


# ---- the builder's meshlet bounds against the REFERENCE's (vendored meshoptimizer, tests/golden/meshopt_bounds.json) ---------
def _cone_culls(apex, axis, cutoff, cam):
    """nanite_shared.hlsli:65-75 / meshopt convention: culled iff dot(normalize(apex - cam), axis) >= cutoff."""
    v = apex - cam
    n = np.linalg.norm(v)
    return n > 0 and float(np.dot(v / n, axis)) >= cutoff


def test_meshlet_bounds_against_the_reference_meshoptimizer_fixture():
    """207 meshlets built by the reference's own meshopt_buildMeshlets (two bumpy spheres, a cube) with the bounds its
    meshopt_computeMeshletBounds gives them (fixture: make_meshopt_fixture.sh compiles the vendored sources in the build
    container).  chordvis_meshlet_bounds -- what chordvis_nanite_build stores -- must
      * be SAFE: a camera position its cone culls sees every triangle of the meshlet from behind (ground truth, the property
        the runtime's cone test relies on; the reference's cone is held to the same bar to validate the sampling);
      * be as conservative as the reference's cone where both are cones: it never culls a sampled camera the reference keeps;
      * stay near it: axis within half a degree, and the AABB containing the reference's bounding sphere centre."""
    import ctypes as C
    import json
    import os
    from chord_amd import lib as L, records as R
    fx = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "meshopt_bounds.json")))
    rng = np.random.default_rng(7)
    dirs = rng.normal(size=(96, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    checked = cones = stricter = 0
    worst_angle = 0.0
    for mesh in fx["meshes"]:
        for ml in mesh["meshlets"]:
            pos = np.asarray(ml["positions"], np.float32).reshape(-1, 3)
            tri = np.asarray(ml["triangles"], np.uint8).reshape(-1, 3)
            out = np.zeros(1, dtype=R.MESHLET)
            assert L.lib.chordvis_meshlet_bounds(pos.ctypes.data, len(pos), tri.ctypes.data, len(tri), out.ctypes.data) == 0
            m = out[0]
            assert np.allclose(m["posMin"], pos.min(axis=0)) and np.allclose(m["posMax"], pos.max(axis=0))
            rc, rr = np.asarray(ml["center"], np.float64), ml["radius"]
            assert (rc >= m["posMin"] - 1e-5).all() and (rc <= m["posMax"] + 1e-5).all()
            axis, apex, cutoff = m["coneAxis"].astype(np.float64), m["coneApex"].astype(np.float64), float(m["coneCutOff"])
            raxis, rapex, rcut = np.asarray(ml["cone_axis"]), np.asarray(ml["cone_apex"]), ml["cone_cutoff"]
            p64 = pos.astype(np.float64)
            a, b, c = p64[tri[:, 0]], p64[tri[:, 1]], p64[tri[:, 2]]
            nrm = np.cross(b - a, c - a)
            keep = np.linalg.norm(nrm, axis=1) > 0
            nrm, a = nrm[keep], a[keep]
            if rcut < 1.0 and cutoff < 1.0:
                cones += 1
                ang = np.degrees(np.arccos(np.clip(np.dot(axis, raxis) / (np.linalg.norm(axis) * np.linalg.norm(raxis)), -1, 1)))
                worst_angle = max(worst_angle, ang)
            ext = float(np.linalg.norm(m["posMax"] - m["posMin"]))
            for d in dirs:
                for dist in (0.6 * ext, 2.0 * ext, 50.0 * ext):
                    cam = rc + d * (rr + dist)
                    front = (np.einsum("ij,ij->i", nrm, cam[None, :] - a) > 1e-9 * ext * ext).any()    # some triangle faces the camera
                    ours = _cone_culls(apex, axis, cutoff, cam) if cutoff < 1.0 else False
                    ref = _cone_culls(rapex, raxis, rcut, cam) if rcut < 1.0 else False
                    checked += 1
                    assert not (ours and front), "the builder's cone culls a camera that sees a front face (%s)" % mesh["name"]
                    assert not (ref and front), "sampling check: the reference's cone culls a visible meshlet?"
                    if ours and not ref:
                        stricter += 1
    assert cones >= 150 and checked > 50000
    assert worst_angle <= 0.5, worst_angle
    assert stricter == 0, "%d of %d sampled cameras are culled by the builder's cone but kept by meshoptimizer's" % (stricter, checked)


def test_obj_reader_round_trip_and_build(tmp_path):
    """chord_amd/obj.py: the OBJ a user would drop in (v / vt / f, polygons, negative indices, a seam) reaches the builder:
    written and read back it is the same mesh, quads are fan-triangulated, relative indices resolve, a position used with two
    different texture coordinates is split -- and chordvis_nanite_build takes the result."""
    from chord_amd import lib as L, obj
    pos, idx, uv = scenes.bumpy_sphere_mesh(24, 1)
    path = str(tmp_path / "sphere.obj")
    obj.write_obj(path, pos, idx, uv)
    p2, i2, uv2 = obj.read_obj(path)
    # (vertices are renumbered in order of first use: the same triangles, corner for corner)
    assert len(i2) == len(idx) and np.allclose(p2[i2], pos[idx], atol=1e-6) and np.allclose(uv2[i2], uv[idx], atol=1e-6)
    assert len(p2) == len(pos)
    quad = tmp_path / "quad.obj"
    quad.write_text("# a quad with relative indices and a uv seam on its first corner\n"
                    "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvt 0.5 0.5\n"
                    "f -4/1 -3/2 -2/3 -1/4\nf 1/5 3/3 2/2\n")
    p3, i3, uv3 = obj.read_obj(str(quad))
    assert len(i3) == 9 and len(p3) == 5                                     # quad -> 2 triangles, + 1 triangle; vertex 1 split by its second vt
    assert np.array_equal(i3[:6], [0, 1, 2, 0, 2, 3]) and np.allclose(uv3[4], [0.5, 0.5]) and np.allclose(p3[4], p3[0])
    built = L.nanite_build(p2, i2, uv2)
    tri = int(((built.meshlets["vertexTriangleCount"] >> 8) & 0xFF)[built.meshlets["lod"] == 0].sum())
    assert tri == len(idx) // 3


@pytest.mark.gpu
def test_quarter_million_triangle_built_mesh_renders_like_the_oracle(gpu):
    """A 258 k-triangle mesh (Sponza-class, SURVEY 8d config 2's size) through chordvis_nanite_build -- 7.5 k LOD-0 meshlets,
    its full LOD DAG and BVH -- instanced near, mid-range and far: command lists of both cull modes and two frames (first /
    two-pass HZB) against the oracle."""
    from chord_amd.renderer import VisibilityRenderer
    scene, cam, view, iv = H.setup_scene(scenes.big_built_mesh_scene)
    assert int(((scene.meshlets["vertexTriangleCount"] >> 8) & 0xFF)[scene.meshlets["lod"] == 0].sum()) > 250000
    want_cmds = orc.instance_culling(scene, view, iv, H.ALL_FLAGS)
    for hier in (0, 1):
        r = VisibilityRenderer(0)
        r.set_cull_mode(hier)
        r.upload_scene(scene)
        r.allocate_gbuffer(cam.width, cam.height)
        r.set_view(view, iv, H.ALL_FLAGS)
        assert np.array_equal(r.read_cmds(r.instance_culling()), want_cmds)
        prev = None
        for frame in range(2):
            r.render_frame()
            want = orc.frame(scene, view, iv, H.ALL_FLAGS, prev_hzb_min=prev)
            H.assert_vis_equal(r.read_visibility(), want["vis"], cam.width, cam.height, "258 k-triangle built mesh, cull mode %d, frame %d" % (hier, frame))
            prev = want["hzb_min"]
        assert r.stats()["overflow"] == 0
        r.close()


# ---- the reference's own asset container (GLTFBinary: cereal binary archive + LZ4, serialize.h:217-320) -------------------
GLTF_FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load_gltf_binary(path):
    h = C.c_void_p()
    rc = L.lib.chordvis_load_gltf_binary(path.encode(), C.byref(h))
    assert rc == L.OK, rc
    try:
        return L.BuiltAsset(h)
    finally:
        L.lib.chordvis_free_built_asset(h)


@pytest.mark.parametrize("name", ["gltf_binary_raw.bin", "gltf_binary_lz4.bin"])
def test_gltf_binary_written_by_the_references_cereal_and_lz4_is_read(name):
    """tests/golden/gltf_binary_{raw,lz4}.bin were written by the reference's vendored cereal + LZ4 through structs that
    mirror GLTFBinary / GLTFMeshlet / GLTFMeshletGroup / GLTFBVHNode member by member (make_gltf_binary_fixture.cpp); the
    library's reader -- its own restatement of both formats -- must find every value the generator put in."""
    want = json.load(open(os.path.join(GLTF_FIX, "gltf_binary.json")))
    a = _load_gltf_binary(os.path.join(GLTF_FIX, name))
    assert np.array_equal(a.positions.reshape(-1), np.array(want["positions"], np.float32))
    assert np.array_equal(a.texcoord0.reshape(-1), np.array(want["texcoords0"], np.float32))
    assert np.array_equal(a.meshlet_data, np.array(want["meshletDatas"], np.uint32))
    assert np.array_equal(a.group_indices, np.array(want["meshletGroupIndices"], np.uint32))
    assert len(a.meshlets) == len(want["meshlets"]) and len(a.groups) == len(want["meshletGroups"]) and len(a.bvh_nodes) == len(want["bvhNodes"])
    for m, w in zip(a.meshlets, want["meshlets"]):          # JSON order = MEMORY order of GPUGLTFMeshlet (the archive permutes it)
        got = list(m["posMin"]) + [m["dataOffset"]] + list(m["posMax"]) + [m["vertexTriangleCount"]] + list(m["coneAxis"]) + [m["coneCutOff"]] + list(m["coneApex"]) + [m["lod"]]
        assert np.array_equal(np.array(got, np.float64), np.array([np.float32(x) if isinstance(x, float) else x for x in w], np.float64))
    for g, w in zip(a.groups, want["meshletGroups"]):
        got = list(g["clusterPosCenter"]) + [g["parentError"]] + list(g["parentPosCenter"]) + [g["error"], g["meshletOffset"], g["meshletCount"]]
        assert np.array_equal(np.array(got, np.float64), np.array([np.float32(x) if isinstance(x, float) else x for x in w], np.float64))
    for b, w in zip(a.bvh_nodes, want["bvhNodes"]):
        got = list(b["sphere"]) + list(b["children"]) + [b["bvhNodeCount"], b["leafMeshletGroupOffset"], b["leafMeshletGroupCount"]]
        assert np.array_equal(np.array(got, np.float64), np.array([np.float32(x) if isinstance(x, float) else x for x in w], np.float64))
    assert a.primitive["vertexCount"][0] == want["vertexCount"] and a.primitive["meshletGroupCount"][0] == len(want["meshletGroups"])


def test_gltf_binary_round_trip_of_a_built_asset(tmp_path):
    """A built asset through chordvis_save_gltf_binary (uncompressed and with the library's own LZ4 encoder) and back: the
    arrays the path reads are identical; truncated and corrupted files are refused."""
    pos, idx, _ = scenes.bumpy_sphere_mesh(48, 3)
    h = L.nanite_build(pos, idx, keep_handle=True)
    ref = L.BuiltAsset(h)
    sizes = {}
    for lz4 in (0, 1):
        path = str(tmp_path / ("a%d.assetbin" % lz4))
        assert L.lib.chordvis_save_gltf_binary(h, path.encode(), lz4) == L.OK
        sizes[lz4] = os.path.getsize(path)
        a = _load_gltf_binary(path)
        for f in ("meshlets", "groups", "group_indices", "meshlet_data", "positions", "bvh_nodes"):
            assert np.array_equal(getattr(a, f), getattr(ref, f)), f
        assert a.lod_count == ref.lod_count and a.primitive["vertexCount"][0] == ref.primitive["vertexCount"][0]
        assert np.array_equal(a.primitive["posMin"], ref.primitive["posMin"]) and np.array_equal(a.primitive["posMax"], ref.primitive["posMax"])
    assert sizes[1] < 0.9 * sizes[0]                               # (indices and repeated words compress)
    L.lib.chordvis_free_built_asset(h)
    data = open(str(tmp_path / "a1.assetbin"), "rb").read()
    for bad in (data[:len(data) // 2], data[:40] + bytes([data[40] ^ 0xFF]) + data[41:], b"", data + b"x"):
        p = str(tmp_path / "bad.assetbin")
        open(p, "wb").write(bad)
        h2 = C.c_void_p()
        rc = L.lib.chordvis_load_gltf_binary(p.encode(), C.byref(h2))
        if rc == L.OK:                                             # (a flipped literal byte still decodes: then the values differ, nothing crashes)
            L.lib.chordvis_free_built_asset(h2)
        else:
            assert rc == L.E_INVALID


def test_gltf_binary_uncompressed_file_is_byte_identical_to_cereals(tmp_path):
    """Loading the reference-written fixture and saving it again uncompressed reproduces cereal's bytes except for the
    attributes this path drops (normals / tangents / LOD-0 indices are written empty): checked by re-reading both."""
    a_path = os.path.join(GLTF_FIX, "gltf_binary_raw.bin")
    h = C.c_void_p()
    assert L.lib.chordvis_load_gltf_binary(a_path.encode(), C.byref(h)) == L.OK
    out = str(tmp_path / "again.bin")
    assert L.lib.chordvis_save_gltf_binary(h, out.encode(), 0) == L.OK
    L.lib.chordvis_free_built_asset(h)
    a, b = _load_gltf_binary(a_path), _load_gltf_binary(out)
    for f in ("meshlets", "groups", "group_indices", "meshlet_data", "positions", "texcoord0", "bvh_nodes"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    # the sections both files hold are the same bytes: header of the archive + positions
    ra, rb = open(a_path, "rb").read(), open(out, "rb").read()
    n = 24 + 4 + 8 + 150 * 12
    assert ra[16:24] != rb[16:24] and ra[24:n] == rb[24:n]         # (string length differs, version tag + positions identical)


def test_gltf_binary_written_by_the_library_is_read_by_the_references_cereal_and_lz4(tmp_path):
    """The other direction: files the LIBRARY writes (its own cereal layout, its own LZ4 encoder) through loadAsset's sequence
    built from the vendored cereal + LZ4 (make_gltf_binary_fixture --check).  That reader ran over the library's files of the
    mesh in tests/golden/gltf_library_mesh.npz (make_gltf_library_fixture.py); gltf_library_check.json holds each file's size and
    SHA-1 with what the reader reported.  The library must write exactly those bytes today, and the report must match its asset."""
    import hashlib
    fix = json.load(open(os.path.join(GLTF_FIX, "gltf_library_check.json")))
    mesh = np.load(os.path.join(GLTF_FIX, fix["mesh"]))
    pos, idx, uv = mesh["positions"], mesh["indices"], mesh["texcoords0"]
    h = L.nanite_build(pos, idx, uv, keep_handle=True)
    a = L.BuiltAsset(h)
    hh = 1469598103934665603

    def mix(v):
        nonlocal hh
        hh = ((hh ^ int(v)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    for m in a.meshlets:
        mix(m["dataOffset"]); mix(m["vertexTriangleCount"]); mix(m["lod"]); mix(np.float32(m["coneCutOff"]).view(np.uint32)); mix(np.float32(m["coneAxis"][0]).view(np.uint32))
    for v in a.meshlet_data: mix(v)
    for b in a.bvh_nodes:
        mix(b["bvhNodeCount"]); mix(b["leafMeshletGroupOffset"]); mix(b["leafMeshletGroupCount"]); mix(b["children"][7])
    for g in a.groups:
        mix(g["meshletOffset"]); mix(g["meshletCount"]); mix(np.float32(g["parentError"]).view(np.uint32))
    for v in a.group_indices: mix(v)
    for lz4, rec in zip((0, 1), fix["files"]):
        assert rec["lz4"] == lz4
        path = str(tmp_path / ("w%d.bin" % lz4))
        assert L.lib.chordvis_save_gltf_binary(h, path.encode(), lz4) == L.OK
        data = open(path, "rb").read()
        assert len(data) == rec["bytes"] and hashlib.sha1(data).hexdigest() == rec["sha1"], "the library no longer writes the bytes the reference read"
        out = rec["reference_check"].split()
        assert out[0] == "OK" and int(out[2]) == lz4, out
        kv = dict(zip(out[1::2], out[2::2]))
        assert int(kv["positions"]) == len(a.positions) and int(kv["texcoords0"]) == len(a.texcoord0) and int(kv["meshlets"]) == len(a.meshlets)
        assert int(kv["meshletDatas"]) == len(a.meshlet_data) and int(kv["bvhNodes"]) == len(a.bvh_nodes) and int(kv["groups"]) == len(a.groups)
        assert int(kv["hash"]) == hh, (kv["hash"], hh)
    L.lib.chordvis_free_built_asset(h)
