"""Scenes, ray sets and hit lists for the specification of shading ray hits (tests/spec_ray_shade_np.py), used by
tests/test_ray_shade_spec.py and meant for the GPU test of the kernel that is to follow: everything here runs without a device.  TEST INFRASTRUCTURE: never imported by chord_amd/."""
import functools

import numpy as np

from chord_amd import lib as L, records as R, scenes

import spec_rays_np as S
import spec_ray_shade_np as RS

F = np.float32
PW, PH = 64, 40
LODS = (0.0, 0.5, 2.25, 20.0)


def triangle_scene():
    """One triangle with texture coordinates beyond [0, 1] and three different vertex normals, as four objects: a trilinear
    one-sided material with base colour, emissive and metallic-roughness textures; a two-sided nearest-mip material without a
    metallic-roughness texture; a material without textures; a material of another materialType.  Object 1 is mirrored and stretched."""
    sb = scenes.SceneBuilder("ray_shade_triangle", True)
    rng = np.random.default_rng(5)
    tex = [sb.add_texture(rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)) for w, h in ((16, 8), (5, 3), (8, 8))]
    tri = sb.add_sampler(R.FILTER_LINEAR_MIPMAP_LINEAR, R.FILTER_LINEAR, R.WRAP_REPEAT, R.WRAP_MIRRORED_REPEAT)
    nmn = sb.add_sampler(R.FILTER_NEAREST_MIPMAP_NEAREST, R.FILTER_NEAREST, R.WRAP_CLAMP_TO_EDGE, R.WRAP_REPEAT)
    lin = sb.add_sampler(R.FILTER_LINEAR, R.FILTER_NEAREST, R.WRAP_MIRRORED_REPEAT, R.WRAP_CLAMP_TO_EDGE)
    mats = [sb.add_material(0, 0, tex[0], tri, pbr=True, emissive=(tex[1], lin), emissive_factor=(1.0, 0.5, 2.0), metallic_roughness=(tex[2], tri),
                            base_color_factor=(0.9, 0.8, 0.7)),
            sb.add_material(1, 0, tex[1], nmn, pbr=True, emissive=(tex[0], nmn), emissive_factor=(0.25, 0.25, 0.25), roughness_factor=0.35,
                            metallic_factor=1.0),
            sb.add_material(1, 0, pbr=True, roughness_factor=0.6, metallic_factor=0.25, base_color_factor=(0.5, 0.25, 0.125), emissive_factor=(1.0, 1.0, 1.0)),
            sb.add_material(0, 0, tex[0], tri, pbr=True, material_type=0)]
    pos = np.array([(0, 0, 0), (2, 0, 0), (0, 1.5, 0.5)], dtype=np.float32)
    m = np.zeros(1, dtype=R.MESHLET)
    m["posMin"], m["posMax"], m["coneCutOff"], m["vertexTriangleCount"] = pos.min(axis=0), pos.max(axis=0), 1.0, 3 | (1 << 8)
    groups = np.zeros(1, dtype=R.MESHLET_GROUP)
    groups["error"], groups["parentError"], groups["meshletCount"] = -1.0, scenes.FLT_MAX, 1
    groups, nodes = scenes.build_bvh(groups)
    nrm = np.array([(0.1, 0.2, 1.0), (-0.6, 0.1, 0.7), (0.0, -0.8, 0.5)], dtype=np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True).astype(np.float32)
    sb.prims.append(dict(bvh_nodes=nodes, positions=pos, texcoords=np.array([(-0.3, 0.2), (2.6, 0.4), (0.5, -1.7)], dtype=np.float32),
                         normals=nrm, tangents=np.tile(np.array([(1.0, 0.0, 0.0, 1.0)], dtype=np.float32), (3, 1)), meshlets=m,
                         meshlet_data=np.array([0, 1, 2, 0 | (1 << 8) | (2 << 16)], dtype=np.uint32), groups=groups,
                         group_indices=np.zeros(1, dtype=np.uint32)))
    sb.add_object(0, scenes.translate(-1.0, 0.0, -4.0), material=mats[0])
    sb.add_object(0, scenes.translate(1.5, 0.2, -5.0) @ scenes.rotate_y(0.4) @ scenes.scale(-1.0, 2.5, 0.5), material=mats[1])
    sb.add_object(0, scenes.translate(-2.0, 1.0, -6.0) @ scenes.rotate_y(-0.3), material=mats[2])
    sb.add_object(0, scenes.translate(0.5, -1.0, -3.0), material=mats[3])
    scene = sb.build()
    cam = scenes.Camera((0.0, 0.5, 1.0), (0.0, 0.0, -1.0), PW, PH)
    L.fill_objects(scene, cam)
    return scene, cam


def hit(obj, u, v, status=1, meshlet=0, triangle=0, t=1.0, prim=0):
    h = np.zeros(1, dtype=R.RAY_HIT)
    h["t"], h["u"], h["v"], h["object"], h["meshlet"], h["triangle"], h["primitive"], h["status"] = t, u, v, obj, meshlet, triangle, prim, status
    return h


def invalid_hits(scene):
    """[(what, hit)] -- one per rule of the header, each one step past its range and at 0xFFFFFFFF"""
    big = 0xFFFFFFFF
    out = [("a miss", hit(0, 0.2, 0.2, status=0)), ("status 2 alone", hit(0, 0.2, 0.2, status=2))]
    for what, val in (("NaN", np.nan), ("inf", np.inf), ("-inf", -np.inf)):
        out += [("u " + what, hit(0, val, 0.2)), ("v " + what, hit(0, 0.2, val))]
    for v in (len(scene.objects), big):
        out.append(("object %#x" % v, hit(v, 0.2, 0.2)))
    for v in (len(scene.meshlets), big):
        out.append(("meshlet %#x" % v, hit(0, 0.2, 0.2, meshlet=v)))
    for v in (1, 128, big):
        out.append(("triangle %#x" % v, hit(0, 0.2, 0.2, triangle=v)))
    return out


def random_rays(scene, n, seed, objects=slice(None)):
    """tests/test_gpu_rays.py's _random_rays: origins in the box of the scene's objects (or of some of them), any direction, every fifth
    ray short."""
    lo, hi = S.object_boxes(scene.objects[objects], scene.primitives)
    lo, hi = lo.min(axis=0).astype(np.float64), hi.max(axis=0).astype(np.float64)
    r = scenes.rand01(seed, np.arange(7 * n)).reshape(n, 7)
    d = r[:, 3:6] * 2.0 - 1.0
    rays = S.make_rays(lo + r[:, :3] * (hi - lo), d, 1e-2, 1e9)
    rays["tMax"][::5] = (r[::5, 6] * np.linalg.norm(hi - lo)).astype(F)
    return rays


def _material():
    return scenes.material_test_scene(PW, PH)


def _general():
    scene, cam, _ = scenes.general_transform_scene(PW, PH, materials=True)
    return scene, cam


def _masked():
    return scenes.masked_test_scene(PW, PH, attributes=True)


def _built():
    return scenes.built_mesh_scene(PW, PH, n=48, attributes=True)


SCENES = {"material": _material, "general": _general, "masked": _masked, "built_mesh": _built}
# the random rays' seed and the objects whose box they start in, chosen on the CPU so that vacuity() holds for the specification: the
# built meshes' scene is 400 m deep and its near spheres are what a ray can meet from inside (the front faces of one-sided objects)
RANDOM = {"material": (23, slice(None)), "general": (25, slice(None)), "masked": (23, slice(None)), "built_mesh": (23, slice(0, 3))}
PBR_SCENES = ("material", "general")             # the scenes whose materials are scenes._pbr_materials'


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene with records filled, camera, view, iv, rays): the pixel rays and 2 000 random ones -- computed once, read-only."""
    scene, cam = SCENES[name]()
    L.fill_objects(scene, cam)
    view, iv = L.make_views(cam)
    rays = np.concatenate([S.pixel_rays(view, PW, PH), random_rays(scene, 2000, *RANDOM[name])])
    rays.setflags(write=False)
    return scene, cam, view, iv, rays


def per_hit_lods(hits):
    """A level per hit that grows with t (a ray cone's footprint), with the special values a host may hand over mixed in."""
    with np.errstate(all="ignore"):
        lods = np.log2(np.maximum(hits["t"].astype(np.float64), 1e-3)).astype(F)
    lods[3::97] = np.nan
    lods[5::89] = np.inf
    lods[7::83] = -np.inf
    lods[11::79] = -1.0
    return lods


def lod_runs(hits):
    """[(label, lod, lods)]: the four uniform levels and the per-hit one"""
    return [("lod %g" % l, l, None) for l in LODS] + [("per-hit lod", 0.0, per_hit_lods(hits))]


def vacuity(scene, name, hits, runs):
    """The conditions a (scene, hit list) must meet for the comparison to mean something, from the specification's output alone.
    runs: [(surface records, stats)] of the lod runs.  Returns a list of failures (empty: fine)."""
    bad = []
    want = runs[0][0]
    valid = (want["flags"] & RS.RAYSURF_VALID) != 0
    if 5 * int(valid.sum()) < len(hits):
        bad.append("%d of %d rays hit: fewer than a fifth" % (valid.sum(), len(hits)))
    if name in PBR_SCENES:
        # scenes._pbr_materials' six, behind the builder's default material 0: every one that an object of the scene names (the material
        # scene names all six, the general one four)
        for m in sorted(set(range(1, 7)) & set(int(x) for x in scene.objects["GLTFMaterialData"])):
            n = int((valid & (want["material"] == m)).sum())
            if n < 16:
                bad.append("material %d is met by %d hits" % (m, n))
    for back in (0, RS.RAYSURF_BACK_FACE):
        for two in (0, RS.RAYSURF_TWO_SIDED):
            if not (valid & ((want["flags"] & (RS.RAYSURF_BACK_FACE | RS.RAYSURF_TWO_SIDED)) == (back | two))).any():
                bad.append("no hit with BACK_FACE %d and TWO_SIDED %d" % (back != 0, two != 0))
    # per mip-filtered (material, slot): two levels over the runs; where the filter blends levels (*_MIPMAP_LINEAR), an l1 != l0 tap
    seen = {}
    for _, stats in runs:
        for st in stats["slots"]:
            if not st["mip_filtered"] or st["last"] == 0:
                continue
            e = seen.setdefault((st["material"], st["slot"]), [set(), False, st])
            e[0].update(int(l) for l in np.unique(st["l0"]))
            e[1] = e[1] or bool((st["l1"] != st["l0"]).any())
    for (m, slot), (levels, blend, st) in seen.items():
        levels_ok = len(levels) >= 2
        tex, smp = RS.SM._TEX_FIELD[slot]
        linear_mips = int(scene.samplers[int(scene.materials[m][smp])]["minFilter"]) in (RS.SM.NEAREST_MIPMAP_LINEAR, RS.SM.LINEAR_MIPMAP_LINEAR)
        if not levels_ok:
            bad.append("material %d slot %s samples only level(s) %s" % (m, slot, sorted(levels)))
        if linear_mips and not blend:
            bad.append("material %d slot %s never blends two levels" % (m, slot))
    return bad


def shade_runs(scene, objects, hits):
    """[(label, lod, lods, want, stats)] of lod_runs through the specification"""
    out = []
    for label, lod, lods in lod_runs(hits):
        stats = {}
        out.append((label, lod, lods, RS.shade(scene, objects, hits, lod=lod, lods=lods, stats=stats), stats))
    return out
