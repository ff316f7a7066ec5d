"""Test-local scenes of the material feedback tests (tests/test_material_feedback_spec.py checks on the CPU that they hold what
tests/test_gpu_material_feedback.py relies on).  TEST INFRASTRUCTURE: never imported by chord_amd/."""
import math

import numpy as np

from chord_amd import records as R, scenes

SIZE = 64                                        # both scenes are rendered at 64 x 64
NO_TEXTURE = 0xFFFFFFFF


def _noise(w, h, seed):
    return (scenes.pcg_hash(np.arange(w * h * 4, dtype=np.uint32) + np.uint32(seed * 7919)) & 0xFF).astype(np.uint8).reshape(h, w, 4)


def _camera():
    """looks down -z at the square [-1, 1]^2 of the plane z = 0, which fills the 64 x 64 image"""
    return scenes.Camera((0.0, 0.0, 1.0 / math.tan(math.radians(22.5))), (0.0, 0.0, -1.0), SIZE, SIZE)


def _quad(sb, uv_scale):
    pb = scenes.PrimitiveBuilder(sb.attributes)
    pb.uv_scale = uv_scale
    pb.add_surface(scenes.plane_surface((-0.5, -0.5, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)), 1, 1, 1)
    return sb.add_primitive(pb)


# texture ids of quads_scene
T_SHARED, T_TWO_SLOTS, T_BIG, T_TWO_LEVELS, T_UNNAMED, T_NON_PBR, T_NO_MIP_FILTER = range(7)


def quads_scene():
    """16 x 16 quads of about 4 x 4 pixels under eight materials that change from quad to quad, so that a 16 x 4 block of pixels
    holds four of them: two materials share T_SHARED, one names T_TWO_SLOTS in two slots, one is not PBR (T_NON_PBR is named by it
    alone), T_UNNAMED is named by nobody, T_NO_MIP_FILTER's sampler has no mip filter, T_BIG's is *_MIPMAP_NEAREST over quads of
    four texture scales, T_TWO_LEVELS has two levels and is minified well past them.  No normals, no tangents."""
    sb = scenes.SceneBuilder("feedback_quads", False)
    two = np.concatenate([_noise(64, 64, 4).reshape(-1), _noise(32, 32, 5).reshape(-1)])
    for t in (_noise(64, 64, 1), _noise(32, 32, 2), _noise(128, 128, 3), R.TextureChain(two, 64, 64, 2), _noise(8, 8, 6), _noise(16, 16, 7),
              _noise(16, 16, 8)):
        sb.add_texture(t) if not isinstance(t, R.TextureChain) else sb.textures.append(t)
    tri = sb.add_sampler(R.FILTER_LINEAR_MIPMAP_LINEAR, R.FILTER_LINEAR)
    lmn = sb.add_sampler(R.FILTER_LINEAR_MIPMAP_NEAREST, R.FILTER_NEAREST, R.WRAP_MIRRORED_REPEAT, R.WRAP_CLAMP_TO_EDGE)
    nml = sb.add_sampler(R.FILTER_NEAREST_MIPMAP_LINEAR, R.FILTER_LINEAR, R.WRAP_REPEAT, R.WRAP_MIRRORED_REPEAT)
    lin = sb.add_sampler(R.FILTER_LINEAR, R.FILTER_LINEAR, R.WRAP_CLAMP_TO_EDGE, R.WRAP_REPEAT)
    mats = [sb.add_material(1, 0, T_SHARED, tri, pbr=True),
            sb.add_material(1, 0, T_SHARED, nml, pbr=True, metallic_roughness=(T_BIG, tri)),
            sb.add_material(1, 0, T_TWO_SLOTS, tri, pbr=True, emissive=(T_TWO_SLOTS, lmn), emissive_factor=(1.0, 1.0, 1.0)),
            sb.add_material(1, 0, T_BIG, lmn, pbr=True),
            sb.add_material(1, 0, T_TWO_LEVELS, tri, pbr=True),
            sb.add_material(1, 0, T_NON_PBR, tri, pbr=True, material_type=0),
            sb.add_material(1, 0, T_NO_MIP_FILTER, lin, pbr=True),
            sb.add_material(1, 0, pbr=True, roughness_factor=0.5)]
    prims = [_quad(sb, s) for s in ((1.0 / 16.0, 1.0 / 16.0), (0.25, 0.5), (1.0, 1.0), (4.0, 16.0))]
    n, cell = 16, 2.0 / 16
    for j in range(n):
        for i in range(n):
            m = scenes.translate(-1.0 + (i + 0.5) * cell, -1.0 + (j + 0.5) * cell, 0.0)
            if (i + j) % 5 == 0:
                m = m @ scenes.rotate_y(1.0)                                  # (a quad seen at an angle: an anisotropic footprint)
            sb.add_object(prims[(i // 4 + j) % 4], m @ scenes.scale(0.85 * cell), material=mats[(i + 2 * j) % 8])
    return sb.build(), _camera()


# texture ids of loop_scene
T_NEAR, T_FAR, T_TILTED = range(3)


def loop_scene():
    """Three strips under power-of-two textures and samplers whose min and mag filters agree on nearest versus bilinear: T_NEAR
    magnified, T_FAR (256 x 256, three repeats over a third of the image) seen only minified by four to five levels, T_TILTED on a
    plane that recedes from the camera (levels 3 and 4 at N = 1, 1 to 3 at N = 16).  With normals and tangents."""
    sb = scenes.SceneBuilder("feedback_loop", True)
    for t in (_noise(64, 64, 11), _noise(256, 256, 12), _noise(128, 128, 13)):
        sb.add_texture(t)
    tri = sb.add_sampler(R.FILTER_LINEAR_MIPMAP_LINEAR, R.FILTER_LINEAR)
    nmn = sb.add_sampler(R.FILTER_NEAREST_MIPMAP_NEAREST, R.FILTER_NEAREST, R.WRAP_MIRRORED_REPEAT, R.WRAP_REPEAT)
    lmn = sb.add_sampler(R.FILTER_LINEAR_MIPMAP_NEAREST, R.FILTER_LINEAR, R.WRAP_REPEAT, R.WRAP_CLAMP_TO_EDGE)
    near = sb.add_material(1, 0, T_NEAR, tri, pbr=True, emissive=(T_NEAR, lmn), emissive_factor=(1.0, 0.5, 0.25))
    far = sb.add_material(1, 0, T_FAR, tri, pbr=True, metallic_roughness=(T_FAR, lmn), occlusion_strength=0.5)
    tilted = sb.add_material(1, 0, T_TILTED, nmn, pbr=True, normal=(T_TILTED, lmn), normal_scale=1.0)
    sb.add_object(_quad(sb, (0.25, 0.25)), scenes.translate(-0.68, 0.0, 0.0) @ scenes.scale(0.62, 1.9, 1.0), material=near)
    sb.add_object(_quad(sb, (3.0, 9.0)), scenes.translate(0.0, 0.0, 0.0) @ scenes.scale(0.62, 1.9, 1.0), material=far)
    sb.add_object(_quad(sb, (2.0, 6.0)), scenes.translate(0.75, 0.0, 0.3) @ scenes.rotate_y(-1.3) @ scenes.scale(3.5, 1.9, 1.0), material=tilted)
    return sb.build(), _camera()


def first_levels(taps):
    """per texture the lowest level with a non-zero count (0 for a row of zeros): what a host would trim to"""
    taps = np.asarray(taps)
    return [int(np.flatnonzero(row)[0]) if row.any() else 0 for row in taps]


def quads_scene_conditions(scene, st, w, h):
    """the conditions of the issue's test 5 that do NOT hold (shared with the GPU test, which asserts the list is empty)"""
    import spec_material_feedback_np as SF
    missing = []
    taps = SF.feedback_of(st, scene, w)
    mat = np.where(st["hit"], st["material"], -1).reshape(h, w)
    most = max(len(np.unique(b[b >= 0])) for y in range(0, h, 4) for x in range(0, w, 16) for b in [mat[y:y + 4, x:x + 16]])
    if most < 4:
        missing.append("a 16 x 4 block with four materials (most: %d)" % most)
    if max(np.count_nonzero(row) for row in taps) < 3:
        missing.append("a texture with taps on three levels")
    two = taps[T_TWO_LEVELS]
    lods = np.concatenate([s["lodq"] for s in st["slots"]["baseColor"] if int(scene.materials[s["material"]]["baseColorId"]) == T_TWO_LEVELS])
    if not (two[1] > 0 and not two[2:].any() and np.any(lods >= 3 * 256)):
        missing.append("taps of the two-level texture clamped to its last level")
    if taps[T_UNNAMED].any() or taps[T_NON_PBR].any():
        missing.append("zero rows for the unnamed texture and the non-PBR material's")
    non_pbr = [m for m in range(len(scene.materials)) if int(scene.materials[m]["baseColorId"]) == T_NON_PBR]
    if not np.any(np.isin(mat, non_pbr)):
        missing.append("visible pixels of the non-PBR material")
    if taps[T_NO_MIP_FILTER, 1:].any() or not taps[T_NO_MIP_FILTER, 0]:
        missing.append("the sampler without a mip filter on level 0 alone")
    shared = [s["material"] for s in st["slots"]["baseColor"] if int(scene.materials[s["material"]]["baseColorId"]) == T_SHARED]
    if len(set(shared)) < 2:
        missing.append("two visible materials sharing a texture")
    if not any(int(scene.materials[s["material"]]["emissiveTexture"]) == T_TWO_SLOTS for s in st["slots"]["emissive"]):
        missing.append("a texture in two slots of one material")
    return missing
