"""Scenes, images, tables and descs for the specification of chordvis_pixel_rays (tests/spec_pixel_rays_np.py), shared by
tests/test_pixel_rays_spec.py, tests/test_pixel_rays_host.py and tests/test_gpu_pixel_rays.py: everything here runs without a device and
is computed once.  TEST INFRASTRUCTURE: never imported by chord_amd/.

Scenes: the triangle and material scenes of tests/ray_shade_cases.py and scenes.small_test_scene with attributes (eight objects: a TLAS
of more than one node).  Images of a (scene, size):
    frame     positionRS, vertexNormal and the depth halves of the visibility words of the scene's own frame at that size -- the
              oracle's frame through tests/spec_resolve_np.py and tests/spec_surface_np.py.
    synthetic the frame's images changed by a seeded generator: most positions lifted off their surface along the normal by 0.02 to
              0.06, the normals scaled by 0.25 to 4 (unnormalised) and most of them turned round -- a ray about a normal that points
              into the surface meets that surface from above, which is what makes hits in scenes whose objects stand far apart -- and,
              where the image has the pixels for them, normals (0, 0, 0), (0, 0, +-1), (1, 0, 0), (0, 0, 1e-30) and NaN, depths of 0
              with a position.w of 0, and positions with an inf and a NaN word.
    1 x 1     one pixel of the scene's 19 x 13 synthetic image, chosen from the specification's answer there under a 1 x 1 table: one
              that hits inside rayLength where there is one.
Every mode runs under five depth settings -- no depth image; deviceZStride 1 and 2, each with and without START_FROM_DEPTH -- and the
sizes, tables and image kinds rotate over them so that every mode of every scene meets every size and every table."""
import functools

import numpy as np

from chord_amd import lib as L, scenes

import helpers as H
import orc
import ray_shade_cases as RC
import spec_pixel_rays_np as PR
import spec_rays_np as S
import spec_resolve_np as SR
import spec_surface_np as SS

F = np.float32
SIZES = ((1, 1), (8, 8), (19, 13), (64, 3), (7, 70))
FRAME_SIZES = ((19, 13),)                                     # the size at which every mode runs on the scene's own frame
TABLES = ((1, 1), (4, 2), (16, 16))
# name -> (mode, flags, hit records asked for)
MODES = {"hemisphere_closest": (PR.HEMISPHERE, 0, True), "hemisphere_any": (PR.HEMISPHERE, PR.ANY_HIT, False),
         "direction_closest": (PR.DIRECTION, 0, True), "direction_any": (PR.DIRECTION, PR.ANY_HIT, False),
         "direction_any_front": (PR.DIRECTION, PR.ANY_HIT | PR.FRONT_ONLY, False)}
# name -> (deviceZStride or 0: no depth image, START_FROM_DEPTH)
DEPTHS = {"no_depth": (0, False), "z1": (1, False), "z1_start": (1, True), "z2": (2, False), "z2_start": (2, True)}
RAY_LENGTH = {PR.HEMISPHERE: 0.1, PR.DIRECTION: 0.03}        # against lifts of 0.02 .. 0.06 (the direction is 1.3 long): some hits fall beyond it
FRONT_RAY_LENGTH = 0.04                                        # FRONT_ONLY traces fewer pixels: more of them hit
FRAME_RAY_LENGTH = 50.0                                        # the frame's own images: whatever else stands in the scene
T_MIN = 1e-3


def _small():
    return scenes.small_test_scene(RC.PW, RC.PH, lods=3, attributes=True)


SCENES = {"triangle": RC.triangle_scene, "material": lambda: RC.case("material")[:2], "small": _small}


@functools.lru_cache(maxsize=None)
def scene(name):
    """(scene with records filled, camera, LOD-0 triangles)"""
    sc, cam = SCENES[name]()
    L.fill_objects(sc, cam)
    return sc, cam, S.lod0_triangles(sc)


def table(tw, th, seed=41):
    """(th, tw, 4) float32: unit directions with z >= 0 from a seeded generator; a texel with z = 0 and one with z = 1 where there is
    room for them"""
    rng = np.random.default_rng(seed + 97 * tw + th)
    z = rng.random(tw * th)
    phi = rng.random(tw * th) * 2.0 * np.pi
    r = np.sqrt(1.0 - z * z)
    t = np.stack([r * np.cos(phi), r * np.sin(phi), z, np.zeros(tw * th)], axis=1).astype(F)
    if tw * th >= 4:
        t[1] = (0.6, -0.8, 0.0, 0.0)
        t[tw * th - 2] = (0.0, 0.0, 1.0, 0.0)
    t.setflags(write=False)
    return t.reshape(th, tw, 4)


@functools.lru_cache(maxsize=None)
def frame_images(name, w, h):
    """(position (h, w, 4), normal (h, w, 4), z (h, w)) float32 of the scene's own frame at w x h"""
    sc, cam, _ = scene(name)
    c2 = scenes.Camera(cam.position, cam.front, w, h, world_up=cam.world_up, jitter=cam.jitter)
    view, iv = L.make_views(c2)
    fr = orc.frame(sc, view, iv, H.ALL_FLAGS)
    pos = SR.resolve(sc, fr["vis"], fr["cmds"], view, iv, w, h, names=("positionRS",))["positionRS"]
    nrm = SS.resolve(sc, fr["vis"], fr["cmds"], view, iv, w, h, names=("vertexNormal",))["vertexNormal"]
    z = (fr["vis"] >> np.uint64(32)).astype(np.uint32).view(F).reshape(h, w)
    for a in (pos, nrm, z):
        a.setflags(write=False)
    return pos, nrm, z


SPECIAL_NORMALS = ((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1e-30), (np.nan, 0.5, 0.5), (0.0, -2.0, 0.0))


@functools.lru_cache(maxsize=None)
def synthetic_images(name, w, h):
    pos, nrm, z = (a.copy() for a in frame_images(name, w, h))
    rng = np.random.default_rng(1000 * w + h)
    n = w * h
    p, q, zz = pos.reshape(n, 4), nrm.reshape(n, 4), z.reshape(n)
    unit = SS.normalize(q[:, :3])
    lift = np.where(rng.random(n) < 0.85, 0.02 + 0.04 * rng.random(n), 0.0).astype(F)
    p[:, :3] += unit * lift[:, None]
    q[:, :3] *= (0.25 * 16.0 ** rng.random(n)).astype(F)[:, None]
    q[rng.random(n) < 0.7, :3] *= F(-1.0)
    valid = np.flatnonzero(zz > 0)
    if len(valid) >= 24:
        # spread over the covered pixels: seven normals, two empty pixels, two non-finite positions
        at = valid[(np.arange(11) * len(valid)) // 11 + len(valid) // 22]
        for k, v in enumerate(SPECIAL_NORMALS):
            q[at[k], :3] = v
        zz[at[7]] = 0.0; p[at[7], 3] = 0.0
        zz[at[8]] = 0.0; p[at[8]] = 0.0
        p[at[9], 0] = np.inf
        p[at[10], 2] = np.nan
    for a in (pos, nrm, z):
        a.setflags(write=False)
    return pos, nrm, z


class Case:
    """One call: the images (host arrays), the table, the desc, and how the depth image lies in memory."""

    def __init__(self, name, scene_name, mode_name, depth_name, kind, position, normal, z, tab, desc, stride, hits):
        self.name, self.scene, self.mode_name, self.depth_name, self.kind = name, scene_name, mode_name, depth_name, kind
        self.position, self.normal, self.z, self.table, self.desc, self.stride, self.hits = position, normal, z, tab, desc, stride, hits

    def __repr__(self):
        return self.name

    def device_z(self):
        """None, or the float32 words of the depth image as the device holds them: the stride's other words are not depths"""
        if self.z is None:
            return None
        flat = np.full(self.z.size * self.stride, np.float32(-7.0), dtype=F)
        flat[::self.stride] = self.z.reshape(-1)
        return flat

    def ctypes_desc(self):
        d, c = self.desc, L.PixelRaysDesc()
        c.width, c.height, c.mode, c.flags, c.tableW, c.tableH = d.width, d.height, d.mode, d.flags, d.tableW, d.tableH
        c.deviceZStride = self.stride if self.z is not None else 0
        c.direction[:] = d.direction
        c.rayLength, c.tMin, c.zNear = float(d.rayLength), float(d.tMin), float(d.zNear)
        return c


def _direction(cam, kind):
    """"synthetic": into the surfaces the camera sees (a lifted position meets its own surface, one on the surface whatever lies
    behind it: the far side of a closed object); otherwise from them towards a light above and behind the camera, which the frame's
    own normals face (FRONT_ONLY); not normalised"""
    f = np.array(cam.front, dtype=np.float64)
    f /= np.linalg.norm(f)
    up = np.array(cam.world_up, dtype=np.float64)
    d = 1.3 * f + 0.15 * up if kind == "synthetic" else -0.8 * f + 0.7 * up
    return tuple(float(F(v)) for v in d)


def _desc(cam, w, h, mode, flags, tw, th, kind, start):
    length = (FRONT_RAY_LENGTH if flags & PR.FRONT_ONLY else RAY_LENGTH[mode]) if kind == "synthetic" else FRAME_RAY_LENGTH
    return PR.Desc(w, h, mode, flags | (PR.START_FROM_DEPTH if start else 0), tw if mode == PR.HEMISPHERE else 0, th if mode == PR.HEMISPHERE else 0,
                   _direction(cam, "light" if kind == "frame" and flags & PR.FRONT_ONLY else "synthetic") if mode == PR.DIRECTION else (0.0, 0.0, 0.0),
                   length, T_MIN, cam.z_near)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for si, sname in enumerate(SCENES):
        sc, cam, tris = scene(sname)
        for mi, (mname, (mode, flags, hits)) in enumerate(MODES.items()):
            for di, (dname, (stride, start)) in enumerate(DEPTHS.items()):
                w, h = SIZES[(di + mi + si) % len(SIZES)]
                tw, th = TABLES[(di + 2 * mi + si) % len(TABLES)]
                kind = "frame" if (w, h) in FRAME_SIZES else "synthetic"
                if (w, h) == (1, 1):
                    tw, th = 1, 1
                    pos, nrm, z = synthetic_images(sname, 19, 13)
                    probe = _desc(cam, 19, 13, mode, flags, 1, 1, kind, start)
                    res, _ = PR.pixel_rays(sc, sc.objects, pos, nrm, z if stride else None, table(1, 1), probe, triangles=tris, meshlet_cull=True)
                    want = (res > 0) & (res < 1) if hits else res == 0
                    pick = np.flatnonzero(want.reshape(-1))
                    k = int(pick[len(pick) // 2]) if len(pick) else int(np.flatnonzero(z.reshape(-1) > 0)[0])
                    pos, nrm, z = (np.ascontiguousarray(a.reshape(-1, *a.shape[2:])[k:k + 1].reshape(1, 1, *a.shape[2:])) for a in (pos, nrm, z))
                else:
                    pos, nrm, z = (frame_images if kind == "frame" else synthetic_images)(sname, w, h)
                desc = _desc(cam, w, h, mode, flags, tw, th, kind, start)
                tab = table(tw, th) if mode == PR.HEMISPHERE else None
                name = "%s-%s-%s-%dx%d-%s" % (sname, mname, dname, w, h, kind)
                out.append(Case(name, sname, mname, dname, kind, pos, nrm, z if stride else None, tab, desc, max(stride, 1), hits))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(case):
    """(out (h, w) float32, hits records.RAY_HIT or None, info) of the specification -- computed once, read-only"""
    sc, cam, tris = scene(case.scene)
    info = {}
    out, hits = PR.pixel_rays(sc, sc.objects, case.position, case.normal, case.z, case.table, case.desc, triangles=tris, meshlet_cull=True, info=info)
    out.setflags(write=False)
    if hits is not None:
        hits.setflags(write=False)
    return out, hits, info
