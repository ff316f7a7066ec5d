"""chordvis_pixel_rays on the GPU, held to what include/chordvis.h promises (RAY QUERIES, "pixel rays"): every word of `out` and of the
hit records equals the specification (tests/spec_pixel_rays_np.py) -- no tolerance, no pixel left out -- on every case of tests/
pixel_rays_cases.py, with guard words around both outputs; the chain frame -> resolve -> pixel rays -> shade on the device equals the
three specifications composed; generate-on-host + chordvis_trace_rays gives the same hit words; the refusals by their messages and what
they leave alone; images written on a caller-owned stream just before the call; the call does not wait.

Device tensors and closing a context: every context here runs on a caller-owned stream (inflight.caller_stream_renderer) under
torch.cuda.stream(stream), so the context's stream IS the current stream, close() leaves it alone, and no device tensor of a
stream-owning context outlives it.  One rule of the header is not reachable from here: a depth-view child context has no handle in
the ABI.  Not run: an image of 2^31 pixels or more, where 2 i + 1 leaves 32 bits -- its position image alone is 32 GB; the kernel's
pixel, depth, table and hit indices are 64-bit by construction (kernels_pixelrays.hip, pixel_rays.h)."""
import numpy as np
import pytest

import helpers as H
import inflight as IF
import pixel_rays_cases as PC
import spec_pixel_rays_np as PR
import spec_ray_shade_np as RS
import spec_resolve_np as SR
import spec_surface_np as SS
from chord_amd import lib as L, records as R, scenes

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
SENTINEL = 0x5EA7BEEF                                                          # (fits an int32 word)
GUARD = 64                                                                     # guard words before and after `out`; two guard records around the hits


def _refused(call, match):
    with pytest.raises(L.ChordvisError, match=match):
        call()


def _device(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).copy())
    return t.to(torch.device("cuda", 0))


class Buffers:
    """A case's images on the device and sentinel-filled outputs with guard words around them (made on the current stream)."""

    def __init__(self, case):
        import torch
        dev = torch.device("cuda", 0)
        d = case.desc
        self.n = d.width * d.height
        self.position, self.normal = _device(case.position), _device(case.normal)
        self.z = None if case.z is None else _device(case.device_z())
        self.table = None if case.table is None else _device(case.table)
        self.out = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        self.hits = torch.full((self.n + 2, 8), SENTINEL, dtype=torch.int32, device=dev) if case.hits else None
        self.desc = case.ctypes_desc()

    def pointers(self):
        return (self.position.data_ptr(), self.normal.data_ptr(), None if self.z is None else self.z.data_ptr(),
                None if self.table is None else self.table.data_ptr(), self.out.data_ptr() + 4 * GUARD,
                None if self.hits is None else self.hits.data_ptr() + 32)

    def call(self, r):
        import ctypes as C
        r._check(L.lib.chordvis_pixel_rays(r._ctx, C.byref(self.desc), *self.pointers()), "pixel_rays")

    def results(self, what):
        """(out words, hit words or None) on the host, the guard words checked"""
        o = self.out.cpu().numpy().view(u32)
        assert (o[:GUARD] == SENTINEL).all() and (o[-GUARD:] == SENTINEL).all(), what + ": a guard word of out was written"
        h = None
        if self.hits is not None:
            h = self.hits.cpu().numpy().view(u32)
            assert (h[0] == SENTINEL).all() and (h[-1] == SENTINEL).all(), what + ": a guard record of the hits was written"
            h = h[1:-1]
        return o[GUARD:-GUARD], h


def _check(case, out, hits, what):
    want_out, want_hits, _ = PC.expected(case)
    w = want_out.view(u32).reshape(-1)
    if not np.array_equal(out, w):
        bad = np.flatnonzero(out != w)
        k = int(bad[0])
        raise AssertionError("%s: out differs from the specification at %d of %d pixels; first: pixel (%d, %d) got %r want %r"
                             % (what, len(bad), len(w), k % case.desc.width, k // case.desc.width, out[k:k + 1].view(f32)[0], want_out.reshape(-1)[k]))
    if case.hits:
        wh = want_hits.view(u32).reshape(-1, 8)
        if not np.array_equal(hits, wh):
            bad = np.flatnonzero((hits != wh).any(axis=1))
            k = int(bad[0])
            raise AssertionError("%s: %d of %d hit records differ; first: pixel %d\n got  %r\n want %r"
                                 % (what, len(bad), len(wh), k, np.ascontiguousarray(hits[k]).view(R.RAY_HIT), want_hits[k]))


def _ray_renderer(scene):
    r, stream = IF.caller_stream_renderer()
    r.upload_scene(scene)
    r.build_ray_scene()
    return r, stream


# ---- 1. the specification: every case ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(PC.SCENES))
def test_images_equal_the_specification(gpu, name):
    import torch
    scene, cam, tris = PC.scene(name)
    cases = [c for c in PC.cases() if c.scene == name]
    assert len(cases) == len(PC.MODES) * len(PC.DEPTHS)
    r, stream = _ray_renderer(scene)
    try:
        info = r.ray_scene_info()
        assert name == "triangle" or info.tlasNodes > 1
        with torch.cuda.stream(stream):
            for c in cases:
                b = Buffers(c)
                b.call(r)
                stream.synchronize()
                out, hits = b.results(c.name)
                _check(c, out, hits, c.name)
                del b
    finally:
        r.close()


# ---- 2. the chain: frame -> resolve -> pixel rays -> shade ---------------------------------------------------------------------

def test_frame_resolve_pixel_rays_shade_on_the_device(gpu):
    """A frame of the material scene into a caller-owned image; resolve_surface writes positionRS and vertexNormal; pixel_rays reads
    the image's depth halves in place (deviceZStride 2) and writes hits; shade_ray_hits shades them: the three specifications composed."""
    import torch
    scene, cam, tris = PC.scene("material")
    w, h = 80, 64                                                              # (a gbuffer is at least 64 pixels per axis)
    view, iv = L.make_views(scenes.Camera(cam.position, cam.front, w, h))
    tab = PC.table(16, 16)
    r, stream = _ray_renderer(scene)
    try:
        r.upload_material_textures()
        dev = torch.device("cuda", 0)
        with torch.cuda.stream(stream):
            vis = torch.zeros(w * h, dtype=torch.int64, device=dev)
            r.allocate_gbuffer(w, h, device_visibility=vis.data_ptr())
            r.set_view(view, iv, H.ALL_FLAGS)
            r.render_frame()
            res = r.resolve_attributes(names=["positionRS", "vertexNormal"])
            dtab = _device(tab)
            out, dhits = r.pixel_rays(res["positionRS"], res["vertexNormal"], mode=L.PIXEL_RAYS_HEMISPHERE, table=dtab, ray_length=PC.FRAME_RAY_LENGTH,
                                      z_near=cam.z_near, depth=vis.data_ptr() + 4, depth_stride=2, start_from_depth=True, hits=True)
            dsurf = r.shade_ray_hits(dhits, lod=1.0)
            stream.synchronize()
            cmds = r.read_cmds(r.last_frame_cmds())
            hvis = vis.cpu().numpy().view(np.uint64)
            got_pos, got_nrm = res["positionRS"].cpu().numpy(), res["vertexNormal"].cpu().numpy()
            got_out, got_hits = out.cpu().numpy(), dhits.cpu().numpy().view(R.RAY_HIT).reshape(-1)
            got_surf = dsurf.cpu().numpy().view(u32).reshape(-1, 16)
            del res, out, dhits, dsurf, dtab, vis
        pos = SR.resolve(scene, hvis, cmds, view, iv, w, h, names=("positionRS",))["positionRS"]
        nrm = SS.resolve(scene, hvis, cmds, view, iv, w, h, names=("vertexNormal",))["vertexNormal"]
        z = (hvis >> np.uint64(32)).astype(u32).view(f32).reshape(h, w)
        assert np.array_equal(got_pos.view(u32), pos.view(u32)) and np.array_equal(got_nrm.view(u32), nrm.view(u32))
        desc = PR.Desc(w, h, PR.HEMISPHERE, PR.START_FROM_DEPTH, 16, 16, rayLength=PC.FRAME_RAY_LENGTH, tMin=0.0, zNear=cam.z_near)
        want_out, want_hits = PR.pixel_rays(scene, scene.objects, pos, nrm, z, tab, desc, triangles=tris, meshlet_cull=True)
        hit = (want_hits["status"] & 1) != 0
        assert (z > 0).sum() > w * h // 2 and hit.sum() > 100 and (~hit & (z.reshape(-1) > 0)).sum() > 100
        assert np.array_equal(got_out.view(u32), want_out.view(u32)), "out of the chain"
        assert got_hits.tobytes() == want_hits.tobytes(), "hits of the chain"
        want_surf = RS.shade(scene, scene.objects, want_hits, lod=1.0)
        assert int((want_surf["flags"] & 1).sum()) == int(hit.sum())
        assert np.array_equal(got_surf, want_surf.view(u32).reshape(-1, 16)), "surfaces of the chain"
    finally:
        r.close()


# ---- 3. generate on the host + chordvis_trace_rays: the path this replaces ------------------------------------------------------

@pytest.mark.parametrize("mode_name", ["hemisphere_closest", "direction_closest", "hemisphere_any"])
def test_host_generated_rays_through_trace_rays_give_the_same_hits(gpu, mode_name):
    import torch
    scene, cam, tris = PC.scene("small")
    cases = [c for c in PC.cases() if c.scene == "small" and c.mode_name == mode_name and c.desc.width * c.desc.height > 64]
    assert len(cases) >= 2
    met = 0
    r, stream = _ray_renderer(scene)
    try:
        with torch.cuda.stream(stream):
            for c in cases:
                any_hit = bool(c.desc.flags & PR.ANY_HIT)
                rays, disp, _ = PR.make_rays(c.position, c.normal, c.z, c.table, c.desc)
                traced = disp == PR.TRACE
                # (a pixel that is not traced has a zero ray here, which chordvis_trace_rays answers with a miss as well)
                via_trace = r.trace_rays(_device(rays.view(np.uint8)), any_hit=any_hit)
                b = Buffers(c)
                b.call(r)
                stream.synchronize()
                out, hits = b.results(c.name)
                t = via_trace.cpu().numpy().view(R.RAY_HIT).reshape(-1)
                assert not t[~traced].view(u32).any()
                if any_hit:
                    assert np.array_equal(out.view(f32) == 0, ((t["status"] & 1) != 0) & traced), c.name
                else:
                    assert t.view(u32).reshape(-1, 8).tolist() == hits.tolist(), c.name
                    met += int(((t["status"] & 1) != 0).sum())
                _check(c, out, hits, c.name)
                del b, via_trace
        assert mode_name.endswith("any") or met > 100, "the closest cases meet something"
    finally:
        r.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals_by_their_messages(gpu):
    import ctypes as C
    import torch
    scene, cam, tris = PC.scene("small")
    case = next(c for c in PC.cases() if c.scene == "small" and c.mode_name == "hemisphere_closest" and c.depth_name == "z1_start")
    front = next(c for c in PC.cases() if c.scene == "small" and c.mode_name == "direction_any_front" and c.depth_name == "z1")
    r, stream = IF.caller_stream_renderer()
    try:
        with torch.cuda.stream(stream):
            b, bf = Buffers(case), Buffers(front)
            stream.synchronize()

            def call(buf=b, desc="own", **ptr):
                names = ("position", "normal", "z", "table", "out", "hits")
                p = dict(zip(names, buf.pointers()))
                p.update(ptr)
                d = buf.desc if desc == "own" else desc
                r._check(L.lib.chordvis_pixel_rays(r._ctx, None if d is None else C.byref(d), *[p[k] for k in names]), "pixel_rays")

            def changed(buf=b, **fields):
                d = type(buf.desc).from_buffer_copy(buf.desc)
                for k, v in fields.items():
                    setattr(d, k, v)
                return d

            def untouched(what):
                stream.synchronize()
                for buf in (b, bf):
                    assert (buf.out.cpu().numpy().view(u32) == SENTINEL).all(), what
                assert (b.hits.cpu().numpy().view(u32) == SENTINEL).all(), what
            assert L.lib.chordvis_pixel_rays(None, C.byref(b.desc), *b.pointers()) == L.E_INVALID
            # chordvis_trace_rays' refusals, in its order
            _refused(call, r"pixel_rays: no scene \(call chordvis_upload_scene first\)")
            r.upload_scene(scene)
            _refused(call, "pixel_rays: no ray scene, or it was dropped")
            _refused(lambda: call(desc=None), "pixel_rays: no ray scene")           # (the context's state comes first)
            r.build_ray_scene()
            _refused(lambda: call(desc=None), "pixel_rays: desc is NULL")
            _refused(lambda: call(desc=changed(mode=2)), "pixel_rays: unknown mode")
            _refused(lambda: call(desc=changed(flags=8)), "pixel_rays: unknown flag bits")
            _refused(lambda: call(desc=changed(flags=0x80000000 | L.PIXEL_RAYS_START_FROM_DEPTH)), "pixel_rays: unknown flag bits")
            _refused(lambda: call(table=None), "CHORD_PIXEL_RAYS_HEMISPHERE needs deviceTable")
            for tw, th in ((0, 4), (4, 0), (3, 4), (4, 6), (0x80000001, 1)):
                _refused(lambda: call(desc=changed(tableW=tw, tableH=th)), "tableW and tableH must be powers of two")
            _refused(lambda: call(z=None), "CHORD_PIXEL_RAYS_START_FROM_DEPTH needs deviceZ")
            _refused(lambda: call(desc=changed(deviceZStride=0)), "deviceZStride must not be 0 with a deviceZ")
            _refused(lambda: call(desc=changed(flags=L.PIXEL_RAYS_ANY_HIT)), "CHORD_PIXEL_RAYS_ANY_HIT writes no hit records")
            _refused(lambda: call(desc=changed(flags=L.PIXEL_RAYS_FRONT_ONLY), hits=None), "CHORD_PIXEL_RAYS_FRONT_ONLY goes with CHORD_PIXEL_RAYS_DIRECTION only")
            _refused(lambda: call(desc=changed(width=0x10000, height=0x10000)), r"width \* height must not exceed 2\^32 - 1")
            _refused(lambda: call(position=None), "devicePosition must be non-NULL and 16-byte aligned")
            _refused(lambda: call(position=b.position.data_ptr() + 8), "devicePosition must be non-NULL and 16-byte aligned")
            _refused(lambda: call(normal=None), "deviceNormal must be non-NULL and 16-byte aligned")
            _refused(lambda: call(normal=b.normal.data_ptr() + 4), "deviceNormal must be non-NULL and 16-byte aligned")
            _refused(lambda: call(buf=bf, normal=None), "deviceNormal must be non-NULL and 16-byte aligned")        # FRONT_ONLY reads it too
            _refused(lambda: call(table=b.table.data_ptr() + 8), "deviceTable must be 16-byte aligned")
            _refused(lambda: call(z=b.z.data_ptr() + 2), "deviceZ must be NULL or 4-byte aligned")
            _refused(lambda: call(out=None), "deviceOut must be non-NULL and 4-byte aligned")
            _refused(lambda: call(out=b.out.data_ptr() + 4 * GUARD + 2), "deviceOut must be non-NULL and 4-byte aligned")
            _refused(lambda: call(hits=b.hits.data_ptr() + 8), "deviceHits must be NULL or 16-byte aligned")
            # an empty image succeeds without a launch and looks at no pointer the desc does not ask for
            assert L.lib.chordvis_pixel_rays(r._ctx, C.byref(changed(width=0, mode=L.PIXEL_RAYS_DIRECTION, flags=0)), None, None, None, None, None, None) == L.OK
            assert L.lib.chordvis_pixel_rays(r._ctx, C.byref(changed(height=0)), None, None, b.z.data_ptr(), b.table.data_ptr(), None, None) == L.OK
            untouched("a refused call wrote")
            # a changed object list drops the TLAS; changed objects ask for a refit
            r.set_object_list(scene.objects[:5].copy())
            _refused(call, "pixel_rays: no ray scene, or it was dropped")
            r.set_object_list(scene.objects.copy())
            _refused(call, "pixel_rays: no ray scene, or it was dropped")
            r.build_ray_scene()
            r.update_objects(scene.objects)
            _refused(call, "pixel_rays: the objects changed .*call chordvis_refit_ray_scene first")
            untouched("a refused call wrote")
            r.refit_ray_scene()
            # what IS allowed: a 4-byte aligned out and depth, a DIRECTION call without normal and table, valid without a view or a G-buffer
            call()
            call(buf=bf)
            plain = changed(buf=bf, flags=L.PIXEL_RAYS_ANY_HIT)
            call(buf=bf, desc=plain, normal=None, table=None)
            stream.synchronize()
            out, hits = b.results(case.name)
            _check(case, out, hits, "after the refusals")
            del b, bf
    finally:
        r.close()


# ---- 5. a caller-owned stream: images written on it just before the call, and the call does not wait ------------------------------

def test_images_written_on_the_stream_just_before_the_call(gpu):
    """Two calls behind a closed gate on a caller-owned stream (tests/inflight.py): the images are copied into place on that stream
    behind the gate too, so they are not there yet when the calls return; both calls return while the device is held, and the answers
    are the specification's once it is released."""
    import torch
    scene, cam, tris = PC.scene("small")
    closest = next(c for c in PC.cases() if c.scene == "small" and c.mode_name == "hemisphere_closest" and c.desc.width * c.desc.height > 400)
    front = next(c for c in PC.cases() if c.scene == "small" and c.mode_name == "direction_any_front" and c.desc.width * c.desc.height > 400)
    sc = IF.Scenario("pixel_rays", scene, 160, 96, H.ALL_FLAGS, [])

    def prepare():
        ctx = IF.Context(sc)
        ctx.r.build_ray_scene()
        with torch.cuda.stream(ctx.stream):
            ctx.bufs = [Buffers(closest), Buffers(front)]
            ctx.src = [(b.position.clone(), b.normal.clone(), None if b.z is None else b.z.clone()) for b in ctx.bufs]
            for b in ctx.bufs:                                                # what a call would read if it ran ahead of the copies
                b.position.fill_(float("nan")); b.normal.zero_()
                if b.z is not None:
                    b.z.zero_()
        ctx.synchronize()
        return ctx

    def script(ctx):
        def write(k):
            with torch.cuda.stream(ctx.stream):
                b, (p, n, z) = ctx.bufs[k], ctx.src[k]
                b.position.copy_(p, non_blocking=True); b.normal.copy_(n, non_blocking=True)
                if z is not None:
                    b.z.copy_(z, non_blocking=True)
        return [("write_images[0]", lambda: write(0), False), ("pixel_rays[0]", lambda: ctx.bufs[0].call(ctx.r), False),
                ("write_images[1]", lambda: write(1), False), ("pixel_rays[1]", lambda: ctx.bufs[1].call(ctx.r), False)]

    ctx, log, _ = IF.run_behind_gate(prepare, script, "two pixel-ray calls in flight")
    try:
        assert IF.waits(log)["pixel_rays"] is False
        with torch.cuda.stream(ctx.stream):
            for c, b in zip((closest, front), ctx.bufs):
                out, hits = b.results(c.name)
                _check(c, out, hits, "in flight, " + c.name)
            ctx.bufs = ctx.src = None
    finally:
        ctx.close()


# ---- 6. the wrapper ------------------------------------------------------------------------------------------------------------

def test_wrapper_on_a_context_that_owns_its_stream(gpu):
    """VisibilityRenderer.pixel_rays on a context with a stream of its own, called from torch's current stream: ordered both ways, and
    nothing on the device outlives the helper."""
    from chord_amd.renderer import VisibilityRenderer
    scene, cam, tris = PC.scene("small")
    c = next(c for c in PC.cases() if c.scene == "small" and c.mode_name == "hemisphere_closest" and c.depth_name == "z2_start")
    f = next(c for c in PC.cases() if c.scene == "small" and c.mode_name == "direction_any_front" and c.depth_name == "no_depth")

    def run(r):
        d = c.desc
        out, hits = r.pixel_rays(_device(c.position), _device(c.normal), table=_device(c.table), ray_length=float(d.rayLength), t_min=float(d.tMin),
                                 z_near=float(d.zNear), depth=_device(c.device_z()), depth_stride=c.stride, start_from_depth=True, hits=True)
        d = f.desc
        mask = r.pixel_rays(_device(f.position), _device(f.normal), mode=L.PIXEL_RAYS_DIRECTION, direction=d.direction, ray_length=float(d.rayLength),
                            t_min=float(d.tMin), any_hit=True, front_only=True)
        r.sync()
        return out.cpu().numpy().view(u32).reshape(-1), hits.cpu().numpy().view(u32).reshape(-1, 8), mask.cpu().numpy().view(u32).reshape(-1)
    r = VisibilityRenderer(0)
    try:
        r.upload_scene(scene)
        r.build_ray_scene()
        out, hits, mask = run(r)
    finally:
        r.close()
    _check(c, out, hits, "the wrapper, " + c.name)
    _check(f, mask, None, "the wrapper, " + f.name)
