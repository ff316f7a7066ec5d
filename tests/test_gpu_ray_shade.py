"""chordvis_shade_ray_hits on the GPU, held to what include/chordvis.h promises (RAY QUERIES, "shading a hit"): every word of every
record equals the specification (tests/spec_ray_shade_np.py) -- no tolerance, no hit left out -- for both texture stores, uniform
and per-hit levels; invalid records give zero words and harm nobody; the wave's edges; the trace's output shaded on the device
without a host round trip; the current objects; absent vertex streams; the refusals and what they leave alone; frames untouched; the
call does not wait; the anisotropy setting does not matter.

Device tensors and closing a context: a VisibilityRenderer(0) owns its stream and close() destroys it, so here device tensors of
such a context are made and read back inside helpers that return numpy arrays (_shade, _frames), and nothing on the device outlives
the helper.  The tests that hold device tensors across several calls run on a caller-owned stream (inflight.caller_stream_renderer /
inflight.Context) under torch.cuda.stream(stream): the context's stream IS the current stream, and close() leaves it alone.

Expected values are computed once per (scene, level run) on the host.  One rule of the header is not reachable from here: a
depth-view child context has no handle in the ABI."""
import functools

import numpy as np
import pytest

import helpers as H
import inflight as IF
import ray_shade_cases as RC
import spec_rays_np as S
import spec_ray_shade_np as RS
import spec_texture_bc_np as BC
from chord_amd import lib as L, records as R, scenes

pytestmark = pytest.mark.gpu
u32 = np.uint32
SENTINEL = 0x5EA7BEEF                                                          # (fits an int32 word)
MATERIAL_FORMATS = [BC.BC3, BC.BC3, BC.BC5, BC.BC1_RGB, BC.BC3]                # albedo, noise, normal, ORM, emissive (tests/test_gpu_texture_blocks.py)


# ---- expected values, once -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _expected(name):
    """(scene, hits of the specification's trace, [(label, lod, lods, want, stats)]) -- host arrays, read-only"""
    scene, cam, view, iv, rays = RC.case(name)
    hits = S.trace(scene, scene.objects, rays, meshlet_cull=True)
    hits.setflags(write=False)
    return scene, hits, RC.shade_runs(scene, scene.objects, hits)


@functools.lru_cache(maxsize=None)
def _expected_blocks():
    """the material scene with block-compressed textures, its decoded twin's expected values"""
    scene, hits, _ = _expected("material")
    bc = BC.bc_scene(scene, MATERIAL_FORMATS)
    twin = BC.decoded_twin(bc)
    return bc, twin, RC.shade_runs(twin, twin.objects, hits)


@functools.lru_cache(maxsize=None)
def _triangle():
    scene, cam = RC.triangle_scene()
    vals = (0.0, 0.125, 1.0 / 3.0, 0.5, 0.875, 1.0)
    hits = np.concatenate([RC.hit(o, u, v, status=st, t=1.0 + o) for o in range(len(scene.objects)) for st in (1, 3) for u in vals for v in vals])
    hits.setflags(write=False)
    return scene, cam, hits


# ---- helpers: nothing on the device outlives them ------------------------------------------------------------------------------

def _renderer(scene, store=L.TEXSTORE_EXPANDED, textures=True):
    from chord_amd.renderer import VisibilityRenderer
    r = VisibilityRenderer(0)
    r.set_material_texture_store(store)
    r.upload_scene(scene)
    if textures:
        r.upload_material_textures()
    return r


def _shade(r, hits, lod=0.0, lods=None):
    """(n, 16) uint32 on the host"""
    out = r.shade_ray_hits(np.asarray(hits), lod=lod, lods=None if lods is None else np.asarray(lods))
    r.sync()
    return out.cpu().numpy().view(u32).reshape(-1, 16)


def _same(got, want, hits, what):
    w = np.ascontiguousarray(want).view(u32).reshape(-1, 16)
    assert got.shape == w.shape, (what, got.shape, w.shape)
    if not np.array_equal(got, w):
        bad = np.flatnonzero((got != w).any(axis=1))
        k = int(bad[0])
        raise AssertionError("%s: %d of %d hits differ from the specification; first: hit %d %r\n got  %r\n want %r"
                             % (what, len(bad), len(w), k, hits[k], got[k].view(RS.RAY_HIT_SURFACE), np.asarray(want)[k]))


def _refused(call, match):
    with pytest.raises(L.ChordvisError, match=match):
        call()


# ---- 1. the specification: every scene, every level run, both stores ------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(RC.SCENES))
def test_records_equal_the_specification(gpu, name):
    scene, hits, runs = _expected(name)
    assert RC.vacuity(scene, name, hits, [(want, stats) for _, _, _, want, stats in runs]) == []
    r = _renderer(scene)
    try:
        for label, lod, lods, want, _ in runs:
            _same(_shade(r, hits, lod, lods), want, hits, "%s, %s" % (name, label))
    finally:
        r.close()


def test_block_store_equals_the_specification_and_the_texel_store(gpu):
    scene, hits, _ = _expected("material")
    bc, twin, runs = _expected_blocks()
    assert RC.vacuity(twin, "material", hits, [(want, stats) for _, _, _, want, stats in runs]) == []
    rb, re = _renderer(bc, L.TEXSTORE_BLOCKS), _renderer(bc, L.TEXSTORE_EXPANDED)
    try:
        assert rb.material_texture_memory()[0] == 0 and rb.material_texture_memory()[1] > 0 and re.material_texture_memory()[1] == 0
        for label, lod, lods, want, _ in runs:
            a, b = _shade(rb, hits, lod, lods), _shade(re, hits, lod, lods)
            _same(a, want, hits, "blocks against the specification on the decoded twin, " + label)
            _same(b, want, hits, "the same scene expanded, " + label)
        # the same CONTEXT under the other store
        rb.set_material_texture_store(L.TEXSTORE_EXPANDED)
        rb.upload_material_textures()
        assert rb.material_texture_memory()[1] == 0
        for label, lod, lods, want, _ in runs[1::3]:
            _same(_shade(rb, hits, lod, lods), want, hits, "the same context expanded, " + label)
    finally:
        rb.close(); re.close()


# ---- 2. invalid records ----------------------------------------------------------------------------------------------------------

def test_invalid_records_among_valid_ones(gpu):
    scene, cam, valid = _triangle()
    cases = RC.invalid_hits(scene)
    lanes = (0, 31, 63, 64)
    hits = valid[np.arange(128 * len(cases) * len(lanes)) % len(valid)].copy()
    where = []
    for j, (what, h) in enumerate(cases):
        for p, lane in enumerate(lanes):
            k = 128 * (j * len(lanes) + p) + lane
            hits[k] = h[0]
            where.append(k)
    want = RS.shade(scene, scene.objects, hits, lod=0.75)
    assert not want[where].view(u32).any() and int((want["flags"] & 1).sum()) == len(hits) - len(where)
    r = _renderer(scene)
    try:
        got = _shade(r, hits, 0.75)
        assert not got[where].any(), "an invalid hit is sixteen zero words"
        _same(got, want, hits, "invalid records among valid ones")
    finally:
        r.close()


# ---- 3. counts, through the raw entry point ------------------------------------------------------------------------------------

def test_counts_and_sentinels(gpu):
    """0, 1, 63, 64, 65 and 4 097 hits: the wave's and the workgroup's edges; nothing is written before the first or after the last
    record; a count of 0 launches nothing and looks at no pointer."""
    import torch
    scene, cam, valid = _triangle()
    r, stream = IF.caller_stream_renderer()
    try:
        r.upload_scene(scene)
        r.upload_material_textures()
        dev = torch.device("cuda", 0)
        with torch.cuda.stream(stream):
            assert L.lib.chordvis_shade_ray_hits(r._ctx, None, 0, 0.0, None, None) == L.OK
            for n in (0, 1, 63, 64, 65, 4097):
                hits = valid[np.arange(n) % len(valid)]
                want = RS.shade(scene, scene.objects, hits, lod=1.25)
                dh = torch.from_numpy(hits.view(np.uint8).copy()).to(dev) if n else torch.zeros(32, dtype=torch.uint8, device=dev)
                out = torch.full((n + 2, 16), SENTINEL, dtype=torch.int32, device=dev)
                r._check(L.lib.chordvis_shade_ray_hits(r._ctx, dh.data_ptr(), n, 1.25, None, out.data_ptr() + 64), "shade_ray_hits")
                got = out.cpu().numpy()
                assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all(), "%d hits: a sentinel record was written" % n
                _same(got[1:-1].view(u32), want, hits, "%d hits" % n)
    finally:
        r.close()


# ---- 4. trace and shade on the device ------------------------------------------------------------------------------------------

def test_trace_then_shade_without_a_host_round_trip(gpu):
    import torch
    scene, want_hits, _ = _expected("general")
    rays = RC.case("general")[4]
    r, stream = IF.caller_stream_renderer()
    try:
        r.upload_scene(scene)
        r.upload_material_textures()
        r.build_ray_scene()
        with torch.cuda.stream(stream):
            drays = torch.from_numpy(np.asarray(rays).view(np.uint8).copy()).to(torch.device("cuda", 0))
            dhits = r.trace_rays(drays)
            t = dhits.view(torch.float32)[:, 0]
            dlods = torch.log2(torch.clamp(t, min=1e-3)).contiguous()         # a ray cone's footprint grows with t
            dsurf = r.shade_ray_hits(dhits, lods=dlods)
            stream.synchronize()
            hits = dhits.cpu().numpy().view(R.RAY_HIT).reshape(-1)
            lods = dlods.cpu().numpy()
            got = dsurf.cpu().numpy().view(u32).reshape(-1, 16)
        assert hits.tobytes() == want_hits.tobytes(), "the trace is the specification's"
        assert (lods[(hits["status"] & 1) != 0] > 0.5).any() and (lods < 0.0).any()
        want = RS.shade(scene, scene.objects, want_hits, lods=lods)
        assert (want["flags"] & 1).sum() > len(hits) // 5
        _same(got, want, hits, "trace -> shade on the device")
    finally:
        r.close()


# ---- 5. the current objects ----------------------------------------------------------------------------------------------------

def test_the_current_objects_are_read(gpu):
    scene0, hits, runs = _expected("material")
    cam = RC.case("material")[1]
    scene = scene0.with_objects(scene0.objects.copy())
    r = _renderer(scene)
    try:
        label, lod, lods, want, _ = runs[1]
        _same(_shade(r, hits, lod, lods), want, hits, "as uploaded")
        # (a) rotated objects: the normals follow, without a refit or a ray scene
        moved = scene.with_objects(scene.objects.copy())
        rot = scenes.rotate_y(0.6) @ scenes.rotate_x(-0.3)
        moved.local_to_world = np.ascontiguousarray(np.stack([(rot @ m.reshape(4, 4).T).T.reshape(16) for m in scene.local_to_world]), dtype=np.float64)
        L.fill_objects(moved, cam)
        r.update_objects(moved.objects)
        want_moved = RS.shade(scene, moved.objects, hits, lod=lod, lods=lods)
        valid = (want["flags"] & 1) != 0
        assert np.array_equal(want_moved["flags"], want["flags"]) and (want_moved["normal"][valid] != want["normal"][valid]).any(axis=1).mean() > 0.9
        assert np.array_equal(want_moved["baseColor"], want["baseColor"])
        _same(_shade(r, hits, lod, lods), want_moved, hits, "after update_objects")
        # (b) a shorter list under other materials: an index that was valid is not any more, and the materials are the new list's
        keep = len(scene.objects) // 2
        objs = moved.objects[:keep].copy()
        objs["GLTFMaterialData"] = np.roll(objs["GLTFMaterialData"], 1)
        cur = scene.with_objects(objs)
        r.set_object_list(cur)
        want_cur = RS.shade(cur, cur.objects, hits, lod=lod, lods=lods)
        gone = valid & (hits["object"] >= keep)
        assert gone.sum() > 50 and not want_cur[gone].view(u32).any()
        still = valid & (hits["object"] < keep)
        assert still.sum() > 50 and (want_cur["material"][still] != want_moved["material"][still]).any()
        _same(_shade(r, hits, lod, lods), want_cur, hits, "after set_object_list")
    finally:
        r.close()


def test_meshlets_of_another_primitive(gpu):
    """A host's own hits that pair an object with a meshlet of another primitive: the vertex ids take the vertexOffset of the OBJECT's
    primitive, as the specification says; where that leaves the positions the hit is invalid."""
    scene, hits, runs = _expected("material")
    _, lod, _, own, _ = runs[1]
    hit = (hits["status"] & 1) != 0
    other = hits.copy()
    other["object"] = np.where(hit, (hits["object"] + 3) % len(scene.objects), hits["object"])
    offset = scene.primitives["vertexOffset"][scene.objects["GLTFPrimitiveDetail"]]
    foreign = hit & (offset[other["object"]] != offset[hits["object"] % len(scene.objects)])
    want = RS.shade(scene, scene.objects, other, lod=lod)
    valid = (want["flags"] & 1) != 0
    assert (foreign & valid).sum() > 100 and (foreign & ~valid).sum() > 10
    assert (want["uv"][foreign & valid] != own["uv"][foreign & valid]).any(axis=1).mean() > 0.9
    r = _renderer(scene)
    try:
        _same(_shade(r, other, lod), want, other, "meshlets of another primitive")
    finally:
        r.close()


# ---- 6. absent streams ---------------------------------------------------------------------------------------------------------

def test_scenes_without_normals_or_texture_coordinates(gpu):
    scene, cam, hits = _triangle()
    lods = RC.per_hit_lods(hits)

    def variant(**kw):
        a = dict(texcoord0=scene.texcoord0, normals=scene.normals, tangents=scene.tangents)
        a.update(kw)
        return R.Scene(scene.objects, scene.primitives, scene.materials, scene.meshlets, scene.groups, scene.group_indices, scene.meshlet_data,
                       scene.positions, textures=scene.texture_images, samplers=scene.samplers, bvh_nodes=scene.bvh_nodes, **a)
    for what, sc in (("no normals", variant(normals=None, tangents=None)), ("no texture coordinates", variant(texcoord0=None))):
        want = RS.shade(sc, sc.objects, hits, lods=lods)
        if sc.normals is None:
            assert not (want["normal"].view(u32) & 0x7FFFFFFF).any() and want["uv"].any()
        else:
            assert not want["uv"].view(u32).any() and want["normal"].any() and want["baseColor"].any() and want["emissive"].any()
        r = _renderer(sc)
        try:
            _same(_shade(r, hits, 0.0, lods), want, hits, what)
        finally:
            r.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals_leave_everything_alone(gpu):
    import torch
    scene, cam, hits = _triangle()
    want = RS.shade(scene, scene.objects, hits, lod=0.5)
    r, stream = IF.caller_stream_renderer()
    try:
        dev = torch.device("cuda", 0)
        with torch.cuda.stream(stream):
            dh = torch.from_numpy(hits.view(np.uint8).copy()).to(dev)
            dl = torch.zeros(len(hits) + 1, dtype=torch.float32, device=dev)
            out = torch.full((len(hits), 16), SENTINEL, dtype=torch.int32, device=dev)

            def shade(hp=dh.data_ptr(), lp=None, op=out.data_ptr(), n=len(hits)):
                r._check(L.lib.chordvis_shade_ray_hits(r._ctx, hp, n, 0.5, lp, op), "shade_ray_hits")

            def untouched(what):
                stream.synchronize()
                assert (out.cpu().numpy() == SENTINEL).all(), what
            assert L.lib.chordvis_shade_ray_hits(None, dh.data_ptr(), len(hits), 0.5, None, out.data_ptr()) == L.E_INVALID
            _refused(shade, r"no scene \(call chordvis_upload_scene first\)")
            r.upload_scene(scene)
            _refused(shade, "no material textures.*call chordvis_upload_material_textures first")
            _refused(lambda: shade(n=0), "call chordvis_upload_material_textures first")
            r.upload_material_textures()
            _refused(lambda: shade(hp=None), "non-NULL and 16-byte aligned")
            _refused(lambda: shade(op=None), "non-NULL and 16-byte aligned")
            _refused(lambda: shade(hp=dh.data_ptr() + 8), "non-NULL and 16-byte aligned")
            _refused(lambda: shade(op=out.data_ptr() + 4), "non-NULL and 16-byte aligned")
            _refused(lambda: shade(lp=dl.data_ptr() + 2), "deviceLods must be NULL .* or 4-byte aligned")
            assert L.lib.chordvis_shade_ray_hits(r._ctx, None, 0, 0.5, None, None) == L.OK
            untouched("a refused call wrote")
            # an upload of the scene drops the material textures: refused until they are back
            r.upload_scene(scene)
            _refused(shade, "call chordvis_upload_material_textures first")
            untouched("a refused call wrote")
            r.upload_material_textures()
            shade(lp=dl.data_ptr() + 4)                                    # 4-byte aligned levels are enough; valid without a view, a G-buffer or a ray scene
            stream.synchronize()
            got = out.cpu().numpy().view(u32)
        _same(got, RS.shade(scene, scene.objects, hits, lods=np.zeros(len(hits), np.float32)), hits, "after the refusals")
        assert want.tobytes() != got.tobytes()
    finally:
        r.close()


def _raw_shade(r, hits, lod):
    """The raw entry point into a sentinel-filled buffer: (the refusal's message or None, the buffer's words on the host).  The device
    tensors live and die in here."""
    import torch
    dev = torch.device("cuda", 0)
    dh = torch.from_numpy(np.asarray(hits).view(np.uint8).copy()).to(dev)
    out = torch.full((len(hits), 16), SENTINEL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    message = None
    try:
        r._check(L.lib.chordvis_shade_ray_hits(r._ctx, dh.data_ptr(), len(hits), lod, None, out.data_ptr()), "shade_ray_hits")
    except L.ChordvisError as e:
        message = str(e)
    r.sync()
    return message, out.cpu().numpy().view(u32)


def test_refused_between_the_frame_phases(gpu):
    """A two-rank sharded frame on one device (helpers.sharded_contexts): between chordvis_frame_phase_cull and chordvis_frame_phase_a a
    shade is refused with the rule's name and writes nothing; once phase a has run, and after the frame, it works again."""
    scene, hits, runs = _expected("material")
    cam = RC.case("material")[1]
    fw, fh = 320, 200
    fview, fiv = L.make_views(scenes.Camera(cam.position, cam.front, fw, fh))
    _, lod, _, want, _ = runs[1]
    ctxs = H.sharded_contexts(scene, fview, fiv, fw, fh, H.ALL_FLAGS, 2)
    try:
        for r in ctxs:
            r.upload_material_textures()
        H.sharded_frame(ctxs)                                              # a first whole frame: the history the next one culls against
        message, got = _raw_shade(ctxs[0], hits, lod)
        assert message is None
        _same(got, want, hits, "a sharded context between frames")
        for r in ctxs:
            r.frame_phase_cull()
        for r in ctxs:
            message, got = _raw_shade(r, hits, lod)
            assert message is not None and "shade_ray_hits: not between chordvis_frame_phase_cull and chordvis_frame_phase_a" in message, message
            assert (got == SENTINEL).all(), "a refused call wrote"
        cx = [r.cull_exchange() for r in ctxs]
        H.sharded_gather(ctxs, [c[0] for c in cx], cx[0][1])
        for r in ctxs:
            r.frame_phase_a()
        message, got = _raw_shade(ctxs[1], hits, lod)                      # phase a has run: allowed again, in the middle of the frame
        assert message is None
        _same(got, want, hits, "after phase a")
        ex = [r.hzb_exchange() for r in ctxs]
        H.sharded_gather(ctxs, [e[0] for e in ex], ex[0][2] * 2)
        for r in ctxs:
            r.frame_phase_b()
        fin = [r.hzb_final_exchange() for r in ctxs]
        H.sharded_gather(ctxs, [f[0] for f in fin], fin[0][1])
        H.sharded_gather(ctxs, [r.visibility_ptr() for r in ctxs], ctxs[0].visibility_chunk_words() * 8)
        for r in ctxs:
            r.frame_phase_c()
        message, got = _raw_shade(ctxs[0], hits, lod)
        assert message is None
        _same(got, want, hits, "after the frame")
    finally:
        for r in ctxs:
            r.close()


# ---- 8. frames untouched -------------------------------------------------------------------------------------------------------

def test_frames_are_untouched(gpu):
    """A frame before and after a shade is bit for bit the frame of a context that never shaded: image, list, HZB and counts."""
    scene, hits, runs = _expected("material")
    cam = RC.case("material")[1]
    fw, fh = 160, 96
    fview, fiv = L.make_views(scenes.Camera(cam.position, cam.front, fw, fh))
    label, lod, lods, want, _ = runs[4]

    def _frames(with_shade):
        r = _renderer(scene)
        out = []
        try:
            r.allocate_gbuffer(fw, fh)
            r.set_view(fview, fiv, H.ALL_FLAGS)
            for k in range(3):
                if with_shade and k >= 1:
                    _same(_shade(r, hits, lod, lods), want, hits, "between frames")
                r.render_frame()
                r.sync()
                out.append((r.read_visibility().tobytes(), r.read_cmds(r.last_frame_cmds()).tobytes(),
                            [None if a is None else a.tobytes() for a in r.read_hzb(r.history_hzb())], r.stats()))
        finally:
            r.close()
        return out
    a, b = _frames(False), _frames(True)
    for k in range(3):
        assert a[k][0] == b[k][0], "frame %d: image" % k
        assert a[k][1] == b[k][1], "frame %d: list" % k
        assert a[k][2] == b[k][2], "frame %d: HZB" % k
        keys = [key for key in a[k][3] if not key.startswith("ms")]              # every field but the measured times
        assert len(keys) >= 18 and "kernelLaunches" in keys and "binEntries" in keys
        for key in keys:
            assert a[k][3][key] == b[k][3][key], (k, key, a[k][3][key], b[k][3][key])
    assert any(np.frombuffer(f[0], dtype=np.uint64).any() for f in a)


# ---- 9. stream order -----------------------------------------------------------------------------------------------------------

def test_shade_does_not_wait(gpu):
    """Two shades (a uniform level, per-hit levels) behind a closed gate on a caller-owned stream (tests/inflight.py): both calls return
    while the device is held, and the records are the specification's once it is released."""
    import torch
    scene, hits, runs = _expected("material")
    _, lod0, _, want0, _ = runs[2]
    _, _, lods1, want1, _ = runs[4]
    sc = IF.Scenario("ray_shade", scene, 160, 96, H.ALL_FLAGS, [])

    def prepare():
        ctx = IF.Context(sc)
        ctx.r.upload_material_textures()
        dev = torch.device("cuda", 0)
        with torch.cuda.stream(ctx.stream):
            ctx.hits = torch.from_numpy(hits.view(np.uint8).copy()).to(dev)
            ctx.lods = torch.from_numpy(np.ascontiguousarray(lods1)).to(dev)
            ctx.out0 = torch.zeros((len(hits), 16), dtype=torch.int32, device=dev)
            ctx.out1 = torch.zeros((len(hits), 16), dtype=torch.int32, device=dev)
        ctx.synchronize()
        return ctx

    def script(ctx):
        def shade(lod, lods, out):
            with torch.cuda.stream(ctx.stream):
                ctx.r.shade_ray_hits(ctx.hits, lod=lod, lods=lods, out=out)
        return [("shade_ray_hits[0]", lambda: shade(lod0, None, ctx.out0), False),
                ("shade_ray_hits[1]", lambda: shade(0.0, ctx.lods, ctx.out1), False)]

    ctx, log, _ = IF.run_behind_gate(prepare, script, "two shades in flight")
    try:
        assert IF.waits(log) == {"shade_ray_hits": False}
        _same(ctx.out0.cpu().numpy().view(u32), want0, hits, "in flight, a uniform level")
        _same(ctx.out1.cpu().numpy().view(u32), want1, hits, "in flight, per-hit levels")
    finally:
        ctx.close()


# ---- 10. settings that must not matter -----------------------------------------------------------------------------------------

def test_anisotropy_changes_no_word(gpu):
    scene, hits, runs = _expected("material")
    r = _renderer(scene)
    try:
        r.set_material_anisotropy(16)
        assert r.material_anisotropy() == 16
        for label, lod, lods, want, _ in runs[2:]:
            _same(_shade(r, hits, lod, lods), want, hits, "anisotropy 16, " + label)
    finally:
        r.close()
