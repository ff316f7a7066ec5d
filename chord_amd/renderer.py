"""Host-side mirror of the reference's pass surface over the C ABI (libchordvis.so).

Names follow source/renderer/mesh/gltf_rendering.h:37-108 and postprocessing.h:41-54:
instance_culling, hzb_culling, render_mesh, visibility_stage0/1, build_hzb, and render_frame for
the hot segment of DeferredRenderer::render (renderer.cpp:315-345).  Everything here only forwards
to the HIP library; there is no CPU implementation of any pass in this package.
"""
import ctypes as C

import numpy as np

from . import lib as L
from . import records as R


class VisibilityRenderer:
    """One device context (graphics::Context + DeferredRenderer state for this path)."""

    def __init__(self, device=0, stream=None, _borrowed_ctx=None):
        self._borrowed = _borrowed_ctx is not None
        if self._borrowed:
            self._ctx = C.c_void_p(_borrowed_ctx)             # a rank of a VisibilityGroup: the group owns it
        else:
            self._ctx = C.c_void_p()
            rc = L.lib.chordvis_create(device, stream, C.byref(self._ctx))
            if rc != L.OK:
                raise L.ChordvisError(
                    "chordvis_create(device=%d) failed with %d: no usable HIP device (the product path has no CPU fallback)" % (device, rc))
        self.device = device
        self.width = self.height = 0
        self.scene = None

    # -- plumbing -------------------------------------------------------------------------------
    def _check(self, rc, what):
        if rc != L.OK:
            msg = L.lib.chordvis_last_error(self._ctx)
            raise L.ChordvisError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""))

    def close(self):
        if self._ctx and not self._borrowed:
            L.lib.chordvis_destroy(self._ctx)
        self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._check(L.lib.chordvis_sync(self._ctx), "sync")

    # -- scene / view ---------------------------------------------------------------------------
    def upload_scene(self, scene):
        self.scene = scene
        self._check(L.lib.chordvis_upload_scene(self._ctx, C.byref(scene.desc)), "upload_scene")

    def upload_material_textures(self, scene=None):
        """Opt-in, after upload_scene: keeps the RGBA texels of every texture a material names and the per-material records
        chordvis_resolve_material samples (default: the scene last uploaded).  Dropped by the next upload_scene."""
        scene = self.scene if scene is None else scene
        self._check(L.lib.chordvis_upload_material_textures(self._ctx, C.byref(scene.desc)), "upload_material_textures")

    def readback_material_texture(self, texture, level=0):
        """(h, w, 4) uint8: the expanded texels of one level of a texture as chordvis_resolve_material reads them (after
        upload_material_textures; block-compressed textures as the library decoded them)."""
        t = self.scene.texture_images[texture]
        level0 = level + self._stored_first_level(texture)     # (set_texture_first_level: `level` counts from the first stored one)
        h, w = max(1, t.shape[0] >> level0), max(1, t.shape[1] >> level0)
        out = np.zeros((h, w, 4), dtype=np.uint8)
        self._check(L.lib.chordvis_readback_material_texture(self._ctx, int(texture), int(level), out.ctypes.data), "readback_material_texture")
        return out

    def readback_material_blocks(self, texture, format=None, levels=None):
        """uint8 array: the whole chain of a texture kept as blocks, in the layout of ChordTexture (after upload_material_textures
        under lib.TEXSTORE_BLOCKS): the bytes supplied, or what set_texture_compress made the GPU encode.  format / levels: of
        the FINISHED chain (default: what the current compress and mips settings give the scene's texture); a chain trimmed by
        set_texture_first_level comes back from its first stored level on.  A lib.ChordvisError for a texture stored as texels."""
        t = self.scene.texture_images[texture]
        if format is None:
            format = self.texture_compress(texture) or getattr(t, "format", 0)
        if levels is None:
            full = max(t.shape[0], t.shape[1]).bit_length()
            levels, mips = self.texture_mips(texture)[0], getattr(t, "mips", full)      # (an image: Scene supplies its full chain)
            levels = mips if not levels else max(mips, min(levels, full))
        first = min(self._stored_first_level(texture), levels - 1)                       # (set_texture_first_level: the stored chain is the smaller texture's)
        n = L.texture_chain_bytes(format, max(1, t.shape[1] >> first), max(1, t.shape[0] >> first), levels - first) if format else 0
        out = np.zeros(max(1, n), dtype=np.uint8)
        self._check(L.lib.chordvis_readback_material_blocks(self._ctx, int(texture), out.ctypes.data, n), "readback_material_blocks")
        return out

    def _stored_first_level(self, texture):
        """firstLevel of chordvis_material_texture_levels; 0 where the store holds nothing of the texture"""
        f = C.c_uint32(0)
        rc = L.lib.chordvis_material_texture_levels(self._ctx, int(texture), C.byref(f), None)
        return f.value if rc == L.OK else 0

    def read_alpha_plane(self, count, offset=0):
        """`count` bytes of the alpha plane the masked buckets sample, from byte `offset` (chordvis_debug_read 7)."""
        out = np.zeros(int(count), dtype=np.uint8)
        self._check(L.lib.chordvis_debug_read(self._ctx, 7, int(offset), int(count), out.ctypes.data), "debug_read")
        return out

    def set_material_anisotropy(self, n):
        """Maximum anisotropy of the material resolve's sampler: 1 (default: the isotropic sampler), 2, 4, 8 or 16 taps along the
        longer derivative.  Per context; kept across upload_scene and upload_material_textures."""
        self._check(L.lib.chordvis_set_material_anisotropy(self._ctx, int(n)), "set_material_anisotropy")

    def material_anisotropy(self):
        return int(L.lib.chordvis_material_anisotropy(self._ctx))

    def set_material_texture_store(self, mode):
        """How LATER upload_material_textures calls store block-compressed textures: lib.TEXSTORE_EXPANDED (default: RGBA8 texels, 4
        bytes each) or lib.TEXSTORE_BLOCKS (a BC chain whose every level is supplied keeps its blocks; the material resolve decodes
        what it taps, to the same images).  Per context; kept across upload_scene and upload_material_textures; a store already
        uploaded stays as it is."""
        self._check(L.lib.chordvis_set_material_texture_store(self._ctx, int(mode)), "set_material_texture_store")

    def material_texture_store(self):
        return int(L.lib.chordvis_material_texture_store(self._ctx))

    def material_texture_memory(self):
        """(texelBytes, blockBytes) of the uploaded material textures: the RGBA8 store and the chains kept as blocks."""
        t, b = C.c_uint64(0), C.c_uint64(0)
        self._check(L.lib.chordvis_material_texture_memory(self._ctx, C.byref(t), C.byref(b)), "material_texture_memory")
        return t.value, b.value

    def set_texture_mips(self, settings):
        """Mip chains made on the GPU by LATER upload_scene / upload_material_textures calls: entry i, a
        lib.TextureMips or a (levels, flags, alphaCutoff8) tuple, belongs to texture id i; None or an empty list: none (the default).
        levels: lib.TEXMIPS_FULL or a count, 0 = as supplied; flags: lib.TEXMIPS_SRGB | lib.TEXMIPS_COVERAGE.  Per context; kept
        across uploads."""
        settings = list(settings or ())
        arr = (L.TextureMips * max(1, len(settings)))()
        for i, m in enumerate(settings):
            arr[i] = m if isinstance(m, L.TextureMips) else L.TextureMips(*m)
        self._check(L.lib.chordvis_set_texture_mips(self._ctx, arr if settings else None, len(settings)), "set_texture_mips")

    def set_texture_compress(self, formats):
        """Block compression on the GPU by LATER upload_material_textures calls under lib.TEXSTORE_BLOCKS:
        entry i is the target of texture id i, 0 (none) or records.TEXFMT_BC1_RGB / BC3 / BC4 / BC5; None or an empty list: none
        (the default).  An RGBA8 texture with a target is encoded whole, made levels included, and keeps no texel; a block
        texture in its target format keeps its supplied levels verbatim and gets its made levels encoded.  Per context; kept
        across uploads; ignored in mode EXPANDED and by upload_scene."""
        formats = [int(f) for f in (formats or ())]
        arr = (C.c_uint32 * max(1, len(formats)))(*formats)
        self._check(L.lib.chordvis_set_texture_compress(self._ctx, arr if formats else None, len(formats)), "set_texture_compress")

    def texture_compress(self, texture):
        """The target format set for a texture id; 0 where nothing is set."""
        f = C.c_uint32(0)
        self._check(L.lib.chordvis_texture_compress(self._ctx, int(texture), C.byref(f)), "texture_compress")
        return f.value

    def set_texture_first_level(self, first):
        """Trimmed chains: entry i is the first level LATER upload_material_textures calls keep of texture id i (clamped to its last
        level); None or an empty list: every texture keeps level 0 (the default).  The stored texture is then the one whose level 0
        is that level, and every level index counts from there.  Per context; kept across uploads; ignored by upload_scene."""
        first = [int(f) for f in (first or ())]
        arr = (C.c_uint32 * max(1, len(first)))(*first)
        self._check(L.lib.chordvis_set_texture_first_level(self._ctx, arr if first else None, len(first)), "set_texture_first_level")

    def texture_first_level(self, texture):
        """The first level set for a texture id; 0 where nothing is set."""
        f = C.c_uint32(0)
        self._check(L.lib.chordvis_texture_first_level(self._ctx, int(texture), C.byref(f)), "texture_first_level")
        return f.value

    def material_texture_levels(self, texture):
        """(firstLevel, levelCount) of what the uploaded store holds of a texture a material names."""
        f, n = C.c_uint32(0), C.c_uint32(0)
        self._check(L.lib.chordvis_material_texture_levels(self._ctx, int(texture), C.byref(f), C.byref(n)), "material_texture_levels")
        return f.value, n.value

    def reset_material_feedback(self):
        """Zeroes the context's feedback buffer (allocating it after a material upload), on the context's stream."""
        self._check(L.lib.chordvis_material_feedback_reset(self._ctx), "material_feedback_reset")

    def material_feedback(self, slot_mask=15, stride=1, offset=(0, 0), drawed_meshlet_cmd=None):
        """Adds, for every pixel (x % stride, y % stride) == offset that resolve_attributes would write material images for and
        every texture slot of slot_mask (lib.FEEDBACK_* bits), 1 to the count of the finest level the material sampler would
        fetch there (chordvis_material_feedback: one launch on the context's stream; counts accumulate until the next reset)."""
        d = L.FeedbackDesc(int(slot_mask), int(stride), (C.c_uint32 * 2)(int(offset[0]), int(offset[1])))
        cmd = drawed_meshlet_cmd if drawed_meshlet_cmd is not None else self.last_frame_cmds()
        self._check(L.lib.chordvis_material_feedback(self._ctx, cmd, C.byref(d)), "material_feedback")

    def read_material_feedback(self, texture_count=None):
        """(textureCount, lib.FEEDBACK_LEVELS) uint32: the counts per texture id and stored level; synchronises."""
        n = len(self.scene.texture_images) if texture_count is None else int(texture_count)
        out = np.zeros((n, L.FEEDBACK_LEVELS), dtype=np.uint32)
        self._check(L.lib.chordvis_readback_material_feedback(self._ctx, out.ctypes.data if n else np.zeros(1, np.uint32).ctypes.data, n), "readback_material_feedback")
        return out

    def reset_geometry_feedback(self):
        """Zeroes the context's geometry feedback buffer (allocating it after a scene upload), on the context's stream."""
        self._check(L.lib.chordvis_geometry_feedback_reset(self._ctx), "geometry_feedback_reset")

    def geometry_feedback(self, stride=1, offset=(0, 0), drawed_meshlet_cmd=None):
        """Adds what the pixels (x % stride, y % stride) == offset of the last frame's image saw to the context's counts and makes
        the seen bitmap that of this call (chordvis_geometry_feedback: one memset and two launches on the context's stream)."""
        d = L.GeometryFeedbackDesc(int(stride), (C.c_uint32 * 2)(int(offset[0]), int(offset[1])), 0)
        cmd = drawed_meshlet_cmd if drawed_meshlet_cmd is not None else self.last_frame_cmds()
        self._check(L.lib.chordvis_geometry_feedback(self._ctx, cmd, C.byref(d)), "geometry_feedback")

    def read_geometry_feedback(self, names=L.GEOMETRY_ARRAYS):
        """{name: uint32 array} of the counts: (objectCount,) for the object arrays, (primitiveCount, lib.GEOMETRY_LODS) for the lod
        arrays, (4,) for totals (lattice pixels looked at, contributing, rejected, seen commands); synchronises."""
        no, npr = len(self.scene.objects), len(self.scene.primitives)
        shape = lambda n: (4,) if n == "totals" else (no,) if n.startswith("object") else (npr, L.GEOMETRY_LODS)
        out = {n: np.zeros(shape(n), dtype=np.uint32) for n in names}
        fb = L.GeometryFeedback(**{n: a.ctypes.data for n, a in out.items()})
        self._check(L.lib.chordvis_readback_geometry_feedback(self._ctx, C.byref(fb), no, npr), "readback_geometry_feedback")
        return out

    def read_geometry_feedback_seen(self):
        """uint32 words of the latest geometry_feedback call's seen bitmap: bit i & 31 of word i >> 5 for command i; synchronises."""
        out = np.zeros((self.last_frame_cmds().capacity + 31) // 32, dtype=np.uint32)
        self._check(L.lib.chordvis_geometry_feedback_seen(self._ctx, out.ctypes.data, len(out)), "geometry_feedback_seen")
        return out

    def visible_clusters(self, capacity=None, drawed_meshlet_cmd=None, out=None):
        """(records, total): the commands the latest geometry_feedback call saw, in list order (chordvis_visible_clusters into a
        device tensor of `capacity` records, default the list's capacity), read back; total may exceed capacity.  out: a torch int32
        tensor of at least 3 * capacity + 1 words on the context's device to use instead (records, then the count word)."""
        import torch
        cmd = drawed_meshlet_cmd if drawed_meshlet_cmd is not None else self.last_frame_cmds()
        capacity = int(cmd.capacity if capacity is None else capacity)
        dev = torch.device("cuda", self.device)
        if out is None:
            with torch.cuda.device(dev):
                out = torch.zeros(3 * capacity + 1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)
        assert out.is_contiguous() and out.numel() >= 3 * capacity + 1
        base = out.data_ptr()
        self._check(L.lib.chordvis_visible_clusters(self._ctx, cmd, base if capacity else None, base + 12 * capacity, capacity), "visible_clusters")
        self.sync()
        host = out.cpu().numpy()
        total = int(host[3 * capacity:3 * capacity + 1].view(np.uint32)[0])
        return host[:3 * min(capacity, total)].copy().view(R.DRAW_CMD), total

    def query_bounds(self, queries, hzb=None, phase=1, want_results=True, capacity=None, want_count=True):
        """chordvis_query_bounds: the frame's frustum and occlusion tests for host-owned boxes.  queries: a numpy array of
        records.BOUNDS_QUERY, or a contiguous CUDA tensor holding such records (160 bytes each) on the context's device.  hzb: an
        L.HZB handle (history_hzb()), or None for everything but the taps.  phase: 1 tests with the current matrices, 0 with last
        frame's.  Returns (results, visible_indices, visible_count), read back: records.BOUNDS_RESULT per query (None unless
        want_results), the uint32 indices of the visible queries in ascending order (at most `capacity` of them; default: room for
        all) and their number, which may exceed capacity (None unless want_count).  The call is ordered behind the current torch
        stream and that one behind the call (as resolve_gbuffer does it)."""
        import torch
        dev = torch.device("cuda", self.device)
        if isinstance(queries, np.ndarray):
            host = np.ascontiguousarray(queries, dtype=R.BOUNDS_QUERY).reshape(-1)
            count = len(host)
            with torch.cuda.device(dev):
                q = torch.from_numpy(host.view(np.uint8).copy()).to(dev) if count else torch.zeros(16, dtype=torch.uint8, device=dev)
        else:
            q = queries
            nbytes = q.numel() * q.element_size()
            assert q.is_cuda and q.is_contiguous() and nbytes % R.BOUNDS_QUERY.itemsize == 0, "query_bounds: a contiguous CUDA tensor of 160-byte records"
            count = nbytes // R.BOUNDS_QUERY.itemsize
        capacity = count if capacity is None else int(capacity)
        with torch.cuda.device(dev):
            res = torch.zeros(4 * count, dtype=torch.int32, device=dev) if want_results else None
            vis = torch.zeros(capacity, dtype=torch.int32, device=dev) if capacity else None
            cnt = torch.zeros(1, dtype=torch.int32, device=dev) if want_count else None
        used = [t for t in (q, res, vis, cnt) if t is not None]
        self._on_my_stream(used, lambda: self._check(L.lib.chordvis_query_bounds(
            self._ctx, C.byref(hzb) if hzb is not None else None, int(phase), q.data_ptr() if count else None, count,
            res.data_ptr() if res is not None and count else None, vis.data_ptr() if vis is not None else None,
            cnt.data_ptr() if cnt is not None else None, capacity), "query_bounds"))
        self.sync()
        total = int(cnt.cpu().numpy().view(np.uint32)[0]) if cnt is not None else None
        results = res.cpu().numpy().view(R.BOUNDS_RESULT).copy() if res is not None else None
        listed = capacity if total is None else min(capacity, total)
        indices = vis.cpu().numpy().view(np.uint32)[:listed].copy() if vis is not None else np.zeros(0, dtype=np.uint32)
        return results, indices, total

    def bin_bounds(self, results, queries=None, tile_size=16, max_per_tile=0, phase=1, flags=0, want_counts=True, want_depth=True,
                   want_totals=True, item_fill=0xFFFFFFFF):
        """chordvis_bin_bounds: the visible boxes of a bounds query binned into screen tiles of tile_size pixels.  results: a numpy
        array of records.BOUNDS_RESULT (what query_bounds returned), or a contiguous CUDA tensor of such records (16 bytes each) on
        the context's device; queries (needed by records.BOUNDS_TILES_FAR only): records.BOUNDS_QUERY, likewise.  Returns a dict, read
        back: tiles (tilesX, tilesY); counts uint32[tiles] (None unless want_counts); items uint32[tiles, max_per_tile] (None when
        max_per_tile is 0) -- row t holds min(counts[t], max_per_tile) ascending query indices, the words behind them keep
        item_fill --; depth uint32[tiles, 2], far and near bits (None unless want_depth); totals uint32[4] (None unless want_totals).
        The call is ordered behind the current torch stream and that one behind the call (as query_bounds does it); a caller's
        tensor handed in has the context's stream recorded on it, so release it before close()."""
        import torch
        dev = torch.device("cuda", self.device)

        def records(a, dtype, what):
            if a is None:
                return None, 0
            if isinstance(a, np.ndarray):
                host = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
                with torch.cuda.device(dev):
                    t = torch.from_numpy(host.view(np.uint8).copy()).to(dev) if len(host) else torch.zeros(16, dtype=torch.uint8, device=dev)
                return t, len(host)
            nbytes = a.numel() * a.element_size()
            assert a.is_cuda and a.is_contiguous() and nbytes % dtype.itemsize == 0, "bin_bounds: %s: a contiguous CUDA tensor of %d-byte records" % (what, dtype.itemsize)
            return a, nbytes // dtype.itemsize

        res, count = records(results, R.BOUNDS_RESULT, "results")
        qry, qcount = records(queries, R.BOUNDS_QUERY, "queries")
        assert qry is None or qcount == count, "bin_bounds: results and queries belong together"
        tx, ty = C.c_uint32(0), C.c_uint32(0)
        tiles = int(L.lib.chordvis_bounds_tile_count(self.width, self.height, int(tile_size), C.byref(tx), C.byref(ty)))
        max_per_tile = int(max_per_tile)
        with torch.cuda.device(dev):
            cnt = torch.zeros(max(tiles, 1), dtype=torch.int32, device=dev) if want_counts else None
            fill = int(np.uint32(item_fill).view(np.int32))
            items = torch.full((max(tiles * max_per_tile, 1),), fill, dtype=torch.int32, device=dev) if max_per_tile else None
            depth = torch.zeros(max(2 * tiles, 1), dtype=torch.int32, device=dev) if want_depth else None
            totals = torch.zeros(4, dtype=torch.int32, device=dev) if want_totals else None
        desc = L.BoundsTilesDesc(int(tile_size), max_per_tile, int(phase), int(flags))
        out = L.BoundsTiles(*(t.data_ptr() if t is not None else None for t in (cnt, items, depth, totals)))
        used = [t for t in (res, qry, cnt, items, depth, totals) if t is not None]
        self._on_my_stream(used, lambda: self._check(L.lib.chordvis_bin_bounds(
            self._ctx, C.byref(desc), res.data_ptr() if res is not None and count else None,
            qry.data_ptr() if qry is not None else None, count, C.byref(out)), "bin_bounds"))
        self.sync()
        host = lambda t, n: t.cpu().numpy().view(np.uint32)[:n].copy() if t is not None else None
        got_items = host(items, tiles * max_per_tile)
        got_depth = host(depth, 2 * tiles)
        return dict(tiles=(tx.value, ty.value), counts=host(cnt, tiles),
                    items=got_items.reshape(tiles, max_per_tile) if got_items is not None else None,
                    depth=got_depth.reshape(tiles, 2) if got_depth is not None else None, totals=host(totals, 4))

    def texture_mips(self, texture):
        """(levels, flags, alphaCutoff8, pad) set for a texture id; zeros where nothing is set."""
        m = L.TextureMips()
        self._check(L.lib.chordvis_texture_mips(self._ctx, int(texture), C.byref(m)), "texture_mips")
        return (m.levels, m.flags, m.alphaCutoff8, m.pad)

    def update_objects(self, objects):
        objects = np.ascontiguousarray(objects, dtype=R.OBJECT)
        self._check(L.lib.chordvis_update_objects(self._ctx, objects.ctypes.data, len(objects)), "update_objects")

    def bind_objects(self, device_ptr, count):
        self._check(L.lib.chordvis_bind_objects(self._ctx, device_ptr, count), "bind_objects")

    def set_object_list(self, objects):
        """chordvis_set_object_list: another object list -- any count >= 1, any primitives and materials of the resident scene -- without
        uploading the scene again; the history HZB and the material textures stay.  objects: records.OBJECT records, or a records.Scene
        over the same assets (scene.with_objects(...)), which then becomes self.scene (what read_objects and the other helpers size
        their arrays by).  Never waits while the list fits what earlier lists had allocated.  A refusal leaves the context as it was."""
        scene = objects if isinstance(objects, R.Scene) else None
        records = np.ascontiguousarray(scene.objects if scene is not None else objects, dtype=R.OBJECT)
        self._check(L.lib.chordvis_set_object_list(self._ctx, records.ctypes.data if len(records) else None, len(records)), "set_object_list")
        if scene is not None:
            self.scene = scene

    # -- object records built on the device (chordvis_build_objects) -------------------------------
    def upload_world_transforms(self, local_to_world, prev_local_to_world=None):
        """chordvis_upload_world_transforms: the objects' f64 world matrices (n, 16) or (n, 4, 4) glm column-major, resident on the
        device from here on; prev_local_to_world None: = current.  Waits for the stream."""
        cur = np.ascontiguousarray(local_to_world, dtype=np.float64).reshape(-1, 16)
        prev = None if prev_local_to_world is None else np.ascontiguousarray(prev_local_to_world, dtype=np.float64).reshape(-1, 16)
        assert prev is None or prev.shape == cur.shape
        self._check(L.lib.chordvis_upload_world_transforms(self._ctx, cur.ctypes.data, prev.ctypes.data if prev is not None else None, len(cur)),
                    "upload_world_transforms")

    def scatter_world_transforms(self, indices, matrices, n=None):
        """chordvis_scatter_world_transforms, one launch that never waits: cur[indices[k]] = matrices[k].  indices / matrices: CUDA
        tensors on the context's device (int32 / uint32 words, float64 x 16 per matrix, contiguous; ordered against the context's
        stream both ways like the resolves' tensors), or raw device pointers (ints) with n given -- those are the caller's to order."""
        if isinstance(indices, int) or isinstance(matrices, int):
            assert isinstance(indices, int) and isinstance(matrices, int) and n is not None, "scatter_world_transforms: raw pointers come with n"
            self._check(L.lib.chordvis_scatter_world_transforms(self._ctx, indices or None, matrices or None, int(n)), "scatter_world_transforms")
            return
        import torch
        assert indices.is_cuda and matrices.is_cuda and indices.is_contiguous() and matrices.is_contiguous()
        assert indices.element_size() == 4 and matrices.dtype == torch.float64
        count = indices.numel() if n is None else int(n)
        assert count <= indices.numel() and matrices.numel() >= 16 * count
        self._on_my_stream([indices, matrices], lambda: self._check(L.lib.chordvis_scatter_world_transforms(
            self._ctx, indices.data_ptr() if count else None, matrices.data_ptr() if count else None, count), "scatter_world_transforms"))

    def build_objects(self, camera_pos, camera_pos_last=None):
        """chordvis_build_objects, one launch that never waits: the camera-relative records of every object from the resident
        transforms.  camera_pos / camera_pos_last: three doubles each (a scenes.Camera's .position); None: = camera_pos."""
        cam = (C.c_double * 3)(*[float(v) for v in camera_pos])
        last = None if camera_pos_last is None else (C.c_double * 3)(*[float(v) for v in camera_pos_last])
        self._check(L.lib.chordvis_build_objects(self._ctx, cam, last), "build_objects")

    def build_objects_status(self):
        """(singular objects of the latest build, the first one's index or 0xFFFFFFFF).  Synchronises."""
        n, first = C.c_uint32(0), C.c_uint32(0)
        self._check(L.lib.chordvis_build_objects_status(self._ctx, C.byref(n), C.byref(first)), "build_objects_status")
        return n.value, first.value

    def read_objects(self, count=None):
        """records.OBJECT array: the object array frames read now (chordvis_readback_objects).  Synchronises."""
        out = np.zeros(len(self.scene.objects) if count is None else int(count), dtype=R.OBJECT)
        self._check(L.lib.chordvis_readback_objects(self._ctx, out.ctypes.data, len(out)), "readback_objects")
        return out

    def read_world_transforms(self, count=None):
        """(cur, prev) float64 (n, 16): the resident world transforms (chordvis_readback_world_transforms).  Synchronises."""
        n = len(self.scene.objects) if count is None else int(count)
        cur, prev = np.zeros((n, 16), dtype=np.float64), np.zeros((n, 16), dtype=np.float64)
        self._check(L.lib.chordvis_readback_world_transforms(self._ctx, cur.ctypes.data, prev.ctypes.data, n), "readback_world_transforms")
        return cur, prev

    # -- ray queries on the resident scene (chordvis_build_ray_scene / chordvis_trace_rays) ---------
    def build_ray_scene(self):
        """chordvis_build_ray_scene: a BLAS per primitive (kept until the next upload_scene) and the TLAS of the current object list,
        refitted.  May wait.  Returns an L.RaySceneInfo."""
        info = L.RaySceneInfo()
        self._check(L.lib.chordvis_build_ray_scene(self._ctx, C.byref(info)), "build_ray_scene")
        return info

    def refit_ray_scene(self):
        """chordvis_refit_ray_scene, one launch that never waits: the TLAS boxes from the object array the frames read now."""
        self._check(L.lib.chordvis_refit_ray_scene(self._ctx), "refit_ray_scene")

    def ray_scene_info(self):
        """chordvis_ray_scene_info: counts and the TLAS root's box, read from the device.  Synchronises."""
        info = L.RaySceneInfo()
        self._check(L.lib.chordvis_ray_scene_info(self._ctx, C.byref(info)), "ray_scene_info")
        return info

    def rebuild_ray_tlas(self):
        """chordvis_rebuild_ray_tlas: the TLAS topology of the current object list built on the device, in stream order, and refitted.
        Needs one build_ray_scene since the last upload_scene.  Waits only for a list longer than every list rebuilt before."""
        self._check(L.lib.chordvis_rebuild_ray_tlas(self._ctx), "rebuild_ray_tlas")

    def read_ray_tlas(self, count=None):
        """(records.RAY_NODE array of tlasNodes nodes, uint32 leafRef per object) of the TLAS, whichever builder made it
        (chordvis_readback_ray_tlas).  count: the current list's object count (None: self.scene's).  Synchronises."""
        info = self.ray_scene_info()
        count = len(self.scene.objects) if count is None else int(count)
        nodes = np.zeros(info.tlasNodes, dtype=R.RAY_NODE)
        leaf_ref = np.zeros(count, dtype=np.uint32)
        self._check(L.lib.chordvis_readback_ray_tlas(self._ctx, nodes.ctypes.data, len(nodes), leaf_ref.ctypes.data, len(leaf_ref)), "readback_ray_tlas")
        return nodes, leaf_ref

    def trace_rays(self, rays, any_hit=False, out=None):
        """chordvis_trace_rays, one launch that never waits.  rays: a contiguous CUDA tensor of records.RAY records (32 bytes each, e.g.
        float32 (n, 8)) on the context's device, or a numpy array of records.RAY, which is copied there.  Returns an int32 CUDA tensor
        (n, 8) of records.RAY_HIT words (out: a tensor to write into); .cpu().numpy().view(records.RAY_HIT) reads them.  The call is
        ordered behind the current torch stream and that one behind the call."""
        import torch
        dev = torch.device("cuda", self.device)
        if isinstance(rays, np.ndarray):
            host = np.ascontiguousarray(rays, dtype=R.RAY).reshape(-1)
            with torch.cuda.device(dev):
                rays = torch.from_numpy(host.view(np.uint8).copy()).to(dev) if len(host) else torch.zeros(0, dtype=torch.uint8, device=dev)
        nbytes = rays.numel() * rays.element_size()
        assert rays.is_cuda and rays.is_contiguous() and nbytes % R.RAY.itemsize == 0, "trace_rays: a contiguous CUDA tensor of 32-byte records"
        count = nbytes // R.RAY.itemsize
        if out is None:
            with torch.cuda.device(dev):
                out = torch.empty((count, 8), dtype=torch.int32, device=dev)
        assert out.is_cuda and out.is_contiguous() and out.numel() * out.element_size() == count * R.RAY_HIT.itemsize
        self._on_my_stream([rays, out], lambda: self._check(L.lib.chordvis_trace_rays(
            self._ctx, rays.data_ptr() if count else None, count, L.RAY_ANY_HIT if any_hit else 0, out.data_ptr() if count else None), "trace_rays"))
        return out

    def shade_ray_hits(self, hits, lod=0.0, lods=None, out=None):
        """chordvis_shade_ray_hits, one launch that never waits: material, normal and uv at every hit.  hits: a contiguous CUDA tensor
        of records.RAY_HIT records (32 bytes each, e.g. what trace_rays returns) on the context's device, or a numpy array of
        records.RAY_HIT, which is copied there.  lod: the texture level of every hit; lods: a level per hit instead, a float32 CUDA
        tensor or a numpy array of n values.  Needs upload_material_textures and no ray scene.  Returns an int32 CUDA tensor (n, 16)
        of records.RAY_HIT_SURFACE words (out: a tensor to write into); .cpu().numpy().view(records.RAY_HIT_SURFACE) reads them.

        Ordering and lifetime: the context's stream waits for the current torch stream before the call and the current torch stream
        waits for the context's stream after it, so every later use of hits, lods and the result on the current stream -- the
        allocator's reuse of their memory after a free included, which is ordered on that stream -- is behind the kernel.  No tensor
        is recorded on the context's stream.  A caller who frees or reuses these tensors on a third stream orders that stream itself."""
        import torch
        dev = torch.device("cuda", self.device)
        if isinstance(hits, np.ndarray):
            host = np.ascontiguousarray(hits, dtype=R.RAY_HIT).reshape(-1)
            with torch.cuda.device(dev):
                hits = torch.from_numpy(host.view(np.uint8).copy()).to(dev) if len(host) else torch.zeros(0, dtype=torch.uint8, device=dev)
        nbytes = hits.numel() * hits.element_size()
        assert hits.is_cuda and hits.is_contiguous() and nbytes % R.RAY_HIT.itemsize == 0, "shade_ray_hits: a contiguous CUDA tensor of 32-byte records"
        assert hits.device.index == self.device, "shade_ray_hits: hits is on cuda:%s, the context on cuda:%d" % (hits.device.index, self.device)
        count = nbytes // R.RAY_HIT.itemsize
        if lods is not None:
            if isinstance(lods, np.ndarray):
                host = np.ascontiguousarray(lods, dtype=np.float32).reshape(-1)
                with torch.cuda.device(dev):
                    lods = torch.from_numpy(host.copy()).to(dev) if len(host) else torch.zeros(0, dtype=torch.float32, device=dev)
            assert lods.is_cuda and lods.is_contiguous() and lods.dtype == torch.float32 and lods.numel() == count, "shade_ray_hits: lods is n float32 values"
            assert lods.device.index == self.device, "shade_ray_hits: lods is on cuda:%s, the context on cuda:%d" % (lods.device.index, self.device)
        if out is None:
            with torch.cuda.device(dev):
                out = torch.empty((count, 16), dtype=torch.int32, device=dev)
        assert out.is_cuda and out.is_contiguous() and out.numel() * out.element_size() == count * R.RAY_HIT_SURFACE.itemsize
        assert out.device.index == self.device, "shade_ray_hits: out is on cuda:%s, the context on cuda:%d" % (out.device.index, self.device)
        self._on_my_stream([], lambda: self._check(L.lib.chordvis_shade_ray_hits(
            self._ctx, hits.data_ptr() if count else None, count, float(lod), lods.data_ptr() if (lods is not None and count) else None,
            out.data_ptr() if count else None), "shade_ray_hits"))
        return out

    def pixel_rays(self, position, normal=None, mode=L.PIXEL_RAYS_HEMISPHERE, table=None, direction=(0.0, 0.0, 0.0), ray_length=1.0, t_min=0.0,
                   z_near=0.0, depth=None, depth_stride=1, any_hit=False, front_only=False, start_from_depth=False, hits=False, out=None,
                   out_hits=None):
        """chordvis_pixel_rays, one launch that never waits: a ray per pixel of the position and normal images, traced and reduced to
        one float per pixel.  position, normal: contiguous float32 CUDA tensors (height, width, 4) on the context's device (what
        resolve_attributes returns as positionRS and vertexNormal / pixelNormal); normal may be None for L.PIXEL_RAYS_DIRECTION without
        front_only.  table: (tableH, tableW, 4) float32, the tangent-space directions of L.PIXEL_RAYS_HEMISPHERE.  depth: None, a
        float32 CUDA tensor of height * width * depth_stride values, or a device address (an int: visibility_ptr() + 4 with
        depth_stride=2 reads the depth halves of the visibility image in place).  hits=True (or out_hits) also writes the closest
        hits.  Returns the (height, width) float32 image, or (image, (height * width, 8) int32 records.RAY_HIT words) with hits.

        Ordering and lifetime as in shade_ray_hits: the context's stream waits for the current torch stream before the call and the
        current torch stream waits for the context's stream after it; no tensor is recorded on the context's stream."""
        import torch
        dev = torch.device("cuda", self.device)

        def image(t, what, channels=4):
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.device.index == self.device, \
                "pixel_rays: %s is a contiguous float32 tensor on cuda:%d" % (what, self.device)
            assert t.dim() == 3 and t.shape[2] == channels, "pixel_rays: %s is (height, width, %d)" % (what, channels)
            return t
        image(position, "position")
        height, width = int(position.shape[0]), int(position.shape[1])
        if normal is not None:
            assert tuple(image(normal, "normal").shape) == tuple(position.shape), "pixel_rays: normal is of position's size"
        d = L.PixelRaysDesc()
        d.width, d.height, d.mode = width, height, int(mode)
        d.flags = (L.PIXEL_RAYS_ANY_HIT if any_hit else 0) | (L.PIXEL_RAYS_FRONT_ONLY if front_only else 0) | \
                  (L.PIXEL_RAYS_START_FROM_DEPTH if start_from_depth else 0)
        if table is not None:
            image(table, "table")
            d.tableH, d.tableW = int(table.shape[0]), int(table.shape[1])
        d.direction[:] = [float(v) for v in direction]
        d.rayLength, d.tMin, d.zNear = float(ray_length), float(t_min), float(z_near)
        zp = None
        if depth is not None:
            d.deviceZStride = int(depth_stride)
            if isinstance(depth, int):
                zp = depth
            else:
                assert depth.is_cuda and depth.is_contiguous() and depth.dtype == torch.float32 and depth.device.index == self.device
                assert depth.numel() >= width * height * int(depth_stride), "pixel_rays: depth holds height * width * depth_stride values"
                zp = depth.data_ptr()
        want_hits = bool(hits) or out_hits is not None
        if out is None:
            with torch.cuda.device(dev):
                out = torch.empty((height, width), dtype=torch.float32, device=dev)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.numel() == width * height and out.device.index == self.device
        if want_hits and out_hits is None:
            with torch.cuda.device(dev):
                out_hits = torch.empty((width * height, 8), dtype=torch.int32, device=dev)
        if want_hits:
            assert out_hits.is_cuda and out_hits.is_contiguous() and out_hits.numel() * out_hits.element_size() == width * height * R.RAY_HIT.itemsize
            assert out_hits.device.index == self.device
        n = width * height
        self._on_my_stream([], lambda: self._check(L.lib.chordvis_pixel_rays(
            self._ctx, C.byref(d), position.data_ptr() if n else None, normal.data_ptr() if (normal is not None and n) else None, zp,
            table.data_ptr() if table is not None else None, out.data_ptr() if n else None,
            out_hits.data_ptr() if (want_hits and n) else None), "pixel_rays"))
        return (out, out_hits) if want_hits else out

    def allocate_gbuffer(self, width, height, device_visibility=None):
        self._check(L.lib.chordvis_allocate_gbuffer(self._ctx, width, height, device_visibility), "allocate_gbuffer")
        self.width, self.height = width, height

    def set_cull_mode(self, hierarchical):
        """0: flat group cull (the reference's dispatch); 1: walk the primitives' BVHs (same command list)."""
        self._check(L.lib.chordvis_set_cull_mode(self._ctx, int(hierarchical)), "set_cull_mode")

    def set_tile_schedule_keep(self, frames):
        """Non-zero (default 1): a raster pass runs under the tile schedule the frame before made for it; 0: a fresh schedule every pass."""
        self._check(L.lib.chordvis_set_tile_schedule_keep(self._ctx, int(frames)), "set_tile_schedule_keep")

    def tile_schedule_keep(self):
        return int(L.lib.chordvis_tile_schedule_keep(self._ctx))

    def set_shard(self, ranks, rank):
        """Screen ownership by 64 x 64 tiles: the default map (compact regions along a generalised Hilbert curve)."""
        self._check(L.lib.chordvis_set_shard(self._ctx, ranks, rank), "set_shard")

    def set_tile_owners(self, owners):
        """An explicit tile map (one owner per tile); None: the default map."""
        if owners is None:
            self._check(L.lib.chordvis_set_tile_owners(self._ctx, None, 0), "set_tile_owners")
            return
        owners = np.ascontiguousarray(owners, dtype=np.uint8)
        self._check(L.lib.chordvis_set_tile_owners(self._ctx, owners.ctypes.data, len(owners)), "set_tile_owners")

    def tile_owners(self):
        out = np.zeros(int(L.lib.chordvis_tile_count(self.width, self.height)), dtype=np.uint8)
        self._check(L.lib.chordvis_get_tile_owners(self._ctx, out.ctypes.data, len(out)), "get_tile_owners")
        return out

    def read_tile_loads(self):
        """Bin entries per tile of the last frame (every rank's tiles, after the end-of-frame exchange)."""
        out = np.zeros(int(L.lib.chordvis_tile_count(self.width, self.height)), dtype=np.uint32)
        self._check(L.lib.chordvis_read_tile_loads(self._ctx, out.ctypes.data, len(out)), "read_tile_loads")
        return out

    def rebalance(self):
        """Tile map from the last frame's loads; returns the old map's heaviest rank / mean."""
        imb = C.c_uint32(0)
        self._check(L.lib.chordvis_rebalance(self._ctx, C.byref(imb)), "rebalance")
        return imb.value / 1000.0

    def set_view(self, view, instance_view, flags):
        self._views = (view, instance_view)       # keep alive
        self._check(L.lib.chordvis_set_view(self._ctx, view.ctypes.data, instance_view.ctypes.data, flags), "set_view")

    # -- buffers for collectives ------------------------------------------------------------------
    def visibility_words(self):
        return int(L.lib.chordvis_visibility_words(self._ctx))

    def visibility_chunk_words(self):
        return int(L.lib.chordvis_visibility_chunk_words(self._ctx))

    def visibility_ptr(self):
        return L.lib.chordvis_visibility_ptr(self._ctx)

    def resolved_visibility_ptr(self):
        return L.lib.chordvis_resolved_visibility_ptr(self._ctx)

    def hzb_exchange(self):
        """(device pointer, halves, halves per rank) of the mid-frame exchange buffer."""
        return (L.lib.chordvis_hzb_exchange_ptr(self._ctx), int(L.lib.chordvis_hzb_exchange_halves(self._ctx)),
                int(L.lib.chordvis_hzb_exchange_chunk_halves(self._ctx)))

    def hzb_final_exchange(self):
        """(device pointer, bytes per rank) of the end-of-frame exchange buffer."""
        return (L.lib.chordvis_hzb_final_exchange_ptr(self._ctx), int(L.lib.chordvis_hzb_final_exchange_chunk_bytes(self._ctx)))

    # -- passes -------------------------------------------------------------------------------------
    def clear_gbuffer(self):
        self._check(L.lib.chordvis_clear_gbuffer(self._ctx), "clear_gbuffer")

    def instance_culling(self):
        out = L.CountAndCmd()
        self._check(L.lib.chordvis_instance_culling(self._ctx, C.byref(out)), "instance_culling")
        return out

    def hzb_culling(self, hzb, first_stage, in_list):
        vis, rej = L.CountAndCmd(), L.CountAndCmd()
        self._check(L.lib.chordvis_hzb_culling(self._ctx, C.byref(hzb), int(first_stage), in_list, C.byref(vis), C.byref(rej)), "hzb_culling")
        return vis, rej

    def render_mesh(self, in_list):
        self._check(L.lib.chordvis_render_mesh(self._ctx, in_list), "render_mesh")

    def visibility_stage0(self, hzb_prev, in_list):
        rej, flag = L.CountAndCmd(), C.c_int(0)
        self._check(L.lib.chordvis_visibility_stage0(self._ctx, C.byref(hzb_prev) if hzb_prev is not None else None,
                                                      in_list, C.byref(rej), C.byref(flag)), "visibility_stage0")
        return bool(flag.value), rej

    def visibility_stage1(self, hzb, in_list):
        self._check(L.lib.chordvis_visibility_stage1(self._ctx, C.byref(hzb), in_list), "visibility_stage1")

    def build_hzb(self, build_min=True, build_max=False, build_valid_range=False, slot=0):
        out = L.HZB()
        self._check(L.lib.chordvis_build_hzb(self._ctx, int(build_min), int(build_max), int(build_valid_range), slot, C.byref(out)), "build_hzb")
        return out

    def render_frame(self):
        self._check(L.lib.chordvis_render_frame(self._ctx), "render_frame")

    def frame_phase_cull(self):
        """Sharded group cull, first half: this rank's share of the group tests -> rank-mask words (all-gather cull_exchange() next)."""
        self._check(L.lib.chordvis_frame_phase_cull(self._ctx), "frame_phase_cull")

    def cull_exchange(self):
        """(device pointer, bytes per rank) of the sharded cull's exchange buffer; (None, 0) when the sharded cull does not apply."""
        return (L.lib.chordvis_cull_exchange_ptr(self._ctx), int(L.lib.chordvis_cull_exchange_chunk_bytes(self._ctx)))

    def debug_fill_cull_exchange(self):
        """Measurement aid: every rank's chunk of the cull exchange buffer computed on this context (one rank timed alone)."""
        self._check(L.lib.chordvis_debug_fill_cull_exchange(self._ctx), "debug_fill_cull_exchange")

    def frame_phase_a(self):
        self._check(L.lib.chordvis_frame_phase_a(self._ctx), "frame_phase_a")

    def frame_phase_b(self):
        self._check(L.lib.chordvis_frame_phase_b(self._ctx), "frame_phase_b")

    def frame_phase_c(self):
        self._check(L.lib.chordvis_frame_phase_c(self._ctx), "frame_phase_c")

    # -- one process per GPU: RCCL communicator owned by the library ---------------------------------
    def comm_init_rank(self, nranks, rank, unique_id):
        """Attach an RCCL communicator (after set_shard); render_frame() then runs the two all-gathers itself."""
        buf = (C.c_char * 128).from_buffer_copy(bytes(unique_id))
        self._check(L.lib.chordvis_comm_init_rank(self._ctx, nranks, rank, buf), "comm_init_rank")

    def comm_set_pipelined(self, unique_id):
        """Second communicator (its own unique id, or None to switch off): the image of frame i travels beside frame i + 1."""
        buf = (C.c_char * 128).from_buffer_copy(bytes(unique_id)) if unique_id is not None else None
        self._check(L.lib.chordvis_comm_set_pipelined(self._ctx, buf), "comm_set_pipelined")

    def comm_destroy(self):
        self._check(L.lib.chordvis_comm_destroy(self._ctx), "comm_destroy")

    def comm_info(self):
        return comm_info(self._ctx)

    def reset_history(self):
        self._check(L.lib.chordvis_reset_history(self._ctx), "reset_history")

    def last_frame_cmds(self):
        out = L.CountAndCmd()
        self._check(L.lib.chordvis_last_frame_cmds(self._ctx, C.byref(out)), "last_frame_cmds")
        return out

    def history_hzb(self):
        out = L.HZB()
        self._check(L.lib.chordvis_history_hzb(self._ctx, C.byref(out)), "history_hzb")
        return out

    def upload_history_hzb(self, hzb_min):
        hzb_min = np.ascontiguousarray(hzb_min, dtype=np.uint16)
        self._check(L.lib.chordvis_upload_history_hzb(self._ctx, hzb_min.ctypes.data), "upload_history_hzb")

    def set_limits(self, max_triangle_records=0, bin_pool_chunks=0, bin_max_chunks_per_tile=0):
        """Work-list capacities (before upload_scene / allocate_gbuffer); 0 keeps a default."""
        lim = L.Limits(int(max_triangle_records), int(bin_pool_chunks), int(bin_max_chunks_per_tile))
        self._check(L.lib.chordvis_set_limits(self._ctx, C.byref(lim)), "set_limits")

    # -- depth-only views (renderShadow's passes, mesh_raster.cpp:331-546) ------------------------------------
    def allocate_depth_views(self, dim, view_count):
        self._check(L.lib.chordvis_allocate_depth_views(self._ctx, dim, view_count), "allocate_depth_views")

    def set_instance_views(self, views):
        views = np.ascontiguousarray(views, dtype=R.INSTANCE_CULLING_VIEW)
        self._check(L.lib.chordvis_set_instance_views(self._ctx, views.ctypes.data, len(views)), "set_instance_views")

    def instance_culling_view(self, view_offset):
        out = L.CountAndCmd()
        self._check(L.lib.chordvis_instance_culling_view(self._ctx, view_offset, C.byref(out)), "instance_culling_view")
        return out

    def hzb_culling_generic(self, hzb, extent_scale, view_offset, use_last_frame, in_list):
        out = L.CountAndCmd()
        self._check(L.lib.chordvis_hzb_culling_generic(self._ctx, C.byref(hzb), extent_scale, view_offset, int(use_last_frame), in_list, C.byref(out)),
                    "hzb_culling_generic")
        return out

    def render_mesh_depth(self, view_offset, in_list, depth_clamped=True, bias_const=0.0, bias_slope=0.0):
        out = L.DepthTarget()
        self._check(L.lib.chordvis_render_mesh_depth(self._ctx, view_offset, int(depth_clamped), bias_const, bias_slope, in_list, C.byref(out)),
                    "render_mesh_depth")
        return out

    def build_hzb_from_depth(self, depth):
        out = L.HZB()
        self._check(L.lib.chordvis_build_hzb_from_depth(self._ctx, C.byref(depth), C.byref(out)), "build_hzb_from_depth")
        return out

    def read_depth(self, depth):
        out = np.empty(depth.width * depth.height, dtype=np.float32)
        self._check(L.lib.chordvis_readback_depth(self._ctx, C.byref(depth), out.ctypes.data), "readback_depth")
        return out

    def render_shadow(self, config, light_dir, tick, valid_range=None, hzb_culling=True):
        """renderShadow: returns (depth targets, views, mask of the cascades re-rendered by this call)."""
        n = int(config["cascadeCount"][0])
        depths = (L.DepthTarget * n)()
        views = np.zeros(n, dtype=R.INSTANCE_CULLING_VIEW)
        ld = np.asarray(light_dir, dtype=np.float32)
        vr = None if valid_range is None else np.asarray(valid_range, dtype=np.uint32)
        mask = C.c_uint32(0)
        self._check(L.lib.chordvis_render_shadow(self._ctx, config.ctypes.data, ld.ctypes.data, vr.ctypes.data if vr is not None else None,
                                                 int(tick), int(hzb_culling), depths, views.ctypes.data, C.byref(mask)), "render_shadow")
        return list(depths), views, mask.value

    def depth_view_stats(self):
        st = L.Stats()
        self._check(L.lib.chordvis_depth_view_stats(self._ctx, C.byref(st)), "depth_view_stats")
        return st.as_dict()

    # -- consumers' first step (visibility_tile.cpp) -------------------------------------------------------
    def visibility_mark(self, drawed_meshlet_cmd=None):
        """visibilityMark (visibility_tile.cpp:20-57); the command list defaults to last_frame_cmds()."""
        out = L.TileMarker()
        cmd = drawed_meshlet_cmd if drawed_meshlet_cmd is not None else self.last_frame_cmds()
        self._check(L.lib.chordvis_visibility_mark(self._ctx, cmd, C.byref(out)), "visibility_mark")
        return out

    def wait_visibility(self, stream=None):
        """Orders `stream` (default: the context's) behind the completion of the last frame's resolved image."""
        self._check(L.lib.chordvis_wait_visibility(self._ctx, stream), "wait_visibility")

    def stream(self):
        """The hipStream_t (as an int) the context enqueues on."""
        return L.lib.chordvis_stream(self._ctx) or 0

    def resolve_attributes(self, names=None, desc=None, drawed_meshlet_cmd=None, out=None):
        """Per-pixel attributes of the visible triangle (lighting.hlsl:278-371, material.hlsli:41-64, nanite_debug.hlsl) in ONE
        launch: {name: tensor} for `names` (default: every target of L.RESOLVE_CHANNELS), each (height, width, channels) float32
        ((height, width) int32 holding RGBA8 for "debugRGBA8") on the context's device.  desc: an L.ResolveDesc or None (all zero).
        out: {name: tensor} to write into instead of fresh tensors.  The tensors are ordered against the context's stream
        both ways: the resolve waits for the current torch stream, which in turn waits for the resolve.
        Names of L.SURFACE_CHANNELS (vertexNormal, tangent, bitangent; float4 each) may be asked for too: the call then goes through
        chordvis_resolve_surface, still one launch (the scene must have been uploaded with normals / tangents).  Likewise the names
        of L.MATERIAL_CHANNELS (baseColor, emissive, pixelNormal, roughMetalAO; float4 each): the call then goes through
        chordvis_resolve_material (after upload_material_textures), one launch for any subset of the fifteen."""
        import torch
        names = list(L.RESOLVE_CHANNELS) if names is None else list(names)
        channels = dict(L.RESOLVE_CHANNELS, **L.SURFACE_CHANNELS, **L.MATERIAL_CHANNELS)
        bad = [n for n in names if n not in channels]
        if bad or not names:
            raise ValueError("resolve_attributes: unknown or no target names %r (known: %s)" % (bad, ", ".join(channels)))
        dev = torch.device("cuda", self.device)
        mine = torch.cuda.ExternalStream(self.stream(), device=dev)
        cur = torch.cuda.current_stream(dev)
        res = {}
        for n in names:
            if out is not None and n in out:
                t = out[n]
            else:
                ch = channels[n]
                shape = (self.height, self.width) if ch == 1 else (self.height, self.width, ch)
                with torch.cuda.device(dev):
                    t = torch.empty(shape, dtype=torch.int32 if n == "debugRGBA8" else torch.float32, device=dev)
            assert t.is_contiguous() and t.numel() == self.width * self.height * channels[n], n
            res[n] = t
        targets = L.ResolveTargets(**{n: t.data_ptr() for n, t in res.items() if n in L.RESOLVE_CHANNELS})
        surface = {n: t.data_ptr() for n, t in res.items() if n in L.SURFACE_CHANNELS}
        material = {n: t.data_ptr() for n, t in res.items() if n in L.MATERIAL_CHANNELS}
        cmd = drawed_meshlet_cmd if drawed_meshlet_cmd is not None else self.last_frame_cmds()
        if mine.cuda_stream != cur.cuda_stream:
            mine.wait_stream(cur)                      # (the allocator may hand out memory torch work on `cur` still uses)
        d = C.byref(desc) if desc is not None else None
        if material:
            self._check(L.lib.chordvis_resolve_material(self._ctx, cmd, d, C.byref(targets), C.byref(L.SurfaceTargets(**surface)),
                                                        C.byref(L.MaterialTargets(**material))), "resolve_material")
        elif surface:
            self._check(L.lib.chordvis_resolve_surface(self._ctx, cmd, d, C.byref(targets), C.byref(L.SurfaceTargets(**surface))),
                        "resolve_surface")
        else:
            self._check(L.lib.chordvis_resolve_attributes(self._ctx, cmd, d, C.byref(targets)), "resolve_attributes")
        if mine.cuda_stream != cur.cuda_stream:
            cur.wait_stream(mine)
            for t in res.values():
                t.record_stream(mine)
        return res

    def _gbuffer_images(self, names, out, width, height, what):
        """{name: tensor} of packed images for `names` (default: all six of L.GBUFFER_IMAGES), taken from `out` where it has them"""
        import torch
        names = list(L.GBUFFER_IMAGES) if names is None else list(names)
        bad = [n for n in names if n not in L.GBUFFER_IMAGES]
        if bad or not names:
            raise ValueError("%s: unknown or no target names %r (known: %s)" % (what, bad, ", ".join(L.GBUFFER_IMAGES)))
        dev = torch.device("cuda", self.device)
        res = {}
        for n in names:
            lanes = L.GBUFFER_IMAGES[n][1]
            if out is not None and n in out:
                t = out[n]
            else:
                with torch.cuda.device(dev):
                    t = torch.empty((height, width, lanes), dtype=torch.float16, device=dev) if lanes else \
                        torch.empty((height, width), dtype=torch.int32, device=dev)
            assert t.is_contiguous() and t.numel() * t.element_size() == width * height * (2 * lanes or 4), n
            res[n] = t
        return res

    def _on_my_stream(self, tensors, call):
        """Runs call() with the context's stream ordered behind the current torch stream, and that one behind the call."""
        import torch
        dev = torch.device("cuda", self.device)
        mine = torch.cuda.ExternalStream(self.stream(), device=dev)
        cur = torch.cuda.current_stream(dev)
        if mine.cuda_stream != cur.cuda_stream:
            mine.wait_stream(cur)
        call()
        if mine.cuda_stream != cur.cuda_stream:
            cur.wait_stream(mine)
            for t in tensors:
                t.record_stream(mine)

    def resolve_gbuffer(self, names=None, out=None, desc=None, drawed_meshlet_cmd=None):
        """The G-buffer in the reference's packed formats (chordvis_resolve_gbuffer, ONE launch): {name: tensor} for `names` (default:
        all six of L.GBUFFER_IMAGES) on the context's device -- (height, width) int32 words for baseColor, vertexNormal, pixelNormal
        (A2B10G10R10_UNORM) and aoRoughnessMetallic (R8G8B8A8_UNORM), (height, width, 2) float16 for motionVector and
        (height, width, 4) float16 for emissive.  out: {name: tensor} to write into instead of fresh tensors.  desc and the stream
        ordering as in resolve_attributes: the tensors are recorded on the context's stream, so let go of them before close(),
        which destroys a stream the context owns."""
        res = self._gbuffer_images(names, out, self.width, self.height, "resolve_gbuffer")
        targets = L.GBufferTargets(**{n: t.data_ptr() for n, t in res.items()})
        cmd = drawed_meshlet_cmd if drawed_meshlet_cmd is not None else self.last_frame_cmds()
        d = C.byref(desc) if desc is not None else None
        self._on_my_stream(res.values(), lambda: self._check(L.lib.chordvis_resolve_gbuffer(self._ctx, cmd, d, C.byref(targets)), "resolve_gbuffer"))
        return res

    def pack_gbuffer(self, sources, names=None, out=None):
        """chordvis_pack_gbuffer: {name: tensor} as resolve_gbuffer returns them, converted from the float tensors in `sources`
        ({name as resolve_attributes returns it: (height, width, 4) float32, (height, width, 2) for motionVector}; roughMetalAO is
        the source of aoRoughnessMetallic).  names: the packed images wanted (default: those whose source is given).  A pure
        per-texel conversion: it knows nothing of coverage."""
        source_of = {n: s for n, (s, _) in L.GBUFFER_IMAGES.items()}
        names = [n for n in L.GBUFFER_IMAGES if source_of[n] in sources] if names is None else list(names)
        first = next(iter(sources.values()))
        height, width = int(first.shape[0]), int(first.shape[1])
        res = self._gbuffer_images(names, out, width, height, "pack_gbuffer")
        for n, t in sources.items():
            assert n in source_of.values() and t.is_contiguous() and tuple(t.shape[:2]) == (height, width) and t.element_size() == 4, n
        src = L.GBufferSources(**{n: t.data_ptr() for n, t in sources.items()})
        targets = L.GBufferTargets(**{n: t.data_ptr() for n, t in res.items()})
        self._on_my_stream(res.values(), lambda: self._check(
            L.lib.chordvis_pack_gbuffer(self._ctx, width, height, C.byref(src), C.byref(targets)), "pack_gbuffer"))
        return res

    def prepare_shading_tile_param(self, shading_type, marker):
        """prepareShadingTileParam (visibility_tile.cpp:59-110)."""
        out = L.ShadingTiles()
        self._check(L.lib.chordvis_prepare_shading_tile_param(self._ctx, int(shading_type), C.byref(marker), C.byref(out)),
                    "prepare_shading_tile_param")
        return out

    def read_tile_marker(self, marker):
        out = np.zeros((marker.markerDim[1], marker.markerDim[0], 4), dtype=np.uint32)
        self._check(L.lib.chordvis_readback_tile_marker(self._ctx, C.byref(marker), out.ctypes.data), "readback_tile_marker")
        return out

    def read_shading_tiles(self, tiles):
        out = np.zeros((max(1, tiles.capacity), 2), dtype=np.uint32)
        n = C.c_uint32(0)
        args = np.zeros(4, dtype=np.uint32)
        self._check(L.lib.chordvis_readback_shading_tiles(self._ctx, C.byref(tiles), out.ctypes.data, tiles.capacity,
                                                           C.byref(n), args.ctypes.data), "readback_shading_tiles")
        return out[:n.value].copy(), args

    # -- readback -------------------------------------------------------------------------------------
    def read_visibility(self):
        out = np.empty(self.width * self.height, dtype=np.uint64)
        self._check(L.lib.chordvis_readback_visibility(self._ctx, out.ctypes.data), "readback_visibility")
        return out

    def read_previous_visibility(self):
        """Pipelined sharded frames: the image of the frame before the last submitted one."""
        out = np.zeros(self.width * self.height, dtype=np.uint64)
        self._check(L.lib.chordvis_readback_previous_visibility(self._ctx, out.ctypes.data), "readback_previous_visibility")
        return out

    def read_cmds(self, handle):
        n = C.c_uint32(0)
        self._check(L.lib.chordvis_readback_cmds(self._ctx, handle, None, 0, C.byref(n)), "readback_cmds")
        out = np.zeros(max(1, n.value), dtype=R.DRAW_CMD)
        self._check(L.lib.chordvis_readback_cmds(self._ctx, handle, out.ctypes.data, len(out), C.byref(n)), "readback_cmds")
        return out[:n.value].copy()

    def read_hzb(self, hzb):
        n = hzb.desc.totalTexels
        mn = np.zeros(n, dtype=np.uint16)
        mx = np.zeros(n, dtype=np.uint16) if hzb.maxTexels else None
        rng = np.zeros(2, dtype=np.uint32) if hzb.validRange else None
        self._check(L.lib.chordvis_readback_hzb(self._ctx, C.byref(hzb), mn.ctypes.data,
                                                mx.ctypes.data if mx is not None else None,
                                                rng.ctypes.data if rng is not None else None), "readback_hzb")
        return mn, mx, rng

    def enable_timers(self, mode=1, period=1):
        """0 off, 1 last frame, 2 accumulate until stats(); only every `period`-th frame is stamped."""
        self._check(L.lib.chordvis_enable_timers(self._ctx, int(mode) | (int(period) << 8)), "enable_timers")

    def last_error(self):
        """Text of the last error this context reported (chordvis_last_error)."""
        msg = L.lib.chordvis_last_error(self._ctx)
        return msg.decode(errors="replace") if msg else ""

    def set_debug(self, flags):
        """Measurement-only ablation switches (0 = production)."""
        self._check(L.lib.chordvis_set_debug(self._ctx, int(flags)), "set_debug")

    def stats(self):
        st = L.Stats()
        self._check(L.lib.chordvis_stats(self._ctx, C.byref(st)), "stats")
        return st.as_dict()


def decode_visibility(vis):
    """(depth float32, slot int64 (-1 = empty), triangle uint8) from packed words — base.hlsli:437-447."""
    vis = np.asarray(vis, dtype=np.uint64)
    depth = (vis >> np.uint64(32)).astype(np.uint32).view(np.float32)
    low = (vis & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    tri = (low & 0xFF).astype(np.uint8)
    slot = ((low >> 8) & 0xFFFFFF).astype(np.int64) - 1
    return depth, slot, tri


def comm_unique_id():
    """ncclGetUniqueId through the library (rank 0; the host distributes the 128 bytes)."""
    buf = (C.c_char * 128)()
    rc = L.lib.chordvis_comm_unique_id(buf)
    if rc != L.OK:
        raise L.ChordvisError("chordvis_comm_unique_id failed (%d): librccl not loadable" % rc)
    return bytes(buf.raw)


def comm_info(ctx=None):
    ver, n = C.c_int(0), C.c_uint32(0)
    origin = C.create_string_buffer(256)
    rc = L.lib.chordvis_comm_info(ctx, C.byref(ver), C.byref(n), origin, 256)
    if rc != L.OK:
        raise L.ChordvisError("chordvis_comm_info failed (%d)" % rc)
    return {"nccl_version_code": ver.value, "ranks": n.value, "library": origin.value.decode()}


class VisibilityGroup:
    """ChordGroup: one process, n devices, one call per frame; the library issues the exchanges (direct peer copies)."""

    def __init__(self, devices):
        devices = list(devices)
        arr = (C.c_int * len(devices))(*devices)
        self._g = C.c_void_p()
        rc = L.lib.chordvis_create_group(len(devices), arr, C.byref(self._g))
        if rc != L.OK:
            raise L.ChordvisError("chordvis_create_group(%r) failed with %d" % (devices, rc))
        self.size = len(devices)
        self.ranks = [VisibilityRenderer(devices[r], _borrowed_ctx=L.lib.chordvis_group_ctx(self._g, r)) for r in range(self.size)]

    def _check(self, rc, what):
        if rc != L.OK:
            msg = L.lib.chordvis_group_last_error(self._g)
            raise L.ChordvisError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""))

    def close(self):
        if self._g:
            for r in self.ranks:
                r.close()
            L.lib.chordvis_destroy_group(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_limits(self, max_triangle_records=0, bin_pool_chunks=0, bin_max_chunks_per_tile=0):
        lim = L.Limits(int(max_triangle_records), int(bin_pool_chunks), int(bin_max_chunks_per_tile))
        self._check(L.lib.chordvis_group_set_limits(self._g, C.byref(lim)), "group_set_limits")

    def upload_scene(self, scene):
        self.scene = scene
        self._check(L.lib.chordvis_group_upload_scene(self._g, C.byref(scene.desc)), "group_upload_scene")

    def allocate_gbuffer(self, width, height):
        self._check(L.lib.chordvis_group_allocate_gbuffer(self._g, width, height), "group_allocate_gbuffer")
        for r in self.ranks:
            r.width, r.height = width, height

    def rebalance(self):
        """chordvis_group_rebalance: every rank's tile map from the last frame's loads; returns the old map's heaviest rank / mean."""
        imb = C.c_uint32(0)
        self._check(L.lib.chordvis_group_rebalance(self._g, C.byref(imb)), "group_rebalance")
        return imb.value / 1000.0

    def update_objects(self, objects):
        objects = np.ascontiguousarray(objects, dtype=R.OBJECT)
        self._check(L.lib.chordvis_group_update_objects(self._g, objects.ctypes.data, len(objects)), "group_update_objects")

    def set_object_list(self, objects):
        """chordvis_group_set_object_list: VisibilityRenderer.set_object_list on every rank (records.OBJECT records, or a Scene)."""
        scene = objects if isinstance(objects, R.Scene) else None
        records = np.ascontiguousarray(scene.objects if scene is not None else objects, dtype=R.OBJECT)
        self._check(L.lib.chordvis_group_set_object_list(self._g, records.ctypes.data if len(records) else None, len(records)), "group_set_object_list")
        if scene is not None:
            self.scene = scene
            for r in self.ranks:
                r.scene = scene

    def upload_world_transforms(self, local_to_world, prev_local_to_world=None):
        """chordvis_group_upload_world_transforms: every rank keeps the f64 world matrices (see VisibilityRenderer)."""
        cur = np.ascontiguousarray(local_to_world, dtype=np.float64).reshape(-1, 16)
        prev = None if prev_local_to_world is None else np.ascontiguousarray(prev_local_to_world, dtype=np.float64).reshape(-1, 16)
        assert prev is None or prev.shape == cur.shape
        self._check(L.lib.chordvis_group_upload_world_transforms(self._g, cur.ctypes.data, prev.ctypes.data if prev is not None else None, len(cur)),
                    "group_upload_world_transforms")

    def build_objects(self, camera_pos, camera_pos_last=None):
        """chordvis_group_build_objects: chordvis_build_objects on every rank."""
        cam = (C.c_double * 3)(*[float(v) for v in camera_pos])
        last = None if camera_pos_last is None else (C.c_double * 3)(*[float(v) for v in camera_pos_last])
        self._check(L.lib.chordvis_group_build_objects(self._g, cam, last), "group_build_objects")

    def set_view(self, view, instance_view, flags):
        self._views = (view, instance_view)
        self._check(L.lib.chordvis_group_set_view(self._g, view.ctypes.data, instance_view.ctypes.data, flags), "group_set_view")

    def render_frame(self):
        self._check(L.lib.chordvis_group_render_frame(self._g), "group_render_frame")

    def sync(self):
        self._check(L.lib.chordvis_group_sync(self._g), "group_sync")

    def enqueue_ms(self):
        """Mean host time per frame of every rank's worker inside render_frame since the last call."""
        out = (C.c_double * self.size)()
        self._check(L.lib.chordvis_group_enqueue_ms(self._g, out, self.size), "group_enqueue_ms")
        return [float(v) for v in out]

    def set_pipelined(self, enable=True):
        """The visibility all-gather of frame i travels beside frame i + 1 (chordvis_group_set_pipelined)."""
        self._check(L.lib.chordvis_group_set_pipelined(self._g, 1 if enable else 0), "group_set_pipelined")
