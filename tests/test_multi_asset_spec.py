"""tests/multi_asset.py on the CPU: the one-asset twin is the same scene as its assets, the two meshlet numberings convert into each
other, the inputs of tests/test_gpu_multi_asset.py are not empty, and its comparisons can fail -- the expected shade records and the
meshlet debug colours change when a hit's or a command's asset-relative meshlet is taken for a concatenated index, which is the mistake
those tests exist to catch.  No device."""
import functools

import numpy as np

import helpers as H
import multi_asset as MA
import orc
import spec_ray_shade_np as RS
import spec_rays_np as S
import spec_resolve_np as SR
from chord_amd import records as R

u32 = np.uint32


@functools.lru_cache(maxsize=None)
def _case():
    """(scene, camera, view, iv, the oracle's frame on the twin, rays, their origin asset, expected hits) -- computed once, read-only."""
    ms, cam = MA.three_assets()
    view, iv = MA.filled(ms, cam)
    frame = orc.frame(ms.spec, view, iv, H.ALL_FLAGS)
    rays, origin = MA.ray_set(ms)
    hits = S.trace(ms.spec, ms.objects, rays, meshlet_cull=True, asset_meshlet_base=ms.asset_meshlet_base)
    for a in (rays, origin, hits, frame["vis"], frame["cmds"]):
        a.setflags(write=False)
    return ms, cam, view, iv, frame, rays, origin, hits


def _owners(ms, vis, cmds):
    """(covered (n,) bool, per pixel the command's slot, the asset of its object or -1)"""
    low = (np.asarray(vis, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    covered = low != 0
    slot = np.where(covered, ((low >> 8) & 0xFFFFFF) - 1, 0)
    return covered, slot, np.where(covered, ms.asset_of_object[cmds["objectId"][slot]], -1)


def test_bases_and_interleaving():
    ms = _case()[0]
    MA.check_bases(ms)
    prim = ms.objects["GLTFPrimitiveDetail"].astype(np.int64)
    assert np.array_equal(ms.asset_of_primitive[prim], ms.asset_of_object), "an object's primitive is of the object's asset"
    assert np.array_equal(ms.asset_of_material[ms.objects["GLTFMaterialData"].astype(np.int64)], ms.asset_of_object)
    assert np.array_equal(ms.primitives["primitiveDatasBufferId"], ms.asset_of_primitive) and not ms.spec.primitives["primitiveDatasBufferId"].any()
    # every material of asset 2 that names a texture names one of asset 2's: the ids are shifted
    m2 = ms.materials[ms.asset_of_material == 2]
    ids = np.concatenate([m2[f] for f, _ in MA._TEX_FIELDS])
    ids = ids[ids != MA.NONE]
    assert len(ids) > 8 and ids.min() >= ms.texture_base[2] > 0 and ids.max() < len(ms.texture_images)
    # asset 1 names its texture and has no texture coordinates: the twin holds zeros there and asset 0's planar ones before them
    v0, v1 = ms.sizes[0]["vertices"], ms.sizes[1]["vertices"]
    assert ms.spec.texcoord0[:v0].any() and not ms.spec.texcoord0[v0:v0 + v1].any() and ms.spec.texcoord0[v0 + v1:].any()
    assert ms.spec.normals[:v0].any() and not ms.spec.normals[v0:v0 + v1].any() and not ms.spec.tangents[v0:v0 + v1].any()
    assert (ms.materials["baseColorId"][ms.asset_of_material == 1] == ms.texture_base[1]).any()
    two, _ = MA.two_assets_one_without_bvh()
    assert two.spec.bvh_nodes is None and two.assets[0].bvh_nodes is not None and two.desc.assetCount == 2


def test_every_asset_alone_owns_the_twins_pixels():
    """Pixel for pixel: where asset a is the nearest surface of the twin's frame, the frame of asset a alone -- its own arrays, its own
    numbering, one asset -- has the same depth and the same (object, meshlet, triangle), the meshlet asset-relative."""
    ms, cam, view, iv, frame, *_ = _case()
    covered, slot, owner = _owners(ms, frame["vis"], frame["cmds"])
    rel = ms.to_asset_relative(frame["cmds"])
    for a in range(3):
        alone = orc.frame(ms.alone(a), view, iv, H.ALL_FLAGS)
        mine = owner == a
        assert mine.sum() > 0
        acov, aslot, _ = _owners(ms, alone["vis"], np.zeros(len(alone["cmds"]), dtype=R.DRAW_CMD))
        assert acov[mine].all(), "asset %d: %d of its pixels in the twin's frame are empty in its own" % (a, (~acov[mine]).sum())
        assert np.array_equal(alone["vis"][mine] >> np.uint64(32), frame["vis"][mine] >> np.uint64(32)), "asset %d: depth" % a
        assert np.array_equal(alone["vis"][mine] & np.uint64(0xFF), frame["vis"][mine] & np.uint64(0xFF)), "asset %d: triangle" % a
        tw, al = rel[slot[mine]], alone["cmds"][aslot[mine]]
        assert np.array_equal(ms.index_in_asset_of_object[tw["objectId"]], al["objectId"]), "asset %d: object" % a
        assert np.array_equal(tw["meshletId"], al["meshletId"]), "asset %d: the asset-relative meshlet" % a
        if a:
            assert (frame["cmds"]["meshletId"][slot[mine]] != al["meshletId"]).all(), "asset %d: the concatenated id is another number" % a


def test_the_numberings_convert_into_each_other():
    ms, cam, view, iv, frame, rays, origin, hits = _case()
    cmds = frame["cmds"]
    rel = ms.to_asset_relative(cmds)
    assert np.array_equal(ms.to_concatenated(rel), cmds) and np.array_equal(ms.to_asset_relative(ms.to_concatenated(rel)), rel)
    own = ms.asset_of_object[cmds["objectId"]]
    assert np.array_equal(rel["meshletId"][own == 0], cmds["meshletId"][own == 0]) and (rel["meshletId"][own > 0] < cmds["meshletId"][own > 0]).all()
    for a in range(3):
        assert (own == a).sum() > 20 and rel["meshletId"][own == a].max() < ms.sizes[a]["meshlets"]
    assert np.array_equal(rel["objectId"], cmds["objectId"]) and np.array_equal(rel["slot"], cmds["slot"])
    # hits: a miss and a record that names no object stay as they are
    cat = ms.to_concatenated(hits)
    assert np.array_equal(ms.to_asset_relative(cat), hits)
    miss = (hits["status"] & 1) == 0
    assert cat[miss].tobytes() == hits[miss].tobytes()
    odd = hits[~miss][:4].copy()
    odd["object"] = [len(ms.objects), 0xFFFFFFFF, len(ms.objects) + 7, 0xFFFFFFFE]
    assert ms.to_concatenated(odd).tobytes() == odd.tobytes() and ms.to_asset_relative(odd).tobytes() == odd.tobytes()
    bad = np.zeros(2, dtype=R.DRAW_CMD)
    bad["objectId"], bad["meshletId"] = [len(ms.objects), 0xFFFFFFFF], [5, 6]
    assert ms.to_asset_relative(bad).tobytes() == bad.tobytes()


def test_input_conditions():
    """What tests/test_gpu_multi_asset.py needs of its inputs, from the oracle and the specification alone."""
    ms, cam, view, iv, frame, rays, origin, hits = _case()
    assert (cam.width, cam.height) == (MA.FW, MA.FH) and len(rays) == MA.PW * MA.PH + 300
    covered, slot, owner = _owners(ms, frame["vis"], frame["cmds"])
    for a in range(3):
        share = (owner == a).sum() / covered.sum()
        print("asset %d owns %.1f %% of %d covered pixels" % (a, 100.0 * share, covered.sum()))
        assert share >= 0.05, (a, share)
    hit = (hits["status"] & 1) != 0
    on = np.where(hit, ms.asset_of_object[np.where(hit, hits["object"], 0)], -1)
    for a in range(3):
        n_hit, n_miss = int((on == a).sum()), int((~hit & (origin == a)).sum())
        print("asset %d: %d closest hits, %d misses among the 100 rays from its box" % (a, n_hit, n_miss))
        assert n_hit >= 50 and n_miss >= 30, (a, n_hit, n_miss)
        assert hits["meshlet"][on == a].max() < ms.sizes[a]["meshlets"]
        assert (ms.spec.meshlets["lod"][hits["meshlet"][on == a] + ms.bases[a]["meshlets"]] == 0).all(), "a hit names a LOD-0 meshlet of its own asset"
    assert (hits["status"] == 3).any() and (~hit & (origin < 0)).sum() >= 30


def test_shade_records_tell_the_numberings_apart():
    """Sensitivity: the expected records of the traced hits with the hit's meshlet read at base + meshlet, and with it taken for a
    concatenated index (what chordvis_shade_ray_hits did before it knew the asset), differ on objects of assets 1 and 2."""
    ms, cam, view, iv, frame, rays, origin, hits = _case()
    right = RS.shade(ms.spec, ms.objects, hits, lod=1.0, asset_meshlet_base=ms.asset_meshlet_base, asset_meshlet_count=ms.asset_meshlet_count)
    wrong = RS.shade(ms.spec, ms.objects, hits, lod=1.0)
    hit = (hits["status"] & 1) != 0
    assert ((right["flags"] & RS.RAYSURF_VALID) != 0).sum() == hit.sum(), "every traced hit is a valid hit"
    differ = (right.view(u32).reshape(-1, 16) != wrong.view(u32).reshape(-1, 16)).any(axis=1)
    on = np.where(hit, ms.asset_of_object[np.where(hit, hits["object"], 0)], -1)
    print("records that differ per asset:", [int((differ & (on == a)).sum()) for a in range(3)])
    assert not differ[on == 0].any() and not differ[~hit].any()
    assert (differ & (on > 0)).sum() >= 50
    # the edges of the numbering
    for what, h, valid in ms.edge_hits():
        rec = RS.shade(ms.spec, ms.objects, h, lod=0.0, asset_meshlet_base=ms.asset_meshlet_base, asset_meshlet_count=ms.asset_meshlet_count)
        assert bool(rec["flags"][0] & RS.RAYSURF_VALID) == valid, what
        assert valid or not rec.view(u32).any(), what
    what, h, _ = ms.edge_hits()[1]
    assert RS.shade(ms.spec, ms.objects, h)["flags"][0] & RS.RAYSURF_VALID, "as a concatenated index the same id is valid"


def test_meshlet_debug_colours_tell_the_numberings_apart():
    ms, cam, view, iv, frame, *_ = _case()
    covered, slot, owner = _owners(ms, frame["vis"], frame["cmds"])
    for mode in (0, 3):
        kw = dict(names=("debugRGBA8",), debug_mode=mode)
        right = SR.resolve(ms.spec, frame["vis"], frame["cmds"], view, iv, MA.FW, MA.FH, asset_meshlet_base=ms.asset_meshlet_base, **kw)["debugRGBA8"]
        wrong = SR.resolve(ms.spec, frame["vis"], frame["cmds"], view, iv, MA.FW, MA.FH, **kw)["debugRGBA8"]
        differ = (right != wrong).reshape(-1)
        assert not differ[owner <= 0].any()
        assert differ.sum() >= 0.05 * covered.sum(), (mode, differ.sum(), covered.sum())
