"""scenes.stacked_layers holds to its purpose under the oracle (no GPU): the scenes that put one binner of the set-up kernels
past the fixed part of a tile's bin (tests/test_gpu_bin_limits.py) -- few enough clusters for a light later pass's wide
kernel, every triangle of the large variant a large record through the centre tile and none clipped, every triangle of the
near-plane variant clipped."""
import numpy as np
import pytest

import helpers as H
import orc
from chord_amd import records as R
from chord_amd import scenes

ONE_PASS = R.FLAG_FRUSTUM_CULL | R.FLAG_CONE_CULL
BIN_FIXED, CHUNK = 16384, 1024


@pytest.fixture(scope="module")
def layers(built_lib):
    out = {}
    for v in ("large", "near"):
        scene, cam, view, iv = H.setup_scene(scenes.stacked_layers, v)
        out[v] = (scene, cam, orc.frame_mt(scene, view, iv, ONE_PASS, None, 8))
    return out


def _screen(scene, cam):
    """Screen positions (pixels, y down) and view depth of every vertex of the layer objects (camera at the origin, -z)."""
    th, aspect = np.tan(0.5 * cam.fovy), cam.width / cam.height
    p = scene.positions.astype(np.float64)
    zv = -p[:, 2]
    sx = (p[:, 0] / (zv * th * aspect) + 1.0) * 0.5 * cam.width
    sy = (1.0 - p[:, 1] / (zv * th)) * 0.5 * cam.height
    return sx, sy, zv


def test_large_layers_are_large_records_through_one_tile_and_never_clipped(layers):
    scene, cam, o = layers["large"]
    st = o["stats"]
    n_layer_clusters = len(scene.meshlets) - 1                          # (the backdrop is one cluster)
    assert len(scene.meshlets) <= 1024                                  # a light later pass of all of them takes the wide kernel
    assert st.clusters == len(scene.meshlets) and st.trianglesClipped == 0 and st.trianglesNear == 0
    assert st.trianglesBackface == st.trianglesOffscreen == st.trianglesSmall == 0
    # the centre tile's bin gets every layer triangle: past the fixed part by more than two pool chunks
    assert 128 * n_layer_clusters > BIN_FIXED + 2 * CHUNK
    sx, sy, zv = _screen(scene, cam)
    tri = scenes._TI
    for m in range(n_layer_clusters):
        base = m * 81
        X, Y = sx[base + tri], sy[base + tri]                           # (128, 3)
        # bbox over far more than 2 x 2 tiles, depth one per layer, in front of the camera
        assert ((X.max(1) - X.min(1)) > 3 * 64).all() or ((Y.max(1) - Y.min(1)) > 3 * 64).all()
        assert np.ptp(zv[base: base + 81]) < 1e-3 and zv[base] > 1.0
        # every triangle has the screen centre (in tile (2, 1)) on one of its edges
        c = np.array([cam.width / 2.0, cam.height / 2.0])
        P = np.stack([X, Y], -1)
        d = []
        for a, b in ((0, 1), (1, 2), (2, 0)):
            e = P[:, b] - P[:, a]
            t = np.clip(((c - P[:, a]) * e).sum(1) / (e * e).sum(1), 0, 1)
            d.append(np.linalg.norm(P[:, a] + t[:, None] * e - c, axis=1))
        assert (np.min(d, axis=0) < 0.5).all(), m
    assert len(np.unique(np.round(zv[: n_layer_clusters * 81: 81], 4))) == n_layer_clusters


def test_near_layers_are_clipped_at_the_near_plane(layers):
    scene, cam, o = layers["near"]
    st = o["stats"]
    assert len(scene.meshlets) <= 1024
    # every triangle straddles the camera plane: all of them go through the clipper, and the binned pieces are theirs
    assert st.trianglesSubmitted == 128 * len(scene.meshlets) and st.trianglesClipped == st.trianglesSubmitted
    assert st.trianglesRastered >= st.trianglesClipped
    assert 128 * len(scene.meshlets) > BIN_FIXED + 2 * CHUNK
    vis = np.asarray(o["vis"], np.uint64).reshape(cam.height, cam.width)
    assert (vis[-64:] != 0).mean() > 0.9                                # the bottom tile row is covered


def test_frame_mt_is_the_frame_for_the_layers(layers, built_lib):
    """(the GPU tests compare with orc.frame_mt, the oracle's threaded form, for speed)"""
    for v in ("large", "near"):
        scene, cam, view, iv = H.setup_scene(scenes.stacked_layers, v)
        a = orc.frame(scene, view, iv, ONE_PASS)
        b = layers[v][2]
        assert np.array_equal(a["vis"], b["vis"]) and a["stats"].as_dict() == b["stats"].as_dict(), v
