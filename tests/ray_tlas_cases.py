"""Lists for the TLAS rebuild's tests (tests/test_ray_tlas_spec.py, tests/test_ray_tlas_host.py, tests/test_gpu_ray_tlas.py): boxes
for the CPU side, object lists of one primitive for the GPU side."""
import numpy as np

from chord_amd import lib as L, records as R, scenes

F = np.float32


# ---- boxes ------------------------------------------------------------------------------------------------------------------------

def random_boxes(n, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-40.0, 40.0, (n, 3))
    e = rng.uniform(0.05, 3.0, (n, 3))
    return (c - e).astype(F), (c + e).astype(F)


def equal_centre_boxes(n):
    """Boxes of growing size about one centre: lo = -e, hi = +e exactly, so every centre is +0."""
    e = (0.5 + np.arange(n)[:, None] * 0.25) * np.ones((1, 3))
    return (-e).astype(F), e.astype(F)


def plane_boxes(n, axis):
    lo, hi = random_boxes(n, 100 + n)
    lo[:, axis], hi[:, axis] = -1.5, 2.5
    return lo, hi


def signed_zero_boxes():
    """Centres whose x is -0 or +0: lo.x * 0.5 + hi.x * 0.5 with (lo, hi) = (-e, e) is +0, with (-0, -0) it is -0."""
    lo, hi = random_boxes(12, 3)
    lo[:, 0], hi[:, 0] = -2.0, 2.0
    lo[::3, 0], hi[::3, 0] = -0.0, -0.0
    return lo, hi


# ---- object lists -----------------------------------------------------------------------------------------------------------------

def _with_matrices(scene, cam, mats):
    out = scene.with_objects(np.zeros(len(mats), dtype=R.OBJECT))
    out.local_to_world = np.ascontiguousarray(np.stack([m.T.reshape(16) for m in mats]), dtype=np.float64)
    L.fill_objects(out, cam)
    return out


def instances(scene, cam, n, seed):
    """n instances of the scene's first primitive on a jittered grid, records filled (the placement of tests/test_gpu_rays.py)."""
    side = int(np.ceil(np.sqrt(n)))
    rnd = scenes.rand01(seed, np.arange(3 * n)).reshape(n, 3)
    return _with_matrices(scene, cam, [
        scenes.translate(2.5 * (k % side) - 1.25 * side + rnd[k, 0], 2.5 * (k // side) - 1.25 * side + rnd[k, 1], -3.0 * rnd[k, 2]) @
        scenes.rotate_y(rnd[k, 0] * 2.0) for k in range(n)])


def equal_instances(scene, cam, n):
    """n instances under ONE matrix: every centre equal, every key ties."""
    return _with_matrices(scene, cam, [scenes.translate(0.25, -0.5, -2.0)] * n)


def plane_instances(scene, cam, n, seed):
    """n unrotated instances at one depth: the z of every centre is the same value."""
    side = int(np.ceil(np.sqrt(n)))
    rnd = scenes.rand01(seed, np.arange(2 * n)).reshape(n, 2)
    return _with_matrices(scene, cam, [scenes.translate(2.5 * (k % side) - 1.25 * side + rnd[k, 0], 2.5 * (k // side) - 1.25 * side + rnd[k, 1], -2.0)
                                       for k in range(n)])


def permuted(scene, cam):
    """The same list with the places permuted among the objects: object k takes the matrix of object (7 k + n / 2 + 1) mod n (a
    rotation by n / 2 + 1 where 7 divides n), so neighbours in index are no longer neighbours in space and the old topology is
    wrong everywhere."""
    n = len(scene.objects)
    perm = (np.arange(n) * 7 + n // 2 + 1) % n if n % 7 else np.roll(np.arange(n), n // 2 + 1)
    assert sorted(perm.tolist()) == list(range(n))
    out = scene.with_objects(scene.objects.copy())
    out.local_to_world = np.ascontiguousarray(scene.local_to_world[perm])
    L.fill_objects(out, cam)
    return out
