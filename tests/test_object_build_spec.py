"""The numpy spec of the object build (tests/spec_object_build_np.py) against the host function chordvis_object_basic_data, byte for
byte, on the input set the GPU tests reuse -- and the conditions that keep that set from being vacuous.  No device calls."""
import numpy as np

import spec_object_build_np as SOB
from chord_amd import records as R, scenes


def test_spec_equals_the_host_function_on_the_input_set(built_lib):
    cases = SOB.input_set()
    assert len(cases) == len(SOB.ORIGINS)
    for case in cases:
        want, want_singular = SOB.host_records(case["cur"], case["prev"], case["cam"], case["cam_last"])
        got, singular = SOB.basic_data(case["cur"], case["prev"], case["cam"], case["cam_last"])
        assert np.array_equal(singular, want_singular), case["name"]
        assert np.flatnonzero(singular).tolist() == case["singular"], case["name"]
        got = got.view(np.uint8).reshape(len(want), SOB.BASIC_BYTES)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert len(bad) == 0, "%s: objects %s differ from chordvis_object_basic_data" % (case["name"], bad[:8])


def test_spec_defaults_are_the_host_functions(built_lib):
    """prev NULL = cur, cameraPosLast NULL = cameraPos"""
    case = SOB.input_set()[1]
    want, _ = SOB.host_records(case["cur"], None, case["cam"], None)
    got, _ = SOB.basic_data(case["cur"], None, case["cam"], None)
    assert np.array_equal(got.view(np.uint8).reshape(want.shape), want)


def test_host_function_leaves_a_singular_objects_matrices_filled(built_lib):
    """The yardstick of the build is the single call, object by object (the batch form returns at the first singular matrix): for a
    matrix with det == 0 it reports an error and leaves the two matrices filled, the inverse and the scale zero"""
    case = SOB.input_set()[0]
    want, singular = SOB.host_records(case["cur"], case["prev"], case["cam"], case["cam_last"])
    s = case["singular"][0]
    rec = want[s].view(np.float32)
    assert singular[s] and not rec[16:32].any() and not rec[48:52].any() and rec[0:16].any() and rec[32:48].any()


def test_the_input_set_exercises_what_it_names(built_lib):
    cases = SOB.input_set()
    classes = set(cases[0]["classes"].tolist())
    assert {scenes.TILTED, scenes.STRETCHED, scenes.MIRRORED} <= classes
    f32 = np.float32
    for case in cases:
        assert not np.array_equal(case["cur"], case["prev"]) and not np.array_equal(case["cam"], case["cam_last"])
        assert np.abs(case["cur"][:, 12:15] - case["cam"]).max() < 64.0, "the camera stays within a few units of the objects"
        assert np.isfinite(case["cur"]).all() and np.isfinite(case["prev"]).all()
    # the binary64 subtraction is really exercised: rounding first and subtracting in binary32 gives other bits
    far = cases[-1]
    early = far["cur"][:, 12:15].astype(f32) - far["cam"].astype(f32)
    late = (far["cur"][:, 12:15] - far["cam"]).astype(f32)
    assert (early != late).any(axis=1).any()
    # the small scales: cofactor products that are tiny normals (2^-40) and subnormals (2^-45), none flushed to zero
    rec, _ = SOB.basic_data(far["cur"], far["prev"], far["cam"], far["cam_last"])
    n = len(far["cur"])
    tiny = f32(np.finfo(np.float32).tiny)
    for k, s in ((n - 4, 2.0 ** -40), (n - 3, 2.0 ** -45), (n - 2, 2.0 ** 20)):
        L = rec[k, 0:16]
        assert np.isclose(float(rec[k, 51]), s, rtol=1e-6), (k, rec[k, 48:52])
        minor = np.abs(L[0] * L[5] * L[10])                # one cofactor product of inv[15]
        if s == 2.0 ** -40:
            assert 0 < minor < f32(2.0 ** -100) and minor >= tiny
        if s == 2.0 ** -45:
            assert 0 < minor < tiny                        # a subnormal: kept
            assert not np.isfinite(rec[k, 16:32]).all()    # its determinant's reciprocal overflows: the host function's own result
    assert R.OBJECT.itemsize == 224 and SOB.BASIC_BYTES == 208
