"""The host-only unit of temporal accumulation (rt_amd/csrc/temporal.cpp) through the CPU restatement's library, which
compiles it in unchanged: forward_view_projection against numpy's inverse, what it refuses, every parameter refusal by its field's
name, and same_history's table.  No GPU."""
import numpy as np
import pytest

from tests import reproject_reference as ref
from tests import temporal_cases as cases

F32 = np.float32
W, H = 96, 54
INVALID_ARGUMENT = 1

CAMERA_FORMS = {
    "pinhole": lambda: cases.toml_scene("basic", W, H),
    "eye": lambda: cases.toml_scene("basic", W, H, *cases.TILTED),
    "orthographic": lambda: cases.orthographic(W, H),
}
# The inverse is rounded ONCE from binary64 to float.  Measured against numpy.linalg.inv in binary64, in units of the last place of the
# inverse's largest element: 0.27 (pinhole), 0.50 (eye), 0.11 (orthographic) — the rounding itself; the two binary64 inversions differ
# far below that.  The bound is one rounding plus as much again.
FORWARD_ULPS = 1.0


@pytest.mark.parametrize("form", list(CAMERA_FORMS))
def test_forward_view_projection_is_numpys_float64_inverse_rounded_once(form):
    inverse = ref.matrix_of(CAMERA_FORMS[form]())
    status, forward, _ = ref.forward(inverse)
    assert status == 0
    want = np.linalg.inv(inverse.astype(np.float64).reshape(4, 4))
    ulp = float(np.spacing(F32(np.abs(want).max())))
    deviation = float(np.abs(forward.astype(np.float64) - want).max()) / ulp
    print(f"{form}: largest deviation {deviation:.3f} ulps of the largest element ({np.abs(want).max():.4g})")
    assert deviation <= FORWARD_ULPS


def test_a_singular_and_a_non_finite_matrix_are_refused_with_a_message():
    singular = np.eye(4, dtype=F32)
    singular[2] = singular[1]
    status, forward, message = ref.forward(singular)
    assert status == INVALID_ARGUMENT and forward is None and "singular" in message
    status, _, message = ref.forward(np.zeros((4, 4), dtype=F32))
    assert status == INVALID_ARGUMENT and "singular" in message
    for poison in (np.nan, np.inf):
        broken = np.eye(4, dtype=F32)
        broken[1, 3] = poison
        status, forward, message = ref.forward(broken)
        assert status == INVALID_ARGUMENT and forward is None and "[1][3]" in message and "finite" in message
    # a matrix that needs its rows exchanged is not singular
    status, forward, _ = ref.forward(np.array([[0, 0, 0, 1], [0, 0, 2, 0], [0, 4, 0, 0], [8, 0, 0, 0]], dtype=F32))
    assert status == 0 and np.array_equal(forward, np.array([[0, 0, 0, 0.125], [0, 0, 0.25, 0], [0, 0.5, 0, 0], [1, 0, 0, 0]], dtype=F32))


def test_the_defaults_pass_the_check():
    p = ref.params()
    assert ref.check(p) == (0, "")
    assert 1 <= p.max_history_samples <= 2**20 and p.position_tolerance > 0 and -1 <= p.normal_threshold <= 1


BAD = [("max_history_samples", 0), ("max_history_samples", 2**20 + 1), ("max_history_samples", 2**32 - 1), ("position_tolerance", 0.0), ("position_tolerance", -0.0), ("position_tolerance", -1.0),
       ("position_tolerance", float("nan")), ("position_tolerance", float("inf")), ("normal_threshold", 1.5), ("normal_threshold", -1.0001), ("normal_threshold", float("nan")), ("normal_threshold", float("inf"))]


@pytest.mark.parametrize("field,value", BAD)
def test_every_out_of_range_parameter_is_refused_with_its_fields_name(field, value):
    status, message = ref.check(ref.params(**{field: value}))
    assert status == INVALID_ARGUMENT and field in message
    assert not any(other in message for other in ("max_history_samples", "position_tolerance", "normal_threshold") if other != field)


@pytest.mark.parametrize("fields", [{"max_history_samples": 1}, {"max_history_samples": 2**20}, {"position_tolerance": 1e-30}, {"position_tolerance": 1e30}, {"normal_threshold": -1.0}, {"normal_threshold": 1.0}])
def test_every_value_at_the_edge_of_its_range_passes(fields):
    assert ref.check(ref.params(**fields))[0] == 0


# ---- same_history: one case per field ---------------------------------------------------------------------------------------------
SM_MATERIALS, BVH, BVH_DEVICE_BUILD, STATS, TRACE_BOXES = 1 << 3, 1 << 10, 1 << 11, 1 << 7, 1 << 13
KEY = {"scene_fingerprint": 0x1234_5678_9ABC_DEF0, "samples_per_pixel": 16, "max_bounces": 6, "matrix": np.eye(4, dtype=F32), "width": 96, "height": 54, "seed": 7, "flags": 0}
RESTARTS = [("scene_fingerprint", 0x1234_5678_9ABC_DEF1), ("scene_fingerprint", 0x0234_5678_9ABC_DEF0), ("max_bounces", 7), ("width", 97), ("height", 53), ("flags", SM_MATERIALS), ("flags", TRACE_BOXES)]
CARRIES_ON = [("matrix", np.diag([1, 2, 3, 4]).astype(F32)), ("seed", 8), ("seed", 2**63), ("samples_per_pixel", 64), ("flags", BVH), ("flags", BVH | BVH_DEVICE_BUILD), ("flags", STATS)]


def test_equal_keys_are_one_history():
    assert ref.same_history(KEY, dict(KEY))


@pytest.mark.parametrize("field,value", RESTARTS, ids=[f"{f}-{i}" for i, (f, _) in enumerate(RESTARTS)])
def test_the_history_starts_again_on_a_change_of(field, value):
    assert not ref.same_history(KEY, dict(KEY, **{field: value}))
    assert not ref.same_history(dict(KEY, **{field: value}), KEY)


@pytest.mark.parametrize("field,value", CARRIES_ON, ids=[f"{f}-{i}" for i, (f, _) in enumerate(CARRIES_ON)])
def test_the_history_is_carried_across_a_change_of(field, value):
    assert ref.same_history(KEY, dict(KEY, **{field: value}))
