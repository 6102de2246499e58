"""The thin lens' host-only unit (rt_amd/csrc/lens.cpp) on the CPU, through the restatement's library, which links it as it
is: the ten lens words against a numpy binary64 derivation from the same matrix (1e-6 relative: they are rounded once from binary64),
against the axes rt's camera was built from (loosely: the float inverse matrix carries the noise §3.4 describes), every refusal with its
field's or the flag's name, and the parser's accepted and refused texts.

Measured (`python -m tests.test_lens_host` prints them): the words deviate from the numpy derivation by at most 4.6e-8 relative (one
rounding to binary32); from rt's own axes — forward = the camera's direction, right = forward x world-up, up = right x forward — by
0 per component through the axis-aligned camera and by 5.8e-6 through the tilted one, the eye by 2.4e-7 and 4.8e-7.  The loose bound
is 1e-4: rt's matrix is the binary32 inverse of projection x view, whose condition number is near / far-scale, about 1e3 here, so
its entries carry about 1e3 x 2^-24 = 6e-5 of relative noise (DESIGN.md §3.4 reports 4.5e-4 in the w row of such a matrix)."""
import ctypes as C

import numpy as np
import pytest

import rt_amd
from rt_amd import capi
from tests import lens_reference as lens_ref

INVALID_ARGUMENT, UNSUPPORTED = 1, 5
LENS = (0.125, 4.2)
ORTHOGRAPHIC = [2.4, 0, 0, 0.0, 0, 1.35, 0, 1.0, 0, 0, -12.0, 3.0, 0, 0, 0, 1.0]  # (tests/test_gpu_parity.py: no finite eye)


def numpy_words(pod, width, height, lens, eye):
    """the contract's text in binary64: near-plane points of the frame's centre and its right and lower neighbours"""
    m = np.array(pod.inverse_view_projection[:], dtype=np.float32).astype(np.float64).reshape(4, 4)

    def near(px, py):
        p = m @ np.array([2.0 / width * px - 1.0, -(2.0 / height) * py + 1.0, 0.0, 1.0])
        return p[:3] / p[3]

    centre = near(width / 2, height / 2)
    right = near(width / 2 + 1, height / 2) - centre
    up = -(near(width / 2, height / 2 + 1) - centre)
    right, up = right / np.linalg.norm(right), up / np.linalg.norm(up)
    fwd = np.cross(right, up)
    fwd = fwd / np.linalg.norm(fwd)
    if not fwd @ (centre - eye.astype(np.float64)) > 0:
        fwd = -fwd
    return np.concatenate([lens[0] * right, lens[0] * up, fwd, [lens[1]]])


def frames():
    axis = lens_ref.named_scene("basic", lens_ref.AXIS_CAMERA)
    tilted = lens_ref.named_scene("basic", lens_ref.TILTED_CAMERA)
    return {"axis-aligned": (axis.describe(96, 54), 96, 54, lens_ref.AXIS_CAMERA, 1), "tilted": (tilted.describe(96, 54), 96, 54, lens_ref.TILTED_CAMERA, 2), "one pixel": (tilted.describe(1, 1), 1, 1, lens_ref.TILTED_CAMERA, 2)}


def relative(got, want):
    """per word, relative to the vector it belongs to (a component that is zero in binary64 may be 1e-9 in the other)"""
    scale = np.concatenate([np.full(3, np.linalg.norm(want[0:3])), np.full(3, np.linalg.norm(want[3:6])), np.ones(3), [abs(want[9])]])
    return float((np.abs(got.astype(np.float64) - want) / scale).max())


def test_the_words_are_the_binary64_derivations():
    for name, (pod, width, height, _, form) in frames().items():
        status, words, eye, got_form = lens_ref.words(pod, width, height, LENS)
        assert status == 0 and got_form == form, name
        assert relative(words, numpy_words(pod, width, height, LENS, eye)) <= 1e-6, name
        assert words[9] == np.float32(LENS[1])
        assert abs(np.linalg.norm(words[6:9].astype(np.float64)) - 1.0) <= 1e-6 and abs(np.linalg.norm(words[0:3].astype(np.float64)) - LENS[0]) <= 1e-6 * LENS[0]


def camera_axes(position, direction):
    forward = np.array(direction, dtype=np.float64)
    forward /= np.linalg.norm(forward)
    right = np.cross(forward, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    return right, np.cross(right, forward), forward


def axes_deviation():
    worst = {}
    for name, (pod, width, height, camera, _) in frames().items():
        _, words, eye, _ = lens_ref.words(pod, width, height, LENS)
        right, up, forward = camera_axes(*camera)
        got = np.concatenate([words[0:3] / LENS[0], words[3:6] / LENS[0], words[6:9]]).astype(np.float64)
        worst[name] = float(np.abs(got - np.concatenate([right, up, forward])).max())
        worst[name + " eye"] = float(np.abs(eye - np.array(camera[0])).max())
    return worst


def test_the_words_are_rts_camera_axes_loosely():
    for name, deviation in axes_deviation().items():
        assert deviation <= 1e-4, (name, deviation)


def test_a_matrix_without_an_eye_is_refused_by_the_flags_name():
    pod = lens_ref.named_scene("basic").describe(96, 54)
    pod.inverse_view_projection = (C.c_float * 16)(*ORTHOGRAPHIC)
    status, message = lens_ref.check_frame(pod, 96, 54, True)
    assert status == UNSUPPORTED and message.startswith("rt_hip_render_device: RT_HIP_FLAG_THIN_LENS ") and "perspective matrix" in message
    assert lens_ref.words(pod, 96, 54, LENS)[0] == UNSUPPORTED
    status, message = lens_ref.check_frame(pod, 96, 54, False)  # (the missing lens is said first)
    assert status == INVALID_ARGUMENT and "rt_hip_set_lens" in message
    fine = lens_ref.named_scene("basic").describe(96, 54)
    assert lens_ref.check_frame(fine, 96, 54, True) == (0, "")
    status, message = lens_ref.check_frame(fine, 96, 54, False)
    assert status == INVALID_ARGUMENT and message == "rt_hip_render_device: RT_HIP_FLAG_THIN_LENS without a lens (rt_hip_set_lens)"


@pytest.mark.parametrize("aperture,focus,field", [(-1.0, 1.0, "aperture_radius"), (float("nan"), 1.0, "aperture_radius"), (float("inf"), 1.0, "aperture_radius"), (-1e-30, 1.0, "aperture_radius"), (0.1, 0.0, "focus_distance"),
                                                  (0.1, -0.0, "focus_distance"), (0.1, -2.0, "focus_distance"), (0.1, float("nan"), "focus_distance"), (0.1, float("inf"), "focus_distance"), (float("nan"), float("nan"), "aperture_radius")])
def test_a_bad_lens_is_refused_by_the_fields_name(aperture, focus, field):
    status, message = lens_ref.check_lens(aperture, focus)
    assert status == INVALID_ARGUMENT and message.startswith(f"rt_hip_set_lens: {field} = "), message


@pytest.mark.parametrize("aperture,focus", [(0.0, 1.0), (-0.0, 1e-30), (0.05, 4.2), (1000.0, 1e-3), (3.0e38, 3.0e38)])
def test_a_good_lens_passes(aperture, focus):
    assert lens_ref.check_lens(aperture, focus) == (0, "")


ACCEPTED = {
    "aperture=0.05,focus=4.2": (0.05, 4.2),
    "focus=4.2,aperture=0.05": (0.05, 4.2),
    "  aperture = 0.05 ,\tfocus= 4.2 ": (0.05, 4.2),
    "aperture=0,focus=1e-3": (0.0, 1e-3),
    "aperture=1e3,focus=0x1p2": (1000.0, 4.0),
    "aperture=-0,focus=1": (-0.0, 1.0),
}
REFUSED = {
    "": "an empty item",
    "aperture=0.05": "'focus' is missing",
    "focus=2": "'aperture' is missing",
    "aperture=0.05,": "an empty item",
    "aperture=0.05,,focus=1": "an empty item",
    "aperture=0.05,focus": "no '='",
    "aperture=0.05,focus=": "not a number",
    "aperture=0.05,focus=4.2x": "not a number",
    "aperture=0.05,focus=4.2,aperture=0.1": "a key given twice",
    "aperture=0.05,focus=4.2,blades=6": "an unknown key",
    "Aperture=0.05,focus=4.2": "an unknown key",
    "=0.05,focus=4.2": "an unknown key",
    "aperture=-0.05,focus=4.2": "aperture_radius = -0.05 is not a finite number >= 0",
    "aperture=nan,focus=4.2": "aperture_radius",
    "aperture=0.05,focus=0": "focus_distance = 0 is not a finite number > 0",
    "aperture=0.05,focus=inf": "focus_distance",
    "aperture=0.05;focus=4.2": "not a number",
    "aperture=" + "9" * 80 + ",focus=1": "not a number",
    "focus=1,aperture=0.05," + "x" * 300: "no '='",
}


def test_the_parser_accepts():
    for spec, (aperture, focus) in ACCEPTED.items():
        status, message, lens = lens_ref.from_spec(spec)
        assert status == 0 and message == "" and (lens.aperture_radius, lens.focus_distance) == (np.float32(aperture), np.float32(focus)), spec


def test_the_parser_refuses_and_leaves_the_lens_alone():
    for spec, why in REFUSED.items():
        status, message, lens = lens_ref.from_spec(spec)
        assert status == INVALID_ARGUMENT and message.startswith("rt_hip_lens_from_spec: ") and why in message, (spec, message)
        assert (lens.aperture_radius, lens.focus_distance) == (-1.0, -1.0) and len(message) < 256
    assert lens_ref.lib().lens_ref_from_spec(None, C.byref(capi.RtHipLens()), None, 0) == INVALID_ARGUMENT
    assert lens_ref.lib().lens_ref_from_spec(b"aperture=1,focus=1", None, None, 0) == INVALID_ARGUMENT


def test_the_librarys_entry_point_is_the_same_parser():
    """rt_hip_lens_from_spec of librt_hip.so (host-only: no device is touched) and its message through rt_hip_last_error"""
    lens = rt_amd.renderer.lens_from_spec("aperture=0.05,focus=4.2")
    assert (lens.aperture_radius, lens.focus_distance) == (np.float32(0.05), np.float32(4.2))
    with pytest.raises(rt_amd.RtHipError) as refused:
        rt_amd.renderer.lens_from_spec("aperture=0.05,focus=0")
    assert refused.value.status == INVALID_ARGUMENT and "focus_distance = 0" in str(refused.value)


if __name__ == "__main__":
    for label, (scene, w, h, _, _) in frames().items():
        _, got_words, got_eye, _ = lens_ref.words(scene, w, h, LENS)
        print(label, "against numpy, relative:", relative(got_words, numpy_words(scene, w, h, LENS, got_eye)))
    print(axes_deviation())
