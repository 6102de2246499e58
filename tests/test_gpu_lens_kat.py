"""rt_amd/csrc/lens_rules.hpp on the device (rt_hip_kat_lens: the header as the lens builds of the render kernels compile it, the
contract's quotient handed in) against the same header compiled with g++ (tests/native/lens_reference.cpp: lens_ref_disk,
lens_ref_bend), word for word, over the CPU test's lattice of 2^16 x 16 numerator pairs and its edge words.  The ray that is bent is a
primary ray of each of the three camera forms a lens frame can have, with that frame's own lens words and eye."""
import numpy as np
import pytest

from tests import lens_reference as lens_ref
from tests.lens_reference import camera_pod

pytestmark = pytest.mark.gpu

LENS = (0.11, 2.7)


def words_of(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def numerators():
    return lens_ref.lattice()


@pytest.mark.parametrize("form,pixel,bent", [("pinhole", (5, 7), 1.0), ("eye", (63, 0), 1.0), ("guarded", (32, 18), 1.0), ("guarded", (0, 35), 0.0)])
def test_disk_and_ray_word_for_word(tracer, numerators, form, pixel, bent):
    """(the guarded matrix bends w so hard that its lower left rays run away from the plane the lens words describe: those stay as they are)"""
    ka, kb = numerators
    pod = camera_pod("basic", form)
    status, lens_words, eye, _ = lens_ref.words(pod, 64, 36, LENS)
    assert status == 0
    _, pinhole, _, _ = lens_ref.ray(pod, 64, 36, LENS, *pixel, sample=3, seed=2)
    ray = np.concatenate([pinhole, eye]).astype(np.float32)
    got = tracer.kat_lens(ka, kb, ray, lens_words)
    want = lens_ref.bend(ka, kb, ray, lens_words)
    assert np.array_equal(words_of(got[:, :2]), words_of(lens_ref.disk(ka, kb)))  # the disk alone
    differing = words_of(got) != words_of(want)
    assert not differing.any(), f"{int(differing.any(axis=1).sum())} of {len(ka)} items differ, first {np.argwhere(differing)[0]}"
    assert (want[:, 8] == bent).all()  # (where the rays were bent the comparison is of lens rays)


def test_a_ray_that_does_not_meet_the_plane_stays(tracer, numerators):
    """cosine <= 0, a zero focus quotient that overflows, NaN words: `bent` is 0 and the ray is the one handed in, on both sides"""
    ka, kb = numerators[0][:4096], numerators[1][:4096]
    pod = camera_pod("basic", "pinhole")
    _, lens_words, eye, _ = lens_ref.words(pod, 64, 36, LENS)
    _, pinhole, _, _ = lens_ref.ray(pod, 64, 36, LENS, 9, 9, sample=1, seed=2)
    behind = np.concatenate([pinhole[:3], -pinhole[3:], eye]).astype(np.float32)
    huge = lens_words.copy()
    huge[9] = 3.0e38
    huge[6:9] *= 1e-3  # cosine ~ 1e-3: the quotient overflows
    broken = lens_words.copy()
    broken[7] = np.nan
    for ray, lw, bent in ((behind, lens_words, 0.0), (np.concatenate([pinhole, eye]).astype(np.float32), huge, 0.0), (np.concatenate([pinhole, eye]).astype(np.float32), broken, 0.0)):
        got, want = tracer.kat_lens(ka, kb, ray, lw), lens_ref.bend(ka, kb, ray, lw)
        assert np.array_equal(words_of(got), words_of(want)) and (want[:, 8] == bent).all()
        assert np.array_equal(words_of(want[:, 2:8]), np.broadcast_to(words_of(ray[:6]), (len(ka), 6)))
