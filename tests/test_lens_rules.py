"""The disk of RT_HIP_FLAG_THIN_LENS (rt_amd/csrc/lens_rules.hpp compiled with g++ into the restatement): the concentric
map with polynomial sine and cosine over a fixed lattice of 2^16 x 16 numerator pairs and the edge words, against the binary64 concentric
map and its own promises.  The bounds are the issue's: radius <= 1 + 2^-22, 5e-7 per component (4 x the 1.2e-7 a binary32 emulation saw),
0.0025 on every share of a quarter (five standard deviations at 2^20 points).

Measured here over the lattice and the edge words (`python -m tests.test_lens_rules` prints them): largest deviation from the binary64
map 1.14e-7 per component, largest radius 1 + 2.5e-8, share below half the radius 0.249997, quadrants 0.249998 .. 0.250002."""
import numpy as np
import pytest

from tests import lens_reference as lens_ref


@pytest.fixture(scope="module")
def points():
    ka, kb = lens_ref.lattice()
    return ka, kb, lens_ref.disk(ka, kb).astype(np.float64)


def concentric_map(ka, kb):
    """Shirley and Chiu's map in binary64, from the same numerators: x, y in [-1, 1); the larger magnitude is the radius (a tie: y)."""
    x, y = ka.astype(np.float64) * 2.0**-23 - 1.0, kb.astype(np.float64) * 2.0**-23 - 1.0
    first = np.abs(x) > np.abs(y)
    major, minor = np.where(first, x, y), np.where(first, y, x)
    with np.errstate(invalid="ignore", divide="ignore"):
        phi = np.where(major == 0.0, 0.0, (np.pi / 4) * minor / np.where(major == 0.0, 1.0, major))
    along, across = major * np.cos(phi), major * np.sin(phi)
    return np.stack([np.where(first, along, across), np.where(first, across, along)], axis=1)


def figures(ka, kb, p):
    radius = np.hypot(p[:, 0], p[:, 1])
    quadrants = [float(np.mean(((p[:, 0] >= 0) == sx) & ((p[:, 1] >= 0) == sy))) for sx in (True, False) for sy in (True, False)]
    return {"deviation": float(np.abs(p - concentric_map(ka, kb)).max()), "radius": float(radius.max()), "inside_half": float(np.mean(radius < 0.5)), "quadrants": quadrants}


def test_every_point_lies_in_the_disk(points):
    _, _, p = points
    assert (p[:, 0] ** 2 + p[:, 1] ** 2 <= (1.0 + 2.0**-22) ** 2).all()
    assert np.isfinite(p).all()


def test_every_component_is_the_concentric_maps(points):
    ka, kb, p = points
    assert np.abs(p - concentric_map(ka, kb)).max() <= 5e-7


def test_the_map_preserves_area(points):
    ka, kb, p = points
    n = 1 << 20  # (the lattice; the edge words are no sample of anything)
    seen = figures(ka[:n], kb[:n], p[:n])
    assert abs(seen["inside_half"] - 0.25) <= 0.0025
    for share in seen["quadrants"]:
        assert abs(share - 0.25) <= 0.0025


def test_the_edge_words(points):
    ka, kb, p = points
    edge = {pair: p[(1 << 20) + i] for i, pair in enumerate(lens_ref.EDGE_WORDS)}
    half, top = lens_ref.HALF, lens_ref.TOP
    assert tuple(edge[(half, half)]) == (0.0, 0.0)  # the zero point, by select: no 0 / 0
    s = np.sqrt(0.5)
    # x = y = -1 and x = y = 1 - 2^-23: ties, the second branch, the corners of the square on the circle
    assert np.allclose(edge[(0, 0)], (-s, -s), atol=5e-7) and np.allclose(edge[(top, top)], (s, s), atol=5e-7)
    # the two ties |x| == |y| take the second branch: major = y, q = x / y = +-1 exactly, so |lx| == |ly| up to the two polynomials' error
    for pair in ((half + 4096, half + 4096), (half + 4096, half - 4096)):
        assert abs(abs(edge[pair][0]) - abs(edge[pair][1])) <= 5e-7 * abs(edge[pair][0]) + 1e-12
    assert edge[(half + 4096, half - 4096)][0] > 0 > edge[(half + 4096, half - 4096)][1]
    # one step beside the centre: radius 2^-23, on the axis the step was taken along
    assert tuple(edge[(half + 1, half)]) == (2.0**-23, 0.0) and tuple(edge[(half - 1, half)]) == (-(2.0**-23), -0.0)
    assert tuple(edge[(half, half + 1)]) == (0.0, 2.0**-23) and tuple(edge[(half, half - 1)]) == (-0.0, -(2.0**-23))


def test_a_numerator_decides_alone(points):
    """the same pair, the same point: the map has no state"""
    ka, kb, p = points
    again = lens_ref.disk(ka[::4097], kb[::4097]).astype(np.float64)
    assert np.array_equal(again, p[::4097])


if __name__ == "__main__":
    a, b = lens_ref.lattice()
    print(figures(a[: 1 << 20], b[: 1 << 20], lens_ref.disk(a[: 1 << 20], b[: 1 << 20]).astype(np.float64)))
    print(figures(a, b, lens_ref.disk(a, b).astype(np.float64)))
