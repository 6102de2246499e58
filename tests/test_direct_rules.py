"""rt_amd/csrc/direct_light_rules.hpp as g++ compiles it, without a GPU: the octahedral map — unit length up to the
contract's normalize, its fold lines and corners, its density |p|^3 / 4 integrating to 1 — and the choice of the light."""
import numpy as np

from tests import direct_reference as direct_ref

TOP = (1 << 24) - 1
HALF = 1 << 23


def unit(point):
    x, y, z, l2 = (np.float32(v) for v in point)
    inv = np.float32(1.0 / np.sqrt(np.float64(l2)))  # (the contract's inv_sqrt is this within an ulp)
    return np.array([x * inv, y * inv, z * inv], dtype=np.float32)


def reference_point(ka, kb):
    """the map in exact rational arithmetic (every value is a multiple of 2^-23 of magnitude <= 2: binary64 holds it exactly)"""
    u, v = ka / HALF - 1.0, kb / HALF - 1.0
    z = 1.0 - abs(u) - abs(v)
    if z < 0:
        u, v = (1.0 - abs(v)) * (1.0 if u >= 0 else -1.0), (1.0 - abs(u)) * (1.0 if v >= 0 else -1.0)
    return u, v, z


def test_corners_fold_lines_and_a_grid_of_numerators():
    ticks = sorted({0, 1, HALF - 1, HALF, HALF + 1, TOP - 1, TOP, HALF // 2, HALF // 2 + 1, HALF + HALF // 2, HALF + HALF // 2 - 1, 12345, 9999999, *range(0, TOP, TOP // 37)})
    for ka in ticks:
        for kb in ticks:
            got = direct_ref.octahedral(ka, kb)
            u, v, z = reference_point(ka, kb)
            assert (float(got[0]), float(got[1]), float(got[2])) == (u, v, z), (ka, kb)
            assert abs(got[0]) + abs(got[1]) + abs(got[2]) == 1.0  # on the octahedron, exactly
            assert got[3] >= np.float32(1.0 / 3.0) * np.float32(1 - 2**-22)  # |p| >= 1/sqrt(3): never zero
            assert abs(float(got[3]) - (u * u + v * v + z * z)) <= 2**-22
            w = unit(got).astype(np.float64)
            assert abs(np.dot(w, w) - 1.0) < 4e-7, (ka, kb)
    # the corners of the square all fold onto the south pole; the centre is the north pole; the fold lines |u| + |v| = 1 are the equator
    for ka, kb in ((0, 0), (0, TOP), (TOP, 0)):
        p = direct_ref.octahedral(ka, kb)
        assert p[2] <= -1.0 + 2**-22 and abs(p[0]) <= 2**-22 and abs(p[1]) <= 2**-22
    assert tuple(direct_ref.octahedral(HALF, HALF)[:3]) == (0.0, 0.0, 1.0)
    assert tuple(direct_ref.octahedral(0, HALF)[:3]) == (-1.0, 0.0, 0.0) and tuple(direct_ref.octahedral(HALF, 0)[:3]) == (0.0, -1.0, 0.0)
    for ka in (HALF // 2, HALF + HALF // 2):
        assert direct_ref.octahedral(ka, HALF + (HALF - abs(ka - HALF)))[2] == 0.0
    # sgn(0) = +1: a folded point with u == 0 keeps a non-negative x
    p = direct_ref.octahedral(HALF, 0)
    assert p[0] == 0.0 and not np.signbit(p[0])


def test_the_density_integrates_to_one():
    """The map sends the uniform square (u, v) in [-1, 1)^2, area 4, onto the octahedron |x| + |y| + |z| = 1, whose faces have the area
    element sqrt(3) du dv at the distance 1 / sqrt(3) from the origin: a cell du dv subtends the solid angle du dv / |p|^3, so omega has
    the density |p|^3 / 4 per unit solid angle — and the cells' solid angles must add up to the sphere's 4 pi.  Midpoint rule over
    256 x 256 cells of the numerator square with the header's own l2 (the integrand is smooth inside a face and the cells do not straddle
    the fold lines, so the rule's error is of the order of h^2 = 6e-5; 1e-3 leaves room for its constant)."""
    n = 256
    k = [int((i + 0.5) * (1 << 24) / n) for i in range(n)]
    l2 = np.array([[direct_ref.octahedral(ka, kb)[3] for kb in k] for ka in k], dtype=np.float64)
    cell = (2.0 / n) ** 2
    solid_angle = (cell / l2**1.5).sum()
    assert abs(solid_angle / (4.0 * np.pi) - 1.0) < 1e-3
    # ... and with the flip of the side rule the facing hemisphere gets both halves: density |p|^3 / 2 over 2 pi
    assert abs((cell / l2**1.5).sum() / 2.0 / (2.0 * np.pi) - 1.0) < 1e-3


def test_the_choice_of_the_light_covers_every_light_and_never_reaches_n():
    for n in (1, 3, 256):
        picks = {(kc * n) >> 24 for kc in (0, 1, TOP, TOP - 1, HALF, *range(0, TOP, 4099))} | {((TOP - i) * n) >> 24 for i in range(8)}
        for light in range(n):  # the first and last numerator that pick each light
            first = -(-(light << 24) // n)
            picks |= {(first * n) >> 24, ((first + 1) * n) >> 24}
            assert (first * n) >> 24 == light and (first == 0 or ((first - 1) * n) >> 24 == light - 1)
        assert picks == set(range(n)), n
        assert (TOP * n) >> 24 == n - 1 and TOP * n < 1 << 32
