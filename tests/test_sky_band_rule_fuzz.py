"""A wider soundness sample for the sky band's rule (rt_amd/csrc/sky_band.cpp) than tests/test_sky_band_rule.py's 26 scenes,
which all sit near the world origin at two landscape sizes.

Here a seeded generator moves the whole world — scene and eye — up to 300 units from the origin, where the rule's |eye| + |c| error terms
are no longer small; renders at six sizes, among them widths below 64, odd widths and a frame taller than it is wide; and places spheres
where the rule is tight: a top near the horizontal plane through the eye (what sets the headline's R), and an eye just outside a sphere.

Every case is checked twice against the oracle's closest-hit query: all claimed rows at eleven jitters per pixel
(test_sky_band_rule.assert_rows_are_sky), and the LAST claimed row at the jitter that aims a ray lowest — kb = 2^24 - 1 — at nine ka
spread over the pixel's width.  The rule may claim fewer rows than are sky, never one that is not: a failure here is a soundness bug of
the rule, and its scene belongs into test_sky_band_rule.constructed_cases()."""
import numpy as np

from oracle import binding as oracle
from tests.test_sky_band_rule import LEVEL, UP, assert_rows_are_sky, band_rows, dump, request_line, scene_of  # noqa: F401  (dump: the fixture)

SEED = 20261020
CASES = 300
SIZES = [(64, 36), (40, 24), (33, 17), (130, 16), (17, 64), (65, 9)]
CAMERAS = LEVEL + [UP]
TRANSLATIONS = ["none", "up to 30", "up to 300"]
# how often a sphere rests on the ground, floats, tops out near eye height, has the eye just outside it: the last kind hides most of the
# frame behind one sphere, and with up to eight spheres a case it must stay rare for a case to keep a band at all
KINDS = [0.4, 0.2, 0.3, 0.1]


def fuzz_cases(seed=SEED, count=CASES):
    """(name, translation class, spheres, eye, direction, size): a world moved as a whole, a ground sphere under its origin (not in every
    seventh case), 1 to 8 spheres in all of four kinds"""
    rng = np.random.default_rng(seed)
    cases = []
    for k in range(count):
        size, direction, ahead = SIZES[k % len(SIZES)], CAMERAS[k % len(CAMERAS)], np.array(LEVEL[k % len(LEVEL)])
        moved = (k // len(SIZES)) % 3  # (every class of translation meets every size)
        reach = (0.0, 30.0, 300.0)[moved]
        shift = np.array([rng.uniform(-reach, reach), rng.uniform(0.0, 200.0) if k % 4 == 3 else 0.0, rng.uniform(-reach, reach)])
        eye = shift + np.array([rng.uniform(-2, 2), rng.uniform(0.6, 3.0), rng.uniform(-2, 4)])
        spheres = [[shift[0], shift[1] - 1000.0, shift[2], 1000.0, 0]] if k % 7 != 6 else []
        count_all = int(rng.integers(1, 9))
        while len(spheres) < count_all:
            radius = float(rng.uniform(0.15, 0.8))
            kind = int(rng.choice(4, p=KINDS))
            if kind == 0:  # resting on the ground
                centre = shift + np.array([rng.uniform(-4, 4), radius, rng.uniform(-4, 4)])
            elif kind == 1:  # floating above it
                centre = shift + np.array([rng.uniform(-4, 4), rng.uniform(1.5, 6.0), rng.uniform(-4, 4)])
            elif kind == 2:  # its top near eye height, in front of the eye: near-tangent to the horizontal plane through the eye
                distance = rng.uniform(1.0, 30.0)
                sideways = np.array([ahead[2], 0.0, -ahead[0]]) * rng.uniform(-0.3, 0.3) * distance
                centre = eye + ahead * distance + sideways
                centre[1] = eye[1] + rng.uniform(-0.02, 0.3) - radius
            else:  # the eye just outside it
                toward = rng.normal(size=3)
                centre = eye + toward / np.linalg.norm(toward) * radius * rng.uniform(1.0, 1.6)
            spheres.append([float(centre[0]), float(centre[1]), float(centre[2]), radius, 0])
        cases.append((f"fuzz-{k}", TRANSLATIONS[moved], spheres, tuple(float(v) for v in eye), direction, size))
    return cases


def assert_the_last_row_misses_at_its_lowest_rays(pod, size, rows, name):
    """row rows - 1, every pixel: kb = 2^24 - 1 aims lowest within the row; nine ka across the pixel"""
    if not rows:
        return
    high = 2.0**24 - 1.0
    origins, directions = [], []
    for x in range(size[0]):
        for ka in np.round(np.linspace(0.0, high, 9)):
            origin, direction = oracle.primary_ray(pod, size[0], size[1], x, rows - 1, float(ka), high)
            origins.append(origin)
            directions.append(direction)
    _, kind, _, _ = oracle.closest_hit(pod, np.array(origins), np.array(directions))
    hits = np.flatnonzero(kind)
    assert hits.size == 0, f"{name}: the band claims {rows} rows, but {hits.size} of the lowest rays of row {rows - 1} hit something (the first: pixel {int(hits[0]) // 9})"


def test_the_generator_is_what_it_says():
    cases = fuzz_cases()
    assert len(cases) == CASES and {size for *_, size in cases} == set(SIZES) and {direction for *_, direction, _ in cases} == set(CAMERAS)
    assert all(1 <= len(spheres) <= 8 for _, _, spheres, *_ in cases)
    assert sum(not any(s[3] == 1000.0 for s in spheres) for _, _, spheres, *_ in cases) == len([k for k in range(CASES) if k % 7 == 6])
    far = [max(abs(eye[0]), abs(eye[2])) for _, moved, _, eye, *_ in cases if moved == "up to 300"]
    assert max(far) > 150.0 and max(eye[1] for _, _, _, eye, *_ in cases) > 100.0
    assert fuzz_cases() == cases and fuzz_cases(seed=SEED + 1) != cases


def test_claimed_rows_are_sky_in_a_moved_world(dump):  # noqa: F811
    claimed = {}
    cases = fuzz_cases()
    for name, moved, spheres, eye, direction, size in cases:
        pod = scene_of(spheres, eye, direction, size)
        assert int(dump([request_line(pod, size)])[0]["pinhole"]) == 1, name  # (an axis-aligned camera: the rule is asked in earnest)
        rows = band_rows(dump, pod, size)
        claimed[name] = (moved, rows)
        assert_rows_are_sky(pod, size, rows, name)
        assert_the_last_row_misses_at_its_lowest_rays(pod, size, rows, name)
    banded = [name for name, (_, rows) in claimed.items() if rows >= 8]
    print(f"{len(banded)} of {len(cases)} cases claim a band: " + ", ".join(f"{moved}: {sum(rows >= 8 and m == moved for m, rows in claimed.values())}" for moved in TRANSLATIONS))
    # not vacuous: at least a quarter of the cases have a band, and in every translation class at least one has
    assert len(banded) * 4 >= len(cases), claimed
    for moved in TRANSLATIONS:
        assert any(m == moved and rows >= 8 for m, rows in claimed.values()), (moved, claimed)
