"""The CPU restatement of RT_HIP_FLAG_DIRECT_LIGHT (tests/native/direct_reference.cpp) on its own, without a GPU: with no
sampled light it is light_reference.cpp's frame, its vertex estimator has the expectation a closed form gives, an occluder makes it
exactly 0, a binary64 tracer written from §3.13's text agrees with it, and `segments` counts the shadow queries.

No test here compares the flag's frame with the RT_HIP_FLAG_EMISSION frame's mean: the two converge to different images (§3.13)."""
import numpy as np
import pytest

import rt_amd
from oracle import binding as oracle
from tests import direct_reference as direct_ref
from tests import light_reference as light_ref

DRAWS = 1 << 18


@pytest.fixture(scope="module")
def camera():
    return rt_amd.Scene.named("basic").describe(64, 36)


def glow(which=1, rgb=(1.0, 1.0, 1.0), n_materials=4):
    table = np.zeros((n_materials, 3), dtype=np.float32)
    table[which] = rgb
    return table


@pytest.mark.parametrize("sm", [False, True])
def test_without_a_sampled_light_it_is_the_light_restatement(camera, sm):
    """A table with no light; a plane that glows; a glowing sphere of radius 0: frame, float mean and counters of light_ref_render, bit
    for bit — and with `direct` off it is that function whatever the scene holds."""
    lights = light_ref.lights_scene().describe(64, 36)
    plane_light = light_ref.scene_pod(camera, spheres=[(0, 0.5, 0, 0.5, 3), (1, 0.5, 0.5, 0.5, 0), (-1, 0.4, 0.5, 0.0, 1)], planes=[(0, 1, 0, 0, 0), (0, 1, 0, -4, 1)])
    for pod, table, direct in ((lights, None, True), (plane_light, glow(), True), (lights, light_ref.LIGHTS_TABLE, False)):
        assert not direct or direct_ref.count(pod, table) == 0
        want_rgba, want_rgb, want = light_ref.render(pod, 64, 36, table, seed=5, sm_materials=sm)
        rgba, rgb, stats = direct_ref.render(pod, 64, 36, table, seed=5, sm_materials=sm, direct=direct)
        assert np.array_equal(rgba, want_rgba) and np.array_equal(rgb.view(np.uint32), want_rgb.view(np.uint32))
        assert stats["segments"] == want["segments"] and stats["primary_samples"] == want["primary_samples"]


def within_five_standard_errors(mean, mean_square, expectation):
    """The estimator's draws are independent (distinct generator steps of one stream), so the mean of DRAWS of them has the standard error
    sqrt(variance / DRAWS) with the variance from the returned second moment; 5 standard errors are exceeded by chance once in 1.7 million."""
    standard_error = np.sqrt(max(mean_square - mean * mean, 0.0) / DRAWS)
    assert standard_error > 0 and abs(mean - expectation) <= 5.0 * standard_error, (mean, expectation, standard_error)


@pytest.mark.parametrize("point,centre,radius", [((0, 0, 0), (0, 3, 0), 0.5), ((2, 0, 0), (0, 3, 0), 0.5), ((0.5, 0, -1), (1, 2, 0.5), 0.75)])
def test_the_vertex_estimator_has_the_closed_forms_expectation(camera, point, centre, radius):
    """An unoccluded sphere light of radiance 1 above a point of the plane y = 0: the irradiance over pi is (R / D)^2 cos(theta), theta between
    the normal and the direction to the centre (the whole sphere is above the horizon in every case here)."""
    pod = light_ref.scene_pod(camera, spheres=[(*centre, radius, 1)], planes=[(0, 1, 0, 0, 0)])
    toward = np.array(centre, dtype=np.float64) - np.array(point, dtype=np.float64)
    distance = np.linalg.norm(toward)
    assert centre[1] - radius > 0
    mean, mean_square, segments = direct_ref.vertex(pod, glow(), point, (0, 1, 0), DRAWS, seed=3)
    within_five_standard_errors(mean, mean_square, (radius / distance) ** 2 * toward[1] / distance)
    assert 0 < segments <= DRAWS


def test_the_vertex_estimator_inside_an_enclosing_light_is_one(camera):
    """A point at the centre of a light of radiance 1 that encloses it: the cosine-weighted mean radiance is 1."""
    pod = light_ref.scene_pod(camera, spheres=[(0, 1, 0, 5, 1)])
    mean, mean_square, segments = direct_ref.vertex(pod, glow(), (0, 1, 0), (0, 1, 0), DRAWS, seed=4)
    within_five_standard_errors(mean, mean_square, 1.0)
    assert 0 < segments <= DRAWS


def test_three_lights_share_the_draws(camera):
    """n = 3: each light is aimed at a third of the time and weighted by 3 — the expectation is the sum of the three closed forms."""
    lights = [((-2, 3, 0), 0.5), ((0, 3, 0), 0.5), ((2, 4, 1), 0.75)]
    pod = light_ref.scene_pod(camera, spheres=[(*c, r, 1) for c, r in lights], planes=[(0, 1, 0, 0, 0)])
    assert direct_ref.count(pod, glow()) == 3
    want = sum((r / np.linalg.norm(c)) ** 2 * c[1] / np.linalg.norm(c) for c, r in lights)
    mean, mean_square, _ = direct_ref.vertex(pod, glow(), (0, 0, 0), (0, 1, 0), DRAWS, seed=5)
    within_five_standard_errors(mean, mean_square, want)


def test_an_occluder_gives_exactly_zero(camera):
    pod = light_ref.scene_pod(camera, spheres=[(0, 3, 0, 0.5, 1), (0, 1.5, 0, 0.8, 0)], planes=[(0, 1, 0, 0, 0)])
    mean, mean_square, segments = direct_ref.vertex(pod, glow(), (0, 0, 0), (0, 1, 0), 1 << 14, seed=6)
    assert mean == 0.0 and mean_square == 0.0
    assert segments > 1000  # the shadow queries ran, were counted, and found the occluder


# ---- a binary64 tracer written from §3.13's text ----------------------------------------------------------------------------------
SPHERES = [(1.6, 2.6, -0.4, 0.6, 1), (-0.9, 0.7, -0.2, 0.7, 0), (0.9, 0.45, 0.6, 0.45, 2), (-0.1, 1.7, 0.4, 0.3, 3)]  # lamp, clay, mirror, occluder
MATERIALS = [(light_ref.LAMBERT, (0.8, 0.8, 0.3), 0.0, 1.0), (light_ref.LAMBERT, (0.5, 0.5, 0.5), 0.0, 1.0), (light_ref.METAL, (0.9, 0.6, 0.4), 0.0, 1.0), (light_ref.LAMBERT, (0.3, 0.5, 0.8), 0.0, 0.8)]
EMISSION = np.array([6.0, 5.0, 3.0])


def closest_hit64(o, d, margin=None):
    """(t, kind, index, risky): spheres and the plane y = 0 in float64; nothing nearer than 0.001; a sphere wins a tie"""
    best_t, kind, index, risky = np.inf, 0, 0, False
    for k, (cx, cy, cz, r, _m) in enumerate(SPHERES):
        e = np.array([cx, cy, cz]) - o
        a = e @ d
        e2 = e @ e
        disc = r * r - (e2 - a * a)
        risky |= abs(np.sqrt(max(e2 - a * a, 0.0)) - r) < 1e-4
        if disc < 0:
            continue
        f = np.sqrt(disc)
        t = a + f if e2 < r * r else a - f
        risky |= abs(t - 1e-3) < 1e-4
        if t >= 1e-3 and t < best_t:
            best_t, kind, index = t, 1, k
    if abs(d[1]) > 1e-6:
        t = -o[1] / d[1]
        risky |= abs(t - 1e-3) < 1e-4 or abs(t - best_t) < 1e-4
        if t >= 1e-3 and t < best_t:
            best_t, kind, index = t, 2, 0
    return best_t, kind, index, risky


def vertex64(ka, kb, kc, x, nrm, sampled):
    """§3.13's vertex rule in float64: (weight, w, light) or None where it skips"""
    n = len(sampled)
    C, R, idx = sampled[(kc * n) >> 24]
    u, v = ka * 2.0**-23 - 1.0, kb * 2.0**-23 - 1.0
    z = 1.0 - abs(u) - abs(v)
    if z < 0:
        u, v = (1.0 - abs(v)) * (1.0 if u >= 0 else -1.0), (1.0 - abs(u)) * (1.0 if v >= 0 else -1.0)
    p = np.array([u, v, z])
    length = np.linalg.norm(p)
    omega = p / length
    d0 = x - C
    inside = d0 @ d0 < R * R
    if not inside and omega @ d0 < 0:
        omega = -omega
    t = C + R * omega - x
    d2 = t @ t
    w = t / np.sqrt(d2)
    cx = nrm @ w
    cy = omega @ w if inside else -(omega @ w)
    risky = abs(cx) < 1e-4 or abs(cy) < 1e-4
    if not (cx > 0) or not (cy > 0) or not (d2 > 0):
        return None, risky
    return (cx * cy * R * R * n * (4 if inside else 2) / (np.pi * d2 * length**3), w, idx), risky


def test_a_binary64_tracer_written_from_the_contract_agrees():
    """max_bounces = 1 at spp 1 is "primary hit plus direct light", and sample 0 goes through the pixel centre and draws nothing before the
    vertex step: the sample is E where the primary ray hits the lamp, the sky where it misses, 0 on the mirror, and at a lambert hit the
    vertex rule's contribution from the stream's first step.  48 x 27, the tolerance of tests/test_light_reference.py's binary64 tracer:
    1e-5 relative, pixels whose float64 path has a margin below 1e-4 (or a weight that moves with the float32 rounding of its vertex, below)
    left out, at most 2 % of the frame."""
    width, height, seed = 48, 27, 2
    camera = rt_amd.Scene.named("basic").describe(width, height)
    pod = light_ref.scene_pod(camera, spheres=SPHERES, planes=[(0, 1, 0, 0, 0)], spp=1, bounces=1, materials=MATERIALS)
    table = np.array([(0, 0, 0), tuple(EMISSION), (0, 0, 0), (0, 0, 0)], dtype=np.float32)
    assert direct_ref.count(pod, table) == 1
    _, rgb, stats = direct_ref.render(pod, width, height, table, seed=seed)
    _, _, implicit = light_ref.render(pod, width, height, table, seed=seed)
    sampled = [(np.array(SPHERES[0][:3]), SPHERES[0][3], 0)]
    attenuation = {m: np.array(albedo) * reflectivity for m, (_, albedo, _, reflectivity) in enumerate(MATERIALS)}
    want = np.zeros((height, width, 3))
    risky = np.zeros((height, width), dtype=bool)
    shadow_queries = kinds = 0
    seen = set()
    for y in range(height):
        for x in range(width):
            origin, direction = oracle.primary_ray(pod, width, height, x, y)[:2]
            o, d = np.array(origin, dtype=np.float64), np.array(direction, dtype=np.float64)
            d /= np.linalg.norm(d)
            t, kind, index, risky[y, x] = closest_hit64(o, d)
            if kind == 0:
                sky_t = 0.5 * (d[1] + 1.0)
                want[y, x] = [1.0 + (c - 1.0) * sky_t for c in (0.5, 0.7, 1.0)]
                seen.add("sky")
                continue
            material = SPHERES[index][4] if kind == 1 else 0
            if material == 1:
                want[y, x] = EMISSION  # seen from the camera the lamp counts on hit
                seen.add("lamp")
                continue
            if MATERIALS[material][0] == light_ref.METAL:
                seen.add("mirror")
                continue  # no vertex rule, and no bounce left: 0
            point = o + d * t
            normal = (point - np.array(SPHERES[index][:3])) / SPHERES[index][3] if kind == 1 else np.array([0.0, 1.0, 0.0])
            ka, kb, kc = (int(u * 2.0**24) for u in oracle.random(seed, y * width + x, 0, 3))
            aimed, near_zero = vertex64(ka, kb, kc, point, normal, sampled)
            risky[y, x] |= near_zero
            if aimed is None:
                seen.add("skipped")
                continue
            weight, w, light = aimed
            # (conditioning: the restatement's vertex is the frozen oracle's float32 hit — near a sphere's silhouette t = a - sqrt(disc) cancels
            # and point and normal are off by up to 1e-5.  Where moving this tracer's vertex onto the oracle's moves the weight by more than
            # half the tolerance, the path has no margin — like a grazing ray's — and says nothing about the vertex rule's arithmetic)
            distance32, _, _, normal32 = oracle.closest_hit(pod, [origin], [direction])
            moved, _ = vertex64(ka, kb, kc, np.array(origin, dtype=np.float64) + np.array(direction, dtype=np.float64) * float(distance32[0]), normal32[0].astype(np.float64), sampled)
            risky[y, x] |= moved is None or abs(moved[0] - weight) > 0.5e-5 * weight
            shadow_queries += 1
            _, shadow_kind, shadow_index, grazing = closest_hit64(point, w)
            risky[y, x] |= grazing
            if shadow_kind == 1 and shadow_index == light:
                want[y, x] = attenuation[material] * EMISSION * weight
                seen.add("lit")
            else:
                seen.add("shadowed")
    assert seen == {"sky", "lamp", "mirror", "skipped", "lit", "shadowed"}
    assert risky.mean() <= 0.02, risky.mean()
    assert np.allclose(rgb.astype(np.float64)[~risky], want[~risky], rtol=1e-5, atol=0.0)
    # `segments` counts the shadow queries: one primary segment per pixel, plus one per vertex that aimed
    assert implicit["segments"] == width * height
    assert abs((stats["segments"] - width * height) - shadow_queries) <= risky.sum() and stats["segments"] > width * height + 100


def test_segments_count_shadow_queries_in_longer_paths():
    pod = light_ref.lights_scene(spp=4).describe(48, 27)
    _, _, direct = direct_ref.render(pod, 48, 27, light_ref.LIGHTS_TABLE, seed=7, want_rgb=False)
    _, _, implicit = light_ref.render(pod, 48, 27, light_ref.LIGHTS_TABLE, seed=7, want_rgb=False)
    assert direct["segments"] > implicit["segments"] and direct["primary_samples"] == implicit["primary_samples"]


# ---- the census of the restatement (direct_ref_render_census) ---------------------------------------------------------------------------
def without_seconds(stats):
    return {k: v for k, v in stats.items() if k != "seconds"}


@pytest.mark.parametrize("sm", [False, True])
def test_a_census_render_is_direct_ref_renders_bytes(sm):
    """lights.toml at 64x36: frame, float mean and stats of direct_ref_render byte for byte — and through the C entry point with the
    census pointer null it is that function too (nothing is counted)."""
    import ctypes as C

    pod = light_ref.lights_scene().describe(64, 36)
    rgba, rgb, stats = direct_ref.render(pod, 64, 36, light_ref.LIGHTS_TABLE, seed=5, sm_materials=sm)
    c_rgba, c_rgb, c_stats, counts, own, watched = direct_ref.render_census(pod, 64, 36, light_ref.LIGHTS_TABLE, seed=5, sm_materials=sm)
    assert rgba.tobytes() == c_rgba.tobytes() and rgb.tobytes() == c_rgb.tobytes() and without_seconds(stats) == without_seconds(c_stats)
    assert list(counts) == oracle.CENSUS_EVENTS and list(own) == direct_ref.OWN_EVENTS and watched is None
    n_rgba, n_rgb, n_stats = np.zeros_like(rgba), np.zeros_like(rgb), oracle.OracleStats()
    own_words = np.full(len(direct_ref.OWN_EVENTS), 7, dtype=np.uint64)
    table = light_ref.LIGHTS_TABLE
    rc = direct_ref.lib().direct_ref_render_census(C.byref(pod), 64, 36, 5, oracle.MATERIALS_SM if sm else 0, None, n_rgba.ctypes.data, n_rgb.ctypes.data, 2, C.byref(n_stats), table.ctypes.data, len(table), 1, None,
                                                   own_words.ctypes.data, -1, 0, None)
    assert rc == 0 and rgba.tobytes() == n_rgba.tobytes() and rgb.tobytes() == n_rgb.tobytes() and without_seconds(stats) == without_seconds(n_stats.as_dict())
    assert (own_words == 0).all()
    # bookkeeping the counts must satisfy: every segment is a sample's first, follows a scatter that went on, or is a shadow query
    scatters = counts["lambert_rule"] + counts["lambert_near_zero"] + counts["lambert_ordinary"] + counts["metal_scattered"] + counts["dielectric_total_internal"] + counts["dielectric_reflected"] + counts["dielectric_refracted"]
    assert stats["segments"] == stats["primary_samples"] + scatters - counts["out_of_bounces"] + own["vertex_aimed"]
    assert own["vertex_aimed"] == own["shadow_visible"] + own["shadow_occluded"]
    # every lambert vertex that goes on to scatter ran the rule once (a lambert scatter never absorbs)
    assert own["vertex_aimed"] + own["vertex_not_aimed"] == counts["lambert_rule"] + counts["lambert_near_zero"] + counts["lambert_ordinary"]
    for event in ("vertex_aimed", "vertex_not_aimed", "shadow_visible", "shadow_occluded", "fold_below", "sampled_light_after_sampling_vertex", "light_on_primary", "first_vertex_aimed", "first_vertex_not_aimed"):
        assert own[event] > 0, event
    assert own["inside_light"] == 0 and own["chose_last_of_256"] == 0 and own["zero_word_k"] == 0
    assert (own["sampled_light_after_other_vertex"] > 0) or not sm  # (behind the glass sphere under the sm table, behind the brass one under both)


def test_the_census_of_a_frame_without_the_flag_counts_no_vertex():
    """`direct` off: light_ref_render's frame, the oracle's events under the loop, and none of the rule's."""
    pod = light_ref.lights_scene().describe(64, 36)
    want_rgba, want_rgb, want = light_ref.render(pod, 64, 36, light_ref.LIGHTS_TABLE, seed=5)
    rgba, rgb, stats, counts, own, _ = direct_ref.render_census(pod, 64, 36, light_ref.LIGHTS_TABLE, seed=5, direct=False)
    assert rgba.tobytes() == want_rgba.tobytes() and rgb.tobytes() == want_rgb.tobytes() and stats["segments"] == want["segments"]
    assert counts["lambert_ordinary"] > 0 and own["light_on_primary"] > 0
    assert all(own[e] == 0 for e in direct_ref.OWN_EVENTS if e != "light_on_primary"), own


def test_the_watched_sample_is_one_sample_of_the_frame():
    """watch = (pixel, sample): the own events of that sample alone — at most one first vertex, and summed over every (pixel, sample) of a
    small frame the watched counts are the frame's."""
    width, height, spp = 6, 4, 3
    pod = light_ref.lights_scene(spp=spp).describe(width, height)
    _, _, _, _, own, _ = direct_ref.render_census(pod, width, height, light_ref.LIGHTS_TABLE, seed=8)
    total = dict.fromkeys(direct_ref.OWN_EVENTS, 0)
    for pixel in range(width * height):
        for sample in range(spp):
            _, _, _, _, again, watched = direct_ref.render_census(pod, width, height, light_ref.LIGHTS_TABLE, seed=8, watch=(pixel, sample), threads=1)
            assert again == own and watched["first_vertex_aimed"] + watched["first_vertex_not_aimed"] + watched["light_on_primary"] <= 1
            for event, n in watched.items():
                total[event] += n
    assert total == own and own["vertex_aimed"] > 0


def test_the_rare_rules_switch_is_honoured_under_the_direct_loop():
    """ORACLE_TEST_NO_RARE_RULES reaches render_frame through direct_ref_render_census as through oracle_render_census: lambert's
    approx_zero replacement off changes a frame whose plane faces a unit vector exactly; direct_ref_render ignores the bit."""
    import ctypes as C

    from tests import light_rare_cases as lrc

    case = lrc.case("direct_approx_zero_exact_lamp_in_front")
    pod, table = case.pod(), case.table()
    on = direct_ref.render_census(pod, lrc.W, lrc.H, table, seed=case.seed)
    off = direct_ref.render_census(pod, lrc.W, lrc.H, table, seed=case.seed, rare_rules=False)
    assert on[3]["lambert_rule"] == off[3]["lambert_rule"] == 1 and on[1].tobytes() != off[1].tobytes()
    rgba, rgb = np.zeros((lrc.H, lrc.W), dtype=np.uint32), np.zeros((lrc.H, lrc.W, 3), dtype=np.float32)
    assert direct_ref.lib().direct_ref_render(C.byref(pod), lrc.W, lrc.H, case.seed, oracle.TEST_NO_RARE_RULES, None, rgba.ctypes.data, rgb.ctypes.data, 1, None, table.ctypes.data, len(table), 1) == 0
    assert rgb.tobytes() == on[1].tobytes()
