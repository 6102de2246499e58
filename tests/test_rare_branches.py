"""The scatter tail's rare branches, on the CPU: the oracle's branch census (oracle_render_census) says that every constructed case of
tests/rare_cases.py reaches the branch it was built for — and, where the branch is one of the two rare RULES (the re-draw of a zero
random vector, lambert's approx_zero replacement), that the target pixel's float mean changes in bits when the rule is switched off.
tests/test_gpu_rare_branches.py then holds every build of the render kernel to these frames.  Every precondition is asserted here, from
the oracle, never from the kernel under test.

Also here: the census itself (a census render is oracle_render's bytes), the recorded stream events re-derived from oracle.random, the
search that found them, and the invariant behind all of it — every event of the census is reached by a constructed case or by a frame
the GPU parity suite renders (profiles/r18/branch_census.txt, written by tools/branch_census.py)."""
import ctypes as C

import numpy as np
import pytest

import rt_amd
from oracle import binding as oracle
from tests import box_reference as box_ref
from tests import rare_cases as rc
from tests.conftest import ROOT
from tools import find_stream_events as search

W, H = rc.W, rc.H


# ---- the census ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,width,height,spp,seed,sm", [("dielectric", 48, 27, 6, 3, True), ("dielectric", 48, 27, 6, 3, False), ("basic", 33, 17, 20, 9, False)])
def test_a_census_render_is_oracle_renders_bytes(name, width, height, spp, seed, sm):
    pod = rt_amd.Scene.named(name).set_sampling(spp).describe(width, height)
    rgba, rgb, stats = oracle.render(pod, width, height, seed=seed, sm_materials=sm)
    c_rgba, c_rgb, c_stats, counts = oracle.render_census(pod, width, height, seed=seed, sm_materials=sm)
    assert rgba.tobytes() == c_rgba.tobytes() and rgb.tobytes() == c_rgb.tobytes()
    assert {k: v for k, v in stats.items() if k != "seconds"} == {k: v for k, v in c_stats.items() if k != "seconds"}
    assert list(counts) == oracle.CENSUS_EVENTS
    # bookkeeping the counts must satisfy: every segment but a sample's first follows a scatter that went on
    scatters = counts["lambert_rule"] + counts["lambert_near_zero"] + counts["lambert_ordinary"] + counts["metal_scattered"] + counts["dielectric_total_internal"] + counts["dielectric_reflected"] + counts["dielectric_refracted"]
    assert stats["segments"] == width * height * spp + scatters - counts["out_of_bounces"]
    assert counts["dielectric_from_inside"] + counts["dielectric_from_outside"] == counts["dielectric_total_internal"] + counts["dielectric_reflected"] + counts["dielectric_refracted"]
    assert (counts["dielectric_from_outside"] > 0) == sm


@pytest.mark.parametrize("name,sm", rc.CASE_TABLES)
def test_the_census_frame_of_every_case_is_the_reference(name, sm):
    case = rc.case(name)
    rgba, rgb, segments = rc.reference(name, sm)
    c_rgba, c_rgb, c_segments, _ = rc.census(name, sm)
    assert rgba.tobytes() == c_rgba.tobytes() and rgb.tobytes() == c_rgb.tobytes() and segments == c_segments
    assert case.pod().samples_per_pixel == case.spp <= 48  # tens of samples, never hundreds


def test_oracle_render_ignores_the_test_only_mode_bit():
    """ORACLE_TEST_NO_RARE_RULES is honoured by oracle_render_census alone: what bench.py, smoke() and every parity test call cannot be
    switched into it."""
    case = rc.case("approx_zero_exact")
    pod = case.pod()
    rgba, rgb = np.zeros((H, W), dtype=np.uint32), np.zeros((H, W, 3), dtype=np.float32)
    assert oracle.lib().oracle_render(C.byref(pod), W, H, case.seed, oracle.TEST_NO_RARE_RULES, None, rgba.ctypes.data, rgb.ctypes.data, 1, None) == 0
    want_rgba, want_rgb, _ = rc.reference(case.name, False)
    assert rgba.tobytes() == want_rgba.tobytes() and rgb.tobytes() == want_rgb.tobytes()
    off = rc.census(case.name, False, rare_rules=False)
    assert off[1].tobytes() != want_rgb.tobytes()  # ... and through the census entry point the bit does switch


# ---- the recorded stream events ----------------------------------------------------------------------------------------------------------
def test_every_recorded_event_draws_the_zero_word():
    """tests/golden/stream_events.json, re-derived from oracle.random: the three draws of that step are 0.0; the inversion of
    tools/find_stream_events.py names the same position; and a handful of each kind is there."""
    assert {kind: len(rc.events_of(kind)) >= 3 for kind in ("redraw_first_scatter", "redraw_second_scatter", "zero_jitter")} == {"redraw_first_scatter": True, "redraw_second_scatter": True, "zero_jitter": True}
    for e in rc.EVENTS:
        draws = oracle.random(e["seed"], e["pixel"], e["sample"], 3 * e["step"])
        assert (draws[-3:].view(np.uint32) == 0).all(), e
        assert (draws[:-3].reshape(-1, 3) != 0).any(axis=1).all(), e  # ... and no earlier step of the sample does
        assert e["width"] == W and 0 <= e["pixel"] < W * H and e["sample"] <= 40
        assert search.kind_of(e["sample"], e["step"]) == e["kind"]
        with np.errstate(over="ignore"):
            position = search.zero_word_positions(np.array([e["seed"]], dtype=np.uint64), np.array([e["pixel"]], dtype=np.uint32))
        assert int(position[0, 0]) == (e["sample"] << 12) + e["step"], e
        if e["kind"] != "zero_jitter":  # random_unit_vector at that step takes two steps, and gives what the NEXT step draws
            u, steps = oracle.unit_vector(e["seed"], e["pixel"], e["sample"], e["step"])
            again, once = oracle.unit_vector(e["seed"], e["pixel"], e["sample"], e["step"] + 1)
            assert (steps, once) == (2, 1) and u.tobytes() == again.tobytes()


def test_the_search_finds_what_the_fixture_records():
    """A thousand seeds around the first entry: the search finds it, and nothing the fixture does not know."""
    found = search.search(W, H, 40, 64000, 1000)
    assert found == [e for e in rc.EVENTS if 64000 <= e["seed"] < 65000] and len(found) == 1


def test_the_unit_vector_leaf_is_the_normalised_step():
    """oracle.unit_vector against the same step's three draws: parallel to them, of unit length to a rounding."""
    for seed, pixel, sample, step in [(7, 27, 0, 1), (7, 27, 17, 2), (1, 0, 3, 5)]:
        u, steps = oracle.unit_vector(seed, pixel, sample, step)
        d = oracle.random(seed, pixel, sample, 3 * step)[-3:].astype(np.float64)
        assert steps == 1 and abs(np.linalg.norm(u.astype(np.float64)) - 1.0) < 2e-7
        assert np.abs(u.astype(np.float64) - d / np.linalg.norm(d)).max() < 2e-7


# ---- the constructed cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sm", rc.CASE_TABLES)
def test_every_case_reaches_the_branch_it_claims(name, sm):
    case = rc.case(name)
    _, rgb, _, counts = rc.census(name, sm)
    for event, (relation, count) in case.expect(sm).items():
        assert (counts[event] == count) if relation == "==" else (counts[event] >= count), (name, sm, event, counts[event], relation, count)
    if case.quiet_seed is not None:  # the neighbouring seed: no such event anywhere in the frame
        quiet = rc.census(name, sm, seed=case.quiet_seed)[3]
        assert quiet["redraw"] == 0 and quiet["zero_jitter"] == 0, (name, quiet)
    rule_applies = case.sensitive and case.expect(sm).get("redraw", ("==", 1))[1] != 0
    if rule_applies:  # with the two rare rules off, the target pixel — and only it — is another number
        off_rgb = rc.census(name, sm, rare_rules=False)[1]
        x, y = case.target_xy
        differs = (off_rgb.view(np.uint32) != rgb.view(np.uint32)).any(axis=-1)
        assert differs[y, x], f"{name}: pixel ({x}, {y}) does not depend on the rule"
        assert differs.sum() == 1 or "with_sphere" in name, (name, np.argwhere(differs))


def test_the_redraw_events_sit_where_the_cases_say():
    """The re-draw cases' event is the sample's first (or second) scatter: every primary ray hits the big sphere, and behind it every first
    scatter reaches the wall."""
    pod = rc.case("redraw_lambert").pod()
    corners = [(x, y, ka, kb) for x in range(W) for y in range(H) for ka in (0.0, 2.0**24 - 1) for kb in (0.0, 2.0**24 - 1)]
    rays = [oracle.primary_ray(pod, W, H, x, y, ka, kb) for x, y, ka, kb in corners]
    distance, kind, _, normal = oracle.closest_hit(pod, [r[0] for r in rays], [r[1] for r in rays])
    assert (kind == 1).all() and (normal[:, 2] >= 0.9).all()  # the sphere, on its cap towards the camera: normal + u heads for z > 0
    for name in ("redraw_second_scatter_wall", "redraw_second_scatter_wall_sample4", "redraw_second_scatter_wall_metal"):
        case = rc.case(name)
        assert next(e for e in rc.EVENTS if e["seed"] == case.seed)["step"] == 3
        counts = rc.census(name, False)[3]
        samples = W * H * case.spp
        if "metal" in name:  # a sample scatters off the sphere, and off the wall unless the sphere absorbed it
            assert counts["metal_scattered"] + counts["metal_absorbed"] >= samples and counts["lambert_ordinary"] >= counts["metal_scattered"] - samples
        else:  # every sample scatters twice (and then some)
            assert counts["lambert_ordinary"] >= 2 * samples


def test_a_closed_sphere_holds_no_path():
    """Why the second-scatter case is built with a wall and not inside a closed sphere: a sphere met from inside keeps its OUTWARD normal
    (mg_ray_tracer.cpp:85), so lambert's normal + u leaves through the surface — exactly one scatter per sample, and the sky."""
    pod = rt_amd.scene_from_arrays([(0.0, 0.0, 0.0, 30.0, 0)], None, [rc.material(rc.LAMBERT)], samples_per_pixel=5, max_bounces=5, inverse_view_projection=rc.FRONT)
    _, rgb, stats, counts = oracle.render_census(pod, W, H, seed=744588)
    assert counts["lambert_ordinary"] == W * H * 5 and counts["metal_scattered"] == 0
    assert stats["segments"] == 2 * W * H * 5 and counts["out_of_bounces"] == 0 and (rgb > 0).all()


@pytest.mark.parametrize("name,sm", rc.CASE_TABLES)
def test_the_box_off_to_the_side_is_never_hit(name, sm):
    """RT_HIP_FLAG_TRACE_BOXES runs get one box far away: the restatement that traces boxes gives the oracle's frame, so oracle.render stays
    the yardstick of those runs too."""
    case = rc.case(name)
    pod = case.pod(boxes=True)
    assert pod.n_boxes == 1
    rgba, rgb, stats = box_ref.render(pod, W, H, seed=case.seed, sm_materials=sm)
    want_rgba, want_rgb, want_segments = rc.reference(name, sm)
    assert rc.same_bits(rgb, want_rgb, nan_ok=case.nan_ok) and rgba.tobytes() == want_rgba.tobytes() and stats["segments"] == want_segments


def test_the_sphere_wins_the_tie():
    case = rc.case("sphere_plane_tie")
    _, rgb, _, counts = rc.census(case.name, False)
    x, y = case.target_xy
    assert counts["sphere_plane_tie"] == 1 and rgb[y, x, 0] > 0 and rgb[y, x, 1] == 0  # the sphere's red, none of the plane's green
    origin, direction = oracle.primary_ray(case.pod(), W, H, x, y)
    distance, kind, _, _ = oracle.closest_hit(case.pod(), [origin], [direction])
    assert kind[0] == 1 and distance[0] == np.float32(3.99)


def test_the_material_extremes_send_what_they_claim_to_the_pack():
    """Summed over the material cases: NaN, negative, infinite and > 1 means; an index of refraction of exactly 1; total internal
    reflection; metal that absorbs most bounces (roughness 5) and metal that absorbs none of its own (roughness 0)."""
    total = dict.fromkeys(oracle.CENSUS_EVENTS, 0)
    nan_pixels = negative = infinite = 0
    for case in rc.extreme_cases():
        for sm in case.tables:
            _, rgb, _, counts = rc.census(case.name, sm)
            for event, count in counts.items():
                total[event] += count
            nan_pixels += int(np.isnan(rgb).any(axis=-1).sum())
            negative += int((rgb < 0).sum())
            infinite += int(np.isinf(rgb).sum())
    for event in ("pack_clamped_above", "pack_negative_or_nan", "pack_non_finite", "dielectric_index_one", "dielectric_total_internal", "metal_absorbed", "metal_scattered"):
        assert total[event] > 0, event
    assert nan_pixels > 0 and negative > 0 and infinite > 0
    rough = rc.census("metal_roughness_5", False)[3]
    smooth = rc.census("metal_roughness_0", False)[3]
    assert rough["metal_absorbed"] > smooth["metal_absorbed"]


# ---- the invariant ---------------------------------------------------------------------------------------------------------------------
def existing_reach():
    """profiles/r18/branch_census.txt: event -> how many of the frames the GPU parity suite renders reach it."""
    table = {}
    for line in (ROOT / "profiles" / "r18" / "branch_census.txt").read_text().splitlines():
        if line and not line.startswith("#"):
            event, frames, _ = line.split()
            table[event] = int(frames)
    return table


def test_every_census_event_is_reached_by_a_constructed_case_or_by_a_frame_the_suite_renders():
    table = existing_reach()
    assert list(table) == oracle.CENSUS_EVENTS, "profiles/r18/branch_census.txt is not of this census: run tools/branch_census.py"
    constructed = dict.fromkeys(oracle.CENSUS_EVENTS, 0)
    for name, sm in rc.CASE_TABLES:
        for event, count in rc.census(name, sm)[3].items():
            constructed[event] += count > 0
    unreached = [event for event in oracle.CENSUS_EVENTS if table[event] == 0 and constructed[event] == 0]
    assert not unreached, f"no frame of the suite reaches: {', '.join(unreached)}"
    # what this file is for: the events the existing frames never reach are reached by constructed cases
    for event in ("redraw", "zero_jitter", "lambert_rule", "lambert_near_zero"):
        assert table[event] == 0 and constructed[event] > 0, (event, table[event], constructed[event])
