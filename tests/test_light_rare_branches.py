"""The rare branches under RT_HIP_FLAG_EMISSION and RT_HIP_FLAG_DIRECT_LIGHT, on the CPU: every constructed case of
tests/light_rare_cases.py reaches the branch it was built for.  For the emission cases that is the oracle's census of the lamp-less case,
which stands because the lamp scene's frame IS that case's frame, bit for bit; for the direct cases it is the census of
tests/direct_reference.py — the oracle's events under the direct trace loop, the restatement's own events, and the own events of the one
watched sample — and, where the branch is one of the two rare rules, the target pixel's float mean changes in bits when the rule is
switched off.  tests/test_gpu_light_rare_branches.py then holds the sixteen light builds to these frames.  Every precondition is asserted
here, from the CPU, never from a kernel.

Also here: the fixture of the extended event search (tests/golden/stream_events_direct.json) re-derived from oracle.random, and the
coverage table as the launch plan gives it: which of the sixteen builds each case class is steered to."""
import numpy as np
import pytest

from oracle import binding as oracle
from tests import light_plan
from tests import light_rare_cases as lrc
from tests import light_reference as light_ref
from tests import rare_cases as rc
from tools import find_stream_events as search

W, H = lrc.W, lrc.H
LIGHTS = [(name, sm) for name, sm in lrc.CASE_TABLES if not lrc.case(name).direct]
DIRECT = [(name, sm) for name, sm in lrc.CASE_TABLES if lrc.case(name).direct]


def holds(counts, expectations, what):
    for event, (relation, count) in expectations.items():
        assert (counts[event] == count) if relation == "==" else (counts[event] >= count), (*what, event, counts[event], relation, count)


# ---- the fixture of the extended search ------------------------------------------------------------------------------------------------
def test_every_recorded_event_of_the_new_fixture_draws_the_zero_word():
    assert len(lrc.direct_events_of(4)) >= 2 and len(lrc.direct_events_of(5)) >= 2
    for e in lrc.DIRECT_EVENTS:
        draws = oracle.random(e["seed"], e["pixel"], e["sample"], 3 * e["step"])
        assert (draws[-3:].view(np.uint32) == 0).all(), e
        assert (draws[:-3].reshape(-1, 3) != 0).any(axis=1).all(), e  # ... and no earlier step of the sample does
        assert e["width"] == W and 0 <= e["pixel"] < W * H and 0 < e["sample"] <= 40 and e["step"] in (4, 5)
        assert search.direct_kind_of(e["sample"], e["step"]) == e["kind"] and search.kind_of(e["sample"], e["step"]) is None


def test_the_extended_search_finds_what_the_new_fixture_records():
    """A thousand seeds around the first step-5 entry: the search finds it and nothing the fixture does not know; the search of the old
    fixture is what it was (tests/test_rare_branches.py)."""
    found = search.search(W, H, 40, 41000, 1000, max_step=5, kind_of=search.direct_kind_of)
    assert found == [e for e in lrc.DIRECT_EVENTS if 41000 <= e["seed"] < 42000] and len(found) == 1


# ---- RT_HIP_FLAG_EMISSION: the lamp is inert ---------------------------------------------------------------------------------------------
def test_every_case_of_rare_cases_has_its_lamp_case():
    bases = {c.base.name for c in lrc.all_cases() if not c.direct}
    assert bases >= {c.name for c in rc.all_cases()} and len(bases) == len(rc.all_cases()) + 4


@pytest.mark.parametrize("name,sm", LIGHTS)
def test_the_inert_lamp_changes_no_bit(name, sm):
    """light_ref.render of the lamp scene — and of the padded scene the scalar-load scan takes — is oracle.render of the lamp-less case:
    packed pixels, float mean, segments.  So no ray reaches lamp or padding, and the oracle's census of that case stands."""
    case = lrc.case(name)
    want_rgba, want_rgb, want_segments = lrc.base_reference(name, sm)
    assert case.table()[-1].min() > 0 and (case.table()[:-1] == 0).all() and case.pod().n_spheres == case.base.pod().n_spheres + 1 and case.pod(padded=True).n_spheres >= 40
    for padded in (False, True):
        rgba, rgb, segments = lrc.reference(name, sm, padded)
        assert rc.same_bits(rgb, want_rgb, nan_ok=case.nan_ok) and rgba.tobytes() == want_rgba.tobytes() and segments == want_segments, (name, sm, padded)
    if case.base.name in {c.name for c in rc.all_cases()}:
        assert want_rgb.tobytes() == rc.reference(case.base.name, sm)[1].tobytes()


@pytest.mark.parametrize("name,sm", [(n, sm) for n, sm in LIGHTS if "tilted" in n or "second_camera" in n])
def test_the_second_camera_cases_reach_their_branch(name, sm):
    """(the cases of tests/rare_cases.py proper are held by tests/test_rare_branches.py; these four are new)"""
    case = lrc.case(name)
    rgb, counts = lrc.base_census(name, sm)
    holds(counts, case.expect(sm), (name, sm))
    if case.sensitive:
        off_rgb, _ = lrc.base_census(name, sm, rare_rules=False)
        x, y = case.target_xy
        assert (off_rgb.view(np.uint32) != rgb.view(np.uint32)).any(axis=-1)[y, x]


def test_every_primary_ray_of_the_tilted_camera_hits_the_big_sphere():
    pod = lrc.case("direct_redraw_behind_aimed_vertex_tilted").pod()
    assert oracle.primary_ray(pod, W, H, 0, 0, want_form=True)[2] == "eye"
    rays = [oracle.primary_ray(pod, W, H, x, y, ka, kb) for x in range(W) for y in range(H) for ka in (0.0, 2.0**24 - 1) for kb in (0.0, 2.0**24 - 1)]
    _, kind, index, _ = oracle.closest_hit(pod, [r[0] for r in rays], [r[1] for r in rays])
    assert (kind == 1).all() and (index == 0).all()


# ---- RT_HIP_FLAG_DIRECT_LIGHT ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sm", DIRECT)
def test_every_direct_case_reaches_the_branch_it_claims(name, sm):
    case = lrc.case(name)
    rgba, rgb, segments = lrc.reference(name, sm)
    c_rgba, c_rgb, c_segments, counts, watched = lrc.census(name, sm)
    assert rgba.tobytes() == c_rgba.tobytes() and rgb.tobytes() == c_rgb.tobytes() and segments == c_segments  # the census frame is the reference
    p_rgba, p_rgb, p_segments = lrc.reference(name, sm, padded=True)  # ... and so is the padded scene's: the padding is inert
    assert rc.same_bits(p_rgb, rgb, nan_ok=case.nan_ok) and p_rgba.tobytes() == rgba.tobytes() and p_segments == segments
    assert case.pod().samples_per_pixel == case.spp <= 48 and 1 <= light_plan.light_counts(case.pod(), case.table())[1]
    holds(counts, case.expect(sm), (name, sm))
    if case.target is not None:
        holds(watched, case.watch(sm), (name, sm, "watched"))
        assert watched["first_vertex_aimed"] + watched["first_vertex_not_aimed"] + watched["light_on_primary"] <= 1
    if case.sensitive:  # with the two rare rules off, the target pixel is another number
        off_rgb = lrc.census(name, sm, rare_rules=False)[1]
        x, y = case.target_xy
        assert (off_rgb.view(np.uint32) != rgb.view(np.uint32)).any(axis=-1)[y, x], f"{name}: pixel ({x}, {y}) does not depend on the rule"


def test_the_flag_changes_the_frames_of_the_direct_cases():
    """(what makes them tests of the direct builds: without the flag the same scene under the same table is another frame)"""
    for name in ("direct_redraw_behind_aimed_vertex", "direct_approx_zero_exact_lamp_in_front", "direct_256_lamps_the_last_is_chosen", "direct_sphere_plane_tie"):
        case = lrc.case(name)
        _, implicit, _ = light_ref.render(case.pod(), W, H, case.table(), seed=case.seed)
        assert implicit.tobytes() != lrc.reference(name, False)[1].tobytes(), name


def test_the_material_extremes_reach_the_direct_sum_with_nan_and_infinite_throughputs():
    nan_pixels = infinite = aimed = 0
    for case in lrc.all_cases():
        if case.direct and case.klass == "extremes":
            for sm in case.tables:
                _, rgb, _, counts, _ = lrc.census(case.name, sm)
                nan_pixels += int(np.isnan(rgb).any(axis=-1).sum())
                infinite += int(np.isinf(rgb).sum())
                aimed += counts["vertex_aimed"]
    assert nan_pixels > 0 and infinite > 0 and aimed > 1000


# ---- coverage, as the launch plan gives it ----------------------------------------------------------------------------------------------
def test_every_build_is_reached_by_the_classes_it_must_be(capsys):
    """Asked of the plan dump for every frame tests/test_gpu_light_rare_branches.py renders (that module asserts each frame's
    kernel_variant against the same answer and the same table over what it ran)."""
    triples = set()
    for name, sm in lrc.CASE_TABLES:
        case = lrc.case(name)
        for what, flags, padded in lrc.runs_of(case, sm):
            for host in (1, 0):
                p = light_plan.planned(case.pod(padded), case.table(), W, H, flags, host)
                assert p["refusal"] == "" and p["direct"] == int(case.direct) and p["sm_table"] == int(sm) and what.split(",")[0] in light_plan.build_name(p), (name, what, p)
                triples.add((case.flag, light_plan.build_name(p), case.klass))
    table = lrc.coverage(triples)
    with capsys.disabled():
        lrc.print_coverage(table)
