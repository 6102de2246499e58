"""The rare branches through the sixteen light builds of render_queue on the GPU: every constructed case of tests/light_rare_cases.py —
under RT_HIP_FLAG_EMISSION the cases of tests/rare_cases.py with an inert lamp; under RT_HIP_FLAG_DIRECT_LIGHT the re-draw behind a
vertex that aimed and behind one that aimed at nothing, k drawn as the zero word, a metal first vertex, the second scatter, approx_zero
behind the shadow query and in the aiming trip, the zero jitter, the tie, the material extremes, the list's edges — under the mg and the
sm table, through every build the case can be steered to: the LDS scan of its camera form, the scalar-load scan (the padded scene), the
hierarchy over the host's tree and over the device builder's; each through rt_hip_render (a page-locked frame) and through
rt_hip_render_device (tensors).  Packed pixels and float mean as uint32, segments, primary_samples, kernel_variant: tolerance 0, against
oracle.render (emission cases: the lamp is inert) or tests/direct_reference.render — never against another GPU frame.

That a case DOES reach its branch is asserted on the CPU from the censuses (tests/test_light_rare_branches.py); nothing here is judged by
what the kernels return.  Before each frame the CPU plan dump (tests/light_plan.py) is asked which build the frame takes, and
kernel_variant is held to its answer; the last test holds what RAN to the coverage table (tests/light_rare_cases.coverage: all eight builds of each flag by the re-draw and the
approx_zero class; the scalar-load scan, the hierarchy and one LDS scan by every other class) and prints it."""
import pytest

from tests import light_plan
from tests import light_rare_cases as lrc
from tests.test_gpu_chunk_sweep import render_into_hbm
from tests.test_gpu_rare_branches import assert_same

pytestmark = pytest.mark.gpu

W, H = lrc.W, lrc.H
RAN = set()  # (flag, build, case class) of every frame this module compared


@pytest.fixture(autouse=True)
def _no_table_outlives_a_test(tracer):
    yield
    tracer.set_emission(None)  # (the session's context is shared: no other test file sees a table)


@pytest.mark.parametrize("name,sm", lrc.CASE_TABLES)
def test_every_case_through_every_build_it_reaches(tracer, name, sm):
    case = lrc.case(name)
    want_rgba, want_rgb, want_segments = lrc.reference(name, sm) if case.direct else lrc.base_reference(name, sm)
    table = case.table()
    tracer.set_emission(table)
    for what, flags, padded in lrc.runs_of(case, sm):
        pod = case.pod(padded)
        for host in (1, 0):
            plan = light_plan.planned(pod, table, W, H, flags, host)
            build = light_plan.build_name(plan)
            assert plan["refusal"] == "" and plan["direct"] == int(case.direct) and what.split(",")[0] in build, (name, what, plan)
            rgba, rgb, stats = tracer.render(pod, W, H, seed=case.seed, flags=flags, want_rgb=True) if host else render_into_hbm(tracer, pod, W, H, case.seed, flags)
            entry = "rt_hip_render" if host else "rt_hip_render_device"
            assert stats["kernel"] == light_plan.kernel_of(plan), (name, what, entry, stats["kernel"], build)
            assert_same(case, f"{what} -> {build}, {entry}", rgba, rgb, want_rgba, want_rgb)
            assert stats["segments"] == want_segments and stats["primary_samples"] == W * H * case.spp, (name, what, entry, stats, want_segments)
            RAN.add((case.flag, build, case.klass))


def test_what_ran_reaches_every_build(capsys):
    """Over the frames compared above (the module runs as a whole): exactly the (flag, build, class) triples the plan dump names for the
    parametrisation — nothing was skipped — and, for each flag, all eight builds reached by the re-draw and the approx_zero class, the
    scalar-load scan, the hierarchy and one LDS scan by every other class."""
    planned = set()
    for name, sm in lrc.CASE_TABLES:
        case = lrc.case(name)
        for _, flags, padded in lrc.runs_of(case, sm):
            for host in (1, 0):
                planned.add((case.flag, light_plan.build_name(light_plan.planned(case.pod(padded), case.table(), W, H, flags, host)), case.klass))
    assert RAN == planned, f"{len(planned - RAN)} (flag, build, class) triples of the parametrisation did not run (this test needs the whole module to have run)"
    table = lrc.coverage(RAN)
    with capsys.disabled():
        lrc.print_coverage(table)
