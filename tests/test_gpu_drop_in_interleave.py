"""The six single-context drop-in calls run through shared host code (rt_amd/csrc/frame_call.hip) and share a context's
stream, module-owned frame, float staging and stats.  Here: the calls of all features interleaved on one context against the same calls
feature by feature on a second one — every packed frame, float image, sample map, info block and work count equal, word for word.  The
library is compared with itself only.  And what rt_hip_stats_fetch reports behind a temporal and an upscaled frame that kept no stats,
and behind one that kept them by RT_HIP_FLAG_STATS alone."""
import numpy as np
import pytest

import rt_amd
from rt_amd import capi

pytestmark = pytest.mark.gpu

W, H, SPP, PASS, SEED = 64, 36, 32, 16, 7
COUNTS = ("segments", "primary_samples", "kernel_variant")


def pod():
    return rt_amd.Scene.named("basic").set_sampling(SPP).describe(W, H)


def calls(t):
    """label -> the call on tracer `t`; every one asks for the float image where the call has one, and for stats."""
    p = pod()
    return {
        "render": lambda: t.render(p, W, H, seed=SEED, want_rgb=True),
        "temporal 1": lambda: t.render_temporal(p, W, H, seed=SEED, want_rgb=True),
        "temporal 2": lambda: t.render_temporal(p, W, H, seed=SEED + 1, want_rgb=True),
        "progressive 1": lambda: t.render_progressive(p, W, H, seed=SEED, pass_samples=PASS, want_rgb=True),
        "progressive 2": lambda: t.render_progressive(p, W, H, seed=SEED, pass_samples=PASS, want_rgb=True),
        "progressive kept": lambda: t.render_progressive(p, W, H, seed=SEED, pass_samples=PASS, want_rgb=True),
        "denoise": lambda: t.denoise_progressive(want_rgb=True)[:2],  # (its third value is a time)
        "upscaled": lambda: t.render_upscaled(p, W, H, seed=SEED, factor=2, want_rgb=True),
        "adaptive 1": lambda: t.render_adaptive(p, W, H, seed=SEED, pass_samples=PASS, want_rgb=True),
        "adaptive 2": lambda: t.render_adaptive(p, W, H, seed=SEED, pass_samples=PASS, want_rgb=True),
    }


INTERLEAVED = ["render", "temporal 1", "progressive 1", "upscaled", "adaptive 1", "denoise", "progressive 2", "temporal 2", "adaptive 2", "progressive kept"]
ALONE = ["render", "temporal 1", "temporal 2", "progressive 1", "denoise", "progressive 2", "progressive kept", "upscaled", "adaptive 1", "adaptive 2"]


def run(order):
    with rt_amd.HipRayTracer(device=0) as t:
        todo = calls(t)
        return {label: todo[label]() for label in order}


def assert_same(label, a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"{label}: {x.dtype} image differs in {(x.view(np.uint32) != y.view(np.uint32)).sum()} words"
        elif "render_ms" in x:  # the stats: the work counts (the times are the run's own)
            assert {k: x[k] for k in COUNTS} == {k: y[k] for k in COUNTS}, label
        else:  # rt_hip_progress, rt_hip_temporal_info, rt_hip_upscale_info, rt_hip_adaptive_info
            assert x == y, label


def test_interleaved_calls_are_the_calls_alone():
    assert sorted(INTERLEAVED) == sorted(ALONE)
    a, b = run(INTERLEAVED), run(ALONE)
    for label in INTERLEAVED:
        assert_same(label, a[label], b[label])
    # the sequence did what its labels say: two passes complete the frame, the third call launches nothing; the history is carried
    assert [a[k][3] for k in ("progressive 1", "progressive 2", "progressive kept")] == [
        {"samples_done": 16, "samples_total": SPP, "passes": 1, "restarted": 1},
        {"samples_done": 32, "samples_total": SPP, "passes": 2, "restarted": 0},
        {"samples_done": 32, "samples_total": SPP, "passes": 2, "restarted": 0},
    ]
    assert a["progressive kept"][2]["kernel"] == "none" and np.array_equal(a["progressive kept"][0], a["progressive 2"][0])
    assert np.array_equal(a["progressive 2"][0], a["render"][0])  # (the one-shot frame, bit for bit)
    assert a["temporal 1"][3]["restarted"] == 1 and a["temporal 2"][3]["restarted"] == 0 and a["temporal 2"][3]["frames"] == 2 and a["temporal 2"][3]["pixels_with_history"] > 0
    assert a["adaptive 1"][4]["passes"] == 1 and a["adaptive 2"][4]["passes"] == 2 and a["adaptive 2"][4]["restarted"] == 0
    assert a["upscaled"][3]["low_width"] == W // 2 and a["upscaled"][3]["low_height"] == H // 2
    assert rt_amd.live_frame_locks() == 0


@pytest.mark.parametrize("call", ["render_temporal", "render_upscaled"])
def test_stats_fetch_behind_a_staged_frame(call):
    """Without a stats pointer and without RT_HIP_FLAG_STATS nothing is timed or counted, and nothing stale is reported; with the flag
    alone the frame's device time is there to fetch."""
    with rt_amd.HipRayTracer(device=0) as t:
        frame = getattr(t, call)
        frame(pod(), W, H, seed=SEED, stats=True)  # (a frame that leaves figures behind)
        assert t.stats()["render_ms"] > 0.0 and t.stats()["segments"] > 0
        frame(pod(), W, H, seed=SEED + 1, stats=False)
        kept = t.stats()
        assert kept["render_ms"] == 0.0 and kept["segments"] == 0 and kept["readback_ms"] == 0.0, kept
        frame(pod(), W, H, seed=SEED + 2, flags=capi.RT_HIP_FLAG_STATS, stats=False)
        assert t.stats()["render_ms"] > 0.0
