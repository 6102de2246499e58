"""RT_HIP_FLAG_FAST's three hardware approximations, MEASURED: contract.hpp's fast sqrt_rn (v_sqrt_f32), rcp_rn (v_rcp_f32), inv_sqrt_rn
(v_rsq_f32) and divide (a * v_rcp_f32(b)), compiled as the fast build of the kernels compiles them (rt_amd/csrc/kat_fast.hip), against
binary64 on the host.

"About 1 ulp" in contract.hpp is what the per-pixel rule of tests/fast_cases.py rests on: its stand-ins for a FAST frame are runs perturbed
by S and S / 2 ulps.  This file ties S to the device: every measured leaf error must be at most S / 2 ulps.  Errors are in float32 ulps
of the exact result's binade, |got - exact| / 2^(floor(log2 |exact|) - 23), and are printed."""
import numpy as np
import pytest

from tests import fast_cases as cases

pytestmark = pytest.mark.gpu

BOUND = cases.S / 2.0
F32 = np.float32


def ulps(got, exact):
    """|got - exact| in float32 ulps of exact's binade (exact: float64, finite, non-zero, a normal float32 in size)"""
    _, exponent = np.frexp(np.abs(exact))
    return np.abs(got.astype(np.float64) - exact) / np.ldexp(1.0, exponent - 24)


def every_significand(exponent_bits):
    return (np.uint32(exponent_bits) + np.arange(1 << 23, dtype=np.uint32)).view(F32)


def worst(name, got, exact, x):
    error = ulps(got, exact)
    at = int(np.argmax(error))
    print(f"  {name}: largest error {error.max():.4f} ulps at x = {float(x[at])!r} ({x[at : at + 1].view(np.uint32)[0]:#010x}), mean {error.mean():.4f}")
    return float(error.max())


@pytest.mark.parametrize("exponent_bits", [0x3F800000, 0x40000000], ids=["[1,2)", "[2,4)"])
def test_every_significand_of_two_adjacent_exponents(tracer, exponent_bits):
    """sqrt and the reciprocal square root over an even and an odd exponent (every other binade repeats one of them but for the scale); the
    reciprocal over one (its error does not depend on the exponent's parity); divide by every significand of a random numerator."""
    x = every_significand(exponent_bits)
    numerator = np.random.default_rng(exponent_bits).uniform(1.0, 2.0, x.size).astype(F32)
    _, _, _, quotient = tracer.kat_fast_math(numerator, x)
    worst_quotient = worst("divide(a, x)", quotient, numerator.astype(np.float64) / x.astype(np.float64), x)
    root, reciprocal, inverse_root, _ = tracer.kat_fast_math(x, x)
    x64 = x.astype(np.float64)
    print(f"x in {('[1, 2)' if exponent_bits == 0x3F800000 else '[2, 4)')}, all 2^23 significands:")
    errors = {"sqrt_rn": worst("sqrt_rn", root, np.sqrt(x64), x), "inv_sqrt_rn": worst("inv_sqrt_rn", inverse_root, 1.0 / np.sqrt(x64), x), "rcp_rn": worst("rcp_rn", reciprocal, 1.0 / x64, x), "divide": worst_quotient}
    for name, error in errors.items():
        assert error <= BOUND, f"{name}: {error} ulps measured, and the stand-ins of tests/fast_cases.py assume at most S / 2 = {BOUND}: S and A have to grow (see its docstring)"


def test_random_inputs_across_the_exponent_range(tracer):
    """8192 random normal inputs whose results are normal too (the contract promises no range guard: see the next test), and divide on
    random pairs within 2^-30 .. 2^30."""
    rng = np.random.default_rng(20240)
    n = 8192
    bits = (rng.integers(1, 254, n, dtype=np.uint32) << np.uint32(23)) | rng.integers(0, 1 << 23, n, dtype=np.uint32)
    x = bits.astype(np.uint32).view(F32)  # positive, 2^-126 <= x < 2^127
    signed = np.where(rng.random(n) < 0.5, -x, x).astype(F32)
    a = (rng.choice([-1.0, 1.0], n) * np.exp2(rng.uniform(-30, 30, n))).astype(F32)
    b = (rng.choice([-1.0, 1.0], n) * np.exp2(rng.uniform(-30, 30, n))).astype(F32)
    root, _, inverse_root, _ = tracer.kat_fast_math(x, x)
    _, reciprocal, _, _ = tracer.kat_fast_math(signed, x)
    _, _, _, quotient = tracer.kat_fast_math(a, b)
    x64 = x.astype(np.float64)
    normal_reciprocal = x <= F32(2.0**126)  # 1 / x >= 2^-126
    print("random inputs over the exponent range:")
    errors = {
        "sqrt_rn": worst("sqrt_rn", root, np.sqrt(x64), x),
        "inv_sqrt_rn": worst("inv_sqrt_rn", inverse_root, 1.0 / np.sqrt(x64), x),
        "rcp_rn": worst("rcp_rn", reciprocal[normal_reciprocal], 1.0 / signed.astype(np.float64)[normal_reciprocal], signed[normal_reciprocal]),
        "divide": worst("divide(a, b)", quotient, a.astype(np.float64) / b.astype(np.float64), b),
    }
    assert np.array_equal(np.signbit(reciprocal), np.signbit(signed)) and np.array_equal(np.signbit(quotient), np.signbit(a) ^ np.signbit(b))
    for name, error in errors.items():
        assert error <= BOUND, f"{name}: {error} ulps measured against S / 2 = {BOUND}"


def test_zeros_infinities_and_nan_keep_sign_and_class_and_the_rest_is_recorded(tracer):
    """Zero, infinity and NaN: sign and class are asserted (what IEEE 754 and the ISA manual say of v_sqrt / v_rcp / v_rsq).  Subnormal and
    negative inputs, and reciprocals that would be subnormal: RECORDED in the output, not asserted — the fast contract has no range guard."""
    inf, nan = F32(np.inf), F32(np.nan)
    special = np.array([0.0, -0.0, inf, -inf, nan], dtype=F32)
    root, reciprocal, inverse_root, _ = tracer.kat_fast_math(special, np.ones_like(special))
    print("x: sqrt_rn, rcp_rn, inv_sqrt_rn")
    for row in zip(special, root, reciprocal, inverse_root):
        print("  " + ", ".join(repr(float(v)) for v in row))

    def same(got, want):
        want = np.array(want, dtype=F32)
        return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(want)].view(np.uint32), want[~np.isnan(want)].view(np.uint32))

    assert same(root, [0.0, -0.0, inf, nan, nan]), root
    assert same(reciprocal, [inf, -inf, 0.0, -0.0, nan]), reciprocal
    assert same(inverse_root, [inf, -inf, 0.0, nan, nan]), inverse_root
    recorded = np.array([1e-45, 1e-40, 1.1754942e-38, -1e-40, -1.0, -4.0, 2.0**127, -(2.0**127), 3.0e38], dtype=F32)
    root, reciprocal, inverse_root, quotient = tracer.kat_fast_math(recorded, np.full_like(recorded, 3.0))
    print("recorded, not asserted — x: sqrt_rn, rcp_rn, inv_sqrt_rn, divide(x, 3)")
    for row in zip(recorded, root, reciprocal, inverse_root, quotient):
        print("  " + ", ".join(repr(float(v)) for v in row))
