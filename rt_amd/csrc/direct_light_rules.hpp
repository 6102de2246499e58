// rt_amd/csrc/direct_light_rules.hpp — the vertex rule of RT_HIP_FLAG_DIRECT_LIGHT, written ONCE so that hipcc and
// g++ both compile it: the direct builds of render_queue (kernels.hip) run this text per aiming lane, tests/native/direct_reference.cpp
// restates the trace loop on the CPU over the very same functions, and the device's frames must equal that restatement bit for bit.
//
// What it holds: the choice of the light from a draw, the octahedral map from two draws to a direction on the light, the side rule
// (a vertex outside the light samples the hemisphere that faces it, a vertex inside the whole sphere), the point on the light, the
// shadow direction and the estimator's weight.  What it does NOT hold: the generator, the closest-hit query and the light list — the
// callers' — and the contract's reciprocal square root, which the caller hands in (contract.hpp's inv_sqrt_rn on the device, the
// oracle's inv_sqrt on the CPU: the same function bit for bit, tests/test_gpu_parity.py).
//
// THIS IS NOT A LOWER-VARIANCE WAY TO THE RT_HIP_FLAG_EMISSION IMAGE.  The contract's lambert scatter inherits the reference's
// positive-octant random_unit_vector, so the implicit estimator's direct light is skewed; the sampled direct term below is the
// physically standard one.  The two frames converge to DIFFERENT images wherever a sampled light illuminates lambert surfaces, and no
// test may compare their means.  Nothing here promises anything about speed either.
//
// The arithmetic is + - x, fused multiply-adds ONLY where RT_HIP_DIRECT_FMA is written, correctly rounded '/' and square root,
// compare-and-select; both compilers are told not to contract (-ffp-contract=off) and every operation stands in ONE order:
//   u = ka * 2^-23 - 1, v = kb * 2^-23 - 1               exact (ka, kb < 2^24)
//   z = (1 - |u|) - |v|                                  exact (multiples of 2^-23 of magnitude <= 2)
//   z < 0: (u, v) = ((1 - |v|) * sgn(u), (1 - |u|) * sgn(v)), sgn(0) = +1, from the OLD u and v
//   l2 = dot(p, p) = fma(z, z, fma(v, v, u * u))         the contract's dot; omega = p * inv_sqrt(l2)
//   d0 = x - C; inside = dot(d0, d0) < R * R; outside and dot(omega, d0) < 0: omega = -omega
//   y = fma(R, omega, C); t = y - x; d2 = dot(t, t); w = t * inv_sqrt(d2)
//   cx = dot(nrm, w); cy = inside ? dot(omega, w) : -dot(omega, w)
//   weight = (((cx * cy) * (R * R)) * (float(n) * (inside ? 4 : 2))) / ((pi * d2) * (l2 * sqrt(l2))),   pi = 0x1.921fb6p+1f
//   aimed = cx > 0 && cy > 0 && d2 > 0 && |weight| <= FLT_MAX   (every comparison false for a NaN: a NaN aims at nothing)
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define RT_HIP_DIRECT_FN __host__ __device__ __forceinline__
#else
#define RT_HIP_DIRECT_FN inline
#endif
#define RT_HIP_DIRECT_FMA(a, b, c) __builtin_fmaf((a), (b), (c))

namespace rt_hip
{
namespace direct_light
{
	constexpr uint32_t max_sampled_lights = 256; // L = (kc * n) >> 24 in 32 bits: kc < 2^24, n <= 2^8
	constexpr float pi = 0x1.921fb6p+1f;
	constexpr float largest_finite = 0x1.fffffep+127f;

	// which of the n sampled lights (1 <= n <= max_sampled_lights) a vertex aims at: kc is the step's third numerator
	RT_HIP_DIRECT_FN uint32_t choose_light(uint32_t kc, uint32_t n) { return (kc * n) >> 24; }

	template <class V>
	RT_HIP_DIRECT_FN float dot3(V a, V b)
	{
		return RT_HIP_DIRECT_FMA(a.z, b.z, RT_HIP_DIRECT_FMA(a.y, b.y, a.x * b.x));
	}

	// the octahedral map: the point p of |x| + |y| + |z| = 1 of the numerators (ka, kb) and l2 = dot(p, p) (>= 1/3: never zero).
	// Normalised, p has the density |p|^3 / 4 per unit solid angle.
	template <class V>
	RT_HIP_DIRECT_FN V octahedral_point(uint32_t ka, uint32_t kb, float& l2)
	{
		const float u = static_cast<float>(ka) * 0x1.0p-23f - 1.0f;
		const float v = static_cast<float>(kb) * 0x1.0p-23f - 1.0f;
		const float au = __builtin_fabsf(u), av = __builtin_fabsf(v);
		const float z = (1.0f - au) - av;
		const bool folded = z < 0.0f;
		const float fu = (1.0f - av) * (u < 0.0f ? -1.0f : 1.0f);
		const float fv = (1.0f - au) * (v < 0.0f ? -1.0f : 1.0f);
		V p;
		p.x = folded ? fu : u;
		p.y = folded ? fv : v;
		p.z = z;
		l2 = dot3(p, p);
		return p;
	}

	template <class V>
	struct aim
	{
		V w;		  // the shadow ray's direction, normalised (meaningful where `aimed` holds)
		float weight; // what the light's emission, times throughput * attenuation, is multiplied by if the light is visible
		bool aimed;	  // false: no shadow segment, nothing is added
	};

	// The vertex rule from the two numerators to the shadow direction and the weight, for the light (C, R) of n sampled lights, at the
	// point x with the hit's stored normal nrm (not flipped).  inv_sqrt is the contract's reciprocal square root.
	template <class V, class InvSqrt>
	RT_HIP_DIRECT_FN aim<V> aim_at(uint32_t ka, uint32_t kb, V x, V nrm, V C, float R, uint32_t n, InvSqrt inv_sqrt)
	{
		float l2;
		const V p = octahedral_point<V>(ka, kb, l2);
		const float inv_p = inv_sqrt(l2);
		V omega;
		omega.x = p.x * inv_p, omega.y = p.y * inv_p, omega.z = p.z * inv_p;
		V d0;
		d0.x = x.x - C.x, d0.y = x.y - C.y, d0.z = x.z - C.z;
		const bool inside = dot3(d0, d0) < R * R;
		const bool flip = !inside && dot3(omega, d0) < 0.0f;
		omega.x = flip ? -omega.x : omega.x, omega.y = flip ? -omega.y : omega.y, omega.z = flip ? -omega.z : omega.z;
		V t;
		t.x = RT_HIP_DIRECT_FMA(R, omega.x, C.x) - x.x, t.y = RT_HIP_DIRECT_FMA(R, omega.y, C.y) - x.y, t.z = RT_HIP_DIRECT_FMA(R, omega.z, C.z) - x.z;
		const float d2 = dot3(t, t);
		const float inv_t = inv_sqrt(d2);
		aim<V> a;
		a.w.x = t.x * inv_t, a.w.y = t.y * inv_t, a.w.z = t.z * inv_t;
		const float cx = dot3(nrm, a.w);
		const float ow = dot3(omega, a.w);
		const float cy = inside ? ow : -ow;
		const float numerator = ((cx * cy) * (R * R)) * (static_cast<float>(n) * (inside ? 4.0f : 2.0f));
		const float denominator = (pi * d2) * (l2 * __builtin_sqrtf(l2));
		a.weight = numerator / denominator;
		a.aimed = cx > 0.0f && cy > 0.0f && d2 > 0.0f && __builtin_fabsf(a.weight) <= largest_finite;
		return a;
	}
}
}
