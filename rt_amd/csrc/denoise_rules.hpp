// rt_amd/csrc/denoise_rules.hpp — the per-element rules of the guide-buffer denoiser, written ONCE so that hipcc
// and g++ both compile them: the kernels of denoise.hip run this text per pixel, tests/native/denoise_reference.cpp restates the whole
// filter serially over the very same functions, and the device's result must equal that restatement bit for bit.
//
// What makes that possible: the filter is defined with + - x, correctly rounded '/', compare-and-select and the contract's dot()
// only — no exp, no pow, no other transcendental — both compilers are told not to contract (-ffp-contract=off), and every sum is a
// plain sequential add in ONE order: dy from -2 to 2 outside, dx from -2 to 2 inside.  Tiling (denoise.hip) is an implementation
// matter of how a tap is FETCHED; it reaches nothing below.
//
// The leaf functions come from whoever includes this header, in namespace rt_hip::denoise::leaf, BEFORE the inclusion:
//     float    dot3(float ax, float ay, float az, float bx, float by, float bz)   the contract's dot(): fma(az, bz, fma(ay, by, ax * bx))
//     float    sqrt_rn(float)                                                       the correctly rounded square root
//     uint32_t pack(float r, float g, float b)                                      clamp to [0, 1] and pack RGBA8888
// denoise.hip hands in contract.hpp's own (dot, sqrt_rn, pack_rgba8888), the CPU restatement the oracle's own (oracle/cpu_ref.cpp):
// none of them is restated here.
#pragma once

#include <stdint.h>
#include "../../include/rt_hip.h" // (rt_hip_denoise_params, rt_hip_status)

#if defined(__HIPCC__)
#define RT_HIP_DENOISE_FN __device__ __forceinline__
#else
#define RT_HIP_DENOISE_FN inline
#endif

namespace rt_hip
{
namespace denoise
{
	constexpr uint32_t max_iterations = 6;		 // taps up to 2 * 2^5 = 64 pixels away
	constexpr uint32_t max_normal_squarings = 8; // (n_p . n_q)^256
	constexpr uint32_t guide_words = 8;			 // per pixel: two float4s

	// The guide record of a pixel: the first hit of the path tracer's sample-0 primary ray (the pixel centre), 8 words.
	//   nx, ny, nz   the hit normal as the tracer computes it (not flipped toward the ray); 0, 0, 0 for sky
	//   depth        the accepted hit distance; -1 for sky (the reference's hit_result convention)
	//   ar, ag, ab   a hit: the attenuation the tracer uses (albedo * reflectivity, the derived per-primitive table); a miss: the sky
	//                colour of the centre ray (mg_ray_tracer.cpp:164)
	//   id           0 = sky, else 1 + the global primitive index of the derived tables (spheres, planes, boxes)
	struct guide
	{
		float nx, ny, nz, depth;
		float ar, ag, ab;
		uint32_t id;
	};
	struct rgb
	{
		float r, g, b;
	};
	struct tap
	{
		guide g;
		rgb c;
	};

	RT_HIP_DENOISE_FN uint32_t bits_of(float f) { return __builtin_bit_cast(uint32_t, f); }
	RT_HIP_DENOISE_FN float float_of(uint32_t u) { return __builtin_bit_cast(float, u); }
	RT_HIP_DENOISE_FN bool is_finite(float f) { return (bits_of(f) & 0x7F800000u) != 0x7F800000u; }
	RT_HIP_DENOISE_FN bool is_finite(rgb c) { return is_finite(c.r) && is_finite(c.g) && is_finite(c.b); }

	// what one iteration derives from the parameters: the tap spacing 2^i and the squared widths
	struct pass_constants
	{
		int32_t step;			   // 2^i
		uint32_t normal_squarings;
		float sigma_depth;
		float sigma_albedo2;	   // sigma_albedo^2
		float sigma_colour2;	   // (sigma_colour * 2^-i)^2: the colour term tightens as the footprint widens
	};
	RT_HIP_DENOISE_FN pass_constants constants_of(const rt_hip_denoise_params& p, uint32_t iteration)
	{
		const float narrowed = p.sigma_colour * float_of((127u - iteration) << 23); // (x 2^-i: exact)
		return { static_cast<int32_t>(1u << iteration), p.normal_squarings, p.sigma_depth, p.sigma_albedo * p.sigma_albedo, narrowed * narrowed };
	}

	// the B3 spline (3/8, 1/4, 1/16) at |offset| in taps
	RT_HIP_DENOISE_FN float spline(int32_t a) { return a == 0 ? 0.375f : (a == 1 ? 0.25f : 0.0625f); }

	// The weight of neighbour q for centre p, a product in a fixed order: spline, normal, depth, albedo, colour.
	//   * sky against hit: 0.  Sky against sky: the spline and the colour term only.
	//   * a tap whose colour has a non-finite channel: 0.
	//   * a weight that comes out as NaN (two hits at an infinite distance: inf - inf) counts as 0 as well.
	// All by select: both sides evaluate every term and pick.
	RT_HIP_DENOISE_FN float tap_weight(const tap& p, const tap& q, int32_t adx, int32_t ady, const pass_constants& k)
	{
		const bool sky_p = p.g.id == 0u, sky_q = q.g.id == 0u;
		const bool hits = !sky_p && !sky_q;
		float w = spline(adx) * spline(ady);

		const float along = leaf::dot3(p.g.nx, p.g.ny, p.g.nz, q.g.nx, q.g.ny, q.g.nz);
		float wn = along > 0.0f ? along : 0.0f;
		for (uint32_t s = 0; s < k.normal_squarings; s++)
			wn = wn * wn;
		w = w * (hits ? wn : 1.0f);

		const float deeper = p.g.depth > q.g.depth ? p.g.depth : q.g.depth;
		const float rz = (p.g.depth - q.g.depth) / (k.sigma_depth * deeper);
		const float wz = 1.0f / (1.0f + rz * rz);
		w = w * (hits ? wz : 1.0f);

		const float dar = p.g.ar - q.g.ar, dag = p.g.ag - q.g.ag, dab = p.g.ab - q.g.ab;
		const float wa = 1.0f / (1.0f + leaf::dot3(dar, dag, dab, dar, dag, dab) / k.sigma_albedo2);
		w = w * (hits ? wa : 1.0f);

		const float dr = p.c.r - q.c.r, dg = p.c.g - q.c.g, db = p.c.b - q.c.b;
		const float wc = 1.0f / (1.0f + leaf::dot3(dr, dg, db, dr, dg, db) / k.sigma_colour2);
		w = w * wc;

		const bool usable = (sky_p == sky_q) && is_finite(q.c) && w == w;
		return usable ? w : 0.0f;
	}

	// The pixel rule: out = (sum of w c_q) / (sum of w) over the 5 x 5 taps at (dx, dy) * step, taps outside the frame skipped.
	//   * the centre tap has no edge-stopping terms: its weight is 9/64 by select, so the denominator is positive
	//   * a centre with a non-finite channel passes through unchanged
	// fetch(x, y) returns the tap record of a pixel INSIDE the frame; how (LDS tile, global memory, a plain array) is the caller's.
	template <typename Fetch>
	RT_HIP_DENOISE_FN rgb filter_pixel(int32_t x, int32_t y, int32_t width, int32_t height, const pass_constants& k, const Fetch& fetch)
	{
		const tap p = fetch(x, y);
		if (!is_finite(p.c))
			return p.c;
		float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
		for (int32_t dy = -2; dy <= 2; dy++)
			for (int32_t dx = -2; dx <= 2; dx++)
			{
				const int32_t qx = x + dx * k.step, qy = y + dy * k.step;
				if (qx < 0 || qx >= width || qy < 0 || qy >= height)
					continue;
				const tap q = fetch(qx, qy);
				const bool centre = dx == 0 && dy == 0;
				const float edge = tap_weight(p, q, dx < 0 ? -dx : dx, dy < 0 ? -dy : dy, k);
				const float w = centre ? 0.140625f : edge;
				const bool finite = is_finite(q.c); // (a weight of 0 must not meet an infinity)
				const rgb c = { finite ? q.c.r : 0.0f, finite ? q.c.g : 0.0f, finite ? q.c.b : 0.0f };
				sw = sw + w;
				sr = sr + w * c.r;
				sg = sg + w * c.g;
				sb = sb + w * c.b;
			}
		return { sr / sw, sg / sw, sb / sw };
	}

	// from a (filtered) mean to RGBA8888: the path tracer's own finish — square root "gamma", clamp, pack (mg_ray_tracer.cpp:196-200)
	RT_HIP_DENOISE_FN uint32_t finish(rgb mean) { return leaf::pack(leaf::sqrt_rn(mean.r), leaf::sqrt_rn(mean.g), leaf::sqrt_rn(mean.b)); }
}
}
