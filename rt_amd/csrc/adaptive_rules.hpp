// rt_amd/csrc/adaptive_rules.hpp — the per-pixel rules of adaptive sampling, written ONCE so that hipcc and g++ both
// compile them: adaptive_update of adaptive.hip runs this text per pixel (and per halo pixel), tests/native/adaptive_reference.cpp
// restates a whole update step serially over the very same functions, and the device's moments and state words must equal that
// restatement bit for bit.
//
// What makes that possible: the rule is + - x, correctly rounded '/', integer division, compare-and-select — nothing else, no leaf
// function from anywhere — both compilers are told not to contract (-ffp-contract=off), and every operation stands in ONE order.
// Every comparison is written so that a NaN means "not converged".
#pragma once

#include <stdint.h>
#include "../../include/rt_hip.h" // (rt_hip_adaptive_params)

#if defined(__HIPCC__)
#define RT_HIP_ADAPTIVE_FN __host__ __device__ __forceinline__
#else
#define RT_HIP_ADAPTIVE_FN inline
#endif

namespace rt_hip
{
namespace adaptive
{
	// the state word of a pixel: the samples its running sum holds in bits 0-30, "stopped" in bit 31
	constexpr uint32_t stopped_bit = 0x80000000u;
	constexpr uint32_t count_mask = 0x7FFFFFFFu;
	RT_HIP_ADAPTIVE_FN bool is_stopped(uint32_t state) { return (state & stopped_bit) != 0u; }
	RT_HIP_ADAPTIVE_FN uint32_t samples_of(uint32_t state) { return state & count_mask; }

	struct moments
	{
		float s1, s2; // sum and sum of squares of the passes' mean luminances y
	};
	struct pass_sum
	{
		float r, g, b; // the fold of ONE pass's chunk sums
	};
	// what one update leaves of a pixel
	struct update
	{
		moments m;
		uint32_t samples; // held after the pass
		bool converged;	  // the pixel's own verdict; whether it STOPS is its neighbourhood's (stops())
	};

	// The update of one pixel after a pass of `pass_samples` samples.
	//   first_pass  neither `before` nor `state` is read: the pixel holds nothing yet
	//   whole_pass  the pass traced the accumulation's pass size: the moments move and the pixel is judged.  A SHORT last pass (the
	//               rest up to the cap) counts its samples and nothing else: nobody converges in it.
	// A stopped pixel was not traced: it is kept as it is (`sum` is not read) and counts as converged.
	RT_HIP_ADAPTIVE_FN update update_pixel(pass_sum sum, moments before, uint32_t state, uint32_t pass_samples, bool first_pass, bool whole_pass, const rt_hip_adaptive_params& k)
	{
		update u;
		if (!first_pass && is_stopped(state))
		{
			u.m = before;
			u.samples = samples_of(state);
			u.converged = true;
			return u;
		}
		const uint32_t n = (first_pass ? 0u : samples_of(state)) + pass_samples;
		u.samples = n;
		if (!whole_pass)
		{
			u.m = first_pass ? moments{ 0.0f, 0.0f } : before;
			u.converged = false;
			return u;
		}
		const float y = ((sum.r + sum.g) + sum.b) / static_cast<float>(3u * pass_samples);
		const float yy = y * y;
		u.m.s1 = first_pass ? y : before.s1 + y;
		u.m.s2 = first_pass ? yy : before.s2 + yy;
		const uint32_t m = n / pass_samples;
		const float mean = u.m.s1 / static_cast<float>(m);
		const float product = u.m.s1 * mean;
		const float d = u.m.s2 - product;
		const float var = (d > 0.0f ? d : 0.0f) / static_cast<float>(m - 1u);
		const float se2 = var / static_cast<float>(m);
		float lim = k.threshold * (mean + k.floor);
		lim = lim * lim;
		u.converged = n >= k.min_samples && m >= 2u && se2 <= lim;
		return u;
	}

	// Whether the pixel at (x, y) of a width x height frame STOPS: it and its eight neighbours inside the frame are converged (a
	// neighbour outside the frame counts as converged).  `converged(qx, qy)` is asked for in-frame coordinates only.
	template <typename Converged>
	RT_HIP_ADAPTIVE_FN bool stops(int32_t x, int32_t y, int32_t width, int32_t height, Converged&& converged)
	{
		bool all = true;
		for (int32_t dy = -1; dy <= 1; dy++)
			for (int32_t dx = -1; dx <= 1; dx++)
			{
				const int32_t qx = x + dx, qy = y + dy;
				if (qx >= 0 && qx < width && qy >= 0 && qy < height)
					all = converged(qx, qy) && all;
			}
		return all;
	}

	// the state word an update and the 3x3 verdict leave (stopping is monotone: a stopped pixel's word is kept)
	RT_HIP_ADAPTIVE_FN uint32_t next_state(uint32_t state, bool first_pass, const update& u, bool stop)
	{
		if (!first_pass && is_stopped(state))
			return state;
		return u.samples | (stop ? stopped_bit : 0u);
	}
}
}
