// rt_amd/csrc/bloom_rules.hpp — the per-element rules of bloom, written ONCE so that hipcc and g++ both compile
// them: the four kernels of bloom.hip run this text, tests/native/bloom_reference.cpp restates the whole pyramid serially over the
// very same functions, and the device's result must equal that restatement bit for bit.
//
// What makes that possible: + - x, correctly rounded '/', compare-and-select, in ONE stated order, no contraction (-ffp-contract=off
// on both compilers) and no log, exp or pow anywhere.  Every tap rule takes its operands in a fixed order and every texel is computed
// by exactly one lane from values that were complete before its launch began: no sum depends on who arrives first.
//
// Nothing here touches memory: a rule is handed the values, an index rule gives the place to fetch them from.  The kernels and the
// restatement differ only in how the values reach the rules (LDS tiles there, plain arrays here).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define RT_HIP_BLOOM_FN __host__ __device__ __forceinline__
#else
#define RT_HIP_BLOOM_FN inline
#endif

namespace rt_hip
{
namespace bloom
{
	constexpr uint32_t max_levels = 8;
	constexpr float cap = 1048576.0f; // 2^20: what a channel is held to on its way into the bright pass

	struct rgb
	{
		float r, g, b;
	};

	// ---- sizes and indices ------------------------------------------------------------------------------------------------------------
	// the next level's side: ceil(n / 2); level 0 is that of the frame's
	RT_HIP_BLOOM_FN uint32_t half_up(uint32_t n) { return (n + 1u) >> 1; }
	// an index held to 0 .. n - 1 (n >= 1)
	RT_HIP_BLOOM_FN uint32_t clamp_index(int32_t i, uint32_t n) { return i < 0 ? 0u : (static_cast<uint32_t>(i) < n ? static_cast<uint32_t>(i) : n - 1u); }
	// the prefilter's source pixel: min(2 X + d, n - 1), d = 0 or 1
	RT_HIP_BLOOM_FN uint32_t quad_index(uint32_t X, uint32_t d, uint32_t n)
	{
		const uint32_t i = 2u * X + d;
		return i < n ? i : n - 1u;
	}
	// the tent's second tap for the fine index x over a coarse level of n: the neighbour of X = x >> 1 on x's side, held to the level
	RT_HIP_BLOOM_FN uint32_t tent_neighbour(uint32_t x, uint32_t n)
	{
		const uint32_t X = x >> 1;
		return (x & 1u) ? (X + 1u < n ? X + 1u : n - 1u) : (X > 0u ? X - 1u : 0u);
	}

	// ---- the bright pass --------------------------------------------------------------------------------------------------------------
	RT_HIP_BLOOM_FN float max_of(float a, float b) { return a > b ? a : b; }
	RT_HIP_BLOOM_FN float min_of(float a, float b) { return a < b ? a : b; }
	// NaN, negatives and zeros go in as 0, everything from 2^20 (+inf too) as 2^20: one bad pixel never spreads
	RT_HIP_BLOOM_FN float sanitise(float c) { return (c == c && c > 0.0f) ? min_of(c, cap) : 0.0f; }

	// What of a pixel is bright: every sanitised channel times scale = w / m, m the largest channel, w how far m lies above the threshold,
	// with a quadratic knee of half-width `knee` below it:
	//   rq = clamp(m - (threshold - knee), 0, 2 knee)     soft = knee > 0 ? rq rq / (4 knee) : 0     w = max(max(soft, m - threshold), 0)
	// knee <= threshold (the parameter check) gives w <= m, so scale <= 1 (DESIGN.md §3.16 has the proof); m = 0 gives scale 0.
	RT_HIP_BLOOM_FN rgb bright(float r, float g, float b, float threshold, float knee)
	{
		const float sr = sanitise(r), sg = sanitise(g), sb = sanitise(b);
		const float m = max_of(sr, max_of(sg, sb));
		const float rq = min_of(max_of(m - (threshold - knee), 0.0f), 2.0f * knee);
		const float soft = knee > 0.0f ? (rq * rq) / (4.0f * knee) : 0.0f;
		const float w = max_of(max_of(soft, m - threshold), 0.0f);
		const float scale = m > 0.0f ? w / m : 0.0f;
		return { sr * scale, sg * scale, sb * scale };
	}

	// ---- the three tap rules, per channel ---------------------------------------------------------------------------------------------
	// prefilter: the 2 x 2 box of bright pixels, b<dx><dy>
	RT_HIP_BLOOM_FN float box4(float b00, float b10, float b01, float b11) { return ((b00 + b10) + (b01 + b11)) * 0.25f; }
	// down: the binomial 1 4 6 4 1 over five taps a b c d e, unnormalised; rows first, then the same over five row sums, then x 1 / 256
	RT_HIP_BLOOM_FN float binomial5(float a, float b, float c, float d, float e) { return ((a + e) + 4.0f * (b + d)) + 6.0f * c; }
	RT_HIP_BLOOM_FN float down_finish(float v) { return v * 0.00390625f; }
	// up and composite: the tent over a texel and its neighbour; rows first (near, far along x), then the same over the two rows
	RT_HIP_BLOOM_FN float tent2(float near, float far) { return 0.75f * near + 0.25f * far; }

	RT_HIP_BLOOM_FN rgb box4(rgb b00, rgb b10, rgb b01, rgb b11) { return { box4(b00.r, b10.r, b01.r, b11.r), box4(b00.g, b10.g, b01.g, b11.g), box4(b00.b, b10.b, b01.b, b11.b) }; }
	RT_HIP_BLOOM_FN rgb tent2(rgb near, rgb far) { return { tent2(near.r, far.r), tent2(near.g, far.g), tent2(near.b, far.b) }; }
	// up[i] = level[i] + scatter x tent(up[i + 1])
	RT_HIP_BLOOM_FN rgb up_sum(rgb level, float scatter, rgb tent) { return { level.r + scatter * tent.r, level.g + scatter * tent.g, level.b + scatter * tent.b }; }
	// out = in + gain x layer: `in` as it is — a NaN stays a NaN, and is the only one
	RT_HIP_BLOOM_FN rgb composite(rgb in, float gain, rgb layer) { return { in.r + gain * layer.r, in.g + gain * layer.g, in.b + gain * layer.b }; }
}
}
