// rt_amd/csrc/tonemap_rules.hpp — the per-element rules of tone mapping, written ONCE so that hipcc and g++ both
// compile them: the kernels of tonemap.hip run this text — per pixel for the histogram and the curve, once per frame for the
// exposure — tests/native/tonemap_reference.cpp restates the whole operation serially over the very same functions, and the
// device's result must equal that restatement bit for bit.
//
// What makes that possible: + - x, correctly rounded '/' and square root, compare-and-select, in ONE stated order, no contraction
// (-ffp-contract=off on both compilers) and no log, exp or pow anywhere: the meter's "log2" is the bit pattern of the luminance.
// The histogram is integers, so the order pixels arrive in cannot matter; what follows it is exact integer arithmetic up to one
// division of two floats.
//
// The leaf function comes from whoever includes this header, in namespace rt_hip::tonemap::leaf, BEFORE the inclusion:
//     uint32_t pack_mean(float r, float g, float b)     a float mean to RGBA8888 as a render finishes a pixel: square root, clamp, pack
// tonemap.hip hands in contract.hpp's own, the CPU restatement the oracle's square root and pack: neither is restated here.
#pragma once

#include <stdint.h>
#include "../../include/rt_hip.h" // (rt_hip_tonemap_params)

#if defined(__HIPCC__)
#define RT_HIP_TONEMAP_FN __device__ __forceinline__
#define RT_HIP_TONEMAP_BITS_FN __host__ __device__ __forceinline__ // (tonemap.hip's host side moves float bits through the state record too)
#else
#define RT_HIP_TONEMAP_FN inline
#define RT_HIP_TONEMAP_BITS_FN inline
#endif

namespace rt_hip
{
namespace tonemap
{
	constexpr uint32_t bins = 256;			  // 8 per octave, 2^-16 .. 2^16
	constexpr uint32_t histogram_words = 257; // the bins, and behind them the skipped pixels
	constexpr uint32_t state_words = 8;		  // exposure bits, target bits, counted, skipped, kept, mean_q8, two reserved
	constexpr int32_t first_bin_bits = 888;	  // bits >> 20 of 2^-16: exponent 111, mantissa 000
	constexpr float cap = 1048576.0f;		  // 2^20: what an exposed channel is held to

	RT_HIP_TONEMAP_BITS_FN uint32_t bits_of(float f) { return __builtin_bit_cast(uint32_t, f); }
	RT_HIP_TONEMAP_BITS_FN float float_of(uint32_t u) { return __builtin_bit_cast(float, u); }

	struct rgb
	{
		float r, g, b;
	};

	// Y = (0.2126 r + 0.7152 g) + 0.0722 b
	RT_HIP_TONEMAP_FN float luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

	// a pixel is metered if its luminance is a number, positive and finite
	RT_HIP_TONEMAP_FN bool counted(float y) { return y == y && y > 0.0f && (bits_of(y) & 0x7F800000u) != 0x7F800000u; }

	// The bin of a counted luminance: its exponent and the top three bits of its mantissa, from 2^-16 — a piecewise-linear log2,
	// 8 bins per octave.  Anything darker lands in bin 0, anything from 2^16 in bin 255.
	RT_HIP_TONEMAP_FN uint32_t bin_of(float y)
	{
		const int32_t b = static_cast<int32_t>(bits_of(y) >> 20) - first_bin_bits; // (y > 0: the sign bit is clear)
		return static_cast<uint32_t>(b < 0 ? 0 : (b > 255 ? 255 : b));
	}

	// What the meter makes of the histogram, in exact integer arithmetic: of the N counted pixels in rank order (darkest first) the
	// lo = floor(N low / 1000) darkest and the hi = floor(N high / 1000) brightest are dropped — a cut may fall inside a bin, which
	// then contributes only its part inside the rank window [lo, N - hi) — and q = floor(256 S / kept) is the mean bin of the kept
	// ones in 1/256 of a bin, S = sum of bin x taken.  low + high < 1000 (the parameter check), so kept >= 1 whenever N >= 1.
	// The metered luminance is the bin map inverted at the bin's centre: bits (888 << 20) + (q << 12) + (1 << 19).
	// target = clamp(key / L, min_exposure, max_exposure), and 1 where nothing was counted.
	struct metered
	{
		uint32_t counted, kept, mean_q8;
		float target;
	};
	RT_HIP_TONEMAP_FN metered meter(const uint32_t* histogram, const rt_hip_tonemap_params& p)
	{
		uint64_t n = 0;
		for (uint32_t b = 0; b < bins; b++)
			n += histogram[b];
		if (n == 0)
			return { 0u, 0u, 0u, 1.0f };
		const uint64_t lo = n * p.low_permille / 1000u, hi = n * p.high_permille / 1000u;
		const uint64_t last = n - hi; // the window is [lo, last)
		uint64_t s = 0, before = 0;
		for (uint32_t b = 0; b < bins; b++)
		{
			const uint64_t after = before + histogram[b];
			const uint64_t from = before > lo ? before : lo, to = after < last ? after : last;
			s += from < to ? (to - from) * b : 0u;
			before = after;
		}
		const uint64_t kept = n - lo - hi;
		const uint32_t q = static_cast<uint32_t>(256u * s / kept);
		const float l = float_of((static_cast<uint32_t>(first_bin_bits) << 20) + (q << 12) + (1u << 19));
		float t = p.key / l;
		t = t < p.min_exposure ? p.min_exposure : t;
		t = t > p.max_exposure ? p.max_exposure : t;
		return { static_cast<uint32_t>(n), static_cast<uint32_t>(kept), q, t };
	}

	// The exposure applied: eased from the frame before where adaptation < 1 and its exposure (the state record's first word) is a
	// finite positive float; the target otherwise.
	RT_HIP_TONEMAP_FN float adapt(uint32_t previous_bits, float target, float adaptation)
	{
		const float prev = float_of(previous_bits);
		const bool eased = adaptation < 1.0f && counted(prev);
		return eased ? prev + adaptation * (target - prev) : target;
	}

	// One pixel: every channel times the exposure, NaN and negatives to 0, held to 2^20 (+inf too), then the curve.
	//   NONE      o = v
	//   REINHARD  extended, on the luminance Yv of v, hue kept: s = (1 + Yv / white^2) / (1 + Yv), o = v s
	//   ACES      per channel: o = (v (2.51 v + 0.03)) / (v (2.43 v + 0.59) + 0.14)
	// Every operand is finite and not negative (white^2 >= 2^-40 by the parameter check): no NaN comes out, whatever goes in.
	RT_HIP_TONEMAP_FN float exposed(float c, float exposure)
	{
		float v = c * exposure;
		v = v > 0.0f ? v : 0.0f;
		return v < cap ? v : cap;
	}
	RT_HIP_TONEMAP_FN float aces(float v) { return (v * (2.51f * v + 0.03f)) / (v * (2.43f * v + 0.59f) + 0.14f); }
	RT_HIP_TONEMAP_FN rgb map_pixel(float r, float g, float b, float exposure, uint32_t curve, float white2)
	{
		const rgb v = { exposed(r, exposure), exposed(g, exposure), exposed(b, exposure) };
		if (curve == RT_HIP_TONEMAP_REINHARD)
		{
			const float yv = luminance(v.r, v.g, v.b);
			const float s = (1.0f + yv / white2) / (1.0f + yv);
			return { v.r * s, v.g * s, v.b * s };
		}
		if (curve == RT_HIP_TONEMAP_ACES)
			return { aces(v.r), aces(v.g), aces(v.b) };
		return v;
	}

	// the packed pixel of a mapped one: the renderer's own finish
	RT_HIP_TONEMAP_FN uint32_t finish(rgb o) { return leaf::pack_mean(o.r, o.g, o.b); }
}
}
