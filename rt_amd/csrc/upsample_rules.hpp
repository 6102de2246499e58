// rt_amd/csrc/upsample_rules.hpp — the per-element rules of guided upsampling, written ONCE so that hipcc and g++
// both compile them: the kernel of upsample.hip runs this text per full-size pixel, tests/native/upsample_reference.cpp restates the
// whole frame serially over the very same functions, and the device's result must equal that restatement bit for bit.
//
// What makes that possible is what makes it possible for the denoiser (denoise_rules.hpp, whose guide, rgb, tap and leaf functions
// are used here and not restated): + - x, correctly rounded '/', compare-and-select and the contract's dot() only, no contraction
// (-ffp-contract=off on both compilers), and ONE summation order: the Y0 row first, X0 before X1.  The geometry is exact integer
// arithmetic; the only floats it makes are quotients of two integers below 2^24.  How a low tap is FETCHED (an LDS tile, a plain
// array) is the caller's and reaches nothing below.
//
// Include after the leaf functions exist, as for denoise_rules.hpp (which this header includes).
#pragma once

#include "denoise_rules.hpp"

namespace rt_hip
{
namespace upsample
{
	constexpr uint32_t max_side = 1u << 22;	 // a frame's side: 2 * side and every remainder below it are exact as floats
	constexpr uint32_t max_factor = 4;		 // rt_hip_upsample_low_size and rt_hip_render_upscaled (the device entry takes any w <= W)
	constexpr uint32_t low_words = 11;		 // a low tap: 8 words of guide, 3 of colour
	constexpr int32_t max_staged_side = 18;	 // the low taps a run of 16 full pixels can reach span at most 17 (w == W); one to spare

	// Where full pixel x of W lies among the w low pixels.  Its centre in low-pixel coordinates is u = ((2x + 1) w - W) / (2W); with
	// n = (2x + 1) w - W:  first = floor(n / 2W) — -1 at the left edge when w < W, never less, since n > -2W — and the remainder
	// r = n - first * 2W in [0, 2W) gives the bilinear weights of `first` and `first + 1`: (2W - r) / 2W and r / 2W.
	struct source
	{
		int32_t first;
		float b0, b1;
	};
	RT_HIP_DENOISE_FN source source_of(uint32_t x, uint32_t W, uint32_t w)
	{
		const int64_t n = (2 * static_cast<int64_t>(x) + 1) * static_cast<int64_t>(w) - static_cast<int64_t>(W);
		const uint32_t two_w = 2u * W;
		int32_t first = -1;
		if (n >= 0)
		{
			const uint64_t un = static_cast<uint64_t>(n); // (at most 2^45; a frame of ordinary size divides in 32 bits)
			first = static_cast<int32_t>((un >> 32) ? un / two_w : static_cast<uint64_t>(static_cast<uint32_t>(un) / two_w));
		}
		const int32_t r = static_cast<int32_t>(n - static_cast<int64_t>(first) * static_cast<int64_t>(two_w));
		const float span = static_cast<float>(static_cast<int32_t>(two_w));
		return { first, static_cast<float>(static_cast<int32_t>(two_w) - r) / span, static_cast<float>(r) / span };
	}

	// what the pixel rule derives from the parameters
	struct constants
	{
		uint32_t normal_squarings;
		float sigma_depth;
		float sigma_albedo2; // sigma_albedo^2
		float min_weight;
	};
	RT_HIP_DENOISE_FN constants constants_of(const rt_hip_upsample_params& p) { return { p.normal_squarings, p.sigma_depth, p.sigma_albedo * p.sigma_albedo, p.min_weight }; }

	// The weight of low tap q (guide and colour) for full pixel p (guide only: it has no colour yet), a product in a fixed order: the
	// bilinear weight b = bx * by, then the normal, depth and albedo terms of denoise::tap_weight — the same arithmetic, the same rules:
	//   * sky against hit: 0.  Sky against sky: b alone.
	//   * a tap whose colour has a non-finite channel: 0.
	//   * a weight that comes out as NaN counts as 0 as well.
	// All by select: both sides evaluate every term and pick.
	RT_HIP_DENOISE_FN float tap_weight(const denoise::guide& p, const denoise::tap& q, float b, const constants& k)
	{
		const bool sky_p = p.id == 0u, sky_q = q.g.id == 0u;
		const bool hits = !sky_p && !sky_q;
		float w = b;

		const float along = denoise::leaf::dot3(p.nx, p.ny, p.nz, q.g.nx, q.g.ny, q.g.nz);
		float wn = along > 0.0f ? along : 0.0f;
		for (uint32_t s = 0; s < k.normal_squarings; s++)
			wn = wn * wn;
		w = w * (hits ? wn : 1.0f);

		const float deeper = p.depth > q.g.depth ? p.depth : q.g.depth;
		const float rz = (p.depth - q.g.depth) / (k.sigma_depth * deeper);
		const float wz = 1.0f / (1.0f + rz * rz);
		w = w * (hits ? wz : 1.0f);

		const float dar = p.ar - q.g.ar, dag = p.ag - q.g.ag, dab = p.ab - q.g.ab;
		const float wa = 1.0f / (1.0f + denoise::leaf::dot3(dar, dag, dab, dar, dag, dab) / k.sigma_albedo2);
		w = w * (hits ? wa : 1.0f);

		const bool usable = (sky_p == sky_q) && denoise::is_finite(q.c) && w == w;
		return usable ? w : 0.0f;
	}

	// The pixel rule.  Over the four low taps (X0 | X1, Y0 | Y1), those outside the low frame skipped, the Y0 row first and X0 before X1:
	//   sw = sum of w, and the sums of w c      (the guided weights above)
	//   sb = sum of b, and the sums of b c      (b = bx * by over the taps with a finite colour: the plain bilinear weights)
	// sw >= min_weight and sw > 0:  out = (sum of w c) / sw.
	// Otherwise the pixel is an ORPHAN — the full frame sees there what none of its low taps saw — and takes the bilinear mean
	// (sum of b c) / sb, or (0, 0, 0) where sb is not positive (no finite tap inside the frame, or only ones of weight 0).
	// fetch_low(X, Y) returns the tap record of a low pixel INSIDE the low frame; how is the caller's.
	struct pixel
	{
		denoise::rgb c;
		bool orphan;
	};
	template <typename Fetch>
	RT_HIP_DENOISE_FN pixel upsample_pixel(uint32_t x, uint32_t y, uint32_t W, uint32_t H, uint32_t w, uint32_t h, const constants& k, const Fetch& fetch_low, const denoise::guide& p)
	{
		const source sx = source_of(x, W, w), sy = source_of(y, H, h);
		float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
		float bw = 0.0f, br = 0.0f, bg = 0.0f, bb = 0.0f;
		for (int32_t j = 0; j < 2; j++)
			for (int32_t i = 0; i < 2; i++)
			{
				const int32_t qx = sx.first + i, qy = sy.first + j;
				if (qx < 0 || qx >= static_cast<int32_t>(w) || qy < 0 || qy >= static_cast<int32_t>(h))
					continue;
				const denoise::tap q = fetch_low(qx, qy);
				const float b = (i ? sx.b1 : sx.b0) * (j ? sy.b1 : sy.b0);
				const float wq = tap_weight(p, q, b, k);
				const bool finite = denoise::is_finite(q.c); // (a weight of 0 must not meet an infinity)
				const denoise::rgb c = { finite ? q.c.r : 0.0f, finite ? q.c.g : 0.0f, finite ? q.c.b : 0.0f };
				const float bq = finite ? b : 0.0f;
				sw = sw + wq;
				sr = sr + wq * c.r;
				sg = sg + wq * c.g;
				sb = sb + wq * c.b;
				bw = bw + bq;
				br = br + bq * c.r;
				bg = bg + bq * c.g;
				bb = bb + bq * c.b;
			}
		const bool guided = sw >= k.min_weight && sw > 0.0f;
		const bool plain = bw > 0.0f;
		const float d = guided ? sw : (plain ? bw : 1.0f);
		const denoise::rgb n = { guided ? sr : (plain ? br : 0.0f), guided ? sg : (plain ? bg : 0.0f), guided ? sb : (plain ? bb : 0.0f) };
		return { { n.r / d, n.g / d, n.b / d }, !guided };
	}
}
}
