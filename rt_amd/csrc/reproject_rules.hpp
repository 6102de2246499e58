// rt_amd/csrc/reproject_rules.hpp — the per-pixel rule of temporal accumulation, written ONCE so that hipcc and g++
// both compile it: reproject_frame of temporal.hip runs this text per pixel, tests/native/reproject_reference.cpp restates the whole
// frame serially over the very same function, and the device's result must equal that restatement bit for bit.
//
// What makes that possible: the rule is defined with + - x, correctly rounded '/', an explicit fma, compare-and-select and one
// float -> int truncation of a value known to be in range — nothing else — both compilers are told not to contract
// (-ffp-contract=off), and every sum is a plain sequential add in ONE order: the four taps with j (rows) outside and i inside.
//
// The leaf functions come from whoever includes this header, in namespace rt_hip::reproject::leaf, BEFORE the inclusion:
//     float dot3(float ax, float ay, float az, float bx, float by, float bz)   the contract's dot(): fma(az, bz, fma(ay, by, ax * bx))
//     float fma(float a, float b, float c)                                     one rounding
//     bool  is_finite(float)
// temporal.hip hands in contract.hpp's own, the CPU restatement the oracle's (oracle/cpu_ref.cpp): none of them is restated here.
#pragma once

#include <stdint.h>
#include "../../include/rt_hip.h" // (rt_hip_temporal_params)

#if defined(__HIPCC__)
#define RT_HIP_REPROJECT_FN __device__ __forceinline__
#define RT_HIP_REPROJECT_HOST_FN __host__ __device__ __forceinline__
#else
#define RT_HIP_REPROJECT_FN inline
#define RT_HIP_REPROJECT_HOST_FN inline
#endif

namespace rt_hip
{
namespace reproject
{
	constexpr uint32_t record_words = 8;		  // per pixel: two float4s
	constexpr uint32_t max_samples_in = 4096;	  // what one traced frame can stand for
	constexpr uint32_t max_history_cap = 1u << 20; // (a float counts samples exactly far beyond)

	// The history record of a pixel, 8 words: px py pz length | nx ny nz id
	//   p        world position of the pixel's first hit (0, 0, 0 for sky)
	//   length   the samples the pixel's colour stands for, as a float; 0: the pixel can be nobody's history
	//   n, id    the guide's normal and id (0 = sky)
	struct record
	{
		float px, py, pz, length;
		float nx, ny, nz;
		uint32_t id;
	};
	struct rgb
	{
		float r, g, b;
	};
	struct tap // one pixel of the previous history
	{
		record q;
		rgb c;
	};
	// what the rule reads of the pixel's guide record (denoise_rules.hpp, struct guide): the first hit's normal, distance and id
	struct surface
	{
		float nx, ny, nz, depth;
		uint32_t id;
	};
	struct ray
	{
		float ox, oy, oz; // origin
		float dx, dy, dz; // unit direction
	};
	// the parameters as the rule uses them
	struct constants
	{
		float max_history;		  // float(max_history_samples): exact
		float position_tolerance; // relative to the hit distance
		float normal_threshold;
	};
	RT_HIP_REPROJECT_HOST_FN constants constants_of(const rt_hip_temporal_params& p) { return { static_cast<float>(p.max_history_samples), p.position_tolerance, p.normal_threshold }; }

	struct result
	{
		rgb out;
		record rec;
		bool had_history;
	};

	RT_HIP_REPROJECT_FN bool is_finite(rgb c) { return leaf::is_finite(c.r) && leaf::is_finite(c.g) && leaf::is_finite(c.b); }

	// The pixel rule.  `g`, `c`, `samples_in` (1 .. 4096, as a float) and `centre` describe the current frame's pixel; P is the
	// PREVIOUS frame's forward view-projection ([r * 4 + c], world -> clip); fetch(x, y) returns the previous history of a pixel INSIDE
	// the frame and is called only if have_history.
	//   * a current colour with a non-finite channel passes through with length 0 and takes no history
	//   * sky takes no history and keeps none: record 0 0 0 samples_in | 0 0 0 0
	//   * there is no test on the sign of clip.w: the position check rejects a point behind the previous camera
	template <typename Fetch>
	RT_HIP_REPROJECT_FN result reproject_pixel(int32_t width, int32_t height, const surface& g, rgb c, float samples_in, const ray& centre, const float* P, bool have_history, const constants& k, const Fetch& fetch)
	{
		const bool usable = is_finite(c);
		if (g.id == 0u)
			return { c, { 0.0f, 0.0f, 0.0f, usable ? samples_in : 0.0f, 0.0f, 0.0f, 0.0f, 0u }, false };
		const float px = leaf::fma(centre.dx, g.depth, centre.ox), py = leaf::fma(centre.dy, g.depth, centre.oy), pz = leaf::fma(centre.dz, g.depth, centre.oz);
		result plain = { c, { px, py, pz, usable ? samples_in : 0.0f, g.nx, g.ny, g.nz, g.id }, false };
		if (!usable || !have_history)
			return plain;

		const float clip_x = leaf::fma(P[2], pz, leaf::fma(P[1], py, leaf::fma(P[0], px, P[3])));
		const float clip_y = leaf::fma(P[6], pz, leaf::fma(P[5], py, leaf::fma(P[4], px, P[7])));
		const float clip_w = leaf::fma(P[14], pz, leaf::fma(P[13], py, leaf::fma(P[12], px, P[15])));
		const float ndc_x = clip_x / clip_w, ndc_y = clip_y / clip_w;
		const float fw = static_cast<float>(width), fh = static_cast<float>(height);
		const float u = (ndc_x + 1.0f) * (0.5f * fw) - 0.5f; // pixel i's centre is at i
		const float v = (1.0f - ndc_y) * (0.5f * fh) - 0.5f;
		if (!(u > -1.0f && u < fw && v > -1.0f && v < fh)) // (NaN and the infinities leave here too)
			return plain;
		const int32_t x0 = static_cast<int32_t>(u + 1.0f) - 1, y0 = static_cast<int32_t>(v + 1.0f) - 1; // (u + 1 in [0, width + 1]: truncation is floor)
		const float fx = u - static_cast<float>(x0), fy = v - static_cast<float>(y0);
		const float reach = k.position_tolerance * g.depth, reach2 = reach * reach;

		float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sl = 0.0f;
		for (int32_t j = 0; j < 2; j++)
			for (int32_t i = 0; i < 2; i++)
			{
				const int32_t qx = x0 + i, qy = y0 + j;
				float w = 0.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f, length = 0.0f; // a tap that does not count adds 0 x 0
				if (qx >= 0 && qx < width && qy >= 0 && qy < height)
				{
					const tap t = fetch(qx, qy);
					const float ex = t.q.px - px, ey = t.q.py - py, ez = t.q.pz - pz;
					const bool counts = t.q.id == g.id && t.q.length > 0.0f && is_finite(t.c) && leaf::dot3(t.q.nx, t.q.ny, t.q.nz, g.nx, g.ny, g.nz) >= k.normal_threshold && leaf::dot3(ex, ey, ez, ex, ey, ez) <= reach2;
					const float bilinear = (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy);
					w = counts ? bilinear : 0.0f;
					cr = counts ? t.c.r : 0.0f, cg = counts ? t.c.g : 0.0f, cb = counts ? t.c.b : 0.0f;
					length = counts ? t.q.length : 0.0f;
				}
				sw = sw + w;
				sr = sr + w * cr;
				sg = sg + w * cg;
				sb = sb + w * cb;
				sl = sl + w * length;
			}
		if (!(sw > 0.0f))
			return plain;
		const float hr = sr / sw, hg = sg / sw, hb = sb / sw, history = sl / sw;
		const float kept = history < k.max_history ? history : k.max_history;
		const float total = kept + samples_in;
		result blended = plain;
		blended.out = { (hr * kept + c.r * samples_in) / total, (hg * kept + c.g * samples_in) / total, (hb * kept + c.b * samples_in) / total };
		blended.rec.length = total;
		blended.had_history = true;
		return blended;
	}
}
}
