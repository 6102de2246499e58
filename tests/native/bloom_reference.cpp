// tests/native/bloom_reference.cpp — the CPU restatement of bloom.  TEST INFRASTRUCTURE, built with g++ alone into
// tests/native/libbloom_reference.so (tests/bloom_reference.py binds it) and into the program of `make sanitize-bloom`.
//
// The operation is rt_amd/csrc/bloom_rules.hpp — the very text the kernels of rt_amd/csrc/bloom.hip run — applied serially, texel after
// texel, from plain arrays: one loop per level and direction, no tile, no staging.  The parameter check, the level plan and the parser
// are rt_amd/csrc/bloom.cpp as it is, compiled in by the Makefile.  The device's result must equal what comes out here bit for bit
// (tests/test_gpu_bloom.py).
#include "../../include/rt_hip.h"
#include "../../rt_amd/csrc/bloom_rules.hpp"
#include "../../rt_amd/csrc/bloom.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace rt_hip;

namespace
{
	bloom::rgb at(const float* image, uint32_t w, uint32_t x, uint32_t y)
	{
		const size_t i = (static_cast<size_t>(y) * w + x) * 3u;
		return { image[i], image[i + 1u], image[i + 2u] };
	}
	void put(float* image, uint32_t w, uint32_t x, uint32_t y, bloom::rgb v)
	{
		const size_t i = (static_cast<size_t>(y) * w + x) * 3u;
		image[i] = v.r, image[i + 1u] = v.g, image[i + 2u] = v.b;
	}
	bloom::rgb tent(const float* coarse, uint32_t wc, uint32_t hc, uint32_t x, uint32_t y)
	{
		const uint32_t X = x >> 1, Xn = bloom::tent_neighbour(x, wc), Y = y >> 1, Yn = bloom::tent_neighbour(y, hc);
		return bloom::tent2(bloom::tent2(at(coarse, wc, X, Y), at(coarse, wc, Xn, Y)), bloom::tent2(at(coarse, wc, X, Yn), at(coarse, wc, Xn, Yn)));
	}
}

extern "C" {

void bloom_ref_default_params(rt_hip_bloom_params* out) { *out = default_bloom_params(); }

// check_bloom_params: the status, and the message into `message` (may be NULL)
int bloom_ref_check(const rt_hip_bloom_params* params, char* message, size_t size)
{
	const bloom_check c = check_bloom_params(*params);
	if (message && size)
		std::snprintf(message, size, "%s", c.message);
	return c.status;
}

int bloom_ref_from_spec(const char* spec, rt_hip_bloom_params* out, char* message, size_t size)
{
	const bloom_check c = bloom_from_spec(spec, out);
	if (message && size)
		std::snprintf(message, size, "%s", c.message);
	return c.status;
}

// plan_bloom laid open: sizes[2 i], sizes[2 i + 1] the width and height of level i, offsets[i] its first float in the scratch
int bloom_ref_plan(uint32_t width, uint32_t height, const rt_hip_bloom_params* params, uint32_t* levels, uint32_t* sizes, uint64_t* offsets, float* norm, float* gain, uint64_t* scratch_bytes)
{
	const rt_hip_bloom_params p = params ? *params : default_bloom_params();
	if (const bloom_check c = check_bloom_params(p); c.status)
		return c.status;
	if (!width || !height)
		return RT_HIP_INVALID_ARGUMENT;
	const bloom_plan plan = plan_bloom(width, height, p);
	*levels = plan.levels;
	for (uint32_t i = 0; i < plan.levels; i++)
		sizes[2u * i] = plan.level[i].width, sizes[2u * i + 1u] = plan.level[i].height, offsets[i] = plan.level[i].offset;
	*norm = plan.norm, *gain = plan.gain, *scratch_bytes = plan.scratch_bytes;
	return RT_HIP_OK;
}

// The whole operation, serially: rt_hip_bloom_device's arguments on host arrays (params NULL = defaults; rgb_out may be rgb_in).
// `down` and `up` (either may be NULL): scratch_bytes each, every level as the way down left it and as the way up left it, laid out as
// the plan says.  Returns the parameters' refusal; nothing is written when it refuses.
int bloom_ref_frame(uint32_t width, uint32_t height, const float* rgb_in, const rt_hip_bloom_params* params, float* down, float* up, float* layer_out, float* rgb_out)
{
	const rt_hip_bloom_params p = params ? *params : default_bloom_params();
	if (const bloom_check c = check_bloom_params(p); c.status)
		return c.status;
	if (!width || !height)
		return RT_HIP_INVALID_ARGUMENT;
	const bloom_plan plan = plan_bloom(width, height, p);
	std::vector<float> pyramid(plan.scratch_bytes / sizeof(float));
	const auto level = [&](uint32_t i) { return pyramid.data() + plan.level[i].offset; };
	const bloom_level* const l = plan.level;

	// the prefilter: the bright pass of 2 x 2 full-size pixels, averaged
	for (uint32_t Y = 0; Y < l[0].height; Y++)
		for (uint32_t X = 0; X < l[0].width; X++)
		{
			const auto bright_at = [&](uint32_t dx, uint32_t dy)
			{
				const bloom::rgb c = at(rgb_in, width, bloom::quad_index(X, dx, width), bloom::quad_index(Y, dy, height));
				return bloom::bright(c.r, c.g, c.b, p.threshold, p.knee);
			};
			put(level(0), l[0].width, X, Y, bloom::box4(bright_at(0, 0), bright_at(1, 0), bright_at(0, 1), bright_at(1, 1)));
		}
	// down: rows first, then the five row sums
	for (uint32_t i = 0; i + 1u < plan.levels; i++)
		for (uint32_t Y = 0; Y < l[i + 1u].height; Y++)
			for (uint32_t X = 0; X < l[i + 1u].width; X++)
			{
				float sums[5][3];
				for (int32_t dy = -2; dy <= 2; dy++)
				{
					const uint32_t y = bloom::clamp_index(static_cast<int32_t>(2u * Y) + dy, l[i].height);
					bloom::rgb t[5];
					for (int32_t dx = -2; dx <= 2; dx++)
						t[dx + 2] = at(level(i), l[i].width, bloom::clamp_index(static_cast<int32_t>(2u * X) + dx, l[i].width), y);
					sums[dy + 2][0] = bloom::binomial5(t[0].r, t[1].r, t[2].r, t[3].r, t[4].r);
					sums[dy + 2][1] = bloom::binomial5(t[0].g, t[1].g, t[2].g, t[3].g, t[4].g);
					sums[dy + 2][2] = bloom::binomial5(t[0].b, t[1].b, t[2].b, t[3].b, t[4].b);
				}
				float v[3];
				for (uint32_t c = 0; c < 3u; c++)
					v[c] = bloom::down_finish(bloom::binomial5(sums[0][c], sums[1][c], sums[2][c], sums[3][c], sums[4][c]));
				put(level(i + 1u), l[i + 1u].width, X, Y, { v[0], v[1], v[2] });
			}
	if (down)
		std::memcpy(down, pyramid.data(), plan.scratch_bytes);
	// up, coarsest to finest, in place
	for (uint32_t i = plan.levels - 1u; i-- > 0u;)
		for (uint32_t y = 0; y < l[i].height; y++)
			for (uint32_t x = 0; x < l[i].width; x++)
				put(level(i), l[i].width, x, y, bloom::up_sum(at(level(i), l[i].width, x, y), p.scatter, tent(level(i + 1u), l[i + 1u].width, l[i + 1u].height, x, y)));
	if (up)
		std::memcpy(up, pyramid.data(), plan.scratch_bytes);
	// the composite
	for (uint32_t y = 0; y < height; y++)
		for (uint32_t x = 0; x < width; x++)
		{
			const bloom::rgb layer = tent(level(0), l[0].width, l[0].height, x, y);
			if (rgb_out)
				put(rgb_out, width, x, y, bloom::composite(at(rgb_in, width, x, y), plan.gain, layer));
			if (layer_out)
				put(layer_out, width, x, y, layer);
		}
	return RT_HIP_OK;
}
}
