// tests/native/upsample_reference.cpp — the CPU restatement of guided upsampling.  TEST INFRASTRUCTURE, built with g++
// alone into tests/native/libupsample_reference.so (tests/upsample_reference.py binds it) and into the program of `make sanitize-upsample`.
//
// The reconstruction is rt_amd/csrc/upsample_rules.hpp — the very text the kernel of rt_amd/csrc/upsample.hip runs per full pixel —
// applied serially, pixel after pixel, from plain arrays.  Its leaf functions are the ORACLE's: this file includes oracle/cpu_ref.cpp
// (as tests/native/denoise_reference.cpp does) and hands its dot(), its square root and its pack() to the rules, where the kernel hands
// in contract.hpp's; neither side restates them.  The parameter and size checks and the low-size rule are rt_amd/csrc/upsample.cpp as
// it is, compiled in by the Makefile.  The device's result must equal what comes out here bit for bit (tests/test_gpu_upsample.py).
#include "../../include/rt_hip.h"

// the oracle's entry points come along under names of their own
#define oracle_render upsample_ref_oracle_render
#define oracle_closest_hit upsample_ref_oracle_closest_hit
#define oracle_random upsample_ref_oracle_random
#define oracle_stream_keys upsample_ref_oracle_stream_keys
#define oracle_sqrt_div upsample_ref_oracle_sqrt_div
#define oracle_inv_sqrt upsample_ref_oracle_inv_sqrt
#define oracle_inv_sqrt_step upsample_ref_oracle_inv_sqrt_step
#define oracle_pack upsample_ref_oracle_pack
#define oracle_sky upsample_ref_oracle_sky
#define oracle_primary_ray upsample_ref_oracle_primary_ray
#define oracle_frame_constants upsample_ref_oracle_frame_constants
#define oracle_dielectric_direction upsample_ref_oracle_dielectric_direction
#define oracle_hits_box upsample_ref_oracle_hits_box
#define oracle_render_census upsample_ref_oracle_render_census
#define oracle_unit_vector upsample_ref_oracle_unit_vector
#include "../../oracle/cpu_ref.cpp"

namespace rt_hip
{
namespace denoise
{
	namespace leaf
	{
		inline float dot3(float ax, float ay, float az, float bx, float by, float bz) { return ::dot(::vec3{ ax, ay, az }, ::vec3{ bx, by, bz }); }
		inline float sqrt_rn(float x) { return std::sqrt(x); }
		inline uint32_t pack(float r, float g, float b) { return ::pack(::vec3{ r, g, b }); }
	}
}
}
#include "../../rt_amd/csrc/upsample_rules.hpp"
#include "../../rt_amd/csrc/upsample.hpp"

#include <cstdio>

using namespace rt_hip;

namespace
{
	struct low_fetch
	{
		const float* rgb;
		const float* guide;
		uint32_t width;
		denoise::tap operator()(int32_t x, int32_t y) const
		{
			const size_t pixel = static_cast<size_t>(y) * static_cast<size_t>(width) + static_cast<size_t>(x);
			const float* const g = guide + pixel * denoise::guide_words;
			return { { g[0], g[1], g[2], g[3], g[4], g[5], g[6], denoise::bits_of(g[7]) }, { rgb[pixel * 3], rgb[pixel * 3 + 1], rgb[pixel * 3 + 2] } };
		}
	};
}

extern "C" {

void upsample_ref_default_params(rt_hip_upsample_params* out) { *out = default_upsample_params(); }

// check_upsample_params: the status, and the message into `message` (may be NULL)
int upsample_ref_check(const rt_hip_upsample_params* params, char* message, size_t size)
{
	const upsample_check c = check_upsample_params(*params);
	if (message && size)
		std::snprintf(message, size, "%s", c.message);
	return c.status;
}

int upsample_ref_check_sizes(uint32_t W, uint32_t H, uint32_t w, uint32_t h, char* message, size_t size)
{
	const upsample_check c = check_upsample_sizes(W, H, w, h);
	if (message && size)
		std::snprintf(message, size, "%s", c.message);
	return c.status;
}

int upsample_ref_low_size(uint32_t W, uint32_t H, uint32_t factor, uint32_t* w, uint32_t* h, char* message, size_t size)
{
	const upsample_check c = upsample_low_size(W, H, factor, w, h);
	if (message && size)
		std::snprintf(message, size, "%s", c.message);
	return c.status;
}

// source_of(x, W, w): first, and the two weights
void upsample_ref_source_of(uint32_t x, uint32_t W, uint32_t w, int32_t* first, float* b0, float* b1)
{
	const upsample::source s = upsample::source_of(x, W, w);
	*first = s.first, *b0 = s.b0, *b1 = s.b1;
}

// the whole reconstruction, serially: rt_hip_upsample_device's arguments on host arrays (params NULL = defaults; any output may be NULL).
// Returns the first refusal's status (parameters, then sizes); nothing is written when it refuses.
int upsample_ref_frame(uint32_t W, uint32_t H, uint32_t w, uint32_t h, const float* rgb_low, const float* guide_low, const float* guide_full, const rt_hip_upsample_params* params, float* rgb_out, uint32_t* rgba_out,
					   uint32_t* orphans_out)
{
	const rt_hip_upsample_params p = params ? *params : default_upsample_params();
	if (const upsample_check c = check_upsample_params(p); c.status)
		return c.status;
	if (const upsample_check c = check_upsample_sizes(W, H, w, h); c.status)
		return c.status;
	const upsample::constants k = upsample::constants_of(p);
	const low_fetch fetch = { rgb_low, guide_low, w };
	uint32_t orphans = 0;
	for (uint32_t y = 0; y < H; y++)
		for (uint32_t x = 0; x < W; x++)
		{
			const size_t pixel = static_cast<size_t>(y) * W + x;
			const float* const g = guide_full + pixel * denoise::guide_words;
			const denoise::guide full = { g[0], g[1], g[2], g[3], g[4], g[5], g[6], denoise::bits_of(g[7]) };
			const upsample::pixel out = upsample::upsample_pixel(x, y, W, H, w, h, k, fetch, full);
			orphans += out.orphan ? 1u : 0u;
			if (rgb_out)
				rgb_out[pixel * 3] = out.c.r, rgb_out[pixel * 3 + 1] = out.c.g, rgb_out[pixel * 3 + 2] = out.c.b;
			if (rgba_out)
				rgba_out[pixel] = denoise::finish(out.c);
		}
	if (orphans_out)
		*orphans_out = orphans;
	return RT_HIP_OK;
}
}
