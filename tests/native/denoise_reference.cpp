// tests/native/denoise_reference.cpp — the CPU restatement of the guide-buffer denoiser.  TEST INFRASTRUCTURE, built
// with g++ alone into tests/native/libdenoise_reference.so (tests/denoise_reference.py binds it).
//
// The filter is rt_amd/csrc/denoise_rules.hpp — the very text the kernels of rt_amd/csrc/denoise.hip run per pixel — applied serially,
// pixel after pixel, iteration after iteration, from plain arrays.  Its leaf functions are the ORACLE's: this file includes
// oracle/cpu_ref.cpp (as tests/native/box_reference.cpp does) and hands its dot(), its square root and its pack() to the rules, where
// the kernels hand in contract.hpp's; neither side restates them.  The parameter check is rt_amd/csrc/denoise.cpp as it is, compiled
// in by the Makefile.  The device's result must equal what comes out here bit for bit (tests/test_gpu_denoise.py).
#include "../../include/rt_hip.h"

// the oracle's entry points come along under names of their own
#define oracle_render denoise_ref_oracle_render
#define oracle_closest_hit denoise_ref_oracle_closest_hit
#define oracle_random denoise_ref_oracle_random
#define oracle_stream_keys denoise_ref_oracle_stream_keys
#define oracle_sqrt_div denoise_ref_oracle_sqrt_div
#define oracle_inv_sqrt denoise_ref_oracle_inv_sqrt
#define oracle_inv_sqrt_step denoise_ref_oracle_inv_sqrt_step
#define oracle_pack denoise_ref_oracle_pack
#define oracle_sky denoise_ref_oracle_sky
#define oracle_primary_ray denoise_ref_oracle_primary_ray
#define oracle_frame_constants denoise_ref_oracle_frame_constants
#define oracle_dielectric_direction denoise_ref_oracle_dielectric_direction
#define oracle_hits_box denoise_ref_oracle_hits_box
#define oracle_render_census denoise_ref_oracle_render_census
#define oracle_unit_vector denoise_ref_oracle_unit_vector
#include "../../oracle/cpu_ref.cpp"

namespace rt_hip
{
namespace denoise
{
	namespace leaf
	{
		inline float dot3(float ax, float ay, float az, float bx, float by, float bz) { return ::dot(::vec3{ ax, ay, az }, ::vec3{ bx, by, bz }); }
		inline float sqrt_rn(float x) { return std::sqrt(x); } // (mg_ray_tracer.cpp:196-198 as the oracle's render_pixel takes it)
		inline uint32_t pack(float r, float g, float b) { return ::pack(::vec3{ r, g, b }); }
	}
}
}
#include "../../rt_amd/csrc/denoise_rules.hpp"
#include "../../rt_amd/csrc/denoise.hpp"

#include <cstdio>
#include <vector>

using namespace rt_hip;

namespace
{
	struct image_fetch
	{
		const float* rgb;
		const float* guide;
		int32_t width;
		denoise::tap operator()(int32_t x, int32_t y) const
		{
			const size_t pixel = static_cast<size_t>(y) * static_cast<size_t>(width) + static_cast<size_t>(x);
			const float* const g = guide + pixel * denoise::guide_words;
			return { { g[0], g[1], g[2], g[3], g[4], g[5], g[6], denoise::bits_of(g[7]) }, { rgb[pixel * 3], rgb[pixel * 3 + 1], rgb[pixel * 3 + 2] } };
		}
	};
}

extern "C" {

void denoise_ref_default_params(rt_hip_denoise_params* out) { *out = default_denoise_params(); }

// check_denoise_params: the status, and the message into `message` (may be NULL)
int denoise_ref_check(const rt_hip_denoise_params* params, char* message, size_t size)
{
	const denoise_check c = check_denoise_params(*params);
	if (message && size)
		std::snprintf(message, size, "%s", c.message);
	return c.status;
}

// finish(): n means -> n packed pixels
void denoise_ref_finish(size_t n, const float* rgb, uint32_t* rgba)
{
	for (size_t i = 0; i < n; i++)
		rgba[i] = denoise::finish({ rgb[i * 3], rgb[i * 3 + 1], rgb[i * 3 + 2] });
}

// the whole filter, serially: rt_hip_denoise_device's arguments on host arrays (params NULL = defaults; either output may be NULL).
// Returns check_denoise_params' status; nothing is written when it refuses.
int denoise_ref_filter(uint32_t width, uint32_t height, const float* rgb_in, const float* guide, const rt_hip_denoise_params* params, float* rgb_out, uint32_t* rgba_out)
{
	const rt_hip_denoise_params p = params ? *params : default_denoise_params();
	if (const denoise_check c = check_denoise_params(p); c.status)
		return c.status;
	const size_t pixels = static_cast<size_t>(width) * height;
	std::vector<float> from(rgb_in, rgb_in + pixels * 3), to(pixels * 3);
	for (uint32_t i = 0; i < p.iterations; i++)
	{
		const denoise::pass_constants k = denoise::constants_of(p, i);
		const image_fetch fetch = { from.data(), guide, static_cast<int32_t>(width) };
		for (int32_t y = 0; y < static_cast<int32_t>(height); y++)
			for (int32_t x = 0; x < static_cast<int32_t>(width); x++)
			{
				const denoise::rgb c = denoise::filter_pixel(x, y, static_cast<int32_t>(width), static_cast<int32_t>(height), k, fetch);
				float* const o = to.data() + (static_cast<size_t>(y) * width + static_cast<size_t>(x)) * 3;
				o[0] = c.r, o[1] = c.g, o[2] = c.b;
			}
		from.swap(to);
	}
	for (size_t i = 0; i < pixels; i++)
	{
		if (rgb_out)
			rgb_out[i * 3] = from[i * 3], rgb_out[i * 3 + 1] = from[i * 3 + 1], rgb_out[i * 3 + 2] = from[i * 3 + 2];
		if (rgba_out)
			rgba_out[i] = denoise::finish({ from[i * 3], from[i * 3 + 1], from[i * 3 + 2] });
	}
	return RT_HIP_OK;
}
}
