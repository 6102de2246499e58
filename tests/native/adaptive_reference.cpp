// tests/native/adaptive_reference.cpp — the CPU restatement of adaptive sampling's update step.  TEST INFRASTRUCTURE,
// built with g++ alone into tests/native/libadaptive_reference.so (tests/adaptive_reference.py binds it).
//
// The rules are rt_amd/csrc/adaptive_rules.hpp — the very text adaptive_update of rt_amd/csrc/adaptive.hip runs per pixel — applied
// serially over a whole frame from plain arrays: every pixel's update first, then every pixel's 3 x 3 verdict, then the state words.
// A pixel is finished with the ORACLE's own pack (this file includes oracle/cpu_ref.cpp, as tests/native/reproject_reference.cpp does):
// sum / float(n), square root, clamp, pack — the worker's last lines.  The defaults, the parameter check and the sequencing are
// rt_amd/csrc/adaptive.cpp as it is, compiled in by the Makefile.  The device's moments, state words and pixels must equal what comes
// out here bit for bit (tests/test_gpu_adaptive.py).
#include "../../include/rt_hip.h"

// the oracle's entry points come along under names of their own
#define oracle_render adaptive_ref_oracle_render
#define oracle_closest_hit adaptive_ref_oracle_closest_hit
#define oracle_random adaptive_ref_oracle_random
#define oracle_stream_keys adaptive_ref_oracle_stream_keys
#define oracle_sqrt_div adaptive_ref_oracle_sqrt_div
#define oracle_inv_sqrt adaptive_ref_oracle_inv_sqrt
#define oracle_inv_sqrt_step adaptive_ref_oracle_inv_sqrt_step
#define oracle_pack adaptive_ref_oracle_pack
#define oracle_sky adaptive_ref_oracle_sky
#define oracle_primary_ray adaptive_ref_oracle_primary_ray
#define oracle_frame_constants adaptive_ref_oracle_frame_constants
#define oracle_dielectric_direction adaptive_ref_oracle_dielectric_direction
#define oracle_hits_box adaptive_ref_oracle_hits_box
#define oracle_render_census adaptive_ref_oracle_render_census
#define oracle_unit_vector adaptive_ref_oracle_unit_vector
#include "../../oracle/cpu_ref.cpp"

#include "../../rt_amd/csrc/adaptive_rules.hpp"
#include "../../rt_amd/csrc/adaptive.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace rt_hip;

extern "C" {

void adaptive_ref_default_params(rt_hip_adaptive_params* out) { *out = default_adaptive_params(); }

uint64_t adaptive_ref_pass_size(uint32_t pass_samples) { return adaptive_pass_size(pass_samples); }

// check_adaptive_params: the status, and the message into `message` (may be NULL)
int adaptive_ref_check(const rt_hip_adaptive_params* params, uint64_t pass_size, char* message, size_t size)
{
	const adaptive_check c = check_adaptive_params(*params, pass_size);
	if (message && size)
		std::snprintf(message, size, "%s", c.message);
	return c.status;
}

// One whole update step, serially: rt_hip_adaptive_update_device's arguments on host arrays (moments and state in place; rgba_out,
// rgb_out and active_pixels may be NULL).  Returns RT_HIP_OK, or the status the arguments are refused with — nothing is written then.
int adaptive_ref_step(uint32_t width, uint32_t height, uint32_t pass_samples, uint32_t first_pass, uint32_t whole_pass, const rt_hip_adaptive_params* params, const float* accum, const float* pass_sum, float* moments, uint32_t* state,
					  uint32_t* rgba_out, float* rgb_out, uint32_t* active_pixels)
{
	const rt_hip_adaptive_params p = params ? *params : default_adaptive_params();
	if (!pass_samples || (whole_pass && pass_samples % 16u))
		return RT_HIP_INVALID_ARGUMENT;
	if (const adaptive_check c = check_adaptive_params(p, whole_pass ? pass_samples : 0u); c.status)
		return c.status;
	const size_t pixels = static_cast<size_t>(width) * height;
	std::vector<adaptive::update> updates(pixels);
	for (size_t i = 0; i < pixels; i++)
	{
		const uint32_t word = first_pass ? 0u : state[i];
		adaptive::pass_sum sum = { 0.0f, 0.0f, 0.0f };
		adaptive::moments before = { 0.0f, 0.0f };
		if (first_pass || !adaptive::is_stopped(word)) // (a stopped pixel was not traced: its pass sum is stale scratch)
		{
			if (whole_pass)
				sum = { pass_sum[i * 3], pass_sum[i * 3 + 1], pass_sum[i * 3 + 2] };
			if (!first_pass)
				before = { moments[i * 2], moments[i * 2 + 1] };
		}
		updates[i] = adaptive::update_pixel(sum, before, word, pass_samples, first_pass != 0u, whole_pass != 0u, p);
	}
	uint32_t active = 0;
	const int32_t w = static_cast<int32_t>(width), h = static_cast<int32_t>(height);
	for (int32_t y = 0; y < h; y++)
		for (int32_t x = 0; x < w; x++)
		{
			const size_t i = static_cast<size_t>(y) * width + static_cast<size_t>(x);
			const uint32_t word = first_pass ? 0u : state[i];
			const bool stop = adaptive::stops(x, y, w, h, [&](int32_t qx, int32_t qy) -> bool { return updates[static_cast<size_t>(qy) * width + static_cast<size_t>(qx)].converged; });
			const uint32_t after = adaptive::next_state(word, first_pass != 0u, updates[i], stop);
			if (first_pass || !adaptive::is_stopped(word)) // (a stopped pixel's words are left as they are)
			{
				if (whole_pass)
					moments[i * 2] = updates[i].m.s1, moments[i * 2 + 1] = updates[i].m.s2;
				state[i] = after;
			}
			active += adaptive::is_stopped(after) ? 0u : 1u;
			// the worker's last lines (oracle/cpu_ref.cpp, render_pixel) over the pixel's own sample count
			const float n = static_cast<float>(adaptive::samples_of(after));
			const ::vec3 mean = { accum[i * 3] / n, accum[i * 3 + 1] / n, accum[i * 3 + 2] / n };
			if (rgb_out)
				rgb_out[i * 3] = mean.x, rgb_out[i * 3 + 1] = mean.y, rgb_out[i * 3 + 2] = mean.z;
			if (rgba_out)
				rgba_out[i] = ::pack(::vec3{ std::sqrt(mean.x), std::sqrt(mean.y), std::sqrt(mean.z) });
		}
	if (active_pixels)
		*active_pixels = active;
	return RT_HIP_OK;
}
}
