// tests/native/tonemap_reference.cpp — the CPU restatement of tone mapping.  TEST INFRASTRUCTURE, built with g++ alone
// into tests/native/libtonemap_reference.so (tests/tonemap_reference.py binds it) and into the program of `make sanitize-tonemap`.
//
// The operation is rt_amd/csrc/tonemap_rules.hpp — the very text the kernels of rt_amd/csrc/tonemap.hip run — applied serially, pixel
// after pixel, from plain arrays: one loop fills the histogram, the meter and the adaptation run once, one loop maps the pixels.  Its
// leaf function is the ORACLE's: this file includes oracle/cpu_ref.cpp (as tests/native/upsample_reference.cpp does) and finishes a
// pixel with its square root and its pack(), where the kernel uses contract.hpp's; neither side restates them.  The parameter check
// and the parser are rt_amd/csrc/tonemap.cpp as it is, compiled in by the Makefile.  The device's result must equal what comes out
// here bit for bit (tests/test_gpu_tonemap.py).
#include "../../include/rt_hip.h"

// the oracle's entry points come along under names of their own
#define oracle_render tonemap_ref_oracle_render
#define oracle_closest_hit tonemap_ref_oracle_closest_hit
#define oracle_random tonemap_ref_oracle_random
#define oracle_stream_keys tonemap_ref_oracle_stream_keys
#define oracle_sqrt_div tonemap_ref_oracle_sqrt_div
#define oracle_inv_sqrt tonemap_ref_oracle_inv_sqrt
#define oracle_inv_sqrt_step tonemap_ref_oracle_inv_sqrt_step
#define oracle_pack tonemap_ref_oracle_pack
#define oracle_sky tonemap_ref_oracle_sky
#define oracle_primary_ray tonemap_ref_oracle_primary_ray
#define oracle_frame_constants tonemap_ref_oracle_frame_constants
#define oracle_dielectric_direction tonemap_ref_oracle_dielectric_direction
#define oracle_hits_box tonemap_ref_oracle_hits_box
#define oracle_render_census tonemap_ref_oracle_render_census
#define oracle_unit_vector tonemap_ref_oracle_unit_vector
#include "../../oracle/cpu_ref.cpp"

namespace rt_hip
{
namespace tonemap
{
	namespace leaf
	{
		inline uint32_t pack_mean(float r, float g, float b) { return ::pack(::vec3{ std::sqrt(r), std::sqrt(g), std::sqrt(b) }); }
	}
}
}
#include "../../rt_amd/csrc/tonemap_rules.hpp"
#include "../../rt_amd/csrc/tonemap.hpp"

#include <cstdio>

using namespace rt_hip;

extern "C" {

void tonemap_ref_default_params(rt_hip_tonemap_params* out) { *out = default_tonemap_params(); }

// check_tonemap_params: the status, and the message into `message` (may be NULL)
int tonemap_ref_check(const rt_hip_tonemap_params* params, char* message, size_t size)
{
	const tonemap_check c = check_tonemap_params(*params);
	if (message && size)
		std::snprintf(message, size, "%s", c.message);
	return c.status;
}

int tonemap_ref_from_spec(const char* spec, rt_hip_tonemap_params* out, char* message, size_t size)
{
	const tonemap_check c = tonemap_from_spec(spec, out);
	if (message && size)
		std::snprintf(message, size, "%s", c.message);
	return c.status;
}

// the meter's first half alone: 257 words, the bins and the skipped pixels
void tonemap_ref_histogram(uint32_t pixels, const float* rgb, uint32_t* histogram)
{
	for (uint32_t b = 0; b < tonemap::histogram_words; b++)
		histogram[b] = 0u;
	for (size_t i = 0; i < pixels; i++)
	{
		const float y = tonemap::luminance(rgb[i * 3], rgb[i * 3 + 1], rgb[i * 3 + 2]);
		histogram[tonemap::counted(y) ? tonemap::bin_of(y) : tonemap::bins]++;
	}
}

// the whole operation, serially: rt_hip_tonemap_device's arguments on host arrays (params NULL = defaults; either output may be NULL,
// rgb_out may be rgb_in).  `state`: the 8-word record, read (word 0) and written as the device reads and writes it.  Returns the
// parameters' refusal; nothing is written when it refuses.
int tonemap_ref_frame(uint32_t width, uint32_t height, const float* rgb_in, const rt_hip_tonemap_params* params, uint32_t* state, float* rgb_out, uint32_t* rgba_out)
{
	const rt_hip_tonemap_params p = params ? *params : default_tonemap_params();
	if (const tonemap_check c = check_tonemap_params(p); c.status)
		return c.status;
	if (!width || !height)
		return RT_HIP_INVALID_ARGUMENT;
	const size_t pixels = static_cast<size_t>(width) * height;
	if (p.exposure > 0.0f)
	{
		state[0] = state[1] = tonemap::bits_of(p.exposure);
		for (uint32_t w = 2; w < tonemap::state_words; w++)
			state[w] = 0u;
	}
	else
	{
		uint32_t histogram[tonemap::histogram_words];
		tonemap_ref_histogram(static_cast<uint32_t>(pixels), rgb_in, histogram);
		const tonemap::metered m = tonemap::meter(histogram, p);
		const float exposure = tonemap::adapt(state[0], m.target, p.adaptation);
		state[0] = tonemap::bits_of(exposure);
		state[1] = tonemap::bits_of(m.target);
		state[2] = m.counted;
		state[3] = histogram[tonemap::bins];
		state[4] = m.kept;
		state[5] = m.mean_q8;
		state[6] = state[7] = 0u;
	}
	const float exposure = tonemap::float_of(state[0]), white2 = p.white * p.white;
	for (size_t i = 0; i < pixels; i++)
	{
		const tonemap::rgb o = tonemap::map_pixel(rgb_in[i * 3], rgb_in[i * 3 + 1], rgb_in[i * 3 + 2], exposure, p.curve, white2);
		if (rgb_out)
			rgb_out[i * 3] = o.r, rgb_out[i * 3 + 1] = o.g, rgb_out[i * 3 + 2] = o.b;
		if (rgba_out)
			rgba_out[i] = tonemap::finish(o);
	}
	return RT_HIP_OK;
}
}
