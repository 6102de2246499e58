// tests/native/reproject_reference.cpp — the CPU restatement of temporal accumulation.  TEST INFRASTRUCTURE, built with
// g++ alone into tests/native/libreproject_reference.so (tests/reproject_reference.py binds it).
//
// The rule is rt_amd/csrc/reproject_rules.hpp — the very text reproject_frame of rt_amd/csrc/temporal.hip runs per pixel — applied
// serially, pixel after pixel, from plain arrays.  Its leaf functions are the ORACLE's: this file includes oracle/cpu_ref.cpp (as
// tests/native/denoise_reference.cpp does) and hands its dot() to the rule, and the pixel's centre ray is oracle_primary_ray's; the
// kernel hands in contract.hpp's and builds the ray as guide_frame does.  Parameters, the forward view-projection and same_history
// are rt_amd/csrc/temporal.cpp as it is, compiled in by the Makefile.  The device's result must equal what comes out here bit for
// bit (tests/test_gpu_temporal.py).
#include "../../include/rt_hip.h"

// the oracle's entry points come along under names of their own
#define oracle_render reproject_ref_oracle_render
#define oracle_closest_hit reproject_ref_oracle_closest_hit
#define oracle_random reproject_ref_oracle_random
#define oracle_stream_keys reproject_ref_oracle_stream_keys
#define oracle_sqrt_div reproject_ref_oracle_sqrt_div
#define oracle_inv_sqrt reproject_ref_oracle_inv_sqrt
#define oracle_inv_sqrt_step reproject_ref_oracle_inv_sqrt_step
#define oracle_pack reproject_ref_oracle_pack
#define oracle_sky reproject_ref_oracle_sky
#define oracle_primary_ray reproject_ref_oracle_primary_ray
#define oracle_frame_constants reproject_ref_oracle_frame_constants
#define oracle_dielectric_direction reproject_ref_oracle_dielectric_direction
#define oracle_hits_box reproject_ref_oracle_hits_box
#define oracle_render_census reproject_ref_oracle_render_census
#define oracle_unit_vector reproject_ref_oracle_unit_vector
#include "../../oracle/cpu_ref.cpp"

namespace rt_hip
{
namespace reproject
{
	namespace leaf
	{
		inline float dot3(float ax, float ay, float az, float bx, float by, float bz) { return ::dot(::vec3{ ax, ay, az }, ::vec3{ bx, by, bz }); }
		inline float fma(float a, float b, float c) { return std::fmaf(a, b, c); }
		inline bool is_finite(float f) { return std::isfinite(f); }
	}
}
}
#include "../../rt_amd/csrc/reproject_rules.hpp"
#include "../../rt_amd/csrc/temporal.hpp"

#include <cstdio>
#include <cstring>

using namespace rt_hip;

namespace
{
	struct history_fetch
	{
		const float* rgb;
		const float* records;
		int32_t width;
		reproject::tap operator()(int32_t x, int32_t y) const
		{
			const size_t pixel = static_cast<size_t>(y) * static_cast<size_t>(width) + static_cast<size_t>(x);
			const float* const r = records + pixel * reproject::record_words;
			uint32_t id;
			std::memcpy(&id, r + 7, sizeof id);
			return { { r[0], r[1], r[2], r[3], r[4], r[5], r[6], id }, { rgb[pixel * 3], rgb[pixel * 3 + 1], rgb[pixel * 3 + 2] } };
		}
	};
}

extern "C" {

void reproject_ref_default_params(rt_hip_temporal_params* out) { *out = default_temporal_params(); }

// check_temporal_params: the status, and the message into `message` (may be NULL)
int reproject_ref_check(const rt_hip_temporal_params* params, char* message, size_t size)
{
	const temporal_check c = check_temporal_params(*params);
	if (message && size)
		std::snprintf(message, size, "%s", c.message);
	return c.status;
}

// forward_view_projection: the status, the matrix into `out` (left alone on refusal), the message into `message` (may be NULL)
int reproject_ref_forward(const float* inverse, float* out, char* message, size_t size)
{
	const temporal_check c = forward_view_projection(inverse, out);
	if (message && size)
		std::snprintf(message, size, "%s", c.message);
	return c.status;
}

// same_history on two keys given field by field (scene_fingerprint, samples_per_pixel, max_bounces, matrix, width, height, seed, flags)
int reproject_ref_same_history(uint64_t print_a, uint32_t spp_a, uint32_t bounces_a, const float* matrix_a, uint32_t width_a, uint32_t height_a, uint64_t seed_a, uint32_t flags_a,
							   uint64_t print_b, uint32_t spp_b, uint32_t bounces_b, const float* matrix_b, uint32_t width_b, uint32_t height_b, uint64_t seed_b, uint32_t flags_b)
{
	frame_key a{}, b{};
	a.scene_fingerprint = print_a, a.samples_per_pixel = spp_a, a.max_bounces = bounces_a, a.width = width_a, a.height = height_a, a.seed = seed_a, a.flags = flags_a;
	b.scene_fingerprint = print_b, b.samples_per_pixel = spp_b, b.max_bounces = bounces_b, b.width = width_b, b.height = height_b, b.seed = seed_b, b.flags = flags_b;
	std::memcpy(a.inverse_view_projection, matrix_a, sizeof a.inverse_view_projection);
	std::memcpy(b.inverse_view_projection, matrix_b, sizeof b.inverse_view_projection);
	return same_history(a, b) ? 1 : 0;
}

// The whole step, serially: rt_hip_reproject_device's arguments on host arrays; `scene` stands for the resident scene (only its matrix
// is read: the current camera).  Returns RT_HIP_OK, or the status the parameters or the previous matrix are refused with — nothing
// is written then.
int reproject_ref_frame(const rt_hip_scene* scene, uint32_t width, uint32_t height, const float* prev_inverse_view_projection, const float* guide, const float* rgb_in, uint32_t samples_in, const float* prev_rgb,
						const float* prev_record, const rt_hip_temporal_params* params, float* rgb_out, float* record_out, uint32_t* pixels_with_history)
{
	const rt_hip_temporal_params p = params ? *params : default_temporal_params();
	if (const temporal_check c = check_temporal_params(p); c.status)
		return c.status;
	if (!samples_in || samples_in > reproject::max_samples_in || (prev_rgb == nullptr) != (prev_record == nullptr))
		return RT_HIP_INVALID_ARGUMENT;
	const bool have_history = prev_rgb != nullptr;
	float P[16] = {};
	if (have_history)
		if (const temporal_check c = forward_view_projection(prev_inverse_view_projection, P); c.status)
			return c.status;
	const reproject::constants k = reproject::constants_of(p);
	const history_fetch fetch = { prev_rgb, prev_record, static_cast<int32_t>(width) };
	uint32_t found = 0;
	for (uint32_t y = 0; y < height; y++)
		for (uint32_t x = 0; x < width; x++)
		{
			const size_t pixel = static_cast<size_t>(y) * width + x;
			const float* const g = guide + pixel * 8;
			uint32_t id;
			std::memcpy(&id, g + 7, sizeof id);
			float origin[3], direction[3];
			oracle_primary_ray(scene, width, height, x, y, 0x1.0p23f, 0x1.0p23f, origin, direction);
			const reproject::result r = reproject::reproject_pixel(static_cast<int32_t>(width), static_cast<int32_t>(height), { g[0], g[1], g[2], g[3], id }, { rgb_in[pixel * 3], rgb_in[pixel * 3 + 1], rgb_in[pixel * 3 + 2] },
																   static_cast<float>(samples_in), { origin[0], origin[1], origin[2], direction[0], direction[1], direction[2] }, P, have_history, k, fetch);
			rgb_out[pixel * 3] = r.out.r, rgb_out[pixel * 3 + 1] = r.out.g, rgb_out[pixel * 3 + 2] = r.out.b;
			float* const o = record_out + pixel * reproject::record_words;
			o[0] = r.rec.px, o[1] = r.rec.py, o[2] = r.rec.pz, o[3] = r.rec.length, o[4] = r.rec.nx, o[5] = r.rec.ny, o[6] = r.rec.nz;
			std::memcpy(o + 7, &r.rec.id, sizeof r.rec.id);
			found += r.had_history ? 1u : 0u;
		}
	if (pixels_with_history)
		*pixels_with_history = found;
	return RT_HIP_OK;
}
}
