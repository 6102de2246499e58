// rt_amd/csrc/lights.hpp — emissive materials' host-only rules (RT_HIP_FLAG_EMISSION): what an emission table may
// hold, which of its rows are lights, whether a frame with the flag may use it, and the text form of a table
// (rt_hip_lights_from_spec).  Plain C++17, no HIP header: built with the host compiler into librt_hip.so and, on the CPU, into
// tests/native/light_plan_dump and the sanitizer program of `make sanitize-lights`.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include "../../include/rt_hip.h"

namespace rt_hip
{
	// (context.hip's; a stand-alone program that links lights.cpp brings its own)
	rt_hip_status fail(rt_hip_status status, const char* format, ...) __attribute__((format(printf, 2, 3)));

	struct light_check
	{
		rt_hip_status status; // RT_HIP_OK, or the refusal's status with
		char message[256];	  // ... the text fail() is given
	};

	// every component finite and >= 0 (-0.0f passes); the message names the offending material index and component
	light_check check_emission_values(const float* emission_rgb, uint32_t n_materials);
	// a material IS A LIGHT iff r > 0 || g > 0 || b > 0
	inline bool is_light(const float* rgb) { return rgb[0] > 0.0f || rgb[1] > 0.0f || rgb[2] > 0.0f; }
	uint32_t count_lights(const float* emission_rgb, uint32_t n_materials);
	// a frame with RT_HIP_FLAG_EMISSION against the context's table: no table, or a row count that is not the resident scene's
	light_check check_emission_table(const char* entry_point, bool have_table, uint32_t table_rows, uint32_t scene_materials);
	// rt_hip_lights_from_spec without the error channel
	light_check lights_from_spec(const char* spec, const char* const* material_names, uint32_t n_materials, float* out_emission_rgb);
}
