// rt_amd/csrc/bloom.hpp — the host-only half of bloom: the default parameters, what a caller's parameters are
// refused for, the level plan of a frame (sizes, how many levels, norm, gain, where each level lies in the scratch) and the
// key=value parser.  Plain C++17, no HIP header: bloom.cpp is built with the host compiler into librt_hip.so and, on the CPU, into
// tests/native/libbloom_reference.so and the program of `make sanitize-bloom`.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include "../../include/rt_hip.h"
#include "bloom_rules.hpp"

namespace rt_hip
{
	rt_hip_bloom_params default_bloom_params();

	struct bloom_check
	{
		rt_hip_status status; // RT_HIP_OK, or RT_HIP_INVALID_ARGUMENT with
		char message[200];	  // ... a text that names the field (the parser: that quotes the text)
	};
	bloom_check check_bloom_params(const rt_hip_bloom_params& params);
	// rt_hip_bloom_from_spec without the error channel: `out` is written only on success
	bloom_check bloom_from_spec(const char* spec, rt_hip_bloom_params* out);

	// The pyramid of a width x height frame (both >= 1) under checked parameters.  Level 0 is ceil(W / 2) x ceil(H / 2), every next one
	// halves the one before with ceil; there are min(params.levels, the count at which a level first is 1 x 1) of them.  The levels lie
	// back to back in ONE scratch block, 3 floats a texel, level i from float `offset`.
	//   norm = sum over i < levels of scatter^i, in float: norm = 0, term = 1, then `levels` times { norm += term; term *= scatter }
	//   gain = intensity / norm     (norm >= 1: the first term)
	struct bloom_level
	{
		uint32_t width, height;
		size_t offset; // in floats
	};
	struct bloom_plan
	{
		uint32_t levels;
		bloom_level level[bloom::max_levels];
		float norm, gain;
		size_t scratch_bytes;
	};
	bloom_plan plan_bloom(uint32_t width, uint32_t height, const rt_hip_bloom_params& params);
}
