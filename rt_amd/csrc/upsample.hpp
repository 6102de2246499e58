// rt_amd/csrc/upsample.hpp — the host-only half of guided upsampling: the default parameters, what a caller's
// parameters and sizes are refused for, and the low-size rule.  Plain C++17, no HIP header: upsample.cpp is built with the host
// compiler into librt_hip.so and, on the CPU, into tests/native/libupsample_reference.so and the program of `make sanitize-upsample`.
#pragma once

#include <stdint.h>
#include "../../include/rt_hip.h"

namespace rt_hip
{
	rt_hip_upsample_params default_upsample_params();

	struct upsample_check
	{
		rt_hip_status status; // RT_HIP_OK, or RT_HIP_INVALID_ARGUMENT with
		char message[160];	  // ... a text that names the field
	};
	upsample_check check_upsample_params(const rt_hip_upsample_params& params);
	// 1 <= w <= W <= 2^22 and 1 <= h <= H <= 2^22
	upsample_check check_upsample_sizes(uint32_t full_width, uint32_t full_height, uint32_t low_width, uint32_t low_height);
	// w = ceil(W / factor), h = ceil(H / factor); factor 1 .. 4
	upsample_check upsample_low_size(uint32_t full_width, uint32_t full_height, uint32_t factor, uint32_t* low_width, uint32_t* low_height);
}
