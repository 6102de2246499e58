// rt_amd/csrc/denoise.hpp — the host-only half of the denoiser: the default parameters and what a caller's
// parameters are refused for.  Plain C++17, no HIP header: denoise.cpp is built with the host compiler into librt_hip.so and, on
// the CPU, into tests/native/libdenoise_reference.so (tests/test_denoise_reference.py holds every refusal).
#pragma once

#include <stdint.h>
#include "../../include/rt_hip.h"

namespace rt_hip
{
	rt_hip_denoise_params default_denoise_params();

	struct denoise_check
	{
		rt_hip_status status; // RT_HIP_OK, or RT_HIP_INVALID_ARGUMENT with
		char message[160];	  // ... a text that names the field
	};
	denoise_check check_denoise_params(const rt_hip_denoise_params& params);
}
