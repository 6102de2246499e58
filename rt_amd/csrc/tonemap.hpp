// rt_amd/csrc/tonemap.hpp — the host-only half of tone mapping: the default parameters, what a caller's parameters
// are refused for, and the CURVE[:EXPOSURE] parser.  Plain C++17, no HIP header: tonemap.cpp is built with the host compiler into
// librt_hip.so and, on the CPU, into tests/native/libtonemap_reference.so and the program of `make sanitize-tonemap`.
#pragma once

#include <stdint.h>
#include "../../include/rt_hip.h"

namespace rt_hip
{
	rt_hip_tonemap_params default_tonemap_params();

	struct tonemap_check
	{
		rt_hip_status status; // RT_HIP_OK, or RT_HIP_INVALID_ARGUMENT with
		char message[200];	  // ... a text that names the field (the parser: that quotes the text)
	};
	tonemap_check check_tonemap_params(const rt_hip_tonemap_params& params);
	// rt_hip_tonemap_from_spec without the error channel: `out` is written only on success
	tonemap_check tonemap_from_spec(const char* spec, rt_hip_tonemap_params* out);
}
