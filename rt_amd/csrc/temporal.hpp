// rt_amd/csrc/temporal.hpp — the host-only half of temporal accumulation: the default parameters and what a caller's
// parameters are refused for, the forward view-projection of a frame's matrix, and when a history has to start again.  Plain C++17,
// no HIP header: temporal.cpp is built with the host compiler into librt_hip.so and, on the CPU, into
// tests/native/libreproject_reference.so (tests/test_temporal_host.py holds every rule).
#pragma once

#include <stdint.h>
#include "../../include/rt_hip.h"
#include "progressive.hpp" // (frame_key: everything a frame depends on)

namespace rt_hip
{
	rt_hip_temporal_params default_temporal_params();

	struct temporal_check
	{
		rt_hip_status status; // RT_HIP_OK, or RT_HIP_INVALID_ARGUMENT with
		char message[160];	  // ... a text that names the field (or says what is wrong with the matrix)
	};
	temporal_check check_temporal_params(const rt_hip_temporal_params& params);

	// world -> clip from a frame's inverse_view_projection (clip -> world), both [r * 4 + c]: inverted in binary64 by Gauss-Jordan
	// elimination with partial pivoting and rounded once to float.  A singular matrix (a zero pivot) or one with a non-finite element is
	// refused, and `out` is then left alone.  How good the inverse is does not enter the bit-exact contract: the device and the CPU
	// restatement consume the same 16 floats.
	temporal_check forward_view_projection(const float inverse[16], float out[16]);

	// Whether a history made under `a` may be carried into a frame of `b`.  It starts again on any change of the columns' fingerprint,
	// max_bounces, the size, RT_HIP_FLAG_SM_MATERIALS or RT_HIP_FLAG_TRACE_BOXES — what changes the scene a pixel shows, or how it is
	// shaded — and NOT on a change of the matrix (that is what reprojection is for), the seed, samples_per_pixel (the lengths count
	// samples), the BVH flags or RT_HIP_FLAG_STATS (bit-identical frames).
	constexpr uint32_t history_frame_flags = RT_HIP_FLAG_SM_MATERIALS | RT_HIP_FLAG_TRACE_BOXES;
	bool same_history(const frame_key& a, const frame_key& b);
}
