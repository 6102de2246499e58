// rt_amd/csrc/adaptive.hpp — the host-only half of adaptive sampling: the default parameters and what a caller's
// parameters are refused for, and the sequencing of an adaptive accumulation — which samples the next call traces, when the
// accumulation starts again, when it is complete.  Plain C++17, no HIP header: adaptive.cpp is built with the host compiler into
// librt_hip.so and, on the CPU, into tests/native/adaptive_plan_dump and tests/native/libadaptive_reference.so
// (tests/test_adaptive_host.py holds every rule).
#pragma once

#include <stdint.h>
#include "../../include/rt_hip.h"
#include "progressive.hpp" // (frame_key, refused_pass_flag, pass_max_samples_per_pixel)

namespace rt_hip
{
	// threshold 0.03, floor 0.01, min_samples 32: what a CPU simulation on oracle frames used — not chosen from a GPU run
	rt_hip_adaptive_params default_adaptive_params();

	// the pass size an accumulation runs with: pass_samples rounded up to whole chunks (0 = one chunk); 64 bits, pass_samples may be anything
	uint64_t adaptive_pass_size(uint32_t pass_samples);

	struct adaptive_check
	{
		rt_hip_status status; // RT_HIP_OK, or RT_HIP_INVALID_ARGUMENT with
		char message[160];	  // ... a text that names the field
	};
	// `pass_size`: adaptive_pass_size() of the accumulation (min_samples is at least two passes)
	adaptive_check check_adaptive_params(const rt_hip_adaptive_params& params, uint64_t pass_size);

	// The flags an adaptive pass takes are exactly the passes' (refused_pass_flag, progressive.hpp): the name of one it does not take, or NULL
	inline const char* refused_adaptive_flag(uint32_t flags) { return refused_pass_flag(flags); }

	// everything the pixels AND the sample map of an adaptive accumulation depend on
	struct adaptive_key
	{
		frame_key frame;					   // (samples_per_pixel is the cap)
		uint32_t threshold_bits, floor_bits;   // the parameters, compared as bit patterns
		uint32_t min_samples;
		uint32_t pass_samples;				   // adaptive_pass_size()
	};
	adaptive_key make_adaptive_key(const frame_key& frame, const rt_hip_adaptive_params& params, uint32_t pass_size);
	bool same_adaptive(const adaptive_key& a, const adaptive_key& b);

	// the accumulation in flight
	struct adaptive_state
	{
		bool started = false; // false: nothing in flight (a new context, or a pass that failed)
		adaptive_key key{};
		uint32_t samples_done = 0;	// what an active pixel holds: a multiple of the pass size, or the cap
		uint32_t active_pixels = 0; // after the last pass
		uint32_t passes = 0;
		uint64_t samples_traced = 0;
	};

	struct adaptive_step
	{
		bool restart;		   // the key differs from the state's (or nothing was in flight): the accumulation starts again at sample 0
		uint32_t first_sample; // the pass traces samples [first_sample, first_sample + n_samples) of the active pixels
		uint32_t n_samples;	   // 0: the accumulation is complete, nothing is launched
		bool whole_pass;	   // n_samples is the pass size: the pixels are judged after it (a short last pass judges nobody)
	};
	adaptive_step next_adaptive_pass(const adaptive_state& state, const adaptive_key& wanted);
	// complete: no pixel is active, or the cap is reached
	bool adaptive_complete(uint32_t cap, uint32_t samples_done, uint32_t active_pixels);
}
