// rt_amd/csrc/adaptive.cpp — adaptive sampling's host-only rules (adaptive.hpp): plain C++17.
#include "adaptive.hpp"
#include "launch_plan.hpp" // (sample_chunk)

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace rt_hip
{
	rt_hip_adaptive_params default_adaptive_params()
	{
		rt_hip_adaptive_params p{};
		p.threshold = 0.03f;
		p.floor = 0.01f;
		p.min_samples = 32;
		return p;
	}

	uint64_t adaptive_pass_size(uint32_t pass_samples)
	{
		const uint64_t wanted = pass_samples ? pass_samples : sample_chunk;
		return (wanted + sample_chunk - 1u) / sample_chunk * sample_chunk;
	}

	adaptive_check check_adaptive_params(const rt_hip_adaptive_params& p, uint64_t pass_size)
	{
		adaptive_check c{};
		c.status = RT_HIP_OK;
		const auto refuse = [&c](const char* field, const char* why, double value)
		{
			c.status = RT_HIP_INVALID_ARGUMENT;
			std::snprintf(c.message, sizeof c.message, "rt_hip_adaptive_params: %s = %g %s", field, value, why);
		};
		if (!std::isfinite(p.threshold) || !(p.threshold >= 0.0f))
			refuse("threshold", "is not a finite number >= 0", p.threshold);
		else if (!std::isfinite(p.floor) || !(p.floor >= 0.0f))
			refuse("floor", "is not a finite number >= 0", p.floor);
		else if (p.min_samples < 2u * pass_size)
		{
			c.status = RT_HIP_INVALID_ARGUMENT;
			std::snprintf(c.message, sizeof c.message, "rt_hip_adaptive_params: min_samples = %u is less than two passes of %llu samples", p.min_samples, static_cast<unsigned long long>(pass_size));
		}
		return c;
	}

	adaptive_key make_adaptive_key(const frame_key& frame, const rt_hip_adaptive_params& params, uint32_t pass_size)
	{
		adaptive_key k{};
		k.frame = frame;
		std::memcpy(&k.threshold_bits, &params.threshold, sizeof k.threshold_bits);
		std::memcpy(&k.floor_bits, &params.floor, sizeof k.floor_bits);
		k.min_samples = params.min_samples;
		k.pass_samples = pass_size;
		return k;
	}

	bool same_adaptive(const adaptive_key& a, const adaptive_key& b)
	{
		return same_frame(a.frame, b.frame) && a.threshold_bits == b.threshold_bits && a.floor_bits == b.floor_bits && a.min_samples == b.min_samples && a.pass_samples == b.pass_samples;
	}

	bool adaptive_complete(uint32_t cap, uint32_t samples_done, uint32_t active_pixels) { return active_pixels == 0u || samples_done >= cap; }

	adaptive_step next_adaptive_pass(const adaptive_state& state, const adaptive_key& wanted)
	{
		adaptive_step step{};
		step.restart = !state.started || !same_adaptive(state.key, wanted);
		const uint32_t cap = wanted.frame.samples_per_pixel;
		step.first_sample = step.restart ? 0u : std::min(state.samples_done, cap);
		if (!step.restart && adaptive_complete(cap, state.samples_done, state.active_pixels))
		{
			step.n_samples = 0u;
			step.whole_pass = false;
			return step;
		}
		step.n_samples = std::min(wanted.pass_samples, cap - step.first_sample);
		step.whole_pass = step.n_samples == wanted.pass_samples;
		return step;
	}
}
