// rt_amd/csrc/upsample.cpp — guided upsampling's parameters, size checks and low-size rule (upsample.hpp): host-only, plain C++17.
#include "upsample.hpp"

#include <cmath>
#include <cstdio>

namespace rt_hip
{
	namespace
	{
		constexpr uint32_t max_side = 1u << 22; // (upsample_rules.hpp's: every integer of the geometry is exact as a float)
		constexpr uint32_t max_factor = 4;
	}

	// The shared names start from the denoiser's defaults (denoise.cpp); min_weight is the winner of the table in DESIGN.md §3.14
	// (mean squared error against the oracle's full-size high-sample frames of three scenes at 96 x 54, rebuilt from factor-2, -3 and
	// -4 frames on the CPU with tests/native/upsample_reference.cpp): a table's winner, not a promise of quality.
	rt_hip_upsample_params default_upsample_params()
	{
		rt_hip_upsample_params p{};
		p.normal_squarings = 3;
		p.sigma_albedo = 0.1f;
		p.sigma_depth = 0.02f;
		p.min_weight = 0.00006103515625f; // 2^-14
		return p;
	}

	upsample_check check_upsample_params(const rt_hip_upsample_params& p)
	{
		upsample_check c{};
		c.status = RT_HIP_OK;
		const auto refuse = [&c](const char* field, const char* why, double value)
		{
			c.status = RT_HIP_INVALID_ARGUMENT;
			std::snprintf(c.message, sizeof c.message, "rt_hip_upsample_params: %s = %g %s", field, value, why);
		};
		const auto bad_sigma = [](float s) { return !std::isfinite(s) || !(s > 0.0f); };
		if (p.normal_squarings > 8u)
			refuse("normal_squarings", "is more than 8", p.normal_squarings);
		else if (bad_sigma(p.sigma_albedo))
			refuse("sigma_albedo", "is not a positive finite number", p.sigma_albedo);
		else if (bad_sigma(p.sigma_depth))
			refuse("sigma_depth", "is not a positive finite number", p.sigma_depth);
		else if (!(p.min_weight > 0.0f) || !(p.min_weight <= 1.0f))
			refuse("min_weight", "is not in (0, 1]", p.min_weight);
		return c;
	}

	upsample_check check_upsample_sizes(uint32_t W, uint32_t H, uint32_t w, uint32_t h)
	{
		upsample_check c{};
		c.status = RT_HIP_OK;
		if (!W || !H || W > max_side || H > max_side)
		{
			c.status = RT_HIP_INVALID_ARGUMENT;
			std::snprintf(c.message, sizeof c.message, "full frame %ux%u (1 .. %u a side)", W, H, max_side);
		}
		else if (!w || !h || w > W || h > H)
		{
			c.status = RT_HIP_INVALID_ARGUMENT;
			std::snprintf(c.message, sizeof c.message, "low frame %ux%u for a full frame of %ux%u (1 .. the full frame's side)", w, h, W, H);
		}
		return c;
	}

	upsample_check upsample_low_size(uint32_t W, uint32_t H, uint32_t factor, uint32_t* w, uint32_t* h)
	{
		upsample_check c{};
		c.status = RT_HIP_OK;
		if (!w || !h)
		{
			c.status = RT_HIP_INVALID_ARGUMENT;
			std::snprintf(c.message, sizeof c.message, "NULL argument");
		}
		else if (!factor || factor > max_factor)
		{
			c.status = RT_HIP_INVALID_ARGUMENT;
			std::snprintf(c.message, sizeof c.message, "factor = %u (1 .. %u)", factor, max_factor);
		}
		else if (!W || !H || W > max_side || H > max_side)
		{
			c.status = RT_HIP_INVALID_ARGUMENT;
			std::snprintf(c.message, sizeof c.message, "full frame %ux%u (1 .. %u a side)", W, H, max_side);
		}
		else
		{
			*w = (W + factor - 1u) / factor;
			*h = (H + factor - 1u) / factor;
		}
		return c;
	}
}
