// rt_amd/csrc/denoise.cpp — the denoiser's parameters (denoise.hpp): host-only, plain C++17.
#include "denoise.hpp"

#include <cmath>
#include <cstdio>

namespace rt_hip
{
	// The winner of the table in DESIGN.md §3.8 (mean squared error against 1024-spp frames of basic.toml and dielectric.toml at
	// 96 x 54, 16-spp input, evaluated on the CPU with tests/native/denoise_reference.cpp): a table's winner, not a promise of quality.
	// (Those 16-spp frames are already close to the truth — a mean squared error of 1e-4 — and every wider or deeper filter the table holds, the
	// first guess of 4 iterations at 0.6 / 0.1 / 0.05 included, blurs more shading than it removes noise: hence ONE narrow iteration.)
	rt_hip_denoise_params default_denoise_params()
	{
		rt_hip_denoise_params p{};
		p.iterations = 1;
		p.normal_squarings = 3;
		p.sigma_colour = 0.2f;
		p.sigma_albedo = 0.1f;
		p.sigma_depth = 0.02f;
		return p;
	}

	denoise_check check_denoise_params(const rt_hip_denoise_params& p)
	{
		denoise_check c{};
		c.status = RT_HIP_OK;
		const auto refuse = [&c](const char* field, const char* why, double value)
		{
			c.status = RT_HIP_INVALID_ARGUMENT;
			std::snprintf(c.message, sizeof c.message, "rt_hip_denoise_params: %s = %g %s", field, value, why);
		};
		const auto bad_sigma = [](float s) { return !std::isfinite(s) || !(s > 0.0f); };
		if (p.iterations > 6u)
			refuse("iterations", "is more than 6 (taps 2^i pixels apart: the seventh iteration would reach 128 pixels)", p.iterations);
		else if (p.normal_squarings > 8u)
			refuse("normal_squarings", "is more than 8", p.normal_squarings);
		else if (bad_sigma(p.sigma_colour))
			refuse("sigma_colour", "is not a positive finite number", p.sigma_colour);
		else if (bad_sigma(p.sigma_albedo))
			refuse("sigma_albedo", "is not a positive finite number", p.sigma_albedo);
		else if (bad_sigma(p.sigma_depth))
			refuse("sigma_depth", "is not a positive finite number", p.sigma_depth);
		return c;
	}
}
