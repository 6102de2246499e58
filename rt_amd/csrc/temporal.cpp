// rt_amd/csrc/temporal.cpp — temporal accumulation's host-only rules (temporal.hpp): plain C++17.
#include "temporal.hpp"

#include <cmath>
#include <cstdio>

namespace rt_hip
{
	// The winner of the table in DESIGN.md §3.9 (mean squared error of eight blended 16-spp frames against the 1024-spp frame of the last
	// camera, basic.toml and dielectric.toml at 96 x 54, camera at rest and on a dolly, evaluated on the CPU with
	// tests/native/reproject_reference.cpp by tools/temporal_tune.py): a table's winner, not a promise of quality.
	rt_hip_temporal_params default_temporal_params()
	{
		rt_hip_temporal_params p{};
		p.max_history_samples = 16;
		p.position_tolerance = 0.05f;
		p.normal_threshold = 0.9f;
		return p;
	}

	temporal_check check_temporal_params(const rt_hip_temporal_params& p)
	{
		temporal_check c{};
		c.status = RT_HIP_OK;
		const auto refuse = [&c](const char* field, const char* why, double value)
		{
			c.status = RT_HIP_INVALID_ARGUMENT;
			std::snprintf(c.message, sizeof c.message, "rt_hip_temporal_params: %s = %g %s", field, value, why);
		};
		if (p.max_history_samples < 1u || p.max_history_samples > (1u << 20))
			refuse("max_history_samples", "is not in 1 .. 1048576", p.max_history_samples);
		else if (!std::isfinite(p.position_tolerance) || !(p.position_tolerance > 0.0f))
			refuse("position_tolerance", "is not a positive finite number", p.position_tolerance);
		else if (!(p.normal_threshold >= -1.0f && p.normal_threshold <= 1.0f))
			refuse("normal_threshold", "is not in -1 .. 1", p.normal_threshold);
		return c;
	}

	temporal_check forward_view_projection(const float inverse[16], float out[16])
	{
		temporal_check c{};
		c.status = RT_HIP_OK;
		double a[4][8];
		for (int r = 0; r < 4; r++)
			for (int k = 0; k < 4; k++)
			{
				if (!std::isfinite(inverse[r * 4 + k]))
				{
					c.status = RT_HIP_INVALID_ARGUMENT;
					std::snprintf(c.message, sizeof c.message, "forward_view_projection: element [%d][%d] of the matrix is not finite", r, k);
					return c;
				}
				a[r][k] = inverse[r * 4 + k];
				a[r][4 + k] = r == k ? 1.0 : 0.0;
			}
		for (int col = 0; col < 4; col++)
		{
			int pivot = col;
			for (int r = col + 1; r < 4; r++)
				if (std::fabs(a[r][col]) > std::fabs(a[pivot][col]))
					pivot = r;
			if (a[pivot][col] == 0.0)
			{
				c.status = RT_HIP_INVALID_ARGUMENT;
				std::snprintf(c.message, sizeof c.message, "forward_view_projection: the matrix is singular (no pivot in column %d)", col);
				return c;
			}
			for (int k = 0; k < 8; k++)
			{
				const double t = a[col][k];
				a[col][k] = a[pivot][k];
				a[pivot][k] = t;
			}
			const double d = a[col][col];
			for (int k = 0; k < 8; k++)
				a[col][k] /= d;
			for (int r = 0; r < 4; r++)
			{
				if (r == col)
					continue;
				const double f = a[r][col];
				for (int k = 0; k < 8; k++)
					a[r][k] -= f * a[col][k];
			}
		}
		float rounded[16];
		for (int r = 0; r < 4; r++)
			for (int k = 0; k < 4; k++)
			{
				rounded[r * 4 + k] = static_cast<float>(a[r][4 + k]);
				if (!std::isfinite(rounded[r * 4 + k]))
				{
					c.status = RT_HIP_INVALID_ARGUMENT;
					std::snprintf(c.message, sizeof c.message, "forward_view_projection: the matrix is singular to float precision (element [%d][%d] of its inverse is not finite)", r, k);
					return c;
				}
			}
		for (int i = 0; i < 16; i++)
			out[i] = rounded[i];
		return c;
	}

	bool same_history(const frame_key& a, const frame_key& b)
	{
		return a.scene_fingerprint == b.scene_fingerprint && a.max_bounces == b.max_bounces && a.width == b.width && a.height == b.height && (a.flags & history_frame_flags) == (b.flags & history_frame_flags);
	}
}
