// rt_amd/csrc/sky_band.hpp — the sky band of a frame: how many rows from the top of the image are PROVABLY sky, so that render.hip
// can hand them to the scene-free kernel of sky_band.hip and launch the scene's kernel over the rows below ("The sky
// band").  Host-only: plain C++17, no HIP header, built with the host compiler into librt_hip.so and, on the CPU, into
// tests/native/sky_band_dump (tests/test_sky_band_rule.py holds every claimed row against the oracle's closest-hit query).
#pragma once

#include <stdint.h>
#include "../../include/rt_hip.h" // (the render flags)
#include "frame_setup.hpp"		  // (frame_params: the pinhole constants the kernels trace from)
#include "launch_plan.hpp"		  // (scan_resident)

namespace rt_hip
{
	constexpr uint32_t sky_band_strip_rows = 8;	  // the band is a whole number of these (every tile height of the tile-per-wave kernels divides it)
	constexpr uint32_t sky_band_cell_columns = 64; // a strip's columns are bisected down to this before the strip is given up
	// The rule costs time in proportion to the spheres, the kernels' frames do not: scenes beyond this many take no band
	constexpr uint32_t sky_band_max_spheres = 64;
	constexpr uint32_t sky_band_max_side = 1u << 15; // (a pixel step must stay far above binary32's resolution of the ray constants)

	// The margin of both conditions, relative to the largest term of the expression it guards.  The kernels evaluate
	// e = c - (eye + T), a = e . d, e . e and r^2 - (e . e - a a) in binary32: a few dozen roundings of 2^-24 relative each, every
	// one on a term no larger than twice the scale the margin multiplies — under 2^-19 of it in all, and 2^-12 is more than a
	// hundred times that.  (The rule's own binary64 arithmetic adds 2^-50.)
	constexpr double sky_band_epsilon = 0x1.0p-12;

	// flags under which a frame takes no band: other arithmetic, other kernels, or primitives the rule does not know
	constexpr uint32_t sky_band_excluded_flags = RT_HIP_FLAG_FAST | RT_HIP_FLAG_PREVIEW | RT_HIP_FLAG_TRACE_BOXES | RT_HIP_FLAG_BOX_BVH | RT_HIP_FLAG_EMISSION | RT_HIP_FLAG_BVH | RT_HIP_FLAG_SM_MATERIALS;

	struct sky_band_request
	{
		const float* spheres; // the resident scene's sphere table as the kernels read it: (cx, cy, cz, r^2) per sphere
		uint32_t n_spheres, n_planes;
		uint32_t flags;		  // the launch's RT_HIP_FLAG_*
		bool pass, adaptive;  // the launch is a pass of a progressive frame / an adaptive pass
		int scan;			  // kernel_build::scan of the frame's plan: the band exists for the tile-per-wave kernels (> 0, or scan_resident)
		const frame_params* frame; // as make_frame_params made it
	};

	// R: a multiple of sky_band_strip_rows, 0 <= R <= height.  For every pixel of rows [0, R) and every jitter in [0, 1)^2 the kernels'
	// closest-hit query of the primary ray reports a miss.  0: no band (the gates, or nothing provable).
	uint32_t sky_band_rows(const sky_band_request& request);
}
