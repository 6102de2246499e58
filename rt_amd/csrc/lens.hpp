// rt_amd/csrc/lens.hpp — the thin lens' host-only rules (RT_HIP_FLAG_THIN_LENS): what a lens may hold, whether a frame
// with the flag may use the context's, the text form of a lens (rt_hip_lens_from_spec) and the ten words the lens builds of the
// kernels are handed, derived in binary64 from the frame's matrix.  Plain C++17, no HIP header: built with the host compiler into
// librt_hip.so and, on the CPU, into tests/native/lens_plan_dump and the sanitizer program of `make sanitize-lens`.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include "../../include/rt_hip.h"
#include "frame_setup.hpp"

namespace rt_hip
{
	// (context.hip's; a stand-alone program that links lens.cpp brings its own)
	rt_hip_status fail(rt_hip_status status, const char* format, ...) __attribute__((format(printf, 2, 3)));

	struct lens_check
	{
		rt_hip_status status; // RT_HIP_OK, or the refusal's status with
		char message[256];	  // ... the text fail() is given
	};

	// aperture_radius finite and >= 0, focus_distance finite and > 0; the message names the offending field
	lens_check check_lens(const char* entry_point, const rt_hip_lens& lens);
	// a frame with RT_HIP_FLAG_THIN_LENS against the context's state and the frame's camera: no lens set (RT_HIP_INVALID_ARGUMENT), or a
	// matrix without a finite eye (RT_HIP_UNSUPPORTED: the frame would take the homogeneous form, whose words the lens words travel in)
	lens_check check_lens_frame(const char* entry_point, bool have_lens, const frame_params& frame);
	// rt_hip_lens_from_spec without the error channel
	lens_check lens_from_spec(const char* spec, rt_hip_lens* out_lens);

	// The ten binary32 words of a lens frame, each rounded ONCE from binary64: U = aperture * right, V = aperture * up, fwd, focus.
	// right, up and fwd are read off the frame's near plane: with E the frame's eye (frame_params::ray_eye for a pinhole, eye_e for the
	// eye form) and near(px, py) the un-projected depth-0 point of the pixel position (px, py),
	//   right = normalised near(cx + 1, cy) - near(cx, cy),  up = normalised -(near(cx, cy + 1) - near(cx, cy)),  (cx, cy) = (W / 2, H / 2)
	//   fwd   = right x up, normalised, negated if fwd . (near(cx, cy) - E) is not > 0
	struct lens_words
	{
		float u[3], v[3], fwd[3], focus;
	};
	lens_words make_lens_words(const frame_params& frame, const float inverse_view_projection[16], const rt_hip_lens& lens);
	// WHERE they travel: a lens frame never takes the homogeneous camera form (check_lens_frame), so the sixteen words only that form
	// reads — frame_params::mx, my, k_near, k_far — are free: mx[0..2] = U, mx[3] = focus, my[0..2] = V, k_near[0..2] = fwd; the rest 0.
	// No kernel argument is added or moved.
	void put_lens_words(frame_params& frame, const lens_words& words);
}
