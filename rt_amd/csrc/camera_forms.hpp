// rt_amd/csrc/camera_forms.hpp — the three camera forms of render_queue (frame_params, frame_setup.hpp): which form a build takes for a
// frame, and what a pixel's samples start from (camera_base: once per item).  Every build of render_queue uses it; a scalar-register
// build and the resident LDS-scan build are compiled for ONE form (queue_build: PINHOLE_ONLY, EYE_ONLY, NEVER_PINHOLE), the others choose
// by the frame's own words, wave-uniformly.  The primary ray per restart takes the same selection but stays in render_queue's fused tail,
// condition and all: as a function here — four signatures tried — and even with only its condition taken from here, the compiler
// allocated and scheduled most kernels differently.
#pragma once

#include "contract.hpp"
#include "kernels.hpp"
#include "lane_state.hpp"

namespace rt_hip
{
	// the form selection: pinhole first, then the eye form, else the homogeneous form (wave-uniform: kernel arguments)
	template <class BUILD>
	__device__ __forceinline__ bool camera_is_pinhole(const frame_params& p)
	{
		return BUILD::PINHOLE_ONLY || (!BUILD::EYE_ONLY && !BUILD::NEVER_PINHOLE && p.pinhole);
	}
	template <class BUILD>
	__device__ __forceinline__ bool camera_has_eye(const frame_params& p) // (asked where camera_is_pinhole said no)
	{
		return BUILD::EYE_ONLY || p.eye_form;
	}

	// what the samples of the pixel at column fx, image row fy start from: lane_state's base words
	template <class BUILD>
	__device__ __forceinline__ void camera_base(lane_state& st, const frame_params& p, float fx, float fy)
	{
		if (camera_is_pinhole<BUILD>(p))
		{
			st.base_x = fma(p.ray_d1[0], fx, fma(p.ray_d2[0], fy, p.ray_d0[0]));
			st.base_y = fma(p.ray_d1[1], fx, fma(p.ray_d2[1], fy, p.ray_d0[1]));
			st.base_z = fma(p.ray_d1[2], fx, fma(p.ray_d2[2], fy, p.ray_d0[2]));
			st.base_w = 0.0f;
		}
		else if (camera_has_eye<BUILD>(p))
		{
			st.base_x = fma(p.eye_q1[0], fx, fma(p.eye_q2[0], fy, p.eye_q0[0]));
			st.base_y = fma(p.eye_q1[1], fx, fma(p.eye_q2[1], fy, p.eye_q0[1]));
			st.base_z = fma(p.eye_q1[2], fx, fma(p.eye_q2[2], fy, p.eye_q0[2]));
			st.base_w = fma(p.eye_w1, fx, fma(p.eye_w2, fy, p.eye_w0));
		}
		else
		{
			st.base_x = fx, st.base_y = fy;
			st.base_z = st.base_w = 0.0f;
		}
	}
}
