// rt_amd/csrc/centre_ray.hpp — the primary ray through a pixel's centre, for the kernels that look at a frame's first hit without
// tracing it: guide_frame (denoise.hip) and reproject_frame (temporal.hip).
//
// The ray is the one the render kernels build for sample 0 (kernels.hip, "restart: primary ray"): through the pixel centre — the
// jitter's numerators are both 2^23 — in the frame's camera form, with the constants make_frame_params derives.  Restated here
// because the render kernels keep it inside their loop; tests/test_gpu_denoise.py holds it to oracle_primary_ray.
#pragma once

#include "contract.hpp"
#include "kernels.hpp"

namespace rt_hip
{
	// (fx, fy): the pixel's coordinates as floats; the camera form is wave-uniform (a kernel argument)
	__device__ __forceinline__ void centre_ray(const frame_params& p, const float fx, const float fy, vec3& origin, vec3& dir)
	{
		const float jx = 0x1.0p23f, jy = 0x1.0p23f;
		vec3 toward;
		if (p.pinhole)
		{
			const vec3 base = { fma(p.ray_d1[0], fx, fma(p.ray_d2[0], fy, p.ray_d0[0])), fma(p.ray_d1[1], fx, fma(p.ray_d2[1], fy, p.ray_d0[1])), fma(p.ray_d1[2], fx, fma(p.ray_d2[2], fy, p.ray_d0[2])) };
			toward = { fma(p.ray_j1[0], jx, fma(p.ray_j2[0], jy, base.x)), fma(p.ray_j1[1], jx, fma(p.ray_j2[1], jy, base.y)), fma(p.ray_j1[2], jx, fma(p.ray_j2[2], jy, base.z)) };
			origin = { p.ray_eye[0] + toward.x, p.ray_eye[1] + toward.y, p.ray_eye[2] + toward.z };
		}
		else if (p.eye_form)
		{
			const vec3 base = { fma(p.eye_q1[0], fx, fma(p.eye_q2[0], fy, p.eye_q0[0])), fma(p.eye_q1[1], fx, fma(p.eye_q2[1], fy, p.eye_q0[1])), fma(p.eye_q1[2], fx, fma(p.eye_q2[2], fy, p.eye_q0[2])) };
			const float base_w = fma(p.eye_w1, fx, fma(p.eye_w2, fy, p.eye_w0));
			toward = { fma(p.eye_jq1[0], jx, fma(p.eye_jq2[0], jy, base.x)), fma(p.eye_jq1[1], jx, fma(p.eye_jq2[1], jy, base.y)), fma(p.eye_jq1[2], jx, fma(p.eye_jq2[2], jy, base.z)) };
			const float ws = fma(p.eye_jw1, jx, fma(p.eye_jw2, jy, base_w));
			// (rcp_rn is the correctly rounded reciprocal for EVERY argument: the plain form's rcp_in_band gives the same bits inside its band)
			const float inv = rcp_rn(ws);
			origin = { fma(toward.x, inv, p.eye_e[0]), fma(toward.y, inv, p.eye_e[1]), fma(toward.z, inv, p.eye_e[2]) };
			if (p.eye_form != 2u && ws * (ws + p.eye_zws) < 0.0f) // the guarded form: near and far points on different sides of w = 0
				toward = { -toward.x, -toward.y, -toward.z };
		}
		else
		{
			const float px = fma(jx, random_scale, fx), py = fma(jy, random_scale, fy);
			const float ndc_x = fma(px, p.sx, -1.0f), ndc_y = fma(py, p.neg_sy, 1.0f);
			float N[4], F[4];
#pragma unroll
			for (int r = 0; r < 4; r++)
			{
				N[r] = fma(p.mx[r], ndc_x, fma(p.my[r], ndc_y, p.k_near[r]));
				F[r] = fma(p.mx[r], ndc_x, fma(p.my[r], ndc_y, p.k_far[r]));
			}
			const float inv_wn = rcp_rn(N[3]);
			origin = { N[0] * inv_wn, N[1] * inv_wn, N[2] * inv_wn };
			toward = { fma(F[0], N[3], -(N[0] * F[3])), fma(F[1], N[3], -(N[1] * F[3])), fma(F[2], N[3], -(N[2] * F[3])) };
			if (N[3] * F[3] < 0.0f)
				toward = { -toward.x, -toward.y, -toward.z };
		}
		dir = toward * inv_sqrt_rn(dot(toward, toward));
	}
}
