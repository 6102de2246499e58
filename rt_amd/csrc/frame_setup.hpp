// rt_amd/csrc/frame_setup.hpp — what one render launch is told before it is planned: is the request one the module renders
// (check_render_request), and the per-frame constants the kernels trace from (make_frame_params: the partition's rows, the
// mixed seed, the camera's form and its binary64 constants).  Host-only: plain C++17, no HIP header, built with the host
// compiler into librt_hip.so and, on the CPU, into tests/native/frame_setup_dump (tests/test_frame_setup.py holds every field
// against the oracle's own copy of the arithmetic, oracle/cpu_ref.cpp make_frame).
#pragma once

#include <stdint.h>
#include "../../include/rt_hip.h" // (rt_hip_status, rt_hip_partition, the render flags)
#include "launch_plan.hpp"		  // (camera_form)

namespace rt_hip
{
	inline bool valid_partition(const rt_hip_partition& p)
	{
		return p.world && p.rank < p.world && p.stripe_rows;
	}

	inline uint32_t local_rows_of(uint32_t height, uint32_t rank, uint32_t world, uint32_t stripe_rows)
	{
		const uint32_t stripes = (height + stripe_rows - 1) / stripe_rows;
		uint32_t rows = 0;
		for (uint32_t b = rank; b < stripes; b += world)
		{
			const uint32_t y0 = b * stripe_rows;
			rows += (height - y0 < stripe_rows) ? height - y0 : stripe_rows;
		}
		return rows;
	}

	// the two halves of the mixed 64-bit seed (contract.hpp, random streams)
	struct frame_keys
	{
		uint32_t a, b;
	};

	inline frame_keys make_frame_keys(uint64_t seed) // the splitmix64 finaliser: a bijection of 64-bit words
	{
		uint64_t z = seed + 0x9E3779B97F4A7C15ull;
		z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
		z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
		z ^= z >> 31;
		return { static_cast<uint32_t>(z), static_cast<uint32_t>(z >> 32) };
	}

	// Per-frame uniforms (kernel arguments -> SGPRs).
	struct frame_params
	{
		uint32_t width, height;			   // full frame
		uint32_t local_rows;			   // rows this rank renders (compact buffer height in use)
		uint32_t rank, world, stripe_rows; // rt_hip_partition
		uint32_t stripe_shift;			   // log2(stripe_rows) if that is a power of two, else 0xFFFFFFFF (general division)
		uint32_t frame_rows;			   // != 0: the output buffers are the WHOLE frame, a pixel goes to its image row (several
										   // GPUs storing straight into one host frame); 0: this rank's compact stripe buffer
		uint32_t samples_per_pixel, max_bounces;
		uint32_t frame_key_a, frame_key_b;  // the two halves of the mixed 64-bit seed (contract.hpp, random streams)
		float sx, neg_sy;				   // 2/W and -(2/H): ndc = (fma(px, sx, -1), fma(py, neg_sy, 1))
		// inverse view-projection, pre-split for depth 0 / depth 1 (camera.hpp:42-48):
		// row_r(depth) = fma(mx[r], ndc.x, fma(my[r], ndc.y, k[r])),  k_near[r] = fma(M[r][2], 0, M[r][3]),
		// k_far[r] = fma(M[r][2], 1, M[r][3])
		float mx[4], my[4], k_near[4], k_far[4];
		// Contract v4, primary rays.  For a camera built as in camera.hpp:122-137 the last row of the inverse view-projection
		// does not depend on x and y, so w is a per-frame constant, the un-projected near and far points are AFFINE in the
		// pixel position, and every near-to-far line passes through the eye: a PINHOLE.  pinhole != 0 says the matrix is one
		// (decided on the host from binary64 constants, frame_setup.cpp; the oracle has the same lines) and the kernels then use
		//   base_c   = fma(ray_d1[c], x, fma(ray_d2[c], y, ray_d0[c]))          once per pixel (x, y: its column and row)
		//   toward_c = fma(ray_j1[c], ka, fma(ray_j2[c], kb, base_c))           per sample; (ka, kb) = the jitter's numerators,
		//                                                                        ray_j = ray_d * 2^-24
		//   origin_c = ray_eye[c] + toward_c                                    the near point (ray_d holds kappa * (far - near)
		//                                                                        = near - eye, kappa = near / (far - near))
		// The scalar-register kernels are built for ONE form; mx .. k_far above serve the preview and any other matrix (an
		// orthographic or sheared frustum, a w that varies over the frame: the homogeneous form with one division per sample).
		uint32_t pinhole;
		float ray_d0[3], ray_d1[3], ray_d2[3];
		float ray_j1[3], ray_j2[3];
		float ray_eye[3];
		// eye_form != 0: the matrix is a PERSPECTIVE one (its depth column Z has a finite point E = Z.xyz / Z.w: the eye every
		// near-to-far line passes through) — what the general-camera kernels use for a camera that is not axis-aligned.  With
		// N = the homogeneous near point, N' = N.xyz - E N.w and s = sign(-Z.w), both s N' and s N.w are affine in the pixel
		// position (binary64 constants, like the pinhole's):
		//   base_c = fma(eye_q1[c], x, fma(eye_q2[c], y, eye_q0[c])),   base_w = fma(eye_w1, x, fma(eye_w2, y, eye_w0))    per pixel
		//   t_c    = fma(eye_jq1[c], ka, fma(eye_jq2[c], kb, base_c)),  ws     = fma(eye_jw1, ka, fma(eye_jw2, kb, base_w)) per sample
		//   origin_c = fma(t_c, 1 / ws, eye_e[c]);   toward = t, negated if ws * (ws + eye_zws) < 0   (= N.w F.w < 0)
		// One division per sample and no far point.  A matrix without a finite eye (an orthographic frustum) takes the
		// homogeneous form from mx .. k_far above.
		uint32_t eye_form; // 1 as above; 2: additionally s N.w and s F.w keep one sign and stay deep inside the reciprocal's band over the whole frame (frame_setup.cpp): no guard, no flip
		float eye_q0[3], eye_q1[3], eye_q2[3];
		float eye_jq1[3], eye_jq2[3];
		float eye_w0, eye_w1, eye_w2, eye_jw1, eye_jw2;
		float eye_e[3];
		float eye_zws;
	};

	// what a frame's constants are made from
	struct frame_request
	{
		uint32_t width, height;
		rt_hip_partition partition;				  // a valid one (check_render_request)
		uint32_t samples_per_pixel, max_bounces;  // of the resident scene
		uint64_t seed;
		float inverse_view_projection[16];		  // of the resident scene, row-major
		bool whole_frame_buffers;				  // the output buffers are the whole frame (frame_params::frame_rows)
	};
	frame_params make_frame_params(const frame_request& request);

	// which camera the kernels of this frame are built for (launch_request::camera)
	inline camera_form camera_form_of(const frame_params& f)
	{
		return f.pinhole ? camera_form::pinhole : (f.eye_form == 2u ? camera_form::plain_eye : camera_form::other);
	}

	// Is this a frame rt_hip_render_device renders?  Flag combinations, the frame's size, the partition: everything that can be
	// said without the context.
	struct render_check
	{
		rt_hip_status status;	   // RT_HIP_OK, or the refusal's status with
		char message[256];		   // ... the text fail() is given
		uint32_t flags;			   // the LAUNCH's flags: the preview has dropped RT_HIP_FLAG_BVH (it keeps its own scan), and
		bool bvh_device_build;	   // RT_HIP_FLAG_BVH_DEVICE_BUILD is taken out into this (the builder's business, ensure_bvh: the launch is RT_HIP_FLAG_BVH's either way)
		rt_hip_partition partition; // `part`, or the whole frame
	};
	render_check check_render_request(uint32_t width, uint32_t height, uint32_t flags, const rt_hip_partition* part);
}
