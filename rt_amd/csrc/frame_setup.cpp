// rt_amd/csrc/frame_setup.cpp — the refusals of rt_hip_render_device and the per-frame constants of the kernels
// (frame_setup.hpp): host-only, plain C++17.  Built with -ffp-contract=off: the binary64 constants below are defined by their
// order of operations.
#include "frame_setup.hpp"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>

namespace rt_hip
{
	namespace
	{
		__attribute__((format(printf, 3, 4))) render_check refuse(render_check check, rt_hip_status status, const char* format, ...)
		{
			check.status = status;
			va_list args;
			va_start(args, format);
			std::vsnprintf(check.message, sizeof(check.message), format, args);
			va_end(args);
			return check;
		}
	}

	render_check check_render_request(uint32_t width, uint32_t height, uint32_t flags, const rt_hip_partition* part)
	{
		render_check check{};
		if (!width || !height)
			return refuse(check, RT_HIP_INVALID_ARGUMENT, "rt_hip_render_device: empty frame %ux%u", width, height);
		if (static_cast<uint64_t>(width) * height > 0xFFFFFFFFull)
			return refuse(check, RT_HIP_INVALID_ARGUMENT, "rt_hip_render_device: %ux%u exceeds the 32-bit pixel index of image_view", width, height);
		if (flags & ~static_cast<uint32_t>(RT_HIP_FLAG_FORCE_TILED | RT_HIP_FLAG_FORCE_RESIDENT | RT_HIP_FLAG_PERSISTENT_FRAME | RT_HIP_FLAG_SM_MATERIALS | RT_HIP_FLAG_PREVIEW | RT_HIP_FLAG_FORCE_STREAMED | RT_HIP_FLAG_FAST | RT_HIP_FLAG_STATS | RT_HIP_FLAG_FORCE_HALF_CHUNKS | RT_HIP_FLAG_FORCE_WHOLE_CHUNKS | RT_HIP_FLAG_BVH | RT_HIP_FLAG_BVH_DEVICE_BUILD | RT_HIP_FLAG_TRACE_BOXES | RT_HIP_FLAG_BOX_BVH | RT_HIP_FLAG_EMISSION | RT_HIP_FLAG_DIRECT_LIGHT | RT_HIP_FLAG_THIN_LENS))
			return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: unknown flag bits 0x%x", flags);
		if ((flags & RT_HIP_FLAG_BVH) && (flags & (RT_HIP_FLAG_FORCE_TILED | RT_HIP_FLAG_FORCE_RESIDENT | RT_HIP_FLAG_FORCE_STREAMED)))
			return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_BVH chooses its own kernel (not with RT_HIP_FLAG_FORCE_TILED / _RESIDENT / _STREAMED)");
		if ((flags & RT_HIP_FLAG_BVH) && (flags & RT_HIP_FLAG_FAST))
			return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_BVH is built for the parity contract's arithmetic only (not with RT_HIP_FLAG_FAST)");
		if (flags & RT_HIP_FLAG_PREVIEW)
			flags &= ~static_cast<uint32_t>(RT_HIP_FLAG_BVH | RT_HIP_FLAG_BVH_DEVICE_BUILD | RT_HIP_FLAG_TRACE_BOXES | RT_HIP_FLAG_BOX_BVH | RT_HIP_FLAG_EMISSION | RT_HIP_FLAG_DIRECT_LIGHT | RT_HIP_FLAG_THIN_LENS); // one ray per pixel: the preview keeps its own scan, which draws boxes already (and shades by albedo: it knows no lights), through the pixel's centre (no lens)
		// the lens builds exist for the parity contract's tile-per-wave whole-chunk kernels, without boxes and without lights
		// (launch_plan.cpp): whatever the context's lens holds, the flag does not go with one that asks for another kernel
		if (flags & RT_HIP_FLAG_THIN_LENS)
		{
			if (flags & RT_HIP_FLAG_FAST)
				return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_THIN_LENS is built for the parity contract's arithmetic only (not with RT_HIP_FLAG_FAST)");
			if (flags & (RT_HIP_FLAG_FORCE_TILED | RT_HIP_FLAG_FORCE_RESIDENT | RT_HIP_FLAG_FORCE_STREAMED))
				return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_THIN_LENS chooses its own kernel (not with RT_HIP_FLAG_FORCE_TILED / _RESIDENT / _STREAMED)");
			if (flags & RT_HIP_FLAG_FORCE_HALF_CHUNKS)
				return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_THIN_LENS is built for whole chunks only (not with RT_HIP_FLAG_FORCE_HALF_CHUNKS)");
			if (flags & (RT_HIP_FLAG_TRACE_BOXES | RT_HIP_FLAG_BOX_BVH))
				return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_THIN_LENS has no build that traces boxes (not with RT_HIP_FLAG_TRACE_BOXES / RT_HIP_FLAG_BOX_BVH)");
			if (flags & (RT_HIP_FLAG_EMISSION | RT_HIP_FLAG_DIRECT_LIGHT))
				return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_THIN_LENS has no build that knows lights (not with RT_HIP_FLAG_EMISSION / RT_HIP_FLAG_DIRECT_LIGHT)");
		}
		// the light builds exist for the parity contract's tile-per-wave whole-chunk kernels, without boxes (launch_plan.cpp): whatever the
		// table holds, the flag does not go with one that asks for another kernel
		// RT_HIP_FLAG_DIRECT_LIGHT modifies RT_HIP_FLAG_EMISSION: refused without it and wherever it is refused, by its own name
		if (flags & RT_HIP_FLAG_DIRECT_LIGHT)
		{
			if (!(flags & RT_HIP_FLAG_EMISSION))
				return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_DIRECT_LIGHT says how RT_HIP_FLAG_EMISSION's sphere lights are found (not without it)");
			if (flags & RT_HIP_FLAG_FAST)
				return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_DIRECT_LIGHT is built for the parity contract's arithmetic only (not with RT_HIP_FLAG_FAST)");
			if (flags & (RT_HIP_FLAG_FORCE_TILED | RT_HIP_FLAG_FORCE_RESIDENT | RT_HIP_FLAG_FORCE_STREAMED))
				return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_DIRECT_LIGHT chooses its own kernel (not with RT_HIP_FLAG_FORCE_TILED / _RESIDENT / _STREAMED)");
			if (flags & RT_HIP_FLAG_FORCE_HALF_CHUNKS)
				return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_DIRECT_LIGHT is built for whole chunks only (not with RT_HIP_FLAG_FORCE_HALF_CHUNKS)");
			if (flags & (RT_HIP_FLAG_TRACE_BOXES | RT_HIP_FLAG_BOX_BVH))
				return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_DIRECT_LIGHT has no build that traces boxes (not with RT_HIP_FLAG_TRACE_BOXES / RT_HIP_FLAG_BOX_BVH)");
		}
		if ((flags & RT_HIP_FLAG_EMISSION) && (flags & RT_HIP_FLAG_FAST))
			return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_EMISSION is built for the parity contract's arithmetic only (not with RT_HIP_FLAG_FAST)");
		if ((flags & RT_HIP_FLAG_EMISSION) && (flags & (RT_HIP_FLAG_FORCE_TILED | RT_HIP_FLAG_FORCE_RESIDENT | RT_HIP_FLAG_FORCE_STREAMED)))
			return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_EMISSION chooses its own kernel (not with RT_HIP_FLAG_FORCE_TILED / _RESIDENT / _STREAMED)");
		if ((flags & RT_HIP_FLAG_EMISSION) && (flags & RT_HIP_FLAG_FORCE_HALF_CHUNKS))
			return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_EMISSION is built for whole chunks only (not with RT_HIP_FLAG_FORCE_HALF_CHUNKS)");
		if ((flags & RT_HIP_FLAG_EMISSION) && (flags & (RT_HIP_FLAG_TRACE_BOXES | RT_HIP_FLAG_BOX_BVH)))
			return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_EMISSION has no build that traces boxes (not with RT_HIP_FLAG_TRACE_BOXES / RT_HIP_FLAG_BOX_BVH)");
		// RT_HIP_FLAG_BOX_BVH modifies RT_HIP_FLAG_TRACE_BOXES: refused without it and wherever it is refused, by its own name
		if ((flags & RT_HIP_FLAG_BOX_BVH) && !(flags & RT_HIP_FLAG_TRACE_BOXES))
			return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_BOX_BVH says how RT_HIP_FLAG_TRACE_BOXES reaches the boxes (not without it)");
		if ((flags & RT_HIP_FLAG_BOX_BVH) && (flags & RT_HIP_FLAG_FAST))
			return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_BOX_BVH is built for the parity contract's arithmetic only, like RT_HIP_FLAG_TRACE_BOXES (not with RT_HIP_FLAG_FAST)");
		if ((flags & RT_HIP_FLAG_BOX_BVH) && (flags & (RT_HIP_FLAG_FORCE_TILED | RT_HIP_FLAG_FORCE_RESIDENT | RT_HIP_FLAG_FORCE_STREAMED)))
			return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_BOX_BVH takes the hierarchy kernel (not with RT_HIP_FLAG_FORCE_TILED / _RESIDENT / _STREAMED)");
		if ((flags & RT_HIP_FLAG_BOX_BVH) && (flags & RT_HIP_FLAG_FORCE_HALF_CHUNKS))
			return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_BOX_BVH is built for whole chunks only, like RT_HIP_FLAG_TRACE_BOXES (not with RT_HIP_FLAG_FORCE_HALF_CHUNKS)");
		// the box builds exist for the parity contract's tile-per-wave whole-chunk kernels (launch_plan.cpp): whatever the scene holds, the
		// flag does not go with one that asks for another kernel
		if ((flags & RT_HIP_FLAG_TRACE_BOXES) && (flags & RT_HIP_FLAG_FAST))
			return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_TRACE_BOXES is built for the parity contract's arithmetic only (not with RT_HIP_FLAG_FAST)");
		if ((flags & RT_HIP_FLAG_TRACE_BOXES) && (flags & (RT_HIP_FLAG_FORCE_TILED | RT_HIP_FLAG_FORCE_RESIDENT | RT_HIP_FLAG_FORCE_STREAMED)))
			return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_TRACE_BOXES chooses its own kernel (not with RT_HIP_FLAG_FORCE_TILED / _RESIDENT / _STREAMED)");
		if ((flags & RT_HIP_FLAG_TRACE_BOXES) && (flags & RT_HIP_FLAG_FORCE_HALF_CHUNKS))
			return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_TRACE_BOXES is built for whole chunks only (not with RT_HIP_FLAG_FORCE_HALF_CHUNKS)");
		if ((flags & RT_HIP_FLAG_BVH_DEVICE_BUILD) && !(flags & RT_HIP_FLAG_BVH))
			return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_BVH_DEVICE_BUILD says how RT_HIP_FLAG_BVH's hierarchy is built (not without it)");
		if ((flags & RT_HIP_FLAG_FORCE_HALF_CHUNKS) && (flags & RT_HIP_FLAG_FORCE_WHOLE_CHUNKS))
			return refuse(check, RT_HIP_INVALID_ARGUMENT, "rt_hip_render_device: RT_HIP_FLAG_FORCE_HALF_CHUNKS and RT_HIP_FLAG_FORCE_WHOLE_CHUNKS exclude each other");
		if ((flags & RT_HIP_FLAG_FAST) && (flags & (RT_HIP_FLAG_SM_MATERIALS | RT_HIP_FLAG_PREVIEW)))
			return refuse(check, RT_HIP_UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_FAST applies to mg_ray_tracer's path only (not with RT_HIP_FLAG_SM_MATERIALS / RT_HIP_FLAG_PREVIEW)");
		check.bvh_device_build = (flags & RT_HIP_FLAG_BVH_DEVICE_BUILD) != 0u;
		flags &= ~static_cast<uint32_t>(RT_HIP_FLAG_BVH_DEVICE_BUILD); // (the builder's business: the launch is RT_HIP_FLAG_BVH's either way)
		check.flags = flags;
		// The launch grid's y dimension counts rows of pixel tiles and holds 65535 of them.  A tile may be ONE row high (a page-locked frame's,
		// from 64 samples a pixel: choose_queue), but it holds at least four pixels, and where one-row tiles would be more than 65535 rows of
		// them the plan takes the next taller shape (launch_plan.cpp, cut_tiles): two rows a tile is what every frame up to here can have.
		if (height > 65535u * 2u)
			return refuse(check, RT_HIP_INVALID_ARGUMENT, "rt_hip_render_device: frame height %u exceeds the supported 131070 rows", height);
		const rt_hip_partition whole = { 0, 1, RT_HIP_DEFAULT_STRIPE_ROWS };
		const rt_hip_partition p = part ? *part : whole;
		if (!valid_partition(p))
			return refuse(check, RT_HIP_INVALID_ARGUMENT, "rt_hip_render_device: invalid partition {rank %u, world %u, stripe_rows %u}", p.rank, p.world, p.stripe_rows);
		check.partition = p;
		return check;
	}

	frame_params make_frame_params(const frame_request& request)
	{
		const uint32_t width = request.width, height = request.height;
		const rt_hip_partition& p = request.partition;
		frame_params f{};
		f.width = width;
		f.height = height;
		f.local_rows = local_rows_of(height, p.rank, p.world, p.stripe_rows);
		f.rank = p.rank;
		f.world = p.world;
		f.stripe_rows = p.stripe_rows;
		f.frame_rows = request.whole_frame_buffers ? 1u : 0u;
		f.stripe_shift = 0xFFFFFFFFu;
		if ((p.stripe_rows & (p.stripe_rows - 1u)) == 0u)
			for (f.stripe_shift = 0; (1u << f.stripe_shift) != p.stripe_rows; f.stripe_shift++)
			{}
		f.samples_per_pixel = request.samples_per_pixel;
		// (the kernels keep "tracing" and the bounces still allowed in one word, lane_trace + count: a count of 2^30 is as good as any
		// larger one — no path of a frame that ever finishes is that long)
		f.max_bounces = std::min<uint32_t>(request.max_bounces, 1u << 30);
		const frame_keys keys = make_frame_keys(request.seed);
		f.frame_key_a = keys.a;
		f.frame_key_b = keys.b;
		f.sx = 2.0f / static_cast<float>(width);
		f.neg_sy = -(2.0f / static_cast<float>(height));
		const float* M = request.inverse_view_projection;
		for (int r = 0; r < 4; r++)
		{
			f.mx[r] = M[r * 4 + 0];
			f.my[r] = M[r * 4 + 1];
			f.k_near[r] = std::fmaf(M[r * 4 + 2], 0.0f, M[r * 4 + 3]);
			f.k_far[r] = std::fmaf(M[r * 4 + 2], 1.0f, M[r * 4 + 3]);
		}
		// Contract v4, primary rays (oracle/cpu_ref.cpp make_frame has the same lines).  w = fma(mx[3], ndc.x, fma(my[3], ndc.y,
		// k[3])) is exactly k[3] for every finite ndc when mx[3] and my[3] are (+-)0 and k[3] is not; then
		//   near(px, py) = (mx X + my Y + k_near) / w_near,   X = (2/W) px - 1,   Y = -(2/H) py + 1,
		// is affine in the pixel position, and so is far - near.  rt's frustum is a pinhole's on top of that: every near-to-far
		// line passes through the eye, near = eye + kappa (far - near) with one kappa for the frame.  The constants are worked
		// out in binary64, in THIS order of operations, and rounded to binary32 once.  A matrix is taken as a pinhole's when the
		// near point's motion per pixel is kappa times the near-to-far vector's to within 1e-5 (relative; 1e-10 of a pixel
		// step: far below what binary32 resolves); anything else goes through the homogeneous form.
		f.eye_form = 0u;
		{
			// the eye form (oracle/cpu_ref.cpp make_frame has the same lines): N_r(px, py) = mx_r X + my_r Y + k_near_r with
			// X = (2/W) px - 1, Y = -(2/H) py + 1, i.e. n0_r + n1_r px + n2_r py; E = Z.xyz / Z.w; s = sign(-Z.w)
			const double sx = 2.0 / static_cast<double>(width), sy = -(2.0 / static_cast<double>(height));
			const double zw = M[3 * 4 + 2];
			const double e[3] = { M[0 * 4 + 2] / zw, M[1 * 4 + 2] / zw, M[2 * 4 + 2] / zw };
			const double sign = zw < 0.0 ? 1.0 : -1.0;
			const double n1w = static_cast<double>(M[12]) * sx, n2w = static_cast<double>(M[13]) * sy;
			const double n0w = static_cast<double>(f.k_near[3]) - static_cast<double>(M[12]) + static_cast<double>(M[13]);
			bool finite = zw != 0.0 && std::isfinite(e[0]) && std::isfinite(e[1]) && std::isfinite(e[2]) && std::isfinite(n0w) && std::isfinite(n1w) && std::isfinite(n2w);
			for (int c = 0; c < 3 && finite; c++)
			{
				const double mx = M[c * 4 + 0], my = M[c * 4 + 1];
				const double n1 = mx * sx, n2 = my * sy, n0 = static_cast<double>(f.k_near[c]) - mx + my;
				f.eye_q0[c] = static_cast<float>(sign * (n0 - e[c] * n0w)), f.eye_q1[c] = static_cast<float>(sign * (n1 - e[c] * n1w)), f.eye_q2[c] = static_cast<float>(sign * (n2 - e[c] * n2w));
				f.eye_jq1[c] = f.eye_q1[c] * 0x1.0p-24f, f.eye_jq2[c] = f.eye_q2[c] * 0x1.0p-24f;
				f.eye_e[c] = static_cast<float>(e[c]);
				finite = std::isfinite(f.eye_q0[c]) && std::isfinite(f.eye_q1[c]) && std::isfinite(f.eye_q2[c]);
			}
			if (finite)
			{
				f.eye_w0 = static_cast<float>(sign * n0w), f.eye_w1 = static_cast<float>(sign * n1w), f.eye_w2 = static_cast<float>(sign * n2w);
				f.eye_jw1 = f.eye_w1 * 0x1.0p-24f, f.eye_jw2 = f.eye_w2 * 0x1.0p-24f;
				f.eye_zws = static_cast<float>(sign * zw);
				f.eye_form = 1u;
				// eye_form 2: over the whole frame s N.w and s N.w + s Z.w (= s F.w) keep ONE sign and stay far inside the band of the
				// kernels' unguarded reciprocal (2^-60 .. 2^60) — both are affine in the pixel position, so their extremes sit at the
				// frame's corners.  Then no lane ever needs the reciprocal's guard or the "near and far straddle w = 0" flip, and the
				// kernels skip both (same bits: the guarded forms are identities there).  Every camera rt can make is such a one.
				bool plain = true;
				double first_w = 0.0;
				for (int corner = 0; corner < 4 && plain; corner++)
				{
					const double x = (corner & 1) ? static_cast<double>(width) : 0.0, y = (corner & 2) ? static_cast<double>(height) : 0.0;
					const double ws = sign * (n0w + n1w * x + n2w * y), fs = ws + sign * zw;
					if (corner == 0)
						first_w = ws;
					plain = std::fabs(ws) >= 0x1.0p-50 && std::fabs(ws) <= 0x1.0p50 && std::fabs(fs) >= 0x1.0p-50 && std::fabs(fs) <= 0x1.0p50 && (ws > 0.0) == (first_w > 0.0) && (ws > 0.0) == (fs > 0.0);
				}
				if (plain)
					f.eye_form = 2u;
			}
		}
		f.pinhole = 0u;
		if (f.mx[3] == 0.0f && f.my[3] == 0.0f && f.k_near[3] != 0.0f && f.k_far[3] != 0.0f && std::isfinite(f.k_near[3]) && std::isfinite(f.k_far[3]))
		{
			const double sx = 2.0 / static_cast<double>(width), sy = -(2.0 / static_cast<double>(height));
			const double iwn = 1.0 / static_cast<double>(f.k_near[3]), iwf = 1.0 / static_cast<double>(f.k_far[3]);
			double o0[3], o1[3], o2[3], d0[3], d1[3], d2[3];
			for (int c = 0; c < 3; c++)
			{
				const double mx = f.mx[c], my = f.my[c], kn = f.k_near[c], kf = f.k_far[c];
				o1[c] = mx * sx * iwn, o2[c] = my * sy * iwn, o0[c] = (kn - mx + my) * iwn;
				const double e1 = mx * sx * iwf, e2 = my * sy * iwf, e0 = (kf - mx + my) * iwf;
				d0[c] = e0 - o0[c], d1[c] = e1 - o1[c], d2[c] = e2 - o2[c];
			}
			const double dd = d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2] + d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2];
			const double od = o1[0] * d1[0] + o1[1] * d1[1] + o1[2] * d1[2] + o2[0] * d2[0] + o2[1] * d2[1] + o2[2] * d2[2];
			const double kappa = od / dd;
			double worst = 0.0, scale = 0.0;
			for (int c = 0; c < 3; c++)
			{
				worst = std::fmax(worst, std::fmax(std::fabs(o1[c] - kappa * d1[c]), std::fabs(o2[c] - kappa * d2[c])));
				scale = std::fmax(scale, std::fmax(std::fabs(o1[c]), std::fabs(o2[c])));
			}
			if (dd > 0.0 && kappa >= 0x1.0p-20 && kappa <= 0x1.0p20 && worst <= 1.0e-5 * scale) // (a NaN anywhere fails a comparison; kappa = near / (far - near) scales the vector the kernels normalise, so its sign and size matter)
			{
				f.pinhole = 1u;
				for (int c = 0; c < 3; c++)
				{
					// (the vector the kernels carry is kappa * (far - near) = near - eye: the near point is then eye + it, one addition)
					f.ray_d0[c] = static_cast<float>(kappa * d0[c]), f.ray_d1[c] = static_cast<float>(kappa * d1[c]), f.ray_d2[c] = static_cast<float>(kappa * d2[c]);
					f.ray_j1[c] = f.ray_d1[c] * 0x1.0p-24f, f.ray_j2[c] = f.ray_d2[c] * 0x1.0p-24f;
					f.ray_eye[c] = static_cast<float>(o0[c] - kappa * d0[c]);
				}
			}
		}
		return f;
	}
}
