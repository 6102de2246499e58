// tests/native/lens_plan_dump.cpp — what a frame with RT_HIP_FLAG_THIN_LENS is told on the host, on the CPU (tests/test_lens_plan.py):
// the refusals of the request (rt_amd/csrc/frame_setup.cpp, check_render_request), the check of the frame against the context's lens and
// its own camera (rt_amd/csrc/lens.cpp, check_lens_frame), what render.hip does with an aperture of 0 and the launch plan
// (rt_amd/csrc/launch_plan.cpp), in the order rt_hip_render_device makes them.  Built from this file and those three alone, with the host
// compiler and nothing of ROCm.  Reads one request per line from standard input —
//     n_spheres n_planes width local_rows samples_per_pixel camera(0 pinhole, 1 plain eye, 2 guarded eye, 3 no finite eye) flags host_frame
//     have_lens aperture_radius
// — and prints one line each: `refused <status> <message>` where rt_hip_render_device refuses it, else name=value for every field of
// the launch_plan, and whether the frame may be offered a sky band.
#include "../../rt_amd/csrc/frame_setup.hpp"
#include "../../rt_amd/csrc/launch_plan.hpp"
#include "../../rt_amd/csrc/lens.hpp"

#include <cinttypes>
#include <cstdarg>
#include <cstdio>

namespace rt_hip
{
	// (lens.cpp's C entry point reports through the library's fail(); nothing here calls it)
	rt_hip_status fail(rt_hip_status status, const char* format, ...)
	{
		va_list args;
		va_start(args, format);
		std::vfprintf(stderr, format, args);
		va_end(args);
		return status;
	}
}

int main()
{
	using namespace rt_hip;
	unsigned n_spheres, n_planes, width, local_rows, samples_per_pixel, camera, flags, host_frame, have_lens;
	float aperture;
	while (std::scanf("%u %u %u %u %u %u %u %u %u %f", &n_spheres, &n_planes, &width, &local_rows, &samples_per_pixel, &camera, &flags, &host_frame, &have_lens, &aperture) == 10)
	{
		const render_check checked = check_render_request(width, local_rows, flags, nullptr);
		if (checked.status)
		{
			std::printf("refused %d %s\n", int(checked.status), checked.message);
			continue;
		}
		uint32_t launch_flags = checked.flags;
		if (launch_flags & RT_HIP_FLAG_THIN_LENS)
		{
			frame_params f{};
			f.pinhole = camera == 0u ? 1u : 0u;
			f.eye_form = camera == 1u ? 2u : (camera == 2u ? 1u : 0u);
			const lens_check lens = check_lens_frame("rt_hip_render_device", have_lens != 0u, f);
			if (lens.status)
			{
				std::printf("refused %d %s\n", int(lens.status), lens.message);
				continue;
			}
			if (!(aperture > 0.0f)) // (render.hip: with an aperture of 0 the flag ends here)
				launch_flags &= ~static_cast<uint32_t>(RT_HIP_FLAG_THIN_LENS);
		}
		launch_request r{};
		r.n_spheres = n_spheres, r.n_planes = n_planes, r.planes_tame = true;
		r.width = width, r.local_rows = local_rows, r.samples_per_pixel = samples_per_pixel;
		r.camera = camera == 0u ? camera_form::pinhole : (camera == 1u ? camera_form::plain_eye : camera_form::other);
		r.flags = launch_flags, r.host_frame = host_frame != 0, r.fast_arithmetic = (launch_flags & RT_HIP_FLAG_FAST) != 0;
		r.lens_aperture = (launch_flags & RT_HIP_FLAG_THIN_LENS) ? aperture : 0.0f;
		const launch_plan p = plan_launch(r);
		if (p.refusal[0])
		{
			std::printf("refused %d rt_hip_render_device: %s\n", int(RT_HIP_UNSUPPORTED), p.refusal);
			continue;
		}
		const queue_params& q = p.queue;
		std::printf("variant=%u big_scene=%d chunks=%u pixels_log2=%u tile_w_log2=%u tiles_x=%u tiles_y=%u block_items=%u lane_cap=%u sparse_rays=%u halves=%u item_samples=%u "
					"scan=%d planes=%d general_camera=%d sub_chunk_items=%d sm_table=%d pass=%d boxes=%d lights=%d lens=%d band_offered=%d grid_x=%u grid_y=%u table_bytes=%zu slot_bytes=%zu lds_bytes=%zu total_items=%" PRIu64
					" item_sums_bytes=%zu pixel_done_bytes=%zu persistent_slot=%d per_cu_cap=%d first_chunk=%u\n",
					p.variant, int(p.big_scene), q.chunks, q.pixels_log2, q.tile_w_log2, q.tiles_x, q.tiles_y, q.block_items, q.lane_cap, q.sparse_rays, q.halves, q.item_samples, p.build.scan, p.build.planes,
					int(p.build.general_camera), int(p.build.sub_chunk_items), int(p.build.sm_table), int(p.build.pass), int(p.build.boxes), int(p.build.lights), int(p.build.lens), int(!p.build.lens) /* render.hip */, p.grid_x,
					p.grid_y, p.table_bytes, p.slot_bytes, p.lds_bytes, p.total_items, p.item_sums_bytes, p.pixel_done_bytes, p.persistent_slot, p.per_cu_cap, p.first_chunk);
	}
	return 0;
}
