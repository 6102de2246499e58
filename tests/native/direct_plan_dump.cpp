// tests/native/direct_plan_dump.cpp — what a frame with RT_HIP_FLAG_DIRECT_LIGHT is told on the host, on the CPU (tests/test_direct_plan.py;
// light_plan_dump.cpp with the sampled-light count and the plan's `direct`):
// the refusals of the request (rt_amd/csrc/frame_setup.cpp, check_render_request), the check of the frame against the context's emission
// table (rt_amd/csrc/lights.cpp, check_emission_table) and the launch plan (rt_amd/csrc/launch_plan.cpp), in the order
// rt_hip_render_device makes them.  Built from this file and those three alone, with the host compiler and nothing of ROCm.  Reads one
// request per line from standard input —
//     n_spheres n_planes width local_rows samples_per_pixel camera(0 pinhole, 1 plain eye, 2 other) flags host_frame
//     table_rows(-1: no table set) n_lights scene_materials n_sampled_lights
// — and prints one line each: `refused <status> <message>` where rt_hip_render_device refuses it, else name=value for every field of
// the launch_plan.
#include "../../rt_amd/csrc/frame_setup.hpp"
#include "../../rt_amd/csrc/launch_plan.hpp"
#include "../../rt_amd/csrc/lights.hpp"

#include <cinttypes>
#include <cstdarg>
#include <cstdio>

namespace rt_hip
{
	// (lights.cpp's C entry point reports through the library's fail(); nothing here calls it)
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
	unsigned n_spheres, n_planes, width, local_rows, samples_per_pixel, camera, flags, host_frame, n_lights, scene_materials, n_sampled;
	int table_rows;
	while (std::scanf("%u %u %u %u %u %u %u %u %d %u %u %u", &n_spheres, &n_planes, &width, &local_rows, &samples_per_pixel, &camera, &flags, &host_frame, &table_rows, &n_lights, &scene_materials, &n_sampled) == 12)
	{
		const render_check checked = check_render_request(width, local_rows, flags, nullptr);
		if (checked.status)
		{
			std::printf("refused %d %s\n", int(checked.status), checked.message);
			continue;
		}
		if (checked.flags & RT_HIP_FLAG_EMISSION)
		{
			const light_check table = check_emission_table("rt_hip_render_device", table_rows >= 0, table_rows >= 0 ? static_cast<uint32_t>(table_rows) : 0u, scene_materials);
			if (table.status)
			{
				std::printf("refused %d %s\n", int(table.status), table.message);
				continue;
			}
		}
		launch_request r{};
		r.n_spheres = n_spheres, r.n_planes = n_planes, r.planes_tame = true;
		r.width = width, r.local_rows = local_rows, r.samples_per_pixel = samples_per_pixel;
		r.camera = static_cast<camera_form>(camera);
		r.flags = checked.flags, r.host_frame = host_frame != 0, r.fast_arithmetic = (checked.flags & RT_HIP_FLAG_FAST) != 0;
		r.n_lights = (checked.flags & RT_HIP_FLAG_EMISSION) ? n_lights : 0u;
		r.n_sampled_lights = ((checked.flags & RT_HIP_FLAG_DIRECT_LIGHT) && r.n_lights) ? n_sampled : 0u; // (as rt_hip_render_device counts them)
		const launch_plan p = plan_launch(r);
		if (p.refusal[0])
		{
			std::printf("refused %d rt_hip_render_device: %s\n", int(RT_HIP_UNSUPPORTED), p.refusal);
			continue;
		}
		const queue_params& q = p.queue;
		std::printf("variant=%u big_scene=%d chunks=%u pixels_log2=%u tile_w_log2=%u tiles_x=%u tiles_y=%u block_items=%u lane_cap=%u sparse_rays=%u halves=%u item_samples=%u "
					"scan=%d planes=%d general_camera=%d sub_chunk_items=%d sm_table=%d pass=%d boxes=%d lights=%d direct=%d grid_x=%u grid_y=%u table_bytes=%zu slot_bytes=%zu lds_bytes=%zu total_items=%" PRIu64
					" item_sums_bytes=%zu pixel_done_bytes=%zu persistent_slot=%d per_cu_cap=%d first_chunk=%u\n",
					p.variant, int(p.big_scene), q.chunks, q.pixels_log2, q.tile_w_log2, q.tiles_x, q.tiles_y, q.block_items, q.lane_cap, q.sparse_rays, q.halves, q.item_samples, p.build.scan, p.build.planes,
					int(p.build.general_camera), int(p.build.sub_chunk_items), int(p.build.sm_table), int(p.build.pass), int(p.build.boxes), int(p.build.lights), int(p.build.direct), p.grid_x, p.grid_y, p.table_bytes, p.slot_bytes, p.lds_bytes,
					p.total_items, p.item_sums_bytes, p.pixel_done_bytes, p.persistent_slot, p.per_cu_cap, p.first_chunk);
	}
	return 0;
}
