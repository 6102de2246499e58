// tests/native/light_sweep_plan_dump.cpp — plan_launch (rt_amd/csrc/launch_plan.cpp) asked on the CPU for frames with RT_HIP_FLAG_EMISSION /
// RT_HIP_FLAG_DIRECT_LIGHT: lds_plan_dump.cpp's request with the two light counts, direct_plan_dump.cpp's `lights` and `direct` in the
// answer (tests/light_plan.py; tests/test_gpu_light_rare_branches.py and tests/test_gpu_light_chunk_sweep.py ask it which build, tile and
// fold path every one of their frames takes).  Built from this file and launch_plan.cpp alone, with the host compiler and nothing of
// ROCm.  Reads one request per line from standard input —
//     n_spheres n_planes width local_rows samples_per_pixel camera(0 pinhole, 1 plain eye, 2 other) flags host_frame
//     n_lights n_sampled_lights lds_limit(0: the plan's default)
// — and prints name=value for every field of the launch_plan the tests read, one line per request; the plan's refusal, empty or not,
// ends the line.  The counts are taken as rt_hip_render_device counts them: lights only under RT_HIP_FLAG_EMISSION, sampled lights only
// under RT_HIP_FLAG_DIRECT_LIGHT with at least one light.
#include "../../rt_amd/csrc/launch_plan.hpp"

#include <cinttypes>
#include <cstdio>

int main()
{
	using namespace rt_hip;
	unsigned n_spheres, n_planes, width, local_rows, samples_per_pixel, camera, flags, host_frame, n_lights, n_sampled;
	unsigned long long lds_limit;
	while (std::scanf("%u %u %u %u %u %u %u %u %u %u %llu", &n_spheres, &n_planes, &width, &local_rows, &samples_per_pixel, &camera, &flags, &host_frame, &n_lights, &n_sampled, &lds_limit) == 11)
	{
		launch_request r{};
		r.n_spheres = n_spheres, r.n_planes = n_planes, r.planes_tame = true;
		r.width = width, r.local_rows = local_rows, r.samples_per_pixel = samples_per_pixel;
		r.camera = static_cast<camera_form>(camera);
		r.flags = flags, r.host_frame = host_frame != 0, r.fast_arithmetic = false;
		r.n_lights = (flags & RT_HIP_FLAG_EMISSION) ? n_lights : 0u;
		r.n_sampled_lights = ((flags & RT_HIP_FLAG_DIRECT_LIGHT) && r.n_lights) ? n_sampled : 0u;
		r.lds_limit = static_cast<size_t>(lds_limit);
		const launch_plan p = plan_launch(r);
		const queue_params& q = p.queue;
		std::printf("variant=%u big_scene=%d chunks=%u pixels_log2=%u tile_w_log2=%u tiles_x=%u tiles_y=%u halves=%u scan=%d planes=%d general_camera=%d sub_chunk_items=%d sm_table=%d pass=%d boxes=%d lights=%d direct=%d "
					"grid_x=%u grid_y=%u table_bytes=%zu slot_bytes=%zu lds_bytes=%zu total_items=%" PRIu64 " refusal=%s\n",
					p.variant, int(p.big_scene), q.chunks, q.pixels_log2, q.tile_w_log2, q.tiles_x, q.tiles_y, q.halves, p.build.scan, p.build.planes, int(p.build.general_camera), int(p.build.sub_chunk_items), int(p.build.sm_table),
					int(p.build.pass), int(p.build.boxes), int(p.build.lights), int(p.build.direct), p.grid_x, p.grid_y, p.table_bytes, p.slot_bytes, p.lds_bytes, p.total_items, p.refusal);
	}
	return 0;
}
