// tests/native/lds_plan_dump.cpp — plan_launch (rt_amd/csrc/launch_plan.cpp) asked on the CPU with EVERY field of a launch_request, the
// device's LDS limit among them (tests/lds_plan.py; tests/test_plan_lds_limit.py, tests/test_gpu_chunk_sweep.py).  Built from this file
// and launch_plan.cpp alone, with the host compiler and nothing of ROCm.  Reads one request per line from standard input —
//     n_spheres n_planes n_boxes width local_rows samples_per_pixel camera(0 pinhole, 1 plain eye, 2 other) flags host_frame
//     pass_first_sample pass_samples adaptive lds_limit(0: the plan's default)
// — and prints name=value for every field of the launch_plan, one line per request; the plan's refusal, empty or not, ends the line.
#include "../../rt_amd/csrc/launch_plan.hpp"

#include <cinttypes>
#include <cstdio>

int main()
{
	using namespace rt_hip;
	unsigned n_spheres, n_planes, n_boxes, width, local_rows, samples_per_pixel, camera, flags, host_frame, pass_first_sample, pass_samples, adaptive;
	unsigned long long lds_limit;
	while (std::scanf("%u %u %u %u %u %u %u %u %u %u %u %u %llu", &n_spheres, &n_planes, &n_boxes, &width, &local_rows, &samples_per_pixel, &camera, &flags, &host_frame, &pass_first_sample, &pass_samples, &adaptive, &lds_limit) == 13)
	{
		launch_request r{};
		r.n_spheres = n_spheres, r.n_planes = n_planes, r.planes_tame = true, r.n_boxes = n_boxes;
		r.width = width, r.local_rows = local_rows, r.samples_per_pixel = samples_per_pixel;
		r.camera = static_cast<camera_form>(camera);
		r.flags = flags, r.host_frame = host_frame != 0, r.fast_arithmetic = (flags & RT_HIP_FLAG_FAST) != 0;
		r.pass_first_sample = pass_first_sample, r.pass_samples = pass_samples, r.adaptive = adaptive != 0;
		r.lds_limit = static_cast<size_t>(lds_limit);
		const launch_plan p = plan_launch(r);
		const queue_params& q = p.queue;
		std::printf("variant=%u big_scene=%d chunks=%u pixels_log2=%u tile_w_log2=%u tiles_x=%u tiles_y=%u halves=%u "
					"scan=%d planes=%d general_camera=%d sub_chunk_items=%d sm_table=%d pass=%d boxes=%d box_tree=%d adaptive=%d grid_x=%u grid_y=%u table_bytes=%zu slot_bytes=%zu lds_bytes=%zu total_items=%" PRIu64
					" first_chunk=%u max_slot_bytes=%zu default_lds_limit=%zu refusal=%s\n",
					p.variant, int(p.big_scene), q.chunks, q.pixels_log2, q.tile_w_log2, q.tiles_x, q.tiles_y, q.halves, p.build.scan, p.build.planes, int(p.build.general_camera), int(p.build.sub_chunk_items), int(p.build.sm_table),
					int(p.build.pass), int(p.build.boxes), int(p.build.box_tree), int(p.build.adaptive), p.grid_x, p.grid_y, p.table_bytes, p.slot_bytes, p.lds_bytes, p.total_items, p.first_chunk, max_slot_bytes, workgroup_lds_bytes,
					p.refusal);
	}
	return 0;
}
