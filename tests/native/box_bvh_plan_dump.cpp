// tests/native/box_bvh_plan_dump.cpp — what a frame with RT_HIP_FLAG_BOX_BVH is told on the host, on the CPU (tests/test_box_bvh_plan.py);
// box_plan_dump.cpp with two more fields: box_tree, and `build`, the scan code of the render_queue instantiation the plan names:
// the refusals of the request (rt_amd/csrc/frame_setup.cpp, check_render_request) and the launch plan (rt_amd/csrc/launch_plan.cpp).
// Built from this file and those two alone, with the host compiler and nothing of ROCm.  Reads one request per line from standard input —
//     n_spheres n_planes n_boxes width local_rows samples_per_pixel camera(0 pinhole, 1 plain eye, 2 other) flags host_frame
// — and prints one line each: `refused <status> <message>` where rt_hip_render_device refuses it (the request's check first, then the
// plan's own refusal), else name=value for every field of the launch_plan.
#include "../../rt_amd/csrc/frame_setup.hpp"
#include "../../rt_amd/csrc/launch_plan.hpp"

#include <cinttypes>
#include <cstdio>

int main()
{
	using namespace rt_hip;
	unsigned n_spheres, n_planes, n_boxes, width, local_rows, samples_per_pixel, camera, flags, host_frame;
	while (std::scanf("%u %u %u %u %u %u %u %u %u", &n_spheres, &n_planes, &n_boxes, &width, &local_rows, &samples_per_pixel, &camera, &flags, &host_frame) == 9)
	{
		const render_check checked = check_render_request(width, local_rows, flags, nullptr);
		if (checked.status)
		{
			std::printf("refused %d %s\n", int(checked.status), checked.message);
			continue;
		}
		launch_request r{};
		r.n_spheres = n_spheres, r.n_planes = n_planes, r.planes_tame = true, r.n_boxes = n_boxes;
		r.width = width, r.local_rows = local_rows, r.samples_per_pixel = samples_per_pixel;
		r.camera = static_cast<camera_form>(camera);
		r.flags = checked.flags, r.host_frame = host_frame != 0, r.fast_arithmetic = (checked.flags & RT_HIP_FLAG_FAST) != 0;
		const launch_plan p = plan_launch(r);
		if (p.refusal[0])
		{
			std::printf("refused %d rt_hip_render_device: %s\n", int(RT_HIP_UNSUPPORTED), p.refusal);
			continue;
		}
		const queue_params& q = p.queue;
		// (build_of, kernels.hip: the box tree before the box builds before the pass builds)
		const bool tile_per_wave = p.build.scan == scan_resident || p.build.scan == scan_bvh;
		const int build = !tile_per_wave ? p.build.scan
						  : p.build.box_tree ? static_cast<int>(scan_bvh_boxtree)
						  : p.build.boxes	 ? static_cast<int>(p.build.scan == scan_bvh ? scan_bvh_boxes : scan_resident_boxes)
						  : p.build.pass	 ? static_cast<int>(p.build.scan == scan_bvh ? scan_bvh_pass : scan_resident_pass)
											 : p.build.scan;
		std::printf("variant=%u big_scene=%d chunks=%u pixels_log2=%u tile_w_log2=%u tiles_x=%u tiles_y=%u block_items=%u lane_cap=%u sparse_rays=%u halves=%u item_samples=%u "
					"scan=%d planes=%d general_camera=%d sub_chunk_items=%d sm_table=%d pass=%d boxes=%d box_tree=%d build=%d grid_x=%u grid_y=%u table_bytes=%zu slot_bytes=%zu lds_bytes=%zu total_items=%" PRIu64
					" item_sums_bytes=%zu pixel_done_bytes=%zu persistent_slot=%d per_cu_cap=%d first_chunk=%u\n",
					p.variant, int(p.big_scene), q.chunks, q.pixels_log2, q.tile_w_log2, q.tiles_x, q.tiles_y, q.block_items, q.lane_cap, q.sparse_rays, q.halves, q.item_samples, p.build.scan, p.build.planes,
					int(p.build.general_camera), int(p.build.sub_chunk_items), int(p.build.sm_table), int(p.build.pass), int(p.build.boxes), int(p.build.box_tree), build, p.grid_x, p.grid_y, p.table_bytes, p.slot_bytes, p.lds_bytes, p.total_items,
					p.item_sums_bytes, p.pixel_done_bytes, p.persistent_slot, p.per_cu_cap, p.first_chunk);
	}
	return 0;
}
