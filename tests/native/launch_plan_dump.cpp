// tests/native/launch_plan_dump.cpp — the launch policy of rt_amd/csrc/launch_plan.cpp on the CPU (tests/test_launch_plan.py).
// Built from this file and launch_plan.cpp alone, with the host compiler and nothing of ROCm: that it builds is the proof that the
// policy is host-only.  Reads one launch_request per line from standard input —
//     n_spheres n_planes planes_tame width local_rows samples_per_pixel camera(0 pinhole, 1 plain eye, 2 other) flags host_frame fast_arithmetic
// — and prints the request followed by every field of its launch_plan, one line per request, under a header line that names the columns.
#include "../../rt_amd/csrc/launch_plan.hpp"

#include <cinttypes>
#include <cstdio>

int main()
{
	using namespace rt_hip;
	std::printf("# n_spheres n_planes planes_tame width local_rows samples_per_pixel camera flags host_frame fast_arithmetic | variant big_scene "
				"chunks pixels_log2 tile_w_log2 tiles_x tiles_y block_items lane_cap sparse_rays halves item_samples | "
				"scan planes general_camera sub_chunk_items sm_table | grid_x grid_y table_bytes slot_bytes lds_bytes total_items item_sums_bytes pixel_done_bytes persistent_slot per_cu_cap | "
				"four_tile_slot_bytes sample_chunk\n");
	unsigned n_spheres, n_planes, planes_tame, width, local_rows, samples_per_pixel, camera, flags, host_frame, fast_arithmetic;
	while (std::scanf("%u %u %u %u %u %u %u %u %u %u", &n_spheres, &n_planes, &planes_tame, &width, &local_rows, &samples_per_pixel, &camera, &flags, &host_frame, &fast_arithmetic) == 10)
	{
		launch_request r{};
		r.n_spheres = n_spheres, r.n_planes = n_planes, r.planes_tame = planes_tame != 0;
		r.width = width, r.local_rows = local_rows, r.samples_per_pixel = samples_per_pixel;
		r.camera = static_cast<camera_form>(camera);
		r.flags = flags, r.host_frame = host_frame != 0, r.fast_arithmetic = fast_arithmetic != 0;
		const launch_plan p = plan_launch(r);
		const queue_params& q = p.queue;
		std::printf("%u %u %u %u %u %u %u %u %u %u | %u %d %u %u %u %u %u %u %u %u %u %u | %d %d %d %d %d | %u %u %zu %zu %zu %" PRIu64 " %zu %zu %d %d | %zu %u\n",
					n_spheres, n_planes, planes_tame, width, local_rows, samples_per_pixel, camera, flags, host_frame, fast_arithmetic,
					p.variant, int(p.big_scene), q.chunks, q.pixels_log2, q.tile_w_log2, q.tiles_x, q.tiles_y, q.block_items, q.lane_cap, q.sparse_rays, q.halves, q.item_samples,
					p.build.scan, p.build.planes, int(p.build.general_camera), int(p.build.sub_chunk_items), int(p.build.sm_table),
					p.grid_x, p.grid_y, p.table_bytes, p.slot_bytes, p.lds_bytes, p.total_items, p.item_sums_bytes, p.pixel_done_bytes, p.persistent_slot, p.per_cu_cap,
					4u * tile_slot_bytes(q), sample_chunk);
	}
	return 0;
}
