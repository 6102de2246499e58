// tests/native/pass_plan_dump.cpp — the host-only policy of progressive frames on the CPU (tests/test_pass_plan.py): the launch plan of a
// pass (rt_amd/csrc/launch_plan.cpp), the sequencing of passes and the flags a pass takes (rt_amd/csrc/progressive.cpp).  Built from this
// file and those two alone, with the host compiler and nothing of ROCm.  One command per line of standard input, one line of output each:
//     plan n_spheres n_planes planes_tame width local_rows samples_per_pixel camera flags host_frame fast_arithmetic pass_first_sample pass_samples
//         -> name=value for every field of the launch_plan
//     next started samples_done <key of the state> <key of the request> pass_samples
//         -> restart first_sample n_samples complete         (a key: fingerprint samples_per_pixel max_bounces 16 x matrix word width height seed flags)
//     flag flags
//         -> the refused flag's name, or "-"
#include "../../rt_amd/csrc/launch_plan.hpp"
#include "../../rt_amd/csrc/progressive.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstring>

using namespace rt_hip;

static bool read_key(frame_key& key)
{
	unsigned long long fingerprint, seed;
	unsigned words[16];
	if (std::scanf("%llu %u %u", &fingerprint, &key.samples_per_pixel, &key.max_bounces) != 3)
		return false;
	for (unsigned& word : words)
		if (std::scanf("%u", &word) != 1)
			return false;
	if (std::scanf("%u %u %llu %u", &key.width, &key.height, &seed, &key.flags) != 4)
		return false;
	key.scene_fingerprint = fingerprint, key.seed = seed;
	for (int i = 0; i < 16; i++)
	{
		const uint32_t bits = words[i];
		std::memcpy(&key.inverse_view_projection[i], &bits, sizeof bits);
	}
	return true;
}

int main()
{
	char command[16];
	while (std::scanf("%15s", command) == 1)
	{
		if (!std::strcmp(command, "plan"))
		{
			unsigned n_spheres, n_planes, planes_tame, width, local_rows, samples_per_pixel, camera, flags, host_frame, fast_arithmetic, first, samples;
			if (std::scanf("%u %u %u %u %u %u %u %u %u %u %u %u", &n_spheres, &n_planes, &planes_tame, &width, &local_rows, &samples_per_pixel, &camera, &flags, &host_frame, &fast_arithmetic, &first, &samples) != 12)
				return 1;
			launch_request r{};
			r.n_spheres = n_spheres, r.n_planes = n_planes, r.planes_tame = planes_tame != 0;
			r.width = width, r.local_rows = local_rows, r.samples_per_pixel = samples_per_pixel;
			r.camera = static_cast<camera_form>(camera);
			r.flags = flags, r.host_frame = host_frame != 0, r.fast_arithmetic = fast_arithmetic != 0;
			r.pass_first_sample = first, r.pass_samples = samples;
			const launch_plan p = plan_launch(r);
			const queue_params& q = p.queue;
			std::printf("variant=%u big_scene=%d chunks=%u pixels_log2=%u tile_w_log2=%u tiles_x=%u tiles_y=%u block_items=%u lane_cap=%u sparse_rays=%u halves=%u item_samples=%u "
						"scan=%d planes=%d general_camera=%d sub_chunk_items=%d sm_table=%d pass=%d grid_x=%u grid_y=%u table_bytes=%zu slot_bytes=%zu lds_bytes=%zu total_items=%" PRIu64
						" item_sums_bytes=%zu pixel_done_bytes=%zu persistent_slot=%d per_cu_cap=%d first_chunk=%u\n",
						p.variant, int(p.big_scene), q.chunks, q.pixels_log2, q.tile_w_log2, q.tiles_x, q.tiles_y, q.block_items, q.lane_cap, q.sparse_rays, q.halves, q.item_samples, p.build.scan, p.build.planes,
						int(p.build.general_camera), int(p.build.sub_chunk_items), int(p.build.sm_table), int(p.build.pass), p.grid_x, p.grid_y, p.table_bytes, p.slot_bytes, p.lds_bytes, p.total_items, p.item_sums_bytes,
						p.pixel_done_bytes, p.persistent_slot, p.per_cu_cap, p.first_chunk);
		}
		else if (!std::strcmp(command, "next"))
		{
			unsigned started;
			pass_state state;
			pass_request request{};
			if (std::scanf("%u %u", &started, &state.samples_done) != 2 || !read_key(state.key) || !read_key(request.key) || std::scanf("%u", &request.pass_samples) != 1)
				return 1;
			state.started = started != 0;
			const pass_step step = next_pass(state, request);
			std::printf("%d %u %u %d\n", int(step.restart), step.first_sample, step.n_samples, int(step.complete));
		}
		else if (!std::strcmp(command, "flag"))
		{
			unsigned flags;
			if (std::scanf("%u", &flags) != 1)
				return 1;
			const char* const refused = refused_pass_flag(flags);
			std::printf("%s\n", refused ? refused : "-");
		}
		else
			return 1;
	}
	return 0;
}
