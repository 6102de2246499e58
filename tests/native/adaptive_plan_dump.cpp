// tests/native/adaptive_plan_dump.cpp — the host-only unit of adaptive sampling on the CPU (tests/test_adaptive_host.py): the defaults,
// the parameter check and the sequencing of an accumulation (rt_amd/csrc/adaptive.cpp), the flags an adaptive pass takes
// (rt_amd/csrc/progressive.cpp) and the launch plan of an adaptive pass (rt_amd/csrc/launch_plan.cpp).  Built from this file and those
// three alone, with the host compiler and nothing of ROCm.  One command per line of standard input, one line of output each:
//     defaults
//         -> threshold floor (both as words) min_samples
//     size pass_samples
//         -> the pass size (adaptive_pass_size)
//     check threshold floor (both as words) min_samples pass_size
//         -> status and the message ("-" where there is none)
//     next started samples_done active_pixels <adaptive key of the state> <adaptive key of the request>
//         -> restart first_sample n_samples whole_pass
//            (an adaptive key: fingerprint samples_per_pixel max_bounces 16 x matrix word width height seed flags | threshold floor (words) min_samples pass_samples)
//     complete cap samples_done active_pixels
//         -> 0 or 1
//     flag flags
//         -> the refused flag's name, or "-"
//     plan n_spheres n_planes planes_tame width local_rows samples_per_pixel camera flags pass_first_sample pass_samples
//         -> name=value for the fields of an adaptive pass's launch_plan
#include "../../rt_amd/csrc/adaptive.hpp"
#include "../../rt_amd/csrc/launch_plan.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstring>

using namespace rt_hip;

static uint32_t word_of(float f)
{
	uint32_t w;
	std::memcpy(&w, &f, sizeof w);
	return w;
}
static float float_of(uint32_t w)
{
	float f;
	std::memcpy(&f, &w, sizeof f);
	return f;
}

static bool read_key(adaptive_key& key)
{
	unsigned long long fingerprint, seed;
	unsigned words[16];
	frame_key& frame = key.frame;
	if (std::scanf("%llu %u %u", &fingerprint, &frame.samples_per_pixel, &frame.max_bounces) != 3)
		return false;
	for (unsigned& word : words)
		if (std::scanf("%u", &word) != 1)
			return false;
	if (std::scanf("%u %u %llu %u", &frame.width, &frame.height, &seed, &frame.flags) != 4)
		return false;
	frame.scene_fingerprint = fingerprint, frame.seed = seed;
	for (int i = 0; i < 16; i++)
		frame.inverse_view_projection[i] = float_of(words[i]);
	return std::scanf("%u %u %u %u", &key.threshold_bits, &key.floor_bits, &key.min_samples, &key.pass_samples) == 4;
}

int main()
{
	char command[16];
	while (std::scanf("%15s", command) == 1)
	{
		if (!std::strcmp(command, "defaults"))
		{
			const rt_hip_adaptive_params p = default_adaptive_params();
			std::printf("%u %u %u\n", word_of(p.threshold), word_of(p.floor), p.min_samples);
		}
		else if (!std::strcmp(command, "size"))
		{
			unsigned pass_samples;
			if (std::scanf("%u", &pass_samples) != 1)
				return 1;
			std::printf("%" PRIu64 "\n", adaptive_pass_size(pass_samples));
		}
		else if (!std::strcmp(command, "check"))
		{
			unsigned threshold, floor, min_samples;
			unsigned long long pass_size;
			if (std::scanf("%u %u %u %llu", &threshold, &floor, &min_samples, &pass_size) != 4)
				return 1;
			rt_hip_adaptive_params p{};
			p.threshold = float_of(threshold), p.floor = float_of(floor), p.min_samples = min_samples;
			const adaptive_check c = check_adaptive_params(p, pass_size);
			std::printf("%d %s\n", int(c.status), c.status ? c.message : "-");
		}
		else if (!std::strcmp(command, "next"))
		{
			unsigned started;
			adaptive_state state;
			adaptive_key wanted{};
			if (std::scanf("%u %u %u", &started, &state.samples_done, &state.active_pixels) != 3 || !read_key(state.key) || !read_key(wanted))
				return 1;
			state.started = started != 0;
			const adaptive_step step = next_adaptive_pass(state, wanted);
			std::printf("%d %u %u %d\n", int(step.restart), step.first_sample, step.n_samples, int(step.whole_pass));
		}
		else if (!std::strcmp(command, "complete"))
		{
			unsigned cap, done, active;
			if (std::scanf("%u %u %u", &cap, &done, &active) != 3)
				return 1;
			std::printf("%d\n", int(adaptive_complete(cap, done, active)));
		}
		else if (!std::strcmp(command, "flag"))
		{
			unsigned flags;
			if (std::scanf("%u", &flags) != 1)
				return 1;
			const char* const refused = refused_adaptive_flag(flags);
			std::printf("%s\n", refused ? refused : "-");
		}
		else if (!std::strcmp(command, "plan"))
		{
			unsigned n_spheres, n_planes, planes_tame, width, local_rows, samples_per_pixel, camera, flags, first, samples;
			if (std::scanf("%u %u %u %u %u %u %u %u %u %u", &n_spheres, &n_planes, &planes_tame, &width, &local_rows, &samples_per_pixel, &camera, &flags, &first, &samples) != 10)
				return 1;
			launch_request r{};
			r.n_spheres = n_spheres, r.n_planes = n_planes, r.planes_tame = planes_tame != 0;
			r.width = width, r.local_rows = local_rows, r.samples_per_pixel = samples_per_pixel;
			r.camera = static_cast<camera_form>(camera);
			r.flags = flags;
			r.pass_first_sample = first, r.pass_samples = samples, r.adaptive = true;
			const launch_plan p = plan_launch(r);
			const queue_params& q = p.queue;
			const int code = p.build.adaptive ? (p.build.scan == scan_bvh ? scan_bvh_adapt : scan_resident_adapt) : p.build.scan;
			std::printf("variant=%u chunks=%u pixels_log2=%u tile_w_log2=%u tiles_x=%u tiles_y=%u scan=%d scan_code=%d is_pass=%d is_adaptive=%d scan_of=%d planes=%d general_camera=%d sm_table=%d pass=%d adaptive=%d grid_x=%u grid_y=%u "
						"slot_bytes=%zu lds_bytes=%zu first_chunk=%u\n",
						p.variant, q.chunks, q.pixels_log2, q.tile_w_log2, q.tiles_x, q.tiles_y, p.build.scan, code, int(scan_is_pass(code)), int(scan_is_adaptive(code)), scan_of(code), p.build.planes, int(p.build.general_camera),
						int(p.build.sm_table), int(p.build.pass), int(p.build.adaptive), p.grid_x, p.grid_y, p.slot_bytes, p.lds_bytes, p.first_chunk);
		}
		else
			return 1;
	}
	return 0;
}
