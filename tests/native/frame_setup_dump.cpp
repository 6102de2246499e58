// tests/native/frame_setup_dump.cpp — rt_amd/csrc/frame_setup.cpp on the CPU (tests/test_frame_setup.py).
// Built from this file and frame_setup.cpp alone, with the host compiler and nothing of ROCm: that it builds is the proof that the
// unit is host-only.  Reads one request per line from standard input —
//     frame width height rank world stripe_rows samples_per_pixel max_bounces seed whole_frame_buffers m0 .. m15
//     check width height flags has_partition rank world stripe_rows
// (seed decimal, m0 .. m15 the inverse view-projection's binary32 BIT PATTERNS in hex, flags in hex) — and prints one line each:
//     frame camera_form=<0 pinhole, 1 plain eye, 2 other> <field>=<hex>[,<hex> ..] ..      every field of frame_params, bit patterns
//     check status=<rt_hip_status> flags=<hex> bvh_device_build=<0|1> rank=<n> world=<n> stripe_rows=<n> | <message>
#include "../../rt_amd/csrc/frame_setup.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstring>

namespace
{
	void put(const char* name, const uint32_t* words, int count)
	{
		std::printf(" %s=", name);
		for (int i = 0; i < count; i++)
			std::printf("%s%08x", i ? "," : "", words[i]);
	}
	void put(const char* name, const float* values, int count)
	{
		uint32_t words[4];
		std::memcpy(words, values, sizeof(float) * static_cast<size_t>(count));
		put(name, words, count);
	}
}

#define PUT(field) put(#field, &f.field, 1)
#define PUT_ALL(field) put(#field, f.field, static_cast<int>(sizeof(f.field) / sizeof(f.field[0])))

int main()
{
	using namespace rt_hip;
	char kind[16];
	while (std::scanf("%15s", kind) == 1)
	{
		if (!std::strcmp(kind, "frame"))
		{
			frame_request r{};
			unsigned whole = 0;
			uint32_t m[16];
			if (std::scanf("%u %u %u %u %u %u %u %" SCNu64 " %u", &r.width, &r.height, &r.partition.rank, &r.partition.world, &r.partition.stripe_rows, &r.samples_per_pixel, &r.max_bounces, &r.seed, &whole) != 9)
				return 2;
			for (uint32_t& word : m)
				if (std::scanf("%x", &word) != 1)
					return 2;
			std::memcpy(r.inverse_view_projection, m, sizeof(m));
			r.whole_frame_buffers = whole != 0;
			const frame_params f = make_frame_params(r);
			static_assert(sizeof(frame_params) == (14 + 16 + 1 + 18 + 1 + 24) * 4, "a field was added: print it below");
			std::printf("frame camera_form=%u", static_cast<unsigned>(camera_form_of(f)));
			PUT(width), PUT(height), PUT(local_rows), PUT(rank), PUT(world), PUT(stripe_rows), PUT(stripe_shift), PUT(frame_rows);
			PUT(samples_per_pixel), PUT(max_bounces), PUT(frame_key_a), PUT(frame_key_b), PUT(sx), PUT(neg_sy);
			PUT_ALL(mx), PUT_ALL(my), PUT_ALL(k_near), PUT_ALL(k_far);
			PUT(pinhole), PUT_ALL(ray_d0), PUT_ALL(ray_d1), PUT_ALL(ray_d2), PUT_ALL(ray_j1), PUT_ALL(ray_j2), PUT_ALL(ray_eye);
			PUT(eye_form), PUT_ALL(eye_q0), PUT_ALL(eye_q1), PUT_ALL(eye_q2), PUT_ALL(eye_jq1), PUT_ALL(eye_jq2);
			PUT(eye_w0), PUT(eye_w1), PUT(eye_w2), PUT(eye_jw1), PUT(eye_jw2), PUT_ALL(eye_e), PUT(eye_zws);
			std::printf("\n");
		}
		else if (!std::strcmp(kind, "check"))
		{
			unsigned width, height, flags, has_partition;
			rt_hip_partition part{};
			if (std::scanf("%u %u %x %u %u %u %u", &width, &height, &flags, &has_partition, &part.rank, &part.world, &part.stripe_rows) != 7)
				return 2;
			const render_check c = check_render_request(width, height, flags, has_partition ? &part : nullptr);
			std::printf("check status=%d flags=%x bvh_device_build=%d rank=%u world=%u stripe_rows=%u | %s\n", static_cast<int>(c.status), c.flags, int(c.bvh_device_build), c.partition.rank, c.partition.world, c.partition.stripe_rows, c.message);
		}
		else
			return 2;
	}
	return 0;
}
