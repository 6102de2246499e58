// tests/native/sky_band_dump.cpp — rt_amd/csrc/sky_band.cpp on the CPU (tests/test_sky_band_rule.py; `make sanitize-sky-band`).
// Built from this file, sky_band.cpp and frame_setup.cpp alone, with the host compiler and nothing of ROCm: that it builds is the
// proof that the rule is host-only.  Reads one request per line from standard input —
//     band flags pass adaptive scan n_planes width height rank world stripe_rows samples_per_pixel max_bounces m0 .. m15 n_spheres { cx cy cz r2 }
//     time repeats <the same fields>
// (flags in hex; m0 .. m15 the inverse view-projection's and cx .. r2 the sphere table's binary32 BIT PATTERNS in hex: the rows the
// kernels read, radius squared) — and prints one line each:
//     band rows=<R> pinhole=<0|1>
//     time rows=<R> ns_per_call=<mean over the repeats>
#include "../../rt_amd/csrc/frame_setup.hpp"
#include "../../rt_amd/csrc/sky_band.hpp"

#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

int main()
{
	using namespace rt_hip;
	char kind[16];
	while (std::scanf("%15s", kind) == 1)
	{
		const bool timed = !std::strcmp(kind, "time");
		if (!timed && std::strcmp(kind, "band"))
			return 2;
		unsigned repeats = 1;
		if (timed && std::scanf("%u", &repeats) != 1)
			return 2;
		frame_request r{};
		unsigned flags, pass, adaptive, n_planes, n_spheres;
		int scan;
		if (std::scanf("%x %u %u %d %u %u %u %u %u %u %u %u", &flags, &pass, &adaptive, &scan, &n_planes, &r.width, &r.height, &r.partition.rank, &r.partition.world, &r.partition.stripe_rows, &r.samples_per_pixel, &r.max_bounces) != 12)
			return 2;
		uint32_t m[16];
		for (uint32_t& word : m)
			if (std::scanf("%x", &word) != 1)
				return 2;
		std::memcpy(r.inverse_view_projection, m, sizeof(m));
		if (std::scanf("%u", &n_spheres) != 1 || n_spheres > 4096u)
			return 2;
		std::vector<uint32_t> words(static_cast<size_t>(n_spheres) * 4u);
		for (uint32_t& word : words)
			if (std::scanf("%x", &word) != 1)
				return 2;
		std::vector<float> table(words.size() + 4u); // (never empty: data() of the request is a valid pointer)
		if (!words.empty())
			std::memcpy(table.data(), words.data(), words.size() * sizeof(uint32_t));
		if (!r.width || !r.height || !r.partition.world || !r.partition.stripe_rows)
			return 2;
		const frame_params f = make_frame_params(r);
		const sky_band_request request = { table.data(), n_spheres, n_planes, flags, pass != 0, adaptive != 0, scan, &f };
		uint32_t rows = 0;
		const auto t0 = std::chrono::steady_clock::now();
		for (unsigned i = 0; i < repeats; i++)
		{
			rows = sky_band_rows(request);
			asm volatile("" : : "r"(rows) : "memory"); // (every repeat is a call)
		}
		const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
		if (timed)
			std::printf("time rows=%u ns_per_call=%.0f\n", rows, ns / (repeats ? repeats : 1u));
		else
			std::printf("band rows=%u pinhole=%u\n", rows, f.pinhole);
	}
	return 0;
}
