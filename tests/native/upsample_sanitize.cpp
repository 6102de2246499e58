// tests/native/upsample_sanitize.cpp — the program of `make sanitize-upsample`: guided upsampling's host-only unit (rt_amd/csrc/upsample.cpp)
// and its serial restatement (tests/native/upsample_reference.cpp over rt_amd/csrc/upsample_rules.hpp) behind a main() of their own, under
// AddressSanitizer and UndefinedBehaviorSanitizer.  CPU only; nothing is loaded into python.  The arrays are sized EXACTLY, so a tap
// fetched outside the low frame or a pixel stored outside the full one is a heap overflow the sanitizer reports.
#include "../../include/rt_hip.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

extern "C" {
void upsample_ref_default_params(rt_hip_upsample_params* out);
int upsample_ref_check(const rt_hip_upsample_params* params, char* message, size_t size);
int upsample_ref_check_sizes(uint32_t W, uint32_t H, uint32_t w, uint32_t h, char* message, size_t size);
int upsample_ref_low_size(uint32_t W, uint32_t H, uint32_t factor, uint32_t* w, uint32_t* h, char* message, size_t size);
void upsample_ref_source_of(uint32_t x, uint32_t W, uint32_t w, int32_t* first, float* b0, float* b1);
int upsample_ref_frame(uint32_t W, uint32_t H, uint32_t w, uint32_t h, const float* rgb_low, const float* guide_low, const float* guide_full, const rt_hip_upsample_params* params, float* rgb_out, uint32_t* rgba_out,
					   uint32_t* orphans_out);
}

namespace
{
	int failures = 0;
	void expect(bool ok, const char* what)
	{
		if (!ok)
		{
			std::fprintf(stderr, "FAILED: %s\n", what);
			failures++;
		}
	}

	uint32_t state = 12345u;
	float uniform() // a small generator of its own: reproducible, no library state
	{
		state = state * 1664525u + 1013904223u;
		return static_cast<float>(state >> 8) / 16777216.0f;
	}

	std::vector<float> make_guide(uint32_t width, uint32_t height)
	{
		std::vector<float> g(static_cast<size_t>(width) * height * 8u);
		for (size_t i = 0; i < g.size() / 8u; i++)
		{
			const bool sky = uniform() < 0.25f;
			const uint32_t id = sky ? 0u : 1u + static_cast<uint32_t>(uniform() * 4.0f);
			const float record[8] = { 0.0f, sky ? 0.0f : 0.6f, sky ? 0.0f : 0.8f, sky ? -1.0f : 1.0f + 2.0f * uniform(), 0.5f, 0.25f + 0.5f * uniform(), 0.5f, 0.0f };
			std::memcpy(&g[i * 8u], record, sizeof record);
			std::memcpy(&g[i * 8u + 7u], &id, sizeof id);
		}
		return g;
	}

	void run_frame(uint32_t W, uint32_t H, uint32_t w, uint32_t h, bool poison)
	{
		std::vector<float> low(static_cast<size_t>(w) * h * 3u);
		for (float& v : low)
			v = uniform();
		if (poison)
		{
			low[0] = std::numeric_limits<float>::quiet_NaN();
			low[low.size() - 1u] = std::numeric_limits<float>::infinity();
		}
		const std::vector<float> guide_low = make_guide(w, h), guide_full = make_guide(W, H);
		std::vector<float> out(static_cast<size_t>(W) * H * 3u);
		std::vector<uint32_t> rgba(static_cast<size_t>(W) * H);
		uint32_t orphans = ~0u;
		expect(upsample_ref_frame(W, H, w, h, low.data(), guide_low.data(), guide_full.data(), nullptr, out.data(), rgba.data(), &orphans) == RT_HIP_OK, "a frame is accepted");
		expect(orphans <= W * H, "the orphans are at most the pixels");
		bool finite = true;
		for (const float v : out)
			finite = finite && std::isfinite(v);
		expect(finite, "no output is NaN or infinite");
		// either output alone, and neither
		expect(upsample_ref_frame(W, H, w, h, low.data(), guide_low.data(), guide_full.data(), nullptr, out.data(), nullptr, nullptr) == RT_HIP_OK, "only the float output");
		expect(upsample_ref_frame(W, H, w, h, low.data(), guide_low.data(), guide_full.data(), nullptr, nullptr, rgba.data(), nullptr) == RT_HIP_OK, "only the packed output");
		std::printf("frame %ux%u from %ux%u: %u orphans\n", W, H, w, h, orphans);
	}
}

int main()
{
	// ragged sizes: one pixel, one low pixel under many, no whole ratio, w == W, a low frame as high as the full one
	const uint32_t shapes[][4] = { { 1, 1, 1, 1 }, { 2, 2, 1, 1 }, { 17, 17, 9, 9 }, { 33, 5, 33, 5 }, { 37, 3, 1, 1 }, { 70, 41, 18, 11 }, { 7, 9, 3, 9 }, { 96, 54, 24, 14 } };
	for (const auto& s : shapes)
	{
		run_frame(s[0], s[1], s[2], s[3], false);
		run_frame(s[0], s[1], s[2], s[3], true);
	}
	// the geometry at the largest side: the first and the last pixel
	for (const uint32_t w : { 1u, 3u, (1u << 22) - 1u, 1u << 22 })
	{
		int32_t first = 0;
		float b0 = 0.0f, b1 = 0.0f;
		upsample_ref_source_of(0u, 1u << 22, w, &first, &b0, &b1);
		expect(first >= -1 && first <= 0 && b0 + b1 == 1.0f, "the first pixel of the widest frame");
		upsample_ref_source_of((1u << 22) - 1u, 1u << 22, w, &first, &b0, &b1);
		expect(first == static_cast<int32_t>(w) - 1 && b0 >= 0.0f && b1 >= 0.0f, "the last pixel of the widest frame");
	}

	// every refusal
	char message[256];
	rt_hip_upsample_params p;
	upsample_ref_default_params(&p);
	expect(upsample_ref_check(&p, message, sizeof message) == RT_HIP_OK, "the defaults are accepted");
	const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
	{
		rt_hip_upsample_params bad = p;
		bad.normal_squarings = 9;
		expect(upsample_ref_check(&bad, message, sizeof message) == RT_HIP_INVALID_ARGUMENT && std::strstr(message, "normal_squarings"), "normal_squarings = 9");
		expect(upsample_ref_check(&bad, nullptr, 0) == RT_HIP_INVALID_ARGUMENT, "... without a message buffer");
		expect(upsample_ref_check(&bad, message, 4) == RT_HIP_INVALID_ARGUMENT && std::strlen(message) == 3, "... into a short one");
	}
	for (const float v : { 0.0f, -1.0f, nan, inf })
	{
		rt_hip_upsample_params bad = p;
		bad.sigma_albedo = v;
		expect(upsample_ref_check(&bad, message, sizeof message) == RT_HIP_INVALID_ARGUMENT && std::strstr(message, "sigma_albedo"), "a bad sigma_albedo");
		bad = p;
		bad.sigma_depth = v;
		expect(upsample_ref_check(&bad, message, sizeof message) == RT_HIP_INVALID_ARGUMENT && std::strstr(message, "sigma_depth"), "a bad sigma_depth");
	}
	for (const float v : { 0.0f, -0.5f, 1.5f, nan, inf })
	{
		rt_hip_upsample_params bad = p;
		bad.min_weight = v;
		expect(upsample_ref_check(&bad, message, sizeof message) == RT_HIP_INVALID_ARGUMENT && std::strstr(message, "min_weight"), "a bad min_weight");
		float pixel[8] = {};
		expect(upsample_ref_frame(1, 1, 1, 1, pixel, pixel, pixel, &bad, pixel, nullptr, nullptr) == RT_HIP_INVALID_ARGUMENT, "... refused by the frame too");
	}
	const uint32_t bad_sizes[][4] = { { 0, 1, 1, 1 }, { 1, 0, 1, 1 }, { (1u << 22) + 1u, 1, 1, 1 }, { 1, (1u << 22) + 1u, 1, 1 }, { 4, 4, 0, 1 }, { 4, 4, 1, 0 }, { 4, 4, 5, 1 }, { 4, 4, 1, 5 }, { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu } };
	for (const auto& s : bad_sizes)
	{
		expect(upsample_ref_check_sizes(s[0], s[1], s[2], s[3], message, sizeof message) == RT_HIP_INVALID_ARGUMENT && std::strstr(message, "frame"), "bad sizes");
		float pixel[8] = {};
		expect(upsample_ref_frame(s[0], s[1], s[2], s[3], pixel, pixel, pixel, nullptr, pixel, nullptr, nullptr) == RT_HIP_INVALID_ARGUMENT, "... refused by the frame too");
	}
	uint32_t w = 7, h = 7;
	for (const uint32_t factor : { 0u, 5u, 0xFFFFFFFFu })
		expect(upsample_ref_low_size(1920, 1080, factor, &w, &h, message, sizeof message) == RT_HIP_INVALID_ARGUMENT && std::strstr(message, "factor") && w == 7 && h == 7, "a bad factor");
	expect(upsample_ref_low_size(1920, 1080, 2, nullptr, &h, message, sizeof message) == RT_HIP_INVALID_ARGUMENT, "a NULL output");
	expect(upsample_ref_low_size(0, 1080, 2, &w, &h, message, sizeof message) == RT_HIP_INVALID_ARGUMENT, "an empty frame");
	expect(upsample_ref_low_size(1u << 22, 1u << 22, 4, &w, &h, message, sizeof message) == RT_HIP_OK && w == (1u << 20) && h == (1u << 20), "the largest frame");
	expect(upsample_ref_low_size(97, 55, 4, &w, &h, message, sizeof message) == RT_HIP_OK && w == 25 && h == 14, "97 x 55 by 4");

	if (failures)
	{
		std::fprintf(stderr, "%d checks failed\n", failures);
		return 1;
	}
	std::printf("all checks passed\n");
	return 0;
}
