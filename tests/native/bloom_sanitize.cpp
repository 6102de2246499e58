// tests/native/bloom_sanitize.cpp — the main() of `make sanitize-bloom`: rt_amd/csrc/bloom.cpp and the serial restatement
// (tests/native/bloom_reference.cpp) under AddressSanitizer and UndefinedBehaviorSanitizer, on the CPU.  TEST INFRASTRUCTURE; nothing is
// loaded into python.  It walks what can step outside an array or shift a sign: ragged sizes from 1 x 1 (every level clamps its indices),
// every level count, hostile and denormal channels, in place, the plan at the largest sides, every parameter refusal, and the parser on
// well-formed, malformed, truncated and oversized texts.  Exit status 0 and "bloom_sanitize: ok" on success.
#include "../../include/rt_hip.h"
#include "../../rt_amd/csrc/bloom.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

extern "C" {
int bloom_ref_check(const rt_hip_bloom_params* params, char* message, size_t size);
int bloom_ref_from_spec(const char* spec, rt_hip_bloom_params* out, char* message, size_t size);
int bloom_ref_plan(uint32_t width, uint32_t height, const rt_hip_bloom_params* params, uint32_t* levels, uint32_t* sizes, uint64_t* offsets, float* norm, float* gain, uint64_t* scratch_bytes);
int bloom_ref_frame(uint32_t width, uint32_t height, const float* rgb_in, const rt_hip_bloom_params* params, float* down, float* up, float* layer_out, float* rgb_out);
}

using namespace rt_hip;

namespace
{
	int failures = 0;
	void expect(bool ok, const char* what)
	{
		if (!ok)
		{
			std::fprintf(stderr, "bloom_sanitize: FAILED: %s\n", what);
			failures++;
		}
	}

	uint32_t state = 12345u;
	float next_float() // (0, 1)
	{
		state = state * 1664525u + 1013904223u;
		return (static_cast<float>(state >> 8) + 0.5f) / 16777216.0f;
	}

	void frames()
	{
		const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
		const uint32_t sizes[][2] = { { 1, 1 }, { 1, 2 }, { 2, 1 }, { 3, 3 }, { 5, 3 }, { 16, 16 }, { 37, 21 }, { 67, 35 }, { 65, 65 }, { 1, 300 }, { 300, 1 } };
		for (const auto& size : sizes)
			for (uint32_t levels = 1; levels <= bloom::max_levels; levels++)
			{
				const uint32_t w = size[0], h = size[1];
				std::vector<float> rgb(static_cast<size_t>(w) * h * 3u);
				for (float& c : rgb)
					c = next_float() < 0.1f ? 40.0f * next_float() : next_float();
				if (levels == 3u) // hostile channels, and denormals
				{
					rgb[0] = nan;
					rgb[rgb.size() / 2u] = inf;
					rgb[rgb.size() - 1u] = -3.0f;
					if (rgb.size() > 4u)
						rgb[3] = 1e-39f, rgb[4] = -inf;
				}
				rt_hip_bloom_params p = default_bloom_params();
				p.levels = levels;
				p.scatter = levels % 2u ? 1.0f : 0.5f;
				if (levels == 5u)
					p.threshold = 0.0f, p.knee = 0.0f;
				uint32_t n = 0, level_sizes[2 * bloom::max_levels] = {};
				uint64_t offsets[bloom::max_levels] = {}, scratch = 0;
				float norm = 0, gain = 0;
				expect(bloom_ref_plan(w, h, &p, &n, level_sizes, offsets, &norm, &gain, &scratch) == RT_HIP_OK && n >= 1u && n <= levels, "plan");
				expect(scratch == 12u * (offsets[n - 1u] / 3u + static_cast<uint64_t>(level_sizes[2u * n - 2u]) * level_sizes[2u * n - 1u]), "the last level ends the scratch");
				// every array exactly as large as documented: a stray index is a heap overflow
				std::vector<float> down(scratch / 4u), up(scratch / 4u), layer(rgb.size()), out(rgb.size());
				expect(bloom_ref_frame(w, h, rgb.data(), &p, down.data(), up.data(), layer.data(), out.data()) == RT_HIP_OK, "frame");
				for (const float v : layer)
					expect(std::isfinite(v) && v >= 0.0f, "the layer is finite and not negative");
				std::vector<float> in_place = rgb;
				expect(bloom_ref_frame(w, h, in_place.data(), &p, nullptr, nullptr, nullptr, in_place.data()) == RT_HIP_OK, "in place");
				expect(std::memcmp(in_place.data(), out.data(), out.size() * sizeof(float)) == 0, "in place is the same bytes");
				expect(bloom_ref_frame(w, h, rgb.data(), nullptr, nullptr, nullptr, layer.data(), nullptr) == RT_HIP_OK, "layer only, default parameters");
			}
		uint32_t n = 0, level_sizes[2 * bloom::max_levels] = {};
		uint64_t offsets[bloom::max_levels] = {}, scratch = 0;
		float norm = 0, gain = 0;
		rt_hip_bloom_params p = default_bloom_params();
		p.levels = 8;
		expect(bloom_ref_plan(32768, 32768, &p, &n, level_sizes, offsets, &norm, &gain, &scratch) == RT_HIP_OK && n == 8u && scratch > (3ull << 30), "the largest frame's plan needs 64 bits");
		expect(bloom_ref_plan(0, 4, &p, &n, level_sizes, offsets, &norm, &gain, &scratch) == RT_HIP_INVALID_ARGUMENT, "a side of 0");
	}

	void refusals()
	{
		const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
		char message[256];
		const auto refused = [&](rt_hip_bloom_params p, const char* field)
		{
			const std::string head = std::string("rt_hip_bloom_params: ") + field + " = ";
			expect(bloom_ref_check(&p, message, sizeof message) == RT_HIP_INVALID_ARGUMENT && std::strncmp(message, head.c_str(), head.size()) == 0, field);
			std::vector<float> rgb(12, 2.0f), out(12, 0.0f);
			expect(bloom_ref_frame(2, 2, rgb.data(), &p, nullptr, nullptr, nullptr, out.data()) == RT_HIP_INVALID_ARGUMENT && out[0] == 0.0f, "a refused frame writes nothing");
		};
		for (const float v : { nan, -1.0f, inf, 0x1p21f })
		{
			rt_hip_bloom_params p = default_bloom_params();
			p.threshold = v;
			refused(p, "threshold");
		}
		for (const float v : { nan, -0.5f, 0x1p-21f, 1.5f, inf })
		{
			rt_hip_bloom_params p = default_bloom_params();
			p.knee = v;
			refused(p, "knee");
		}
		for (const float v : { nan, -0.1f, 1025.0f, inf })
		{
			rt_hip_bloom_params p = default_bloom_params();
			p.intensity = v;
			refused(p, "intensity");
		}
		for (const float v : { nan, -0.1f, 1.5f, inf })
		{
			rt_hip_bloom_params p = default_bloom_params();
			p.scatter = v;
			refused(p, "scatter");
		}
		for (const uint32_t v : { 0u, 9u, 0xFFFFFFFFu })
		{
			rt_hip_bloom_params p = default_bloom_params();
			p.levels = v;
			refused(p, "levels");
		}
	}

	void parser()
	{
		char message[256];
		rt_hip_bloom_params p{};
		for (const char* good : { "default", "intensity=0.25", "levels=8", "threshold=2,knee=1.5", "scatter=1,levels=1,intensity=0,threshold=0,knee=0", "knee=.25", "intensity=1e-1" })
			expect(bloom_ref_from_spec(good, &p, message, sizeof message) == RT_HIP_OK && bloom_ref_check(&p, message, sizeof message) == RT_HIP_OK, good);
		const std::string oversized(5000, 'x'), long_value = "intensity=" + std::string(4000, '1'), many = [] {
			std::string s;
			for (int i = 0; i < 500; i++)
				s += "glow=1,";
			return s;
		}();
		for (const char* bad : { "", "bloom", "intensity", "intensity=", "=1", "=", ",", "intensity=0.1,", ",intensity=0.1", "intensity=0.1;knee=0.2", "intensity=0.1,intensity=0.2", "glow=1", "intensity= 1", "intensity=+1",
								 "intensity=-1", "intensity=nan", "intensity=inf", "intensity=0x1p0", "intensity=1e99", "levels=2.5", "levels=0", "levels=9", "levels=99999999999999999999", "knee=2", "scatter=1.5", "threshold=1,knee",
								 oversized.c_str(), long_value.c_str(), many.c_str() })
		{
			rt_hip_bloom_params untouched = default_bloom_params();
			untouched.levels = 3;
			expect(bloom_ref_from_spec(bad, &untouched, message, sizeof message) == RT_HIP_INVALID_ARGUMENT && untouched.levels == 3u, bad);
			expect(std::strncmp(message, "rt_hip_bloom_from_spec: '", 25) == 0 && std::strlen(message) < 200u, "the message quotes the text and fits");
		}
		// truncated texts: every prefix of a long good one, each in a heap block of exactly its size
		const std::string whole = "threshold=1.25,knee=0.75,intensity=0.125,scatter=0.5,levels=7";
		for (size_t length = 0; length <= whole.size(); length++)
		{
			char* const text = static_cast<char*>(std::malloc(length + 1u));
			std::memcpy(text, whole.data(), length);
			text[length] = 0;
			(void)bloom_ref_from_spec(text, &p, message, sizeof message);
			std::free(text);
		}
		expect(bloom_ref_from_spec(nullptr, &p, message, sizeof message) == RT_HIP_INVALID_ARGUMENT && bloom_ref_from_spec("default", nullptr, message, sizeof message) == RT_HIP_INVALID_ARGUMENT, "NULL arguments");
	}
}

int main()
{
	frames();
	refusals();
	parser();
	if (failures)
		return 1;
	std::puts("bloom_sanitize: ok");
	return 0;
}
