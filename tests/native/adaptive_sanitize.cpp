// tests/native/adaptive_sanitize.cpp — `make sanitize-adaptive`: adaptive sampling's host-only unit (rt_amd/csrc/adaptive.cpp) and the
// serial restatement of its update step (tests/native/adaptive_reference.cpp) behind a main() of their own, built with
// AddressSanitizer and UndefinedBehaviorSanitizer.  CPU only; nothing here is loaded into python.
#include "../../rt_amd/csrc/adaptive.hpp"
#include "../../rt_amd/csrc/adaptive_rules.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

using namespace rt_hip;

extern "C" int adaptive_ref_step(uint32_t width, uint32_t height, uint32_t pass_samples, uint32_t first_pass, uint32_t whole_pass, const rt_hip_adaptive_params* params, const float* accum, const float* pass_sum, float* moments, uint32_t* state,
								 uint32_t* rgba_out, float* rgb_out, uint32_t* active_pixels);

#define EXPECT(condition)                                                                                              \
	do                                                                                                                 \
	{                                                                                                                  \
		if (!(condition))                                                                                              \
		{                                                                                                              \
			std::fprintf(stderr, "adaptive_sanitize: %s:%d: %s\n", __FILE__, __LINE__, #condition);                   \
			std::exit(1);                                                                                              \
		}                                                                                                              \
	}                                                                                                                  \
	while (false)

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

int main()
{
	// the parameter check: the defaults pass, every field is refused by name
	const rt_hip_adaptive_params d = default_adaptive_params();
	EXPECT(check_adaptive_params(d, 16).status == RT_HIP_OK);
	EXPECT(adaptive_pass_size(0) == 16 && adaptive_pass_size(17) == 32 && adaptive_pass_size(0xFFFFFFFFu) == 0x100000000ull);
	const float bad[] = { -1.0f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity() };
	for (const float value : bad)
	{
		rt_hip_adaptive_params p = d;
		p.threshold = value;
		EXPECT(check_adaptive_params(p, 16).status == RT_HIP_INVALID_ARGUMENT);
		p = d, p.floor = value;
		EXPECT(check_adaptive_params(p, 16).status == RT_HIP_INVALID_ARGUMENT);
	}
	{
		rt_hip_adaptive_params p = d;
		p.min_samples = 31;
		EXPECT(check_adaptive_params(p, 16).status == RT_HIP_INVALID_ARGUMENT);
		EXPECT(check_adaptive_params(d, 32).status == RT_HIP_INVALID_ARGUMENT);
		EXPECT(check_adaptive_params(d, 0x100000000ull).status == RT_HIP_INVALID_ARGUMENT);
	}

	// the sequencing: to completion by the cap (a short last pass), and by "no pixel active"
	frame_key frame{};
	frame.samples_per_pixel = 40, frame.width = 37, frame.height = 23, frame.seed = 7;
	const adaptive_key key = make_adaptive_key(frame, d, 16);
	adaptive_state state;
	uint32_t passes = 0;
	for (;; passes++)
	{
		const adaptive_step step = next_adaptive_pass(state, key);
		if (!step.n_samples)
			break;
		EXPECT(step.restart == (passes == 0));
		EXPECT(step.whole_pass == (step.n_samples == 16u));
		state.started = true, state.key = key, state.samples_done = step.first_sample + step.n_samples, state.active_pixels = 5;
	}
	EXPECT(passes == 3 && state.samples_done == 40);
	state.samples_done = 32, state.active_pixels = 0;
	EXPECT(next_adaptive_pass(state, key).n_samples == 0);
	adaptive_key other = key;
	other.pass_samples = 32;
	EXPECT(next_adaptive_pass(state, other).restart);

	// update steps over a 37 x 23 frame: random sums with NaNs among them, to the cap of 72 with a short last pass of 8
	const uint32_t width = 37, height = 23;
	const size_t pixels = static_cast<size_t>(width) * height;
	std::vector<float> accum(pixels * 3), pass_sum(pixels * 3), moments(pixels * 2, std::numeric_limits<float>::quiet_NaN()), rgb(pixels * 3);
	std::vector<uint32_t> words(pixels, 0xFFFFFFFFu), rgba(pixels);
	uint32_t seed = 12345u, active = 0, previous_active = static_cast<uint32_t>(pixels);
	for (uint32_t pass = 0; pass < 5; pass++)
	{
		const bool whole = pass < 4;
		for (size_t i = 0; i < pixels * 3; i++)
		{
			// flat pixels in the left half of the frame (they converge), noisy ones in the right half, a NaN now and then
			const bool flat = (i / 3) % width < width / 2;
			pass_sum[i] = flat ? 8.0f : static_cast<float>(lcg(seed) >> 8) * 0x1.0p-20f;
			if (lcg(seed) % 211u == 0u)
				pass_sum[i] = std::numeric_limits<float>::quiet_NaN();
			accum[i] = pass ? accum[i] + pass_sum[i] : pass_sum[i];
		}
		const std::vector<uint32_t> before = words;
		EXPECT(adaptive_ref_step(width, height, whole ? 16u : 8u, pass == 0, whole, &d, accum.data(), pass_sum.data(), moments.data(), words.data(), rgba.data(), rgb.data(), &active) == RT_HIP_OK);
		EXPECT(active <= previous_active);
		previous_active = active;
		for (size_t i = 0; i < pixels; i++)
		{
			if (pass && adaptive::is_stopped(before[i]))
				EXPECT(words[i] == before[i]); // monotone
			EXPECT((rgba[i] & 255u) == 255u);
		}
	}
	EXPECT(active < pixels); // the flat half has stopped
	EXPECT(adaptive_ref_step(width, height, 24u, 0, 1, &d, accum.data(), pass_sum.data(), moments.data(), words.data(), nullptr, nullptr, nullptr) == RT_HIP_INVALID_ARGUMENT);
	std::printf("adaptive_sanitize: ok (%u of %zu pixels still active after 72 samples)\n", active, pixels);
	return 0;
}
