// tests/native/tonemap_sanitize.cpp — the program of `make sanitize-tonemap`: tone mapping's host-only unit (rt_amd/csrc/tonemap.cpp) and its
// serial restatement (tests/native/tonemap_reference.cpp over rt_amd/csrc/tonemap_rules.hpp) behind a main() of their own, under
// AddressSanitizer and UndefinedBehaviorSanitizer.  CPU only; nothing is loaded into python.  The arrays are sized EXACTLY, so a pixel read
// or stored outside its frame, a bin outside the histogram or a word outside the state record is a heap overflow the sanitizer reports;
// the parser gets texts in buffers of exactly their length.
#include "../../include/rt_hip.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

extern "C" {
void tonemap_ref_default_params(rt_hip_tonemap_params* out);
int tonemap_ref_check(const rt_hip_tonemap_params* params, char* message, size_t size);
int tonemap_ref_from_spec(const char* spec, rt_hip_tonemap_params* out, char* message, size_t size);
void tonemap_ref_histogram(uint32_t pixels, const float* rgb, uint32_t* histogram);
int tonemap_ref_frame(uint32_t width, uint32_t height, const float* rgb_in, const rt_hip_tonemap_params* params, uint32_t* state, float* rgb_out, uint32_t* rgba_out);
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

	const float not_a_number = std::numeric_limits<float>::quiet_NaN(), infinity = std::numeric_limits<float>::infinity();

	// channels over sixty octaves (both end bins), or nothing but what the meter skips and the curves must survive
	std::vector<float> make_frame(uint32_t pixels, bool hostile)
	{
		std::vector<float> rgb(static_cast<size_t>(pixels) * 3u);
		const float poison[] = { not_a_number, infinity, -infinity, 0.0f, -0.0f, -1.0f, 3.0e38f, 1.0e-45f };
		for (float& v : rgb)
			v = hostile ? poison[static_cast<uint32_t>(uniform() * 8.0f) & 7u] : std::ldexp(1.0f + uniform(), static_cast<int>(uniform() * 60.0f) - 30);
		return rgb;
	}

	void run_frame(uint32_t W, uint32_t H, bool hostile)
	{
		const uint32_t pixels = W * H;
		const std::vector<float> rgb = make_frame(pixels, hostile);
		std::vector<uint32_t> histogram(257u);
		tonemap_ref_histogram(pixels, rgb.data(), histogram.data());
		uint64_t total = 0;
		for (const uint32_t count : histogram)
			total += count;
		expect(total == pixels, "every pixel is in a bin or skipped");
		for (uint32_t curve = 0; curve < 3u; curve++)
			for (const float exposure : { 0.0f, 0.5f })
				for (const float adaptation : { 1.0f, 0.25f })
				{
					rt_hip_tonemap_params p;
					tonemap_ref_default_params(&p);
					p.curve = curve, p.exposure = exposure, p.adaptation = adaptation;
					std::vector<uint32_t> record(8u, 0u);
					std::vector<float> out(rgb.size());
					std::vector<uint32_t> rgba(pixels);
					for (int call = 0; call < 3; call++) // (the record of one call is the next one's: the adaptation sequence)
						expect(tonemap_ref_frame(W, H, rgb.data(), &p, record.data(), out.data(), rgba.data()) == RT_HIP_OK, "a frame is accepted");
					float applied;
					std::memcpy(&applied, &record[0], sizeof applied);
					expect(std::isfinite(applied) && applied > 0.0f, "the exposure is a positive finite number");
					expect(exposure > 0.0f ? record[2] + record[3] == 0u : record[2] + record[3] == pixels, "counted + skipped is every pixel (nothing under a manual exposure)");
					expect(record[4] <= record[2] && record[6] == 0u && record[7] == 0u, "kept <= counted, reserved words 0");
					bool sane = true;
					for (const float v : out)
						sane = sane && std::isfinite(v) && v >= 0.0f;
					expect(sane, "no output is NaN, infinite or negative");
					// either output alone, and in place
					expect(tonemap_ref_frame(W, H, rgb.data(), &p, record.data(), out.data(), nullptr) == RT_HIP_OK, "only the float output");
					expect(tonemap_ref_frame(W, H, rgb.data(), &p, record.data(), nullptr, rgba.data()) == RT_HIP_OK, "only the packed output");
					std::vector<float> in_place = rgb;
					std::vector<uint32_t> fresh(8u, 0u), again(8u, 0u);
					std::vector<float> apart(rgb.size());
					expect(tonemap_ref_frame(W, H, in_place.data(), &p, fresh.data(), in_place.data(), nullptr) == RT_HIP_OK, "in place");
					expect(tonemap_ref_frame(W, H, rgb.data(), &p, again.data(), apart.data(), nullptr) == RT_HIP_OK, "apart");
					expect(std::memcmp(in_place.data(), apart.data(), apart.size() * sizeof(float)) == 0 && fresh == again, "in place is what apart is");
				}
		std::printf("frame %ux%u%s: %u of %u pixels skipped\n", W, H, hostile ? " (hostile)" : "", histogram[256], pixels);
	}

	int parse(const std::string& text, rt_hip_tonemap_params* out, char* message, size_t size)
	{
		std::vector<char> exact(text.begin(), text.end()); // exactly the text and its terminator: a read past it is reported
		exact.push_back('\0');
		return tonemap_ref_from_spec(exact.data(), out, message, size);
	}
}

int main()
{
	// ragged sizes: one pixel, fewer than a run of 4, a tail behind whole runs, one workgroup plus a pixel
	const uint32_t shapes[][2] = { { 1, 1 }, { 1, 3 }, { 7, 1 }, { 5, 3 }, { 257, 1 }, { 70, 41 }, { 64, 36 } };
	for (const auto& s : shapes)
	{
		run_frame(s[0], s[1], false);
		run_frame(s[0], s[1], true);
	}

	// every bin, alone: a frame of one grey value in the middle of bin b puts every pixel there, and the meter reads it back
	for (uint32_t b = 0; b < 256u; b++)
	{
		const uint32_t bits = ((888u + b) << 20) + (1u << 19);
		float v;
		std::memcpy(&v, &bits, sizeof v);
		const std::vector<float> rgb(3u * 5u, v);
		std::vector<uint32_t> histogram(257u);
		tonemap_ref_histogram(5u, rgb.data(), histogram.data());
		expect(histogram[b] == 5u, "a grey frame lands in its bin");
		rt_hip_tonemap_params p;
		tonemap_ref_default_params(&p);
		p.low_permille = 999, p.high_permille = 0; // (floor(5 x 999 / 1000) = 4: one pixel kept)
		std::vector<uint32_t> record(8u, 0u);
		std::vector<uint32_t> rgba(5u);
		expect(tonemap_ref_frame(5, 1, rgb.data(), &p, record.data(), nullptr, rgba.data()) == RT_HIP_OK && record[4] == 1u && record[5] == b * 256u, "one kept pixel, the bin's own mean");
	}

	// every refusal of the parameters
	char message[256];
	rt_hip_tonemap_params p;
	tonemap_ref_default_params(&p);
	expect(tonemap_ref_check(&p, message, sizeof message) == RT_HIP_OK, "the defaults are accepted");
	const auto refused = [&](rt_hip_tonemap_params bad, const char* field)
	{
		float pixel[3] = { 1.0f, 1.0f, 1.0f };
		uint32_t record[8] = {}, packed = 0;
		expect(tonemap_ref_check(&bad, message, sizeof message) == RT_HIP_INVALID_ARGUMENT && std::strstr(message, field), field);
		expect(tonemap_ref_check(&bad, nullptr, 0) == RT_HIP_INVALID_ARGUMENT, "... without a message buffer");
		expect(tonemap_ref_check(&bad, message, 4) == RT_HIP_INVALID_ARGUMENT && std::strlen(message) == 3, "... into a short one");
		expect(tonemap_ref_frame(1, 1, pixel, &bad, record, nullptr, &packed) == RT_HIP_INVALID_ARGUMENT && packed == 0u, "... refused by the frame too, nothing written");
	};
	for (const uint32_t v : { 3u, 0xFFFFFFFFu })
	{
		rt_hip_tonemap_params bad = p;
		bad.curve = v;
		refused(bad, "curve");
	}
	for (const uint32_t v : { 1000u, 0xFFFFFFFFu })
	{
		rt_hip_tonemap_params bad = p;
		bad.low_permille = v;
		refused(bad, "low_permille");
		bad = p;
		bad.high_permille = v;
		refused(bad, "high_permille");
	}
	{
		rt_hip_tonemap_params bad = p;
		bad.low_permille = 500, bad.high_permille = 500;
		refused(bad, "high_permille");
	}
	for (const float v : { 0.0f, -1.0f, not_a_number, infinity, -infinity })
	{
		rt_hip_tonemap_params bad = p;
		if (v != 0.0f)
		{
			bad.exposure = v;
			refused(bad, "exposure");
		}
		bad = p, bad.key = v;
		refused(bad, "key");
		bad = p, bad.white = v;
		refused(bad, "white");
		bad = p, bad.min_exposure = v;
		refused(bad, "min_exposure");
		bad = p, bad.max_exposure = v;
		refused(bad, "max_exposure");
		bad = p, bad.adaptation = v;
		refused(bad, "adaptation");
	}
	{
		rt_hip_tonemap_params bad = p;
		bad.white = 0x1p-21f;
		refused(bad, "white");
		bad.white = 0x1p21f;
		refused(bad, "white");
		bad = p, bad.max_exposure = 0x1p-11f;
		refused(bad, "max_exposure");
		bad = p, bad.adaptation = 1.5f;
		refused(bad, "adaptation");
	}

	// the parser: well-formed, malformed, truncated and oversized texts
	const rt_hip_tonemap_params untouched = { 7u, 7u, 7u, 7.0f, 7.0f, 7.0f, 7.0f, 7.0f, 7.0f };
	for (const char* good : { "none", "reinhard", "aces", "aces:auto", "reinhard:2", "none:0.125", "aces:.5", "aces:1e-3", "aces:3E2" })
	{
		rt_hip_tonemap_params out = untouched;
		expect(parse(good, &out, message, sizeof message) == RT_HIP_OK && out.curve <= 2u && tonemap_ref_check(&out, nullptr, 0) == RT_HIP_OK, good);
	}
	std::vector<std::string> bad_texts = { "", ":", "a", "ace", "acess", "ACES", " aces", "aces ", "aces:", "aces:a", "aces:aut", "aces:autos", "aces:0", "aces:-1", "aces:+1", "aces: 1", "aces:1 ", "aces:1x", "aces:nan", "aces:inf",
										   "aces:1e99", "aces:1e", "aces:0x10", "aces:auto:1", "none:1:2", "reinhard,2", "aces:.", "aces:e5", std::string(300, 'a'), "aces:" + std::string(300, '9'), std::string(70, ':') };
	for (const char* whole : { "reinhard:auto", "aces:0.37" }) // ... and every proper prefix of two good ones that is not itself good
		for (size_t n = 0; n < std::strlen(whole); n++)
		{
			const std::string prefix(whole, n);
			if (prefix != "reinhard" && prefix != "aces" && prefix != "aces:0." && prefix != "aces:0.3")
				bad_texts.push_back(prefix);
		}
	for (const std::string& text : bad_texts)
	{
		rt_hip_tonemap_params out = untouched;
		expect(parse(text, &out, message, sizeof message) == RT_HIP_INVALID_ARGUMENT && std::strstr(message, "rt_hip_tonemap_from_spec") && std::memcmp(&out, &untouched, sizeof out) == 0, text.c_str());
		expect(parse(text, &out, nullptr, 0) == RT_HIP_INVALID_ARGUMENT, "... without a message buffer");
		expect(parse(text, &out, message, 4) == RT_HIP_INVALID_ARGUMENT && std::strlen(message) == 3, "... into a short one");
	}
	{
		rt_hip_tonemap_params out = untouched;
		expect(tonemap_ref_from_spec(nullptr, &out, message, sizeof message) == RT_HIP_INVALID_ARGUMENT && std::strstr(message, "NULL"), "a NULL text");
		expect(tonemap_ref_from_spec("aces", nullptr, message, sizeof message) == RT_HIP_INVALID_ARGUMENT && std::strstr(message, "NULL"), "a NULL output");
	}

	if (failures)
	{
		std::fprintf(stderr, "%d checks failed\n", failures);
		return 1;
	}
	std::printf("all checks passed\n");
	return 0;
}
