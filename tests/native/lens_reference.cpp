// tests/native/lens_reference.cpp — the CPU restatement of RT_HIP_FLAG_THIN_LENS: the frozen oracle with a sample loop
// that knows a lens.  TEST INFRASTRUCTURE, built with g++ alone into tests/native/liblens_reference.so (tests/lens_reference.py binds it).
//
// Everything but render_pixel's sample loop IS the oracle: this file includes oracle/cpu_ref.cpp — frame constants, primary rays, random
// streams, the closest-hit query, scatter, the trace loop, pack, the thread pool — and restates none of it; the lens' own arithmetic is
// rt_amd/csrc/lens_rules.hpp, the text the device runs, and the ten lens words come from rt_amd/csrc/lens.cpp as it is.  It adds
//     lens_ref_render   oracle_render's arguments plus the lens (NULL, or a radius of 0: the oracle's function bit for bit)
//     lens_ref_ray      one sample's ray, the numerators of its steps and how many steps it drew in front of the trace
//     lens_ref_disk     the concentric map of lens_rules.hpp
//     lens_ref_bend     disk point and lens ray of a given ray, eye and lens words (what rt_hip_kat_lens computes on the device)
//     lens_ref_words    the ten lens words of a frame, and its eye
//
// HOW the oracle's render_frame comes to call the loop below: the tag-overload trick of light_reference.cpp, on render_pixel.  Inside the
// included file every `render_pixel(f, x, y, rgba, rgb, c)` is rewritten to carry a seventh argument, lens_ref::with_lens().  In a CALL
// that is a value of the tag type, which selects the overload declared right below and defined at the end of this file.  In the oracle's
// own DEFINITION the same tokens declare an unnamed parameter of type "function returning the tag", i.e. a pointer to one: that overload
// is the oracle's loop untouched (nothing calls it here).
#include "../../include/rt_hip.h"

namespace lens_ref
{
	struct with_lens
	{};
}

namespace
{
	struct frame;
	struct counters;
	void render_pixel(const frame& f, uint32_t x, uint32_t y, uint32_t& out_rgba, float* out_rgb, counters& c, lens_ref::with_lens);
}

#define render_pixel(f, x, y, rgba, rgb, c) render_pixel(f, x, y, rgba, rgb, c, lens_ref::with_lens())
// the oracle's entry points come along under names of their own
#define oracle_render lens_ref_oracle_render
#define oracle_closest_hit lens_ref_oracle_closest_hit
#define oracle_random lens_ref_oracle_random
#define oracle_stream_keys lens_ref_oracle_stream_keys
#define oracle_sqrt_div lens_ref_oracle_sqrt_div
#define oracle_inv_sqrt lens_ref_oracle_inv_sqrt
#define oracle_inv_sqrt_step lens_ref_oracle_inv_sqrt_step
#define oracle_pack lens_ref_oracle_pack
#define oracle_sky lens_ref_oracle_sky
#define oracle_primary_ray lens_ref_oracle_primary_ray
#define oracle_frame_constants lens_ref_oracle_frame_constants
#define oracle_dielectric_direction lens_ref_oracle_dielectric_direction
#define oracle_hits_box lens_ref_oracle_hits_box
#define oracle_render_census lens_ref_oracle_render_census
#define oracle_unit_vector lens_ref_oracle_unit_vector
#include "../../oracle/cpu_ref.cpp"
#undef render_pixel

// the rules header takes its leaf function from the includer: plain '/', correctly rounded
namespace rt_hip
{
namespace lens
{
namespace leaf
{
	inline float divide(float a, float b) { return a / b; }
}
}
}
#include "../../rt_amd/csrc/lens_rules.hpp"
#include "../../rt_amd/csrc/lens.hpp"

#include <cstdarg>
#include <cstdio>
#include <mutex>

namespace rt_hip
{
	// (lens.cpp reports through context.hip's fail(); here the status is all a caller gets)
	rt_hip_status fail(rt_hip_status status, const char*, ...) { return status; }
}

namespace
{
	// the lens of the render in flight (set by lens_ref_render around its call of render_frame; read-only while the pool's threads run).
	// ONE render at a time: lens_ref_render holds render_in_flight from before it sets these until render_frame has returned, so two
	// callers in one process wait for each other instead of tracing each other's lens.
	std::mutex render_in_flight;
	bool lens_active = false;
	rt_hip::lens::words<vec3> lens_in_flight{};

	rt_hip::lens::words<vec3> words_of(const rt_hip::lens_words& w)
	{
		return { { w.u[0], w.u[1], w.u[2] }, { w.v[0], w.v[1], w.v[2] }, { w.fwd[0], w.fwd[1], w.fwd[2] }, w.focus };
	}

	// the frame's lens words, as render.hip derives them: make_frame_params, then make_lens_words.  false: no finite eye.
	bool frame_lens_words(const rt_hip_scene* scene, uint32_t width, uint32_t height, const rt_hip_lens& lens, rt_hip::lens_words& out, rt_hip::frame_params* out_frame = nullptr)
	{
		rt_hip::frame_request wanted{};
		wanted.width = width, wanted.height = height, wanted.partition = { 0, 1, RT_HIP_DEFAULT_STRIPE_ROWS };
		wanted.samples_per_pixel = scene->samples_per_pixel, wanted.max_bounces = scene->max_bounces;
		std::memcpy(wanted.inverse_view_projection, scene->inverse_view_projection, sizeof wanted.inverse_view_projection);
		const rt_hip::frame_params p = rt_hip::make_frame_params(wanted);
		if (out_frame)
			*out_frame = p;
		if (!p.pinhole && !p.eye_form)
			return false;
		out = rt_hip::make_lens_words(p, scene->inverse_view_projection, lens);
		return true;
	}

	inline vec3 eye_of(const frame& f) { return f.pinhole_rays ? vec3{ f.ray_eye[0], f.ray_eye[1], f.ray_eye[2] } : vec3{ f.eye_e[0], f.eye_e[1], f.eye_e[2] }; }

	// THE LENS STEP (§3.17): one more generator step of the sample's own stream, its two numerators mapped to the disk, and the pinhole's
	// ray r bent through that point of the lens — or left as it is where it does not meet the focus plane in front of the lens
	inline ray lens_ray(const frame& f, const ray& r, const rt_hip::lens::words<vec3>& w, random_stream& rng, random_stream::step* out_step = nullptr)
	{
		const random_stream::step k = rng.next_step(); // random<vec2>(): one step
		if (out_step)
			*out_step = k;
		const rt_hip::lens::disk_point on_disk = rt_hip::lens::disk(k.a, k.b);
		const rt_hip::lens::bent_ray<vec3> bent = rt_hip::lens::bend(r.dir, eye_of(f), w, on_disk);
		return bent.bent ? ray{ bent.origin, normalize(bent.toward) } : r;
	}

	// render_pixel (oracle/cpu_ref.cpp:819-869) with the lens step between the primary ray and the trace; everything else as there
	void render_pixel(const frame& f, uint32_t x, uint32_t y, uint32_t& out_rgba, float* out_rgb, counters& c, lens_ref::with_lens)
	{
		const rt_hip_scene& s = *f.scene;
		const uint32_t pixel_index = y * f.width + x;
		vec3 colour = { 0, 0, 0 };
		vec3 chunk = { 0, 0, 0 };
		for (uint32_t i = 0, e = s.samples_per_pixel; i < e; i++)
		{
			random_stream rng{ f.keys, pixel_index, i };
			float ka = 0x1.0p23f, kb = 0x1.0p23f; // sample 0 goes through the pixel centre and draws no jitter
			if (i)
			{
				const random_stream::step k = rng.next_step();
				ka = static_cast<float>(k.a);
				kb = static_cast<float>(k.b);
				if (k.a == 0u && k.b == 0u)
					note(ORACLE_CENSUS_ZERO_JITTER);
			}
			ray r = primary_ray(f, x, y, ka, kb);
			if (lens_active) // (sample 0 too: it draws the lens step from its window's start)
				r = lens_ray(f, r, lens_in_flight, rng);
			const vec3 sample = f.trace_order == ORACLE_TRACE_RECURSIVE ? trace_recursive(f, r, s.max_bounces, rng, c) : trace_iterative(f, r, s.max_bounces, rng, c);
			chunk = chunk + sample;
			if ((i + 1) % sample_chunk == 0 || i + 1 == e)
			{
				colour = (i < sample_chunk) ? chunk : colour + chunk;
				chunk = { 0, 0, 0 };
			}
		}
		const float n = static_cast<float>(s.samples_per_pixel);
		colour = { colour.x / n, colour.y / n, colour.z / n };
		if (probe.count)
			for (const float v : { colour.x, colour.y, colour.z })
				if (!std::isfinite(v))
					note(ORACLE_CENSUS_PACK_NON_FINITE);
		if (out_rgb)
		{
			out_rgb[0] = colour.x;
			out_rgb[1] = colour.y;
			out_rgb[2] = colour.z;
		}
		colour = { std::sqrt(colour.x), std::sqrt(colour.y), std::sqrt(colour.z) };
		if (probe.count)
			for (const float* v : { &colour.x, &colour.y, &colour.z })
			{
				if (*v > 1.0f)
					note(ORACLE_CENSUS_PACK_CLAMPED_ABOVE);
				else if (!(*v >= 0.0f))
					note(ORACLE_CENSUS_PACK_NEGATIVE_OR_NAN);
			}
		out_rgba = pack(colour);
	}
}

// oracle_render's arguments plus the lens.  1: a bad argument (the oracle's own, a lens rt_hip_set_lens refuses, or — with an aperture —
// a matrix without a finite eye)
extern "C" int lens_ref_render(const rt_hip_scene* scene,
							   uint32_t width,
							   uint32_t height,
							   uint64_t seed,
							   int mode,
							   const rt_hip_partition* part,
							   uint32_t* rgba8,
							   float* rgb_f32,
							   int n_threads,
							   oracle_stats* stats,
							   const rt_hip_lens* lens)
{
	if (!scene || !width || !height)
		return 1;
	const std::lock_guard<std::mutex> one_at_a_time(render_in_flight);
	lens_active = false;
	if (lens)
	{
		if (rt_hip::check_lens("lens_ref_render", *lens).status)
			return 1;
		if (lens->aperture_radius > 0.0f)
		{
			rt_hip::lens_words w{};
			if (!frame_lens_words(scene, width, height, *lens, w))
				return 1;
			lens_in_flight = words_of(w);
			lens_active = true;
		}
	}
	const int rc = render_frame(scene, width, height, seed, mode, part, rgba8, rgb_f32, n_threads, stats, nullptr);
	lens_active = false;
	return rc;
}

// sample `sample` of pixel (x, y): out_ray = origin, direction (6 floats); out_pinhole = the pinhole's ray it was bent from (6 floats);
// out_numerators = the jitter's (ka, kb) and the lens step's (2^23, 2^23 for sample 0's jitter); out_steps = generator steps drawn in
// front of the trace.  A lens of radius 0 (or NULL) draws no lens step.
extern "C" int lens_ref_ray(const rt_hip_scene* scene, uint32_t width, uint32_t height, uint64_t seed, const rt_hip_lens* lens, uint32_t x, uint32_t y, uint32_t sample, float* out_ray, float* out_pinhole, uint32_t* out_numerators,
							uint32_t* out_steps)
{
	if (!scene || !width || !height || x >= width || y >= height || !out_ray)
		return 1;
	const frame f = make_frame(scene, width, height, seed, ORACLE_TRACE_ITERATIVE);
	random_stream rng{ f.keys, y * width + x, sample };
	const uint32_t start = rng.counter;
	random_stream::step jitter = { 1u << 23, 1u << 23, 0u }, on_lens = { 0u, 0u, 0u };
	if (sample)
		jitter = rng.next_step();
	ray r = primary_ray(f, x, y, static_cast<float>(jitter.a), static_cast<float>(jitter.b));
	const ray pinhole = r;
	if (lens && lens->aperture_radius > 0.0f)
	{
		rt_hip::lens_words w{};
		if (rt_hip::check_lens("lens_ref_ray", *lens).status || !frame_lens_words(scene, width, height, *lens, w))
			return 1;
		r = lens_ray(f, r, words_of(w), rng, &on_lens);
	}
	const float ray_words[6] = { r.origin.x, r.origin.y, r.origin.z, r.dir.x, r.dir.y, r.dir.z };
	std::memcpy(out_ray, ray_words, sizeof ray_words);
	if (out_pinhole)
	{
		const float words[6] = { pinhole.origin.x, pinhole.origin.y, pinhole.origin.z, pinhole.dir.x, pinhole.dir.y, pinhole.dir.z };
		std::memcpy(out_pinhole, words, sizeof words);
	}
	if (out_numerators)
		out_numerators[0] = jitter.a, out_numerators[1] = jitter.b, out_numerators[2] = on_lens.a, out_numerators[3] = on_lens.b;
	if (out_steps)
	{
		// the stride is odd: counter = start + steps * stride (mod 2^32) has one solution below 4096, found by walking
		uint32_t steps = 0;
		for (uint32_t at = start; at != rng.counter; at += rng.stride)
			steps++;
		*out_steps = steps;
	}
	return 0;
}

// out[2 i ..] = the disk point of the numerators (ka[i], kb[i])
extern "C" void lens_ref_disk(uint32_t n, const uint32_t* ka, const uint32_t* kb, float* out)
{
	for (uint32_t i = 0; i < n; i++)
	{
		const rt_hip::lens::disk_point p = rt_hip::lens::disk(ka[i], kb[i]);
		out[2u * i] = p.x, out[2u * i + 1u] = p.y;
	}
}

// rt_hip_kat_lens on the CPU: ray_words[9] = origin, normalised direction, eye; lens_words[10] = U, V, fwd, focus ->
// out[9 i ..] = (lx, ly, origin.xyz, direction.xyz, bent as 0 / 1)
extern "C" void lens_ref_bend(uint32_t n, const uint32_t* ka, const uint32_t* kb, const float* in, const float* lw, float* out)
{
	const vec3 o = { in[0], in[1], in[2] }, d = { in[3], in[4], in[5] }, eye = { in[6], in[7], in[8] };
	const rt_hip::lens::words<vec3> w = { { lw[0], lw[1], lw[2] }, { lw[3], lw[4], lw[5] }, { lw[6], lw[7], lw[8] }, lw[9] };
	for (uint32_t i = 0; i < n; i++)
	{
		const rt_hip::lens::disk_point on_disk = rt_hip::lens::disk(ka[i], kb[i]);
		const rt_hip::lens::bent_ray<vec3> bent = rt_hip::lens::bend(d, eye, w, on_disk);
		const vec3 origin = bent.bent ? bent.origin : o;
		const vec3 dir = bent.bent ? normalize(bent.toward) : d;
		float* const r = out + 9u * i;
		r[0] = on_disk.x, r[1] = on_disk.y, r[2] = origin.x, r[3] = origin.y, r[4] = origin.z, r[5] = dir.x, r[6] = dir.y, r[7] = dir.z, r[8] = bent.bent ? 1.0f : 0.0f;
	}
}

// the ten lens words of a frame (U, V, fwd, focus) and its eye (3 floats), as render.hip derives them; out_form: 1 pinhole, 2 plain eye, 3
// guarded eye.  Returns the status of the frame's check (rt_hip_status): RT_HIP_UNSUPPORTED for a matrix without a finite eye.
extern "C" int lens_ref_words(const rt_hip_scene* scene, uint32_t width, uint32_t height, const rt_hip_lens* lens, float* out_words, float* out_eye, uint32_t* out_form)
{
	if (!scene || !lens || !width || !height || !out_words)
		return RT_HIP_INVALID_ARGUMENT;
	if (const rt_hip_status st = rt_hip::check_lens("lens_ref_words", *lens).status)
		return st;
	rt_hip::lens_words w{};
	rt_hip::frame_params p{};
	const bool has_eye = frame_lens_words(scene, width, height, *lens, w, &p);
	if (const rt_hip_status st = rt_hip::check_lens_frame("lens_ref_words", true, p).status)
		return st;
	if (!has_eye)
		return RT_HIP_UNSUPPORTED;
	rt_hip::frame_params carrier = p;
	rt_hip::put_lens_words(carrier, w); // (through the words they travel in, so that the packing is under test too)
	const float words[10] = { carrier.mx[0], carrier.mx[1], carrier.mx[2], carrier.my[0], carrier.my[1], carrier.my[2], carrier.k_near[0], carrier.k_near[1], carrier.k_near[2], carrier.mx[3] };
	std::memcpy(out_words, words, sizeof words);
	if (out_eye)
		for (int c = 0; c < 3; c++)
			out_eye[c] = p.pinhole ? p.ray_eye[c] : p.eye_e[c];
	if (out_form)
		*out_form = p.pinhole ? 1u : (p.eye_form == 2u ? 2u : 3u);
	return RT_HIP_OK;
}

// the host-only checks, for tests/test_lens_host.py: the message of a refusal (empty: accepted) and its status
extern "C" int lens_ref_check_lens(float aperture_radius, float focus_distance, char* out_message, size_t message_bytes)
{
	const rt_hip::lens_check c = rt_hip::check_lens("rt_hip_set_lens", rt_hip_lens{ aperture_radius, focus_distance });
	if (out_message && message_bytes)
		std::snprintf(out_message, message_bytes, "%s", c.status ? c.message : "");
	return c.status;
}
extern "C" int lens_ref_from_spec(const char* spec, rt_hip_lens* out_lens, char* out_message, size_t message_bytes)
{
	const rt_hip::lens_check c = rt_hip::lens_from_spec(spec, out_lens);
	if (out_message && message_bytes)
		std::snprintf(out_message, message_bytes, "%s", c.status ? c.message : "");
	return c.status;
}
extern "C" int lens_ref_check_frame(const rt_hip_scene* scene, uint32_t width, uint32_t height, int have_lens, char* out_message, size_t message_bytes)
{
	rt_hip::lens_words w{};
	rt_hip::frame_params p{};
	frame_lens_words(scene, width, height, rt_hip_lens{ 0.0f, 1.0f }, w, &p);
	const rt_hip::lens_check c = rt_hip::check_lens_frame("rt_hip_render_device", have_lens != 0, p);
	if (out_message && message_bytes)
		std::snprintf(out_message, message_bytes, "%s", c.status ? c.message : "");
	return c.status;
}
