// tests/native/direct_reference.cpp — the CPU restatement of RT_HIP_FLAG_DIRECT_LIGHT: the frozen oracle with a trace
// loop that knows lights AND samples the sphere lights directly.  TEST INFRASTRUCTURE, built with g++ alone into
// tests/native/libdirect_reference.so (tests/direct_reference.py binds it).
//
// Everything but the trace loop IS the oracle (this file includes oracle/cpu_ref.cpp through the tag-overload trick light_reference.cpp
// explains), and the vertex rule IS rt_amd/csrc/direct_light_rules.hpp, the text the device runs.  It adds
//     direct_ref_render   light_ref_render's arguments plus `direct` (0: the RT_HIP_FLAG_EMISSION frame; else the flag's frame)
//     direct_ref_render_census   direct_ref_render with the oracle's branch census (note() fires inside the included oracle code under this
//                         loop too) and the restatement's OWN events, counted here only — oracle/cpu_ref.* know nothing of them
//     direct_ref_vertex   test only: the vertex rule N times at one point, visibility query included -> mean and mean square of the weight
//     direct_ref_octahedral, direct_ref_aim   the rules header's two known answers as g++ compiles them (tests/test_gpu_direct_light.py)
// With no sampled light the frame is light_ref_render's bit for bit (tests/test_direct_reference.py).
//
// NOT a lower-variance way to the RT_HIP_FLAG_EMISSION image: see the header of direct_light_rules.hpp.
#include "../../include/rt_hip.h"
#include "../../rt_amd/csrc/direct_light_rules.hpp"

namespace direct_ref
{
	struct with_direct
	{};
	using without_direct = with_direct (*)();
}

namespace
{
	struct vec3;
	struct ray;
	struct frame;
	struct random_stream;
	struct counters;
	vec3 trace_iterative(const frame& f, ray r, uint32_t max_bounces, random_stream& rng, counters& c, direct_ref::with_direct);
}

#define trace_iterative(f, r, bounces, rng, c) trace_iterative(f, r, bounces, rng, c, direct_ref::with_direct())
// the oracle's entry points come along under names of their own
#define oracle_render direct_ref_oracle_render
#define oracle_closest_hit direct_ref_oracle_closest_hit
#define oracle_random direct_ref_oracle_random
#define oracle_stream_keys direct_ref_oracle_stream_keys
#define oracle_sqrt_div direct_ref_oracle_sqrt_div
#define oracle_inv_sqrt direct_ref_oracle_inv_sqrt
#define oracle_inv_sqrt_step direct_ref_oracle_inv_sqrt_step
#define oracle_pack direct_ref_oracle_pack
#define oracle_sky direct_ref_oracle_sky
#define oracle_primary_ray direct_ref_oracle_primary_ray
#define oracle_frame_constants direct_ref_oracle_frame_constants
#define oracle_dielectric_direction direct_ref_oracle_dielectric_direction
#define oracle_hits_box direct_ref_oracle_hits_box
#define oracle_render_census direct_ref_oracle_render_census
#define oracle_unit_vector direct_ref_oracle_unit_vector
#include "../../oracle/cpu_ref.cpp"
#undef trace_iterative

namespace
{
	// the table and the sampled lights of the render in flight (set around render_frame; read-only while the pool's threads run)
	const float* emission_table = nullptr;
	uint32_t emission_rows = 0;
	struct sampled_light
	{
		vec3 centre;
		float radius;
		vec3 emission;
		uint32_t sphere;
	};
	std::vector<sampled_light> sampled;	  // at most direct_light::max_sampled_lights, in sphere-index order
	std::vector<unsigned char> is_sampled; // per sphere

	inline bool is_light(uint32_t material)
	{
		if (material >= emission_rows)
			return false;
		const float* const e = emission_table + static_cast<size_t>(material) * 3u;
		return e[0] > 0.0f || e[1] > 0.0f || e[2] > 0.0f;
	}

	// A sphere is a SAMPLED LIGHT iff its material is a light and its radius is finite and > 0; the first 256 such spheres are sampled.
	void list_sampled_lights(const rt_hip_scene& s, bool direct)
	{
		sampled.clear();
		is_sampled.assign(s.n_spheres, 0);
		for (uint32_t i = 0; direct && i < s.n_spheres && sampled.size() < rt_hip::direct_light::max_sampled_lights; i++)
		{
			const uint32_t m = s.sphere_material[i];
			const float radius = s.sphere_radius[i];
			if (!is_light(m) || !std::isfinite(radius) || !(radius > 0.0f))
				continue;
			const float* const e = emission_table + static_cast<size_t>(m) * 3u;
			sampled.push_back({ { s.sphere_center_x[i], s.sphere_center_y[i], s.sphere_center_z[i] }, radius, { e[0], e[1], e[2] }, i });
			is_sampled[i] = 1;
		}
	}

	// ---- the restatement's own census (direct_ref_render_census; tests/direct_reference.py OWN_EVENTS has the names, in this order) ----
	// Counted into atomics shared by the pool's threads, and only while a census render is in flight: with `own_on` false nothing below
	// is touched.  The counting reads what the loop computes anyway (or recomputes it from the step's numerators) and changes none of it.
	enum own_event
	{
		OWN_VERTEX_AIMED,	  // a lambert vertex's rule aimed: a shadow query ran
		OWN_VERTEX_NOT_AIMED, // ... aimed at nothing: no shadow segment
		OWN_SHADOW_VISIBLE,
		OWN_SHADOW_OCCLUDED,
		OWN_ZERO_WORD_K,	 // k.a == k.b == k.c == 0: light 0, the octahedral corner u = v = -1, the fold with sgn
		OWN_FOLD_BELOW,		 // z < 0
		OWN_INSIDE_LIGHT,	 // the vertex lies inside the light it chose
		OWN_SAMPLED_LIGHT_AFTER_SAMPLING_VERTEX, // `return direct + 0`
		OWN_SAMPLED_LIGHT_AFTER_OTHER_VERTEX,	 // a sampled light met behind a metal / dielectric vertex: throughput * E
		OWN_LIGHT_ON_PRIMARY,					 // a primary ray met a light
		OWN_CHOSE_LAST_OF_256,					 // choose_light gave 255 of 256
		OWN_FIRST_VERTEX_AIMED,					 // the sample's FIRST vertex is lambert and aimed (what a watched sample is asked)
		OWN_FIRST_VERTEX_NOT_AIMED,
		OWN_SAMPLED_LIGHT_AFTER_OTHER_VERTEX_LATER, // ... behind a metal / dielectric vertex that FOLLOWS one that sampled: `sampled_before` had to be cleared
		OWN_EVENTS
	};
	std::atomic<uint64_t> own_counts[OWN_EVENTS], watch_counts[OWN_EVENTS];
	bool own_on = false;
	// the one (pixel, sample) whose events are ALSO counted into watch_counts: its stream is known by its key and by where its counter
	// stands when the trace loop is entered (after the jitter's step, which sample 0 does not draw)
	struct
	{
		bool on = false;
		uint32_t key = 0, counter = 0;
	} watch;

	inline void own(int event, bool watched)
	{
		if (!own_on)
			return;
		own_counts[event].fetch_add(1, std::memory_order_relaxed);
		if (watched)
			watch_counts[event].fetch_add(1, std::memory_order_relaxed);
	}

	[[maybe_unused]] vec3 (*const oracle_trace_iterative)(const frame&, ray, uint32_t, random_stream&, counters&, direct_ref::without_direct) = trace_iterative;

	struct contract_inv_sqrt
	{
		float operator()(float x) const { return inv_sqrt(x); }
	};

	// the vertex rule (§3.13) at x with the hit's stored normal: one generator step, the rules header, the unchanged closest-hit query.
	// Returns whether the light is visible, with the weight and the light's emission E; counts the shadow segment.
	inline bool vertex_rule(const rt_hip_scene& scene, vec3 x, vec3 nrm, random_stream& rng, counters& c, vec3& E, float& weight, bool watched = false, bool first = false)
	{
		const random_stream::step k = rng.next_step();
		const uint32_t n = static_cast<uint32_t>(sampled.size());
		const uint32_t chosen = rt_hip::direct_light::choose_light(k.c, n);
		const sampled_light& light = sampled[chosen];
		E = light.emission;
		const rt_hip::direct_light::aim<vec3> a = rt_hip::direct_light::aim_at(k.a, k.b, x, nrm, light.centre, light.radius, n, contract_inv_sqrt());
		weight = a.weight;
		if (own_on) // the census: the rule's inner branches, from the numerators and the header's own functions once more
		{
			float l2;
			const vec3 d0 = x - light.centre;
			if (k.a == 0u && k.b == 0u && k.c == 0u)
				own(OWN_ZERO_WORD_K, watched);
			if (rt_hip::direct_light::octahedral_point<vec3>(k.a, k.b, l2).z < 0.0f)
				own(OWN_FOLD_BELOW, watched);
			if (rt_hip::direct_light::dot3(d0, d0) < light.radius * light.radius)
				own(OWN_INSIDE_LIGHT, watched);
			if (n == rt_hip::direct_light::max_sampled_lights && chosen == n - 1u)
				own(OWN_CHOSE_LAST_OF_256, watched);
			own(a.aimed ? OWN_VERTEX_AIMED : OWN_VERTEX_NOT_AIMED, watched);
			if (first)
				own(a.aimed ? OWN_FIRST_VERTEX_AIMED : OWN_FIRST_VERTEX_NOT_AIMED, watched);
		}
		if (!a.aimed)
			return false;
		c.segments++;
		const hit_result shadow = closest_hit(scene, ray{ x, a.w });
		const bool visible = shadow && shadow.kind == 1u && shadow.index == light.sphere; // (no distance is compared)
		own(visible ? OWN_SHADOW_VISIBLE : OWN_SHADOW_OCCLUDED, watched);
		return visible;
	}

	// trace_iterative of light_reference.cpp with §3.13's `direct` and `sampled_before`
	vec3 trace_iterative(const frame& f, ray r, uint32_t max_bounces, random_stream& rng, counters& c, direct_ref::with_direct)
	{
		vec3 throughput = { 1.0f, 1.0f, 1.0f };
		vec3 direct = { 0.0f, 0.0f, 0.0f };
		bool sampled_before = false;
		const bool watched = own_on && watch.on && rng.function_key == watch.key && rng.counter == watch.counter;
		bool first = true;		   // no vertex yet
		bool ever_sampled = false; // (the census: a vertex of this path has run the rule)
		while (true)
		{
			if (!(max_bounces--))
			{
				note(ORACLE_CENSUS_OUT_OF_BOUNCES);
				return direct + vec3{ 0, 0, 0 };
			}
			c.segments++;
			const hit_result hit = closest_hit(*f.scene, r);
			if (!hit)
				return direct + throughput * sky(r.dir.y);
			if (is_light(hit.material))
			{
				if (first)
					own(OWN_LIGHT_ON_PRIMARY, watched);
				else if (hit.kind == 1u && is_sampled[hit.index])
				{
					own(sampled_before ? OWN_SAMPLED_LIGHT_AFTER_SAMPLING_VERTEX : OWN_SAMPLED_LIGHT_AFTER_OTHER_VERTEX, watched);
					if (!sampled_before && ever_sampled)
						own(OWN_SAMPLED_LIGHT_AFTER_OTHER_VERTEX_LATER, watched);
				}
				if (hit.kind == 1u && is_sampled[hit.index] && sampled_before)
					return direct + vec3{ 0, 0, 0 }; // the previous vertex has accounted for this light
				const float* const e = emission_table + static_cast<size_t>(hit.material) * 3u;
				return direct + throughput * vec3{ e[0], e[1], e[2] };
			}
			const material& m = f.materials[hit.material];
			const bool lambert = m.type != RT_HIP_MATERIAL_METAL && !(f.sm_materials && refracts_in_sm(m.type));
			if (lambert && !sampled.empty())
			{
				vec3 E;
				float weight;
				if (vertex_rule(*f.scene, r.at(hit.distance), hit.normal, rng, c, E, weight, watched, first))
					direct = direct + ((throughput * m.attenuation) * E) * weight;
				sampled_before = true;
				ever_sampled = true;
			}
			else
				sampled_before = false;
			first = false;
			vec3 attenuation;
			ray scattered;
			if (!scatter(f, r, hit, rng, scattered, attenuation))
				return direct + vec3{ 0, 0, 0 };
			throughput = throughput * attenuation;
			r = scattered;
		}
	}

	int check_table(const rt_hip_scene* scene, const float* emission_rgb, uint32_t n_emission)
	{
		if (emission_rgb && n_emission != scene->n_materials)
			return 1;
		for (uint32_t i = 0; emission_rgb && i < n_emission * 3u; i++)
			if (!std::isfinite(emission_rgb[i]) || !(emission_rgb[i] >= 0.0f))
				return 1;
		return 0;
	}
}

namespace
{
	int render_with(const rt_hip_scene* scene, uint32_t width, uint32_t height, uint64_t seed, int mode, const rt_hip_partition* part, uint32_t* rgba8, float* rgb_f32, int n_threads, oracle_stats* stats, const float* emission_rgb,
					uint32_t n_emission, int direct, uint64_t* census)
	{
		if (!scene || (mode & ORACLE_TRACE_RECURSIVE) || check_table(scene, emission_rgb, n_emission))
			return 1;
		emission_table = emission_rgb;
		emission_rows = emission_rgb ? n_emission : 0u;
		list_sampled_lights(*scene, direct != 0);
		const int rc = render_frame(scene, width, height, seed, mode, part, rgba8, rgb_f32, n_threads, stats, census);
		emission_table = nullptr;
		emission_rows = 0;
		sampled.clear();
		is_sampled.clear();
		return rc;
	}
}

// light_ref_render's arguments plus `direct`.  1: a bad argument (as light_ref_render)
extern "C" int direct_ref_render(const rt_hip_scene* scene,
								 uint32_t width,
								 uint32_t height,
								 uint64_t seed,
								 int mode,
								 const rt_hip_partition* part,
								 uint32_t* rgba8,
								 float* rgb_f32,
								 int n_threads,
								 oracle_stats* stats,
								 const float* emission_rgb,
								 uint32_t n_emission,
								 int direct)
{
	return render_with(scene, width, height, seed, mode, part, rgba8, rgb_f32, n_threads, stats, emission_rgb, n_emission, direct, nullptr);
}

// direct_ref_render with the censuses.  census: ORACLE_CENSUS_EVENTS words, the oracle's events (cpu_ref.h) under this trace loop;
// own_census: direct_ref_own_events() words, the events counted in this file.  watch_pixel >= 0: watch_census (as many words) gets the
// own events of the ONE sample (watch_pixel, watch_sample), so that a test can ask what a constructed vertex did.  With `census` null the
// call IS direct_ref_render (nothing is counted; the own arrays, if given, are zeroed).  ORACLE_TEST_NO_RARE_RULES in `mode` is honoured as
// oracle_render_census honours it — render_frame reads it where a census is open — so sensitivity can be shown under the direct loop too.
extern "C" int direct_ref_render_census(const rt_hip_scene* scene,
										uint32_t width,
										uint32_t height,
										uint64_t seed,
										int mode,
										const rt_hip_partition* part,
										uint32_t* rgba8,
										float* rgb_f32,
										int n_threads,
										oracle_stats* stats,
										const float* emission_rgb,
										uint32_t n_emission,
										int direct,
										uint64_t* census,
										uint64_t* own_census,
										int64_t watch_pixel,
										uint32_t watch_sample,
										uint64_t* watch_census)
{
	for (int e = 0; e < OWN_EVENTS; e++)
	{
		own_counts[e] = 0, watch_counts[e] = 0;
		if (own_census)
			own_census[e] = 0;
		if (watch_census)
			watch_census[e] = 0;
	}
	own_on = census != nullptr;
	watch.on = own_on && watch_pixel >= 0 && watch_census;
	if (watch.on)
	{
		const random_stream at_entry(make_frame_keys(seed), static_cast<uint32_t>(watch_pixel), watch_sample);
		watch.key = at_entry.function_key;
		watch.counter = at_entry.counter + (watch_sample ? at_entry.stride : 0u); // (sample 0 draws no jitter)
	}
	const int rc = render_with(scene, width, height, seed, mode, part, rgba8, rgb_f32, n_threads, stats, emission_rgb, n_emission, direct, census);
	for (int e = 0; own_on && e < OWN_EVENTS; e++)
	{
		if (own_census)
			own_census[e] = own_counts[e].load();
		if (watch_census)
			watch_census[e] = watch_counts[e].load();
	}
	own_on = false;
	watch.on = false;
	return rc;
}

extern "C" int direct_ref_own_events() { return OWN_EVENTS; }

// how many sampled lights the scene has under the table (what the device's list must hold)
extern "C" int direct_ref_count(const rt_hip_scene* scene, const float* emission_rgb, uint32_t n_emission)
{
	if (!scene || check_table(scene, emission_rgb, n_emission))
		return -1;
	emission_table = emission_rgb;
	emission_rows = emission_rgb ? n_emission : 0u;
	list_sampled_lights(*scene, true);
	const int n = static_cast<int>(sampled.size());
	emission_table = nullptr;
	emission_rows = 0;
	sampled.clear();
	is_sampled.clear();
	return n;
}

// TEST ONLY: the vertex rule `draws` times at `point` with `normal`, from the stream of (seed, pixel, sample 0) stepped on and on.
// out[0] = mean of the weight (0 where not aimed or not visible), out[1] = mean of its square, out[2] = shadow segments counted.
extern "C" int direct_ref_vertex(const rt_hip_scene* scene, const float* emission_rgb, uint32_t n_emission, const float* point, const float* normal, uint64_t seed, uint32_t pixel, uint64_t draws, double* out)
{
	if (!scene || !point || !normal || !out || check_table(scene, emission_rgb, n_emission))
		return 1;
	emission_table = emission_rgb;
	emission_rows = emission_rgb ? n_emission : 0u;
	list_sampled_lights(*scene, true);
	int rc = 1;
	if (!sampled.empty())
	{
		random_stream rng(make_frame_keys(seed), pixel, 0u);
		counters c;
		double sum = 0.0, squares = 0.0;
		for (uint64_t i = 0; i < draws; i++)
		{
			vec3 E;
			float weight;
			const double w = vertex_rule(*scene, { point[0], point[1], point[2] }, { normal[0], normal[1], normal[2] }, rng, c, E, weight) ? static_cast<double>(weight) : 0.0;
			sum += w;
			squares += w * w;
		}
		out[0] = draws ? sum / static_cast<double>(draws) : 0.0;
		out[1] = draws ? squares / static_cast<double>(draws) : 0.0;
		out[2] = static_cast<double>(c.segments);
		rc = 0;
	}
	emission_table = nullptr;
	emission_rows = 0;
	sampled.clear();
	is_sampled.clear();
	return rc;
}

// the rules header as g++ compiles it: the octahedral point (x, y, z, l2) ...
extern "C" void direct_ref_octahedral(uint32_t ka, uint32_t kb, float* out4)
{
	float l2;
	const vec3 p = rt_hip::direct_light::octahedral_point<vec3>(ka, kb, l2);
	out4[0] = p.x, out4[1] = p.y, out4[2] = p.z, out4[3] = l2;
}

// ... and the aim: in = x, nrm, C (3 floats each); out = w.xyz, weight, aimed (as 0 / 1)
extern "C" void direct_ref_aim(uint32_t ka, uint32_t kb, const float* in9, float R, uint32_t n, float* out5)
{
	const rt_hip::direct_light::aim<vec3> a =
		rt_hip::direct_light::aim_at(ka, kb, vec3{ in9[0], in9[1], in9[2] }, vec3{ in9[3], in9[4], in9[5] }, vec3{ in9[6], in9[7], in9[8] }, R, n, contract_inv_sqrt());
	out5[0] = a.w.x, out5[1] = a.w.y, out5[2] = a.w.z, out5[3] = a.weight, out5[4] = a.aimed ? 1.0f : 0.0f;
}
