// tests/native/light_reference.cpp — the CPU restatement of RT_HIP_FLAG_EMISSION: the frozen oracle with a trace loop
// that knows lights.  TEST INFRASTRUCTURE, built with g++ alone into tests/native/liblight_reference.so (tests/light_reference.py binds it).
//
// Everything but the trace loop IS the oracle: this file includes oracle/cpu_ref.cpp — frame constants, primary rays, random streams,
// the closest-hit query, scatter, the chunk-wise pixel sum, pack, the thread pool — and restates none of it.  It adds
//     light_ref_render   oracle_render's arguments plus the emission table (3 floats per material) and its row count
// With no light in the table (or no table) it is the oracle's function bit for bit (tests/test_light_reference.py).
//
// HOW the oracle's render_pixel comes to call the loop below: the tag-overload trick of box_reference.cpp.  Inside the included file every
// `trace_iterative(f, r, b, rng, c)` is rewritten to `trace_iterative(f, r, b, rng, c, light_ref::with_lights())`.  In a CALL the sixth
// argument is a value of the tag type, which selects the overload declared right below and defined at the end of this file.  In the
// oracle's own DEFINITION the same tokens declare an unnamed parameter of type "function returning the tag", i.e. a pointer to one:
// that overload is the oracle's loop untouched (nothing calls it here: the loop below runs for every table, and with no light in it computes
// what the oracle's does, which tests/test_light_reference.py holds bit for bit).
#include "../../include/rt_hip.h"

namespace light_ref
{
	struct with_lights
	{};
	using without_lights = with_lights (*)();
}

namespace
{
	struct vec3;
	struct ray;
	struct frame;
	struct random_stream;
	struct counters;
	vec3 trace_iterative(const frame& f, ray r, uint32_t max_bounces, random_stream& rng, counters& c, light_ref::with_lights);
}

#define trace_iterative(f, r, bounces, rng, c) trace_iterative(f, r, bounces, rng, c, light_ref::with_lights())
// the oracle's entry points come along under names of their own
#define oracle_render light_ref_oracle_render
#define oracle_closest_hit light_ref_oracle_closest_hit
#define oracle_random light_ref_oracle_random
#define oracle_stream_keys light_ref_oracle_stream_keys
#define oracle_sqrt_div light_ref_oracle_sqrt_div
#define oracle_inv_sqrt light_ref_oracle_inv_sqrt
#define oracle_inv_sqrt_step light_ref_oracle_inv_sqrt_step
#define oracle_pack light_ref_oracle_pack
#define oracle_sky light_ref_oracle_sky
#define oracle_primary_ray light_ref_oracle_primary_ray
#define oracle_frame_constants light_ref_oracle_frame_constants
#define oracle_dielectric_direction light_ref_oracle_dielectric_direction
#define oracle_hits_box light_ref_oracle_hits_box
#define oracle_render_census light_ref_oracle_render_census
#define oracle_unit_vector light_ref_oracle_unit_vector
#include "../../oracle/cpu_ref.cpp"
#undef trace_iterative

namespace
{
	// the table of the render in flight (set by light_ref_render around its call of render_frame; read-only while the pool's threads run)
	const float* emission_table = nullptr;
	uint32_t emission_rows = 0;

	// A material IS A LIGHT iff r > 0 || g > 0 || b > 0.
	inline bool is_light(uint32_t material)
	{
		if (material >= emission_rows)
			return false;
		const float* const e = emission_table + static_cast<size_t>(material) * 3u;
		return e[0] > 0.0f || e[1] > 0.0f || e[2] > 0.0f;
	}

	// (the oracle's own loop stays addressable, so that the compiler does not report it unused)
	[[maybe_unused]] vec3 (*const oracle_trace_iterative)(const frame&, ray, uint32_t, random_stream&, counters&, light_ref::without_lights) = trace_iterative;

	// trace_iterative (oracle/cpu_ref.cpp:783-804) with the light rule of DESIGN.md §3.12:
	//   the bounce check comes first and c.segments++ happens as ever — a path with no bounce left returns 0 before it can reach a light;
	//   the closest-hit query is unchanged;
	//   if the accepted hit's material is a light the sample is throughput * emission (component-wise, throughput on the left, exactly
	//   as throughput * sky(...)) and the path ends: no random draw, no scatter — whatever the material's type, albedo, roughness and
	//   reflectivity, under either scatter table, from either side.
	vec3 trace_iterative(const frame& f, ray r, uint32_t max_bounces, random_stream& rng, counters& c, light_ref::with_lights)
	{
		vec3 throughput = { 1.0f, 1.0f, 1.0f };
		while (true)
		{
			if (!(max_bounces--))
			{
				note(ORACLE_CENSUS_OUT_OF_BOUNCES);
				return { 0, 0, 0 };
			}
			c.segments++;
			const hit_result hit = closest_hit(*f.scene, r);
			if (!hit)
				return throughput * sky(r.dir.y);
			if (is_light(hit.material))
			{
				const float* const e = emission_table + static_cast<size_t>(hit.material) * 3u;
				return throughput * vec3{ e[0], e[1], e[2] };
			}
			vec3 attenuation;
			ray scattered;
			if (!scatter(f, r, hit, rng, scattered, attenuation))
				return { 0, 0, 0 };
			throughput = throughput * attenuation;
			r = scattered;
		}
	}
}

// oracle_render's arguments plus the table.  1: a bad argument (the oracle's own, a table whose row count is not the scene's n_materials, a
// component that is not a finite number >= 0, or the recursive trace order — the rule is written against the contract's iterative loop)
extern "C" int light_ref_render(const rt_hip_scene* scene,
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
								uint32_t n_emission)
{
	if (!scene || (mode & ORACLE_TRACE_RECURSIVE))
		return 1;
	if (emission_rgb && n_emission != scene->n_materials)
		return 1;
	for (uint32_t i = 0; emission_rgb && i < n_emission * 3u; i++)
		if (!std::isfinite(emission_rgb[i]) || !(emission_rgb[i] >= 0.0f))
			return 1;
	emission_table = emission_rgb;
	emission_rows = emission_rgb ? n_emission : 0u;
	const int rc = render_frame(scene, width, height, seed, mode, part, rgba8, rgb_f32, n_threads, stats, nullptr);
	emission_table = nullptr;
	emission_rows = 0;
	return rc;
}
