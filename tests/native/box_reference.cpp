// tests/native/box_reference.cpp — the CPU restatement of RT_HIP_FLAG_TRACE_BOXES: the frozen oracle with a
// test_boxes that hits.  TEST INFRASTRUCTURE, built with g++ alone into tests/native/libbox_reference.so (tests/box_reference.py binds it).
//
// Everything but the boxes IS the oracle: this file includes oracle/cpu_ref.cpp — frame constants, primary rays, random streams,
// scatter, the chunk-wise pixel sum, pack, the thread pool — and restates none of it.  It adds the box test's face (hits_box_face, the
// text of rt_amd/csrc/contract.hpp), test_boxes and the third select of mg_ray_tracer.cpp:162, and exports
//     box_ref_render        oracle_render's signature and mode bits
//     box_ref_closest_hit   oracle_closest_hit's signature; kind 3 = box
// With n_boxes == 0 both are the oracle's functions bit for bit (tests/test_box_reference.py).
//
// HOW the oracle's trace() comes to call the query below.  Inside the included file every `closest_hit(s, r)` is rewritten to
// `closest_hit(s, r, box_ref::with_boxes())`.  In a CALL the third argument is a value of the tag type, which selects the overload
// declared right below and defined at the end of this file.  In the oracle's own DEFINITION the same tokens declare an unnamed
// parameter of type "function returning the tag", i.e. a pointer to one: that overload is the oracle's query untouched, and the one
// below reaches it by passing a null pointer of that type.
#include "../../include/rt_hip.h"

namespace box_ref
{
	struct with_boxes
	{};
	using without_boxes = with_boxes (*)();
}

namespace
{
	struct ray;
	struct hit_result;
	hit_result closest_hit(const rt_hip_scene& s, const ray& r, box_ref::with_boxes);
}

#define closest_hit(scene, ray) closest_hit(scene, ray, box_ref::with_boxes())
// the two entry points this library is for; the oracle's other leaf functions come along under names of their own
#define oracle_render box_ref_render
#define oracle_closest_hit box_ref_closest_hit
#define oracle_random box_ref_oracle_random
#define oracle_stream_keys box_ref_oracle_stream_keys
#define oracle_sqrt_div box_ref_oracle_sqrt_div
#define oracle_inv_sqrt box_ref_oracle_inv_sqrt
#define oracle_inv_sqrt_step box_ref_oracle_inv_sqrt_step
#define oracle_pack box_ref_oracle_pack
#define oracle_sky box_ref_oracle_sky
#define oracle_primary_ray box_ref_oracle_primary_ray
#define oracle_frame_constants box_ref_oracle_frame_constants
#define oracle_dielectric_direction box_ref_oracle_dielectric_direction
#define oracle_hits_box box_ref_oracle_hits_box
#define oracle_render_census box_ref_oracle_render_census
#define oracle_unit_vector box_ref_oracle_unit_vector
#include "../../oracle/cpu_ref.cpp"
#undef closest_hit

namespace
{
	// hits_box (oracle/cpu_ref.cpp) with the face that was hit, as its OUTWARD normal — never flipped toward the ray, as sphere and
	// plane normals are not.  The reference defines no box normal; DESIGN.md §3.7 does, and rt_amd/csrc/contract.hpp has this text:
	//   entering (t is tmin): the first axis in x, y, z order whose select_min(t1, t2) equals tmin; -1 on it for a direction
	//                         component that points up the axis, +1 for one that points down it
	//   leaving (t is tmax, the origin inside): the first axis whose select_max(t1, t2) equals tmax; the component's own sign
	// The component's sign is read off its reciprocal, `inv < 0`: a zero component has the sign of its sign bit (1 / -0 = -inf),
	// a NaN counts as positive.  z is the axis when neither x nor y compares equal.
	inline bool hits_box_face(const ray& r, vec3 lo, vec3 hi, float& t, vec3& normal)
	{
		const vec3 inv = { 1.0f / r.dir.x, 1.0f / r.dir.y, 1.0f / r.dir.z };
		const vec3 t1 = { (lo.x - r.origin.x) * inv.x, (lo.y - r.origin.y) * inv.y, (lo.z - r.origin.z) * inv.z };
		const vec3 t2 = { (hi.x - r.origin.x) * inv.x, (hi.y - r.origin.y) * inv.y, (hi.z - r.origin.z) * inv.z };
		const vec3 near = { select_min(t1.x, t2.x), select_min(t1.y, t2.y), select_min(t1.z, t2.z) };
		const vec3 far = { select_max(t1.x, t2.x), select_max(t1.y, t2.y), select_max(t1.z, t2.z) };
		const float tmin = select_max(select_max(near.x, near.y), near.z);
		const float tmax = select_min(select_min(far.x, far.y), far.z);
		if (!(tmax >= tmin) || tmax < 0.0f)
			return false;
		const bool entering = tmin >= 0.0f;
		t = entering ? tmin : tmax;
		const bool on_x = (entering ? near.x : far.x) == t;
		const bool on_y = !on_x && (entering ? near.y : far.y) == t;
		const bool on_z = !on_x && !on_y;
		const float along = on_x ? inv.x : (on_y ? inv.y : inv.z);
		const float sign = ((along < 0.0f) != entering) ? -1.0f : 1.0f;
		normal = { on_x ? sign : 0.0f, on_y ? sign : 0.0f, on_z ? sign : 0.0f };
		return true;
	}

	// the test_boxes the reference leaves a stub (mg_ray_tracer.cpp:89-93), written like its test_spheres / test_planes (:36-87)
	inline hit_result test_boxes(const rt_hip_scene& s, const ray& r)
	{
		bool have = false;
		uint32_t hit_index = 0;
		float hit_dist = 0.0f;
		vec3 hit_normal = { 0, 0, 0 };
		for (uint32_t i = 0; i < s.n_boxes; i++)
		{
			const vec3 c = { s.box_center_x[i], s.box_center_y[i], s.box_center_z[i] };
			const vec3 e = { s.box_extents_x[i], s.box_extents_y[i], s.box_extents_z[i] };
			float t;
			vec3 normal;
			const bool hit = hits_box_face(r, c - e, c + e, t, normal);
			if (!hit || t < min_hit_dist || (have && hit_dist <= t))
				continue;
			have = true;
			hit_index = i;
			hit_dist = t;
			hit_normal = normal;
		}
		if (!have)
			return no_hit;
		return { hit_dist, hit_normal, s.box_material[hit_index], 3u, hit_index };
	}

	// hit = select(test_boxes, select(test_spheres, test_planes)), mg_ray_tracer.cpp:160-162: a box wins a distance tie
	hit_result closest_hit(const rt_hip_scene& s, const ray& r, box_ref::with_boxes)
	{
		const hit_result others = closest_hit(s, r, box_ref::without_boxes(nullptr)); // the oracle's query as it stands
		return select(test_boxes(s, r), others);
	}
}
