// rt_amd/csrc/scene.hip — the caller's scene columns: pointer and index checks, the fingerprint that decides whether the
// columns resident in HBM are still the caller's (rt has no scene version counter, src/main.cpp:233-311), the image of the
// single HBM block with its derived per-primitive tables, and residency per context.
//
// The columns are exactly the soagen columns the reference fills at load (src/scene.cpp:583,595; src/soa.toml:6-45) and
// whose split float columns none of its renderers reads.
#include "internal.hpp"
#include "bvh.hpp"
#include "box_bvh.hpp"
#include "box_bvh_scan.hpp"
#include "bvh_build.hpp"
#include "bvh_build_device.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <exception>

using namespace rt_hip;

namespace
{
	// the part of the scene check that is cheap enough for every call: counts against NULL pointers
	rt_hip_status check_scene_pointers(const rt_hip_scene& s)
	{
		if (!s.samples_per_pixel || !s.max_bounces)
			return fail(RT_HIP_INVALID_ARGUMENT, "scene: samples_per_pixel and max_bounces must be >= 1");
		if (s.n_spheres && (!s.sphere_center_x || !s.sphere_center_y || !s.sphere_center_z || !s.sphere_radius || !s.sphere_material))
			return fail(RT_HIP_INVALID_ARGUMENT, "scene: %u spheres but a sphere column is NULL", s.n_spheres);
		if (s.n_planes && (!s.plane_normal_x || !s.plane_normal_y || !s.plane_normal_z || !s.plane_d || !s.plane_material))
			return fail(RT_HIP_INVALID_ARGUMENT, "scene: %u planes but a plane column is NULL", s.n_planes);
		if (!s.n_materials && (s.n_spheres || s.n_planes || s.n_boxes))
			return fail(RT_HIP_INVALID_ARGUMENT, "scene: primitives present but no materials");
		if (s.n_materials && (!s.material_type || !s.material_albedo || !s.material_roughness || !s.material_reflectivity))
			return fail(RT_HIP_INVALID_ARGUMENT, "scene: %u materials but a material column is NULL", s.n_materials);
		if (s.n_boxes && (!s.box_center_x || !s.box_center_y || !s.box_center_z || !s.box_extents_x || !s.box_extents_y || !s.box_extents_z || !s.box_material))
			return fail(RT_HIP_INVALID_ARGUMENT, "scene: %u boxes but a box column is NULL", s.n_boxes);
		return ok();
	}

	// the part that walks the columns: needed only when their content is new (an unchanged fingerprint means these very
	// bytes passed before).  The reference's loader rejects out-of-range material indices (src/scene.cpp:568-574); an index
	// that got past it would read out of bounds on the device, so it is refused here too.
	rt_hip_status check_scene_indices(const rt_hip_scene& s)
	{
		for (uint32_t i = 0; i < s.n_spheres; i++)
			if (s.sphere_material[i] >= s.n_materials)
				return fail(RT_HIP_INVALID_ARGUMENT, "scene: sphere %u has material index %u out-of-range", i, s.sphere_material[i]);
		for (uint32_t i = 0; i < s.n_planes; i++)
			if (s.plane_material[i] >= s.n_materials)
				return fail(RT_HIP_INVALID_ARGUMENT, "scene: plane %u has material index %u out-of-range", i, s.plane_material[i]);
		for (uint32_t i = 0; i < s.n_boxes; i++)
			if (s.box_material[i] >= s.n_materials)
				return fail(RT_HIP_INVALID_ARGUMENT, "scene: box %u has material index %u out-of-range", i, s.box_material[i]);
		return ok();
	}

	constexpr size_t align_up(size_t v, size_t a)
	{
		return (v + a - 1) / a * a;
	}

	// A fingerprint of the caller's scene columns — FNV-1a style over 8-byte words, not a cryptographic hash.  rt has no
	// scene version counter (src/main.cpp:233-311), so every render() has to decide whether the columns in HBM are
	// still the caller's.  The columns are hashed WHERE THEY LIE, before anything is staged or copied: an unchanged scene
	// costs one pass over its bytes and nothing else.  Four interleaved lanes: one multiply per word is a dependency chain
	// of 3-4 cycles, and a single lane would spend 0.3 ms on the 2 MB of a 100 000-sphere scene.
	struct fingerprinter
	{
		static constexpr uint64_t prime = 0x100000001B3ull;
		uint64_t lane[4] = { 0xCBF29CE484222325ull, 0x9E3779B97F4A7C15ull, 0xBF58476D1CE4E5B9ull, 0x94D049BB133111EBull };

		void add(const void* data, size_t bytes)
		{
			const unsigned char* p = static_cast<const unsigned char*>(data);
			const size_t total = bytes;
			for (; bytes >= 32; bytes -= 32, p += 32)
			{
				uint64_t w[4];
				std::memcpy(w, p, 32);
				for (int k = 0; k < 4; k++)
					lane[k] = (lane[k] ^ w[k]) * prime;
			}
			for (; bytes >= 8; bytes -= 8, p += 8)
			{
				uint64_t w;
				std::memcpy(&w, p, 8);
				lane[0] = (lane[0] ^ w) * prime;
			}
			for (; bytes; bytes--, p++)
				lane[1] = (lane[1] ^ *p) * prime;
			lane[2] = (lane[2] ^ total) * prime; // the column's length: moving a row from one column to the next changes the print
		}
		void add_count(uint32_t n) { lane[3] = (lane[3] ^ n) * prime; }
		uint64_t value() const
		{
			uint64_t h = lane[0];
			for (int k = 1; k < 4; k++)
				h = (h ^ (lane[k] + (h << 6) + (h >> 2))) * prime;
			return h;
		}
	};

	uint64_t fingerprint_of(const rt_hip_scene& s)
	{
		fingerprinter f;
		f.add_count(s.n_spheres), f.add_count(s.n_planes), f.add_count(s.n_materials), f.add_count(s.n_boxes);
		const size_t sphere_bytes = static_cast<size_t>(s.n_spheres) * 4, plane_bytes = static_cast<size_t>(s.n_planes) * 4;
		const size_t material_bytes = static_cast<size_t>(s.n_materials) * 4, box_bytes = static_cast<size_t>(s.n_boxes) * 4;
		for (const void* column : { static_cast<const void*>(s.sphere_center_x), static_cast<const void*>(s.sphere_center_y), static_cast<const void*>(s.sphere_center_z),
									static_cast<const void*>(s.sphere_radius), static_cast<const void*>(s.sphere_material) })
			f.add(column, sphere_bytes);
		for (const void* column : { static_cast<const void*>(s.plane_normal_x), static_cast<const void*>(s.plane_normal_y), static_cast<const void*>(s.plane_normal_z),
									static_cast<const void*>(s.plane_d), static_cast<const void*>(s.plane_material) })
			f.add(column, plane_bytes);
		f.add(s.material_type, material_bytes);
		f.add(s.material_albedo, material_bytes * 4);
		f.add(s.material_roughness, material_bytes);
		f.add(s.material_reflectivity, material_bytes);
		for (const void* column : { static_cast<const void*>(s.box_center_x), static_cast<const void*>(s.box_center_y), static_cast<const void*>(s.box_center_z),
									static_cast<const void*>(s.box_extents_x), static_cast<const void*>(s.box_extents_y), static_cast<const void*>(s.box_extents_z),
									static_cast<const void*>(s.box_material) })
			f.add(column, box_bytes);
		return f.value();
	}

	scene_layout layout_of(const rt_hip_scene& s)
	{
		constexpr size_t column_alignment = 256;
		size_t offset = 0;
		const auto place = [&](size_t bytes)
		{
			const size_t at = offset;
			offset = align_up(offset + bytes, column_alignment);
			return at;
		};
		const size_t sphere_bytes = static_cast<size_t>(s.n_spheres) * 4;
		const size_t plane_bytes = static_cast<size_t>(s.n_planes) * 4;
		const size_t n_primitives = static_cast<size_t>(s.n_spheres) + s.n_planes + s.n_boxes; // (a box's rows: its material's entries, RT_HIP_FLAG_TRACE_BOXES)
		scene_layout L{};
		L.scx = place(sphere_bytes), L.scy = place(sphere_bytes), L.scz = place(sphere_bytes), L.sr = place(sphere_bytes), L.sm = place(sphere_bytes);
		L.pnx = place(plane_bytes), L.pny = place(plane_bytes), L.pnz = place(plane_bytes), L.pd = place(plane_bytes), L.pm = place(plane_bytes);
		L.shading = place(static_cast<size_t>(s.n_materials) * sizeof(float4));
		L.type = place(static_cast<size_t>(s.n_materials) * 4);
		L.geometry = place(n_primitives * sizeof(float4));
		L.prim_shading = place(n_primitives * sizeof(float4));
		L.prim_metal = place(n_primitives * 4);
		L.prim_shading_sm = place(n_primitives * sizeof(float4));
		L.prim_scatter_sm = place(n_primitives * 4);
		L.box_bounds = place(static_cast<size_t>(s.n_boxes) * 2 * sizeof(float4));
		L.albedo = place(static_cast<size_t>(s.n_materials) * sizeof(float4));
		L.total = offset ? offset : column_alignment;
		return L;
	}

}

namespace rt_hip
{
	rt_hip_status open_request(scene_request& r, const rt_hip_scene* scene)
	{
		if (const rt_hip_status st = check_scene_pointers(*scene))
			return st;
		r.scene = scene;
		r.layout = layout_of(*scene);
		r.print = fingerprint_of(*scene);
		return ok();
	}

	// The image is built in `owner`'s page-locked staging buffer and copied to HBM from there — by every member of a
	// multi-GPU context that needs it (the buffer is portable).  Not in a std::vector: the HIP runtime page-locks pageable
	// sources of large copies on the fly and keeps such locks cached by address after the copy (frame.hip, "Why the module
	// stages"); this module hands it no pageable memory at all, its own included.
	static rt_hip_status build_image(rt_hip_ctx* owner, scene_request& r)
	{
		const rt_hip_scene& s = *r.scene;
		const scene_layout& L = r.layout;
		RT_HIP_TRY(hipSetDevice(owner->device));
		RT_HIP_TRY(owner->scene_staging.reserve(L.total));
		unsigned char* const host = owner->scene_staging.as<unsigned char>();
		std::memset(host, 0, L.total);
		const auto put = [&](size_t at, const void* src, size_t bytes)
		{
			if (bytes)
				std::memcpy(host + at, src, bytes);
		};
		const size_t sphere_bytes = static_cast<size_t>(s.n_spheres) * 4;
		const size_t plane_bytes = static_cast<size_t>(s.n_planes) * 4;
		const size_t n_primitives = static_cast<size_t>(s.n_spheres) + s.n_planes + s.n_boxes;
		put(L.scx, s.sphere_center_x, sphere_bytes);
		put(L.scy, s.sphere_center_y, sphere_bytes);
		put(L.scz, s.sphere_center_z, sphere_bytes);
		put(L.sr, s.sphere_radius, sphere_bytes);
		put(L.sm, s.sphere_material, sphere_bytes);
		put(L.pnx, s.plane_normal_x, plane_bytes);
		put(L.pny, s.plane_normal_y, plane_bytes);
		put(L.pnz, s.plane_normal_z, plane_bytes);
		put(L.pd, s.plane_d, plane_bytes);
		put(L.pm, s.plane_material, plane_bytes);
		for (uint32_t m = 0; m < s.n_materials; m++)
		{
			// attenuation = vec3{ albedo * reflectivity } (mg_ray_tracer.cpp:115,131; colour * float, colour.hpp:144-149)
			const float refl = s.material_reflectivity[m];
			const float shading[4] = { s.material_albedo[m * 4 + 0] * refl,
									   s.material_albedo[m * 4 + 1] * refl,
									   s.material_albedo[m * 4 + 2] * refl,
									   s.material_roughness[m] };
			put(L.shading + m * sizeof(float4), shading, sizeof(shading));
		}
		put(L.type, s.material_type, static_cast<size_t>(s.n_materials) * 4);
		put(L.albedo, s.material_albedo, static_cast<size_t>(s.n_materials) * sizeof(float4));
		for (uint32_t i = 0; i < s.n_boxes; i++)
		{
			// corners = center -/+ extents (muu::bounding_box), material index riding in the spare lane
			float bounds[8] = { s.box_center_x[i] - s.box_extents_x[i], s.box_center_y[i] - s.box_extents_y[i], s.box_center_z[i] - s.box_extents_z[i], 0.0f,
								s.box_center_x[i] + s.box_extents_x[i], s.box_center_y[i] + s.box_extents_y[i], s.box_center_z[i] + s.box_extents_z[i], 0.0f };
			std::memcpy(&bounds[3], &s.box_material[i], 4);
			put(L.box_bounds + i * 2 * sizeof(float4), bounds, sizeof(bounds));
		}
		// derived per-primitive tables (spheres, then planes; then the boxes, of which RT_HIP_FLAG_TRACE_BOXES' kernels read the shading and
		// scatter rows: a box's corners are in box_bounds, its geometry row stays zero)
		r.small = small_scene{};
		r.small_sm = small_scene{};
		for (size_t i = 0; i < n_primitives; i++)
		{
			const bool is_sphere = i < s.n_spheres;
			const bool is_box = i >= static_cast<size_t>(s.n_spheres) + s.n_planes;
			const size_t k = is_sphere ? i : (is_box ? i - s.n_spheres - s.n_planes : i - s.n_spheres);
			float geometry[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
			uint32_t material;
			if (is_box)
				material = s.box_material[k];
			else if (is_sphere)
			{
				const float radius = s.sphere_radius[k];
				geometry[0] = s.sphere_center_x[k], geometry[1] = s.sphere_center_y[k], geometry[2] = s.sphere_center_z[k];
				geometry[3] = radius * radius; // radius^2, as hits_sphere squares it
				material = s.sphere_material[k];
			}
			else
			{
				geometry[0] = s.plane_normal_x[k], geometry[1] = s.plane_normal_y[k], geometry[2] = s.plane_normal_z[k];
				geometry[3] = s.plane_d[k];
				material = s.plane_material[k];
			}
			const uint32_t type = s.material_type[material];
			const uint32_t metal = type == RT_HIP_MATERIAL_METAL ? scatter_metal : scatter_lambert; // mg_ray_tracer.cpp:142-152
			// sm_ray_tracer.cpp:221-236
			const bool refracts = type == RT_HIP_MATERIAL_DIELECTRIC || type == RT_HIP_MATERIAL_AIR || type == RT_HIP_MATERIAL_VACUUM
							   || type == RT_HIP_MATERIAL_WATER || type == RT_HIP_MATERIAL_ICE;
			const uint32_t scatter_sm = refracts ? scatter_dielectric : metal;
			float shading_mg[4], shading_sm[4];
			std::memcpy(shading_mg, host + L.shading + material * sizeof(float4), sizeof(float4));
			std::memcpy(shading_sm, shading_mg, sizeof(float4));
			if (refracts)
				shading_sm[3] = s.material_reflectivity[material]; // index of refraction instead of the (unused) roughness
			put(L.geometry + i * sizeof(float4), geometry, sizeof(geometry));
			put(L.prim_shading + i * sizeof(float4), shading_mg, sizeof(float4));
			put(L.prim_metal + i * 4, &metal, 4);
			put(L.prim_shading_sm + i * sizeof(float4), shading_sm, sizeof(float4));
			put(L.prim_scatter_sm + i * 4, &scatter_sm, 4);
			if (i < scalar_max_spheres && !is_box) // (what the scalar-register kernel is given: meaningful for scenes of <= 8 spheres and planes)
			{
				std::memcpy(&r.small.geometry[i], geometry, sizeof(geometry));
				std::memcpy(&r.small.shading[i], shading_mg, sizeof(float4));
				r.small.scatter[i] = metal;
				std::memcpy(&r.small_sm.geometry[i], geometry, sizeof(geometry));
				std::memcpy(&r.small_sm.shading[i], shading_sm, sizeof(float4));
				r.small_sm.scatter[i] = scatter_sm;
			}
		}
		r.image = host;
		return ok();
	}

	// Make `ctx` hold the request's scene: nothing but the frame's scalars if the columns' fingerprint is the resident
	// one (the reference re-renders an unchanged scene every dirty frame, src/main.cpp:315-321), the full path otherwise.
	// Leaves ctx->device current.
	rt_hip_status make_resident(rt_hip_ctx* ctx, scene_request& r)
	{
		const auto t0 = std::chrono::steady_clock::now();
		const rt_hip_scene& s = *r.scene;
		const scene_layout& L = r.layout;
		RT_HIP_TRY(hipSetDevice(ctx->device));
		const bool resident = ctx->have_scene && ctx->scene_fingerprint == r.print && ctx->scene_bytes == L.total && ctx->scene_columns.bytes >= L.total;
		if (!resident)
		{
			if (!r.indices_checked)
			{
				if (const rt_hip_status st = check_scene_indices(s))
					return st;
				r.indices_checked = true;
			}
			if (!r.image)
				if (const rt_hip_status st = build_image(ctx, r))
					return st;
			RT_HIP_TRY(hipDeviceSynchronize()); // a previous frame may still be reading the old scene
			ctx->have_scene = false;
			RT_HIP_TRY(ctx->scene_columns.reserve(L.total));
			RT_HIP_TRY(hipMemcpy(ctx->scene_columns.ptr, r.image, L.total, hipMemcpyHostToDevice));
			ctx->scene_fingerprint = r.print;
			ctx->scene_bytes = L.total;
			ctx->scene_uploads++; // (a sphere hierarchy built for the previous scene is stale from here on: ensure_bvh)
			// ... and a box hierarchy only if the box pairs themselves changed (ensure_box_bvh): FNV-1a over their words
			uint64_t box_print = 0xcbf29ce484222325ull ^ s.n_boxes;
			for (size_t k = 0; k < static_cast<size_t>(s.n_boxes) * 8u; k++)
			{
				uint32_t word;
				std::memcpy(&word, r.image + L.box_bounds + k * 4u, 4);
				box_print = (box_print ^ word) * 0x100000001b3ull;
			}
			ctx->box_columns_print = box_print;
			ctx->small = r.small;
			ctx->small_sm = r.small_sm;
			// the sphere rows of the geometry table, as the kernels read them, for the sky band's rule (sky_band.hpp)
			ctx->sphere_table.clear();
			if (s.n_spheres <= sky_band_max_spheres)
			{
				ctx->sphere_table.resize(static_cast<size_t>(s.n_spheres) * 4u);
				if (s.n_spheres)
					std::memcpy(ctx->sphere_table.data(), r.image + L.geometry, ctx->sphere_table.size() * sizeof(float));
			}

			unsigned char* base = ctx->scene_columns.as<unsigned char>();
			device_scene& d = ctx->scene;
			d.n_spheres = s.n_spheres;
			d.n_planes = s.n_planes;
			d.n_materials = s.n_materials;
			d.sphere_cx = reinterpret_cast<const float*>(base + L.scx);
			d.sphere_cy = reinterpret_cast<const float*>(base + L.scy);
			d.sphere_cz = reinterpret_cast<const float*>(base + L.scz);
			d.sphere_r = reinterpret_cast<const float*>(base + L.sr);
			d.sphere_material = reinterpret_cast<const uint32_t*>(base + L.sm);
			d.plane_nx = reinterpret_cast<const float*>(base + L.pnx);
			d.plane_ny = reinterpret_cast<const float*>(base + L.pny);
			d.plane_nz = reinterpret_cast<const float*>(base + L.pnz);
			d.plane_d = reinterpret_cast<const float*>(base + L.pd);
			d.plane_material = reinterpret_cast<const uint32_t*>(base + L.pm);
			d.material_shading = reinterpret_cast<const float4*>(base + L.shading);
			d.material_type = reinterpret_cast<const uint32_t*>(base + L.type);
			d.primitive_geometry = reinterpret_cast<const float4*>(base + L.geometry);
			d.primitive_shading = reinterpret_cast<const float4*>(base + L.prim_shading);
			d.primitive_scatter = reinterpret_cast<const uint32_t*>(base + L.prim_metal);
			d.primitive_shading_sm = reinterpret_cast<const float4*>(base + L.prim_shading_sm);
			d.primitive_scatter_sm = reinterpret_cast<const uint32_t*>(base + L.prim_scatter_sm);
			d.n_boxes = s.n_boxes;
			d.box_bounds = reinterpret_cast<const float4*>(base + L.box_bounds);
			d.material_albedo = reinterpret_cast<const float4*>(base + L.albedo);
			d.planes_tame = 1u;
			for (uint32_t k = 0; k < s.n_planes; k++)
				for (const float n : { s.plane_normal_x[k], s.plane_normal_y[k], s.plane_normal_z[k] })
					if (!(std::fabs(n) <= 0x1p40f)) // (a NaN fails too)
						d.planes_tame = 0u;
		}
		ctx->samples_per_pixel = s.samples_per_pixel;
		ctx->max_bounces = s.max_bounces;
		std::memcpy(ctx->inverse_view_projection, s.inverse_view_projection, sizeof(ctx->inverse_view_projection));
		ctx->have_scene = true;
		ctx->phases.scene_resident = resident ? 1u : 0u;
		ctx->stats.upload_ms = static_cast<float>(seconds_since(t0) * 1e3);
		return ok();
	}

	// RT_HIP_FLAG_BVH_DEVICE_BUILD: the hierarchy built by bvh_build.hip from the table where it lies, enqueued on the frame's
	// stream.  Nothing is read back.  The call waits in two cases only: a block has to grow (what it held may still be read), and
	// `wait` (the frame keeps stats: upload_ms is to hold the build, as it holds the host's).
	static rt_hip_status build_bvh_on_device(rt_hip_ctx* ctx, hipStream_t stream, bool wait)
	{
		const auto t0 = std::chrono::steady_clock::now();
		const uint32_t n = ctx->scene.n_spheres;
		if (n > lbvh::max_spheres)
			return fail(RT_HIP_UNSUPPORTED, "RT_HIP_FLAG_BVH_DEVICE_BUILD: more than 2^26 spheres");
		RT_HIP_TRY(hipSetDevice(ctx->device));
		const bvh_build_sizes sizes = bvh_build_sizes_for(n);
		ctx->bvh_descriptor = nullptr;
		ctx->bvh_built_for = 0;
		if (sizes.block_bytes > ctx->bvh_block.bytes || sizes.scratch_bytes > ctx->bvh_scratch.bytes)
			RT_HIP_TRY(hipDeviceSynchronize()); // a previous frame may still be reading the tree that is about to be freed
		else if (ctx->launched && ctx->last_stream != stream)
			RT_HIP_TRY(hipStreamSynchronize(ctx->last_stream)); // ... or, on another stream, the tree that is about to be overwritten
		if (ctx->bvh_block.reserve(sizes.block_bytes) != hipSuccess || ctx->bvh_scratch.reserve(sizes.scratch_bytes) != hipSuccess)
		{
			(void)hipGetLastError();
			return fail(RT_HIP_RUNTIME_ERROR, "RT_HIP_FLAG_BVH_DEVICE_BUILD: no device memory for a hierarchy of %u spheres (%zu + %zu bytes)", n, sizes.block_bytes, sizes.scratch_bytes);
		}
		RT_HIP_TRY(build_bvh_device(ctx->scene.primitive_geometry, n, ctx->bvh_block.ptr, ctx->bvh_scratch.ptr, stream));
		ctx->launched = true;
		ctx->last_stream = stream;
		if (wait)
			RT_HIP_TRY(hipStreamSynchronize(stream));
		ctx->bvh_descriptor = ctx->bvh_block.as<const device_bvh>();
		ctx->bvh_built_for = ctx->scene_uploads;
		ctx->bvh_device_built = true;
		ctx->stats.upload_ms += static_cast<float>(seconds_since(t0) * 1e3);
		return ok();
	}

	// RT_HIP_FLAG_BVH: make ctx->bvh_descriptor describe a hierarchy of the resident scene, built at the first such frame after an
	// upload — or after a frame that asked for the other builder — and kept until the next one.  The host builder (bvh.cpp) works
	// from the (c, r^2) table read back from the device, the very floats the linear kernels read.  The build's time is added to
	// upload_ms.
	rt_hip_status ensure_bvh(rt_hip_ctx* ctx, bool device_build, hipStream_t stream, bool wait)
	{
		if (ctx->bvh_built_for == ctx->scene_uploads && ctx->bvh_device_built == device_build)
			return ok();
		if (device_build)
			return build_bvh_on_device(ctx, stream, wait);
		const auto t0 = std::chrono::steady_clock::now();
		const uint32_t n = ctx->scene.n_spheres;
		RT_HIP_TRY(hipSetDevice(ctx->device));
		RT_HIP_TRY(hipDeviceSynchronize()); // a previous frame may still be reading the old tree
		ctx->bvh_built_for = 0;
		std::vector<float> geometry(static_cast<size_t>(n) * 4);
		if (n)
			RT_HIP_TRY(hipMemcpy(geometry.data(), ctx->scene.primitive_geometry, static_cast<size_t>(n) * sizeof(float4), hipMemcpyDeviceToHost));
		bvh_host tree;
		std::string why;
		if (!build_bvh(geometry.data(), n, tree, why))
			return fail(RT_HIP_UNSUPPORTED, "RT_HIP_FLAG_BVH: %s", why.c_str());
		// one block: the descriptor the kernel reads first, nodes, leaf-ordered spheres, their scene indices, the always list
		// (256-byte aligned starts)
		const auto aligned = [](size_t bytes) { return (bytes + 255u) & ~static_cast<size_t>(255u); };
		const size_t nodes_at = aligned(sizeof(device_bvh)), spheres_at = nodes_at + aligned(tree.nodes.size() * 4), order_at = spheres_at + aligned(tree.spheres.size() * 4);
		const size_t always_at = order_at + aligned(tree.order.size() * 4), total = always_at + aligned(tree.always.size() * 4);
		std::vector<unsigned char> image(total, 0);
		std::memcpy(image.data() + nodes_at, tree.nodes.data(), tree.nodes.size() * 4);
		std::memcpy(image.data() + spheres_at, tree.spheres.data(), tree.spheres.size() * 4);
		std::memcpy(image.data() + order_at, tree.order.data(), tree.order.size() * 4);
		std::memcpy(image.data() + always_at, tree.always.data(), tree.always.size() * 4);
		ctx->bvh_descriptor = nullptr;
		RT_HIP_TRY(ctx->bvh_block.reserve(image.size()));
		unsigned char* const base = ctx->bvh_block.as<unsigned char>();
		device_bvh b{};
		b.nodes = reinterpret_cast<const float4*>(base + nodes_at);
		b.spheres = reinterpret_cast<const float4*>(base + spheres_at);
		b.order = reinterpret_cast<const uint32_t*>(base + order_at);
		b.always = reinterpret_cast<const uint32_t*>(base + always_at);
		b.root = tree.root;
		b.n_tree = static_cast<uint32_t>(tree.order.size());
		b.n_always = static_cast<uint32_t>(tree.always.size());
		b.cx = tree.centre[0], b.cy = tree.centre[1], b.cz = tree.centre[2], b.radius = tree.radius;
		std::memcpy(image.data(), &b, sizeof(b));
		RT_HIP_TRY(hipMemcpy(ctx->bvh_block.ptr, image.data(), image.size(), hipMemcpyHostToDevice));
		ctx->bvh_descriptor = reinterpret_cast<const device_bvh*>(base);
		ctx->bvh_built_for = ctx->scene_uploads;
		ctx->bvh_device_built = false;
		ctx->stats.upload_ms += static_cast<float>(seconds_since(t0) * 1e3);
		return ok();
	}

	// RT_HIP_FLAG_EMISSION: the light variant of the four per-primitive tables.  From the resident tables read back from
	// the device — the very rows the ordinary builds read — and the primitives' material indices: a primitive whose material is a light
	// gets (emission.rgb, 0) and scatter_emit under both scatter tables, every other row is the ordinary table's.  One block, 256-byte
	// aligned starts.  Stale after a scene upload (even of an unchanged fingerprint's re-upload) and after rt_hip_set_emission.
	rt_hip_status ensure_light_tables(rt_hip_ctx* ctx)
	{
		if (ctx->light_tables_uploads == ctx->scene_uploads && ctx->light_tables_version == ctx->emission_version && ctx->light_shading)
			return ok();
		const auto t0 = std::chrono::steady_clock::now();
		const device_scene& d = ctx->scene;
		if (ctx->emission_rows != d.n_materials) // (the caller's check; an index below must stay inside the table)
			return fail(RT_HIP_INVALID_ARGUMENT, "RT_HIP_FLAG_EMISSION: the emission table has %u rows, the resident scene %u materials", ctx->emission_rows, d.n_materials);
		RT_HIP_TRY(hipSetDevice(ctx->device));
		RT_HIP_TRY(hipDeviceSynchronize()); // a previous frame may still be reading the old tables
		ctx->light_tables_uploads = 0;
		ctx->light_shading = ctx->light_shading_sm = nullptr;
		ctx->light_scatter = ctx->light_scatter_sm = nullptr;
		ctx->light_scatter_direct = ctx->light_scatter_sm_direct = nullptr;
		ctx->sampled_lights = 0;
		const size_t n_primitives = static_cast<size_t>(d.n_spheres) + d.n_planes + d.n_boxes;
		std::vector<uint32_t> material(n_primitives, 0u);
		std::vector<float> box_bounds(static_cast<size_t>(d.n_boxes) * 8u);
		if (d.n_spheres)
			RT_HIP_TRY(hipMemcpy(material.data(), d.sphere_material, static_cast<size_t>(d.n_spheres) * 4u, hipMemcpyDeviceToHost));
		if (d.n_planes)
			RT_HIP_TRY(hipMemcpy(material.data() + d.n_spheres, d.plane_material, static_cast<size_t>(d.n_planes) * 4u, hipMemcpyDeviceToHost));
		if (d.n_boxes)
		{
			RT_HIP_TRY(hipMemcpy(box_bounds.data(), d.box_bounds, box_bounds.size() * 4u, hipMemcpyDeviceToHost));
			for (uint32_t i = 0; i < d.n_boxes; i++) // (the material index rides in the min corner's spare lane: build_image)
				std::memcpy(&material[static_cast<size_t>(d.n_spheres) + d.n_planes + i], &box_bounds[static_cast<size_t>(i) * 8u + 3u], 4);
		}
		const size_t shading_bytes = align_up(n_primitives * sizeof(float4), 256), scatter_bytes = align_up(n_primitives * 4u, 256);
		// (RT_HIP_FLAG_DIRECT_LIGHT, DESIGN.md §3.13: the sampled-light list in FRONT of the shading table — kernels.hpp, direct_list_bytes — and the two
		// scatter tables a second time, with scatter_emit_sampled in the sampled lights' rows)
		const size_t list_at = 0, shading_at = direct_list_bytes, scatter_at = shading_at + shading_bytes, shading_sm_at = scatter_at + scatter_bytes, scatter_sm_at = shading_sm_at + shading_bytes;
		const size_t scatter_direct_at = scatter_sm_at + scatter_bytes, scatter_sm_direct_at = scatter_direct_at + scatter_bytes;
		const size_t total = scatter_sm_direct_at + scatter_bytes;
		std::vector<unsigned char> image(total, 0);
		if (n_primitives)
		{
			RT_HIP_TRY(hipMemcpy(image.data() + shading_at, d.primitive_shading, n_primitives * sizeof(float4), hipMemcpyDeviceToHost));
			RT_HIP_TRY(hipMemcpy(image.data() + scatter_at, d.primitive_scatter, n_primitives * 4u, hipMemcpyDeviceToHost));
			RT_HIP_TRY(hipMemcpy(image.data() + shading_sm_at, d.primitive_shading_sm, n_primitives * sizeof(float4), hipMemcpyDeviceToHost));
			RT_HIP_TRY(hipMemcpy(image.data() + scatter_sm_at, d.primitive_scatter_sm, n_primitives * 4u, hipMemcpyDeviceToHost));
		}
		for (size_t i = 0; i < n_primitives; i++)
		{
			const uint32_t m = material[i];
			if (m >= ctx->emission_rows) // (make_resident refuses such an index: never)
				return fail(RT_HIP_RUNTIME_ERROR, "RT_HIP_FLAG_EMISSION: primitive %zu has material index %u out-of-range", i, m);
			const float* const rgb = ctx->emission.data() + static_cast<size_t>(m) * 3u;
			if (!is_light(rgb))
				continue;
			const float row[4] = { rgb[0], rgb[1], rgb[2], 0.0f };
			const uint32_t emit = scatter_emit;
			for (const size_t at : { shading_at, shading_sm_at })
				std::memcpy(image.data() + at + i * sizeof(float4), row, sizeof row);
			for (const size_t at : { scatter_at, scatter_sm_at })
				std::memcpy(image.data() + at + i * 4u, &emit, 4);
		}
		// the direct variant of the scatter tables and the list: a sphere whose material is a light and whose radius is finite and > 0 is a
		// SAMPLED light, the first direct_max_lights of them in sphere order; every other light keeps scatter_emit
		std::memcpy(image.data() + scatter_direct_at, image.data() + scatter_at, n_primitives * 4u);
		std::memcpy(image.data() + scatter_sm_direct_at, image.data() + scatter_sm_at, n_primitives * 4u);
		uint32_t n_sampled = 0;
		if (d.n_spheres)
		{
			std::vector<float> columns(static_cast<size_t>(d.n_spheres) * 4u);
			const float* const sources[4] = { d.sphere_cx, d.sphere_cy, d.sphere_cz, d.sphere_r };
			for (size_t c = 0; c < 4; c++)
				RT_HIP_TRY(hipMemcpy(columns.data() + c * d.n_spheres, sources[c], static_cast<size_t>(d.n_spheres) * 4u, hipMemcpyDeviceToHost));
			for (uint32_t i = 0; i < d.n_spheres && n_sampled < direct_max_lights; i++)
			{
				const float* const rgb = ctx->emission.data() + static_cast<size_t>(material[i]) * 3u;
				const float radius = columns[3u * static_cast<size_t>(d.n_spheres) + i];
				if (!is_light(rgb) || !std::isfinite(radius) || !(radius > 0.0f))
					continue;
				const uint32_t sampled = scatter_emit_sampled;
				const float rows[8] = { columns[i], columns[static_cast<size_t>(d.n_spheres) + i], columns[2u * static_cast<size_t>(d.n_spheres) + i], radius, rgb[0], rgb[1], rgb[2], 0.0f };
				unsigned char* const entry = image.data() + list_at + direct_list_header_bytes + static_cast<size_t>(n_sampled) * sizeof rows;
				std::memcpy(entry, rows, sizeof rows);
				std::memcpy(entry + 28, &i, 4); // (the sphere's index as bits, in the emission row's spare lane)
				std::memcpy(image.data() + scatter_direct_at + static_cast<size_t>(i) * 4u, &sampled, 4);
				std::memcpy(image.data() + scatter_sm_direct_at + static_cast<size_t>(i) * 4u, &sampled, 4);
				n_sampled++;
			}
		}
		std::memcpy(image.data() + list_at, &n_sampled, 4);
		RT_HIP_TRY(ctx->light_tables.reserve(total));
		RT_HIP_TRY(hipMemcpy(ctx->light_tables.ptr, image.data(), total, hipMemcpyHostToDevice));
		const unsigned char* const base = ctx->light_tables.as<unsigned char>();
		ctx->light_shading = reinterpret_cast<const float4*>(base + shading_at);
		ctx->light_scatter = reinterpret_cast<const uint32_t*>(base + scatter_at);
		ctx->light_shading_sm = reinterpret_cast<const float4*>(base + shading_sm_at);
		ctx->light_scatter_sm = reinterpret_cast<const uint32_t*>(base + scatter_sm_at);
		ctx->light_scatter_direct = reinterpret_cast<const uint32_t*>(base + scatter_direct_at);
		ctx->light_scatter_sm_direct = reinterpret_cast<const uint32_t*>(base + scatter_sm_direct_at);
		ctx->sampled_lights = n_sampled;
		ctx->light_tables_uploads = ctx->scene_uploads;
		ctx->light_tables_version = ctx->emission_version;
		ctx->stats.upload_ms += static_cast<float>(seconds_since(t0) * 1e3);
		return ok();
	}

	rt_hip_status ensure_box_bvh(rt_hip_ctx* ctx, hipStream_t stream)
	{
		RT_HIP_TRY(hipSetDevice(ctx->device));
		const uint32_t n = ctx->scene.n_boxes;
		if (!(ctx->box_bvh_built && ctx->box_bvh_print == ctx->box_columns_print && ctx->box_bvh_count == n))
		{
			const auto t0 = std::chrono::steady_clock::now();
			RT_HIP_TRY(hipDeviceSynchronize()); // a previous frame may still be reading the old tree
			ctx->box_bvh_built = false;
			ctx->box_bvh_sphere_stamp = 0;
			// from the pairs read back from the device: the very floats the linear box builds read
			std::vector<float> bounds(static_cast<size_t>(n) * 8);
			if (n)
				RT_HIP_TRY(hipMemcpy(bounds.data(), ctx->scene.box_bounds, static_cast<size_t>(n) * 2u * sizeof(float4), hipMemcpyDeviceToHost));
			box_bvh_host tree;
			std::string why;
			if (!build_box_bvh(bounds.data(), n, tree, why))
				return fail(RT_HIP_UNSUPPORTED, "RT_HIP_FLAG_BOX_BVH: %s", why.c_str());
			// one block: the two descriptors the kernel reads first, nodes, leaf-ordered corners, their scene indices, the always
			// list (256-byte aligned starts)
			const auto aligned = [](size_t bytes) { return (bytes + 255u) & ~static_cast<size_t>(255u); };
			const size_t nodes_at = aligned(box_bvh_descriptor_offset + sizeof(device_box_bvh)), corners_at = nodes_at + aligned(tree.nodes.size() * 4), order_at = corners_at + aligned(tree.corners.size() * 4);
			const size_t always_at = order_at + aligned(tree.order.size() * 4), total = always_at + aligned(tree.always.size() * 4);
			std::vector<unsigned char> image(total, 0);
			std::memcpy(image.data() + nodes_at, tree.nodes.data(), tree.nodes.size() * 4);
			std::memcpy(image.data() + corners_at, tree.corners.data(), tree.corners.size() * 4);
			std::memcpy(image.data() + order_at, tree.order.data(), tree.order.size() * 4);
			std::memcpy(image.data() + always_at, tree.always.data(), tree.always.size() * 4);
			RT_HIP_TRY(ctx->box_bvh_block.reserve(image.size()));
			unsigned char* const base = ctx->box_bvh_block.as<unsigned char>();
			device_box_bvh b{};
			b.nodes = reinterpret_cast<const float4*>(base + nodes_at);
			b.corners = reinterpret_cast<const float4*>(base + corners_at);
			b.order = reinterpret_cast<const uint32_t*>(base + order_at);
			b.always = reinterpret_cast<const uint32_t*>(base + always_at);
			b.root = tree.root;
			b.n_tree = static_cast<uint32_t>(tree.order.size());
			b.n_always = static_cast<uint32_t>(tree.always.size());
			std::memcpy(image.data() + box_bvh_descriptor_offset, &b, sizeof(b));
			RT_HIP_TRY(hipMemcpy(ctx->box_bvh_block.ptr, image.data(), image.size(), hipMemcpyHostToDevice));
			ctx->box_bvh_print = ctx->box_columns_print;
			ctx->box_bvh_count = n;
			ctx->box_bvh_built = true;
			ctx->box_bvh_builds++;
			ctx->stats.upload_ms += static_cast<float>(seconds_since(t0) * 1e3);
		}
		// the sphere hierarchy's descriptor in front, as the kernel expects it where item_sums points (stream-ordered: after a device
		// build enqueued on `stream`, and after whatever frame of this stream still reads the old copy)
		const uint64_t stamp = 2u * ctx->bvh_built_for + (ctx->bvh_device_built ? 1u : 0u);
		if (!ctx->bvh_descriptor || !ctx->bvh_built_for)
			return fail(RT_HIP_RUNTIME_ERROR, "RT_HIP_FLAG_BOX_BVH: no sphere hierarchy to travel with");
		if (ctx->box_bvh_sphere_stamp != stamp)
		{
			RT_HIP_TRY(hipMemcpyAsync(ctx->box_bvh_block.ptr, ctx->bvh_descriptor, sizeof(device_bvh), hipMemcpyDeviceToDevice, stream));
			ctx->box_bvh_sphere_stamp = stamp;
		}
		return ok();
	}
}

extern "C" rt_hip_status rt_hip_scene_check(const rt_hip_scene* scene, uint64_t* out_fingerprint)
{
	if (!scene)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_scene_check: NULL argument");
	if (const rt_hip_status st = check_scene_pointers(*scene))
		return st;
	if (const rt_hip_status st = check_scene_indices(*scene))
		return st;
	if (out_fingerprint)
		*out_fingerprint = fingerprint_of(*scene);
	return ok();
}

extern "C" rt_hip_status rt_hip_scene_upload(rt_hip_ctx* ctx, const rt_hip_scene* scene)
{
	if (!ctx || !scene)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_scene_upload: NULL argument");
	try // nothing may propagate through the C boundary (the staging image allocates)
	{
		const auto t0 = std::chrono::steady_clock::now();
		scene_request request;
		if (const rt_hip_status st = open_request(request, scene))
			return st;
		if (const rt_hip_status st = make_resident(ctx, request))
			return st;
		ctx->stats.upload_ms = static_cast<float>(seconds_since(t0) * 1e3); // including the fingerprint pass
		return ok();
	}
	catch (const std::exception& e)
	{
		return fail(RT_HIP_RUNTIME_ERROR, "rt_hip_scene_upload: %s", e.what());
	}
	catch (...)
	{
		return fail(RT_HIP_RUNTIME_ERROR, "rt_hip_scene_upload: unknown exception");
	}
}
