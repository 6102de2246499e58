/*
 * rt_hip.h — C ABI of the MI355X (gfx950) renderer module for marzer/rt.
 *
 * This is the drop-in boundary for ONE path of the reference: mg_ray_tracer::render
 * (reference src/renderers/mg_ray_tracer.cpp:178-205) behind renderer_interface::render
 * (reference src/renderer.hpp:9-14).  Everything that crosses it is plain C: pointers, sizes,
 * POD structs.  No C++ types, no exceptions, no torch types.
 *
 * The reference-side binding (a ~60 line renderer that gathers the soagen column pointers and
 * the camera matrix and calls rt_hip_render) is shown in INTEGRATION.md and shim/hip_ray_tracer.cpp.
 *
 * Every function that can fail returns an rt_hip_status (0 = success).  On failure a
 * human-readable message is available from rt_hip_last_error() (thread-local).  The reference's
 * render() is `noexcept` and returns void (src/renderer.hpp:11); the shim therefore logs the
 * message in the reference's `error: ...` style (src/main.cpp:43-47) and leaves the caller's
 * pre-cleared frame (src/main.cpp:318) untouched.
 */
#ifndef RT_HIP_H
#define RT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 6 (round 5): arithmetic contract v4 — the same entry points, DIFFERENT frames for a given seed — and three more words at the
 * end of rt_hip_phases.  5 (round 4): rt_hip_live_frame_locks added; the known-answer hooks of rounds 1-3 moved to the test-only
 * library (include/rt_hip_kat.h); rt_hip_render without RT_HIP_FLAG_PERSISTENT_FRAME delivers through the module's own frame.
 * A consumer checks rt_hip_abi_version() against the header it was compiled with. */
#define RT_HIP_ABI_VERSION 6u

/* librt_hip.so is built with hidden visibility: these entry points are ALL it exports. */
#if defined(__GNUC__)
#define RT_HIP_API __attribute__((visibility("default")))
#else
#define RT_HIP_API
#endif

typedef enum rt_hip_status
{
	RT_HIP_OK				 = 0,
	RT_HIP_INVALID_ARGUMENT	 = 1, /* null pointer, zero size, out-of-range material index, ... */
	RT_HIP_NO_DEVICE		 = 2, /* no gfx950 device visible / bad device ordinal */
	RT_HIP_RUNTIME_ERROR	 = 3, /* a HIP call failed; message carries hipGetErrorString */
	RT_HIP_NO_SCENE			 = 4, /* render requested before a scene was uploaded */
	RT_HIP_UNSUPPORTED		 = 5, /* unknown flag bits */
	RT_HIP_TIMEOUT			 = 6  /* rt_hip_join_ranks: the other ranks did not arrive within the deadline */
} rt_hip_status;

/* Material kinds, in the order of `enum class material_type` (reference src/common.hpp:105-115).
 * mg_ray_tracer shades metal with metal_scatter and EVERYTHING else with lambert_scatter
 * (reference src/renderers/mg_ray_tracer.cpp:142-152). */
enum
{
	RT_HIP_MATERIAL_LAMBERT	   = 0,
	RT_HIP_MATERIAL_METAL	   = 1,
	RT_HIP_MATERIAL_DIELECTRIC = 2,
	RT_HIP_MATERIAL_AIR		   = 3,
	RT_HIP_MATERIAL_VACUUM	   = 4,
	RT_HIP_MATERIAL_WATER	   = 5,
	RT_HIP_MATERIAL_ICE		   = 6,
	RT_HIP_MATERIAL_DIAMOND	   = 7,
	RT_HIP_MATERIAL_COUNT	   = 8
};

/*
 * The scene as the renderer sees it: the soagen struct-of-arrays columns of rt::spheres / rt::planes /
 * rt::materials (reference src/soa.toml:6-33, accessors src/soa.hpp:177-199) plus the two scalars of
 * rt::scene (reference src/scene.hpp:10-11) and the camera's inverse view-projection for the frame
 * size being rendered (reference src/camera.hpp:18,122-137).
 *
 * All pointers are HOST pointers borrowed for the duration of the call that takes the struct.
 * Columns hold exactly n_* valid rows; soagen's padding rows past size() are never read
 * (reference vendor/soagen.hpp:3777,7075-7082).  A count of 0 allows the matching pointers to be NULL.
 */
typedef struct rt_hip_scene
{
	/* rt::spheres — center_x/center_y/center_z/radius/material columns (src/soa.toml:25-33) */
	uint32_t n_spheres;
	const float* sphere_center_x;
	const float* sphere_center_y;
	const float* sphere_center_z;
	const float* sphere_radius;
	const uint32_t* sphere_material;

	/* rt::planes — normal_x/normal_y/normal_z/d/material columns (src/soa.toml:15-23);
	 * plane equation n·p + d = 0 with |n| = 1 (src/scene.cpp:580-583) */
	uint32_t n_planes;
	const float* plane_normal_x;
	const float* plane_normal_y;
	const float* plane_normal_z;
	const float* plane_d;
	const uint32_t* plane_material;

	/* rt::materials — type/albedo/roughness/reflectivity columns (src/soa.toml:6-13);
	 * albedo is rt::colour = 4 floats r,g,b,a per material (src/colour.hpp:17-57) */
	uint32_t n_materials;
	const uint32_t* material_type;
	const float* material_albedo;
	const float* material_roughness;
	const float* material_reflectivity;

	/* rt::scene::samples_per_pixel / max_bounces (src/scene.hpp:10-11), both >= 1 */
	uint32_t samples_per_pixel;
	uint32_t max_bounces;

	/* viewport::inverse_view_projection for THIS frame size (src/camera.hpp:18,134).
	 * Fixed order, independent of muu's storage order: element [r*4 + c] = m(r, c), so that
	 * transform_position(v) = (M * (v.x, v.y, v.z, 1)).xyz / .w  with row r = sum_c m(r,c) * v_c. */
	float inverse_view_projection[16];

	/* rt::boxes — center_x..center_z/extents_x..extents_z/material columns (src/soa.toml:35-45); extents are half
	 * sizes (muu::bounding_box).  mg_ray_tracer never hits boxes (mg_ray_tracer.cpp:89-93): the preview
	 * (RT_HIP_FLAG_PREVIEW, reference src/renderers/rasterizer.cpp:57) draws them, and the traced frame does under
	 * RT_HIP_FLAG_TRACE_BOXES only. */
	uint32_t n_boxes;
	const float* box_center_x;
	const float* box_center_y;
	const float* box_center_z;
	const float* box_extents_x;
	const float* box_extents_y;
	const float* box_extents_z;
	const uint32_t* box_material;
} rt_hip_scene;

/*
 * How the image is split across the GPUs of one node: rows are grouped into stripes of `stripe_rows`
 * rows; stripe b belongs to rank (b % world).  A rank renders only its own stripes into a compact
 * buffer of rt_hip_local_rows() rows x W pixels (stripe b of the image = stripe b / world of the local
 * buffer).  Random streams are keyed by the GLOBAL pixel index, so the assembled image does not depend
 * on `world`.  {0, 1, any} = the whole image.  (New: the reference is single-process,
 * src/renderers/mg_ray_tracer.cpp:203.)
 */
typedef struct rt_hip_partition
{
	uint32_t rank;
	uint32_t world;
	uint32_t stripe_rows;
} rt_hip_partition;

#define RT_HIP_DEFAULT_STRIPE_ROWS 8u

/* Work counters of the most recent render on a context (all ranks count their own share). */
typedef struct rt_hip_stats
{
	uint64_t primary_samples; /* pixels rendered by this rank x samples_per_pixel */
	uint64_t segments;		  /* calls of trace() that did not return at the bounce limit check, i.e. closest-hit queries */
	uint64_t sphere_tests;	  /* segments x n_spheres (also under RT_HIP_FLAG_BVH: the linear scan's count, not the spheres the tree visited) */
	uint64_t plane_tests;	  /* segments x n_planes (box tests under RT_HIP_FLAG_TRACE_BOXES are not counted) */
	float render_ms;		  /* device time of the render kernel(s), HIP events on the launch stream */
	float upload_ms;		  /* host wall time of the last scene upload */
	float readback_ms;		  /* rt_hip_render only: host wall time from "kernels done" to "frame in the caller's buffer" */
	uint32_t kernel_variant;  /* which kernel ran: RT_HIP_KERNEL_* */
} rt_hip_stats;

enum
{
	RT_HIP_KERNEL_NONE		= 0,
	RT_HIP_KERNEL_RESIDENT	= 1, /* a pixel tile per wave; planes (and fewer than 40 spheres) resident in LDS for the lifetime of the workgroup (<= 1024 of them) */
	RT_HIP_KERNEL_TILED		= 2, /* primitives streamed from the SoA columns through LDS in tiles (large scenes) */
	RT_HIP_KERNEL_SMALL		= 3, /* <= 8 primitives (>= 1 sphere, <= 3 planes): scene in scalar registers, scan fully unrolled */
	RT_HIP_KERNEL_PREVIEW	= 4, /* RT_HIP_FLAG_PREVIEW: one primary ray per pixel, N.L shading */
	RT_HIP_KERNEL_STREAMED	= 5, /* primitives read from the table in HBM/L2 with wave-uniform scalar loads: no staging, no barriers */
	RT_HIP_KERNEL_BVH		= 6	 /* RT_HIP_FLAG_BVH: a pixel tile per wave, spheres through the bounding volume hierarchy, one traversal per lane */
};

/* Render flags.  0 = the parity contract: arithmetic bit-identical to oracle/ (see DESIGN.md §3). */
enum
{
	RT_HIP_FLAG_NONE = 0u,
	/* force the LDS-tiled kernel even for scenes that fit a smaller one (testing) */
	RT_HIP_FLAG_FORCE_TILED = 1u << 0,
	/* force the LDS-resident kernel for scenes that would take the scalar-register one (testing) */
	RT_HIP_FLAG_FORCE_RESIDENT = 1u << 1,
	/* rt_hip_render only, OPT-IN: zero-copy delivery.  By default (flag absent) the kernels store finished pixels into a
	 * page-locked frame the MODULE owns and host threads carry them on into `pixels_rgba8888` while the frame is still being
	 * traced: the caller's buffer is plain memory to the module, touched only by CPU stores inside the call, and may be
	 * freed, re-created or recycled at will between two calls (what rt does on every resize, reference src/window.cpp:198-203).
	 * WITH the flag the caller promises that `pixels_rgba8888` stays allocated, at this address and size, until the next
	 * rt_hip_render call on this context with another buffer, rt_hip_forget_frame or rt_hip_destroy.  The module then
	 * page-locks the CALLER's buffer once and maps it into the GPU's address space: the kernels store every finished pixel
	 * straight into it and no second copy of the frame exists (a few tens of microseconds less per 1080p frame).  A caller
	 * that frees the buffer and may get the same address back from its allocator before the next frame MUST call
	 * rt_hip_forget_frame() in between: a mapping re-created under a live page-lock is a GPU memory fault
	 * (INTEGRATION.md §3). */
	RT_HIP_FLAG_PERSISTENT_FRAME = 1u << 2,
	/* shade with sm_ray_tracer's scatter table (reference src/renderers/sm_ray_tracer.cpp:221-236) instead of
	 * mg_ray_tracer's: dielectric, air, vacuum, water and ice refract/reflect through dielectric_scatter (:181-219),
	 * with the material's reflectivity as index of refraction.  Everything else is unchanged.  Opt-in: the parity
	 * contract of this module is mg_ray_tracer, under which those materials are lambert. */
	RT_HIP_FLAG_SM_MATERIALS = 1u << 3,
	/* draw the fast preview of reference src/renderers/rasterizer.cpp:24-85 instead of tracing paths (rt shows it at
	 * low resolution while the camera moves, src/main.cpp:106,319): ONE ray through each pixel centre, closest hit
	 * over planes, then boxes, then spheres, shaded 0.25 + 0.75 * albedo * (N . direction to the eye), the sky where
	 * nothing is hit.  Deterministic: seed, samples_per_pixel and max_bounces are not read; d_rgb_f32 / rgb_f32
	 * receive the colour before packing.  Partition, gather and assemble work as for the traced frame. */
	RT_HIP_FLAG_PREVIEW = 1u << 4,
	/* force the scalar-streamed kernel (it is what scenes above about 1300 primitives get) */
	RT_HIP_FLAG_FORCE_STREAMED = 1u << 5,
	/* Contract "v2-fast": the kernels built with the hardware's reciprocal / square-root / reciprocal-square-root
	 * approximations (about 1 ulp each, no correction steps, no range guards) and with multiply-adds contracted — the
	 * latitude the reference's own build takes (-ffast-math -ffp-contract=fast, meson.build:153-160).  Same random
	 * streams, same algorithm, same operation order otherwise.  The frame is NOT bit-identical to the oracle's: the
	 * per-pixel float mean agrees to a few 1e-6 relative wherever no sample's hit/miss decision flipped at a silhouette
	 * (tests/test_gpu_fast.py states and checks the bounds).  Not available with RT_HIP_FLAG_SM_MATERIALS or
	 * RT_HIP_FLAG_PREVIEW.  Opt-in; flags == 0 stays the parity contract. */
	RT_HIP_FLAG_FAST = 1u << 6,
	/* rt_hip_render only: keep the work counters and the kernel's device time of this frame for a later
	 * rt_hip_stats_fetch / rt_hip_phases_fetch even though `stats` is NULL.  A call with stats == NULL and without this flag
	 * is the plug-in's call (shim/hip_ray_tracer.cpp): nothing but the launch and the wait is enqueued — no timing events, no
	 * zeroing and read-back of the counters — which is what the launch-bound low-resolution preview frames of
	 * reference src/main.cpp:315-321 want; rt_hip_stats_fetch after such a frame reports render_ms = 0 and segments = 0. */
	RT_HIP_FLAG_STATS = 1u << 7,
	/* Work items of the small-scene kernels are whole 16-sample chunks, or — for launches that hold only a few chunks per
	 * lane of the device — half chunks (HISTORY.md §5 "Half-chunk items"): the launch code decides by the size of the launch, and the frame is
	 * the same bit for bit either way.  These two take the decision away from it (tests; never both). */
	RT_HIP_FLAG_FORCE_HALF_CHUNKS = 1u << 8,
	RT_HIP_FLAG_FORCE_WHOLE_CHUNKS = 1u << 9,
	/* OPT-IN: trace the spheres through a bounding volume hierarchy (binned-SAH binary tree, leaves of up to four spheres;
	 * planes keep their linear scan) instead of testing every sphere on every path segment: O(log n) per query instead of
	 * O(n), for scenes of thousands of spheres and more.  The PROMISE: the same frame, bit for bit, and the same `segments`
	 * as without the flag — every sphere the tree reaches is tested with the linear scan's arithmetic, ties go to the lower
	 * index, and no sphere is culled whose computed distance could win.  The tree is built on the host at the
	 * first such frame after the scene's columns changed (counted in `upload_ms`), kept while they stay the same, and freed
	 * with the context.  kernel_variant reports RT_HIP_KERNEL_BVH.  Refused (RT_HIP_UNSUPPORTED) with RT_HIP_FLAG_FORCE_TILED,
	 * _FORCE_RESIDENT, _FORCE_STREAMED and RT_HIP_FLAG_FAST; ignored with RT_HIP_FLAG_PREVIEW (one ray per pixel: nothing to
	 * gain).  Works with RT_HIP_FLAG_SM_MATERIALS and on every kind of context.  LDS: the kernel's traversal stacks (24 KiB) stand in
	 * front of the pixels' chunk sums, 65 664 bytes together at 3409 samples and 73 728 at 4096 — a frame, a pass or an adaptive pass is
	 * launched only if the DEVICE gives one workgroup that much (hipDeviceProp_t::sharedMemPerBlock, read when the context is made), and is
	 * otherwise refused with RT_HIP_UNSUPPORTED and a message that says how many samples fit (3408 at 64 KiB).  The MI355X gives a
	 * workgroup 160 KiB and renders these frames: observed (tests/test_gpu_chunk_sweep.py), not derived.  A library older than this flag
	 * refuses the bit with RT_HIP_UNSUPPORTED (unknown flag bits): that is how a caller finds out whether it is there. */
	RT_HIP_FLAG_BVH = 1u << 10,
	/* OPT-IN, modifies RT_HIP_FLAG_BVH: build the hierarchy on the GPU from the resident (c, r^2) table — a Morton-ordered
	 * binary tree (radix sort, one launch per level, bottom-up boxes) instead of the host's binned SAH — on the frame's stream,
	 * with no read-back of the table and no host build.  The PROMISE is RT_HIP_FLAG_BVH's: the same frame bit for bit, the same
	 * `segments`, kernel_variant RT_HIP_KERNEL_BVH; the traversal does not depend on the tree's shape.  What changes is where
	 * the time goes: the build leaves the host, and the Morton tree is not the SAH tree, so a cached frame may render slower
	 * through it (DESIGN.md §9 has the measured table; nothing here promises a net gain).  The cached tree remembers its
	 * builder: asking for the other one after the same upload rebuilds it.  `upload_ms` includes the build on frames that keep
	 * stats (the call then waits for it).  Takes scenes of up to 2^26 spheres.  Refused (RT_HIP_UNSUPPORTED) without
	 * RT_HIP_FLAG_BVH and wherever RT_HIP_FLAG_BVH is refused; ignored with RT_HIP_FLAG_PREVIEW. */
	RT_HIP_FLAG_BVH_DEVICE_BUILD = 1u << 11,
	/* (bit 12 stays unassigned: the tests pin 1u << 12 as "unknown flag bits") */
	/* OPT-IN: trace the scene's BOXES.  The reference's path tracers never hit a box (test_boxes is a stub that always misses,
	 * mg_ray_tracer.cpp:89-93, sm_ray_tracer.cpp:90), and without this flag neither does the module: a scene with boxes renders
	 * exactly as it always did.  With it every closest-hit query also scans the boxes — the slab test of the preview, accepted
	 * like spheres and planes (nothing nearer than 0.001, ties to the lower index), combined as the reference's own line
	 * mg_ray_tracer.cpp:162 combines its stub: a box wins a distance tie against a sphere or a plane — and a box hit is shaded
	 * through box_material like any other primitive, from its outward face normal (DESIGN.md §3.7 has the contract; the frame is
	 * held bit for bit to its CPU restatement, tests/native/box_reference.cpp).  kernel_variant reports RT_HIP_KERNEL_RESIDENT, or
	 * RT_HIP_KERNEL_BVH with RT_HIP_FLAG_BVH and for scenes of the streamed kernel's size (the hierarchy is then built as for
	 * RT_HIP_FLAG_BVH); scenes of the scalar-register kernel's size take the resident one.  Box tests are not counted: `segments`
	 * counts as before, rt_hip_stats is unchanged.
	 * Works with RT_HIP_FLAG_SM_MATERIALS, RT_HIP_FLAG_BVH, RT_HIP_FLAG_BVH_DEVICE_BUILD and RT_HIP_FLAG_STATS, in rt_hip_render and
	 * rt_hip_render_device, on every kind of context.  With n_boxes == 0 it changes nothing at all; ignored with
	 * RT_HIP_FLAG_PREVIEW, which draws boxes already.  Refused (RT_HIP_UNSUPPORTED, the message names the flag) with
	 * RT_HIP_FLAG_FAST, RT_HIP_FLAG_FORCE_TILED, _FORCE_RESIDENT, _FORCE_STREAMED and RT_HIP_FLAG_FORCE_HALF_CHUNKS, by both
	 * progressive entry points, for more than 256 boxes (a linear scan from LDS; the hierarchy over boxes is RT_HIP_FLAG_BOX_BVH's) and for a frame whose
	 * tables and chunk sums exceed a workgroup's LDS.  Known limit: a ray refracted INTO a box starts on its face, and where its
	 * entry distance comes out as a tiny positive number the 0.001 rule rejects the box and the exit face is not found (the
	 * reference's sphere test has the same weakness).  A library older than this flag refuses the bit (unknown flag bits): that
	 * is how a caller finds out whether it is there. */
	RT_HIP_FLAG_TRACE_BOXES = 1u << 13,
	/* OPT-IN, modifies RT_HIP_FLAG_TRACE_BOXES: the closest-hit query reaches the boxes through a HIERARCHY (a binned-SAH binary tree
	 * over the boxes' extents, built on the host, walked per lane on the sphere hierarchy's LDS stack) instead of the linear scan
	 * from LDS, and the 256-box cap does not apply: the cap is the tree's, 2^26 boxes.  The PROMISE: the frame, the float mean and
	 * `segments` are bit for bit those of the box contract — the same slab arithmetic on every box reached, ties
	 * to the lower index, a box wins a tie against a sphere or a plane, the same face normal; a node is skipped only where no box
	 * inside it can give an accepted distance, which for boxes needs no padding at all.  A ray with a zero,
	 * subnormal or non-finite direction component, or a non-finite origin, scans the boxes linearly instead.  The frame is planned
	 * onto the hierarchy kernel whatever the sphere count (the sphere tree is built as for RT_HIP_FLAG_BVH; zero spheres work):
	 * kernel_variant reports RT_HIP_KERNEL_BVH.  rt_hip_stats is unchanged, box tests stay uncounted.  The tree is built at the
	 * first such frame after the scene's columns changed (counted in `upload_ms`), kept while they stay the same, and freed with
	 * the context.  With n_boxes == 0 it changes nothing at all; ignored with RT_HIP_FLAG_PREVIEW.  Refused (RT_HIP_UNSUPPORTED,
	 * the message names the flag) without RT_HIP_FLAG_TRACE_BOXES, wherever RT_HIP_FLAG_TRACE_BOXES is refused, and by
	 * rt_hip_render_temporal, rt_hip_denoise_progressive and rt_hip_guide_device, whose guide kernel keeps its linear scan.  Nothing
	 * is promised about speed (DESIGN.md §3.10 has the measured table).  A library older than this flag refuses the bit (unknown
	 * flag bits). */
	RT_HIP_FLAG_BOX_BVH = 1u << 14,
	/* (bit 15 stays unassigned, like bit 12: the tests pin 1u << 15 as "unknown flag bits") */
	/* OPT-IN: EMISSIVE MATERIALS — lights.  The reference has no emitters: all its light is the sky gradient.  With this flag a
	 * material whose row of the context's emission table (rt_hip_set_emission: r, g, b per material of the resident scene) has a
	 * component above 0 IS A LIGHT, and a path whose accepted closest hit has such a material ends there with
	 * throughput * emission (component-wise, throughput on the left, as throughput * sky): no random draw, no scatter.  The bounce
	 * check comes first as ever — a path with no bounce left is worth 0 before it can reach a light — and the query, its acceptance
	 * rule and its ties are unchanged.  A light ignores its material's type, albedo, roughness and reflectivity under both scatter
	 * tables and is not sided (a sphere from inside, a plane from behind emit the same).  Everything behind the sample is the
	 * contract's: chunk fold, mean, sqrt, pack — a mean above 1 stays in rgb_f32 and the packed byte clamps.  rt_hip_stats is
	 * unchanged; a segment that ends on a light is counted like any other.  The PROMISE: the frame, the float mean and `segments`
	 * are bit for bit those of the CPU restatement (tests/native/light_reference.cpp); WITHOUT the flag nothing
	 * changes, and with the flag and a table in which no material is a light the frame is the flag-less one in every respect
	 * (plan, kernel, kernel_variant, frame, counters).  A frame with at least one light takes a light build of the resident kernel
	 * (RT_HIP_KERNEL_RESIDENT; scenes of the scalar-register kernel's size too) or, with RT_HIP_FLAG_BVH and for scenes of the
	 * streamed kernel's size, of the hierarchy kernel (RT_HIP_KERNEL_BVH).  Nothing is promised about speed.
	 * Works with RT_HIP_FLAG_SM_MATERIALS, RT_HIP_FLAG_BVH, RT_HIP_FLAG_BVH_DEVICE_BUILD, RT_HIP_FLAG_STATS,
	 * RT_HIP_FLAG_PERSISTENT_FRAME and RT_HIP_FLAG_FORCE_WHOLE_CHUNKS, in rt_hip_render and rt_hip_render_device, with a partition
	 * and on every kind of context; ignored with RT_HIP_FLAG_PREVIEW.  Refused with RT_HIP_INVALID_ARGUMENT when no table is set
	 * or its row count is not the resident scene's n_materials.  Refused (RT_HIP_UNSUPPORTED, the message names the flag) with
	 * RT_HIP_FLAG_FAST, RT_HIP_FLAG_FORCE_TILED, _FORCE_RESIDENT, _FORCE_STREAMED, RT_HIP_FLAG_FORCE_HALF_CHUNKS,
	 * RT_HIP_FLAG_TRACE_BOXES and RT_HIP_FLAG_BOX_BVH, and by both progressive entry points, both adaptive entry points,
	 * rt_hip_render_temporal, rt_hip_denoise_progressive and rt_hip_guide_device.  A library older than this flag refuses the bit
	 * (unknown flag bits): that is how a caller finds out whether it is there. */
	RT_HIP_FLAG_EMISSION = 1u << 16,
	/* DIRECT LIGHT SAMPLING (opt-in): modifies RT_HIP_FLAG_EMISSION — refused without it (RT_HIP_UNSUPPORTED, by
	 * this flag's name) and wherever that flag is refused.  A sphere whose material is a light and whose radius is finite and > 0
	 * is a SAMPLED LIGHT; at most the first 256 of them in sphere order are sampled, every other light (planes, further spheres,
	 * degenerate spheres) counts on hit as under RT_HIP_FLAG_EMISSION alone.  At every hit whose scatter function is lambert (under
	 * the scatter table in force) the path draws ONE more generator step, picks a sampled light and a point on it (an octahedral
	 * map over the hemisphere that faces the vertex, or over the whole sphere from inside), and if the unchanged closest-hit query
	 * from the vertex toward that point returns this very sphere adds throughput * attenuation * emission * weight to the sample;
	 * then the scatter runs as ever.  A sampled light that the NEXT segment of such a vertex hits is worth 0 (the vertex has
	 * accounted for it); after a metal or dielectric vertex, and from the camera, it counts on hit.  A shadow query consumes no
	 * bounce and IS a segment: rt_hip_stats keeps its layout and `segments` counts shadow queries too.  The PROMISE: frame, float
	 * mean and `segments` are bit for bit those of the CPU restatement (tests/native/direct_reference.cpp over
	 * rt_amd/csrc/direct_light_rules.hpp).  With no sampled light the frame is the RT_HIP_FLAG_EMISSION frame in every respect.
	 * THIS IS NOT A LOWER-VARIANCE WAY TO THE RT_HIP_FLAG_EMISSION IMAGE: the contract's lambert scatter draws its directions from
	 * the positive octant (as the reference does), so the light a path finds by running into it is skewed, while the sampled term
	 * is the physically standard one — the two frames converge to DIFFERENT images where a sampled light illuminates lambert
	 * surfaces.  Nothing is promised about speed.  Works wherever RT_HIP_FLAG_EMISSION works; ignored with RT_HIP_FLAG_PREVIEW;
	 * refused by name by both progressive entry points, both adaptive entry points, rt_hip_render_temporal,
	 * rt_hip_denoise_progressive and rt_hip_guide_device.  A library older than this flag refuses the bit (unknown flag bits). */
	RT_HIP_FLAG_DIRECT_LIGHT = 1u << 17,
	/* A THIN-LENS CAMERA (opt-in): depth of field.  Every sample's primary ray starts on a disk of the context's
	 * lens (rt_hip_set_lens: aperture_radius around the eye, in the camera's plane) and passes the point where the pinhole's ray
	 * meets the plane focus_distance along the view direction: what lies on that plane is sharp, everything else is blurred.  The
	 * lens point takes ONE more generator step of the sample's own stream, directly after the jitter step (sample 0 draws no
	 * jitter but does draw the lens step), mapped to the disk by a concentric map with polynomial sine and cosine — no sin, no
	 * cos, no rejection (rt_amd/csrc/lens_rules.hpp).  The reference has no lens: the contract is this module's own, and the
	 * PROMISE is that frame, float mean and `segments` are bit for bit those of the CPU restatement
	 * (tests/native/lens_reference.cpp over the same header).  With aperture_radius == 0 the frame is the flag-less frame in every
	 * respect; with an aperture it is a one-shot frame of the parity arithmetic on the resident kernel (RT_HIP_KERNEL_RESIDENT;
	 * scenes of the scalar-register kernel's size too) or, with RT_HIP_FLAG_BVH and for scenes of the streamed kernel's size, the
	 * hierarchy kernel (RT_HIP_KERNEL_BVH), in whole chunks, without a sky band.  Nothing is promised about speed.
	 * Works with RT_HIP_FLAG_SM_MATERIALS, RT_HIP_FLAG_BVH, RT_HIP_FLAG_BVH_DEVICE_BUILD, RT_HIP_FLAG_STATS,
	 * RT_HIP_FLAG_PERSISTENT_FRAME and RT_HIP_FLAG_FORCE_WHOLE_CHUNKS, in rt_hip_render, rt_hip_render_device,
	 * rt_hip_render_tonemapped and rt_hip_render_bloomed, with a partition and on every kind of context; ignored with
	 * RT_HIP_FLAG_PREVIEW.  Refused with RT_HIP_INVALID_ARGUMENT when no lens is set.  Refused (RT_HIP_UNSUPPORTED, the message
	 * names the flag) for a matrix without a finite eye (a lens needs a perspective matrix), with RT_HIP_FLAG_FAST,
	 * RT_HIP_FLAG_FORCE_TILED, _FORCE_RESIDENT, _FORCE_STREAMED, RT_HIP_FLAG_FORCE_HALF_CHUNKS, RT_HIP_FLAG_TRACE_BOXES,
	 * RT_HIP_FLAG_BOX_BVH, RT_HIP_FLAG_EMISSION and RT_HIP_FLAG_DIRECT_LIGHT, and by both progressive entry points, both adaptive
	 * entry points, rt_hip_render_temporal, rt_hip_render_upscaled and rt_hip_guide_device.  A library older than this flag
	 * refuses the bit (unknown flag bits). */
	RT_HIP_FLAG_THIN_LENS = 1u << 18
};

typedef struct rt_hip_ctx rt_hip_ctx;

/* ---- library ---------------------------------------------------------------------------------------------------- */

RT_HIP_API uint32_t rt_hip_abi_version(void);

/* Message for the most recent failure on the calling thread ("" if none).  Never NULL. */
RT_HIP_API const char* rt_hip_last_error(void);

/* Number of visible HIP devices.  Replaces nothing in the reference (CPU-only). */
RT_HIP_API rt_hip_status rt_hip_device_count(int* count);

/* ---- context ---------------------------------------------------------------------------------------------------- */

/* One context per GPU per renderer instance; owns the device copy of the scene, the stats block and
 * staging buffers.  Mirrors the lifetime of a renderer object in the reference: created by
 * description::create (src/renderer.hpp:39), destroyed through the virtual destructor (src/renderer.hpp:13). */
RT_HIP_API rt_hip_status rt_hip_create(rt_hip_ctx** out_ctx, int device);
RT_HIP_API void rt_hip_destroy(rt_hip_ctx* ctx);

/*
 * One renderer over SEVERAL GPUs of this process — what lets the reference's single blocking
 * render(scene, back_buffer) call (src/renderers/mg_ray_tracer.cpp:178-205; the caller waits in it, src/window.cpp:213-217)
 * use a whole node.  The context owns one member per entry of `devices`; rt_hip_render() on it then
 *   - keeps the scene replicated on every member (each re-uploads only when the host columns changed),
 *   - launches member r's share of the frame — rt_hip_partition{r, n_devices, RT_HIP_DEFAULT_STRIPE_ROWS} — on that
 *     member's own stream, all members concurrently,
 *   - collects the compact stripe buffers on devices[0] with ONE gather over xGMI (RCCL: a communicator per member from
 *     ncclCommInitAll, one ncclGather inside a group call),
 *   - de-interleaves them there and copies the frame to the caller's host buffer once.
 * The frame is bit-identical to the single-GPU one (random streams are keyed by the global pixel index).
 *   devices    device ordinals, rank order; devices[0] is the root.  NULL = 0 .. n_devices-1.
 *   multi_flags RT_HIP_MULTI_*.
 * Every other entry point (rt_hip_scene_upload, rt_hip_render_device, the known-answer calls, ...) used on such a context
 * acts on the root member alone.  n_devices == 1 is allowed and still goes through the communicator.
 */
enum
{
	RT_HIP_MULTI_NONE = 0u,
	/* move the stripes with hipMemcpyPeerAsync instead of RCCL.  RCCL refuses a communicator that names a device twice;
	 * with this flag `devices` may (a one-GPU box can then exercise the whole multi-member path: tests). */
	RT_HIP_MULTI_PEER_COPY = 1u << 0,
	/* no gather: when the caller's back buffer is page-locked (RT_HIP_FLAG_PERSISTENT_FRAME) every member's kernel stores
	 * its pixels straight into their image rows of that buffer, each over its own PCIe link, and rt_hip_render returns when
	 * the last member's launch is done — no stripe buffers, no collective, no de-interleave, no copy.  What a frame of a
	 * few milliseconds wants on 8 GPUs, where gather + assemble + copy cost as much as a member's share of the tracing.
	 * Opt-in: the documented default remains the single RCCL gather.  (Calls without the flag, or that ask for the float
	 * mean, take the gathered way.) */
	RT_HIP_MULTI_DIRECT_FRAME = 1u << 1
};
RT_HIP_API rt_hip_status rt_hip_create_multi(rt_hip_ctx** out_ctx, const int* devices, int n_devices, uint32_t multi_flags);

/*
 * The same renderer with ONE PROCESS PER GPU (how `torchrun` launches a job): every process creates one rank of it.
 *   rt_hip_unique_id   on one process: a fresh RCCL id (rccl.h: ncclGetUniqueId); hand the bytes to every rank by any means
 *                      (the harness broadcasts them with torch.distributed).
 *   rt_hip_create_rank on every process, collectively (rccl.h: ncclCommInitRank): rank `rank` of `world` on `device`.
 * rt_hip_render() on such a context is collective too: every rank passes the same scene, size, seed and flags and renders
 * rt_hip_partition{rank, world, 8}; the stripes are gathered on rank 0 with the same single ncclGather; rank 0 assembles
 * and fills ITS caller's `pixels_rgba8888` (the other ranks may pass NULL and return once their stripes are sent).
 * rgb_f32 must be NULL or non-NULL on all ranks alike.  Nothing in the reference corresponds (it is one process).
 */
#define RT_HIP_UNIQUE_ID_BYTES 128
RT_HIP_API rt_hip_status rt_hip_unique_id(char out_id[RT_HIP_UNIQUE_ID_BYTES]);
RT_HIP_API rt_hip_status rt_hip_create_rank(rt_hip_ctx** out_ctx, int device, int rank, int world, const char id[RT_HIP_UNIQUE_ID_BYTES]);
/*
 * rt_hip_create_rank in two halves, so that the part that can fail on ONE rank alone — no such device, not a gfx950, out
 * of memory — is over before anything collective starts (a rank that fails inside rt_hip_create_rank leaves the others
 * waiting in ncclCommInitRank):
 *   1. every process: rt_hip_create(&ctx, device)                                — local, may fail alone
 *   2. the launcher lets the ranks agree that all of them hold a context (bench.py: one all_reduce), and only then
 *   3. every process: rt_hip_join_ranks(ctx, rank, world, id, timeout_ms)        — collective (rccl.h: ncclCommInitRank)
 * rt_hip_join_ranks waits at most `timeout_ms` milliseconds for the communicator (0 = RT_HIP_JOIN_TIMEOUT_MS from the
 * environment, else 120 000) and then gives up with RT_HIP_TIMEOUT; the context stays a valid single-GPU context, which the
 * caller may use or destroy.  On success the context is what rt_hip_create_rank returns.
 */
RT_HIP_API rt_hip_status rt_hip_join_ranks(rt_hip_ctx* ctx, int rank, int world, const char id[RT_HIP_UNIQUE_ID_BYTES], uint32_t timeout_ms);

/*
 * ONE PROCESS PER GPU WITHOUT AN EXCHANGE STEP — what RT_HIP_MULTI_DIRECT_FRAME is for one process, for `torchrun`-style
 * jobs.  The caller's back buffer is a SHARED mapping (shm_open / memfd + mmap(MAP_SHARED)) that every rank's process
 * maps; each rank page-locks its own mapping and its kernel stores the rank's stripes straight into their image rows,
 * over that GPU's own PCIe link, while the frame is still being traced.  No RCCL, no stripe buffers, no assemble, no
 * copy: the gathered form puts 7/8 of an 8-GPU frame through rank 0's single PCIe link AFTER the tracing (0.14 ms for a
 * 1080p frame whose tracing takes 0.36 ms per rank).  The ranks meet in a control block in POSIX shared memory
 * (rt_amd/csrc/frame_group.hpp) twice per frame — "everybody is in the call", "everybody's stripes are in place".
 *   rt_hip_join_frame_group(ctx, rank, world, name, timeout_ms) on a context from rt_hip_create, on every process,
 *       collectively.  `name` is a fresh shm_open name ("/rt_hip_<something unique>") all ranks were handed by any means;
 *       rank 0 creates the object, the others wait for it; when all have mapped it the name is removed again.  Waits at
 *       most timeout_ms (0 = RT_HIP_JOIN_TIMEOUT_MS, else 120 000) -> RT_HIP_TIMEOUT; the context then stays a plain one.
 *   rt_hip_render(ctx, scene, pixels, ...) on EVERY rank, with the same scene, size, seed and flags and with `pixels` =
 *       that process's mapping of the one shared buffer (the library checks all of this: a rank called with other
 *       arguments, or whose `pixels` is not the memory rank 0 renders into, fails the frame on every rank).  Returns on
 *       every rank when the WHOLE frame is in the buffer.  RT_HIP_FLAG_PERSISTENT_FRAME is implied; rgb_f32 must be NULL.
 *       `stats` / rt_hip_stats_fetch give the whole frame (counts summed over the ranks, the slowest rank's kernel time;
 *       a rank that was called without `stats` and without RT_HIP_FLAG_STATS contributes zeros),
 *       rt_hip_member_stats(ctx, r, ..) / rt_hip_member_device(ctx, r, ..) rank r's share and device, for any r < world.
 * A rank that fails, leaves (rt_hip_destroy) or stays away longer than RT_HIP_GROUP_DEADLINE_MS (default 120 000) breaks
 * the group: every rank's current and later rt_hip_render returns an error naming the rank and the reason; the renderer
 * is then destroyed and made anew.  Nothing in the reference corresponds (it is one process, one thread pool).
 */
RT_HIP_API rt_hip_status rt_hip_join_frame_group(rt_hip_ctx* ctx, int rank, int world, const char* name, uint32_t timeout_ms);

/* How the stripes of a multi-GPU frame reach the root: what a context was created with (and what a bench line should say). */
enum
{
	RT_HIP_TRANSPORT_NONE		  = 0, /* one GPU: nothing to exchange */
	RT_HIP_TRANSPORT_RCCL_GATHER  = 1, /* one ncclGather to rank 0 */
	RT_HIP_TRANSPORT_PEER_COPY	  = 2, /* RT_HIP_MULTI_PEER_COPY: hipMemcpyPeerAsync into the root */
	RT_HIP_TRANSPORT_DIRECT_FRAME = 3, /* RT_HIP_MULTI_DIRECT_FRAME took effect in the most recent frame: no exchange at all */
	RT_HIP_TRANSPORT_SHARED_FRAME = 4  /* rt_hip_join_frame_group: every rank's process stores into ONE shared back buffer */
};
/* What member `member` of the context talks through, as RCCL itself reports it (rccl.h: ncclCommCount, ncclCommUserRank,
 * ncclCommCuDevice): the communicator's size, this member's rank in it, and the device the communicator lives on.  Contexts
 * without a communicator (one GPU, peer copies) report the context's own world / rank / device.  Any out pointer may be NULL. */
RT_HIP_API rt_hip_status rt_hip_comm_info(const rt_hip_ctx* ctx, int member, int* out_ranks, int* out_rank, int* out_device, uint32_t* out_transport);

/* number of members of a context (1 for rt_hip_create) and the device of member `rank` */
RT_HIP_API rt_hip_status rt_hip_member_count(const rt_hip_ctx* ctx, int* out_count);
RT_HIP_API rt_hip_status rt_hip_member_device(const rt_hip_ctx* ctx, int rank, int* out_device);
/* counters of member `rank`'s share of the most recent rt_hip_render (rt_hip_stats_fetch on a multi context returns the
 * whole frame: counts summed, render_ms = the slowest member) */
RT_HIP_API rt_hip_status rt_hip_member_stats(rt_hip_ctx* ctx, int rank, rt_hip_stats* out_stats);

/* ---- partition helpers (pure host arithmetic; usable without a GPU) ------------------------------------------- */

/* Rows of an H-row image owned by part->rank. */
RT_HIP_API rt_hip_status rt_hip_local_rows(uint32_t height, const rt_hip_partition* part, uint32_t* out_rows);
/* max over ranks of rt_hip_local_rows: the per-rank buffer height used for the equal-sized gather. */
RT_HIP_API rt_hip_status rt_hip_padded_local_rows(uint32_t height, const rt_hip_partition* part, uint32_t* out_rows);

/*
 * What rt_hip_render does with the caller's columns before anything touches a GPU, on its own (pure host code; usable
 * without a device): the pointer / count check, the material-index check (the reference's loader refuses out-of-range
 * indices, src/scene.cpp:568-574) and the fingerprint that decides whether the columns resident in HBM are still the
 * caller's (rt has no scene version counter, src/main.cpp:233-311).  Reads exactly n_* rows of every column — never the
 * padding rows soagen keeps behind size() (vendor/soagen.hpp:3777,7075-7082).  out_fingerprint may be NULL.
 */
RT_HIP_API rt_hip_status rt_hip_scene_check(const rt_hip_scene* scene, uint64_t* out_fingerprint);

/* ---- the hot path ----------------------------------------------------------------------------------------------- */

/* Copy the scene columns to HBM (once per scene/camera change).  The reference has no scene version
 * counter (src/main.cpp:233-311), so rt_hip_render() calls this every frame; a caller that knows the
 * scene is unchanged keeps it resident and calls rt_hip_render_device() only. */
RT_HIP_API rt_hip_status rt_hip_scene_upload(rt_hip_ctx* ctx, const rt_hip_scene* scene);

/*
 * Render this rank's stripes of a width x height frame from the resident scene.
 *   d_rgba8   DEVICE buffer, padded_local_rows x width uint32, receives RGBA8888 packed exactly as
 *             rt::colour::operator uint32_t (src/colour.hpp:101-106); row-major, no pitch (src/image.hpp:143-147).
 *   d_rgb_f32 optional DEVICE buffer, padded_local_rows x width x 3 floats: the per-pixel mean radiance
 *             before the sqrt "gamma" (mg_ray_tracer.cpp:195), for float-level parity checks.  May be NULL.
 *   seed      key of the counter-based random streams (the reference seeds from std::random_device,
 *             src/random.cpp:12-13, and is not reproducible).
 *   stream    hipStream_t to launch on (NULL = the default stream).  Asynchronous: returns after enqueue.
 */
RT_HIP_API rt_hip_status rt_hip_render_device(rt_hip_ctx* ctx,
								   uint32_t width,
								   uint32_t height,
								   uint64_t seed,
								   uint32_t flags,
								   const rt_hip_partition* part, /* NULL = whole image */
								   uint32_t* d_rgba8,
								   float* d_rgb_f32,
								   void* stream);

/* Rank 0, after the gather: de-interleave `world` compact per-rank buffers (each padded_local_rows x width,
 * concatenated in rank order) into the width x height frame.  Device to device, asynchronous on `stream`. */
RT_HIP_API rt_hip_status rt_hip_assemble_device(rt_hip_ctx* ctx,
									 uint32_t width,
									 uint32_t height,
									 uint32_t world,
									 uint32_t stripe_rows,
									 const uint32_t* d_gathered,
									 uint32_t* d_frame,
									 void* stream);

/* Synchronise with the last render on this context and read its counters. */
RT_HIP_API rt_hip_status rt_hip_stats_fetch(rt_hip_ctx* ctx, rt_hip_stats* out_stats);

/*
 * Where the time of the most recent rt_hip_render went (frames rendered with `stats` or RT_HIP_FLAG_STATS; otherwise the
 * device times are 0).  Device times come from HIP events on the root's stream; on one GPU only render_ms is non-zero.
 * Nothing in the reference corresponds: it prints no timing at all (src/main.cpp:30-47).
 */
typedef struct rt_hip_phases
{
	float render_ms;	 /* the root member's kernel (its share of the frame) */
	float gather_ms;	 /* end of the root's kernel -> every rank's stripes are on the root (waits for the slowest rank) */
	float assemble_ms;	 /* de-interleave; with a page-locked back buffer this IS the transfer to the host (stores over PCIe) */
	float copy_ms;		 /* device-to-host copy of the assembled frame (0 when it was assembled straight into the back buffer) */
	float host_issue_ms; /* host wall time from entry into rt_hip_render until everything was enqueued */
	float host_wait_ms;	 /* host wall time blocked until the frame was complete */
	uint32_t transport;	 /* RT_HIP_TRANSPORT_* that this frame took */
	uint32_t scene_resident; /* 1: the columns' fingerprint matched, nothing was uploaded */
	/* ABI 6.  The default frame mode (module-owned page-locked frame + host carrier threads): how the frame reached the caller's
	 * buffer.  carrier_bands = 64 KB bands the frame was carried in (0: the kernels stored straight into the caller's page-locked
	 * buffer, or a multi-GPU / preview path); carrier_bands_early = of those, carried over BEFORE the stream had drained — by
	 * the helper threads, while the frame was being traced; carrier_helpers = helper threads the context runs (0: the caller's own
	 * thread carries everything after the kernel).  A frame whose carrier_bands_early is 0 although carrier_helpers is not was
	 * carried by the caller's thread alone: the helpers never got to run (frame delivery). */
	uint32_t carrier_bands;
	uint32_t carrier_bands_early;
	uint32_t carrier_helpers;
} rt_hip_phases;
RT_HIP_API rt_hip_status rt_hip_phases_fetch(rt_hip_ctx* ctx, rt_hip_phases* out_phases);

/*
 * The drop-in for renderer_interface::render(const scene&, image_view&, muu::thread_pool&)
 * (src/renderer.hpp:11; mg_ray_tracer.cpp:178): upload `scene`, render the whole frame on the context's
 * GPU, and copy it into the caller's HOST pixel buffer (image_view::data(), width*height uint32) before
 * returning — the caller presents it immediately (src/window.cpp:215-216).
 *   rgb_f32  optional HOST buffer of 3*width*height floats (pre-gamma mean), may be NULL.
 *   stats    optional, may be NULL.
 */
RT_HIP_API rt_hip_status rt_hip_render(rt_hip_ctx* ctx,
							const rt_hip_scene* scene,
							uint32_t* pixels_rgba8888,
							uint32_t width,
							uint32_t height,
							uint64_t seed,
							uint32_t flags,
							float* rgb_f32,
							rt_hip_stats* stats);

/* ---- progressive frames: resumable sample passes ------------------------------------------------------------------ */
/*
 * A frame in PASSES: every call traces the next run of samples of every pixel and leaves the frame as it then stands, so that a
 * caller sees a noisy frame at once and watches it converge while the camera rests.  The arithmetic contract makes this exact
 * (DESIGN.md §3.6): a pixel's value is the fold, in chunk order, of sums of 16 consecutive samples, and a sample's random window
 * does not depend on the sample count — so the frame after samples [0, s) is, BIT FOR BIT, the one-shot frame of the same scene
 * at samples_per_pixel = s, and the frame after the last pass is rt_hip_render's.  A pixel's running sum lives between passes
 * in an accumulator of 3 floats per pixel.
 * Additions to ABI 6 (RT_HIP_ABI_VERSION stays 6): a caller that may meet an older library looks them up with dlsym.
 * Both entry points take RT_HIP_FLAG_NONE, RT_HIP_FLAG_SM_MATERIALS, RT_HIP_FLAG_BVH, RT_HIP_FLAG_BVH_DEVICE_BUILD and
 * RT_HIP_FLAG_STATS (the device level keeps its counters anyway, as rt_hip_render_device does) and refuse every other flag with RT_HIP_UNSUPPORTED and a message that
 * names it: passes are built for the parity contract's tile-per-wave kernels only.  kernel_variant is RT_HIP_KERNEL_RESIDENT,
 * or RT_HIP_KERNEL_BVH — with RT_HIP_FLAG_BVH, and for every scene of the streamed kernel's size (above about 1300 primitives)
 * with or without the flag.  samples_per_pixel may be anything up to 2^20 (beyond that the samples' windows alias): rt_hip_render's
 * limit of 4096 applies to ONE PASS, not to the frame; a pass that is too large is refused with RT_HIP_UNSUPPORTED — so is a pass
 * through the hierarchy whose stacks and chunk sums the device does not give one workgroup the LDS for (RT_HIP_FLAG_BVH above).
 * What passes cost next to the one-shot frame through the same kernel (per pass: a launch, 12 bytes per pixel read and
 * written, the per-pixel finish): DESIGN.md §3.6 says what has been measured (tools/progressive_bench.py); nothing here
 * promises more than it says.
 */
typedef struct rt_hip_progress
{
	uint32_t samples_done;	/* samples per pixel the delivered frame holds */
	uint32_t samples_total; /* the scene's samples_per_pixel */
	uint32_t passes;		/* passes launched for this accumulation so far */
	uint32_t restarted;		/* 1: this call started a new accumulation (the first call, or something the frame depends on changed) */
} rt_hip_progress;

/*
 * Device level: samples [first_sample, first_sample + n_samples) of the resident scene, folded onto d_accum; d_rgba8 (and
 * d_rgb_f32, optional) receive the frame at first_sample + n_samples samples per pixel.  Buffers, partition, seed and stream as
 * for rt_hip_render_device (streams are keyed by the global pixel).
 *   first_sample  a multiple of 16 (else RT_HIP_INVALID_ARGUMENT).  0 starts an accumulation: d_accum is not read, and need not
 *                 be cleared.
 *   n_samples     a multiple of 16, or whatever reaches the scene's samples_per_pixel (the last pass)
 *   d_accum       DEVICE buffer, padded_local_rows x width x 3 floats, the caller's to keep from pass to pass: pass k must find
 *                 what pass k-1 of the same scene, size, seed, partition and flags left
 */
RT_HIP_API rt_hip_status rt_hip_render_pass_device(rt_hip_ctx* ctx,
										uint32_t width,
										uint32_t height,
										uint64_t seed,
										uint32_t flags,
										const rt_hip_partition* part, /* NULL = whole image */
										uint32_t first_sample,
										uint32_t n_samples,
										float* d_accum,
										uint32_t* d_rgba8,
										float* d_rgb_f32,
										void* stream);

/*
 * Drop-in level: rt_hip_render in passes.  Every call traces the next pass_samples samples (rounded up to a multiple of 16,
 * clamped to what is left; 0 = all that is left) of the accumulation in flight and fills `pixels_rgba8888` (and rgb_f32) with
 * the frame as it then stands — or starts a new accumulation, if anything the frame depends on differs from the call before:
 * the columns' fingerprint, samples_per_pixel, max_bounces, the matrix, the size, the seed, RT_HIP_FLAG_SM_MATERIALS.  (A
 * caller keeps the seed constant while the camera rests.)  The accumulator belongs to the context: 12 bytes per pixel, grown
 * on demand, freed with it.  The frame travels as in rt_hip_render without RT_HIP_FLAG_PERSISTENT_FRAME: the caller's
 * buffer is plain memory and may be another one on every call.
 *   A call on a FINISHED accumulation launches nothing: it delivers the finished frame again, leaves `passes` as it was, and
 *   reports stats of zero work (primary_samples = segments = 0, render_ms = 0, kernel_variant = RT_HIP_KERNEL_NONE).
 *   stats         optional: THIS PASS — primary_samples = pixels x the pass's samples, segments = the pass's; summed over the
 *                 passes of a frame they are the one-shot frame's.
 *   out_progress  optional.
 * Contexts from rt_hip_create only: multi-GPU, rank and frame-group contexts return RT_HIP_UNSUPPORTED.
 */
RT_HIP_API rt_hip_status rt_hip_render_progressive(rt_hip_ctx* ctx,
										const rt_hip_scene* scene,
										uint32_t* pixels_rgba8888,
										uint32_t width,
										uint32_t height,
										uint64_t seed,
										uint32_t flags,
										uint32_t pass_samples,
										float* rgb_f32,
										rt_hip_stats* stats,
										rt_hip_progress* out_progress);

/* ---- denoising low-sample frames: first-hit guide buffers and an edge-avoiding a-trous filter ---------------------------- */
/*
 * The first passes of a progressive frame are raw Monte-Carlo noise.  These entry points smooth such a frame without blurring
 * across what the scene itself says is an edge: a GUIDE of the resident scene (first-hit normal, depth, albedo and primitive of
 * every pixel, from the path tracer's own sample-0 primary ray) steers a 5 x 5 B3-spline a-trous wavelet filter, one launch per
 * iteration with taps 2^i pixels apart.  The filter is a contract of its own: + - x, correctly rounded division
 * and compare-and-select in a fixed order, so that the device's result equals a serial CPU restatement bit for bit — it is NOT
 * the reference's arithmetic (the reference has no denoiser), and a filtered frame is no path tracer's frame.
 * Additions to ABI 6 (RT_HIP_ABI_VERSION stays 6): a caller that may meet an older library looks them up with dlsym.
 */
typedef struct rt_hip_denoise_params
{
	uint32_t iterations;	   /* 0 .. 6; 0 = pass-through */
	uint32_t normal_squarings; /* 0 .. 8: the normal term is max(0, n_p . n_q) squared this many times */
	float sigma_colour;		   /* width of the colour term at iteration 0; halved with every iteration */
	float sigma_albedo;		   /* width of the albedo term */
	float sigma_depth;		   /* width of the depth term, relative to the deeper of the two hits */
} rt_hip_denoise_params;

/* the defaults a NULL `params` stands for (DESIGN.md §3.8 has the table they were chosen from); pure host code */
RT_HIP_API rt_hip_status rt_hip_denoise_default_params(rt_hip_denoise_params* out_params);

/*
 * The guide of the resident scene for a whole width x height frame: 8 words per pixel, row-major —
 *   nx, ny, nz, depth | ar, ag, ab, id
 * the hit normal as the tracer computes it (0, 0, 0 for sky), the hit distance (-1 for sky), the attenuation the tracer uses
 * for the hit (the sky colour of the ray for a miss), and as uint32 bits 0 for sky or 1 + the primitive's index counted
 * spheres first, then planes, then boxes.  d_guide: DEVICE buffer of 8 * width * height floats, 16-byte aligned.  Asynchronous on `stream`.
 * Flags: RT_HIP_FLAG_TRACE_BOXES makes the ray hit the scene's boxes too (at most 256, as for a frame); RT_HIP_FLAG_SM_MATERIALS,
 * RT_HIP_FLAG_BVH, RT_HIP_FLAG_BVH_DEVICE_BUILD and RT_HIP_FLAG_STATS are accepted and change nothing; every other flag is
 * refused with RT_HIP_UNSUPPORTED and its name.  On a multi-GPU, rank or frame-group context the root member answers.
 */
RT_HIP_API rt_hip_status rt_hip_guide_device(rt_hip_ctx* ctx, uint32_t width, uint32_t height, uint32_t flags, float* d_guide, void* stream);

/*
 * The filter, a pure image operation on DEVICE buffers: d_rgb_in (3 * width * height floats, a frame's float mean) and d_guide
 * (rt_hip_guide_device's) give d_rgb_out (3 * width * height floats, optional) and d_rgba8_out (width * height packed pixels:
 * square root, clamp and pack as rt_hip_render finishes a pixel; optional) — not both NULL.  d_rgb_out must not overlap d_rgb_in.
 * params == NULL: the defaults.  With iterations == 0 d_rgb_out is d_rgb_in bit for bit and d_rgba8_out is what rt_hip_render
 * packs from that mean.  Between iterations the image lives in two scratch images of the context (12 bytes per pixel each, grown on
 * demand, freed with it): two calls on one context must not run at the same time on different streams.  Asynchronous on `stream`.
 */
RT_HIP_API rt_hip_status rt_hip_denoise_device(rt_hip_ctx* ctx,
									uint32_t width,
									uint32_t height,
									const float* d_rgb_in,
									const float* d_guide,
									const rt_hip_denoise_params* params, /* NULL = defaults */
									float* d_rgb_out,					 /* nullable */
									uint32_t* d_rgba8_out,				 /* nullable, not both NULL */
									void* stream);

/*
 * The accumulation in flight of rt_hip_render_progressive, denoised: mean = accumulator / samples_done, the guide of the
 * accumulation's own matrix, size and flags (built once per accumulation and kept), the filter, and the result copied into the
 * caller's plain HOST memory: pixels_rgba8888 (width * height) and, optionally, rgb_f32 (3 * width * height floats).  The float
 * frame never crosses the bus on its way in.  Works after any successful rt_hip_render_progressive call, finished or not, and
 * leaves the accumulation alone: the next pass continues as if the call had not happened.  render_ms (optional): device time of
 * guide + filter.  RT_HIP_INVALID_ARGUMENT ("no accumulation in flight") where there is none; contexts from rt_hip_create only.
 */
RT_HIP_API rt_hip_status rt_hip_denoise_progressive(rt_hip_ctx* ctx, const rt_hip_denoise_params* params, uint32_t* pixels_rgba8888, float* rgb_f32, float* render_ms);

/* ---- temporal accumulation: accumulated frames kept across camera moves ------------------------------------------------- */
/*
 * rt_hip_render_progressive starts again whenever the matrix changes: while the camera moves, every frame is a fresh low-sample
 * frame.  These entry points carry the samples already traced across a move instead.  For every pixel of the current frame the
 * first hit's world position (from the guide) is projected through the PREVIOUS frame's view-projection, the history accumulated
 * there is fetched with four bilinear taps, each tap is checked to be the same surface (primitive id, normal, world position), and
 * the history is blended with the current frame's mean in proportion to the samples each stands for, the history's share capped.
 * A contract of its own: + - x, correctly rounded division, explicit fma and compare-and-select in a fixed order,
 * so that the device's result equals a serial CPU restatement bit for bit — it is NOT the reference's arithmetic (the reference
 * drops to its preview while the camera moves), and a blended frame is no path tracer's frame.  Known limits: the FIRST hit alone
 * decides validity, so what is seen IN a metal or glass surface lags behind the camera until the cap washes it out; sky pixels
 * keep no history; the history is a mean with a cap, not a variance-aware filter.
 * Additions to ABI 6 (RT_HIP_ABI_VERSION stays 6): a caller that may meet an older library looks them up with dlsym.
 */
typedef struct rt_hip_temporal_params
{
	uint32_t max_history_samples; /* 1 .. 2^20: the most samples a pixel's history may count for in a blend */
	float position_tolerance;	  /* > 0: a tap is the same surface if it lies within this x the hit distance of the pixel's point */
	float normal_threshold;		  /* -1 .. 1: ... and its normal's dot product with the pixel's is at least this */
} rt_hip_temporal_params;

/* the defaults a NULL `params` stands for (DESIGN.md §3.9 has the table they were chosen from); pure host code */
RT_HIP_API rt_hip_status rt_hip_temporal_default_params(rt_hip_temporal_params* out_params);

/*
 * One reprojection step on DEVICE buffers.  The current camera is the RESIDENT scene's (as for rt_hip_guide_device): d_guide is
 * that call's output for this size, d_rgb_in the current frame's float mean, standing for samples_in (1 .. 4096) samples per pixel.
 * The history is two buffers a previous call wrote — d_prev_rgb (3 words per pixel: the blended mean, never a filtered one) and
 * d_prev_record (8 words per pixel, 16-byte aligned: px py pz length | nx ny nz id) — made under prev_inverse_view_projection (HOST,
 * 16 floats); both NULL: no history (the matrix is then not read).  Outputs: d_rgb_out and d_record_out (16-byte aligned), which
 * must not overlap any input, and optionally the number of pixels that found history (one word, overwritten).  A singular or
 * non-finite previous matrix is refused with RT_HIP_INVALID_ARGUMENT.  Asynchronous on `stream`; on a multi-GPU, rank or
 * frame-group context the root member answers.
 */
RT_HIP_API rt_hip_status rt_hip_reproject_device(rt_hip_ctx* ctx,
									uint32_t width,
									uint32_t height,
									const float prev_inverse_view_projection[16],
									const float* d_guide,
									const float* d_rgb_in,
									uint32_t samples_in,
									const float* d_prev_rgb,	 /* nullable, with d_prev_record */
									const float* d_prev_record,
									const rt_hip_temporal_params* params, /* NULL = defaults */
									float* d_rgb_out,
									float* d_record_out,
									uint32_t* d_pixels_with_history, /* nullable */
									void* stream);

typedef struct rt_hip_temporal_info
{
	uint32_t frames;			  /* frames blended into this history so far */
	uint32_t restarted;			  /* 1: this call started a new history */
	uint32_t pixels_with_history; /* pixels of this frame that found history */
	uint32_t pixels;			  /* width x height */
} rt_hip_temporal_info;

/*
 * Drop-in level: one call is one frame.  The scene is uploaded by fingerprint as in rt_hip_render; the one-shot frame of
 * samples_per_pixel (1 .. 4096) samples is traced into a device float mean by the launch rt_hip_render_device makes; its guide is
 * built; the mean is blended with the context's history (two sets of 44 bytes per pixel, ping-pong, grown on demand, freed with the
 * context); with `filter` the a-trous filter of rt_hip_denoise_device runs on the blended mean (its output never enters the
 * history); the result is packed as rt_hip_render packs and copied into the caller's plain HOST memory.
 *   seed      pass a NEW seed every frame: the same seed twice traces the same samples and adds no information.
 *   The history starts again on any change of the columns' fingerprint, max_bounces, the size, RT_HIP_FLAG_SM_MATERIALS or
 *   RT_HIP_FLAG_TRACE_BOXES — and not on a change of the matrix, the seed or samples_per_pixel.  It is state of its own: a
 *   progressive accumulation in flight, the denoiser's kept guide and rt_hip_render's frames are left alone.
 *   stats     optional: the traced frame; render_ms additionally holds guide, reprojection and filter.
 * Flags: RT_HIP_FLAG_SM_MATERIALS, RT_HIP_FLAG_BVH, RT_HIP_FLAG_BVH_DEVICE_BUILD, RT_HIP_FLAG_TRACE_BOXES and RT_HIP_FLAG_STATS;
 * every other flag is refused with RT_HIP_UNSUPPORTED and its name.  Contexts from rt_hip_create only.
 */
RT_HIP_API rt_hip_status rt_hip_render_temporal(rt_hip_ctx* ctx,
									const rt_hip_scene* scene,
									uint32_t* pixels_rgba8888,
									uint32_t width,
									uint32_t height,
									uint64_t seed,
									uint32_t flags,
									const rt_hip_temporal_params* temporal, /* NULL = defaults */
									const rt_hip_denoise_params* filter,	/* NULL = no spatial filter */
									float* rgb_f32,							/* nullable */
									rt_hip_stats* stats,
									rt_hip_temporal_info* out_info);

/* ---- guided upsampling: trace a smaller frame, rebuild the full one ------------------------------------------------------- */
/*
 * Every entry point above traces every pixel of the full-size frame.  These trace FEWER PIXELS: a low frame of w x h pixels seen
 * through the same matrix covers exactly the view of the W x H frame (the NDC mapping depends on the size through 2 / width and
 * 2 / height alone), and a joint-bilateral kernel rebuilds the full frame from it: every full pixel takes its four bilinear low
 * taps, each weighted by how well the low guide record of the tap agrees with the FULL guide record of the pixel (normal, depth,
 * albedo: the denoiser's terms), so that a silhouette of the full frame stays a silhouette.  A full pixel none of whose taps saw
 * its surface — a thin sphere, a silhouette sliver — is an ORPHAN: it takes the plain bilinear mean and is counted; orphans are the
 * known limit of the method, they are reported, not re-traced.  A contract of its own: exact integer geometry,
 * + - x, correctly rounded division and compare-and-select in a fixed order, so that the device's result equals a serial CPU
 * restatement bit for bit — it is NOT the reference's arithmetic (the reference has no upsampler), and a rebuilt frame is no path
 * tracer's frame.  No speed and no quality is promised.
 * Additions to ABI 6 (RT_HIP_ABI_VERSION stays 6): a caller that may meet an older library looks them up with dlsym.
 */
typedef struct rt_hip_upsample_params
{
	uint32_t normal_squarings; /* 0 .. 8: the normal term is max(0, n_p . n_q) squared this many times */
	float sigma_albedo;		   /* > 0: width of the albedo term */
	float sigma_depth;		   /* > 0: width of the depth term, relative to the deeper of the two hits */
	float min_weight;		   /* (0, 1]: a pixel whose guided weights sum to less is an orphan */
} rt_hip_upsample_params;

/* the defaults a NULL `params` stands for (DESIGN.md §3.14 has the table min_weight was chosen from); pure host code */
RT_HIP_API rt_hip_status rt_hip_upsample_default_params(rt_hip_upsample_params* out_params);

/* the low frame rt_hip_render_upscaled traces for `factor` (1 .. 4): ceil(width / factor) x ceil(height / factor); pure host code */
RT_HIP_API rt_hip_status rt_hip_upsample_low_size(uint32_t width, uint32_t height, uint32_t factor, uint32_t* out_low_width, uint32_t* out_low_height);

/*
 * The reconstruction, a pure image operation on DEVICE buffers: d_rgb_low (3 * low_width * low_height floats, a low frame's float
 * mean), d_guide_low and d_guide_full (rt_hip_guide_device's records at the two sizes, 16-byte aligned) give d_rgb_out
 * (3 * width * height floats, optional) and d_rgba8_out (width * height packed pixels: square root, clamp and pack as
 * rt_hip_render finishes a pixel; optional) — not both NULL — and, optionally, the number of orphans (one word, overwritten).
 * 1 <= low_width <= width <= 2^22, likewise the heights; the two sizes need not be in a whole ratio.  No output may overlap an
 * input or another output.  params == NULL: the defaults.  It reads no scene: any buffers of the right shape will do.
 * Asynchronous on `stream`; on a multi-GPU, rank or frame-group context the root member answers.
 */
RT_HIP_API rt_hip_status rt_hip_upsample_device(rt_hip_ctx* ctx,
									uint32_t width,
									uint32_t height,
									uint32_t low_width,
									uint32_t low_height,
									const float* d_rgb_low,
									const float* d_guide_low,
									const float* d_guide_full,
									const rt_hip_upsample_params* params, /* NULL = defaults */
									float* d_rgb_out,					  /* nullable */
									uint32_t* d_rgba8_out,				  /* nullable, not both NULL */
									uint32_t* d_orphans,				  /* nullable */
									void* stream);

typedef struct rt_hip_upscale_info
{
	uint32_t low_width, low_height; /* the traced frame */
	uint32_t orphans;				/* full pixels that fell back to the plain bilinear mean */
	uint32_t pixels;				/* width x height */
} rt_hip_upscale_info;

/*
 * Drop-in level: one call is one frame.  The scene is uploaded by fingerprint as in rt_hip_render; the one-shot frame is traced at
 * ceil(width / factor) x ceil(height / factor) with the scene's own matrix, seed and samples into a device float mean, by the
 * launch rt_hip_render_device makes; the guide is built at the low and at the full size; with `filter` the a-trous filter of
 * rt_hip_denoise_device runs on the LOW mean with the low guide; the full frame is rebuilt, packed as rt_hip_render packs, and
 * copied into the caller's plain HOST memory: pixels_rgba8888 (width * height) and, optionally, rgb_f32 (3 * width * height).
 * The scratch (low mean, two guides, full outputs) belongs to the context, is grown on demand and freed with it.  It is state of
 * its own: a progressive accumulation in flight, the temporal history and the denoiser's kept guide are left alone.
 *   factor    2 .. 4
 *   stats     optional: the traced LOW frame's (primary_samples = low_width x low_height x samples_per_pixel); render_ms
 *             additionally holds guides, filter and upsampling.
 * Flags: RT_HIP_FLAG_SM_MATERIALS, RT_HIP_FLAG_BVH, RT_HIP_FLAG_BVH_DEVICE_BUILD, RT_HIP_FLAG_TRACE_BOXES and RT_HIP_FLAG_STATS;
 * every other flag is refused with RT_HIP_UNSUPPORTED and its name.  Contexts from rt_hip_create only.
 */
RT_HIP_API rt_hip_status rt_hip_render_upscaled(rt_hip_ctx* ctx,
									const rt_hip_scene* scene,
									uint32_t* pixels_rgba8888,
									uint32_t width,
									uint32_t height,
									uint64_t seed,
									uint32_t flags,
									uint32_t factor,
									const rt_hip_upsample_params* upsample, /* NULL = defaults */
									const rt_hip_denoise_params* filter,	/* NULL = no filter on the low frame */
									float* rgb_f32,							/* nullable */
									rt_hip_stats* stats,
									rt_hip_upscale_info* out_info);

/* ---- adaptive sampling: passes that stop converged pixels ---------------------------------------------------------------- */
/*
 * rt_hip_render_progressive gives every pixel the same number of samples.  An ADAPTIVE accumulation is a progressive accumulation
 * whose passes trace the pixels that are still ACTIVE only: after every whole pass each active pixel's luminance statistics over
 * its passes are updated, and a pixel STOPS once it and its eight neighbours inside the frame have converged (standard error of
 * the passes' mean luminance within threshold x (mean + floor), at least min_samples samples, at least two passes).  A stopped
 * pixel is never traced again; the accumulation is complete when no pixel is active or the cap — the scene's samples_per_pixel,
 * at most 2^20 — is reached.  The last pass traces what is left up to the cap; a short one counts its samples and judges nobody.
 * THE PROMISE: pixel (x, y) of the float mean and of the packed frame is, BIT FOR BIT, the one-shot frame's
 * pixel at samples_per_pixel = n(x, y), where n is the sample map the call returns — a pixel's value is a left fold over 16-sample
 * chunk sums and a sample's random window does not depend on the sample count, per pixel as per frame.  The stop rule itself is a
 * contract of its own (+ - x, correctly rounded division, compare-and-select in a fixed order, a NaN never converges): the device's
 * decisions equal a serial CPU restatement bit for bit.  It is NOT the reference's (the reference has no adaptive sampling).
 * KNOWN LIMIT: a feature that a pixel's first min_samples samples never found is not found later either — the usual bias of
 * variance-driven stopping; the 3 x 3 condition narrows it around silhouettes and does not remove it.
 * The defaults were taken from a CPU simulation on oracle frames, not from a GPU run; DESIGN.md §3.11 says what has been measured
 * on the device, and nothing here promises a speed-up beyond what it says.
 * Additions to ABI 6 (RT_HIP_ABI_VERSION stays 6): a caller that may meet an older library looks them up with dlsym.
 * Flags: those of the passes — RT_HIP_FLAG_SM_MATERIALS, RT_HIP_FLAG_BVH, RT_HIP_FLAG_BVH_DEVICE_BUILD, RT_HIP_FLAG_STATS; every
 * other flag (RT_HIP_FLAG_FAST and the box flags among them) is refused with RT_HIP_UNSUPPORTED and its name.  Whole images only:
 * no partition, no multi-GPU, rank or frame-group context at the drop-in level.
 */
typedef struct rt_hip_adaptive_params
{
	float threshold;	  /* finite, >= 0: the relative standard error a pixel converges at; default 0.03 */
	float floor;		  /* finite, >= 0: added to the mean luminance, so that dark pixels converge too; default 0.01 */
	uint32_t min_samples; /* >= 2 x the pass size; above the cap nothing stops and the frame is the progressive frame; default 32 */
} rt_hip_adaptive_params;

/* the defaults a NULL `params` stands for; pure host code */
RT_HIP_API rt_hip_status rt_hip_adaptive_default_params(rt_hip_adaptive_params* out_params);

/*
 * The update step alone, a pure per-pixel operation on DEVICE buffers of a whole width x height frame (row-major, laid out like the
 * float mean): after a pass of pass_samples samples (a multiple of 16 — or, with whole_pass == 0, whatever the short last pass
 * traced) whose own fold is in d_pass_sum (3 floats per pixel) and whose running sums are in d_accum (3 floats per pixel),
 * d_moments (2 floats per pixel: S1, S2) and d_state (one word per pixel: samples held in bits 0-30, "stopped" in bit 31) are
 * brought up to date and EVERY pixel, stopped or not, is finished from d_accum and its own sample count into d_rgba8_out (and
 * d_rgb_out, 3 floats per pixel).  first_pass != 0: d_moments and d_state are written and not read.  d_active_pixels (one word,
 * overwritten): the pixels still active after the step.  A stopped pixel's words are left as they are.  Needs no scene.
 * Asynchronous on `stream`; on a multi-GPU, rank or frame-group context the root member answers.  The new words travel through a
 * scratch image of the context (12 bytes per pixel, grown on demand, freed with it), which rt_hip_adaptive_pass_device and
 * rt_hip_render_adaptive use too: the adaptive calls of one context must be ordered on ONE stream (or by the caller), never run at the
 * same time on different streams.
 */
RT_HIP_API rt_hip_status rt_hip_adaptive_update_device(rt_hip_ctx* ctx,
									uint32_t width,
									uint32_t height,
									uint32_t pass_samples,
									uint32_t first_pass,
									uint32_t whole_pass,
									const rt_hip_adaptive_params* params, /* NULL = defaults */
									const float* d_accum,
									const float* d_pass_sum,
									float* d_moments,
									uint32_t* d_state,
									uint32_t* d_rgba8_out,
									float* d_rgb_out,		   /* nullable */
									uint32_t* d_active_pixels, /* nullable */
									void* stream);

/*
 * One adaptive pass on the resident scene, whole image: samples [first_sample, first_sample + n_samples) of every ACTIVE pixel
 * (render), then the update step.  first_sample is a multiple of 16; n_samples is the accumulation's pass size (a multiple of 16),
 * or less in the last pass, which ends on the scene's samples_per_pixel.  first_sample == 0 starts an accumulation: nothing of
 * d_block is read, and it need not be cleared.
 *   Whether a pass is WHOLE (the pixels are judged after it) is not an argument: a pass is taken as whole when n_samples is a
 *   multiple of 16 that divides first_sample — true of every pass of the accumulation's size — and as the short last pass otherwise.
 *   LIMITATION: a short last pass that happens to be whole chunks dividing first_sample (pass size 32, cap 48: the last pass is
 *   [32, 48)) is judged as a whole pass of ITS size.  The pixels are unaffected — the cap has been reached, nothing is traced again —
 *   but the stopped bits and d_active_pixels it leaves are not the contract's.  A caller who reads them keeps the cap a multiple of
 *   the pass size; rt_hip_render_adaptive knows its pass size and has no such case.
 *   d_block   DEVICE buffer of 9 x width x height words, the caller's to keep from pass to pass, P = width x height:
 *               words [0, 3P)   accum     the running sums, exactly rt_hip_render_pass_device's accumulator
 *               words [3P, 4P)  state     uint32
 *               words [4P, 7P)  pass_sum  scratch, rewritten by every pass for the pixels it traced
 *               words [7P, 9P)  moments   S1, S2
 *   d_rgba8, d_rgb_f32 (nullable), d_active_pixels (nullable): as rt_hip_adaptive_update_device's outputs.
 *   rt_hip_stats_fetch after it: THIS PASS — primary_samples = pixels that were active x n_samples (counted on the device by the
 *   update step: the host does not know the state words), segments = the pass's.
 */
RT_HIP_API rt_hip_status rt_hip_adaptive_pass_device(rt_hip_ctx* ctx,
									uint32_t width,
									uint32_t height,
									uint64_t seed,
									uint32_t flags,
									uint32_t first_sample,
									uint32_t n_samples,
									const rt_hip_adaptive_params* params, /* NULL = defaults */
									float* d_block,
									uint32_t* d_rgba8,
									float* d_rgb_f32,		   /* nullable */
									uint32_t* d_active_pixels, /* nullable */
									void* stream);

typedef struct rt_hip_adaptive_info
{
	uint32_t samples_done;	 /* samples an ACTIVE pixel holds after this call (the most any pixel holds) */
	uint32_t samples_total;	 /* the cap: the scene's samples_per_pixel */
	uint32_t passes;		 /* passes launched for this accumulation so far */
	uint32_t restarted;		 /* 1: this call started a new accumulation */
	uint32_t active_pixels;	 /* pixels still active after this call */
	uint32_t pixels;		 /* width x height */
	uint64_t samples_traced; /* over all passes so far: the sum of the sample map */
	uint32_t complete;		 /* 1: no pixel is active or the cap is reached; later calls launch nothing */
} rt_hip_adaptive_info;

/*
 * Drop-in level: one call is one adaptive pass, delivered as rt_hip_render_progressive delivers.  pass_samples is rounded up to a
 * multiple of 16 (0 = 16).  The accumulation starts again if anything the frame depends on differs from the call before — what
 * rt_hip_render_progressive looks at, and besides the parameters' bit patterns and pass_samples.  Its state belongs to the context
 * (36 bytes per pixel, grown on demand, freed with it) and is separate from the progressive accumulation, the denoiser's kept
 * guide and the temporal history.  Denoising it in place is not offered: pass rgb_f32 through rt_hip_denoise_device.
 *   A call on a COMPLETE accumulation launches nothing: it delivers the kept frame again and reports stats of zero work.
 *   sample_counts  optional: width x height uint32, the map n(x, y)
 *   stats          optional: THIS PASS — primary_samples = pixels that were active x the pass's samples, segments = the pass's
 */
RT_HIP_API rt_hip_status rt_hip_render_adaptive(rt_hip_ctx* ctx,
									const rt_hip_scene* scene,
									uint32_t* pixels_rgba8888,
									uint32_t width,
									uint32_t height,
									uint64_t seed,
									uint32_t flags,
									uint32_t pass_samples,
									const rt_hip_adaptive_params* params, /* NULL = defaults */
									float* rgb_f32,						  /* nullable */
									uint32_t* sample_counts,			  /* nullable */
									rt_hip_stats* stats,
									rt_hip_adaptive_info* out_info);

/*
 * Where the most recent successful rt_hip_render_adaptive call of THIS PROCESS (any context, any thread) left its accumulation: what a
 * driver that reaches the module only through a plug-in's render() asks to learn whether the accumulation is complete (rt_headless
 * --adaptive).  RT_HIP_INVALID_ARGUMENT before the first such call.  Pure host code, safe to call from any thread.
 */
RT_HIP_API rt_hip_status rt_hip_adaptive_last_info(rt_hip_adaptive_info* out_info);

/* ---- emissive materials (RT_HIP_FLAG_EMISSION): additions to ABI 6 — rt_hip_scene keeps its size ---------------- */

/*
 * The context's EMISSION TABLE: one row of 3 floats (r, g, b) per material of the resident scene, copied inside the call.  Every
 * component must be finite and >= 0: a NaN, a negative value or an infinity is RT_HIP_INVALID_ARGUMENT, the message naming the
 * material's index and the component; -0.0f passes and counts as zero.  A material IS A LIGHT iff r > 0 || g > 0 || b > 0.
 * NULL / 0 clears the table.  The table is state of the context: it survives scene uploads (a frame with the flag checks its row
 * count against the resident scene's n_materials), and on a context from rt_hip_create_multi it reaches every member device.
 * Without RT_HIP_FLAG_EMISSION no frame reads it.
 */
RT_HIP_API rt_hip_status rt_hip_set_emission(rt_hip_ctx* ctx, const float* emission_rgb, uint32_t n_materials);

/*
 * An emission table from a text: how a host whose materials have no emission column (rt::materials, src/soa.toml:6-12) reaches the
 * feature.  Host-only; touches no device.  `spec` is a list of items KEY=R,G,B separated by ';' (KEY=V is the grey light V,V,V;
 * blanks around keys, numbers and separators are ignored).  An all-digit KEY is a material index; any other KEY is a material name
 * and sets EVERY material of that name (`material_names`: n_materials strings, may be NULL when only indices are used).  An empty
 * spec gives an all-zero table.  RT_HIP_INVALID_ARGUMENT, with a message that quotes the item: an unknown name, an index out of
 * range, a missing '=', an empty item (a trailing ';'), two or more than three numbers, anything that is not a number, and a value
 * that is negative, NaN or infinite.  out_emission_rgb receives 3 * n_materials floats (untouched on failure).
 */
RT_HIP_API rt_hip_status rt_hip_lights_from_spec(const char* spec, const char* const* material_names, uint32_t n_materials, float* out_emission_rgb);

/* ---- a thin-lens camera (RT_HIP_FLAG_THIN_LENS): additions to ABI 6 — rt_hip_scene keeps its size --------------- */

/* world units; the distance is measured along the view direction */
typedef struct rt_hip_lens
{
	float aperture_radius; /* finite, >= 0; 0: frames with the flag are the flag-less frames */
	float focus_distance;  /* finite, > 0 */
} rt_hip_lens;

/*
 * The context's LENS, copied inside the call.  aperture_radius must be finite and >= 0, focus_distance finite and > 0: anything
 * else is RT_HIP_INVALID_ARGUMENT, the message naming the field.  NULL clears the lens.  The lens is state of the context: it
 * survives scene uploads, and on a context from rt_hip_create_multi it reaches every member device.  Without
 * RT_HIP_FLAG_THIN_LENS no frame reads it.
 */
RT_HIP_API rt_hip_status rt_hip_set_lens(rt_hip_ctx* ctx, const rt_hip_lens* lens);

/*
 * A lens from a text: "aperture=0.05,focus=4.2" (both keys, each once, in either order; blanks around keys, numbers and
 * separators are ignored).  Host-only; touches no device.  RT_HIP_INVALID_ARGUMENT, with a message that says why: an unknown or
 * repeated key, a missing key, a missing '=', an empty item, anything that is not a number, and a value rt_hip_set_lens refuses.
 * out_lens is untouched on failure.
 */
RT_HIP_API rt_hip_status rt_hip_lens_from_spec(const char* spec, rt_hip_lens* out_lens);

/* ---- tone mapping for HDR frames: device auto-exposure, three curves --------------------------------------- */
/*
 * With RT_HIP_FLAG_EMISSION the float mean of a frame lies far above 1, and the only way from a float mean to pixels above is the
 * renderer's own finish: square root, clamp to [0, 1], pack.  These entry points put an EXPOSURE and a TONE CURVE in front of that
 * finish, on the device: the exposure is metered from an integer histogram of the frame's log2 luminance (8 bins per octave from
 * 2^-16 to 2^16, a trimmed mean of the bins in exact integer arithmetic), optionally eased toward from the exposure of the frame
 * before, and never leaves the device on its way to the pixels.  A contract of its own: + - x, correctly rounded division and
 * square root, compare-and-select in one stated order, no log, exp or pow anywhere, so that the device's result equals a serial CPU
 * restatement bit for bit — it is NOT the reference's arithmetic (the reference has no tone mapping).  No speed is promised.
 * Additions to ABI 6 (RT_HIP_ABI_VERSION stays 6): a caller that may meet an older library looks them up with dlsym.
 */
#define RT_HIP_TONEMAP_NONE 0u	   /* o = v */
#define RT_HIP_TONEMAP_REINHARD 1u /* extended Reinhard on luminance, hue kept: o = v (1 + Yv / white^2) / (1 + Yv) */
#define RT_HIP_TONEMAP_ACES 2u	   /* the Narkowicz rational fit, per channel */

typedef struct rt_hip_tonemap_params
{
	uint32_t curve;			/* RT_HIP_TONEMAP_NONE, _REINHARD or _ACES; default ACES */
	uint32_t low_permille;	/* the darkest pixels the meter drops, in thousandths of the metered ones; default 50 */
	uint32_t high_permille; /* ... and the brightest; low_permille + high_permille < 1000; default 20 */
	float exposure;			/* 0 = auto (metered); finite and > 0 = manual: nothing is metered; default 0 */
	float key;				/* finite, > 0: the luminance the metered one is mapped to; default 0.18 */
	float white;			/* 2^-20 .. 2^20: REINHARD's white point, the luminance that maps to 1; default 4 */
	float min_exposure;		/* finite, > 0: the metered exposure is clamped to [min_exposure, max_exposure]; default 2^-10 */
	float max_exposure;		/* finite, >= min_exposure; default 2^10 */
	float adaptation;		/* (0, 1]: 1 = the metered target at once; less: prev + adaptation x (target - prev); default 1 */
} rt_hip_tonemap_params;

typedef struct rt_hip_tonemap_info
{
	float exposure;	   /* the exposure applied */
	float target;	   /* the metered target (manual exposure: the exposure) */
	uint32_t counted;  /* pixels that were metered; 0 under a manual exposure, like the three below */
	uint32_t skipped;  /* pixels whose luminance is NaN, not positive or infinite: not metered */
	uint32_t kept;	   /* metered pixels inside the rank window */
	uint32_t mean_q8;  /* the trimmed mean bin, in 1/256 of a bin */
} rt_hip_tonemap_info;

/* the defaults a NULL `params` stands for; pure host code */
RT_HIP_API rt_hip_status rt_hip_tonemap_default_params(rt_hip_tonemap_params* out_params);

/*
 * Parameters from a text, CURVE[:EXPOSURE]: CURVE is none, reinhard or aces; EXPOSURE is auto (the default) or a positive finite
 * number.  Everything else keeps its default.  Host-only; touches no device.  RT_HIP_INVALID_ARGUMENT, with a message that quotes
 * the text, for anything else; out_params is untouched then.
 */
RT_HIP_API rt_hip_status rt_hip_tonemap_from_spec(const char* spec, rt_hip_tonemap_params* out_params);

/*
 * Tone mapping as a pure image operation on DEVICE buffers of a whole width x height frame: d_rgb_in (3 * width * height floats, a
 * frame's float mean in linear light, 16-byte aligned) gives d_rgb_out (3 * width * height floats: the mapped frame, linear light,
 * neither clamped nor gamma-encoded; optional) and d_rgba8_out (width * height packed pixels: square root, clamp and pack as
 * rt_hip_render finishes a pixel; optional) — not both NULL.  d_rgb_out == d_rgb_in exactly is allowed (in place); every other
 * overlap between the buffers is refused.
 *   d_state   the caller's 8-word DEVICE record, written by every call: exposure (float bits), target (float bits), counted,
 *             skipped, kept, mean_q8, and two reserved words (0).  With params->adaptation < 1 word 0 is also READ, as the exposure
 *             of the frame before (a word that is not a finite positive float — a zeroed record — starts over at the target).
 * Three launches on `stream` (histogram, exposure, pixels; one under a manual exposure) and no readback: asynchronous.  The
 * histogram's 257 words belong to the context: the tone-mapping calls of one context must be ordered on ONE stream (or by the
 * caller).  It reads no scene.  On a multi-GPU, rank or frame-group context the root member answers.
 */
RT_HIP_API rt_hip_status rt_hip_tonemap_device(rt_hip_ctx* ctx,
									uint32_t width,
									uint32_t height,
									const float* d_rgb_in,
									const rt_hip_tonemap_params* params, /* NULL = defaults */
									uint32_t* d_state,
									float* d_rgb_out,	   /* nullable; may be d_rgb_in */
									uint32_t* d_rgba8_out, /* nullable, not both NULL */
									void* stream);

/*
 * Drop-in level: one call is one tone-mapped frame.  The scene is uploaded by fingerprint as in rt_hip_render; the one-shot frame
 * is traced into a device float mean by the launch rt_hip_render_device makes, mapped by the three launches above and copied into
 * the caller's plain HOST memory: pixels_rgba8888 (width * height) and, optionally, rgb_f32 (3 * width * height: the MAPPED frame
 * in linear light).  The context keeps the state record from call to call (what params->adaptation < 1 eases from) and zeroes it
 * when the frame's size changes.
 *   stats     optional: the traced frame's; render_ms runs through the last of the three launches.
 * Flags: every flag of a one-shot frame (RT_HIP_FLAG_EMISSION and RT_HIP_FLAG_DIRECT_LIGHT among them) and RT_HIP_FLAG_STATS;
 * RT_HIP_FLAG_PREVIEW and RT_HIP_FLAG_PERSISTENT_FRAME are refused with RT_HIP_UNSUPPORTED and their names.  Contexts from
 * rt_hip_create only.
 */
RT_HIP_API rt_hip_status rt_hip_render_tonemapped(rt_hip_ctx* ctx,
									const rt_hip_scene* scene,
									uint32_t* pixels_rgba8888,
									uint32_t width,
									uint32_t height,
									uint64_t seed,
									uint32_t flags,
									const rt_hip_tonemap_params* params, /* NULL = defaults */
									float* rgb_f32,						 /* nullable */
									rt_hip_stats* stats,
									rt_hip_tonemap_info* out_info);		 /* nullable */

/* ---- bloom for HDR frames: a device pyramid in front of the tone curve -------------------------------------- */
/*
 * Tone mapping is a global operator: a lamp comes out as a hard-edged disc, and a lamp of 4 looks like a lamp of 400.  What tells a
 * viewer that something is brighter than the display is the glow around it.  These entry points add that glow to a float frame, on
 * the device, BEFORE the exposure and the curve: what of every pixel lies above a threshold (through a quadratic knee) is averaged
 * 2 x 2 into a half-size level, filtered down a pyramid of up to 8 levels with a separable 5-tap binomial, summed back up with a
 * tent, each coarser level weighted by `scatter`, and added to the frame times intensity / (1 + scatter + scatter^2 + ...).
 * A contract of its own: + - x, correctly rounded division and compare-and-select in one stated order, no log, exp or pow anywhere,
 * so that the device's result equals a serial CPU restatement bit for bit — it is NOT the reference's arithmetic (the reference has
 * no bloom).  No speed is promised.  Additions to ABI 6 (RT_HIP_ABI_VERSION stays 6): a caller that may meet an older library
 * looks them up with dlsym.
 */
typedef struct rt_hip_bloom_params
{
	float threshold; /* 0 .. 2^20: the largest channel above which a pixel glows; default 1 */
	float knee;		 /* 0, or 2^-20 .. threshold: the half-width of the quadratic knee below and above the threshold; default 0.5 */
	float intensity; /* 0 .. 2^10: how much of the glow layer is added (the layer is normalised by the levels' weights); default 0.1 */
	float scatter;	 /* 0 .. 1: the weight of every coarser level relative to the one before: 0 = a tight glow, 1 = a wide one; default 0.7 */
	uint32_t levels; /* 1 .. 8: the pyramid's levels, fewer where the frame reaches 1 x 1 before; default 6 */
} rt_hip_bloom_params;

typedef struct rt_hip_bloom_info
{
	uint32_t levels;		/* the levels a frame of this size gets: min(params->levels, the count at which a level first is 1 x 1) */
	uint32_t last_width;	/* the coarsest level's size */
	uint32_t last_height;
	uint64_t scratch_bytes; /* what the pyramid takes of device memory: 12 bytes a texel, all levels */
} rt_hip_bloom_info;

/* the defaults a NULL `params` stands for; pure host code */
RT_HIP_API rt_hip_status rt_hip_bloom_default_params(rt_hip_bloom_params* out_params);

/*
 * Parameters from a text: `default`, or items KEY=VALUE separated by ',' with the keys intensity, threshold, knee, scatter and
 * levels, each at most once; a value is a plain decimal number (levels: a whole one).  Everything else keeps its default.
 * Host-only; touches no device.  RT_HIP_INVALID_ARGUMENT, with a message that quotes the text, for anything else and for values
 * the parameter check refuses (that message names the field too); out_params is untouched then.
 */
RT_HIP_API rt_hip_status rt_hip_bloom_from_spec(const char* spec, rt_hip_bloom_params* out_params);

/*
 * The pyramid a width x height frame (1 .. 32768 a side) gets under `params` (NULL = defaults).  Level 0 is ceil(width / 2) x
 * ceil(height / 2), every next level halves the one before with ceil.  Host-only; touches no device.
 */
RT_HIP_API rt_hip_status rt_hip_bloom_plan(uint32_t width, uint32_t height, const rt_hip_bloom_params* params, rt_hip_bloom_info* out_info);

/*
 * Bloom as a pure image operation on DEVICE buffers of a whole width x height frame: d_rgb_in (3 * width * height floats, a frame's
 * float mean in linear light) gives d_rgb_out (3 * width * height floats: d_rgb_in + gain x layer, per channel; optional) and
 * d_layer_out (3 * width * height floats: the glow layer alone, before the gain; optional) — not both NULL.  d_rgb_out == d_rgb_in
 * exactly is allowed (in place); every other overlap between the buffers is refused.  NaN, negative and infinite channels enter the
 * pyramid as 0, 0 and 2^20: a bad pixel does not spread, and d_rgb_out keeps it as it was (NaN + anything is that NaN).
 * 2 x levels launches on `stream` (prefilter, levels - 1 down, levels - 1 up, composite: at most 16) and no readback:
 * asynchronous.  The pyramid's scratch belongs to the context and grows on demand: the bloom calls of one context must be ordered
 * on ONE stream (or by the caller), and a call that grows the scratch frees the block the call before used — with calls in flight
 * on another stream that is the caller's to order.  It reads no scene.  On a multi-GPU, rank or frame-group context the root
 * member answers.
 */
RT_HIP_API rt_hip_status rt_hip_bloom_device(rt_hip_ctx* ctx,
									uint32_t width,
									uint32_t height,
									const float* d_rgb_in,
									const rt_hip_bloom_params* params, /* NULL = defaults */
									float* d_rgb_out,				   /* nullable; may be d_rgb_in */
									float* d_layer_out,				   /* nullable, not both NULL */
									void* stream);

/*
 * Drop-in level: one call is one bloomed, tone-mapped frame.  As rt_hip_render_tonemapped, with the bloom launches between the
 * traced frame and the meter: the one-shot frame is traced into a device float mean, bloomed in place, metered, exposed and mapped,
 * and copied into the caller's plain HOST memory (pixels_rgba8888 and, optionally, rgb_f32: the MAPPED frame in linear light).  The
 * meter sees the bloomed frame.  The context keeps a state record for these calls, separate from rt_hip_render_tonemapped's, and
 * zeroes it when the frame's size changes.
 *   stats     optional: the traced frame's; render_ms runs through the last launch.
 * Flags, refusals (RT_HIP_FLAG_PREVIEW and RT_HIP_FLAG_PERSISTENT_FRAME by name, unknown bits) and the contexts taken (those from
 * rt_hip_create only) are rt_hip_render_tonemapped's.
 */
RT_HIP_API rt_hip_status rt_hip_render_bloomed(rt_hip_ctx* ctx,
									const rt_hip_scene* scene,
									uint32_t* pixels_rgba8888,
									uint32_t width,
									uint32_t height,
									uint64_t seed,
									uint32_t flags,
									const rt_hip_bloom_params* bloom_params,	 /* NULL = defaults */
									const rt_hip_tonemap_params* tonemap_params, /* NULL = defaults */
									float* rgb_f32,								 /* nullable */
									rt_hip_stats* stats,
									rt_hip_tonemap_info* out_tonemap_info);		 /* nullable */

/* Drop the page-lock taken under RT_HIP_FLAG_PERSISTENT_FRAME (see there).  Waits for the context's stream first. */
RT_HIP_API void rt_hip_forget_frame(rt_hip_ctx* ctx);

/* Page-locks on CALLERS' memory that contexts of this process hold right now: 0 unless somebody rendered with
 * RT_HIP_FLAG_PERSISTENT_FRAME (or as a rank of a frame group) and has neither moved on to another buffer nor called
 * rt_hip_forget_frame / rt_hip_destroy since.  A diagnostic for integrators and for this repository's tests (which assert
 * 0 after every GPU test): memory the module no longer knows about can never be written by it. */
RT_HIP_API uint32_t rt_hip_live_frame_locks(void);

#ifdef __cplusplus
}
#endif

#endif /* RT_HIP_H */
