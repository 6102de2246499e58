/*
 * rt_hip_kat.h — known-answer entry points of librt_hip_kat.so, the TEST-ONLY companion of librt_hip.so.
 *
 * Device implementations of the leaf functions of the mg_ray_tracer path (reference src/renderers/mg_ray_tracer.cpp:36-140,
 * src/random.hpp:12-66), run on inputs of the caller's choosing, for parity tests against oracle/.  The reference has no
 * tests and nothing in it corresponds.  NOT part of the drop-in surface of include/rt_hip.h: a deployment
 * ships librt_hip.so alone.  `ctx` is a context from rt_hip_create (librt_hip.so); failures leave their message in
 * rt_hip_kat_last_error().
 */
#ifndef RT_HIP_KAT_H
#define RT_HIP_KAT_H

#include "rt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Message for the most recent failure of a call below on the calling thread ("" if none).  Never NULL. */
RT_HIP_API const char* rt_hip_kat_last_error(void);

/* out[i] = bits of the i-th draw: rt_hip random stream (seed, pixel, sample, draw k) for k in [0, n). */
RT_HIP_API rt_hip_status rt_hip_kat_random(rt_hip_ctx* ctx, uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t n, float* out);

/* For n rays (origin/direction as 3 floats each, AoS) against the resident scene: closest-hit distance
 * (< 0 = miss), primitive kind (0 none, 1 sphere, 2 plane), primitive index, and hit normal (3 floats). */
RT_HIP_API rt_hip_status rt_hip_kat_closest_hit(rt_hip_ctx* ctx,
									 uint32_t n,
									 const float* origins,
									 const float* directions,
									 float* out_distance,
									 uint32_t* out_kind,
									 uint32_t* out_index,
									 float* out_normal);

/* rt_hip_kat_closest_hit, answered by RT_HIP_FLAG_BVH's traversal (the render kernel's own code: bvh_scan.hpp) through a
 * hierarchy built for the resident scene as the render path builds it.  Must equal rt_hip_kat_closest_hit bit for bit. */
RT_HIP_API rt_hip_status rt_hip_kat_closest_hit_bvh(rt_hip_ctx* ctx,
										 uint32_t n,
										 const float* origins,
										 const float* directions,
										 float* out_distance,
										 uint32_t* out_kind,
										 uint32_t* out_index,
										 float* out_normal);

/* Host only (no context, no GPU): the sphere hierarchy RT_HIP_FLAG_BVH builds for `scene`.  out_counts[5] = { inner nodes,
 * spheres in the tree, spheres in the always list, depth (inner-node levels of the deepest path), root link }.  Every other
 * output may be NULL; each is sized for the worst case, n = scene->n_spheres:
 *   out_nodes   16 floats per node (at most n): box A min xyz, link A (bits), box A max xyz, link B (bits), box B min xyz, 0,
 *               box B max xyz, 0.  A link is a node index, or 0x80000000 | (count - 1) << 29 | first for a leaf of `count`
 *               spheres at leaf slots first .. first + count - 1;
 *   out_order   n: the scene index of each leaf slot;      out_spheres  4n: the (cx, cy, cz, r^2) of each leaf slot;
 *   out_always  n: scene indices outside the tree;          out_bound    4: centre xyz and radius of the ball around the tree. */
RT_HIP_API rt_hip_status rt_hip_kat_bvh_build(const rt_hip_scene* scene,
								   uint32_t out_counts[5],
								   float* out_nodes,
								   uint32_t* out_order,
								   float* out_spheres,
								   uint32_t* out_always,
								   float out_bound[4]);

/* The tree that the product's device builder (RT_HIP_FLAG_BVH_DEVICE_BUILD, rt_amd/csrc/bvh_build.hip) makes for the scene resident
 * on `ctx`, read back.  The outputs mean what rt_hip_kat_bvh_build's mean, with one difference: node k is the node that cuts the
 * leaf order between slots k and k + 1, so out_counts[0] counts node SLOTS (tree spheres - 1, or 0 for a tree of one leaf) and
 * the slots no cut uses are all zero.  Must equal tests/native/lbvh_reference.cpp byte for byte. */
RT_HIP_API rt_hip_status rt_hip_kat_bvh_build_device(rt_hip_ctx* ctx,
											  uint32_t out_counts[5],
											  float* out_nodes,
											  uint32_t* out_order,
											  float* out_spheres,
											  uint32_t* out_always,
											  float out_bound[4]);

/* rt_hip_kat_closest_hit_bvh through the device builder's tree.  Must equal rt_hip_kat_closest_hit bit for bit. */
RT_HIP_API rt_hip_status rt_hip_kat_closest_hit_bvh_device(rt_hip_ctx* ctx,
													uint32_t n,
													const float* origins,
													const float* directions,
													float* out_distance,
													uint32_t* out_kind,
													uint32_t* out_index,
													float* out_normal);

/* rt_hip_kat_closest_hit with the scene's BOXES in the query, as RT_HIP_FLAG_TRACE_BOXES' kernels answer it (the same device
 * functions: rt_amd/csrc/scan.hpp, contract.hpp hits_box_face): kind 3 = box, index = the box's, normal = its outward face normal
 * (DESIGN.md §3.7).  At most 256 boxes (RT_HIP_UNSUPPORTED beyond).  Must equal tests/native/box_reference.cpp bit for bit. */
RT_HIP_API rt_hip_status rt_hip_kat_closest_hit_boxes(rt_hip_ctx* ctx,
											   uint32_t n,
											   const float* origins,
											   const float* directions,
											   float* out_distance,
											   uint32_t* out_kind,
											   uint32_t* out_index,
											   float* out_normal);

/* Host only (no context, no GPU): the box hierarchy RT_HIP_FLAG_BOX_BVH builds for `scene` (rt_amd/csrc/box_bvh.cpp), from the pairs
 * the upload derives (corners = center -/+ extents, the material index as bits in the fourth word of the first).  out_counts[5] =
 * { inner nodes, boxes in the tree, boxes in the always list, depth, root link }, the nodes and links laid out as
 * rt_hip_kat_bvh_build's.  Every other output may be NULL; each is sized for the worst case, n = scene->n_boxes:
 *   out_nodes   16 floats per node (at most n);             out_order   n: the scene index of each leaf slot;
 *   out_corners 8n: the two float4s of each leaf slot;      out_always  n: scene indices outside the tree, ascending. */
RT_HIP_API rt_hip_status rt_hip_kat_box_bvh_build(const rt_hip_scene* scene, uint32_t out_counts[5], float* out_nodes, uint32_t* out_order, float* out_corners, uint32_t* out_always);

/* rt_hip_kat_closest_hit_boxes with the boxes reached through RT_HIP_FLAG_BOX_BVH's traversal (the render kernel's own code:
 * rt_amd/csrc/box_bvh_scan.hpp, its fall-back to the linear scan included) over a hierarchy built for the resident scene as the
 * render path builds it.  Any number of boxes.  Must equal tests/native/box_reference.cpp bit for bit. */
RT_HIP_API rt_hip_status rt_hip_kat_closest_hit_boxes_bvh(rt_hip_ctx* ctx,
												   uint32_t n,
												   const float* origins,
												   const float* directions,
												   float* out_distance,
												   uint32_t* out_kind,
												   uint32_t* out_index,
												   float* out_normal);

/* How many box hierarchies `ctx` has built on the host so far: a frame that reuses the cached tree leaves it as it was. */
RT_HIP_API rt_hip_status rt_hip_kat_box_bvh_builds(rt_hip_ctx* ctx, uint64_t* out_builds);

/* out_sqrt[i] = sqrtf(a[i]), out_div[i] = a[i] / b[i] as the device computes them (must be correctly rounded). */
RT_HIP_API rt_hip_status rt_hip_kat_sqrt_div(rt_hip_ctx* ctx, uint32_t n, const float* a, const float* b, float* out_sqrt, float* out_div);

/* Runs ALL 2^32 binary32 bit patterns through the kernels' shortened sqrt / reciprocal / reciprocal-sqrt sequences and
 * compares each result, bit for bit, with the compiler's general correctly rounded expansion (sqrt, reciprocal) and with
 * the arithmetic contract's definition of normalize()'s reciprocal square root evaluated through binary64.
 * out_mismatches[k] = number of differing inputs, out_first[k] = smallest differing input's bits (valid if count > 0),
 * k = 0 sqrt, 1 reciprocal, 2 reciprocal of sqrt.  All three counts must be 0. */
RT_HIP_API rt_hip_status rt_hip_kat_exhaustive_math(rt_hip_ctx* ctx, uint64_t out_mismatches[3], uint32_t out_first[3]);

/* RT_HIP_FLAG_FAST's leaf functions (the fast half of rt_amd/csrc/contract.hpp, compiled as the fast build of the kernels is:
 * rt_amd/csrc/kat_fast.hip) per element: out_sqrt[i] = sqrt_rn(x[i]), out_rcp[i] = rcp_rn(x[i]), out_rsq[i] = inv_sqrt_rn(x[i]),
 * out_div[i] = divide(x[i], y[i]).  The hardware's approximations as they are: tests MEASURE their error against binary64. */
RT_HIP_API rt_hip_status rt_hip_kat_fast_math(rt_hip_ctx* ctx, uint32_t n, const float* x, const float* y, float* out_sqrt, float* out_rcp, float* out_rsq, float* out_div);

/* RT_HIP_FLAG_DIRECT_LIGHT's rules (rt_amd/csrc/direct_light_rules.hpp) as the device computes them; both must equal
 * the same header compiled with g++ (tests/native/direct_reference.cpp) bit for bit.
 * The octahedral map: out[4 i ..] = (p.x, p.y, p.z, dot(p, p)) of the numerators (ka[i], kb[i]), each below 2^24. */
RT_HIP_API rt_hip_status rt_hip_kat_direct_octahedral(rt_hip_ctx* ctx, uint32_t n, const uint32_t* ka, const uint32_t* kb, float* out);
/* The aim and its weight: in[9 i ..] = vertex x, its normal, the light's centre (3 floats each); radius[i]; n_lights (1 .. 256) ->
 * out[5 i ..] = (w.x, w.y, w.z, weight, aimed as 0 / 1). */
RT_HIP_API rt_hip_status rt_hip_kat_direct_aim(rt_hip_ctx* ctx, uint32_t n, const uint32_t* ka, const uint32_t* kb, const float* in, const float* radius, uint32_t n_lights, float* out);

/* RT_HIP_FLAG_THIN_LENS's rules (rt_amd/csrc/lens_rules.hpp) as the lens builds of the kernels compute them; must equal
 * the same header compiled with g++ (tests/native/lens_reference.cpp) bit for bit.  ka, kb: n pairs of numerators, each below 2^24.
 * ray[9] = the pinhole's ray (origin, normalised direction) and the eye; lens_words[10] = U, V, fwd, focus ->
 * out[9 i ..] = (lx, ly, origin.xyz, direction.xyz, bent as 0 / 1): the disk point and the lens ray, normalised. */
RT_HIP_API rt_hip_status rt_hip_kat_lens(rt_hip_ctx* ctx, uint32_t n, const uint32_t* ka, const uint32_t* kb, const float* ray, const float* lens_words, float* out);

#ifdef __cplusplus
}
#endif

#endif /* RT_HIP_KAT_H */
