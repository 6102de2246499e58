// rt_amd/csrc/kat.hip — librt_hip_kat.so, the TEST-ONLY companion of librt_hip.so (include/rt_hip_kat.h): device
// implementations of the path's leaf functions run on inputs of the tests' choosing — the random streams, the closest-hit
// scan (the render kernels' own code: scan.hpp), the square root and the division, and every binary32 bit pattern through
// the shortened exact-math sequences of contract.hpp.  The reference has no tests; these entry points are
// how tests/ pin the kernels' arithmetic function by function against oracle/.
//
// Not part of the drop-in surface: nothing in librt_hip.so refers to this file, and a deployment does not ship it.  It
// includes internal.hpp for the layout of rt_hip_ctx only (it reads a context's device and its resident scene), links
// librt_hip.so for nothing but the public rt_hip.h calls, and — like the product — hands the HIP runtime no caller
// memory: inputs and results travel through page-locked blocks of its own.
#include "../../include/rt_hip_kat.h"
#include "internal.hpp"
#include "scan.hpp"
#include "bvh_scan.hpp"
#include "box_bvh_scan.hpp"
#include "bvh_build.hpp"
#include "bvh_build_device.hpp"
#include "direct_light_rules.hpp"
// (RT_HIP_FLAG_THIN_LENS's rules take their leaf function from the includer, as kernels.hip hands it in)
namespace rt_hip::lens::leaf
{
	__device__ __forceinline__ float divide(float a, float b) { return rt_hip::divide(a, b); }
}
#include "lens_rules.hpp"

#include <algorithm>
#include <vector>

using namespace rt_hip;

namespace
{
	thread_local std::string g_kat_error;

	rt_hip_status kat_fail(rt_hip_status status, const char* format, ...) __attribute__((format(printf, 2, 3)));
	rt_hip_status kat_fail(rt_hip_status status, const char* format, ...)
	{
		char buffer[512];
		va_list args;
		va_start(args, format);
		std::vsnprintf(buffer, sizeof(buffer), format, args);
		va_end(args);
		g_kat_error = buffer;
		return status;
	}

#define RT_HIP_KAT_TRY(expr)                                                                                           \
	do                                                                                                                 \
	{                                                                                                                  \
		const hipError_t rt_hip_try_err = (expr);                                                                      \
		if (rt_hip_try_err != hipSuccess)                                                                              \
			return kat_fail(RT_HIP_RUNTIME_ERROR, "%s failed: %s", #expr, hipGetErrorString(rt_hip_try_err));          \
	}                                                                                                                  \
	while (false)

	// one call's scratch: a device block and a page-locked host block of the same size, freed when the call returns
	struct scratch
	{
		device_buffer device;
		pinned_buffer host;
		~scratch()
		{
			device.release();
			host.release();
		}
		hipError_t reserve(size_t bytes)
		{
			const hipError_t e = device.reserve(bytes);
			return e != hipSuccess ? e : host.reserve(bytes);
		}
	};
}

namespace rt_hip
{
namespace
{
	// ---- known-answer kernels -----------------------------------------------------------------------------------
	__global__ void kat_random(frame_keys frame, uint32_t pixel, uint32_t sample, uint32_t n, float* out)
	{
		if (blockIdx.x || threadIdx.x)
			return;
		stream_keys keys;
		keys.function_key = pixel_function_key(frame.a, pixel);
		keys.stride = pixel_stride(frame.b, keys.function_key);
		// the stream flattened, as oracle_random has it: the three draws of the first step, of the second, ...
		uint32_t counter = sample_counter(keys.stride, sample);
		for (uint32_t i = 0; i < n; i += 3u)
		{
			const uint32_t word = next_step_word(counter, keys);
			const uint32_t product[3] = { word * step_mul_a, word * step_mul_b, word * step_mul_c };
			for (uint32_t j = 0; j < 3u && i + j < n; j++)
				out[i + j] = step_numerator(product[j]) * random_scale;
		}
	}

	// BVH: the spheres through RT_HIP_FLAG_BVH's traversal (`tree`) instead of the linear scan
	// BOXES: RT_HIP_FLAG_TRACE_BOXES' query — the scene's boxes (at most box_max_count: checked by the caller) scanned after spheres and
	// planes, the three-way selection, a box's normal from the contract's face rule (scan.hpp: the render kernels' own functions)
	template <bool BVH, bool BOXES = false>
	__global__ __launch_bounds__(block_threads) void kat_closest_hit(const device_scene s,
																	 uint32_t n,
																	 const float* __restrict__ origins,
																	 const float* __restrict__ directions,
																	 float* __restrict__ out_distance,
																	 uint32_t* __restrict__ out_kind,
																	 uint32_t* __restrict__ out_index,
																	 float* __restrict__ out_normal,
																	 const device_bvh tree) // [BVH] the hierarchy of the scene
	{
		__shared__ float4 tile[tile_primitives];
		const uint32_t i = blockIdx.x * block_threads + threadIdx.x;
		const bool alive = i < n;
		vec3 o = { 0, 0, 0 }, d = { 0, 0, 1 };
		if (alive)
		{
			o = { origins[i * 3], origins[i * 3 + 1], origins[i * 3 + 2] };
			d = { directions[i * 3], directions[i * 3 + 1], directions[i * 3 + 2] };
		}
		candidate planes = { 0.0f, 0u, false };
		candidate spheres = { 0.0f, 0u, false };
		for (uint32_t first = 0; first < s.n_planes; first += tile_primitives)
		{
			const uint32_t count = min(tile_primitives, s.n_planes - first);
			__syncthreads();
			stage_planes(tile, s, first, count);
			__syncthreads();
			if (alive)
				scan_lds<false>(planes, o, d, tile, count, first);
		}
		if constexpr (BVH)
		{
			__shared__ uint32_t stacks[bvh_max_depth * block_threads];
			if (alive && !bvh_spheres(spheres, o, d, tree, s.primitive_geometry, stacks + threadIdx.x))
			{
				spheres = { 0.0f, 0u, false }; // what the render kernel does too: the sequential rule decides
				scan_lds<true>(spheres, o, d, s.primitive_geometry, s.n_spheres, 0);
			}
		}
		else
			for (uint32_t first = 0; first < s.n_spheres; first += tile_primitives)
			{
				const uint32_t count = min(tile_primitives, s.n_spheres - first);
				__syncthreads();
				stage_spheres(tile, s, first, count);
				__syncthreads();
				if (alive)
					scan_lds<true>(spheres, o, d, tile, count, first);
			}
		__shared__ float4 box_tile[BOXES ? 2u * box_max_count : 1u];
		if constexpr (BOXES)
		{
			for (uint32_t k = threadIdx.x; k < 2u * s.n_boxes; k += block_threads)
				box_tile[k] = s.box_bounds[k];
			__syncthreads();
		}
		if (alive)
		{
			float distance;
			uint32_t index;
			uint32_t kind;
			vec3 normal;
			float4 shading;
			uint32_t scatter;
			if constexpr (BOXES)
			{
				candidate boxes = { 0.0f, 0u, false };
				const vec3 inv = box_reciprocals(d);
				scan_boxes(boxes, o, inv, box_tile, s.n_boxes);
				kind = select_hit(spheres, planes, boxes, distance, index);
				fetch_hit<false>(s, box_tile, o, d, inv, kind, distance, index, normal, shading, scatter);
			}
			else
			{
				kind = select_hit(spheres, planes, distance, index);
				fetch_hit<false>(s, o, d, kind, distance, index, normal, shading, scatter);
			}
			if (!kind)
				normal = { 0.0f, 0.0f, 0.0f }; // hit_result{ -1 } of the reference: no normal
			out_distance[i] = distance;
			out_kind[i] = kind;
			out_index[i] = kind ? index : 0u;
			out_normal[i * 3 + 0] = normal.x;
			out_normal[i * 3 + 1] = normal.y;
			out_normal[i * 3 + 2] = normal.z;
		}
	}

	// RT_HIP_FLAG_BOX_BVH's query: spheres and planes as above (the linear scans), the boxes — any number — through the render kernel's own
	// traversal (box_bvh_scan.hpp) with its fall-back to the linear scan over the pairs in memory, the three-way selection, the face rule
	__global__ __launch_bounds__(block_threads) void kat_closest_hit_box_tree(const device_scene s,
																				  uint32_t n,
																				  const float* __restrict__ origins,
																				  const float* __restrict__ directions,
																				  float* __restrict__ out_distance,
																				  uint32_t* __restrict__ out_kind,
																				  uint32_t* __restrict__ out_index,
																				  float* __restrict__ out_normal,
																				  const device_box_bvh tree)
	{
		__shared__ float4 tile[tile_primitives];
		__shared__ uint32_t stacks[bvh_max_depth * block_threads];
		const uint32_t i = blockIdx.x * block_threads + threadIdx.x;
		const bool alive = i < n;
		vec3 o = { 0, 0, 0 }, d = { 0, 0, 1 };
		if (alive)
		{
			o = { origins[i * 3], origins[i * 3 + 1], origins[i * 3 + 2] };
			d = { directions[i * 3], directions[i * 3 + 1], directions[i * 3 + 2] };
		}
		candidate planes = { 0.0f, 0u, false };
		candidate spheres = { 0.0f, 0u, false };
		for (uint32_t first = 0; first < s.n_planes; first += tile_primitives)
		{
			const uint32_t count = min(tile_primitives, s.n_planes - first);
			__syncthreads();
			stage_planes(tile, s, first, count);
			__syncthreads();
			if (alive)
				scan_lds<false>(planes, o, d, tile, count, first);
		}
		for (uint32_t first = 0; first < s.n_spheres; first += tile_primitives)
		{
			const uint32_t count = min(tile_primitives, s.n_spheres - first);
			__syncthreads();
			stage_spheres(tile, s, first, count);
			__syncthreads();
			if (alive)
				scan_lds<true>(spheres, o, d, tile, count, first);
		}
		if (alive)
		{
			candidate boxes = { 0.0f, 0u, false };
			const vec3 inv = box_reciprocals(d);
			if (!bvh_boxes(boxes, o, inv, tree, s.box_bounds, stacks + threadIdx.x))
			{
				boxes = { 0.0f, 0u, false }; // what the render kernel does too: the linear scan decides
				scan_boxes(boxes, o, inv, s.box_bounds, s.n_boxes);
			}
			float distance;
			uint32_t index;
			vec3 normal;
			float4 shading;
			uint32_t scatter;
			const uint32_t kind = select_hit(spheres, planes, boxes, distance, index);
			fetch_hit<false>(s, s.box_bounds, o, d, inv, kind, distance, index, normal, shading, scatter);
			if (!kind)
				normal = { 0.0f, 0.0f, 0.0f };
			out_distance[i] = distance;
			out_kind[i] = kind;
			out_index[i] = kind ? index : 0u;
			out_normal[i * 3 + 0] = normal.x;
			out_normal[i * 3 + 1] = normal.y;
			out_normal[i * 3 + 2] = normal.z;
		}
	}

	__global__ void kat_sqrt_div(uint32_t n, const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out_sqrt, float* __restrict__ out_div)
	{
		const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
		if (i < n)
		{
			out_sqrt[i] = __builtin_sqrtf(a[i]);
			out_div[i] = a[i] / b[i];
		}
	}

	// RT_HIP_FLAG_DIRECT_LIGHT's rules header as the render kernels run it (the contract's inv_sqrt_rn handed in)
	__global__ void kat_direct_octahedral(uint32_t n, const uint32_t* __restrict__ ka, const uint32_t* __restrict__ kb, float* __restrict__ out)
	{
		const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
		if (i < n)
		{
			float l2;
			const vec3 p = direct_light::octahedral_point<vec3>(ka[i], kb[i], l2);
			out[4u * i + 0u] = p.x, out[4u * i + 1u] = p.y, out[4u * i + 2u] = p.z, out[4u * i + 3u] = l2;
		}
	}
	__global__ void kat_direct_aim(uint32_t n, const uint32_t* __restrict__ ka, const uint32_t* __restrict__ kb, const float* __restrict__ in, const float* __restrict__ radius, uint32_t n_lights, float* __restrict__ out)
	{
		const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
		if (i < n)
		{
			const float* const v = in + 9u * i;
			const direct_light::aim<vec3> a = direct_light::aim_at(ka[i], kb[i], vec3{ v[0], v[1], v[2] }, vec3{ v[3], v[4], v[5] }, vec3{ v[6], v[7], v[8] }, radius[i], n_lights, contract_inv_sqrt{});
			out[5u * i + 0u] = a.w.x, out[5u * i + 1u] = a.w.y, out[5u * i + 2u] = a.w.z, out[5u * i + 3u] = a.weight, out[5u * i + 4u] = a.aimed ? 1.0f : 0.0f;
		}
	}

	// RT_HIP_FLAG_THIN_LENS's rules header as the lens builds of the render kernels run it: the disk point of each pair of numerators, and the
	// ray (in[0..2] origin, in[3..5] normalised direction, in[6..8] eye) bent through it by the lens words in[9..18], normalised as the
	// kernels' tail normalises a new direction
	__global__ void kat_lens(uint32_t n, const uint32_t* __restrict__ ka, const uint32_t* __restrict__ kb, const float* __restrict__ in, float* __restrict__ out)
	{
		const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
		if (i < n)
		{
			const lens::disk_point on_disk = lens::disk(ka[i], kb[i]);
			const vec3 o = { in[0], in[1], in[2] }, d = { in[3], in[4], in[5] }, eye = { in[6], in[7], in[8] };
			const lens::words<vec3> w = { { in[9], in[10], in[11] }, { in[12], in[13], in[14] }, { in[15], in[16], in[17] }, in[18] };
			const lens::bent_ray<vec3> bent = lens::bend(d, eye, w, on_disk);
			const vec3 origin = bent.bent ? bent.origin : o;
			const vec3 dir = bent.bent ? bent.toward * inv_sqrt_rn(dot(bent.toward, bent.toward)) : d;
			float* const r = out + 9u * i;
			r[0] = on_disk.x, r[1] = on_disk.y, r[2] = origin.x, r[3] = origin.y, r[4] = origin.z, r[5] = dir.x, r[6] = dir.y, r[7] = dir.z, r[8] = bent.bent ? 1.0f : 0.0f;
		}
	}

	// every one of the 2^32 binary32 bit patterns through sqrt_rn / rcp_rn / inv_sqrt_rn against hipcc's general
	// correctly rounded expansions (inv_sqrt_rn: against the contract's definition, evaluated through binary64);
	// result[2k] = mismatches, result[2k+1] = smallest mismatching input + 1
	__device__ __forceinline__ bool same_float(float a, float b)
	{
		return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b);
	}

	__global__ __launch_bounds__(block_threads) void kat_exhaustive_math(unsigned long long* __restrict__ result)
	{
		const uint32_t tid = blockIdx.x * block_threads + threadIdx.x; // 2^22 threads x 2^10 patterns each
		uint32_t bad[3] = { 0, 0, 0 };
		unsigned long long first[3] = { ~0ull, ~0ull, ~0ull };
		for (uint32_t k = 0; k < 1024u; k++)
		{
			const uint32_t bits = (k << 22) | tid;
			const float x = __uint_as_float(bits);
			const bool ok[3] = { same_float(sqrt_rn(x), __builtin_sqrtf(x)),
								 // (the plane test's form too, over the arguments its caller may hand it: not below 2^-60, or NaN)
								 same_float(rcp_rn(x), 1.0f / x) && (__builtin_fabsf(x) < 0x1p-60f || same_float(rcp_rn_not_tiny_where(x, true), 1.0f / x)),
								 same_float(inv_sqrt_rn(x), inv_sqrt_definition(x)) };
#pragma unroll
			for (int f = 0; f < 3; f++)
				if (!ok[f])
				{
					bad[f]++;
					if (static_cast<unsigned long long>(bits) + 1ull < first[f])
						first[f] = static_cast<unsigned long long>(bits) + 1ull;
				}
		}
#pragma unroll
		for (int f = 0; f < 3; f++)
			if (bad[f])
			{
				atomicAdd(&result[2 * f], static_cast<unsigned long long>(bad[f]));
				atomicMin(&result[2 * f + 1], first[f]);
			}
	}


static void launch_kat_random(uint32_t frame_key_a, uint32_t frame_key_b, uint32_t pixel, uint32_t sample, uint32_t n, float* d_out, hipStream_t stream)
{
	hipLaunchKernelGGL(kat_random, dim3(1), dim3(64), 0, stream, frame_keys{ frame_key_a, frame_key_b }, pixel, sample, n, d_out);
}

static void launch_kat_closest_hit(bool bvh,
							bool boxes,
							const device_scene& scene,
							const device_bvh& tree,
							uint32_t n,
							const float* d_origins,
							const float* d_directions,
							float* d_distance,
							uint32_t* d_kind,
							uint32_t* d_index,
							float* d_normal,
							hipStream_t stream)
{
	const dim3 grid((n + block_threads - 1) / block_threads);
	if (boxes)
		hipLaunchKernelGGL((kat_closest_hit<false, true>), grid, dim3(block_threads), 0, stream, scene, n, d_origins, d_directions, d_distance, d_kind, d_index, d_normal, tree);
	else if (bvh)
		hipLaunchKernelGGL(kat_closest_hit<true>, grid, dim3(block_threads), 0, stream, scene, n, d_origins, d_directions, d_distance, d_kind, d_index, d_normal, tree);
	else
		hipLaunchKernelGGL(kat_closest_hit<false>, grid, dim3(block_threads), 0, stream, scene, n, d_origins, d_directions, d_distance, d_kind, d_index, d_normal, tree);
}

static void launch_kat_closest_hit_box_tree(const device_scene& scene, const device_box_bvh& tree, uint32_t n, const float* d_origins, const float* d_directions, float* d_distance, uint32_t* d_kind, uint32_t* d_index, float* d_normal, hipStream_t stream)
{
	const dim3 grid((n + block_threads - 1) / block_threads);
	hipLaunchKernelGGL(kat_closest_hit_box_tree, grid, dim3(block_threads), 0, stream, scene, n, d_origins, d_directions, d_distance, d_kind, d_index, d_normal, tree);
}

static void launch_kat_sqrt_div(uint32_t n, const float* d_a, const float* d_b, float* d_sqrt, float* d_div, hipStream_t stream)
{
	const dim3 grid((n + block_threads - 1) / block_threads);
	hipLaunchKernelGGL(kat_sqrt_div, grid, dim3(block_threads), 0, stream, n, d_a, d_b, d_sqrt, d_div);
}

static void launch_kat_direct(uint32_t n, const uint32_t* d_ka, const uint32_t* d_kb, const float* d_in, const float* d_radius, uint32_t n_lights, float* d_out, hipStream_t stream)
{
	const dim3 grid((n + block_threads - 1) / block_threads);
	if (d_in)
		hipLaunchKernelGGL(kat_direct_aim, grid, dim3(block_threads), 0, stream, n, d_ka, d_kb, d_in, d_radius, n_lights, d_out);
	else
		hipLaunchKernelGGL(kat_direct_octahedral, grid, dim3(block_threads), 0, stream, n, d_ka, d_kb, d_out);
}

static void launch_kat_exhaustive_math(unsigned long long* d_result, hipStream_t stream)
{
	hipLaunchKernelGGL(kat_exhaustive_math, dim3((1u << 22) / block_threads), dim3(block_threads), 0, stream, d_result);
}

}
}

extern "C" const char* rt_hip_kat_last_error(void)
{
	return g_kat_error.c_str();
}

extern "C" rt_hip_status rt_hip_kat_random(rt_hip_ctx* ctx, uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t n, float* out)
{
	if (!ctx || !out || !n)
		return kat_fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_kat_random: invalid argument");
	RT_HIP_KAT_TRY(hipSetDevice(ctx->device));
	const size_t bytes = static_cast<size_t>(n) * sizeof(float);
	scratch s;
	RT_HIP_KAT_TRY(s.reserve(bytes));
	const frame_keys keys = make_frame_keys(seed);
	launch_kat_random(keys.a, keys.b, pixel, sample, n, s.device.as<float>(), nullptr);
	RT_HIP_KAT_TRY(hipGetLastError());
	RT_HIP_KAT_TRY(hipMemcpy(s.host.ptr, s.device.ptr, bytes, hipMemcpyDeviceToHost));
	std::memcpy(out, s.host.ptr, bytes);
	return RT_HIP_OK;
}

// bvh: 0 = the linear scan, 1 = the host builder's hierarchy, 2 = the device builder's, 3 = the linear scan with the scene's boxes,
// 4 = the linear scan with the scene's boxes through THEIR hierarchy (RT_HIP_FLAG_BOX_BVH)
static rt_hip_status closest_hit(int bvh,
								 rt_hip_ctx* ctx,
								 uint32_t n,
								 const float* origins,
								 const float* directions,
								 float* out_distance,
								 uint32_t* out_kind,
								 uint32_t* out_index,
								 float* out_normal)
{
	const bool boxes = bvh == 3, box_tree = bvh == 4;
	if (boxes || box_tree)
		bvh = 0;
	const char* const name = box_tree ? "rt_hip_kat_closest_hit_boxes_bvh" : boxes ? "rt_hip_kat_closest_hit_boxes" : (bvh == 2 ? "rt_hip_kat_closest_hit_bvh_device" : (bvh ? "rt_hip_kat_closest_hit_bvh" : "rt_hip_kat_closest_hit"));
	if (!ctx || !n || !origins || !directions || !out_distance || !out_kind || !out_index || !out_normal)
		return kat_fail(RT_HIP_INVALID_ARGUMENT, "%s: invalid argument", name);
	if (!ctx->have_scene)
		return kat_fail(RT_HIP_NO_SCENE, "%s: no scene uploaded", name);
	RT_HIP_KAT_TRY(hipSetDevice(ctx->device));
	const device_scene& scene = ctx->scene;
	if (boxes && scene.n_boxes > box_max_count)
		return kat_fail(RT_HIP_UNSUPPORTED, "%s: %u boxes (at most %u are traced)", name, scene.n_boxes, box_max_count);
	device_bvh tree_desc{};
	scratch tree_block;
	device_buffer device_tree, device_tree_scratch;
	struct release_device_tree
	{
		device_buffer &a, &b;
		~release_device_tree() { a.release(), b.release(); }
	} release_tree{ device_tree, device_tree_scratch };
	if (bvh == 2)
	{
		// the device builder's tree of the resident scene, used where it lies (the descriptor is read back for the kernel's argument)
		if (scene.n_spheres > lbvh::max_spheres)
			return kat_fail(RT_HIP_UNSUPPORTED, "%s: more than 2^26 spheres", name);
		const bvh_build_sizes sizes = bvh_build_sizes_for(scene.n_spheres);
		RT_HIP_KAT_TRY(device_tree.reserve(sizes.block_bytes));
		RT_HIP_KAT_TRY(device_tree_scratch.reserve(sizes.scratch_bytes));
		RT_HIP_KAT_TRY(tree_block.host.reserve(sizeof(device_bvh)));
		RT_HIP_KAT_TRY(build_bvh_device(scene.primitive_geometry, scene.n_spheres, device_tree.ptr, device_tree_scratch.ptr, nullptr));
		RT_HIP_KAT_TRY(hipMemcpy(tree_block.host.ptr, device_tree.ptr, sizeof(device_bvh), hipMemcpyDeviceToHost));
		std::memcpy(&tree_desc, tree_block.host.ptr, sizeof(device_bvh));
	}
	else if (bvh)
	{
		// the hierarchy of the resident scene, built as the render path builds it (scene.hip, ensure_bvh): from the table on the device
		const uint32_t spheres = scene.n_spheres;
		std::vector<float> geometry(static_cast<size_t>(spheres) * 4);
		if (spheres)
			RT_HIP_KAT_TRY(hipMemcpy(geometry.data(), scene.primitive_geometry, static_cast<size_t>(spheres) * sizeof(float4), hipMemcpyDeviceToHost));
		bvh_host tree;
		std::string why;
		if (!build_bvh(geometry.data(), spheres, tree, why))
			return kat_fail(RT_HIP_UNSUPPORTED, "%s: %s", name, why.c_str());
		const size_t nodes_bytes = tree.nodes.size() * 4, spheres_bytes = tree.spheres.size() * 4, order_bytes = tree.order.size() * 4, always_bytes = tree.always.size() * 4;
		const size_t total = nodes_bytes + spheres_bytes + order_bytes + always_bytes + 16;
		RT_HIP_KAT_TRY(tree_block.reserve(total));
		unsigned char* const h = tree_block.host.as<unsigned char>();
		std::memcpy(h, tree.nodes.data(), nodes_bytes);
		std::memcpy(h + nodes_bytes, tree.spheres.data(), spheres_bytes);
		std::memcpy(h + nodes_bytes + spheres_bytes, tree.order.data(), order_bytes);
		std::memcpy(h + nodes_bytes + spheres_bytes + order_bytes, tree.always.data(), always_bytes);
		RT_HIP_KAT_TRY(hipMemcpy(tree_block.device.ptr, h, total, hipMemcpyHostToDevice));
		const unsigned char* const d = tree_block.device.as<unsigned char>();
		tree_desc.nodes = reinterpret_cast<const float4*>(d);
		tree_desc.spheres = reinterpret_cast<const float4*>(d + nodes_bytes);
		tree_desc.order = reinterpret_cast<const uint32_t*>(d + nodes_bytes + spheres_bytes);
		tree_desc.always = reinterpret_cast<const uint32_t*>(d + nodes_bytes + spheres_bytes + order_bytes);
		tree_desc.root = tree.root;
		tree_desc.n_tree = static_cast<uint32_t>(tree.order.size());
		tree_desc.n_always = static_cast<uint32_t>(tree.always.size());
		tree_desc.cx = tree.centre[0], tree_desc.cy = tree.centre[1], tree_desc.cz = tree.centre[2], tree_desc.radius = tree.radius;
	}
	device_box_bvh box_desc{};
	if (box_tree)
	{
		// the box hierarchy of the resident scene, built as the render path builds it (scene.hip, ensure_box_bvh): from the pairs on the device
		const uint32_t count = scene.n_boxes;
		std::vector<float> bounds(static_cast<size_t>(count) * 8);
		if (count)
			RT_HIP_KAT_TRY(hipMemcpy(bounds.data(), scene.box_bounds, static_cast<size_t>(count) * 2u * sizeof(float4), hipMemcpyDeviceToHost));
		box_bvh_host tree;
		std::string why;
		if (!build_box_bvh(bounds.data(), count, tree, why))
			return kat_fail(RT_HIP_UNSUPPORTED, "%s: %s", name, why.c_str());
		const size_t nodes_bytes = tree.nodes.size() * 4, corners_bytes = tree.corners.size() * 4, order_bytes = tree.order.size() * 4, always_bytes = tree.always.size() * 4;
		const size_t total = nodes_bytes + corners_bytes + order_bytes + always_bytes + 16;
		RT_HIP_KAT_TRY(tree_block.reserve(total));
		unsigned char* const h = tree_block.host.as<unsigned char>();
		std::memcpy(h, tree.nodes.data(), nodes_bytes);
		std::memcpy(h + nodes_bytes, tree.corners.data(), corners_bytes);
		std::memcpy(h + nodes_bytes + corners_bytes, tree.order.data(), order_bytes);
		std::memcpy(h + nodes_bytes + corners_bytes + order_bytes, tree.always.data(), always_bytes);
		RT_HIP_KAT_TRY(hipMemcpy(tree_block.device.ptr, h, total, hipMemcpyHostToDevice));
		const unsigned char* const d = tree_block.device.as<unsigned char>();
		box_desc.nodes = reinterpret_cast<const float4*>(d);
		box_desc.corners = reinterpret_cast<const float4*>(d + nodes_bytes);
		box_desc.order = reinterpret_cast<const uint32_t*>(d + nodes_bytes + corners_bytes);
		box_desc.always = reinterpret_cast<const uint32_t*>(d + nodes_bytes + corners_bytes + order_bytes);
		box_desc.root = tree.root;
		box_desc.n_tree = static_cast<uint32_t>(tree.order.size());
		box_desc.n_always = static_cast<uint32_t>(tree.always.size());
	}
	const size_t vec_bytes = static_cast<size_t>(n) * 3 * sizeof(float);
	const size_t scalar_bytes = static_cast<size_t>(n) * sizeof(float);
	scratch in, out;
	RT_HIP_KAT_TRY(in.reserve(2 * vec_bytes));
	RT_HIP_KAT_TRY(out.reserve(vec_bytes + 3 * scalar_bytes));
	std::memcpy(in.host.as<unsigned char>(), origins, vec_bytes);
	std::memcpy(in.host.as<unsigned char>() + vec_bytes, directions, vec_bytes);
	RT_HIP_KAT_TRY(hipMemcpy(in.device.ptr, in.host.ptr, 2 * vec_bytes, hipMemcpyHostToDevice));
	unsigned char* const d_in = in.device.as<unsigned char>();
	unsigned char* const d_out = out.device.as<unsigned char>();
	float* d_distance = reinterpret_cast<float*>(d_out);
	uint32_t* d_kind = reinterpret_cast<uint32_t*>(d_out + scalar_bytes);
	uint32_t* d_index = reinterpret_cast<uint32_t*>(d_out + 2 * scalar_bytes);
	float* d_normal = reinterpret_cast<float*>(d_out + 3 * scalar_bytes);
	if (box_tree)
		launch_kat_closest_hit_box_tree(scene, box_desc, n, reinterpret_cast<const float*>(d_in), reinterpret_cast<const float*>(d_in + vec_bytes), d_distance, d_kind, d_index, d_normal, nullptr);
	else
		launch_kat_closest_hit(bvh != 0, boxes, scene, tree_desc, n, reinterpret_cast<const float*>(d_in), reinterpret_cast<const float*>(d_in + vec_bytes), d_distance, d_kind, d_index, d_normal, nullptr);
	RT_HIP_KAT_TRY(hipGetLastError());
	RT_HIP_KAT_TRY(hipMemcpy(out.host.ptr, out.device.ptr, vec_bytes + 3 * scalar_bytes, hipMemcpyDeviceToHost));
	const unsigned char* const h_out = out.host.as<unsigned char>();
	std::memcpy(out_distance, h_out, scalar_bytes);
	std::memcpy(out_kind, h_out + scalar_bytes, scalar_bytes);
	std::memcpy(out_index, h_out + 2 * scalar_bytes, scalar_bytes);
	std::memcpy(out_normal, h_out + 3 * scalar_bytes, vec_bytes);
	return RT_HIP_OK;
}

extern "C" rt_hip_status rt_hip_kat_closest_hit(rt_hip_ctx* ctx,
												uint32_t n,
												const float* origins,
												const float* directions,
												float* out_distance,
												uint32_t* out_kind,
												uint32_t* out_index,
												float* out_normal)
{
	return closest_hit(0, ctx, n, origins, directions, out_distance, out_kind, out_index, out_normal);
}

extern "C" rt_hip_status rt_hip_kat_closest_hit_bvh(rt_hip_ctx* ctx,
													uint32_t n,
													const float* origins,
													const float* directions,
													float* out_distance,
													uint32_t* out_kind,
													uint32_t* out_index,
													float* out_normal)
{
	return closest_hit(1, ctx, n, origins, directions, out_distance, out_kind, out_index, out_normal);
}

extern "C" rt_hip_status rt_hip_kat_closest_hit_boxes(rt_hip_ctx* ctx,
													  uint32_t n,
													  const float* origins,
													  const float* directions,
													  float* out_distance,
													  uint32_t* out_kind,
													  uint32_t* out_index,
													  float* out_normal)
{
	return closest_hit(3, ctx, n, origins, directions, out_distance, out_kind, out_index, out_normal);
}

extern "C" rt_hip_status rt_hip_kat_closest_hit_boxes_bvh(rt_hip_ctx* ctx,
															  uint32_t n,
															  const float* origins,
															  const float* directions,
															  float* out_distance,
															  uint32_t* out_kind,
															  uint32_t* out_index,
															  float* out_normal)
{
	return closest_hit(4, ctx, n, origins, directions, out_distance, out_kind, out_index, out_normal);
}

extern "C" rt_hip_status rt_hip_kat_box_bvh_builds(rt_hip_ctx* ctx, uint64_t* out_builds)
{
	if (!ctx || !out_builds)
		return kat_fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_kat_box_bvh_builds: NULL argument");
	*out_builds = ctx->box_bvh_builds;
	return RT_HIP_OK;
}

extern "C" rt_hip_status rt_hip_kat_box_bvh_build(const rt_hip_scene* scene, uint32_t out_counts[5], float* out_nodes, uint32_t* out_order, float* out_corners, uint32_t* out_always)
{
	if (!scene || !out_counts)
		return kat_fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_kat_box_bvh_build: NULL argument");
	const uint32_t n = scene->n_boxes;
	if (n && (!scene->box_center_x || !scene->box_center_y || !scene->box_center_z || !scene->box_extents_x || !scene->box_extents_y || !scene->box_extents_z || !scene->box_material))
		return kat_fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_kat_box_bvh_build: NULL box column");
	// the pairs as the upload derives them (scene.hip, build_image): corners = center -/+ extents, the material index riding in the spare lane
	std::vector<float> bounds(static_cast<size_t>(n) * 8, 0.0f);
	for (uint32_t i = 0; i < n; i++)
	{
		float* const b = &bounds[static_cast<size_t>(i) * 8];
		b[0] = scene->box_center_x[i] - scene->box_extents_x[i], b[1] = scene->box_center_y[i] - scene->box_extents_y[i], b[2] = scene->box_center_z[i] - scene->box_extents_z[i];
		b[4] = scene->box_center_x[i] + scene->box_extents_x[i], b[5] = scene->box_center_y[i] + scene->box_extents_y[i], b[6] = scene->box_center_z[i] + scene->box_extents_z[i];
		std::memcpy(&b[3], &scene->box_material[i], 4);
	}
	box_bvh_host tree;
	std::string why;
	if (!build_box_bvh(bounds.data(), n, tree, why))
		return kat_fail(RT_HIP_UNSUPPORTED, "rt_hip_kat_box_bvh_build: %s", why.c_str());
	out_counts[0] = static_cast<uint32_t>(tree.nodes.size() / 16);
	out_counts[1] = static_cast<uint32_t>(tree.order.size());
	out_counts[2] = static_cast<uint32_t>(tree.always.size());
	out_counts[3] = tree.depth;
	out_counts[4] = tree.root;
	if (out_nodes)
		std::memcpy(out_nodes, tree.nodes.data(), tree.nodes.size() * 4);
	if (out_order)
		std::memcpy(out_order, tree.order.data(), tree.order.size() * 4);
	if (out_corners)
		std::memcpy(out_corners, tree.corners.data(), tree.corners.size() * 4);
	if (out_always)
		std::memcpy(out_always, tree.always.data(), tree.always.size() * 4);
	return RT_HIP_OK;
}

extern "C" rt_hip_status rt_hip_kat_closest_hit_bvh_device(rt_hip_ctx* ctx,
														   uint32_t n,
														   const float* origins,
														   const float* directions,
														   float* out_distance,
														   uint32_t* out_kind,
														   uint32_t* out_index,
														   float* out_normal)
{
	return closest_hit(2, ctx, n, origins, directions, out_distance, out_kind, out_index, out_normal);
}

extern "C" rt_hip_status rt_hip_kat_bvh_build_device(rt_hip_ctx* ctx,
													 uint32_t out_counts[5],
													 float* out_nodes,
													 uint32_t* out_order,
													 float* out_spheres,
													 uint32_t* out_always,
													 float out_bound[4])
{
	if (!ctx || !out_counts)
		return kat_fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_kat_bvh_build_device: NULL argument");
	if (!ctx->have_scene)
		return kat_fail(RT_HIP_NO_SCENE, "rt_hip_kat_bvh_build_device: no scene uploaded");
	const uint32_t n = ctx->scene.n_spheres;
	if (n > lbvh::max_spheres)
		return kat_fail(RT_HIP_UNSUPPORTED, "rt_hip_kat_bvh_build_device: more than 2^26 spheres");
	RT_HIP_KAT_TRY(hipSetDevice(ctx->device));
	const bvh_build_sizes sizes = bvh_build_sizes_for(n);
	scratch tree, work; // (the host halves: the tree read back, and the build's header)
	RT_HIP_KAT_TRY(tree.reserve(sizes.block_bytes));
	RT_HIP_KAT_TRY(work.device.reserve(sizes.scratch_bytes));
	RT_HIP_KAT_TRY(work.host.reserve(sizeof(bvh_build_header)));
	RT_HIP_KAT_TRY(build_bvh_device(ctx->scene.primitive_geometry, n, tree.device.ptr, work.device.ptr, nullptr));
	RT_HIP_KAT_TRY(hipMemcpy(tree.host.ptr, tree.device.ptr, sizes.block_bytes, hipMemcpyDeviceToHost));
	RT_HIP_KAT_TRY(hipMemcpy(work.host.ptr, work.device.ptr, sizeof(bvh_build_header), hipMemcpyDeviceToHost));
	const unsigned char* const h = tree.host.as<unsigned char>();
	device_bvh d;
	std::memcpy(&d, h, sizeof(d));
	const bvh_build_header& header = *work.host.as<bvh_build_header>();
	uint32_t depth = 0;
	for (uint32_t level = 1; level <= lbvh::max_depth; level++)
		if (header.level_count[level])
			depth = level;
	const uint32_t node_slots = d.n_tree > lbvh::leaf_spheres ? d.n_tree - 1u : 0u;
	out_counts[0] = node_slots;
	out_counts[1] = d.n_tree;
	out_counts[2] = d.n_always;
	out_counts[3] = depth;
	out_counts[4] = d.root;
	if (out_nodes)
		std::memcpy(out_nodes, h + sizes.nodes_at, static_cast<size_t>(node_slots) * 64u);
	if (out_order)
		std::memcpy(out_order, h + sizes.order_at, static_cast<size_t>(d.n_tree) * 4u);
	if (out_spheres)
		std::memcpy(out_spheres, h + sizes.spheres_at, static_cast<size_t>(d.n_tree) * 16u);
	if (out_always)
		std::memcpy(out_always, h + sizes.order_at + static_cast<size_t>(d.n_tree) * 4u, static_cast<size_t>(d.n_always) * 4u);
	if (out_bound)
		out_bound[0] = d.cx, out_bound[1] = d.cy, out_bound[2] = d.cz, out_bound[3] = d.radius;
	return RT_HIP_OK;
}

extern "C" rt_hip_status rt_hip_kat_bvh_build(const rt_hip_scene* scene,
											  uint32_t out_counts[5],
											  float* out_nodes,
											  uint32_t* out_order,
											  float* out_spheres,
											  uint32_t* out_always,
											  float out_bound[4])
{
	if (!scene || !out_counts)
		return kat_fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_kat_bvh_build: NULL argument");
	const uint32_t n = scene->n_spheres;
	if (n && (!scene->sphere_center_x || !scene->sphere_center_y || !scene->sphere_center_z || !scene->sphere_radius))
		return kat_fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_kat_bvh_build: NULL sphere column");
	// the sphere rows of the primitive table as the upload derives them (scene.hip, build_image)
	std::vector<float> geometry(static_cast<size_t>(n) * 4);
	for (uint32_t i = 0; i < n; i++)
	{
		const float radius = scene->sphere_radius[i];
		geometry[i * 4 + 0] = scene->sphere_center_x[i];
		geometry[i * 4 + 1] = scene->sphere_center_y[i];
		geometry[i * 4 + 2] = scene->sphere_center_z[i];
		geometry[i * 4 + 3] = radius * radius;
	}
	bvh_host tree;
	std::string why;
	if (!build_bvh(geometry.data(), n, tree, why))
		return kat_fail(RT_HIP_UNSUPPORTED, "rt_hip_kat_bvh_build: %s", why.c_str());
	out_counts[0] = static_cast<uint32_t>(tree.nodes.size() / 16);
	out_counts[1] = static_cast<uint32_t>(tree.order.size());
	out_counts[2] = static_cast<uint32_t>(tree.always.size());
	out_counts[3] = tree.depth;
	out_counts[4] = tree.root;
	if (out_nodes)
		std::memcpy(out_nodes, tree.nodes.data(), tree.nodes.size() * 4);
	if (out_order)
		std::memcpy(out_order, tree.order.data(), tree.order.size() * 4);
	if (out_spheres)
		std::memcpy(out_spheres, tree.spheres.data(), tree.spheres.size() * 4);
	if (out_always)
		std::memcpy(out_always, tree.always.data(), tree.always.size() * 4);
	if (out_bound)
	{
		std::memcpy(out_bound, tree.centre, sizeof(tree.centre));
		out_bound[3] = tree.radius;
	}
	return RT_HIP_OK;
}

extern "C" rt_hip_status rt_hip_kat_sqrt_div(rt_hip_ctx* ctx, uint32_t n, const float* a, const float* b, float* out_sqrt, float* out_div)
{
	if (!ctx || !n || !a || !b || !out_sqrt || !out_div)
		return kat_fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_kat_sqrt_div: invalid argument");
	RT_HIP_KAT_TRY(hipSetDevice(ctx->device));
	const size_t bytes = static_cast<size_t>(n) * sizeof(float);
	scratch in, out;
	RT_HIP_KAT_TRY(in.reserve(2 * bytes));
	RT_HIP_KAT_TRY(out.reserve(2 * bytes));
	std::memcpy(in.host.as<unsigned char>(), a, bytes);
	std::memcpy(in.host.as<unsigned char>() + bytes, b, bytes);
	RT_HIP_KAT_TRY(hipMemcpy(in.device.ptr, in.host.ptr, 2 * bytes, hipMemcpyHostToDevice));
	unsigned char* const d_in = in.device.as<unsigned char>();
	unsigned char* const d_out = out.device.as<unsigned char>();
	launch_kat_sqrt_div(n, reinterpret_cast<const float*>(d_in), reinterpret_cast<const float*>(d_in + bytes), reinterpret_cast<float*>(d_out), reinterpret_cast<float*>(d_out + bytes), nullptr);
	RT_HIP_KAT_TRY(hipGetLastError());
	RT_HIP_KAT_TRY(hipMemcpy(out.host.ptr, out.device.ptr, 2 * bytes, hipMemcpyDeviceToHost));
	std::memcpy(out_sqrt, out.host.ptr, bytes);
	std::memcpy(out_div, out.host.as<unsigned char>() + bytes, bytes);
	return RT_HIP_OK;
}

// kat_fast.hip: this library's one unit built with the Makefile's FASTFLAGS — contract.hpp's fast leaf functions, one thread per element
namespace rt_hip
{
	void launch_kat_fast_math(uint32_t n, const float* d_x, const float* d_y, float* d_sqrt, float* d_rcp, float* d_rsq, float* d_div, hipStream_t stream);
}

extern "C" rt_hip_status rt_hip_kat_fast_math(rt_hip_ctx* ctx, uint32_t n, const float* x, const float* y, float* out_sqrt, float* out_rcp, float* out_rsq, float* out_div)
{
	if (!ctx || !n || !x || !y || !out_sqrt || !out_rcp || !out_rsq || !out_div)
		return kat_fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_kat_fast_math: invalid argument");
	RT_HIP_KAT_TRY(hipSetDevice(ctx->device));
	const size_t bytes = static_cast<size_t>(n) * sizeof(float);
	scratch in, out;
	RT_HIP_KAT_TRY(in.reserve(2 * bytes));
	RT_HIP_KAT_TRY(out.reserve(4 * bytes));
	std::memcpy(in.host.as<unsigned char>(), x, bytes);
	std::memcpy(in.host.as<unsigned char>() + bytes, y, bytes);
	RT_HIP_KAT_TRY(hipMemcpy(in.device.ptr, in.host.ptr, 2 * bytes, hipMemcpyHostToDevice));
	const float* const d_in = in.device.as<float>();
	float* const d_out = out.device.as<float>();
	launch_kat_fast_math(n, d_in, d_in + n, d_out, d_out + n, d_out + 2 * static_cast<size_t>(n), d_out + 3 * static_cast<size_t>(n), nullptr);
	RT_HIP_KAT_TRY(hipGetLastError());
	RT_HIP_KAT_TRY(hipMemcpy(out.host.ptr, out.device.ptr, 4 * bytes, hipMemcpyDeviceToHost));
	float* const results[4] = { out_sqrt, out_rcp, out_rsq, out_div };
	for (size_t k = 0; k < 4; k++)
		std::memcpy(results[k], out.host.as<unsigned char>() + k * bytes, bytes);
	return RT_HIP_OK;
}

// both entries of RT_HIP_FLAG_DIRECT_LIGHT's rules: in = NULL is the octahedral map (4 floats out per item), else the aim (5 floats out)
static rt_hip_status kat_direct(const char* name, rt_hip_ctx* ctx, uint32_t n, const uint32_t* ka, const uint32_t* kb, const float* in, const float* radius, uint32_t n_lights, float* out)
{
	if (!ctx || !n || !ka || !kb || !out || (in && (!radius || n_lights < 1u || n_lights > direct_light::max_sampled_lights)))
		return kat_fail(RT_HIP_INVALID_ARGUMENT, "%s: invalid argument", name);
	for (uint32_t i = 0; i < n; i++)
		if ((ka[i] | kb[i]) >> 24)
			return kat_fail(RT_HIP_INVALID_ARGUMENT, "%s: item %u: a numerator must be below 2^24", name, i);
	RT_HIP_KAT_TRY(hipSetDevice(ctx->device));
	const size_t words = static_cast<size_t>(n) * 4u, in_bytes = 2u * words + (in ? static_cast<size_t>(n) * 40u : 0u), out_bytes = static_cast<size_t>(n) * (in ? 20u : 16u);
	scratch input, output;
	RT_HIP_KAT_TRY(input.reserve(in_bytes));
	RT_HIP_KAT_TRY(output.reserve(out_bytes));
	unsigned char* const host = input.host.as<unsigned char>();
	std::memcpy(host, ka, words);
	std::memcpy(host + words, kb, words);
	if (in)
	{
		std::memcpy(host + 2u * words, in, static_cast<size_t>(n) * 36u);
		std::memcpy(host + 2u * words + static_cast<size_t>(n) * 36u, radius, words);
	}
	RT_HIP_KAT_TRY(hipMemcpy(input.device.ptr, input.host.ptr, in_bytes, hipMemcpyHostToDevice));
	const unsigned char* const d = input.device.as<unsigned char>();
	launch_kat_direct(n, reinterpret_cast<const uint32_t*>(d), reinterpret_cast<const uint32_t*>(d + words), in ? reinterpret_cast<const float*>(d + 2u * words) : nullptr,
					  in ? reinterpret_cast<const float*>(d + 2u * words + static_cast<size_t>(n) * 36u) : nullptr, n_lights, output.device.as<float>(), nullptr);
	RT_HIP_KAT_TRY(hipGetLastError());
	RT_HIP_KAT_TRY(hipMemcpy(output.host.ptr, output.device.ptr, out_bytes, hipMemcpyDeviceToHost));
	std::memcpy(out, output.host.ptr, out_bytes);
	return RT_HIP_OK;
}

extern "C" rt_hip_status rt_hip_kat_direct_octahedral(rt_hip_ctx* ctx, uint32_t n, const uint32_t* ka, const uint32_t* kb, float* out)
{
	return kat_direct("rt_hip_kat_direct_octahedral", ctx, n, ka, kb, nullptr, nullptr, 1u, out);
}

extern "C" rt_hip_status rt_hip_kat_direct_aim(rt_hip_ctx* ctx, uint32_t n, const uint32_t* ka, const uint32_t* kb, const float* in, const float* radius, uint32_t n_lights, float* out)
{
	if (!in)
		return kat_fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_kat_direct_aim: invalid argument");
	return kat_direct("rt_hip_kat_direct_aim", ctx, n, ka, kb, in, radius, n_lights, out);
}

extern "C" rt_hip_status rt_hip_kat_lens(rt_hip_ctx* ctx, uint32_t n, const uint32_t* ka, const uint32_t* kb, const float* ray, const float* lens_words, float* out)
{
	if (!ctx || !n || !ka || !kb || !ray || !lens_words || !out)
		return kat_fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_kat_lens: invalid argument");
	for (uint32_t i = 0; i < n; i++)
		if ((ka[i] | kb[i]) >> 24)
			return kat_fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_kat_lens: item %u: a numerator must be below 2^24", i);
	RT_HIP_KAT_TRY(hipSetDevice(ctx->device));
	const size_t words = static_cast<size_t>(n) * 4u, in_bytes = 2u * words + 19u * sizeof(float), out_bytes = static_cast<size_t>(n) * 9u * sizeof(float);
	scratch input, output;
	RT_HIP_KAT_TRY(input.reserve(in_bytes));
	RT_HIP_KAT_TRY(output.reserve(out_bytes));
	unsigned char* const host = input.host.as<unsigned char>();
	std::memcpy(host, ka, words);
	std::memcpy(host + words, kb, words);
	std::memcpy(host + 2u * words, ray, 9u * sizeof(float));
	std::memcpy(host + 2u * words + 9u * sizeof(float), lens_words, 10u * sizeof(float));
	RT_HIP_KAT_TRY(hipMemcpy(input.device.ptr, input.host.ptr, in_bytes, hipMemcpyHostToDevice));
	const unsigned char* const d = input.device.as<unsigned char>();
	hipLaunchKernelGGL(kat_lens, dim3((n + block_threads - 1) / block_threads), dim3(block_threads), 0, nullptr, n, reinterpret_cast<const uint32_t*>(d), reinterpret_cast<const uint32_t*>(d + words),
					   reinterpret_cast<const float*>(d + 2u * words), output.device.as<float>());
	RT_HIP_KAT_TRY(hipGetLastError());
	RT_HIP_KAT_TRY(hipMemcpy(output.host.ptr, output.device.ptr, out_bytes, hipMemcpyDeviceToHost));
	std::memcpy(out, output.host.ptr, out_bytes);
	return RT_HIP_OK;
}

extern "C" rt_hip_status rt_hip_kat_exhaustive_math(rt_hip_ctx* ctx, uint64_t out_mismatches[3], uint32_t out_first[3])
{
	if (!ctx || !out_mismatches || !out_first)
		return kat_fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_kat_exhaustive_math: NULL argument");
	RT_HIP_KAT_TRY(hipSetDevice(ctx->device));
	scratch s;
	RT_HIP_KAT_TRY(s.reserve(6 * sizeof(unsigned long long)));
	unsigned long long* const host = s.host.as<unsigned long long>();
	const unsigned long long initial[6] = { 0, ~0ull, 0, ~0ull, 0, ~0ull };
	std::memcpy(host, initial, sizeof(initial));
	RT_HIP_KAT_TRY(hipMemcpy(s.device.ptr, host, sizeof(initial), hipMemcpyHostToDevice));
	launch_kat_exhaustive_math(s.device.as<unsigned long long>(), nullptr);
	RT_HIP_KAT_TRY(hipGetLastError());
	RT_HIP_KAT_TRY(hipMemcpy(host, s.device.ptr, sizeof(initial), hipMemcpyDeviceToHost));
	for (int f = 0; f < 3; f++)
	{
		out_mismatches[f] = host[2 * f];
		out_first[f] = host[2 * f] ? static_cast<uint32_t>(host[2 * f + 1] - 1ull) : 0u;
	}
	return RT_HIP_OK;
}

#ifdef RT_HIP_REGION_COUNTERS
// experiment variant only: out[0..12] = runs, out[13..25] = lanes of the most recent launch on this context
extern "C" __attribute__((visibility("default"))) rt_hip_status rt_hip_debug_region_counters(rt_hip_ctx* ctx, uint64_t* out)
{
	if (!ctx || !out)
		return kat_fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_debug_region_counters: NULL argument");
	RT_HIP_KAT_TRY(hipSetDevice(ctx->device));
	RT_HIP_KAT_TRY(hipEventSynchronize(ctx->counters_copied));
	for (unsigned i = 0; i < device_counters::regions; i++)
	{
		out[i] = ctx->counters_host->region_runs[i];
		out[device_counters::regions + i] = ctx->counters_host->region_lanes[i];
	}
	return RT_HIP_OK;
}
#endif

#ifdef RT_HIP_WAVE_CLOCKS
// experiment variant only: out[3 * w + {0, 1, 2}] = start / queue-dry / end tick (100 MHz) of wave w of the most recent
// persistent launch on this context, for w < *count (in: capacity of `out` in waves; out: waves the build records)
extern "C" __attribute__((visibility("default"))) rt_hip_status rt_hip_debug_wave_clocks(rt_hip_ctx* ctx, uint64_t* out, uint32_t* count)
{
	if (!ctx || !out || !count)
		return kat_fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_debug_wave_clocks: NULL argument");
	RT_HIP_KAT_TRY(hipSetDevice(ctx->device));
	RT_HIP_KAT_TRY(hipEventSynchronize(ctx->counters_copied));
	const uint32_t n = std::min<uint32_t>(*count, device_counters::clocked_waves);
	for (uint32_t w = 0; w < n; w++)
		for (int k = 0; k < 3; k++)
			out[3 * w + k] = ctx->counters_host->wave_clocks[w][k];
	*count = n;
	return RT_HIP_OK;
}
#endif
