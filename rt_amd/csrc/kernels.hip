// rt_amd/csrc/kernels.hip — the gfx950 kernels of the mg_ray_tracer path.
//
// What runs here is the whole of reference src/renderers/mg_ray_tracer.cpp:178-205 for one frame: the per-pixel
// worker (:182-201), trace (:155-174), the closest-hit scans (:36-102) and the scatter functions (:110-140).
//
// Execution model (MI355X / CDNA4, 64-wide waves, 256-thread workgroups = 4 waves):
//   * a lane traces one ray at a time; the unit of work is one CHUNK of 16 consecutive samples of one pixel (the
//     arithmetic contract sums a pixel chunk-wise: each chunk in sample order, chunk sums in chunk order);
//   * a wave owns a small pixel tile (2x2 ... 8x8) and works through a queue of its (pixel, chunk) items: a lane pulls
//     the next item when it finishes one (ballot + mbcnt, no atomics), parks the chunk sum in a wave-private LDS slot,
//     and at the end the pixels' slots are folded in chunk order and stored.  Short items keep all lanes busy and
//     keep waves short, so that a launch has tens of thousands of waves to balance over the 1024 SIMDs;
//   * the (sample, bounce) double loop is FLATTENED: each loop trip advances every lane by one path segment.  A trip is
//     closest-hit query -> a miss ends the sample (sky) -> free lanes pull items -> ONE fused tail for "scatter a hit"
//     and "start the next sample" (both consume random draws and end in the normalisation of a direction: issued
//     once for the wave; only what really differs runs under its own lane mask);
//   * the closest-hit scan reads every primitive with a WAVE-UNIFORM operand and skips a primitive's square-root half
//     when no lane of the wave can hit it (ballots combined on the scalar unit);
//   * one kernel template, its modes chosen by scene size:
//       small    (<= 8 spheres, no planes: basic.toml, dielectric.toml): the spheres arrive as kernel arguments and
//                live in SGPRs; the scan is fully unrolled straight-line code with scalar operands; only the
//                per-lane lookups of the winning sphere go through LDS;
//       resident (<= 1024 primitives): all primitives are staged ONCE per workgroup into LDS as float4s; the scan
//                reads them as broadcast ds_read_b128 (no bank conflicts), four spheres per group;
//       tiled    (anything larger): primitives stream from the SoA columns in HBM/L2 through one LDS tile of 1024
//                shared by the workgroup's waves (coalesced dword loads per column, radius squared on the way in);
//                the workgroup moves in lock step, one path segment per trip, with barriers around each tile;
//       streamed (larger scenes from 32 samples per pixel): the resident loop reading the primitive table with
//                wave-uniform scalar loads from HBM/L2, the next group's load issued before this group's probes; a
//                wave left with a handful of rays walks the table once per ray with all 64 lanes instead.
//     The two big-scene modes are launched persistent and draw single (pixel, chunk) items from ONE launch-wide
//     sequence; a pixel's chunk sums meet in HBM ("rolling items", see render_queue): there a trip costs one scan
//     over all primitives whatever the number of lanes holding a ray, so lane occupancy is everything — and so is
//     that the whole launch runs dry at one moment.
// No MFMA: this is intersection arithmetic (subtract / dot / compare / sqrt), not a contraction.
//
// This file is compiled TWICE into librt_hip.so: as it stands (the parity contract: -ffp-contract=off, exactly rounded
// square roots and quotients), and with -DRT_HIP_FAST_BUILD -ffp-contract=fast (RT_HIP_FLAG_FAST: contract.hpp's
// hardware approximations), where it provides launch_render_fast() and nothing else.
//
// What is launched is decided elsewhere: launch_plan.cpp (plan_launch: which kernel, which build, queue shape, grid, LDS — host-only
// policy, tested on the CPU).  This file holds the kernels and the dispatch from a plan's kernel_build to the instantiation.
// What render_queue is made of lies in headers by subject: queue_build.hpp (every build's properties, and the argument words that mean
// different things per build), scan.hpp / scan_streamed.hpp / bvh_scan.hpp / box_bvh_scan.hpp (the closest-hit scans), camera_forms.hpp
// and lane_state.hpp (what a lane carries, what a pixel's samples start from), handover.hpp (the rolling kernels' cross-wave protocol),
// pixel_output.hpp (rows, finishing a pixel, the segment count).
#include "kernels.hpp"
#include "contract.hpp"
#include "scan.hpp"
#include "bvh_scan.hpp"
#include "box_bvh_scan.hpp"
#include "scan_streamed.hpp"
#include "handover.hpp"
#include "pixel_output.hpp"
#include "lane_state.hpp"
#include "queue_build.hpp"
#include "direct_light_rules.hpp"
#include "camera_forms.hpp"
// (RT_HIP_FLAG_THIN_LENS's rules take their leaf function from the includer: the contract's correctly rounded quotient)
namespace rt_hip::lens::leaf
{
	__device__ __forceinline__ float divide(float a, float b) { return rt_hip::divide(a, b); }
}
#include "lens_rules.hpp"

#ifdef RT_HIP_FAST_BUILD
#define render_queue render_queue_fast
#define launch_render launch_render_fast
#endif

#include "../../include/rt_hip.h"

#include <algorithm>

// Region counters (tools/region_profile.py; built only as an experiment variant, never in the product): how often each
// part of a loop trip runs and with how many lanes — the dynamic side of profiles/r02/isa_trip_breakdown.txt.
#ifdef RT_HIP_REGION_COUNTERS
#define RT_HIP_REGION(i)                                                                                               \
	do                                                                                                                 \
	{                                                                                                                  \
		region_runs[i] += 1u;                                                                                          \
		region_lanes[i] += static_cast<uint32_t>(__builtin_popcountll(__builtin_amdgcn_ballot_w64(true)));             \
	}                                                                                                                  \
	while (false)
#else
#define RT_HIP_REGION(i) ((void)0)
#endif

namespace rt_hip
{
	static_assert(bvh_stack_float4s * 4u == bvh_max_depth * block_threads, "the BVH kernel's LDS stacks hold bvh_max_depth words per thread");

	namespace
	{
		// ---- small / resident kernel: a wave works through a queue of (pixel, sample chunk) items -----------------------
		//
		// The pixel sum is defined chunk-wise (arithmetic contract: chunks of 16 consecutive samples, each summed in
		// sample order, chunk sums added in chunk order).  That makes ONE CHUNK the unit of work: a wave owns a small
		// tile of P pixels = P x K items (K = chunks per pixel); its 64 lanes pull items from the wave's queue as they
		// finish the previous one, park every chunk sum in a wave-private LDS slot, and at the end P lanes fold the
		// slots in chunk order and write the pixels.  Short items keep every lane busy until the queue is empty and
		// keep waves short, so that a launch has tens of thousands of them to balance over the chip; which lane
		// computes which chunk cannot change a result.
		//
		// The builds — SCAN (the scan proper NS and its pass / adaptive / box / box-tree / light builds), HALF, NP, GC — and every property the
		// body branches on: queue_build.hpp, one paragraph each.  SM: scatter table of sm_ray_tracer (RT_HIP_FLAG_SM_MATERIALS) instead of
		// mg_ray_tracer's.
		//
		// ROLLING ITEMS (NS < 0).  In a big scene a trip is one closest-hit scan over all primitives — the same cost for a
		// wave with one lane holding a ray as for a wave with 64 — so what matters is that every lane holds a ray in every
		// trip, and that all waves of the launch run dry at the same moment.  The big-scene kernels are therefore launched
		// persistent, and their unit of hand-out is the single ITEM: all (pixel, chunk) items of this rank's rows form ONE
		// launch-wide sequence (pixel-major, bottom row first); a wave draws small blocks of consecutive items from one
		// counter — one block ahead, so that the atomic's latency is off the path — and gives them to its lanes as they
		// fall free, in the same trip.  A pixel's chunks may end up in different waves, on different CUs and XCDs: every
		// finished chunk sum goes to a scratch slot in HBM (write-through stores, drained), then the pixel's arrival
		// counter is incremented; whoever brings the LAST chunk of a pixel reads all of them back (loads that bypass the
		// non-coherent caches), folds them in chunk order and writes the pixel.  Which lane of which wave that is cannot
		// change a bit of the result.
		// Round 2 handed out pixel TILES (128 items, two open per wave, sums in LDS).  Measured with per-wave clocks on the
		// 100 000-sphere frame (profiles/r03/config5_streamed/wave_tail_*.txt): the queue ran dry after 74 % of the launch
		// and a wave then still owned up to 256 items — four rounds of 34 trips for its lanes — so 20 % of all wave-time
		// was spent waiting for the slowest waves.  With items the stragglers' excess is one item, not four tiles' worth.
		// (For small scenes the per-trip cost is the shading code, and lanes that never start together lose the phase
		// coherence that keeps it short — profiles/r01/queue_shape_sweep.txt.  They keep one tile per wave.)
		template <int SCAN, bool SM, bool HALF = false, int NP = 0, bool GC = false>
		__global__ __launch_bounds__(block_threads, (queue_build<SCAN, HALF, NP, GC>::waves)) void render_queue(const frame_params p,
																	  const queue_params q,
																	  const small_scene small,
																	  const device_scene s,
																	  const float4* __restrict__ geometry, // = s.primitive_geometry, as a plain read-only argument
																	  uint32_t* __restrict__ out_rgba,
																	  float* __restrict__ out_rgb,
																	  device_counters* __restrict__ counters,
																	  unsigned long long* item_sums, // [NS < 0] chunk sums in transit: 16 bytes per item; [NS == scan_bvh] the device_bvh
																									 // descriptor (rolling_buffers::bvh)
																	  uint32_t* pixel_done)			 // [NS < 0] items arrived per pixel (zeroed in front of every launch); [PASS] the accumulator
		{
			// what this build is (queue_build.hpp has the why of each)
			using build = queue_build<SCAN, HALF, NP, GC>;
			constexpr int NS = build::NS;
			constexpr bool PASS = build::PASS, ADAPT = build::ADAPT, BOXES = build::BOXES, BOXTREE = build::BOXTREE, LIGHTS = build::LIGHTS, DIRECT = build::DIRECT;
			constexpr bool LENS = build::LENS; // (RT_HIP_FLAG_THIN_LENS, DESIGN.md §3.17: the restart's second step and the lens ray)
			constexpr bool RESIDENT = build::RESIDENT, RESIDENT_SCALAR_SCAN = build::RESIDENT_SCALAR_SCAN, BVH = build::BVH, ROLLING = build::ROLLING;
			constexpr bool INDEXED = build::INDEXED, SCALAR_SEGMENTS = build::SCALAR_SEGMENTS;
			constexpr uint32_t slot_floats = build::slot_floats;
			// (the camera form per build: the restart below selects as camera_forms.hpp does.  Its three branches stay in the body, selection
			// included — as functions of that header they moved the instructions of 133 to 211 kernels)
			constexpr bool PINHOLE_ONLY = build::PINHOLE_ONLY, EYE_ONLY = build::EYE_ONLY, NEVER_PINHOLE = build::NEVER_PINHOLE;
			extern __shared__ float4 lds[];
			// [NS > 0] 8 geometry (with the scatter function) + 8 shading float4s | [NS == scan_resident] all primitives; then the chunk slots
			float4* const lds_geometry = lds;
			float4* const lds_shading = lds + scalar_max_spheres;
			const bool spheres_in_lds = RESIDENT && !RESIDENT_SCALAR_SCAN;
			const uint32_t lds_spheres = spheres_in_lds ? s.n_spheres : 0u;
			uint32_t table_float4s = NS > 0 ? small_table_float4s : (RESIDENT ? lds_spheres + s.n_planes : (NS == scan_tiled ? tile_primitives : (BVH ? bvh_stack_float4s : 0u)));
			// [BOXES] the boxes' corners behind that table (launch_plan.cpp: at most box_max_count, and the whole within a workgroup's LDS)
			float4* const lds_boxes = lds + table_float4s;
			if constexpr (BOXES && !BOXTREE)
				table_float4s += 2u * s.n_boxes;
			if (NS > 0)
			{
				if (threadIdx.x == 0)
				{
#pragma unroll
					for (int i = 0; i < NS + NP; i++) // constant indices: the argument block is never indexed dynamically
					{
						// (what a hit looks up: the centre / the normal, and in the fourth word — the scan has radius^2 / d from the
						// scalar registers — the scatter function: ONE 16-byte read for both)
						lds_geometry[i] = make_float4(small.geometry[i].x, small.geometry[i].y, small.geometry[i].z, __uint_as_float(small.scatter[i]));
						lds_shading[i] = small.shading[i];
					}
				}
			}
			else if (RESIDENT)
			{
				for (uint32_t i = threadIdx.x; i < lds_spheres + s.n_planes; i += block_threads)
					lds[i] = s.primitive_geometry[(s.n_spheres - lds_spheres) + i];
			}
			if constexpr (BOXES && !BOXTREE)
			{
				for (uint32_t i = threadIdx.x; i < 2u * s.n_boxes; i += block_threads)
					lds_boxes[i] = s.box_bounds[i];
			}
			__syncthreads();

#ifdef RT_HIP_REGION_COUNTERS
			uint32_t region_runs[device_counters::regions] = {}, region_lanes[device_counters::regions] = {};
#endif
			// what travels to this build in argument words it does not otherwise read.  (`PASS ? .. : 0`: where the build has no use for a word its
			// name stays a constant, which no lambda below captures.)
			const queue_words words = unpack_words<build>(q, item_sums, pixel_done);
			const uint32_t first_chunk = PASS ? words.first_chunk : 0u;
			float* const accum = PASS ? words.accum : nullptr;
			// [BVH] the hierarchy, read once into scalar registers (its pointers and counts are the same for the whole launch)
			device_bvh bvh{};
			if constexpr (BVH)
				bvh = *words.bvh;
			// [BOXTREE] ... and the boxes' hierarchy
			device_box_bvh box_tree{};
			if constexpr (BOXTREE)
				box_tree = *words.box_tree;
			// [DIRECT] the sampled-light list in front of the light variant's shading table, and its count (wave-uniform: >= 1, the plan's rule)
			const float4* direct_list = nullptr;
			uint32_t direct_n = 0;
			if constexpr (DIRECT)
			{
				const unsigned char* const list = reinterpret_cast<const unsigned char*>(s.primitive_shading) - direct_list_bytes;
				direct_n = *reinterpret_cast<const uint32_t*>(list);
				direct_list = reinterpret_cast<const float4*>(list + direct_list_header_bytes);
			}
			const uint32_t lane = threadIdx.x & 63u;
			const uint32_t wave = threadIdx.x >> 6;
			const uint32_t chunk_items = q.chunks << q.pixels_log2;	   // chunks of one pixel tile: P x K
			const uint32_t items = HALF ? 2u * chunk_items : chunk_items; // work items of the tile
			// chunk-sum slots of this wave's tile (one tile per wave; the rolling kernels keep no sums in LDS)
			float* const slots = reinterpret_cast<float*>(lds + table_float4s) + static_cast<size_t>(wave) * chunk_items * slot_floats;
			const uint32_t tile_w = 1u << q.tile_w_log2;
			const uint32_t tile_h = (1u << q.pixels_log2) >> q.tile_w_log2;

			// one tile per wave: workgroups are handed out bottom row first — the lower part of a frame is usually the
			// expensive one (ground under sky), and starting with it keeps the cheap sky tiles for the tail.
			// Below a SKY BAND (sky_band.hpp; render.hip) the grid covers the rows under the band only, and the band's height — the first row
			// of this launch — arrives in q.block_items, a word the tile-per-wave builds that are no pass do not otherwise read (0 in every
			// other launch of theirs: kernels.hpp, rolling_buffers).  One scalar addition in front of the loop: every row this kernel
			// then speaks of is an image row, checked against p.local_rows = the frame's height.  (In global_row, where a multi-GPU
			// rank's rows become image rows, the same offset moved the register table of 126 of the 326 builds: DESIGN.md §5.)
			const uint32_t tile_x0 = (blockIdx.x * 4u + wave) * tile_w;
			const uint32_t tile_y0 = (gridDim.y - 1u - blockIdx.y) * tile_h + ((!ROLLING && !PASS) ? q.block_items : 0u);
			uint32_t next_item = 0; // wave-uniform queue head
			// [ADAPT] bit i: pixel i of this wave's tile has stopped — not traced, not folded (wave-uniform: one ballot of the tile's state words)
			unsigned long long tile_stopped = 0;
			float* pass_sums = nullptr;
			if constexpr (ADAPT)
			{
				const adaptive_words adaptive = unpack_adaptive_words(accum, p);
				pass_sums = adaptive.pass_sums;
				const uint32_t lx = tile_x0 + (lane & (tile_w - 1u));
				const uint32_t ly = tile_y0 + (lane >> q.tile_w_log2);
				const bool in_frame = lane < (1u << q.pixels_log2) && lx < p.width && ly < p.local_rows;
				bool stopped = false;
				if (first_chunk && in_frame) // (the first pass reads nothing: every pixel is active)
					stopped = (adaptive.pixel_state[static_cast<size_t>(output_row(ly, p)) * p.width + lx] & 0x80000000u) != 0u;
				tile_stopped = __builtin_amdgcn_ballot_w64(stopped);
				if ((__builtin_amdgcn_ballot_w64(in_frame) & ~tile_stopped) == 0) // nothing to trace, nothing to fold (no barrier follows in these kernels)
					return;
			}

			// rolling items: the launch-wide sequence, the block this wave is handing out, the block drawn ahead
			// rolling + HALF: a pixel is cut into items of q.item_samples consecutive samples, whatever the chunks are
			const uint32_t items_per_pixel = (ROLLING && HALF) ? (p.samples_per_pixel + q.item_samples - 1u) / q.item_samples : q.chunks;
			const unsigned long long total_items = static_cast<unsigned long long>(p.width) * p.local_rows * items_per_pixel;
			unsigned long long block_next = 0, block_end = 0; // [block_next, block_end): not yet given to a lane
			unsigned long long prefetched = 0;				  // first item of the block after that
			uint32_t prefetched_count = ROLLING ? min(64u, q.lane_cap) : 64u; // (the first block is a whole wave's worth — or the wave's cap: every lane that may hold a ray starts at once)
			bool dry = false;								  // the launch-wide sequence has run out
			if (ROLLING)
				prefetched = fetch_items(counters, prefetched_count);
#ifdef RT_HIP_WAVE_CLOCKS
			const unsigned long long clock_start = wall_clock64();
			unsigned long long clock_dry = 0;
#endif

			lane_state st;
			// path segments traced: on the scalar unit (SCALAR_SEGMENTS) or per lane
			unsigned long long wave_segments = 0;
			uint32_t lane_segments = 0;
			uint32_t slot = 0; // chunk-sum slot of the item in flight on this lane; rolling: its pixel's place in the hand-out order
			// what the lane does in the current trip:
			//   free    - between items                       restart - has a sample to start (needs a primary ray)
			//   trace   - has a ray: closest-hit query next    retired - the queue ran dry
			// ONE register says both: 0 free, 1 restart, 3 retired, and from lane_trace (4) upwards "tracing, and the path may still
			// make (mode - 4) bounces after the segment in flight" — the bounce count of `if (!(max_bounces--)) return {}` (:157).  A
			// restart sets both with one move, a bounce takes one off, and the lane that would go below 4 has run out of bounces.
			// (Round 4 tried the mode as three lane MASKS kept in scalar registers instead of a number in a vector register: same
			// vector instruction count, 42 % more scalar ones, 2.64 -> 2.85 ms — profiles/r04/ab_mode_masks.txt, HISTORY.md.)
			enum : uint32_t { lane_free = 0, lane_restart = 1, lane_retired = 3, lane_trace = 4 };
			uint32_t mode = lane_free;
			// [DIRECT] what a lane carries besides: the direct light of the sample in flight; across a shadow query the contribution
			// that is added if the aimed sphere is visible, that sphere, and the vertex's normal; whether the query in flight IS a shadow query;
			// and whether the vertex the segment in flight leaves has sampled the lights itself
			vec3 direct_sum = { 0.0f, 0.0f, 0.0f }, pending = { 0.0f, 0.0f, 0.0f }, kept_normal = { 0.0f, 0.0f, 0.0f };
			uint32_t pending_sphere = 0;
			bool shadow = false, sampled_before = false;
#define RT_HIP_IS(m) ((m) == lane_trace ? mode >= lane_trace : mode == (m))
#define RT_HIP_BECOME(m) (mode = (m))

			// all items of a tile are in: fold the chunk sums of each pixel in chunk order and write it (:195-200)
			const auto fold_tile = [&](const float* sums, uint32_t x0, uint32_t y0)
			{
				if constexpr (ADAPT)
				{
					// The adaptive builds' fold, in a block of its own so that every other build's text stays what it was.  Per value — a
					// channel of a pixel where the tile has at most 16 pixels (lane = channel * P + pixel), else a pixel's three — the running sum
					// goes on as PASS's does and the pass's OWN fold (c0, + c1, ... in chunk order) is stored next to it; a stopped pixel is
					// neither read nor written; no pixel is finished.
					const bool by_channel = (3u << q.pixels_log2) <= 64u; // wave-uniform
					const uint32_t pixel = by_channel ? lane & ((1u << q.pixels_log2) - 1u) : lane;
					const uint32_t first_channel = by_channel ? lane >> q.pixels_log2 : 0u;
					const uint32_t channels = by_channel ? (first_channel < 3u ? 1u : 0u) : 3u;
					const uint32_t lx = x0 + (pixel & (tile_w - 1u));
					const uint32_t ly = y0 + (pixel >> q.tile_w_log2);
					if (pixel < (1u << q.pixels_log2) && lx < p.width && ly < p.local_rows && !((tile_stopped >> pixel) & 1ull))
					{
						const size_t at_pixel = (static_cast<size_t>(output_row(ly, p)) * p.width + lx) * 3u;
						for (uint32_t k = 0; k < channels; k++)
						{
							const uint32_t channel = first_channel + k;
							const float c0 = sums[pixel * 3u + channel];
							float own = c0;
							float sum = first_chunk ? accum[at_pixel + channel] + c0 : c0;
							for (uint32_t c = 1; c < q.chunks; c++)
							{
								const float next = sums[((c << q.pixels_log2) + pixel) * 3u + channel];
								sum = sum + next;
								own = own + next;
							}
							accum[at_pixel + channel] = sum;
							pass_sums[at_pixel + channel] = own;
						}
					}
					return;
				}
				if (!ROLLING && (3u << q.pixels_log2) <= 64u) // wave-uniform
				{
					// Small tiles (<= 16 pixels: from 113 samples per pixel upwards) are folded one CHANNEL per lane — lane
					// = channel * P + pixel — so that the chunk loop, the division by the sample count and the square
					// root are issued once for all three channels instead of three times by a third of the lanes.  Per
					// channel the arithmetic is what finish_pixel does; the packed bytes then meet in the pixel's lane.
					const uint32_t channel = lane >> q.pixels_log2;
					const uint32_t pixel = lane & ((1u << q.pixels_log2) - 1u);
					const uint32_t lx = x0 + (pixel & (tile_w - 1u));
					const uint32_t ly = y0 + (pixel >> q.tile_w_log2);
					const bool live = channel < 3u && lx < p.width && ly < p.local_rows;
					float sum = 0.0f;
					if (live)
					{
						if (HALF)
						{
							for (uint32_t c = 0; c < q.chunks; c++)
							{
								const float* const slot_of_chunk = sums + ((c << q.pixels_log2) + pixel) * slot_floats;
								float chunk_sum = slot_of_chunk[channel]; // samples 0..7 of the chunk, then 8.. in order
								const uint32_t parked = parked_samples(p.samples_per_pixel, c);
								for (uint32_t j = 0; j < parked; j++)
									chunk_sum = chunk_sum + slot_of_chunk[3u + j * 3u + channel];
								sum = c ? sum + chunk_sum : chunk_sum;
							}
						}
						else
						{
							sum = sums[pixel * 3u + channel];
							// [PASS] the pixel's running sum goes on from the earlier passes' chunks (pass 0: from the first chunk's sum, as in one shot)
							float* running = nullptr;
							if constexpr (PASS)
							{
								running = accum + (static_cast<size_t>(output_row(ly, p)) * p.width + lx) * 3u + channel;
								if (first_chunk)
									sum = *running + sum;
							}
							for (uint32_t c = 1; c < q.chunks; c++)
								sum = sum + sums[((c << q.pixels_log2) + pixel) * 3u + channel];
							if constexpr (PASS)
								*running = sum;
						}
					}
					const float mean = sum / static_cast<float>(p.samples_per_pixel);
					const size_t o = static_cast<size_t>(output_row(live ? ly : 0u, p)) * p.width + lx;
					if (live && out_rgb)
						out_rgb[o * 3u + channel] = mean;
					const uint32_t byte = static_cast<uint32_t>(clamp01(__builtin_sqrtf(mean)) * 255.99999f);
					const uint32_t green = __shfl(byte, lane + (1u << q.pixels_log2), 64);
					const uint32_t blue = __shfl(byte, lane + (2u << q.pixels_log2), 64);
					if (live && channel == 0u)
						__hip_atomic_store(&out_rgba[o], (byte << 24u) | (green << 16u) | (blue << 8u) | 255u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
					return;
				}
				for (uint32_t pixel = lane; pixel < (1u << q.pixels_log2); pixel += 64u)
				{
					const uint32_t lx = x0 + (pixel & (tile_w - 1u));
					const uint32_t ly = y0 + (pixel >> q.tile_w_log2);
					if (lx < p.width && ly < p.local_rows)
					{
						vec3 colour = { 0.0f, 0.0f, 0.0f };
						if (HALF)
						{
							for (uint32_t c = 0; c < q.chunks; c++)
							{
								const float* const slot_of_chunk = sums + ((c << q.pixels_log2) + pixel) * slot_floats;
								vec3 chunk_sum = { slot_of_chunk[0], slot_of_chunk[1], slot_of_chunk[2] };
								const uint32_t parked = parked_samples(p.samples_per_pixel, c);
								for (uint32_t j = 0; j < parked; j++)
									chunk_sum = chunk_sum + vec3{ slot_of_chunk[3u + j * 3u], slot_of_chunk[4u + j * 3u], slot_of_chunk[5u + j * 3u] };
								colour = c ? colour + chunk_sum : chunk_sum;
							}
						}
						else
						{
							colour = { sums[pixel * 3u], sums[pixel * 3u + 1u], sums[pixel * 3u + 2u] };
							float* running = nullptr;
							if constexpr (PASS)
							{
								running = accum + (static_cast<size_t>(output_row(ly, p)) * p.width + lx) * 3u;
								if (first_chunk)
									colour = vec3{ running[0], running[1], running[2] } + colour;
							}
							for (uint32_t c = 1; c < q.chunks; c++)
							{
								const uint32_t at = ((c << q.pixels_log2) + pixel) * 3u;
								colour = colour + vec3{ sums[at], sums[at + 1u], sums[at + 2u] };
							}
							if constexpr (PASS)
								running[0] = colour.x, running[1] = colour.y, running[2] = colour.z;
						}
						finish_pixel(colour, p, lx, ly, out_rgba, out_rgb);
					}
				}
			};
			// rolling: the lane's item is finished.  One chunk per pixel (<= 16 samples): the sum IS the pixel.  Otherwise the
			// sum is published, the pixel's arrival counter incremented, and the lane that brings the last chunk folds them.
			const auto complete_item = [&]()
			{
				const uint32_t row = slot / p.width; // hand-out order: bottom row first
				const uint32_t lx = slot - row * p.width;
				const uint32_t ly = p.local_rows - 1u - row;
				if (HALF)
				{
					// sub-chunk items: every sample's value went to its own place (end_sample); the lane that brings a pixel's
					// last item adds them up as the contract says — sixteen in sample order per chunk, chunks in chunk order
					unsigned long long* const samples = item_sums + 2u * static_cast<size_t>(slot) * p.samples_per_pixel;
					const uint32_t before = count_arrival(&pixel_done[slot]);
					if (before + 1u == items_per_pixel)
					{
						last_arrival();
						vec3 colour = { 0.0f, 0.0f, 0.0f };
						for (uint32_t first = 0; first < p.samples_per_pixel; first += sample_chunk)
						{
							const uint32_t end = min(first + sample_chunk, p.samples_per_pixel);
							vec3 chunk_sum = { 0.0f, 0.0f, 0.0f };
							uint32_t i = first;
							for (; i + 8u <= end; i += 8u) // eight loads in flight, then eight additions in sample order
							{
								vec3 value[8];
								read_sums8(samples + 2u * i, value);
#pragma unroll
								for (uint32_t k = 0; k < 8u; k++)
									chunk_sum = chunk_sum + value[k];
							}
							for (; i < end; i++)
								chunk_sum = chunk_sum + read_sum(samples + 2u * i);
							colour = first ? colour + chunk_sum : chunk_sum;
						}
						finish_pixel(colour, p, lx, ly, out_rgba, out_rgb); // (the counter stays: every launch zeroes its counters first)
					}
					return;
				}
				if (q.chunks == 1u) // (wave-uniform)
				{
					finish_pixel(st.chunk_sum, p, lx, ly, out_rgba, out_rgb);
					return;
				}
				const uint32_t chunk = (st.sample_end - 1u) / sample_chunk;
				unsigned long long* const sums = item_sums + 2u * static_cast<size_t>(slot) * q.chunks;
				publish_sum(sums + 2u * chunk, st.chunk_sum);
				const uint32_t before = count_arrival(&pixel_done[slot]);
				if (before + 1u == q.chunks)
				{
					last_arrival();
					vec3 colour = read_sum(sums);
					for (uint32_t c = 1; c < q.chunks; c++)
						colour = colour + read_sum(sums + 2u * c);
					finish_pixel(colour, p, lx, ly, out_rgba, out_rgb); // (the counter stays: every launch zeroes its counters first)
				}
			};

			// on to the next sample of the item in flight; false = that was the last one.  The lane's stream moves to the next
			// sample's window (a restarting lane has no other use for its position).  The kernels that look at a sample's INDEX
			// (half chunks park by it, rolling items publish by it) count indices; the others count windows only.
			const auto next_sample = [&]() -> bool
			{
#ifdef RT_HIP_FAST_BUILD
				st.window += st.keys.stride << draws_per_sample_log2;
#else
				// (written out with its result tied to its operand's register: hipcc otherwise forms the sum in the counter's register
				// and carries the window through two more moves to the end of the query)
				asm("v_lshl_add_u32 %0, %1, %2, %0" : "+v"(st.window) : "v"(st.keys.stride), "n"(draws_per_sample_log2));
#endif
				if (INDEXED)
					return ++st.sample < st.sample_end;
				return st.window != st.window_end;
			};

			// `colour += trace(...)` (:193) for the sample in flight, then the next sample of the chunk or the end of the item
			const auto end_sample = [&](vec3 contribution)
			{
				if constexpr (DIRECT) // `return direct + X`
				{
					contribution = direct_sum + contribution;
					direct_sum = { 0.0f, 0.0f, 0.0f };
					sampled_before = false;
				}
				if (HALF && ROLLING)
				{
					publish_sum(item_sums + 2u * (static_cast<size_t>(slot) * p.samples_per_pixel + st.sample), contribution);
					if (next_sample())
						RT_HIP_BECOME(lane_restart);
					else
					{
						complete_item();
						RT_HIP_BECOME(lane_free);
					}
					return;
				}
				if (HALF)
				{
					// slot = (half-chunk index << pixels_log2) + pixel; its chunk's LDS slot; sample bit 3 = second half
					const uint32_t half_chunk = slot >> q.pixels_log2;
					float* const slot_of_chunk = slots + ((((half_chunk >> 1u) << q.pixels_log2) + (slot & ((1u << q.pixels_log2) - 1u))) * slot_floats);
					if (st.sample & 8u) // second half: the sample's value is parked as it is
					{
						float* const place = slot_of_chunk + 3u + (st.sample & 7u) * 3u;
						place[0] = contribution.x;
						place[1] = contribution.y;
						place[2] = contribution.z;
					}
					else
						st.chunk_sum = st.chunk_sum + contribution;
					if (next_sample())
						RT_HIP_BECOME(lane_restart);
					else
					{
						if (!((st.sample - 1u) & 8u)) // first half: its partial sum
						{
							slot_of_chunk[0] = st.chunk_sum.x;
							slot_of_chunk[1] = st.chunk_sum.y;
							slot_of_chunk[2] = st.chunk_sum.z;
						}
						RT_HIP_BECOME(lane_free);
					}
					return;
				}
				st.chunk_sum = st.chunk_sum + contribution;
				if (next_sample())
					RT_HIP_BECOME(lane_restart);
				else
				{
					if (ROLLING)
						complete_item();
					else
					{
						slots[slot * 3u + 0u] = st.chunk_sum.x;
						slots[slot * 3u + 1u] = st.chunk_sum.y;
						slots[slot * 3u + 2u] = st.chunk_sum.z;
					}
					RT_HIP_BECOME(lane_free);
				}
			};

			while (true)
			{
				// ---- closest-hit query for every lane that holds a ray (trace(), :160-162) -----------------------------------
				RT_HIP_REGION(0); // a trip
				const bool tracing = RT_HIP_IS(lane_trace);
				if (SCALAR_SEGMENTS)
					wave_segments += static_cast<unsigned>(__builtin_popcountll(__builtin_amdgcn_ballot_w64(tracing)));
				candidate tiled_planes = { 0.0f, 0u, false };
				candidate tiled_spheres = { 0.0f, 0u, false };
				if (NS == scan_tiled && __syncthreads_or(tracing)) // nothing to stream on the very first trip: no lane holds a ray yet
				{
					// all 256 threads stage, lanes without a ray just do not scan
					for (uint32_t first = 0; first < s.n_planes; first += tile_primitives)
					{
						const uint32_t count = min(tile_primitives, s.n_planes - first);
						__syncthreads(); // previous tile fully consumed
						stage_planes(lds, s, first, count);
						__syncthreads();
						if (tracing)
							scan_lds<false>(tiled_planes, st.origin, st.dir, lds, count, first);
					}
					for (uint32_t first = 0; first < s.n_spheres; first += tile_primitives)
					{
						const uint32_t count = min(tile_primitives, s.n_spheres - first);
						__syncthreads();
						stage_spheres(lds, s, first, count);
						__syncthreads();
						if (tracing)
							scan_lds<true>(tiled_spheres, st.origin, st.dir, lds, count, first);
					}
				}

				// After the query a lane either SHADES a hit (scatter: three draws, a new direction) or, having missed,
				// RESTARTS with the next sample's primary ray (two draws, a new direction).  Both end in the same
				// operations — random draws and the normalisation of a direction — which are therefore issued once for
				// the whole wave; only the pieces that really differ run under their own lane masks.
				// streamed kernel, a wave with a handful of rays: one cooperative scan per ray (see scan_spheres_together)
				candidate together = { 0.0f, 0u, false };
				bool scanned_together = false;
#ifdef RT_HIP_NO_SPARSE_WAVES // (experiment builds: the kernel without the cooperative scan)
				constexpr bool sparse_waves = false;
#else
				constexpr bool sparse_waves = true;
#endif
				if (sparse_waves && NS == scan_streamed && s.n_spheres >= sparse_min_spheres)
				{
					unsigned long long holders = __builtin_amdgcn_ballot_w64(tracing);
					if (holders != 0 && static_cast<uint32_t>(__builtin_popcountll(holders)) <= q.sparse_rays)
					{
						while (holders != 0) // (wave-uniform)
						{
							const int src = __builtin_ctzll(holders);
							holders &= holders - 1u;
							const vec3 o = { __int_as_float(__builtin_amdgcn_readlane(__float_as_int(st.origin.x), src)), __int_as_float(__builtin_amdgcn_readlane(__float_as_int(st.origin.y), src)),
											 __int_as_float(__builtin_amdgcn_readlane(__float_as_int(st.origin.z), src)) };
							const vec3 d = { __int_as_float(__builtin_amdgcn_readlane(__float_as_int(st.dir.x), src)), __int_as_float(__builtin_amdgcn_readlane(__float_as_int(st.dir.y), src)),
											 __int_as_float(__builtin_amdgcn_readlane(__float_as_int(st.dir.z), src)) };
							candidate found;
							const bool clean = scan_spheres_together(found, o, d, geometry, s.n_spheres, lane);
							if (clean && lane == static_cast<uint32_t>(src))
							{
								together = found;
								scanned_together = true;
							}
						}
					}
				}

				bool shade = false;
				[[maybe_unused]] bool from_shadow = false; // [DIRECT] the lane shades behind its shadow query: it has aimed already
				vec3 normal; // meaningful only where `shade` holds: deliberately not initialised
				float4 shading;
				uint32_t scatter_kind = scatter_lambert;
				if (tracing)
				{
					RT_HIP_REGION(1); // query: probes
					if (!SCALAR_SEGMENTS)
						lane_segments++;
					uint32_t kind;
					float distance;
					uint32_t small_index = 0;
					[[maybe_unused]] uint32_t direct_index = 0; // [DIRECT] the accepted hit's index among its kind
					if (NS == scan_tiled)
					{
						uint32_t index;
						kind = select_hit(tiled_spheres, tiled_planes, distance, index);
						fetch_hit<SM>(s, st.origin, st.dir, kind, distance, index, normal, shading, scatter_kind);
					}
					else if (NS > 0)
					{
						// The discriminants of a GROUP of spheres first (independent straight-line code with scalar operands), one
						// branch for "no lane can hit any of them", then their square-root halves in index order.  Up to four spheres
						// are one group.  From five spheres on they go in groups of three: every discriminant of a group is three live
						// vector registers until its square-root half has run, and seven or eight at once put the kernel over its
						// budget (72 at 7 waves per SIMD) — round 4 lived with 12-16 bytes of scratch there; in round 5 the same source
						// took 84-124 bytes with the contract-v4 tail, and dielectric.toml went from 2.7 to 9.4 ms
						// (profiles/r05/codegen_ab.txt; tools/kernel_registers.py lists every build's registers and scratch).
						candidate best = { 0.0f, 0u, false };
						constexpr int spheres_ns = NS > 0 ? NS : 1; // (this branch is compiled, though never taken, for NS <= 0)
#ifdef RT_HIP_PROBE_GROUP
						constexpr int group = RT_HIP_PROBE_GROUP; // (A/B builds)
#else
						constexpr int group = spheres_ns <= 4 ? spheres_ns : 3;
#endif
#pragma unroll
						for (int first = 0; first < NS; first += group)
						{
							sphere_probe probes[group];
							unsigned long long lanes[group];
							unsigned long long any_lane = 0;
#pragma unroll
							for (int i = 0; i < group; i++)
								if (first + i < NS)
								{
									probes[i] = probe_sphere(st.origin, st.dir, small.geometry[first + i]); // SGPR operands
									lanes[i] = __builtin_amdgcn_ballot_w64(probes[i].pos);
									any_lane |= lanes[i];
								}
							if (any_lane != 0)
							{
#pragma unroll
								for (int i = 0; i < group; i++)
									if (first + i < NS)
									{
										if (lanes[i] != 0)
											RT_HIP_REGION(2); // square-root half of one sphere
										finish_sphere(best, probes[i], small.geometry[first + i].w, static_cast<uint32_t>(first + i), lanes[i]);
									}
							}
						}
						if (NP > 0)
						{
							// test_planes (:36-60) over the plane slots, with its own best candidate; then select(spheres, planes) (:96-102,160) —
							// select_hit() (scan.hpp) on the comparisons' masks: written over sentinel distances it costs three selects and a
							// divergent block more per query.  `>= 0` is hit_result's `operator bool` (:29-32; false for a NaN distance).
							float plane_distance;
							uint32_t plane_slot = static_cast<uint32_t>(NS);
							bool plane;
							if (NP == 1)
								plane = test_one_plane(st.origin, st.dir, small.geometry[NS > 0 ? NS : 0], plane_distance);
							else
							{
								candidate best_plane = { 0.0f, 0u, false };
#pragma unroll
								for (int j = 0; j < NP; j++)
									test_plane(best_plane, st.origin, st.dir, small.geometry[(NS > 0 ? NS : 0) + j], static_cast<uint32_t>(j));
								plane = best_plane.have && best_plane.t >= 0.0f;
								plane_distance = best_plane.t;
								plane_slot += best_plane.index;
							}
							const bool nearer = best.t <= plane_distance;
							const bool sphere = best.have && best.t >= 0.0f;
							const bool use_sphere = sphere && (!plane || nearer);
							const bool use_plane = plane && !use_sphere;
							distance = use_sphere ? best.t : plane_distance; // (a miss never reads it)
							kind = use_sphere ? 1u : (use_plane ? 2u : 0u);
							small_index = use_sphere ? best.index : plane_slot; // the winner's slot (one select; with one plane its index is a constant)
						}
						else
						{
							const bool hit = best.have && best.t >= 0.0f;
							kind = hit ? 1u : 0u;
							distance = best.t;
							small_index = best.index; // the lookups of the winning sphere follow below, in the one `hit` region
						}
					}
					else
					{
						candidate planes = { 0.0f, 0u, false };
						candidate spheres = { 0.0f, 0u, false };
						// resident: the LDS copy; streamed: the table in HBM/L2 itself, read with wave-uniform (scalar) loads
						const float4* const primitives = RESIDENT ? lds : geometry;
						scan_lds<false>(planes, st.origin, st.dir, RESIDENT ? lds + lds_spheres : geometry + s.n_spheres, s.n_planes, 0);
						if (BVH)
						{
							// the lane's traversal stack: word k at lds[k * block_threads + threadIdx.x] (consecutive lanes, consecutive banks)
							if (!bvh_spheres(spheres, st.origin, st.dir, bvh, geometry, reinterpret_cast<uint32_t*>(lds) + threadIdx.x))
							{
								spheres = { 0.0f, 0u, false }; // a degenerate ray or a non-finite distance: the sequential rule decides
								scan_streamed_spheres(spheres, st.origin, st.dir, geometry, s.n_spheres);
							}
#ifdef RT_HIP_BVH_CHECK
							candidate linear = { 0.0f, 0u, false };
							scan_streamed_spheres(linear, st.origin, st.dir, geometry, s.n_spheres);
							const bool same = linear.have == spheres.have && (!linear.have || (__float_as_uint(linear.t) == __float_as_uint(spheres.t) && linear.index == spheres.index));
							atomicAdd(&counters->bvh_checked, 1ull);
							if (!same)
								atomicAdd(&counters->bvh_disagreements, 1ull);
#endif
						}
						else if (NS == scan_streamed || NS == scan_streamed_dense)
						{
							if (scanned_together)
								spheres = together;
							else
								scan_streamed_spheres(spheres, st.origin, st.dir, geometry, s.n_spheres);
						}
						// From a few dozen spheres on the resident kernel reads the sphere table as the streamed kernel does — wave-uniform
						// scalar loads of (c, r^2) groups from the table in memory, the next group's load issued before this group's
						// probes — instead of broadcast reads from its LDS copy: a table of this size sits in the scalar cache, the probes
						// take their operands from scalar registers, and neither the LDS pipe nor four vector registers per sphere in
						// flight are spent on it (64 spheres x 256 spp 12.9 -> 12.5 ms, 200 spheres 9.6 -> 8.7, 700 33.3 -> 29.9; below
						// about 40 the LDS copy is ahead: 12 spheres 1.17 against 1.24 ms; profiles/r05/resident_scalar_ab.txt)
						else if (RESIDENT_SCALAR_SCAN)
							scan_streamed_spheres(spheres, st.origin, st.dir, geometry, s.n_spheres);
						else
							scan_lds<true>(spheres, st.origin, st.dir, primitives, s.n_spheres, 0);
						uint32_t index;
						if constexpr (BOXTREE)
						{
							candidate boxes = { 0.0f, 0u, false };
							const vec3 inv = box_reciprocals(st.dir);
							// (the lane's stack again: the sphere traversal above has returned)
							if (!bvh_boxes(boxes, st.origin, inv, box_tree, s.box_bounds, reinterpret_cast<uint32_t*>(lds) + threadIdx.x))
							{
								boxes = { 0.0f, 0u, false }; // a zero, subnormal or non-finite component: the linear scan decides
								scan_boxes(boxes, st.origin, inv, s.box_bounds, s.n_boxes);
							}
							kind = select_hit(spheres, planes, boxes, distance, index);
							fetch_hit<SM>(s, s.box_bounds, st.origin, st.dir, inv, kind, distance, index, normal, shading, scatter_kind);
						}
						else if constexpr (BOXES)
						{
							candidate boxes = { 0.0f, 0u, false };
							const vec3 inv = box_reciprocals(st.dir);
							scan_boxes(boxes, st.origin, inv, lds_boxes, s.n_boxes);
							kind = select_hit(spheres, planes, boxes, distance, index);
							fetch_hit<SM>(s, lds_boxes, st.origin, st.dir, inv, kind, distance, index, normal, shading, scatter_kind);
						}
						else
						{
							kind = select_hit(spheres, planes, distance, index);
							fetch_hit<SM>(s, st.origin, st.dir, kind, distance, index, normal, shading, scatter_kind);
							if constexpr (DIRECT)
								direct_index = index;
						}
					}
					if (DIRECT && shadow)
					{
						// the answer of a shadow query: the light is visible iff the accepted hit is the aimed sphere (no distance is compared).  The
						// lane then scatters as the lambert vertex it is, from the unchanged origin; its throughput holds the attenuation already.
						if (kind == 1u && direct_index == pending_sphere)
							direct_sum = direct_sum + pending;
						shadow = false;
						from_shadow = true;
						sampled_before = true;
						shade = true;
						normal = kept_normal;
						shading = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
						scatter_kind = scatter_lambert;
					}
					else if (!kind)
					{
						RT_HIP_REGION(4); // miss: sky, end of sample
						end_sample(st.throughput * sky(st.dir.y)); // miss (:163-164)
					}
					else if (DIRECT && scatter_kind == scatter_emit_sampled && sampled_before)
					{
						// a sampled light behind a vertex that has sampled the lights itself: worth 0 (§3.13)
						end_sample({ 0.0f, 0.0f, 0.0f });
					}
					else if (LIGHTS && (scatter_kind == scatter_emit || (DIRECT && scatter_kind == scatter_emit_sampled)))
					{
						// the accepted hit's material is a light: the sample is throughput * emission and the path ends — no draw, no scatter (§3.12)
						end_sample(st.throughput * vec3{ shading.x, shading.y, shading.z });
					}
					else
					{
						shade = true;
						// r.at(t): where the scattered ray starts (:122,139).  The lane is done with the old origin — it goes straight
						// into the ray's registers (as a value of its own it was copied there, three moves per scatter, after the hand-out).
						st.origin = ray_at(st.origin, st.dir, distance);
						if (NS > 0)
						{
							RT_HIP_REGION(3); // hit: lookups + normal
							const float4 g = lds_geometry[small_index];
							shading = lds_shading[small_index];
							scatter_kind = __float_as_uint(g.w);
							if (NP > 0 && kind == 2u)
								normal = { g.x, g.y, g.z }; // the plane's normal as it is, not flipped toward the ray (:58)
							else
							{
								// (a branch, not a select: a wave whose hits are all on the ground plane — most of a frame's — skips the
								// normalisation altogether)
								if (NP > 0)
									asm volatile("; hit: some lane hit a sphere" ::: "memory");
								normal = normalize(st.origin - vec3{ g.x, g.y, g.z }); // direction(center, r.at(t)) (:85)
							}
						}
					}
				}


				// ---- hand out items to free lanes (converged): a lane whose chunk just ended with a miss restarts right below ----
				const unsigned long long asking = __builtin_amdgcn_ballot_w64(RT_HIP_IS(lane_free));
				// a free lane becomes the owner of item `item` of the tile at (x0, y0)
				// a free lane starts on chunk `chunk` of the pixel at (lx, ly) of this rank's rows
				// (HALF: `chunk` counts half-chunks of 8 samples; one that lies wholly behind the last sample is empty)
				const auto start_item = [&](uint32_t lx, uint32_t ly, uint32_t chunk)
				{
					const uint32_t item_samples = (HALF && ROLLING) ? q.item_samples : (HALF ? sample_chunk / 2u : sample_chunk);
					if (HALF && !ROLLING && chunk * item_samples >= p.samples_per_pixel)
						return; // (the lane stays free and asks again)
					const uint32_t gy = global_row(ly, p);
					st.chunk_sum = { 0.0f, 0.0f, 0.0f };
					camera_base<build>(st, p, static_cast<float>(lx), static_cast<float>(gy));
					st.keys.function_key = pixel_function_key(p.frame_key_a, gy * p.width + lx); // image_view::position_of, image.hpp:155-159
					st.keys.stride = pixel_stride(p.frame_key_b, st.keys.function_key);
					const uint32_t first = (PASS ? first_chunk + chunk : chunk) * item_samples, end = min(first + item_samples, p.samples_per_pixel);
					st.sample = first;
					st.sample_end = end;
					st.window = sample_counter(st.keys.stride, first);
					st.window_end = sample_counter(st.keys.stride, end);
					RT_HIP_BECOME(lane_restart);
				};
				// a free lane becomes the owner of item `item` of the tile at (x0, y0)
				const auto take_item = [&](uint32_t item, uint32_t x0, uint32_t y0)
				{
					const uint32_t pixel = item & ((1u << q.pixels_log2) - 1u); // chunk-major item order
					const uint32_t chunk = item >> q.pixels_log2;
					const uint32_t lx = x0 + (pixel & (tile_w - 1u));
					const uint32_t ly = y0 + (pixel >> q.tile_w_log2);
					if constexpr (ADAPT)
					{
						if (lx < p.width && ly < p.local_rows && !((tile_stopped >> pixel) & 1ull))
							start_item(lx, ly, chunk);
						// else: outside the frame, or a stopped pixel — the item is empty, ask again next trip
					}
					else if (lx < p.width && ly < p.local_rows)
						start_item(lx, ly, chunk);
					// else: a pixel outside the frame — the item is empty, ask again next trip
				};
				if (!ROLLING && asking != 0)
				{
					RT_HIP_REGION(6); // hand-out
					const uint32_t rank = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(asking >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(asking), 0u));
					if (RT_HIP_IS(lane_free))
					{
						slot = next_item + rank;
						if (slot >= items)
							RT_HIP_BECOME(lane_retired);
						else
						{
							RT_HIP_REGION(7); // a lane takes an item: pixel coordinates, stream keys
							take_item(slot, tile_x0, tile_y0);
						}
					}
					next_item += static_cast<uint32_t>(__builtin_popcountll(asking));
				}
				if (ROLLING && asking != 0)
				{
					const uint32_t rank = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(asking >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(asking), 0u));
					uint32_t want = static_cast<uint32_t>(__builtin_popcountll(asking));
					if (q.lane_cap < 64u) // (wave-uniform) a sparse launch: this wave holds at most lane_cap rays, see choose_queue
					{
						const uint32_t holding = static_cast<uint32_t>(__builtin_popcountll(__builtin_amdgcn_ballot_w64(RT_HIP_IS(lane_trace) || RT_HIP_IS(lane_restart))));
						want = min(want, q.lane_cap > holding ? q.lane_cap - holding : 0u);
					}
					uint32_t served = 0; // asking lanes given an item so far, in rank order
					while (served < want)
					{
						if (block_next == block_end) // this wave's block is used up: on to the one drawn ahead
						{
							if (dry)
								break;
							if (prefetched >= total_items)
							{
								dry = true;
#ifdef RT_HIP_WAVE_CLOCKS
								clock_dry = wall_clock64();
#endif
								break;
							}
							block_next = prefetched;
							block_end = min(prefetched + prefetched_count, total_items);
							prefetched_count = q.block_items;
							prefetched = fetch_items(counters, prefetched_count);
						}
						const uint32_t take = static_cast<uint32_t>(min(static_cast<unsigned long long>(want - served), block_end - block_next)); // >= 1
						if (RT_HIP_IS(lane_free) && rank - served < take) // served <= rank < served + take
						{
							// item -> (pixel in hand-out order, chunk): pixel-major, so that a pixel's chunks are started together
							const unsigned long long item = block_next + (rank - served);
							uint32_t pixel, chunk;
							if ((total_items >> 32) == 0) // (wave-uniform)
							{
								pixel = static_cast<uint32_t>(item) / items_per_pixel;
								chunk = static_cast<uint32_t>(item) - pixel * items_per_pixel;
							}
							else
							{
								pixel = static_cast<uint32_t>(item / items_per_pixel);
								chunk = static_cast<uint32_t>(item - static_cast<unsigned long long>(pixel) * items_per_pixel);
							}
							const uint32_t row = pixel / p.width; // bottom row first
							slot = pixel;
							start_item(pixel - row * p.width, p.local_rows - 1u - row, chunk);
						}
						served += take;
						block_next += take;
					}
					if (dry && RT_HIP_IS(lane_free))
						RT_HIP_BECOME(lane_retired);
				}
				const bool queue_empty = __builtin_amdgcn_ballot_w64(!RT_HIP_IS(lane_retired)) == 0;
				if (NS == scan_tiled)
				{
					if (__syncthreads_and(queue_empty)) // the four waves leave together
						break;
				}
				else if (queue_empty)
					break;

				const bool restart = RT_HIP_IS(lane_restart);
				// (Every trip of a live wave has lanes here: no vote in front of the tail.  A restarting lane's stream already
				// stands at its sample's window — next_sample / start_item put it there — so both kinds of lane draw from
				// st.counter and nothing is selected or multiplied per trip.)
				{
					RT_HIP_REGION(8); // the fused tail: one generator step
					// ONE generator step for every lane (contract v4): a scattering lane's random<vec3>() (random_unit_vector,
					// random.hpp:57-66: the third word follows below) or random<float>(), a restarting lane's random<vec2>() (the
					// pixel jitter, :189).  As numerators k of u = k * 2^-24: the scaling is folded into the jitter's constants and
					// cancels in the unit vector.
					// (The step advances EVERY lane's counter in place — a free or retired lane's too, whose counter nobody reads before
					// start_item sets it.  Nothing below needs the value it had: "the stream stood at 0" reads "it now stands at one
					// stride".  Advanced in a copy and written back by the lanes that shade or restart, it cost a register move per trip.)
					// A restarting lane draws from the start of its sample's window, a scattering lane goes on where it stands: one select.
					// (Rounds 4-5 had next_sample() copy the window into the counter instead — a move per miss, and three more per trip
					// that carried the two versions of the counter through the hit / miss join.)
					st.counter = restart ? st.window : st.counter;
#ifdef RT_HIP_FAST_BUILD
					uint32_t word = next_step_word(st.counter, st.keys);
#else
					// (the addition written out with its result tied to its operand's register: hipcc otherwise adds into a second
					// register and moves the sum back at the end of the trip)
					asm("v_add_u32 %0, %0, %1" : "+v"(st.counter) : "v"(st.keys.stride));
					uint32_t word = step_word_at(st.counter, st.keys);
#endif
					uint32_t word_a = word * step_mul_a, word_b = word * step_mul_b;
					float d0 = step_numerator(word_a);
					float d1 = step_numerator(word_b);
					vec3 toward; // the vector whose direction the new ray takes (set on both paths below)
					// dot(toward, toward).  (sm's dielectric_scatter does not normalise what it returns: its lanes leave the 1 here,
					// whose reciprocal square root is 1, and x * 1 is x for every x.)
					float toward2;
					if (SM)
						toward2 = 1.0f;
					if constexpr (DIRECT)
					{
						if (shade && !from_shadow && scatter_kind == scatter_lambert)
						{
							// the VERTEX RULE (§3.13; direct_light_rules.hpp) with the step just drawn: the light from its third numerator, the point on
							// it from the first two.  Gather loads: every lane reads the light it chose.
							const uint32_t chosen = direct_light::choose_light((word * step_mul_c) >> 8, direct_n);
							const float4 ball = direct_list[2u * chosen], glow = direct_list[2u * chosen + 1u];
							const direct_light::aim<vec3> a =
								direct_light::aim_at(word_a >> 8, word_b >> 8, st.origin, normal, vec3{ ball.x, ball.y, ball.z }, ball.w, direct_n, contract_inv_sqrt{});
							sampled_before = true;
							if (a.aimed)
							{
								// an aiming lane: the shadow query is its next, from the unchanged origin; it consumes no bounce
								st.throughput = st.throughput * vec3{ shading.x, shading.y, shading.z };
								pending = (st.throughput * vec3{ glow.x, glow.y, glow.z }) * a.weight;
								pending_sphere = __float_as_uint(glow.w);
								kept_normal = normal;
								st.dir = a.w;
								shadow = true;
								shade = false;
							}
							else
							{
								// aims at nothing: the lane scatters in this trip, with a step of its own
								word = next_step_word(st.counter, st.keys);
								word_a = word * step_mul_a, word_b = word * step_mul_b;
								d0 = step_numerator(word_a);
								d1 = step_numerator(word_b);
							}
						}
						else if (shade && !from_shadow)
							sampled_before = false; // a metal or dielectric vertex samples nothing
					}
					if (shade && SM && scatter_kind == scatter_dielectric)
					{
						// dielectric_scatter, sm_ray_tracer.cpp:181-219 (refract :161-172, schlick :174-179); shading.w = the
						// material's reflectivity, which the reference uses as the index of refraction.  ONE draw.
						const float refl = shading.w;
						const vec3 d = st.dir;
						const float dn = dot(d, normal);
						const float k = 2.0f * dn;
						const vec3 reflected = { fma(-k, normal.x, d.x), fma(-k, normal.y, d.y), fma(-k, normal.z, d.z) };
						const float len = sqrt_rn(dot(d, d)); // (== __builtin_sqrtf, bit for bit: contract.hpp)
						const bool inside = dn > 0.0f;
						const vec3 outward = inside ? vec3{ -normal.x, -normal.y, -normal.z } : normal;
						const float eta = inside ? refl : rcp_rn(refl);
						const float cosine = inside ? (refl * dn) / len : (-dn) / len;
						float reflect_prob = 1.0f;
						vec3 refracted = { 0.0f, 0.0f, 0.0f };
						const float cos_i = -dot(d, outward);
						const float sin2_t = (eta * eta) * fma(-cos_i, cos_i, 1.0f);
						if (!(sin2_t > 1.0f)) // refract() returned true
						{
							const float cos_t = sqrt_rn(1.0f - sin2_t);
							const float kk = fma(eta, cos_i, -cos_t);
							refracted = { fma(kk, outward.x, eta * d.x), fma(kk, outward.y, eta * d.y), fma(kk, outward.z, eta * d.z) };
							float r0 = (1.0f - refl) / (1.0f + refl);
							r0 = r0 * r0;
							const double x = static_cast<double>(1.0f - cosine); // pow(1 - cosine, 5) in double, by multiplication
							const double x2 = x * x;
							const double x5 = (x2 * x2) * x;
							reflect_prob = static_cast<float>(static_cast<double>(r0) + static_cast<double>(1.0f - r0) * x5);
						}
						toward = (d0 * random_scale < reflect_prob) ? reflected : refracted;
						st.throughput = st.throughput * vec3{ shading.x, shading.y, shading.z };
						const bool dead = mode == lane_trace; // no bounce left: the next trace() call would return {} at :157-158
						mode--;
						if (dead)
							end_sample({ 0.0f, 0.0f, 0.0f });
					}
					else if (shade)
					{
						RT_HIP_REGION(9); // scatter: third draw, unit vector, new direction
						uint32_t word_c = word * step_mul_c;
						while (((word_a | word_b | word_c) >> 8) == 0u) // `if (p == zero) continue` (random.hpp:61-62): the next step
						{
							word = next_step_word(st.counter, st.keys);
							word_a = word * step_mul_a, word_b = word * step_mul_b, word_c = word * step_mul_c;
							d0 = step_numerator(word_a);
							d1 = step_numerator(word_b);
						}
						const vec3 u = normalize_unit_cube_numerators({ d0, d1, step_numerator(word_c) });
						vec3 scatter = normal + u; // lambert (:117)
						bool absorbed = false;
						if (scatter_kind == scatter_metal)
						{
							RT_HIP_REGION(5); // metal: normalise the incoming direction, reflect, spread by the roughness
							// reflect(normalize(r.direction), n) + roughness * random_unit_vector() (:133-134, common.hpp:100-103)
							const vec3 v = normalize(st.dir);
							const float k = 2.0f * dot(v, normal);
							const vec3 reflected = { fma(-k, normal.x, v.x), fma(-k, normal.y, v.y), fma(-k, normal.z, v.z) };
							scatter = { fma(shading.w, u.x, reflected.x), fma(shading.w, u.y, reflected.y), fma(shading.w, u.z, reflected.z) };
							absorbed = dot(scatter, normal) <= 0.0f; // (:135-136)
							toward2 = dot(scatter, scatter);
						}
						else
						{
							toward2 = dot(scatter, scatter);
							// `if (scatter.approx_zero()) scatter = normal` (:118-119): all three components within 1e-6 of zero.  Then the
							// sum of their squares is at most 3e-12 (and a hair: three roundings) — a single comparison every lane can
							// afford; the three of the rule itself run behind a vote that practically never fires.
							if (__builtin_amdgcn_ballot_w64(toward2 <= 3.0001e-12f) != 0)
							{
								asm volatile("; lambert: some lane's scatter vector is next to zero" ::: "memory");
								if (__builtin_fabsf(scatter.x) <= approx_zero_epsilon && __builtin_fabsf(scatter.y) <= approx_zero_epsilon && __builtin_fabsf(scatter.z) <= approx_zero_epsilon)
								{
									scatter = normal;
									toward2 = dot(scatter, scatter);
								}
							}
						}
						st.throughput = st.throughput * vec3{ shading.x, shading.y, shading.z }; // attenuation * trace(...) (:171)
						toward = scatter;
						// absorbed, or the next trace() call would return {} at :157-158 (`if (!(max_bounces--))`: the count is kept
						// as the bounces still allowed after the segment in flight, and only a bounce touches it)
						const bool dead = absorbed || mode == lane_trace;
						mode--; // (a dead lane's mode is set by end_sample right below)
						if (dead)
						{
							RT_HIP_REGION(12); // absorbed or out of bounces: the sample is worth nothing
							end_sample({ 0.0f, 0.0f, 0.0f });
						}
					}
					else if (restart)
					{
						RT_HIP_REGION(10); // restart: primary ray
						// worker lambda :189-193 — jittered position, un-project to near and far, build the primary ray
						float jx = d0, jy = d1;
						// sample 0 goes through the pixel centre (0.5 = 2^23 * 2^-24) and draws nothing (:189).  Its window is the one
						// that starts at stream position 0.  One restart in spp is such a sample, and a wave meets them all in its first
						// trips: a vote keeps the two selects and the rewind out of every other trip.
						const bool at_sample_0 = st.window == 0u;
						if (__builtin_amdgcn_ballot_w64(at_sample_0) != 0)
						{
							asm volatile("; restart: some lane is at its pixel's sample 0" ::: "memory");
							if (at_sample_0)
							{
								jx = jy = 0x1.0p23f;
								st.counter = 0u; // (the sample draws nothing: back to the window's start)
							}
						}
						if (PINHOLE_ONLY || (!EYE_ONLY && !NEVER_PINHOLE && p.pinhole)) // (wave-uniform: a kernel argument)
						{
							// rt's camera: the near-to-far vector from the pixel's base and the jitter, the near point from it (contract
							// v4; constants from the host).  The LDS / big-scene kernels carry both forms; a scalar-register kernel is
							// built for ONE of them (GC): as kernel arguments the two sets of scalars together would cost its loop, which
							// lives on its scalar registers, a spill per lane mask.
							toward = { fma(p.ray_j1[0], jx, fma(p.ray_j2[0], jy, st.base_x)), fma(p.ray_j1[1], jx, fma(p.ray_j2[1], jy, st.base_y)),
									   fma(p.ray_j1[2], jx, fma(p.ray_j2[2], jy, st.base_z)) };
							st.origin = { p.ray_eye[0] + toward.x, p.ray_eye[1] + toward.y, p.ray_eye[2] + toward.z }; // (toward = near - eye)
						}
						else if (EYE_ONLY || LENS || p.eye_form) // (wave-uniform; a lens frame always has an eye: lens.hpp, check_lens_frame)
						{
							// a perspective matrix that is no pinhole's in binary32 — a camera that is not axis-aligned: rounding noise in
							// its w row.  Every near-to-far line passes through the eye E; the near point relative to it (times N.w) and
							// N.w itself move with the jitter like the pinhole's vector does: ONE reciprocal per sample, no far point
							// (round 4: two reciprocals and sixteen multiply-adds for the two points).
							toward = { fma(p.eye_jq1[0], jx, fma(p.eye_jq2[0], jy, st.base_x)), fma(p.eye_jq1[1], jx, fma(p.eye_jq2[1], jy, st.base_y)),
									   fma(p.eye_jq1[2], jx, fma(p.eye_jq2[2], jy, st.base_z)) };
							const float ws = fma(p.eye_jw1, jx, fma(p.eye_jw2, jy, st.base_w));
							// (wave-uniform) the host has shown ws in the band and N.w F.w > 0 for the whole frame — every frame of a camera
							// that looks at its scene; the scalar-register kernels are built for such frames only (choose_kernel), anything
							// else — near and far points on different sides of w = 0, a w at the band's ends — goes through the resident kernel
							const bool plain = EYE_ONLY || p.eye_form == 2u;
							float inv;
							if (plain)
								inv = rcp_in_band(ws);
							else
							{
								asm volatile("; restart: the guarded reciprocal" ::: "memory");
								inv = rcp_rn(ws);
							}
							st.origin = { fma(toward.x, inv, p.eye_e[0]), fma(toward.y, inv, p.eye_e[1]), fma(toward.z, inv, p.eye_e[2]) };
							// far - near = s N' |Z.w| / (N.w F.w): s N' unless the near and far points lie on different sides of w = 0
							if (!plain && __builtin_amdgcn_ballot_w64(ws * (ws + p.eye_zws) < 0.0f) != 0)
							{
								asm volatile("; restart: some lane's near and far points straddle w = 0" ::: "memory");
								if (ws * (ws + p.eye_zws) < 0.0f)
									toward = { -toward.x, -toward.y, -toward.z };
							}
						}
						else
						{
							// no finite eye (an orthographic frustum): un-project to depth 0 and depth 1 (camera.hpp:42-48) in homogeneous form, N and F.  The
							// near point needs its division; the direction does not — far / F.w - near / N.w is F N.w - N F.w over
							// N.w F.w, and normalize() removes a positive factor: one reciprocal per sample (round 4: two).
							const float px = fma(jx, random_scale, st.base_x); // == x + jx * 2^-24: the product is exact
							const float py = fma(jy, random_scale, st.base_y);
							const float ndc_x = fma(px, p.sx, -1.0f);
							const float ndc_y = fma(py, p.neg_sy, 1.0f);
							float N[4], F[4];
#pragma unroll
							for (int r = 0; r < 4; r++)
							{
								N[r] = fma(p.mx[r], ndc_x, fma(p.my[r], ndc_y, p.k_near[r]));
								F[r] = fma(p.mx[r], ndc_x, fma(p.my[r], ndc_y, p.k_far[r]));
							}
							const float inv_wn = rcp_rn(N[3]);
							st.origin = { N[0] * inv_wn, N[1] * inv_wn, N[2] * inv_wn };
							toward = { fma(F[0], N[3], -(N[0] * F[3])), fma(F[1], N[3], -(N[1] * F[3])), fma(F[2], N[3], -(N[2] * F[3])) };
							if (N[3] * F[3] < 0.0f)
								toward = { -toward.x, -toward.y, -toward.z };
						}
						if constexpr (LENS)
						{
							// the LENS STEP (§3.17; lens_rules.hpp): one more step of the sample's own stream under the restarting lanes' mask, directly
							// behind the jitter step — sample 0, which has rewound to its window's start, draws it from there — then the primary ray
							// just made, normalised as the tail below would have, is bent through the step's point of the lens.  The ten lens words
							// lie in the words of p that only the homogeneous form reads (lens.hpp, put_lens_words); a lane whose ray does not meet
							// the focus plane in front of the lens keeps the pinhole's ray, by select.
							const uint32_t lens_word = next_step_word(st.counter, st.keys);
							const lens::disk_point on_disk = lens::disk((lens_word * step_mul_a) >> 8, (lens_word * step_mul_b) >> 8);
							const vec3 d = toward * inv_sqrt_rn(dot(toward, toward));
							const bool through_pinhole = PINHOLE_ONLY || (!NEVER_PINHOLE && p.pinhole);
							const vec3 eye = { through_pinhole ? p.ray_eye[0] : p.eye_e[0], through_pinhole ? p.ray_eye[1] : p.eye_e[1], through_pinhole ? p.ray_eye[2] : p.eye_e[2] };
							const lens::words<vec3> lens_words = { { p.mx[0], p.mx[1], p.mx[2] }, { p.my[0], p.my[1], p.my[2] }, { p.k_near[0], p.k_near[1], p.k_near[2] }, p.mx[3] };
							const lens::bent_ray<vec3> bent = lens::bend(d, eye, lens_words, on_disk);
							st.origin = { bent.bent ? bent.origin.x : st.origin.x, bent.bent ? bent.origin.y : st.origin.y, bent.bent ? bent.origin.z : st.origin.z };
							toward = { bent.bent ? bent.toward.x : toward.x, bent.bent ? bent.toward.y : toward.y, bent.bent ? bent.toward.z : toward.z };
						}
						toward2 = dot(toward, toward);
						st.throughput = { 1.0f, 1.0f, 1.0f };
						mode = lane_trace + (p.max_bounces - 1u); // tracing, max_bounces - 1 bounces to go after the primary segment
					}
					if (shade || restart)
					{
						RT_HIP_REGION(11); // normalise the new direction: toward * inv_sqrt(dot(toward, toward))
						const float inv = inv_sqrt_rn(toward2);
						st.dir = toward * inv;
					}
				}
			}

			// ---- one tile per wave: fold and write its pixels now (rolling tiles were folded as their last item came in) ----
			if (!ROLLING)
			{
				// the slots are private to the wave: no workgroup barrier (the other three waves may still be tracing, and
				// a wave that has written its pixels should free its slot), only ordering against this wave's own writes
				__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
				fold_tile(slots, tile_x0, tile_y0);
			}
			if (!SCALAR_SEGMENTS)
			{
				wave_segments = lane_segments;
#pragma unroll
				for (int offset = 32; offset > 0; offset >>= 1)
					wave_segments += __shfl_down(wave_segments, offset, 64);
			}
			add_segments(counters, wave_segments);
#ifdef RT_HIP_WAVE_CLOCKS
			if (ROLLING && lane == 0)
			{
				const uint32_t id = blockIdx.x * 4u + wave;
				if (id < device_counters::clocked_waves)
				{
					counters->wave_clocks[id][0] = clock_start;
					counters->wave_clocks[id][1] = clock_dry;
					counters->wave_clocks[id][2] = wall_clock64();
				}
			}
#endif
#ifdef RT_HIP_REGION_COUNTERS
			if (lane == 0)
				for (unsigned i = 0; i < device_counters::regions; i++)
				{
					atomicAdd(&counters->region_runs[i], static_cast<unsigned long long>(region_runs[i]));
					atomicAdd(&counters->region_lanes[i], static_cast<unsigned long long>(region_lanes[i]));
				}
#endif
		}

#ifndef RT_HIP_FAST_BUILD
		// ---- preview: reference src/renderers/rasterizer.cpp:24-85 ----------------------------------------------------
		// One thread per pixel, one ray through the pixel centre; every lane of a wave walks the same primitive, so the
		// reads below are wave-uniform (scalar loads through the constant cache / L2).  4 bytes written per pixel and a
		// few dozen flops per primitive: a frame of a small scene is bound by the store and the launch, nothing to tune.
		__global__ __launch_bounds__(block_threads) void preview_frame(const frame_params p,
																	   const device_scene s,
																	   uint32_t* __restrict__ out_rgba,
																	   float* __restrict__ out_rgb,
																	   device_counters* __restrict__ counters)
		{
			const uint32_t lx = blockIdx.x * 64u + (threadIdx.x & 63u);
			const uint32_t ly = blockIdx.y * (block_threads / 64u) + (threadIdx.x >> 6);
			const bool alive = lx < p.width && ly < p.local_rows;
			const uint32_t gy = global_row(alive ? ly : 0u, p);

			// :30-32 — near and far points of the pixel centre
			const float ndc_x = fma(static_cast<float>(lx) + 0.5f, p.sx, -1.0f);
			const float ndc_y = fma(static_cast<float>(gy) + 0.5f, p.neg_sy, 1.0f);
			float near_row[4], far_row[4];
#pragma unroll
			for (int r = 0; r < 4; r++)
			{
				near_row[r] = fma(p.mx[r], ndc_x, fma(p.my[r], ndc_y, p.k_near[r]));
				far_row[r] = fma(p.mx[r], ndc_x, fma(p.my[r], ndc_y, p.k_far[r]));
			}
			const float inv_wn = rcp_rn(near_row[3]), inv_wf = rcp_rn(far_row[3]);
			const vec3 near_pos = { near_row[0] * inv_wn, near_row[1] * inv_wn, near_row[2] * inv_wn };
			const vec3 far_pos = { far_row[0] * inv_wf, far_row[1] * inv_wf, far_row[2] * inv_wf };
			const vec3 delta = far_pos - near_pos;
			const vec3 dir = normalize(delta);					// vec3::direction(near, far) (:39)
			float dist = sqrt_rn(dot(delta, delta)) + 1.0f;		// max_dist + 1 (:33,35)
			bool hit = false;
			uint32_t material = 0;
			vec3 hit_pos = { 0.0f, 0.0f, 0.0f };
			vec3 normal = { 0.0f, 1.0f, 0.0f };					// vec3::constants::up (:38)

			// hit_tests (:41-61): a candidate replaces the current one only if strictly nearer; planes, boxes, spheres
			for (uint32_t i = 0; i < s.n_planes; i++)
			{
				const float4 g = s.primitive_geometry[s.n_spheres + i];
				float t;
				if (hits_plane(near_pos, dir, { g.x, g.y, g.z }, g.w, t) && t < dist)
				{
					dist = t, hit = true, material = s.plane_material[i];
					hit_pos = ray_at(near_pos, dir, t);
					normal = { g.x, g.y, g.z };
				}
			}
			for (uint32_t i = 0; i < s.n_boxes; i++)
			{
				const float4 lo = s.box_bounds[2u * i], hi = s.box_bounds[2u * i + 1u];
				float t;
				if (hits_box(near_pos, dir, { lo.x, lo.y, lo.z }, { hi.x, hi.y, hi.z }, t) && t < dist)
				{
					dist = t, hit = true, material = __float_as_uint(lo.w);
					hit_pos = ray_at(near_pos, dir, t); // the normal stays what it was: the reference sets none for a box (:56-59)
				}
			}
			for (uint32_t i = 0; i < s.n_spheres; i++)
			{
				const float4 g = s.primitive_geometry[i];
				float t;
				if (hits_sphere(near_pos, dir, { g.x, g.y, g.z }, g.w, t) && t < dist)
				{
					dist = t, hit = true, material = s.sphere_material[i];
					hit_pos = ray_at(near_pos, dir, t);
					normal = normalize(hit_pos - vec3{ g.x, g.y, g.z });
				}
			}

			vec3 colour;
			if (hit)
			{
				// min(0.25 + lambert(N, direction to the eye, albedo) * 0.75, 1) (:66-73); lambert = (L . N) * albedo (:13-20)
				const float4 albedo = s.material_albedo[material];
				const float k = dot(normalize(near_pos - hit_pos), normal);
				const vec3 v = { (k * albedo.x) * 0.75f + 0.25f, (k * albedo.y) * 0.75f + 0.25f, (k * albedo.z) * 0.75f + 0.25f };
				colour = { select_min(v.x, 1.0f), select_min(v.y, 1.0f), select_min(v.z, 1.0f) };
			}
			else
			{
				// lerp(sky_start, sky_end, y / (H - 1)) (:76-80).  Both sky colours are built from integers through
				// colour's clamping constructor (colour.hpp:72-91), which turns every non-zero byte into 1.0: the sky is
				// white, and NaN for a one-row frame (0 / 0), which packs to black.
				const float t = static_cast<float>(gy) / static_cast<float>(p.height - 1u);
				const float c = fma(1.0f - 1.0f, t, 1.0f);
				colour = { c, c, c };
			}
			if (alive)
			{
				const size_t o = static_cast<size_t>(p.frame_rows ? gy : ly) * p.width + lx;
				if (out_rgb)
				{
					out_rgb[o * 3 + 0] = colour.x;
					out_rgb[o * 3 + 1] = colour.y;
					out_rgb[o * 3 + 2] = colour.z;
				}
				out_rgba[o] = pack_rgba8888(colour);
			}
			// one closest-hit query per pixel: the count is known, so a single store stands in for the per-wave atomics of the
			// render kernels (at one ray per pixel their serialisation on one address would be most of the launch: 0.40 vs 0.02 ms)
			if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
				counters->segments[0] = static_cast<unsigned long long>(p.local_rows) * p.width;
		}

		// ---- multi-GPU assemble: rank-major compact stripes -> frame ------------------------------------------------
		// `width` counts 32-bit words per row: pixels for the RGBA8888 frame, 3 x pixels for the float mean.
		// Rows of ranks below `first_rank` are left alone (the root's own stripes, when its kernel has already stored them
		// straight into the frame).  TO_HOST: the frame is the caller's page-locked back buffer — system-scope stores, written
		// through at once, so that the words cross PCIe while the kernel runs instead of behind its end-of-kernel write-back
		// (finish_pixel has the measurement).
		template <bool TO_HOST>
		__global__ __launch_bounds__(block_threads) void assemble_stripes(uint32_t width,
																		  uint32_t height,
																		  uint32_t world,
																		  uint32_t stripe_rows,
																		  uint32_t padded_local_rows,
																		  uint32_t first_rank,
																		  const uint32_t* __restrict__ gathered,
																		  uint32_t* __restrict__ frame)
		{
			const uint32_t x = blockIdx.x * block_threads + threadIdx.x;
			if (x >= width)
				return;
			// a workgroup takes rows blockIdx.y, blockIdx.y + gridDim.y, ...: one each up to assemble_max_grid_y rows (launch_assemble)
			for (uint32_t y = blockIdx.y; y < height; y += gridDim.y)
			{
				const uint32_t stripe = y / stripe_rows;
				const uint32_t rank = stripe % world;
				if (rank < first_rank) // (block-uniform: a block lies within one row at a time)
					continue;
				const uint32_t local_row = (stripe / world) * stripe_rows + (y % stripe_rows);
				const uint32_t word = gathered[(static_cast<size_t>(rank) * padded_local_rows + local_row) * width + x];
				if (TO_HOST)
					__hip_atomic_store(&frame[static_cast<size_t>(y) * width + x], word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
				else
					frame[static_cast<size_t>(y) * width + x] = word;
			}
		}

#endif // !RT_HIP_FAST_BUILD

		// ---- the dispatch: from a plan's kernel_build to the instantiation of render_queue it names -------------------------------
		// Every instantiation has one signature, so the selection RETURNS the kernel and launch_render launches through the pointer.
		// Two things here are deliberate beyond the mapping itself.  Which build reads which aliased argument word is pack_words'
		// business, not the selection's (kernels.hpp, rolling_buffers).  And a kernel's place in the code object follows the order in which
		// this code first names the instantiations — DESIGN.md §3.12 has that place as a suspect for effects of microseconds — so the
		// order of mention below is part of what the listings check (tools/kernel_listing_diff.py compares text; the sequence of
		// .amdhsa_kernel lines is compared next to it): the table kernels are reached through as many templates as the scalar-register
		// ones, and build_of names a scan's plain builds first.
		using queue_kernel = decltype(&render_queue<1, false>);

		// the build of scan NS (NS spheres in scalar registers, or scan_*) under one scatter table: plain, sub-chunk items, or — the two
		// tile-per-wave table scans of the parity build — its box / box-tree / light / adaptive / pass build, in the plan's and the API's
		// order of precedence (boxes: whole chunks, never a pass; lights: never with boxes; adaptive implies pass)
		template <int NS, bool SM, int NP, bool GC>
		queue_kernel build_of(const kernel_build& build)
		{
			// (the scan's plain builds, named first: see above)
			[[maybe_unused]] constexpr queue_kernel plain[] = { render_queue<NS, SM, !SM>, render_queue<NS, SM, false> };
#ifndef RT_HIP_FAST_BUILD
			if constexpr (NS == scan_resident || NS == scan_bvh)
			{
				constexpr bool tree = NS == scan_bvh;
				if (build.boxes)
				{
					if constexpr (tree)
						if (build.box_tree)
							return render_queue<scan_bvh_boxtree, SM, false, NP, GC>;
					return render_queue<tree ? scan_bvh_boxes : scan_resident_boxes, SM, false, NP, GC>;
				}
				if (build.lights && !build.direct)
					return render_queue<tree ? scan_bvh_lights : scan_resident_lights, SM, false, NP, GC>;
				if (build.adaptive)
					return render_queue<tree ? scan_bvh_adapt : scan_resident_adapt, SM, false, NP, GC>;
				if (build.pass)
					return render_queue<tree ? scan_bvh_pass : scan_resident_pass, SM, false, NP, GC>;
				if (build.direct) // (RT_HIP_FLAG_DIRECT_LIGHT with a sampled light: implies lights, never a pass; named last — the order of mention is the code object's)
					return render_queue<tree ? scan_bvh_direct : scan_resident_direct, SM, false, NP, GC>;
				if (build.lens) // (RT_HIP_FLAG_THIN_LENS with an aperture: never a pass, never with boxes or lights; named after every older build)
					return render_queue<tree ? scan_bvh_lens : scan_resident_lens, SM, false, NP, GC>;
			}
#endif
			if constexpr (!SM) // (the sm table keeps whole chunks: one set of kernels fewer to build)
				if (build.sub_chunk_items)
					return render_queue<NS, SM, true, NP, GC>;
			return render_queue<NS, SM, false, NP, GC>;
		}

		template <int NS, int NP = 0, bool GC = false>
		queue_kernel table_of(const kernel_build& build)
		{
#ifndef RT_HIP_FAST_BUILD // (the API refuses RT_HIP_FLAG_FAST together with RT_HIP_FLAG_SM_MATERIALS)
			if (build.sm_table)
				return build_of<NS, true, NP, GC>(build);
#endif
			return build_of<NS, false, NP, GC>(build);
		}

		// the scalar-register builds there are: (spheres, planes) with spheres + planes <= scalar_max_spheres, planes <= scalar_max_planes
		// (choose_kernel admits no others), each for the eye form (GC) and for the pinhole
		struct small_builds
		{
			int spheres, planes;
			queue_kernel (*general_camera)(const kernel_build&);
			queue_kernel (*pinhole)(const kernel_build&);
		};
		constexpr small_builds small_kernels[] = {
			{ 1, 0, table_of<1, 0, true>, table_of<1, 0, false> },
			{ 2, 0, table_of<2, 0, true>, table_of<2, 0, false> },
			{ 3, 0, table_of<3, 0, true>, table_of<3, 0, false> },
			{ 4, 0, table_of<4, 0, true>, table_of<4, 0, false> },
			{ 5, 0, table_of<5, 0, true>, table_of<5, 0, false> },
			{ 6, 0, table_of<6, 0, true>, table_of<6, 0, false> },
			{ 7, 0, table_of<7, 0, true>, table_of<7, 0, false> },
			{ 8, 0, table_of<8, 0, true>, table_of<8, 0, false> },
			{ 1, 1, table_of<1, 1, true>, table_of<1, 1, false> },
			{ 2, 1, table_of<2, 1, true>, table_of<2, 1, false> },
			{ 3, 1, table_of<3, 1, true>, table_of<3, 1, false> },
			{ 4, 1, table_of<4, 1, true>, table_of<4, 1, false> },
			{ 5, 1, table_of<5, 1, true>, table_of<5, 1, false> },
			{ 6, 1, table_of<6, 1, true>, table_of<6, 1, false> },
			{ 7, 1, table_of<7, 1, true>, table_of<7, 1, false> },
			{ 1, 2, table_of<1, 2, true>, table_of<1, 2, false> },
			{ 2, 2, table_of<2, 2, true>, table_of<2, 2, false> },
			{ 3, 2, table_of<3, 2, true>, table_of<3, 2, false> },
			{ 4, 2, table_of<4, 2, true>, table_of<4, 2, false> },
			{ 5, 2, table_of<5, 2, true>, table_of<5, 2, false> },
			{ 6, 2, table_of<6, 2, true>, table_of<6, 2, false> },
			{ 1, 3, table_of<1, 3, true>, table_of<1, 3, false> },
			{ 2, 3, table_of<2, 3, true>, table_of<2, 3, false> },
			{ 3, 3, table_of<3, 3, true>, table_of<3, 3, false> },
			{ 4, 3, table_of<4, 3, true>, table_of<4, 3, false> },
			{ 5, 3, table_of<5, 3, true>, table_of<5, 3, false> },
		};

		// the instantiation `build` names; nullptr for a scalar-register build that does not exist (nothing is launched then)
		queue_kernel select_kernel(const kernel_build& build)
		{
			if (build.scan > 0) // the scalar-register kernels: build.scan spheres, then build.planes planes
			{
				const int spheres = std::min(build.scan, static_cast<int>(scalar_max_spheres)), planes = std::min(build.planes, static_cast<int>(scalar_max_planes));
				for (const small_builds& known : small_kernels)
					if (known.spheres == spheres && known.planes == planes)
						return build.general_camera ? known.general_camera(build) : known.pinhole(build);
				return nullptr;
			}
			switch (build.scan)
			{
#ifndef RT_HIP_FAST_BUILD // (the API refuses RT_HIP_FLAG_FAST together with RT_HIP_FLAG_BVH)
				case scan_bvh: return table_of<scan_bvh>(build);
#endif
				case scan_resident:
					if (build.planes) // (the scalar-load scan: one build for every camera form)
						return table_of<scan_resident, 1, false>(build);
					return build.general_camera ? table_of<scan_resident, 0, true>(build) : table_of<scan_resident, 0, false>(build);
				case scan_streamed_dense: return table_of<scan_streamed_dense>(build);
				case scan_streamed: return table_of<scan_streamed>(build);
				default: return table_of<scan_tiled>(build);
			}
		}

		// the aliased argument words of a launch, packed as the builds read them (the contract: kernels.hpp, rolling_buffers; the device's
		// side: queue_build.hpp, unpack_words)
		struct kernel_words
		{
			queue_params queue;			   // block_items: [pass builds] the pass's first chunk; [other tile-per-wave builds] the launch's first image row
			unsigned long long* item_sums; // [scan_bvh and its builds] the hierarchy's descriptor(s)
			uint32_t* pixel_done;		   // [pass builds] the accumulator (adaptive: the block that starts with it)
		};
		kernel_words pack_words(const rolling_buffers& rolling, const launch_plan& plan, uint32_t first_row)
		{
			const kernel_build& build = plan.build;
			kernel_words words = { plan.queue, rolling.item_sums, rolling.pixel_done };
			// a tile-per-wave launch (below: unless it is a pass) starts at image row first_row: the rows under a sky band (render.hip)
			if (!scan_is_persistent(build.scan))
				words.queue.block_items = first_row;
			if (build.scan == scan_bvh)
				words.item_sums = reinterpret_cast<unsigned long long*>(const_cast<device_bvh*>(rolling.bvh));
#ifndef RT_HIP_FAST_BUILD
			// (the pass builds, as build_of selects them)
			if ((build.scan == scan_resident || build.scan == scan_bvh) && !build.boxes && !build.lights && (build.adaptive || build.pass))
			{
				words.queue.block_items = plan.first_chunk;
				words.pixel_done = reinterpret_cast<uint32_t*>(rolling.accum);
			}
#endif
			return words;
		}
	}

	// picks the instantiation plan.build names and launches it: every decision is the plan's (launch_plan.hpp)
	uint32_t launch_render(const launch_arguments& a)
	{
		const launch_plan& plan = a.plan;
		if (plan.variant == RT_HIP_KERNEL_NONE)
			return RT_HIP_KERNEL_NONE;
		const queue_kernel kernel = select_kernel(plan.build);
		if (!kernel)
			return plan.variant;
		dim3 grid(plan.grid_x, plan.grid_y); // small scenes: the grid of tiles; big scenes: x = the most workgroups the items can occupy
		if (scan_is_persistent(plan.build.scan))
		{
			// persistent launch: exactly what the device keeps resident (surplus workgroups would only find the queue dry).
			// The answer is remembered per context (= per device and host thread of use), per kernel and LDS size.
			launch_cache::entry& known = a.cache.persistent[plan.persistent_slot];
			if (known.lds_bytes != plan.lds_bytes || known.per_cu < 1)
			{
				int per_cu = 0;
				if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, static_cast<int>(block_threads), plan.lds_bytes) != hipSuccess || per_cu < 1)
					per_cu = 4;
				// Not more workgroups than the kernels were compiled for (5 waves per SIMD = 5 workgroups per CU), even when the
				// register allocation of a build happens to leave room for a sixth (round 4 saw 6 144 waves instead of 5 120
				// on one build): the launch's shape should not depend on that.  Measured, it makes no difference either way
				// (config 5: 5.479 against 5.476 s, profiles/r04/persistent_waves_ab.txt).
				per_cu = std::min(per_cu, plan.per_cu_cap);
				(void)hipGetLastError();
				known.lds_bytes = plan.lds_bytes;
				known.per_cu = per_cu;
			}
			grid = dim3(std::min(grid.x, a.compute_units * static_cast<uint32_t>(known.per_cu)));
		}
		const kernel_words words = pack_words(a.rolling, plan, a.first_row);
		hipLaunchKernelGGL(kernel, grid, dim3(block_threads), plan.lds_bytes, a.stream, a.frame, words.queue, a.small, a.scene, a.scene.primitive_geometry, a.d_rgba8, a.d_rgb_f32, a.d_counters, words.item_sums, words.pixel_done);
		return plan.variant;
	}

#ifndef RT_HIP_FAST_BUILD
	void launch_preview(const frame_params& frame, const device_scene& scene, uint32_t* d_rgba8, float* d_rgb_f32, device_counters* d_counters, hipStream_t stream)
	{
		if (!frame.width || !frame.local_rows)
			return;
		const uint32_t rows_per_block = block_threads / 64u;
		const dim3 grid((frame.width + 63u) / 64u, (frame.local_rows + rows_per_block - 1u) / rows_per_block);
		hipLaunchKernelGGL(preview_frame, grid, dim3(block_threads), 0, stream, frame, scene, d_rgba8, d_rgb_f32, d_counters);
	}

	void launch_assemble(uint32_t width,
						 uint32_t height,
						 uint32_t world,
						 uint32_t stripe_rows,
						 uint32_t padded_local_rows,
						 const uint32_t* d_gathered,
						 uint32_t* d_frame,
						 uint32_t first_rank,
						 bool frame_is_host_memory,
						 hipStream_t stream)
	{
		// one workgroup per 256 words of a row; in y one per row while the grid holds them, beyond that a workgroup strides over rows
		// (the multi-GPU frame's height is the render's, up to 131070 rows, and rt_hip_assemble_device puts no cap on it)
		constexpr uint32_t assemble_max_grid_y = 65535u;
		const dim3 grid((width + block_threads - 1) / block_threads, std::min(height, assemble_max_grid_y));
		if (frame_is_host_memory)
			hipLaunchKernelGGL(assemble_stripes<true>, grid, dim3(block_threads), 0, stream, width, height, world, stripe_rows, padded_local_rows, first_rank, d_gathered, d_frame);
		else
			hipLaunchKernelGGL(assemble_stripes<false>, grid, dim3(block_threads), 0, stream, width, height, world, stripe_rows, padded_local_rows, first_rank, d_gathered, d_frame);
	}

#endif // !RT_HIP_FAST_BUILD
}
