// rt_amd/csrc/sky_band.hip — the sky band's kernel: rows [0, R) of a frame whose every primary ray is known to miss (sky_band.hpp has
// the rule, DESIGN.md §5 the measurements).  Scene-free: per (pixel, chunk of 16 samples), in sample order, exactly what a lane of
// render_queue does that restarts and then misses — the same inline functions, the same order of operations — without an origin, a
// probe, a mode word or a vote.  Parity contract only (the band is never taken under RT_HIP_FLAG_FAST).
//
// Shape: a workgroup owns 64 consecutive pixels of one row; its four waves take the chunks of those pixels four at a time (wave w:
// chunks w, 4 + w, ...), a lane per (pixel, chunk), park the chunk sums in LDS, and the first wave folds them onto the pixels' running
// sums in chunk order — the first chunk's sum is the start value, as in fold_tile — and finishes the pixels.  At 1920 x 528 x 256
// samples that is 15 840 workgroups of 4 x 4 short items: every CU is full until the last few.
#include "kernels.hpp"
#include "contract.hpp"
#include "pixel_output.hpp"
#include "lane_state.hpp"
#include "camera_forms.hpp"

namespace rt_hip
{
	namespace
	{
		struct pinhole_build // (camera_forms.hpp: the band exists for the pinhole form alone)
		{
			static constexpr bool PINHOLE_ONLY = true, EYE_ONLY = false, NEVER_PINHOLE = false;
		};

		constexpr uint32_t band_pixels = 64; // of one row, per workgroup

		// p: the frame's constants with local_rows = R, the band's rows (world 1, rank 0: local row = image row = output row)
		__global__ __launch_bounds__(block_threads) void sky_band_rows_kernel(const frame_params p, const uint32_t chunks, uint32_t* __restrict__ out_rgba, float* __restrict__ out_rgb, device_counters* __restrict__ counters)
		{
			__shared__ float sums[block_threads / 64u][3][band_pixels];
			const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
			const uint32_t lx = blockIdx.x * band_pixels + lane, ly = blockIdx.y;
			const uint32_t gy = global_row(ly, p);
			// (a lane beyond the row's end traces like the others — nothing it computes touches memory — and stores nothing)
			lane_state st;
			camera_base<pinhole_build>(st, p, static_cast<float>(lx), static_cast<float>(gy));
			st.keys.function_key = pixel_function_key(p.frame_key_a, gy * p.width + lx);
			st.keys.stride = pixel_stride(p.frame_key_b, st.keys.function_key);
			vec3 colour = { 0.0f, 0.0f, 0.0f };
			for (uint32_t first_chunk = 0; first_chunk < chunks; first_chunk += block_threads / 64u) // (uniform over the workgroup)
			{
				const uint32_t chunk = first_chunk + wave; // (wave-uniform)
				if (chunk < chunks)
				{
					// start_item
					const uint32_t first = chunk * sample_chunk, end = min(first + sample_chunk, p.samples_per_pixel);
					st.chunk_sum = { 0.0f, 0.0f, 0.0f };
					st.window = sample_counter(st.keys.stride, first);
					st.window_end = sample_counter(st.keys.stride, end);
					do
					{
						// the fused tail of a restarting lane: one generator step from the start of the sample's window
						st.counter = st.window + st.keys.stride;
						const uint32_t word = step_word_at(st.counter, st.keys);
						float jx = step_numerator(word * step_mul_a), jy = step_numerator(word * step_mul_b);
						if (st.window == 0u) // sample 0 goes through the pixel centre and draws nothing
							jx = jy = 0x1.0p23f;
						const vec3 toward = { fma(p.ray_j1[0], jx, fma(p.ray_j2[0], jy, st.base_x)), fma(p.ray_j1[1], jx, fma(p.ray_j2[1], jy, st.base_y)),
											  fma(p.ray_j1[2], jx, fma(p.ray_j2[2], jy, st.base_z)) };
						const float inv = inv_sqrt_rn(dot(toward, toward));
						const float dir_y = toward.y * inv;
						// the miss: end_sample(throughput * sky(dir.y)) with the restart's throughput, then next_sample
						st.throughput = { 1.0f, 1.0f, 1.0f };
						st.chunk_sum = st.chunk_sum + st.throughput * sky(dir_y);
						st.window += st.keys.stride << draws_per_sample_log2;
					}
					while (st.window != st.window_end);
					sums[wave][0][lane] = st.chunk_sum.x;
					sums[wave][1][lane] = st.chunk_sum.y;
					sums[wave][2][lane] = st.chunk_sum.z;
				}
				__syncthreads();
				if (wave == 0u)
				{
					const uint32_t parked = min(chunks - first_chunk, block_threads / 64u);
					for (uint32_t k = 0; k < parked; k++)
					{
						const vec3 sum = { sums[k][0][lane], sums[k][1][lane], sums[k][2][lane] };
						colour = (first_chunk + k) ? colour + sum : sum;
					}
				}
				__syncthreads(); // (the slots are written again in the next round)
			}
			if (wave == 0u && lx < p.width)
				finish_pixel(colour, p, lx, ly, out_rgba, out_rgb);
			// one path segment per sample: the count is known, one addition per workgroup
			if (threadIdx.x == 0u)
			{
				const uint32_t pixels = min(band_pixels, p.width - blockIdx.x * band_pixels);
				atomicAdd(&counters->segments[(blockIdx.x + blockIdx.y * 7u) % device_counters::segment_counters], static_cast<unsigned long long>(pixels) * p.samples_per_pixel);
			}
		}
	}

	void launch_sky_band(const frame_params& band, uint32_t* d_rgba8, float* d_rgb_f32, device_counters* d_counters, hipStream_t stream)
	{
		if (!band.width || !band.local_rows || !band.samples_per_pixel)
			return;
		const uint32_t chunks = (band.samples_per_pixel + sample_chunk - 1u) / sample_chunk;
		const dim3 grid((band.width + band_pixels - 1u) / band_pixels, band.local_rows);
		hipLaunchKernelGGL(sky_band_rows_kernel, grid, dim3(block_threads), 0, stream, band, chunks, d_rgba8, d_rgb_f32, d_counters);
	}
}
