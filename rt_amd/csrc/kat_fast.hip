// rt_amd/csrc/kat_fast.hip — the one unit of librt_hip_kat.so (TEST-ONLY, include/rt_hip_kat.h) that is compiled as RT_HIP_FLAG_FAST's
// build of the kernels is: the Makefile's FASTFLAGS (-DRT_HIP_FAST_BUILD -ffp-contract=fast), so contract.hpp gives it the fast leaf
// functions — the hardware's v_sqrt / v_rcp / v_rsq as they are, divide() as a multiplication by the reciprocal.  One kernel runs them
// on inputs of the tests' choosing; kat.hip holds the entry point (rt_hip_kat_fast_math) and calls the launcher below.
// Nothing in librt_hip.so refers to this file.
#include "contract.hpp"

#ifndef RT_HIP_FAST_BUILD
#error "kat_fast.hip is built with the Makefile's FASTFLAGS: it measures the fast half of contract.hpp"
#endif

namespace rt_hip
{
namespace
{
	__global__ void kat_fast_math(uint32_t n, const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ out_sqrt, float* __restrict__ out_rcp, float* __restrict__ out_rsq, float* __restrict__ out_div)
	{
		const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
		if (i < n)
		{
			out_sqrt[i] = sqrt_rn(x[i]);
			out_rcp[i] = rcp_rn(x[i]);
			out_rsq[i] = inv_sqrt_rn(x[i]);
			out_div[i] = divide(x[i], y[i]);
		}
	}
}

	// (declared in kat.hip, which owns the buffers: all six hold n floats on the current device)
	void launch_kat_fast_math(uint32_t n, const float* d_x, const float* d_y, float* d_sqrt, float* d_rcp, float* d_rsq, float* d_div, hipStream_t stream)
	{
		constexpr uint32_t threads = 256;
		hipLaunchKernelGGL(kat_fast_math, dim3((n + threads - 1) / threads), dim3(threads), 0, stream, n, d_x, d_y, d_sqrt, d_rcp, d_rsq, d_div);
	}
}
