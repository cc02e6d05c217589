// Wavefront and block primitives of the device code: the ONE prefix scan and the ONE butterfly reduction per level.  Device-only,
// wave64 (gfx9): the lane of a thread is threadIdx.x & 63, whatever the block's size, and every lane of the wavefront calls.
// T: uint32_t or unsigned long long.  The grid level (three launches, or one block over everything) is scan.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace hry {
namespace dev {

// inclusive prefix sum over the lanes; W: the lanes 0 .. W - 1 hold the values that count (a power of two; the others get rubbish)
template <typename T, int W = 64>
__device__ __forceinline__ T wave_incl_scan(T v)
{
	const int lane = threadIdx.x & 63;
#pragma unroll
	for (int d = 1; d < W; d <<= 1) { const T o = __shfl_up(v, d, 64); if (lane >= d) v += o; }
	return v;
}
// exclusive prefix sum; total: the sum over the wavefront, in every lane
template <typename T>
__device__ __forceinline__ T wave_excl_scan(T v, T &total)
{
	const T inc = wave_incl_scan(v);
	total = __shfl(inc, 63, 64);
	return inc - v;
}

// xor butterflies: the result in every lane
template <typename T> __device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
	for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
	return v;
}
template <typename T> __device__ __forceinline__ T wave_max(T v)
{
#pragma unroll
	for (int d = 32; d; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
	return v;
}
template <typename T> __device__ __forceinline__ T wave_min(T v)
{
#pragma unroll
	for (int d = 32; d; d >>= 1) { const T o = __shfl_xor(v, d, 64); v = o < v ? o : v; }
	return v;
}

// exclusive prefix sum over a block of 1024 threads: a scan per wavefront, then wave 0 scans the 16 wave totals.  s_wave: 17
// words of LDS; two barriers, so every thread of the block calls, and a caller that calls again puts a barrier in between.
// block_total: the sum over the block, in every thread
template <typename T>
__device__ __forceinline__ T block_excl_scan(T v, T *s_wave, T &block_total)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const T inc = wave_incl_scan(v);
	if (lane == 63) s_wave[wave] = inc;
	__syncthreads();
	if (wave == 0) {
		const T w = lane < 16 ? s_wave[lane] : T(0), wi = wave_incl_scan<T, 16>(w);
		if (lane < 16) s_wave[lane] = wi - w;
		if (lane == 15) s_wave[16] = wi;
	}
	__syncthreads();
	block_total = s_wave[16];
	return s_wave[wave] + inc - v;
}

}   // namespace dev
}   // namespace hry
