// Ordering one long segment of 32-bit ids where it lies in global memory, by a workgroup of 256 threads (normals.hip: k_nrm_hubs,
// edges.hip: k_edge_hubs).  Every thread of the block calls block_sort_segment; it ends with a barrier.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace hry {
namespace dev {

__device__ __forceinline__ void order_pair(uint32_t *a, uint64_t i, uint64_t p, uint64_t len)
{
	if (p >= len) return;   // (beyond the segment: a virtual +infinity, which stays where it is)
	const uint32_t x = a[i], y = a[p];
	if (x > y) { a[i] = y; a[p] = x; }
}

// bitonic sort with every comparison ascending (mirror, then halving strides), so that the end of the segment needs no padding
__device__ __forceinline__ void block_sort_segment(uint32_t *a, uint64_t len, uint32_t tid)
{
	for (uint64_t k = 2; (k >> 1) < len; k <<= 1) {
		const uint64_t half = k >> 1, pairs = ((len + k - 1) / k) * half;
		for (uint64_t t = tid; t < pairs; t += 256) {
			const uint64_t base = (t / half) * k, j = t % half;
			order_pair(a, base + j, base + k - 1 - j, len);
		}
		__syncthreads();
		for (uint64_t j = k >> 2; j > 0; j >>= 1) {
			for (uint64_t t = tid; t < pairs; t += 256) {
				const uint64_t i = (t / j) * 2 * j + t % j;
				order_pair(a, i, i + j, len);
			}
			__syncthreads();
		}
	}
}

}   // namespace dev
}   // namespace hry
