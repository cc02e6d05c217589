// The grid-level exclusive scans of 32-bit counters and their launchers; the wavefront and block levels are wave.hpp.  Two of them:
//   launch_excl_scan    three launches, any n: block sums (k_scan_sums), scan of the sums by one block (k_scan_top), apply
//                       (k_scan_apply).  Users: the twin matcher and the components (twins.hip), the vertex normals (normals.hip),
//                       the numbering maps (order.cpp), the events (events.hip)
//   launch_scan_counts  one launch of one block, a thread per run of the input (k_scan_counts): for inputs a sixty-fourth of their
//                       problem -- the wavefront counts of the first-occurrence numbering (dedup.hip) and of the ingest's face
//                       offsets (ingest.hip)
// Both stay: which one is better where has not been measured.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "wave.hpp"

namespace hry {
namespace dev {

constexpr int kScanBlock = 1024;   // (what block_excl_scan is written for)

__global__ __launch_bounds__(kScanBlock) void k_scan_sums(const uint32_t *in, uint32_t n, uint32_t *sums)
{
	__shared__ uint32_t s_wave[17];
	const uint32_t i = blockIdx.x * kScanBlock + threadIdx.x;
	uint32_t total;
	block_excl_scan(i < n ? in[i] : 0u, s_wave, total);
	if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
__global__ __launch_bounds__(kScanBlock) void k_scan_top(uint32_t *sums, uint32_t nb)   // one block: exclusive scan in place, any nb
{
	__shared__ uint32_t s_wave[17];
	uint32_t carry = 0;
	for (uint32_t base = 0; base < nb; base += kScanBlock) {
		const uint32_t i = base + threadIdx.x;
		const uint32_t v = i < nb ? sums[i] : 0u;
		uint32_t total;
		const uint32_t ex = block_excl_scan(v, s_wave, total);
		if (i < nb) sums[i] = carry + ex;
		carry += total;
		__syncthreads();
	}
}
__global__ __launch_bounds__(kScanBlock) void k_scan_apply(const uint32_t *in, uint32_t n, const uint32_t *sums, uint32_t *out, uint32_t *total_out)
{
	__shared__ uint32_t s_wave[17];
	const uint32_t i = blockIdx.x * kScanBlock + threadIdx.x;
	const uint32_t v = i < n ? in[i] : 0u;
	uint32_t total;
	const uint32_t ex = block_excl_scan(v, s_wave, total) + sums[blockIdx.x];
	if (i < n) out[i] = ex;
	if (i == n - 1) *total_out = ex + v;
}

size_t scan_sums_words(uint32_t n) { return (size_t)blocks_for(n, kScanBlock) + 2; }
void launch_excl_scan(hipStream_t st, const uint32_t *in, uint32_t n, uint32_t *sums, uint32_t *out, uint32_t *total_out)
{
	if (!total_out) total_out = out + n;
	if (!n) { (void)hipMemsetAsync(total_out, 0, 4, st); return; }
	const unsigned nb = blocks_for(n, kScanBlock);
	hipLaunchKernelGGL(k_scan_sums, dim3(nb), dim3(kScanBlock), 0, st, in, n, sums);
	hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(kScanBlock), 0, st, sums, nb);
	hipLaunchKernelGGL(k_scan_apply, dim3(nb), dim3(kScanBlock), 0, st, in, n, (const uint32_t*)sums, out, total_out);
}

// one block: a thread sums its run of (n + 1023) / 1024 entries, the block scans the 1024 sums, the thread writes its run
__global__ __launch_bounds__(kScanBlock) void k_scan_counts(const uint32_t *counts, uint32_t n, uint32_t *out)
{
	__shared__ uint32_t s_wave[17];
	const uint32_t per = (n + 1023) / 1024, b = threadIdx.x * per, e = min(n, b + per);
	uint32_t sum = 0;
	for (uint32_t i = b; i < e; ++i) sum += counts[i];
	uint32_t total, run = block_excl_scan(sum, s_wave, total);
	for (uint32_t i = b; i < e; ++i) { out[i] = run; run += counts[i]; }
	if (threadIdx.x == 1023) out[n] = total;
}
void launch_scan_counts(hipStream_t st, const uint32_t *counts, uint32_t n, uint32_t *out)
{
	hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(kScanBlock), 0, st, counts, n, out);
}

}   // namespace dev
}   // namespace hry
