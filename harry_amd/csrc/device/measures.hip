// Area, signed volume and box of every shell (shells.cpp) or patch (orient.cpp) of a render build's triangles: the triangles carry a
// label, the labels a lowest triangle ("Shells").  Every floating-point operation is an individually rounded IEEE double
// operation in a fixed order (-ffp-contract=off), and there are no floating-point atomics: the bits depend on the view alone.
// wave64, 256 threads a block.
//   k_sh_chunks    a workgroup per chunk of 256 triangles: the area and volume terms and each triangle's box into LDS; the first
//                  lane of every shell present sums the shell's terms of the chunk in ascending t and leaves the partial in the slot
//                  of its triangle; a chunk that is all one shell (the common case) is summed by thread 0 while the wavefronts
//                  reduce the box by butterflies.  The box goes to the shell by integer atomicMin / atomicMax on an
//                  order-preserving encoding of the float
//   k_sh_pscatter  the marked triangles (one per shell and chunk) into their shell's segment of pseg, in any order (pcount counts
//                  down as the cursor), behind the scan of pcount into pstart
//   k_sh_sums      a lane per shell: sorts its segment (ascending triangle = ascending chunk; one entry almost everywhere) and adds
//                  the partials left to right; more than kSegMax entries are listed for k_sh_hubs
//   k_sh_hubs      a workgroup per listed shell: its entries into the slots of their chunks in LDS (chunks spanning more than 8192:
//                  bitonic sort of the segment where it lies, seg_sort.hpp), then tiles of 256 partials through LDS, thread 0
//                  adding them left to right.  The list has a slot for every shell that can qualify: it cannot overflow
#include <hip/hip_runtime.h>

#include "dev_types.hpp"
#include "hip_handles.hpp"
#include "kernels.hpp"
#include "seg_sort.hpp"
#include "wave.hpp"

namespace hry {
namespace dev {

namespace {

constexpr uint32_t kShellChunk = 256, kSegMax = 32, kHubLds = 8192;

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 sub(const D3 &a, const D3 &b) { return D3{ a.x - b.x, a.y - b.y, a.z - b.z }; }
__device__ __forceinline__ D3 cross(const D3 &a, const D3 &b) { return D3{ a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
__device__ __forceinline__ double dot(const D3 &a, const D3 &b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ double length(const D3 &a) { return sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
__device__ __forceinline__ double finite_or_zero(double x) { return fabs(x) < __builtin_inf() ? x : 0.0; }   // (NaN: 0)

// the float rows of output vertex u; nullptr for an index no render build writes
__device__ __forceinline__ const float *row(const MeasuresView &v, uint32_t u) { return u < v.nout ? v.pos + (size_t)u * v.pos_stride : nullptr; }
__device__ __forceinline__ D3 position(const MeasuresView &v, uint32_t u)
{
	const float *p = row(v, u);
	if (!p) { const double q = __builtin_nan(""); return D3{ q, q, q }; }
	return D3{ (double)p[0], (double)p[1], (double)p[2] };
}

// floats as unsigned keys in the floats' order, -0 below +0; no finite float has the key 0 or 0xffffffff
__device__ __forceinline__ uint32_t float_key(float f)
{
	const uint32_t b = __float_as_uint(f);
	return b & 0x80000000u ? ~b : b | 0x80000000u;
}
__device__ __forceinline__ float key_float(uint32_t k) { return __uint_as_float(k & 0x80000000u ? k & 0x7fffffffu : ~k); }

// area, signed volume and box of shell s from its sums
__device__ __forceinline__ void finish_shell(const MeasuresView &v, const MeasuresWork &w, uint32_t s, double area, double volume)
{
	float *m = v.measures + (size_t)s * 8;
	m[0] = (float)(0.5 * area);
	m[1] = (float)(volume / 6.0);
	for (uint32_t k = 0; k < 3; ++k) {
		const uint32_t lo = w.box_lo[(size_t)s * 3 + k], hi = w.box_hi[(size_t)s * 3 + k];
		m[2 + k] = lo == kNoElement ? __builtin_inff() : key_float(lo);
		m[5 + k] = hi == 0 ? -__builtin_inff() : key_float(hi);
	}
}

}   // namespace

__global__ __launch_bounds__(256) void k_sh_chunks(MeasuresView v, MeasuresWork w)
{
	__shared__ uint32_t l_shell[kShellChunk], l_lo[kShellChunk][3], l_hi[kShellChunk][3], l_red[4][6];
	__shared__ double l_area[kShellChunk], l_vol[kShellChunk];
	const uint32_t tid = threadIdx.x, base = blockIdx.x * kShellChunk, t = base + tid;
	const bool valid = t < v.ntri;
	const uint32_t shell = valid ? v.label[t] : kNoElement;
	uint32_t lo[3] = { kNoElement, kNoElement, kNoElement }, hi[3] = { 0, 0, 0 };
	double area = 0.0, vol = 0.0;
	if (valid && shell < v.nl) {
		const uint32_t i0 = v.indices[3 * (size_t)t], i1 = v.indices[3 * (size_t)t + 1], i2 = v.indices[3 * (size_t)t + 2];
		const D3 p0 = position(v, i0), p1 = position(v, i1), p2 = position(v, i2);
		area = finite_or_zero(length(cross(sub(p1, p0), sub(p2, p0))));
		const uint32_t t0 = v.first[shell];
		const D3 o = position(v, t0 < v.ntri ? v.indices[3 * (size_t)t0] : kNoElement);
		vol = finite_or_zero(dot(sub(p0, o), cross(sub(p1, o), sub(p2, o))));
		const uint32_t idx[3] = { i0, i1, i2 };
		for (int c = 0; c < 3; ++c) {
			const float *p = row(v, idx[c]);
			if (!p) continue;
			for (int k = 0; k < 3; ++k) {
				const float x = p[k];
				if (!(fabsf(x) < __builtin_inff())) continue;
				const uint32_t key = float_key(x);
				lo[k] = min(lo[k], key); hi[k] = max(hi[k], key);
			}
		}
	}
	l_shell[tid] = shell; l_area[tid] = area; l_vol[tid] = vol;
	for (int k = 0; k < 3; ++k) { l_lo[tid][k] = lo[k]; l_hi[tid][k] = hi[k]; }
	__syncthreads();
	const uint32_t here = min(kShellChunk, v.ntri - base), shell0 = l_shell[0];
	const bool uniform = __syncthreads_and(!valid || shell == shell0) != 0;
	if (uniform) {
		if (shell0 >= v.nl) return;
		// the wavefronts reduce the box while thread 0 adds the terms (invalid lanes hold the neutral keys)
		for (int k = 0; k < 3; ++k) {
			const uint32_t a = wave_min(lo[k]), b = wave_max(hi[k]);
			if ((tid & 63) == 0) { l_red[tid >> 6][k] = a; l_red[tid >> 6][3 + k] = b; }
		}
		if (tid == 0) {
			double A = 0.0, V = 0.0;
			for (uint32_t j = 0; j < here; ++j) { A = A + l_area[j]; V = V + l_vol[j]; }
			w.partial[2 * (size_t)t] = A; w.partial[2 * (size_t)t + 1] = V;
			atomicAdd(&w.pcount[shell0], 1u);
		}
		if (valid) w.flag[t] = tid == 0 ? 1u : 0u;
		__syncthreads();
		if (tid < 3) {
			const uint32_t a = min(min(l_red[0][tid], l_red[1][tid]), min(l_red[2][tid], l_red[3][tid]));
			if (a != kNoElement) atomicMin(&w.box_lo[(size_t)shell0 * 3 + tid], a);
		} else if (tid < 6) {
			const uint32_t b = max(max(l_red[0][tid], l_red[1][tid]), max(l_red[2][tid], l_red[3][tid]));
			if (b != 0) atomicMax(&w.box_hi[(size_t)shell0 * 3 + tid - 3], b);
		}
		return;
	}
	// several shells: the first lane of each speaks for it
	bool first = valid && shell < v.nl && (tid == 0 || l_shell[tid - 1] != shell);
	for (uint32_t j = 0; first && j + 1 < tid; ++j) first = l_shell[j] != shell;
	if (valid) w.flag[t] = first ? 1u : 0u;
	if (!first) return;
	double A = 0.0, V = 0.0;
	for (uint32_t j = tid; j < here; ++j) {
		if (l_shell[j] != shell) continue;
		A = A + l_area[j]; V = V + l_vol[j];
		for (int k = 0; k < 3; ++k) { lo[k] = min(lo[k], l_lo[j][k]); hi[k] = max(hi[k], l_hi[j][k]); }
	}
	w.partial[2 * (size_t)t] = A; w.partial[2 * (size_t)t + 1] = V;
	atomicAdd(&w.pcount[shell], 1u);
	for (int k = 0; k < 3; ++k) {
		if (lo[k] != kNoElement) atomicMin(&w.box_lo[(size_t)shell * 3 + k], lo[k]);
		if (hi[k] != 0) atomicMax(&w.box_hi[(size_t)shell * 3 + k], hi[k]);
	}
}

// (pcount[s] holds s's partials on entry and counts down: the last free slot of the segment is taken first)
__global__ __launch_bounds__(256) void k_sh_pscatter(MeasuresView v, MeasuresWork w)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= v.ntri || !w.flag[t]) return;
	const uint32_t s = v.label[t];
	if (s >= v.nl) return;
	const uint32_t k = atomicSub(&w.pcount[s], 1u);
	const uint64_t at = (uint64_t)w.pstart[s] + k - 1;
	if (k && at < v.ntri) w.pseg[at] = t;
}

__global__ __launch_bounds__(256) void k_sh_sums(MeasuresView v, MeasuresWork w, uint32_t hub_cap)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= v.nl) return;
	const uint32_t b = w.pstart[s], end = w.pstart[s + 1];
	const uint32_t len = end >= b && end <= v.ntri ? end - b : 0;
	if (len > kSegMax) {
		const uint32_t k = atomicAdd(&w.hubs[0], 1u);
		if (k < hub_cap) w.hubs[1 + k] = s;   // (hub_cap: every shell that can have so many partials)
		return;
	}
	uint32_t *a = w.pseg + b;
	for (uint32_t i = 1; i < len; ++i) {   // insertion sort by triangle
		const uint32_t x = a[i];
		uint32_t j = i;
		while (j > 0 && a[j - 1] > x) { a[j] = a[j - 1]; --j; }
		a[j] = x;
	}
	double A = 0.0, V = 0.0;
	for (uint32_t i = 0; i < len; ++i) {
		if (a[i] >= v.ntri) continue;
		A = A + w.partial[2 * (size_t)a[i]]; V = V + w.partial[2 * (size_t)a[i] + 1];
	}
	finish_shell(v, w, s, A, V);
}

__global__ __launch_bounds__(256) void k_sh_hubs(MeasuresView v, MeasuresWork w, uint32_t hub_cap)
{
	__shared__ double l_a[256], l_v[256];
	__shared__ uint32_t l_seg[kHubLds], l_min, l_max;
	const uint32_t listed = min(w.hubs[0], hub_cap), tid = threadIdx.x;
	for (uint32_t h = blockIdx.x; h < listed; h += gridDim.x) {
		const uint32_t s = w.hubs[1 + h];
		if (s >= v.nl) continue;
		const uint32_t b = w.pstart[s], end = w.pstart[s + 1];
		if (end < b || end > v.ntri) continue;
		uint32_t len = end - b;
		uint32_t *a = w.pseg + b;
		// a shell has one entry per chunk: where its chunks span at most kHubLds (two million triangles) every entry goes straight to
		// the slot of its chunk in LDS and nothing is sorted; the slots of chunks without the shell hold kNoElement and add nothing
		if (tid == 0) { l_min = kNoElement; l_max = 0; }
		__syncthreads();
		uint32_t lo = kNoElement, hi = 0;
		for (uint32_t i = tid; i < len; i += 256) if (a[i] < v.ntri) { lo = min(lo, a[i] / kShellChunk); hi = max(hi, a[i] / kShellChunk); }
		lo = wave_min(lo); hi = wave_max(hi);
		if ((tid & 63) == 0 && lo != kNoElement) { atomicMin(&l_min, lo); atomicMax(&l_max, hi); }
		__syncthreads();
		const uint32_t c0 = l_min, span = l_min <= l_max ? l_max - l_min + 1 : 0;
		if (span <= kHubLds) {
			for (uint32_t i = tid; i < span; i += 256) l_seg[i] = kNoElement;
			__syncthreads();
			for (uint32_t i = tid; i < len; i += 256) if (a[i] < v.ntri) l_seg[a[i] / kShellChunk - c0] = a[i];
			__syncthreads();
			a = l_seg; len = span;
		} else block_sort_segment(a, len, tid);
		double A = 0.0, V = 0.0;   // (thread 0's)
		for (uint32_t at = 0; at < len; at += 256) {
			const uint32_t i = at + tid;
			const bool have = i < len && a[i] < v.ntri;
			l_a[tid] = have ? w.partial[2 * (size_t)a[i]] : 0.0;
			l_v[tid] = have ? w.partial[2 * (size_t)a[i] + 1] : 0.0;
			__syncthreads();
			if (tid == 0) for (uint32_t j = 0, m = min(256u, len - at); j < m; ++j) { A = A + l_a[j]; V = V + l_v[j]; }
			__syncthreads();
		}
		if (tid == 0) finish_shell(v, w, s, A, V);
	}
}

// ---- the scratch and the launcher
uint32_t shells_hub_capacity(uint32_t ntri) { return ntri / (kSegMax + 1) + 1; }

size_t measures_reserve(Carve &W, uint32_t T)   // (at most T labels of everything per label)
{
	const size_t first = W.reserve((size_t)T * 16);                                          // partial
	W.reserve((size_t)T * 4); W.reserve(((size_t)T + 1) * 4); W.reserve((size_t)T * 4);      // pcount, pstart, pseg
	W.reserve((size_t)T * 12); W.reserve((size_t)T * 12);                                    // box_lo, box_hi
	W.reserve(((size_t)shells_hub_capacity(T) + 1) * 4);                                     // hubs
	return first;
}

MeasuresWork measures_bind(const Carve &W, void *base, size_t first, uint32_t *flag, uint32_t *sums)
{
	MeasuresWork w{};
	w.flag = flag; w.sums = sums;
	w.partial = W.ptr<double>(base, first); w.pcount = W.ptr<uint32_t>(base, first + 1); w.pstart = W.ptr<uint32_t>(base, first + 2);
	w.pseg = W.ptr<uint32_t>(base, first + 3); w.box_lo = W.ptr<uint32_t>(base, first + 4); w.box_hi = W.ptr<uint32_t>(base, first + 5);
	w.hubs = W.ptr<uint32_t>(base, first + 6);
	return w;
}

void measures_clear(hipStream_t st, const MeasuresWork &w, uint32_t nl)
{
	HIP_OK(hipMemsetAsync(w.pcount, 0, (size_t)nl * 4, st));
	HIP_OK(hipMemsetAsync(w.box_lo, 0xff, (size_t)nl * 12, st));
	HIP_OK(hipMemsetAsync(w.box_hi, 0, (size_t)nl * 12, st));
	HIP_OK(hipMemsetAsync(w.hubs, 0, 4, st));
}

void launch_measures(hipStream_t st, const MeasuresView &v, const MeasuresWork &w)
{
	if (!v.ntri || !v.nl || !v.pos) return;
	const uint32_t cap = shells_hub_capacity(v.ntri);
	hipLaunchKernelGGL(k_sh_chunks, dim3(blocks_for(v.ntri, kShellChunk)), dim3(256), 0, st, v, w);
	launch_excl_scan(st, w.pcount, v.nl, w.sums, w.pstart);
	hipLaunchKernelGGL(k_sh_pscatter, dim3(blocks_for(v.ntri, 256)), dim3(256), 0, st, v, w);
	hipLaunchKernelGGL(k_sh_sums, dim3(blocks_for(v.nl, 256)), dim3(256), 0, st, v, w, cap);
	hipLaunchKernelGGL(k_sh_hubs, dim3(std::min<uint32_t>(cap, 1024)), dim3(256), 0, st, v, w, cap);
}

}   // namespace dev
}   // namespace hry
