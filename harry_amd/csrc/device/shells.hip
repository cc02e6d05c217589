// Shells of a render build: the connected pieces of its triangles, their counts, boundary loops and measures (driver: shells.cpp;
// contract: include/harry_amd.h, hry_shells_build; DESIGN.md 7a, "Shells").  The adjacency is the edges build's: every side knows
// its edge (tri_edges) and every edge its sides in ascending order (edge_offsets / edge_sides).  wave64, 256 threads a block.
//   k_sh_hook_local / k_sh_hook  lock-free union-find over the triangles (union_find.hpp): a side unites its triangle with the triangle
//                              of its edge's first side -- first inside a workgroup's 8192 triangles in LDS, then, for the sides that
//                              leave them, in HBM.  The root of a shell is its lowest triangle
//   k_sh_roots + k_scan_*      root flags and their exclusive scan: dense shell numbers in order of the lowest triangle
//   k_sh_label                 a lane per triangle: walks to its root (the unions are over), tri_shell, face_shell, shell_first;
//                              triangles and faces per shell
//   k_dedup_*<ShellVertexKey>  (dedup.hip) numbers the distinct (shell, decoded vertex) pairs over the 3 T corners
//   k_sh_vertices              a lane per corner: the first corner of a pair counts one vertex for its shell
//   k_loop_min                 a lane per edge: edge_shell, loop_par[e] = e; a boundary edge leaves its number, by integer atomicMin,
//                              in the slot of the pair at either end
//   k_loop_hook                a boundary edge unites with what the slots at its two ends hold: a second union-find, over edges.
//                              A slot belongs to one shell's vertex: loops of two shells that touch at a point stay apart
//   k_sh_edges                 a lane per edge: edges, boundary, nonmanifold, misoriented, loops (a boundary edge that is a root)
//   k_sh_summary               a lane per shell: the five reductions of hry_shells_summary behind S
// Every per-shell count is an integer atomic, aggregated per wavefront first (WaveCounter, wave_counter.hpp): neighbouring triangles, edges and corners
// mostly share a shell, so a wavefront sends one atomic per column.
// Measures (every floating-point operation an individually rounded IEEE double operation in a fixed order: -ffp-contract=off; no
// floating-point atomics; the bits depend on the render and edges builds alone):
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
// Bytes per triangle of a closed manifold mesh: DESIGN.md 7a.
#include <hip/hip_runtime.h>

#include "dev_types.hpp"
#include "kernels.hpp"
#include "seg_sort.hpp"
#include "union_find.hpp"
#include "wave.hpp"
#include "wave_counter.hpp"

namespace hry {
namespace dev {

namespace {

constexpr uint32_t kNoElement = 0xffffffffu;
constexpr uint32_t kShellChunk = 256, kSegMax = 32, kHubLds = 8192;
enum : uint32_t { kColTri, kColFace, kColVertex, kColEdge, kColBoundary, kColNonmanifold, kColMisoriented, kColLoops };

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 sub(const D3 &a, const D3 &b) { return D3{ a.x - b.x, a.y - b.y, a.z - b.z }; }
__device__ __forceinline__ D3 cross(const D3 &a, const D3 &b) { return D3{ a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
__device__ __forceinline__ double dot(const D3 &a, const D3 &b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ double length(const D3 &a) { return sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
__device__ __forceinline__ double finite_or_zero(double x) { return fabs(x) < __builtin_inf() ? x : 0.0; }   // (NaN: 0)

// the float rows of output vertex u; nullptr for an index no render build writes
__device__ __forceinline__ const float *row(const ShellsView &v, uint32_t u) { return u < v.nout ? v.pos + (size_t)u * v.pos_stride : nullptr; }
__device__ __forceinline__ D3 position(const ShellsView &v, uint32_t u)
{
	const float *p = row(v, u);
	if (!p) { const double q = __builtin_nan(""); return D3{ q, q, q }; }
	return D3{ (double)p[0], (double)p[1], (double)p[2] };
}
__device__ __forceinline__ uint32_t vertex_of(const ShellsView &v, uint32_t u) { return u < v.nout ? v.vsrc[u] : kNoElement; }
__device__ __forceinline__ uint32_t next_corner(uint32_t s) { return s % 3 == 2 ? s - 2 : s + 1; }

// floats as unsigned keys in the floats' order, -0 below +0; no finite float has the key 0 or 0xffffffff
__device__ __forceinline__ uint32_t float_key(float f)
{
	const uint32_t b = __float_as_uint(f);
	return b & 0x80000000u ? ~b : b | 0x80000000u;
}
__device__ __forceinline__ float key_float(uint32_t k) { return __uint_as_float(k & 0x80000000u ? k & 0x7fffffffu : ~k); }

// the sides of edge e: false for an edge the buffers do not hold
__device__ __forceinline__ bool edge_segment(const ShellsView &v, uint32_t e, uint32_t &b, uint32_t &len)
{
	if (e >= v.ne) return false;
	b = v.offsets[e];
	const uint32_t end = v.offsets[e + 1];
	if (end <= b || end > v.n) return false;
	len = end - b;
	return v.sides[b] < v.n;
}

// area, signed volume and box of shell s from its sums
__device__ __forceinline__ void finish_shell(const ShellsView &v, const ShellsWork &w, uint32_t s, double area, double volume)
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

// the triangle side s hooks its own to: that of its edge's first side (kNoElement: none, or its own)
__device__ __forceinline__ uint32_t hook_target(const ShellsView &v, uint32_t s)
{
	uint32_t b, len;
	if (!edge_segment(v, v.tri_edges[s], b, len)) return kNoElement;
	const uint32_t first = v.sides[b] / 3;
	return first != s / 3 ? first : kNoElement;
}

// In two passes, as k_cc_hook_local / k_cc_hook of twins.hip: triangles that lie near each other in the buffer mostly ARE neighbours,
// so a workgroup first unites its own kHookTris triangles in LDS -- the same lock-free union-find, no traffic -- and writes every
// triangle's local root as its parent; the second pass takes only the sides that leave a workgroup's triangles to the union-find in
// HBM, where a shell now arrives as one root per workgroup instead of triangle by triangle.  Every word of par is written here
constexpr uint32_t kHookTris = 8192, kHookThreads = 1024;   // 32 KB of parents in LDS
__global__ __launch_bounds__(kHookThreads) void k_sh_hook_local(ShellsView v, uint32_t *par)
{
	__shared__ uint32_t l_par[kHookTris];
	const uint32_t base = blockIdx.x * kHookTris;
	for (uint32_t i = threadIdx.x; i < kHookTris; i += kHookThreads) l_par[i] = i;
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < kHookTris; i += kHookThreads) {
		const uint32_t t = base + i;
		if (t >= v.ntri) break;
		for (uint32_t k = 0; k < 3; ++k) {
			const uint32_t o = hook_target(v, 3 * t + k);
			if (o >= v.ntri || o - base >= kHookTris) continue;   // none, or it leaves the workgroup's triangles: the second pass
			lds_unite(l_par, i, o - base);
		}
	}
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < kHookTris; i += kHookThreads) {   // (the unions are over: a root read is final)
		if (base + i >= v.ntri) break;
		uint32_t x = i, q = l_par[x];
		while (q != x) { x = q; q = l_par[x]; }
		par[base + i] = base + x;
	}
}

__global__ __launch_bounds__(256) void k_sh_hook(ShellsView v, uint32_t *par)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= v.n) return;
	const uint32_t t = s / 3, o = hook_target(v, s);
	if (o >= v.ntri || o - (t - t % kHookTris) < kHookTris) return;   // none, or united in LDS by the first pass
	uf_unite(par, t, o);
}

__global__ __launch_bounds__(256) void k_sh_roots(const uint32_t *par, uint32_t n, uint32_t *flag)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) flag[i] = par[i] == i ? 1u : 0u;
}

// (the unions are over: the walk reads final parents with plain loads and stores nothing into par)
__global__ __launch_bounds__(256) void k_sh_label(ShellsView v, const uint32_t *par, const uint32_t *num)
{
	const uint32_t col[2] = { kColTri, kColFace };
	WaveCounter<2> wc;
	for (uint32_t tile = 0; tile < kTiles; ++tile) {
		const uint64_t at = ((uint64_t)blockIdx.x * kTiles + tile) * 256 + threadIdx.x;
		const uint32_t t = (uint32_t)at;
		const bool valid = at < v.ntri;
		uint32_t shell = kNoElement;
		bool new_face = false;
		if (valid) {
			uint32_t x = t, p = par[x];
			while (p != x && p < v.ntri) { x = p; p = par[x]; }
			shell = num[x];
			v.tri_shell[t] = shell;
			if (x == t && shell < v.ns) v.first[shell] = t;
			const uint32_t f = v.tri_face[t];
			if (f < v.nf) {
				v.face_shell[f] = shell;   // (the fan triangles of a face are one shell: they all write the same word)
				new_face = t == 0 || v.tri_face[t - 1] != f;   // (and they are neighbours in the buffer)
			}
		}
		const bool add[2] = { true, new_face };
		wc.add(v.counts, v.ns, valid, shell, add, col);
	}
	wc.flush(v.counts, col);
}

__global__ __launch_bounds__(256) void k_sh_vertices(ShellsView v, const uint32_t *first_of)
{
	const uint32_t col[1] = { kColVertex };
	WaveCounter<1> wc;
	for (uint32_t tile = 0; tile < kTiles; ++tile) {
		const uint64_t at = ((uint64_t)blockIdx.x * kTiles + tile) * 256 + threadIdx.x;
		const uint32_t c = (uint32_t)at;
		const bool valid = at < v.n;
		const bool add[1] = { valid && first_of[c] == c };
		wc.add(v.counts, v.ns, valid, valid ? v.tri_shell[c / 3] : kNoElement, add, col);
	}
	wc.flush(v.counts, col);
}

__global__ __launch_bounds__(256) void k_loop_min(ShellsView v, const uint32_t *pair_id, uint32_t *slot, uint32_t *loop_par)
{
	const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= v.ne) return;
	loop_par[e] = e;
	uint32_t b, len;
	if (!edge_segment(v, e, b, len)) { v.edge_shell[e] = kNoElement; return; }
	const uint32_t s = v.sides[b];
	v.edge_shell[e] = v.tri_shell[s / 3];
	if (len != 1) return;
	const uint32_t p0 = pair_id[s], p1 = pair_id[next_corner(s)];
	if (p0 < v.n) atomicMin(&slot[p0], e);
	if (p1 < v.n) atomicMin(&slot[p1], e);
}

__global__ __launch_bounds__(256) void k_loop_hook(ShellsView v, const uint32_t *pair_id, const uint32_t *slot, uint32_t *loop_par)
{
	const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t b, len;
	if (!edge_segment(v, e, b, len) || len != 1) return;
	const uint32_t s = v.sides[b];
	const uint32_t p0 = pair_id[s], p1 = pair_id[next_corner(s)];
	const uint32_t a0 = p0 < v.n ? slot[p0] : kNoElement, a1 = p1 < v.n ? slot[p1] : kNoElement;
	if (a0 < v.ne && a0 != e) uf_unite(loop_par, e, a0);
	if (a1 < v.ne && a1 != e) uf_unite(loop_par, e, a1);
}

__global__ __launch_bounds__(256) void k_sh_edges(ShellsView v, const uint32_t *loop_par)
{
	const uint32_t col[5] = { kColEdge, kColBoundary, kColNonmanifold, kColMisoriented, kColLoops };
	WaveCounter<5> wc;
	for (uint32_t tile = 0; tile < kTiles; ++tile) {
		const uint64_t at = ((uint64_t)blockIdx.x * kTiles + tile) * 256 + threadIdx.x;
		const uint32_t e = at < v.ne ? (uint32_t)at : kNoElement;
		uint32_t b = 0, len = 0, shell = kNoElement;
		bool valid = edge_segment(v, e, b, len), against = false, root = false;
		if (valid) {
			shell = v.edge_shell[e];
			if (len == 1) root = loop_par[e] == e;
			if (len == 2 && v.sides[b + 1] < v.n) {   // both sides run from the same decoded vertex to the same decoded vertex
				const uint32_t s0 = v.sides[b], s1 = v.sides[b + 1];
				against = vertex_of(v, v.indices[s0]) == vertex_of(v, v.indices[s1]) &&
				          vertex_of(v, v.indices[next_corner(s0)]) == vertex_of(v, v.indices[next_corner(s1)]);
			}
		}
		const bool add[5] = { true, len == 1, len > 2, against, root };
		wc.add(v.counts, v.ns, valid, shell, add, col);
	}
	wc.flush(v.counts, col);
}

// summary: closed, nonmanifold, misoriented (shells), loops (sum), largest (triangles)
__global__ __launch_bounds__(256) void k_sh_summary(const uint32_t *counts, uint32_t ns, uint32_t *summary)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t c[8] = {};
	if (s < ns) for (int k = 0; k < 8; ++k) c[k] = counts[(size_t)s * 8 + k];
	const bool valid = s < ns;
	const uint32_t closed = (uint32_t)__popcll(__ballot(valid && c[kColBoundary] == 0 && c[kColNonmanifold] == 0));
	const uint32_t nonman = (uint32_t)__popcll(__ballot(valid && c[kColNonmanifold] > 0));
	const uint32_t mis = (uint32_t)__popcll(__ballot(valid && c[kColMisoriented] > 0));
	const uint32_t loops = wave_sum(c[kColLoops]), largest = wave_max(c[kColTri]);
	if ((threadIdx.x & 63) == 0) {
		if (closed) atomicAdd(&summary[0], closed);
		if (nonman) atomicAdd(&summary[1], nonman);
		if (mis) atomicAdd(&summary[2], mis);
		if (loops) atomicAdd(&summary[3], loops);
		if (largest) atomicMax(&summary[4], largest);
	}
}

// ---- measures
__global__ __launch_bounds__(256) void k_sh_chunks(ShellsView v, ShellsWork w)
{
	__shared__ uint32_t l_shell[kShellChunk], l_lo[kShellChunk][3], l_hi[kShellChunk][3], l_red[4][6];
	__shared__ double l_area[kShellChunk], l_vol[kShellChunk];
	const uint32_t tid = threadIdx.x, base = blockIdx.x * kShellChunk, t = base + tid;
	const bool valid = t < v.ntri;
	const uint32_t shell = valid ? v.tri_shell[t] : kNoElement;
	uint32_t lo[3] = { kNoElement, kNoElement, kNoElement }, hi[3] = { 0, 0, 0 };
	double area = 0.0, vol = 0.0;
	if (valid && shell < v.ns) {
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
		if (shell0 >= v.ns) return;
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
	bool first = valid && shell < v.ns && (tid == 0 || l_shell[tid - 1] != shell);
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
__global__ __launch_bounds__(256) void k_sh_pscatter(ShellsView v, ShellsWork w)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= v.ntri || !w.flag[t]) return;
	const uint32_t s = v.tri_shell[t];
	if (s >= v.ns) return;
	const uint32_t k = atomicSub(&w.pcount[s], 1u);
	const uint64_t at = (uint64_t)w.pstart[s] + k - 1;
	if (k && at < v.ntri) w.pseg[at] = t;
}

__global__ __launch_bounds__(256) void k_sh_sums(ShellsView v, ShellsWork w, uint32_t hub_cap)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= v.ns) return;
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

__global__ __launch_bounds__(256) void k_sh_hubs(ShellsView v, ShellsWork w, uint32_t hub_cap)
{
	__shared__ double l_a[256], l_v[256];
	__shared__ uint32_t l_seg[kHubLds], l_min, l_max;
	const uint32_t listed = min(w.hubs[0], hub_cap), tid = threadIdx.x;
	for (uint32_t h = blockIdx.x; h < listed; h += gridDim.x) {
		const uint32_t s = w.hubs[1 + h];
		if (s >= v.ns) continue;
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

// ---- launchers
uint32_t shells_hub_capacity(uint32_t ntri) { return ntri / (kSegMax + 1) + 1; }

void launch_shells_roots(hipStream_t st, const ShellsView &v, const ShellsWork &w)
{
	if (v.ntri) {
		hipLaunchKernelGGL(k_sh_hook_local, dim3(blocks_for(v.ntri, kHookTris)), dim3(kHookThreads), 0, st, v, w.par);
		hipLaunchKernelGGL(k_sh_hook, dim3(blocks_for(v.n, 256)), dim3(256), 0, st, v, w.par);
		hipLaunchKernelGGL(k_sh_roots, dim3(blocks_for(v.ntri, 256)), dim3(256), 0, st, (const uint32_t*)w.par, v.ntri, w.flag);
	}
	launch_excl_scan(st, w.flag, v.ntri, w.sums, w.num);
}

void launch_shells_label(hipStream_t st, const ShellsView &v, const ShellsWork &w)
{
	if (v.ntri) hipLaunchKernelGGL(k_sh_label, dim3(blocks_for(v.ntri, 256 * kTiles)), dim3(256), 0, st, v, (const uint32_t*)w.par, (const uint32_t*)w.num);
}

void launch_shells_counts(hipStream_t st, const ShellsView &v, const ShellsWork &w)
{
	if (!v.ntri || !v.ns) return;
	hipLaunchKernelGGL(k_sh_vertices, dim3(blocks_for(v.n, 256 * kTiles)), dim3(256), 0, st, v, w.pair_first_of);
	if (v.ne) {
		const dim3 grid(blocks_for(v.ne, 256));
		hipLaunchKernelGGL(k_loop_min, grid, dim3(256), 0, st, v, (const uint32_t*)w.pair_id, w.slot, w.loop_par);
		hipLaunchKernelGGL(k_loop_hook, grid, dim3(256), 0, st, v, (const uint32_t*)w.pair_id, (const uint32_t*)w.slot, w.loop_par);
		hipLaunchKernelGGL(k_sh_edges, dim3(blocks_for(v.ne, 256 * kTiles)), dim3(256), 0, st, v, (const uint32_t*)w.loop_par);
	}
	hipLaunchKernelGGL(k_sh_summary, dim3(blocks_for(v.ns, 256)), dim3(256), 0, st, (const uint32_t*)v.counts, v.ns, w.summary);
}

void launch_shells_measures(hipStream_t st, const ShellsView &v, const ShellsWork &w)
{
	if (!v.ntri || !v.ns || !v.pos) return;
	const uint32_t cap = shells_hub_capacity(v.ntri);
	hipLaunchKernelGGL(k_sh_chunks, dim3(blocks_for(v.ntri, kShellChunk)), dim3(256), 0, st, v, w);
	launch_excl_scan(st, w.pcount, v.ns, w.sums, w.pstart);
	hipLaunchKernelGGL(k_sh_pscatter, dim3(blocks_for(v.ntri, 256)), dim3(256), 0, st, v, w);
	hipLaunchKernelGGL(k_sh_sums, dim3(blocks_for(v.ns, 256)), dim3(256), 0, st, v, w, cap);
	hipLaunchKernelGGL(k_sh_hubs, dim3(std::min<uint32_t>(cap, 1024)), dim3(256), 0, st, v, w, cap);
}

}   // namespace dev
}   // namespace hry
