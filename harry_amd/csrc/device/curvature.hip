// Vertex areas and curvatures of a render build (driver: curvature.cpp; contract: include/harry_amd.h, hry_curvature_build; DESIGN.md
// 7a, "Curvature").  The pattern of normals.hip, tangents.hip and creases.hip -- count, scan, scatter, order per segment -- with the
// slots of one DECODED vertex as a segment: a uv seam does not cut the ring a curvature is summed over.  A slot's eight terms (its
// angle, its share of the mixed area, its Laplace vector, its triangle's normal) are recomputed from the three positions of its
// triangle where the vertex sums them: no per-triangle buffer is written and read back (DESIGN.md counts both variants).  Every
// floating-point operation is an individually rounded IEEE double operation in a fixed order (the tree is built with
// -ffp-contract=off), and there are no floating-point atomics: the bits of every buffer and of the totals depend on the render build
// and its edges build alone.
//   k_cur_ends      a lane per edge: where edge_offsets gives it one side, or more than two, the two decoded ends of its first side
//                   get bit 0, or bit 1 (integer atomic-or)
//   k_cur_count     one counter per decoded vertex: its slots (integer atomics)
//   k_scan_*        exclusive scan of the counters (scan.hip: launch_excl_scan)
//   k_cur_scatter   slots into their vertex's segment, in any order (the counters count down as cursors)
//   k_cur_vertices  a lane per decoded vertex: sorts its segment by slot (insertion sort: a handful of entries), adds the eight sums
//                   in that order, finishes the vertex into the working buffer; per wavefront a ballot and one integer atomic per
//                   class (wave_counter.hpp).
//                   Segments of more than kCurvSegMax slots are listed for k_cur_hubs
//   k_cur_hubs      a workgroup per listed vertex: bitonic sort of the segment where it lies (seg_sort.hpp), every thread sums one
//                   contiguous range of it in order and thread 0 adds the 256 partial sums in thread order -- the association of
//                   normals.hip, which the segment's length alone determines -- and finishes the vertex.  The list has a slot for
//                   every vertex that can qualify (3 T / (kCurvSegMax + 1)): it cannot overflow
//   k_cur_expand    a lane per output vertex: the row of its decoded vertex, into the six buffers
//   k_cur_fold      the totals: a workgroup per 256 consecutive rows of three doubles, three threads add one column each in row
//                   order from +0; launched in rounds until one row remains
// Random access with L2-resident gathers; bytes per triangle of a closed manifold triangle mesh (D = T / 2, E = 3 T / 2): DESIGN.md
// "Curvature" counts them.
#include <hip/hip_runtime.h>

#include "dev_types.hpp"
#include "face_normal.hpp"
#include "kernels.hpp"
#include "seg_sort.hpp"
#include "wave_counter.hpp"

namespace hry {
namespace dev {

namespace {

constexpr uint32_t kCurvSegMax = 32, kCurvFold = 256;
constexpr double kPi = 3.14159265358979323846, kTwoPi = 6.28318530717958647692;   // the doubles nearest pi and 2 pi

__device__ __forceinline__ D3 position(const CurvView &v, uint32_t u)
{
	if (u >= v.nout) { const double q = __builtin_nan(""); return D3{ q, q, q }; }   // (no render build writes such an index)
	const float *p = v.pos + (size_t)u * v.pos_stride;
	return D3{ (double)p[0], (double)p[1], (double)p[2] };
}
__device__ __forceinline__ double dot3(const D3 &a, const D3 &b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ bool finite1(double x) { return fabs(x) < __builtin_inf(); }   // (false for NaN)

// corner k of a triangle: d_k = a . b, x_k = |a x b|, c_k = d_k / x_k or 0 (the rule of edge_cot)
struct Corner { double d, x, c; };
__device__ __forceinline__ Corner corner_of(const D3 &a, const D3 &b)
{
	const double x = length3(cross3(a, b)), d = dot3(a, b), q = d / x;
	return Corner{ d, x, usable_length(x) && finite1(q) ? q : 0.0 };
}

// the running sums of one decoded vertex, or of one range of a hub's segment
struct Sums { double theta, area; D3 L, S; };
__device__ __forceinline__ Sums no_sums() { return Sums{ 0.0, 0.0, D3{ 0.0, 0.0, 0.0 }, D3{ 0.0, 0.0, 0.0 } }; }

// what slot s adds.  The three corners are worked out in the triangle's own order and the slot's are picked by selects: nothing here
// is indexed at run time, so everything stays in registers
__device__ __forceinline__ void add_slot(const CurvView &v, uint32_t s, Sums &acc)
{
	if (s >= v.n) return;
	const uint32_t t = s / 3, k = s - 3 * t;
	const D3 p0 = position(v, v.indices[3 * t]), p1 = position(v, v.indices[3 * t + 1]), p2 = position(v, v.indices[3 * t + 2]);
	const D3 a0 = sub3(p1, p0), b0 = sub3(p2, p0);
	const D3 N = cross3(a0, b0);
	const double len = length3(N);
	if (!usable_length(len)) return;   // a triangle without a normal contributes no terms
	const D3 a1 = sub3(p2, p1), b1 = sub3(p0, p1), a2 = sub3(p0, p2), b2 = sub3(p1, p2);
	const Corner c0 = corner_of(a0, b0), c1 = corner_of(a1, b1), c2 = corner_of(a2, b2);
	const D3 a = k == 0 ? a0 : k == 1 ? a1 : a2, b = k == 0 ? b0 : k == 1 ? b1 : b2;
	const double dk = k == 0 ? c0.d : k == 1 ? c1.d : c2.d, xk = k == 0 ? c0.x : k == 1 ? c1.x : c2.x;
	const double cn = k == 0 ? c1.c : k == 1 ? c2.c : c0.c;   // c at corner k + 1, opposite edge b
	const double cp = k == 0 ? c2.c : k == 1 ? c0.c : c1.c;   // c at corner k + 2, opposite edge a
	const double area_t = 0.5 * len;
	const bool obtuse = c0.d < 0.0 || c1.d < 0.0 || c2.d < 0.0;
	const double share = obtuse ? (dk < 0.0 ? 0.5 * area_t : 0.25 * area_t) : 0.125 * (dot3(a, a) * cp + dot3(b, b) * cn);
	acc.theta += atan2(xk, dk);
	acc.area += share;
	acc.L.x += -(cp * a.x + cn * b.x); acc.L.y += -(cp * a.y + cn * b.y); acc.L.z += -(cp * a.z + cn * b.z);
	acc.S.x += N.x; acc.S.y += N.y; acc.S.z += N.z;
}

// decoded vertex d with `slots` slots and the sums a: its class, its row of seven floats and its three terms of the totals
__device__ __forceinline__ uint32_t finish_vertex(const CurvWork &w, uint32_t d, uint32_t slots, const Sums &a)
{
	const uint32_t ends = w.ends[d];
	const uint32_t base = !slots ? 0u : (ends & 2u) ? 3u : (ends & 1u) ? 2u : 1u;
	const bool ok = usable_length(a.area);
	const double defect = base == 0 ? 0.0 : (base == 2 ? kPi : kTwoPi) - a.theta;
	const double four = 4.0 * a.area, ls = length3(a.S);
	const double H = usable_length(ls) ? dot3(a.L, a.S) / (ls * four) : length3(a.L) / four;
	float *o = w.rows + (size_t)d * 7;
	o[0] = ok ? (float)a.area : 0.0f;
	o[1] = (float)defect;
	o[2] = ok ? (float)(defect / a.area) : 0.0f;
	o[3] = ok ? (float)(a.L.x / four) : 0.0f; o[4] = ok ? (float)(a.L.y / four) : 0.0f; o[5] = ok ? (float)(a.L.z / four) : 0.0f;
	o[6] = ok ? (float)H : 0.0f;
	const bool live = base != 0 && ok;
	double *q = w.terms + (size_t)d * 3;
	q[0] = live ? a.area : 0.0; q[1] = live ? defect : 0.0; q[2] = live ? H * a.area : 0.0;
	const uint32_t cls = base | (ok ? 0u : 8u);
	w.cls[d] = cls;
	return cls;
}

}   // namespace

__global__ __launch_bounds__(256) void k_cur_ends(CurvView v, uint32_t *ends)
{
	const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t b = 0, end = 0;
	if (!side_segment(v, e, b, end) || end <= b) return;
	const uint32_t len = end - b;
	if (len == 2) return;
	const uint32_t s = v.sides[b], bit = len == 1 ? 1u : 2u;
	if (s >= v.n) return;   // (no edges build writes such a side)
	const uint32_t d0 = vertex_of(v, v.indices[s]), d1 = vertex_of(v, v.indices[next_corner(s)]);
	if (d0 < v.nv) atomicOr(&ends[d0], bit);
	if (d1 < v.nv) atomicOr(&ends[d1], bit);
}

__global__ __launch_bounds__(256) void k_cur_count(CurvView v, uint32_t *count)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= v.n) return;
	const uint32_t d = vertex_of(v, v.indices[s]);
	if (d < v.nv) atomicAdd(&count[d], 1u);
}

// (count[d] holds d's slots on entry and counts down: the last free place of the segment is taken first)
__global__ __launch_bounds__(256) void k_cur_scatter(CurvView v, const uint32_t *start, uint32_t *count, uint32_t *seg)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= v.n) return;
	const uint32_t d = vertex_of(v, v.indices[s]);
	if (d >= v.nv) return;
	const uint32_t k = atomicSub(&count[d], 1u);
	const uint64_t pos = (uint64_t)start[d] + k - 1;
	if (k && pos < v.n) seg[pos] = s;
}

// classes: interior, boundary, irregular, isolated vertices, vertices with bit 8
__global__ __launch_bounds__(256) void k_cur_vertices(CurvView v, CurvWork w, uint32_t hub_cap)
{
	const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t cls = kNoElement;   // (a lane without a vertex, or with one k_cur_hubs finishes and counts)
	if (d < v.nv) {
		const uint32_t b = w.start[d], e = w.start[d + 1];
		const uint32_t len = e >= b && e <= v.n ? e - b : 0;
		if (len > kCurvSegMax) {
			const uint32_t k = atomicAdd(&w.hubs[0], 1u);
			if (k < hub_cap) w.hubs[1 + k] = d;   // (hub_cap: every vertex that can have so many slots)
		} else {
			uint32_t *a = w.seg + b;
			for (uint32_t i = 1; i < len; ++i) {   // insertion sort by slot
				const uint32_t x = a[i];
				uint32_t j = i;
				while (j > 0 && a[j - 1] > x) { a[j] = a[j - 1]; --j; }
				a[j] = x;
			}
			Sums s = no_sums();
			for (uint32_t i = 0; i < len; ++i) add_slot(v, a[i], s);
			cls = finish_vertex(w, d, len, s);
		}
	}
	// the classes, a wavefront at a time (every lane takes part): the five counters are the columns of one row of wave_counter.hpp
	const bool counted = cls != kNoElement;
	const uint32_t base = cls & 7u;
	const bool add[5] = { base == 1, base == 2, base == 3, base == 0, (cls & 8u) != 0 };
	const uint32_t col[5] = { 0, 1, 2, 3, 4 };
	WaveCounter<5> classes;
	classes.add(w.classes, 1, counted, 0, add, col);
	classes.flush(w.classes, col);
}

__global__ __launch_bounds__(256) void k_cur_hubs(CurvView v, CurvWork w, uint32_t hub_cap)
{
	__shared__ double part[8 * 256];
	const uint32_t listed = min(w.hubs[0], hub_cap), tid = threadIdx.x;
	for (uint32_t h = blockIdx.x; h < listed; h += gridDim.x) {
		const uint32_t d = w.hubs[1 + h];
		if (d >= v.nv) continue;
		const uint32_t b = w.start[d], e = w.start[d + 1];
		if (e < b || e > v.n) continue;
		const uint64_t len = e - b;
		uint32_t *a = w.seg + b;
		block_sort_segment(a, len, tid);
		const uint64_t chunk = (len + 255) / 256, lo = min(len, tid * chunk), hi = min(len, lo + chunk);
		Sums s = no_sums();
		for (uint64_t i = lo; i < hi; ++i) add_slot(v, a[i], s);
		double *p = part + 8 * tid;
		p[0] = s.theta; p[1] = s.area; p[2] = s.L.x; p[3] = s.L.y; p[4] = s.L.z; p[5] = s.S.x; p[6] = s.S.y; p[7] = s.S.z;
		__syncthreads();
		if (tid == 0) {
			for (uint32_t t = 1; t < 256; ++t) {
				const double *q = part + 8 * t;
				s.theta += q[0]; s.area += q[1]; s.L.x += q[2]; s.L.y += q[3]; s.L.z += q[4]; s.S.x += q[5]; s.S.y += q[6]; s.S.z += q[7];
			}
			const uint32_t cls = finish_vertex(w, d, (uint32_t)len, s);
			atomicAdd(&w.classes[(cls & 7u) == 1 ? 0 : (cls & 7u) == 2 ? 1 : (cls & 7u) == 3 ? 2 : 3], 1u);
			if (cls & 8u) atomicAdd(&w.classes[4], 1u);
		}
		__syncthreads();
	}
}

__global__ __launch_bounds__(256) void k_cur_expand(CurvView v, const uint32_t *cls, const float *rows)
{
	const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
	if (u >= v.nout) return;
	const uint32_t d = v.vsrc[u];
	const bool ok = d < v.nv;   // (no render build names another vertex)
	const float *r = rows + (size_t)(ok ? d : 0) * 7;
	v.vertex_class[u] = ok ? cls[d] : 8u;
	v.area[u] = ok ? r[0] : 0.0f;
	v.defect[u] = ok ? r[1] : 0.0f;
	v.gaussian[u] = ok ? r[2] : 0.0f;
	float *o = v.mean_normal + (size_t)u * 3;
	o[0] = ok ? r[3] : 0.0f; o[1] = ok ? r[4] : 0.0f; o[2] = ok ? r[5] : 0.0f;
	v.mean[u] = ok ? r[6] : 0.0f;
}

// out[c] = the sum of rows [256 c, 256 c + 256) of src, per column, from +0 in row order
__global__ __launch_bounds__(256) void k_cur_fold(const double *src, uint32_t rows, double *out)
{
	__shared__ double part[3 * kCurvFold];
	const uint32_t c = blockIdx.x, tid = threadIdx.x;
	const uint64_t row = (uint64_t)c * kCurvFold + tid;
	const uint32_t here = (uint32_t)min((uint64_t)kCurvFold, (uint64_t)rows - (uint64_t)c * kCurvFold);
	if (tid < here) { part[3 * tid] = src[row * 3]; part[3 * tid + 1] = src[row * 3 + 1]; part[3 * tid + 2] = src[row * 3 + 2]; }
	__syncthreads();
	if (tid < 3) {
		double s = 0.0;
		for (uint32_t i = 0; i < here; ++i) s += part[3 * i + tid];
		out[(size_t)c * 3 + tid] = s;
	}
}

// ---- launchers
uint32_t curvature_hub_capacity(uint32_t nslots) { return nslots / (kCurvSegMax + 1) + 1; }
uint32_t curvature_fold_rows(uint32_t rows) { return (uint32_t)(((uint64_t)rows + kCurvFold - 1) / kCurvFold); }

const double *launch_curvature(hipStream_t st, const CurvView &v, const CurvWork &w)
{
	const uint32_t cap = curvature_hub_capacity(v.n);
	if (v.nv) {
		if (v.ne) hipLaunchKernelGGL(k_cur_ends, dim3(blocks_for(v.ne, 256)), dim3(256), 0, st, v, w.ends);
		if (v.n) hipLaunchKernelGGL(k_cur_count, dim3(blocks_for(v.n, 256)), dim3(256), 0, st, v, w.count);
		launch_excl_scan(st, w.count, v.nv, w.sums, w.start);
		if (v.n) hipLaunchKernelGGL(k_cur_scatter, dim3(blocks_for(v.n, 256)), dim3(256), 0, st, v, (const uint32_t*)w.start, w.count, w.seg);
		hipLaunchKernelGGL(k_cur_vertices, dim3(blocks_for(v.nv, 256)), dim3(256), 0, st, v, w, cap);
		hipLaunchKernelGGL(k_cur_hubs, dim3(std::min<uint32_t>(cap, 1024)), dim3(256), 0, st, v, w, cap);
	}
	if (v.nout) hipLaunchKernelGGL(k_cur_expand, dim3(blocks_for(v.nout, 256)), dim3(256), 0, st, v, (const uint32_t*)w.cls, (const float*)w.rows);
	if (!v.nv) return nullptr;
	// the totals: rounds of 256 rows into one, at least one round, until one row remains
	const double *src = w.terms;
	double *dst = w.fold_a;
	uint32_t rows = v.nv;
	do {
		const uint32_t folded = curvature_fold_rows(rows);
		hipLaunchKernelGGL(k_cur_fold, dim3(folded), dim3(256), 0, st, src, rows, dst);
		src = dst; rows = folded;
		dst = dst == w.fold_a ? w.fold_b : w.fold_a;
	} while (rows > 1);
	return src;
}

}   // namespace dev
}   // namespace hry
