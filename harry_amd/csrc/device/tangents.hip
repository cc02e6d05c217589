// Tangent frames of a render build (driver: tangents.cpp; contract: include/harry_amd.h, hry_tangents_build; DESIGN.md 7a,
// "Tangents").  The pattern of normals.hip and edges.hip -- count, scan, scatter, order per segment -- with other segments: the
// items are the 3 T index slots of the triangles and a segment is the slots of one OUTPUT vertex, so that a uv seam splits the frame.
// Every floating-point operation is an individually rounded IEEE double operation in a fixed order (the tree is built with
// -ffp-contract=off), and there are no floating-point atomics: the bits of both outputs depend on the render build alone.
//   k_tan_triangles a lane per triangle: Tr and Br of the contract, negated where det < 0 (angle mode: divided by their lengths),
//                   into the working buffer (48 B per triangle) with one word that says degenerate / det > 0 / det < 0; per
//                   wavefront one integer atomic for the uv-degenerate triangles
//   k_tan_count     one counter per output vertex: its slots (integer atomics)
//   k_scan_*        exclusive scan of the counters (scan.hip: launch_excl_scan)
//   k_tan_scatter   slots into their vertex's segment, in any order (the counters count down as cursors)
//   k_tan_vertices  a lane per output vertex: sorts its segment by slot (insertion sort: a handful of entries), adds both sums in
//                   that order, notes the signs of det it met, projects, writes the rows; per wavefront one integer atomic per
//                   class of vertex.  Segments of more than kTanSegMax slots are listed for k_tan_hubs
//   k_tan_hubs      a workgroup per listed vertex: bitonic sort of the segment where it lies (seg_sort.hpp), every thread sums one
//                   contiguous range of it in order and thread 0 adds the 256 partial sums in thread order -- the association of
//                   normals.hip, which the segment's length alone determines -- and finishes the vertex.  The list has a slot for
//                   every vertex that can qualify (3 T / (kTanSegMax + 1)): it cannot overflow
// Streaming work with L2-resident gathers; bytes per triangle of a closed mesh (U = T / 2): triangles 12 indices + 36 positions +
// 24 uv gathered, 48 + 4 out; count 12 + 12; scan 6; scatter 12 + 12 + 12 + 12; vertices 2 offsets + 12 + 12 (sort) + 156 terms and
// signs gathered + 6 normal + 8 out (+ 6 bitangents): about 400.  Angle mode gathers 36 of indices and 108 of positions more.
#include <hip/hip_runtime.h>

#include "dev_types.hpp"
#include "kernels.hpp"
#include "seg_sort.hpp"

namespace hry {
namespace dev {

namespace {

constexpr uint32_t kTanSegMax = 32;
enum : uint32_t { kTanDegenerate = 0, kTanPositive = 1, kTanNegative = 2 };   // a triangle's word; a vertex's signs: their union

struct D3 { double x, y, z; };

__device__ __forceinline__ D3 position(const TanView &v, uint32_t u)
{
	if (u >= v.nout) { const double q = __builtin_nan(""); return D3{ q, q, q }; }   // (no render build writes such an index)
	const float *p = v.pos + (size_t)u * v.pos_stride;
	return D3{ (double)p[0], (double)p[1], (double)p[2] };
}
__device__ __forceinline__ D3 sub(const D3 &a, const D3 &b) { return D3{ a.x - b.x, a.y - b.y, a.z - b.z }; }
__device__ __forceinline__ D3 cross(const D3 &a, const D3 &b) { return D3{ a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
__device__ __forceinline__ double dot(const D3 &a, const D3 &b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ double length(const D3 &a) { return sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
__device__ __forceinline__ bool usable(double len) { return len > 0.0 && len < __builtin_inf(); }   // (false for NaN)
__device__ __forceinline__ bool finite3(const D3 &a) { return fabs(a.x) < __builtin_inf() && fabs(a.y) < __builtin_inf() && fabs(a.z) < __builtin_inf(); }

// the running sums of one vertex, or of one range of a hub's segment
struct Sums { D3 T, B; uint32_t signs, terms; };

// what slot s adds (tb: the working buffer's rows, sign: the triangles' words)
__device__ __forceinline__ void add_slot(const TanView &v, const double *tb, const uint32_t *sign, uint32_t s, Sums &a)
{
	if (s >= v.n) return;
	const uint32_t t = s / 3, k = s - 3 * t, g = sign[t];
	if (g == kTanDegenerate) return;   // a uv-degenerate triangle contributes nothing
	const double *w = tb + (size_t)t * 6;
	a.signs |= g; ++a.terms;
	if (!v.angle) { a.T.x += w[0]; a.T.y += w[1]; a.T.z += w[2]; a.B.x += w[3]; a.B.y += w[4]; a.B.z += w[5]; return; }
	const D3 p = position(v, v.indices[s]);
	const D3 e = sub(position(v, v.indices[3 * t + (k + 1) % 3]), p), f = sub(position(v, v.indices[3 * t + (k + 2) % 3]), p);
	const double theta = atan2(length(cross(e, f)), dot(e, f));
	a.T.x += theta * w[0]; a.T.y += theta * w[1]; a.T.z += theta * w[2];
	a.B.x += theta * w[3]; a.B.y += theta * w[4]; a.B.z += theta * w[5];
}

// the rows of output vertex u from its sums; the classes it falls into: 1 framed, 2 mirrored, 4 mixed
__device__ __forceinline__ uint32_t finish_vertex(const TanView &v, uint32_t u, const Sums &a)
{
	const float *nf = v.nrm + (size_t)u * v.nrm_stride;
	const D3 n0{ (double)nf[0], (double)nf[1], (double)nf[2] };
	const double nl = length(n0);
	const D3 n{ n0.x / nl, n0.y / nl, n0.z / nl };
	const double d = dot(n, a.T);
	const D3 R{ a.T.x - n.x * d, a.T.y - n.y * d, a.T.z - n.z * d };
	const double rl = length(R);
	const bool ok = a.terms != 0 && usable(nl) && usable(rl);
	const D3 t{ R.x / rl, R.y / rl, R.z / rl };
	const D3 c = cross(n, t);
	const double w = dot(c, a.B) < 0.0 ? -1.0 : 1.0;
	float *o = v.tangents + (size_t)u * 4;
	o[0] = ok ? (float)t.x : 0.0f; o[1] = ok ? (float)t.y : 0.0f; o[2] = ok ? (float)t.z : 0.0f; o[3] = ok ? (float)w : 0.0f;
	if (v.bitangents) {
		float *b = v.bitangents + (size_t)u * 3;
		b[0] = ok ? (float)(w * c.x) : 0.0f; b[1] = ok ? (float)(w * c.y) : 0.0f; b[2] = ok ? (float)(w * c.z) : 0.0f;
	}
	return (ok ? 1u : 0u) | (ok && w < 0.0 ? 2u : 0u) | (a.signs == (kTanPositive | kTanNegative) ? 4u : 0u);
}

}   // namespace

// classes: framed, mirrored, mixed vertices, uv-degenerate triangles
__global__ __launch_bounds__(256) void k_tan_triangles(TanView v, double *tb, uint32_t *sign, uint32_t *classes)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	const bool live = t < v.n / 3;
	uint32_t g = kTanDegenerate;
	if (live) {
		const uint32_t i0 = v.indices[3 * t], i1 = v.indices[3 * t + 1], i2 = v.indices[3 * t + 2];
		D3 Tr{ 0.0, 0.0, 0.0 }, Br{ 0.0, 0.0, 0.0 };
		if (i0 < v.nout && i1 < v.nout && i2 < v.nout) {
			const D3 p0 = position(v, i0), e1 = sub(position(v, i1), p0), e2 = sub(position(v, i2), p0);
			const float *q0 = v.uv + (size_t)i0 * v.uv_stride, *q1 = v.uv + (size_t)i1 * v.uv_stride, *q2 = v.uv + (size_t)i2 * v.uv_stride;
			const double a1 = (double)q1[0] - (double)q0[0], b1 = (double)q1[1] - (double)q0[1];
			const double a2 = (double)q2[0] - (double)q0[0], b2 = (double)q2[1] - (double)q0[1];
			const double det = a1 * b2 - a2 * b1;
			Tr = D3{ e1.x * b2 - e2.x * b1, e1.y * b2 - e2.y * b1, e1.z * b2 - e2.z * b1 };
			Br = D3{ e2.x * a1 - e1.x * a2, e2.y * a1 - e1.y * a2, e2.z * a1 - e1.z * a2 };
			if (det < 0.0) { Tr = D3{ -Tr.x, -Tr.y, -Tr.z }; Br = D3{ -Br.x, -Br.y, -Br.z }; }
			bool ok = det != 0.0 && fabs(det) < __builtin_inf() && finite3(Tr) && finite3(Br);   // (false for a NaN det)
			if (ok && v.angle) {
				const double lt = length(Tr), lb = length(Br);
				ok = lt != 0.0 && lb != 0.0;
				if (ok) { Tr = D3{ Tr.x / lt, Tr.y / lt, Tr.z / lt }; Br = D3{ Br.x / lb, Br.y / lb, Br.z / lb }; }
			}
			if (ok) g = det < 0.0 ? kTanNegative : kTanPositive;
		}
		if (g == kTanDegenerate) { Tr = D3{ 0.0, 0.0, 0.0 }; Br = Tr; }
		double *w = tb + (size_t)t * 6;
		w[0] = Tr.x; w[1] = Tr.y; w[2] = Tr.z; w[3] = Br.x; w[4] = Br.y; w[5] = Br.z;
		sign[t] = g;
	}
	const uint64_t degenerate = __ballot(live && g == kTanDegenerate);   // (every lane takes part)
	if ((threadIdx.x & 63) == 0 && degenerate) atomicAdd(&classes[3], (uint32_t)__popcll(degenerate));
}

__global__ __launch_bounds__(256) void k_tan_count(const uint32_t *indices, uint32_t n, uint32_t nout, uint32_t *count)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= n) return;
	const uint32_t u = indices[s];
	if (u < nout) atomicAdd(&count[u], 1u);
}

// (count[u] holds u's slots on entry and counts down: the last free place of the segment is taken first)
__global__ __launch_bounds__(256) void k_tan_scatter(const uint32_t *indices, uint32_t n, uint32_t nout, const uint32_t *start, uint32_t *count, uint32_t *seg)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= n) return;
	const uint32_t u = indices[s];
	if (u >= nout) return;
	const uint32_t k = atomicSub(&count[u], 1u);
	const uint64_t pos = (uint64_t)start[u] + k - 1;
	if (k && pos < n) seg[pos] = s;
}

__global__ __launch_bounds__(256) void k_tan_vertices(TanView v, const uint32_t *start, uint32_t *seg, const double *tb, const uint32_t *sign, uint32_t *hubs,
                                                      uint32_t hub_cap, uint32_t *classes)
{
	const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t cls = 0;
	if (u < v.nout) {
		const uint32_t b = start[u], e = start[u + 1];
		const uint32_t len = e >= b && e <= v.n ? e - b : 0;
		if (len > kTanSegMax) {
			const uint32_t k = atomicAdd(&hubs[0], 1u);
			if (k < hub_cap) hubs[1 + k] = u;   // (hub_cap: every vertex that can have so many slots; k_tan_hubs counts its classes)
		} else {
			uint32_t *a = seg + b;
			for (uint32_t i = 1; i < len; ++i) {   // insertion sort by slot
				const uint32_t x = a[i];
				uint32_t j = i;
				while (j > 0 && a[j - 1] > x) { a[j] = a[j - 1]; --j; }
				a[j] = x;
			}
			Sums s{ D3{ 0.0, 0.0, 0.0 }, D3{ 0.0, 0.0, 0.0 }, 0, 0 };
			for (uint32_t i = 0; i < len; ++i) add_slot(v, tb, sign, a[i], s);
			cls = finish_vertex(v, u, s);
		}
	}
	// the classes, a wavefront at a time (every lane takes part)
	const uint64_t framed = __ballot(cls & 1), mirrored = __ballot(cls & 2), mixed = __ballot(cls & 4);
	if ((threadIdx.x & 63) == 0) {
		if (framed) atomicAdd(&classes[0], (uint32_t)__popcll(framed));
		if (mirrored) atomicAdd(&classes[1], (uint32_t)__popcll(mirrored));
		if (mixed) atomicAdd(&classes[2], (uint32_t)__popcll(mixed));
	}
}

__global__ __launch_bounds__(256) void k_tan_hubs(TanView v, const uint32_t *start, uint32_t *seg, const double *tb, const uint32_t *sign, const uint32_t *hubs,
                                                  uint32_t hub_cap, uint32_t *classes)
{
	__shared__ double part[6 * 256];
	__shared__ uint32_t met[2 * 256];
	const uint32_t listed = min(hubs[0], hub_cap), tid = threadIdx.x;
	for (uint32_t h = blockIdx.x; h < listed; h += gridDim.x) {
		const uint32_t u = hubs[1 + h];
		if (u >= v.nout) continue;
		const uint32_t b = start[u], e = start[u + 1];
		if (e < b || e > v.n) continue;
		const uint64_t len = e - b;
		uint32_t *a = seg + b;
		block_sort_segment(a, len, tid);
		const uint64_t chunk = (len + 255) / 256, lo = min(len, tid * chunk), hi = min(len, lo + chunk);
		Sums s{ D3{ 0.0, 0.0, 0.0 }, D3{ 0.0, 0.0, 0.0 }, 0, 0 };
		for (uint64_t i = lo; i < hi; ++i) add_slot(v, tb, sign, a[i], s);
		double *p = part + 6 * tid;
		p[0] = s.T.x; p[1] = s.T.y; p[2] = s.T.z; p[3] = s.B.x; p[4] = s.B.y; p[5] = s.B.z;
		met[2 * tid] = s.signs; met[2 * tid + 1] = s.terms;
		__syncthreads();
		if (tid == 0) {
			for (uint32_t t = 1; t < 256; ++t) {
				const double *q = part + 6 * t;
				s.T.x += q[0]; s.T.y += q[1]; s.T.z += q[2]; s.B.x += q[3]; s.B.y += q[4]; s.B.z += q[5];
				s.signs |= met[2 * t]; s.terms += met[2 * t + 1];
			}
			const uint32_t cls = finish_vertex(v, u, s);
			if (cls & 1) atomicAdd(&classes[0], 1u);
			if (cls & 2) atomicAdd(&classes[1], 1u);
			if (cls & 4) atomicAdd(&classes[2], 1u);
		}
		__syncthreads();
	}
}

// ---- launchers
uint32_t tangents_hub_capacity(uint32_t nslots) { return nslots / (kTanSegMax + 1) + 1; }

void launch_tangents(hipStream_t st, const TanView &v, const TanWork &w)
{
	const uint32_t cap = tangents_hub_capacity(v.n);
	if (v.n) {
		hipLaunchKernelGGL(k_tan_triangles, dim3(blocks_for(v.n / 3, 256)), dim3(256), 0, st, v, w.terms, w.sign, w.classes);
		if (v.nout) hipLaunchKernelGGL(k_tan_count, dim3(blocks_for(v.n, 256)), dim3(256), 0, st, v.indices, v.n, v.nout, w.count);
	}
	if (!v.nout) return;
	launch_excl_scan(st, w.count, v.nout, w.sums, w.start);
	if (v.n) hipLaunchKernelGGL(k_tan_scatter, dim3(blocks_for(v.n, 256)), dim3(256), 0, st, v.indices, v.n, v.nout, (const uint32_t*)w.start, w.count, w.seg);
	hipLaunchKernelGGL(k_tan_vertices, dim3(blocks_for(v.nout, 256)), dim3(256), 0, st, v, (const uint32_t*)w.start, w.seg, (const double*)w.terms, (const uint32_t*)w.sign,
	                   w.hubs, cap, w.classes);
	hipLaunchKernelGGL(k_tan_hubs, dim3(std::min<uint32_t>(cap, 1024)), dim3(256), 0, st, v, (const uint32_t*)w.start, w.seg, (const double*)w.terms, (const uint32_t*)w.sign,
	                   (const uint32_t*)w.hubs, cap, w.classes);
}

}   // namespace dev
}   // namespace hry
