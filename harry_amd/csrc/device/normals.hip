// Face and vertex normals of a render build (driver: render.cpp; contract: include/harry_amd.h, hry_render_build_ex).
// The build has org and the face offsets but no twins, so a vertex finds its corners the way twins.hip does: count, scan, scatter,
// order per vertex.  Every floating-point operation is an individually rounded IEEE double operation in a fixed order (the tree is
// built with -ffp-contract=off), and there are no floating-point atomics: the bits of both outputs depend on the mesh alone.
//   k_nrm_faces     a lane per face: N_f = sum of the fan triangles' cross products relative to corner 0, in double, into the working
//                   buffer (24 B per face: N_f in area mode, N_f / |N_f| in angle mode, zeros for a face that contributes nothing)
//                   and, where asked for, the unit normal as floats
//   k_nrm_count     one counter per vertex: its corners (integer atomics)
//   k_scan_*        exclusive scan of the counters (scan.hip: launch_excl_scan)
//   k_nrm_scatter   corners into their vertex's segment, in any order
//   k_nrm_vertices  a lane per vertex: sorts its segment by corner id (insertion sort: a handful of entries), sums the corners'
//                   contributions in that order, normalises.  Segments of more than kNrmSegMax corners are listed for k_nrm_hubs
//   k_nrm_hubs      a workgroup per listed vertex: bitonic sort of the segment where it lies, then every thread sums one contiguous
//                   range of it in order and thread 0 adds the 256 partial sums in thread order -- an association that the
//                   segment's length alone determines.  The list has a slot for every vertex that can qualify (ne / (kNrmSegMax + 1)):
//                   it cannot overflow
//   k_nrm_expand    unwelded meshes: normals[u] = the normal of vertex_source[u]
// Streaming work with L2-resident gathers; bytes per triangle of an all-triangle mesh (nv = T / 2): faces 12 org + 36 positions +
// 24 N_f (+ 12 face_normals), count 12, scan 6, scatter 12 + 12 + 12, vertices 12 + 12 (sort) + 72 N_f + 6 out: about 230.
#include <hip/hip_runtime.h>

#include "dev_types.hpp"
#include "kernels.hpp"
#include "seg_sort.hpp"

namespace hry {
namespace dev {

namespace {

struct D3 { double x, y, z; };

__device__ __forceinline__ D3 position(const NrmView &n, uint32_t v)
{
	if (v >= n.nv) { const double q = __builtin_nan(""); return D3{ q, q, q }; }   // (no reader builds such a corner: its face drops out)
	const float *p = n.pos + (size_t)v * n.pos_stride;
	return D3{ (double)p[0], (double)p[1], (double)p[2] };
}
__device__ __forceinline__ D3 sub(const D3 &a, const D3 &b) { return D3{ a.x - b.x, a.y - b.y, a.z - b.z }; }
__device__ __forceinline__ D3 cross(const D3 &a, const D3 &b) { return D3{ a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
__device__ __forceinline__ double length(const D3 &a) { return sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
__device__ __forceinline__ bool usable(double len) { return len > 0.0 && len < __builtin_inf(); }   // (false for NaN)

// the corners [lo, hi) of face f, false when the tables do not hold them
__device__ __forceinline__ bool face_span(const NrmView &n, uint32_t f, uint32_t &lo, uint32_t &hi)
{
	if (f >= n.nf) return false;
	if (n.eface) { lo = n.foff[f]; hi = n.foff[f + 1]; }
	else { if (f > 0x55555554u) return false; lo = 3 * f; hi = lo + 3; }   // every face a triangle: no table
	return hi >= lo + 3 && hi <= n.ne;
}

// what corner c of vertex v adds to S_v (w: the working buffer's row of c's face)
__device__ __forceinline__ void add_corner(const NrmView &n, const double *fn, uint32_t v, uint32_t c, D3 &s)
{
	if (c >= n.ne) return;
	const uint32_t f = n.eface ? n.eface[c] : c / 3;
	if (f >= n.nf) return;
	const D3 w{ fn[(size_t)f * 3], fn[(size_t)f * 3 + 1], fn[(size_t)f * 3 + 2] };
	if (w.x == 0.0 && w.y == 0.0 && w.z == 0.0) return;   // a face without a normal contributes nothing
	if (!n.angle) { s.x += w.x; s.y += w.y; s.z += w.z; return; }
	uint32_t lo, hi;
	if (!face_span(n, f, lo, hi)) return;
	const uint32_t nx = c + 1 == hi ? lo : c + 1, pv = c == lo ? hi - 1 : c - 1;
	const D3 p = position(n, v), a = sub(position(n, n.org[nx]), p), b = sub(position(n, n.org[pv]), p);
	const double theta = atan2(length(cross(a, b)), a.x * b.x + a.y * b.y + a.z * b.z);
	s.x += theta * w.x; s.y += theta * w.y; s.z += theta * w.z;
}

__device__ __forceinline__ void write_unit(const D3 &s, float *out)
{
	const double len = length(s);
	const bool ok = usable(len);
	out[0] = ok ? (float)(s.x / len) : 0.0f;
	out[1] = ok ? (float)(s.y / len) : 0.0f;
	out[2] = ok ? (float)(s.z / len) : 0.0f;
}

}   // namespace

__global__ __launch_bounds__(256) void k_nrm_faces(NrmView n, double *fn, float *face_normals)
{
	const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
	if (f >= n.nf) return;
	uint32_t lo, hi;
	D3 s{ 0.0, 0.0, 0.0 };
	double len = 0.0;
	if (face_span(n, f, lo, hi)) {
		const D3 p0 = position(n, n.org[lo]);
		D3 a = sub(position(n, n.org[lo + 1]), p0), b = sub(position(n, n.org[lo + 2]), p0);
		s = cross(a, b);
		for (uint32_t k = lo + 3; k < hi; ++k) {   // polygons: the further fan triangles, in order
			a = b; b = sub(position(n, n.org[k]), p0);
			const D3 t = cross(a, b);
			s.x += t.x; s.y += t.y; s.z += t.z;
		}
		len = length(s);
	}
	const bool ok = usable(len);
	const D3 u = ok ? D3{ s.x / len, s.y / len, s.z / len } : D3{ 0.0, 0.0, 0.0 };
	const D3 w = !ok ? u : n.angle ? u : s;
	fn[(size_t)f * 3] = w.x; fn[(size_t)f * 3 + 1] = w.y; fn[(size_t)f * 3 + 2] = w.z;
	if (face_normals) { face_normals[(size_t)f * 3] = (float)u.x; face_normals[(size_t)f * 3 + 1] = (float)u.y; face_normals[(size_t)f * 3 + 2] = (float)u.z; }
}

__global__ __launch_bounds__(256) void k_nrm_count(const uint32_t *org, uint32_t ne, uint32_t nv, uint32_t *count)
{
	const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= ne) return;
	const uint32_t v = org[c];
	if (v < nv) atomicAdd(&count[v], 1u);
}

__global__ __launch_bounds__(256) void k_nrm_scatter(const uint32_t *org, uint32_t ne, uint32_t nv, const uint32_t *start, uint32_t *fill, uint32_t *seg)
{
	const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= ne) return;
	const uint32_t v = org[c];
	if (v >= nv) return;
	const uint32_t pos = start[v] + atomicAdd(&fill[v], 1u);
	if (pos < ne) seg[pos] = c;
}

constexpr uint32_t kNrmSegMax = 32;

__global__ __launch_bounds__(256) void k_nrm_vertices(NrmView n, const uint32_t *start, uint32_t *seg, const double *fn, uint32_t *hubs, uint32_t hub_cap, float *out)
{
	const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
	if (v >= n.nv) return;
	const uint32_t b = start[v], e = start[v + 1];
	if (e < b || e > n.ne) return;
	if (e - b > kNrmSegMax) {
		const uint32_t k = atomicAdd(&hubs[0], 1u);
		if (k < hub_cap) hubs[1 + k] = v;   // (hub_cap: every vertex that can have so many corners)
		return;
	}
	for (uint32_t i = b + 1; i < e; ++i) {   // insertion sort by corner id
		const uint32_t x = seg[i];
		uint32_t j = i;
		while (j > b && seg[j - 1] > x) { seg[j] = seg[j - 1]; --j; }
		seg[j] = x;
	}
	D3 s{ 0.0, 0.0, 0.0 };
	for (uint32_t i = b; i < e; ++i) add_corner(n, fn, v, seg[i], s);
	write_unit(s, out + (size_t)v * 3);
}

__global__ __launch_bounds__(256) void k_nrm_hubs(NrmView n, const uint32_t *start, uint32_t *seg, const double *fn, const uint32_t *hubs, uint32_t hub_cap, float *out)
{
	__shared__ double part[3 * 256];
	const uint32_t listed = min(hubs[0], hub_cap), tid = threadIdx.x;
	for (uint32_t h = blockIdx.x; h < listed; h += gridDim.x) {
		const uint32_t v = hubs[1 + h];
		if (v >= n.nv) continue;
		const uint32_t b = start[v], e = start[v + 1];
		if (e < b || e > n.ne) continue;
		const uint64_t len = e - b;
		uint32_t *a = seg + b;
		block_sort_segment(a, len, tid);
		const uint64_t chunk = (len + 255) / 256, lo = min(len, tid * chunk), hi = min(len, lo + chunk);
		D3 s{ 0.0, 0.0, 0.0 };
		for (uint64_t i = lo; i < hi; ++i) add_corner(n, fn, v, a[i], s);
		part[3 * tid] = s.x; part[3 * tid + 1] = s.y; part[3 * tid + 2] = s.z;
		__syncthreads();
		if (tid == 0) {
			for (uint32_t t = 1; t < 256; ++t) { s.x += part[3 * t]; s.y += part[3 * t + 1]; s.z += part[3 * t + 2]; }
			write_unit(s, out + (size_t)v * 3);
		}
		__syncthreads();
	}
}

__global__ __launch_bounds__(256) void k_nrm_expand(const float *vn, const uint32_t *vsrc, uint64_t words, uint32_t nv, float *out)
{
	const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += step) {
		const uint64_t u = w / 3;
		const uint32_t v = vsrc[u];
		out[w] = v < nv ? vn[(size_t)v * 3 + (uint32_t)(w - u * 3)] : 0.0f;
	}
}

// ---- launchers
uint32_t normals_hub_capacity(uint32_t ne) { return ne / (kNrmSegMax + 1) + 1; }

void launch_face_normals(hipStream_t st, const NrmView &n, double *fn, float *face_normals)
{
	if (n.nf) hipLaunchKernelGGL(k_nrm_faces, dim3(blocks_for(n.nf, 256)), dim3(256), 0, st, n, fn, face_normals);
}

void launch_vertex_normals(hipStream_t st, const NrmView &n, const double *fn, uint32_t *count, uint32_t *fill, uint32_t *start, uint32_t *sums, uint32_t *seg,
                           uint32_t *hubs, float *out)
{
	if (!n.nv) return;
	const uint32_t cap = normals_hub_capacity(n.ne);
	if (n.ne) hipLaunchKernelGGL(k_nrm_count, dim3(blocks_for(n.ne, 256)), dim3(256), 0, st, n.org, n.ne, n.nv, count);
	launch_excl_scan(st, count, n.nv, sums, start);
	if (n.ne) hipLaunchKernelGGL(k_nrm_scatter, dim3(blocks_for(n.ne, 256)), dim3(256), 0, st, n.org, n.ne, n.nv, (const uint32_t*)start, fill, seg);
	hipLaunchKernelGGL(k_nrm_vertices, dim3(blocks_for(n.nv, 256)), dim3(256), 0, st, n, (const uint32_t*)start, seg, fn, hubs, cap, out);
	hipLaunchKernelGGL(k_nrm_hubs, dim3(std::min<uint32_t>(cap, 1024)), dim3(256), 0, st, n, (const uint32_t*)start, seg, fn, (const uint32_t*)hubs, cap, out);
}

void launch_normals_expand(hipStream_t st, const float *vn, const uint32_t *vsrc, uint32_t nout, uint32_t nv, float *out)
{
	const uint64_t words = 3ull * nout;
	if (words) hipLaunchKernelGGL(k_nrm_expand, dim3(std::min<uint64_t>(blocks_for(words, 256), 1u << 20)), dim3(256), 0, st, vn, vsrc, words, nv, out);
}

}   // namespace dev
}   // namespace hry
