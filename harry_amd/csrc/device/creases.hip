// Hard edges and split normals of a render build (driver: creases.cpp; contract: include/harry_amd.h, hry_creases_build; DESIGN.md
// 7a, "Creases").  The items are the 3 T index slots of the triangles.  A smooth edge unites, at each of its two decoded end
// vertices, the slots of its two sides there (union_find.hpp: the root of a set is its smallest member, whatever order the atomics
// complete in); a set is a smooth group, the fan one normal is summed over.  dedup.hip's first-occurrence numbering (CreaseKey) gives
// every slot its split vertex between the two halves.  Behind it, the pattern of normals.hip and tangents.hip with the groups as
// segments: count, scan, scatter, order per segment.  Every floating-point operation is an individually rounded IEEE double
// operation in a fixed order (the tree is built with -ffp-contract=off), and there are no floating-point atomics: the bits of every
// buffer depend on the render build, its edges build, the limit and the flags alone.
//   k_crs_classify  a lane per edge: its class from its segment of edge_sides, the decoded ends of its sides, tri_face and edge_cos,
//                   into the working buffer; a SMOOTH edge unites twice; per wavefront one integer atomic per class counter
//   k_crs_roots     a lane per slot: its root and whether it is one
//   k_scan_*        exclusive scan of the root flags: the groups' numbers by ascending smallest slot (scan.hip: launch_excl_scan)
//   k_dedup_*       the split vertices (dedup.hip), from creases.cpp; W and G come down before the outputs are allocated
//   k_crs_labels    a lane per slot and edge: slot_group, edge_class; a root counts its group at its decoded vertex, and the one
//                   that finds exactly one group there before it makes the vertex a split one; one counter per group: its slots
//   k_crs_terms     a lane per triangle: N_t, or N_t / |N_t| with corner-angle weights, zeros where |N_t| is 0 or not finite (24 B)
//   k_crs_scatter   slots into their group's segment, in any order (the counters count down as cursors)
//   k_crs_groups    a lane per group: sorts its segment by slot (insertion sort: a handful of entries), adds the terms in that
//                   order, normalises into the working buffer.  Segments of more than kCreaseSegMax slots are listed for k_crs_hubs
//   k_crs_hubs      a workgroup per listed group: bitonic sort of the segment where it lies (seg_sort.hpp), every thread sums one
//                   contiguous range of it in order and thread 0 adds the 256 partial sums in thread order -- the association of
//                   normals.hip, which the segment's length alone determines.  The list has a slot for every group that can qualify
//                   (3 T / (kCreaseSegMax + 1)): it cannot overflow
//   k_crs_expand    a lane per split vertex: vertex_source, and the normal of the group of its first slot
// Random access with L2-resident gathers; bytes per triangle of a closed manifold triangle mesh (E = 3 T / 2, G = T / 2 groups when
// all is smooth): DESIGN.md "Creases" counts them.
#include <hip/hip_runtime.h>

#include "dev_types.hpp"
#include "kernels.hpp"
#include "seg_sort.hpp"
#include "union_find.hpp"

namespace hry {
namespace dev {

namespace {

constexpr uint32_t kCreaseSegMax = 32;
enum : uint32_t { kSmooth = 0, kSharp = 1, kBoundary = 2, kNonmanifold = 3, kMisoriented = 4, kDegenerate = 5 };   // HRY_CREASE_*

struct D3 { double x, y, z; };

__device__ __forceinline__ D3 position(const CreaseView &v, uint32_t u)
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

// what slot s adds to the sum of its group (tn: the working buffer's rows)
__device__ __forceinline__ void add_slot(const CreaseView &v, const double *tn, uint32_t s, D3 &a)
{
	if (s >= v.n) return;
	const uint32_t t = s / 3, k = s - 3 * t;
	const D3 w{ tn[(size_t)t * 3], tn[(size_t)t * 3 + 1], tn[(size_t)t * 3 + 2] };
	if (w.x == 0.0 && w.y == 0.0 && w.z == 0.0) return;   // a triangle without a normal contributes nothing
	if (!v.angle) { a.x += w.x; a.y += w.y; a.z += w.z; return; }
	const D3 p = position(v, v.indices[s]);
	const D3 e = sub(position(v, v.indices[3 * t + (k + 1) % 3]), p), f = sub(position(v, v.indices[3 * t + (k + 2) % 3]), p);
	const double theta = atan2(length(cross(e, f)), dot(e, f));
	a.x += theta * w.x; a.y += theta * w.y; a.z += theta * w.z;
}

__device__ __forceinline__ void write_unit(const D3 &s, float *out)
{
	const double len = length(s);
	const bool ok = usable(len);
	out[0] = ok ? (float)(s.x / len) : 0.0f;
	out[1] = ok ? (float)(s.y / len) : 0.0f;
	out[2] = ok ? (float)(s.z / len) : 0.0f;
}

// the slot of side s at decoded vertex x: s itself where it starts there, else the slot of its other end
__device__ __forceinline__ uint32_t slot_at(const CreaseView &v, uint32_t s, uint32_t x) { return vertex_of(v, v.indices[s]) == x ? s : next_corner(s); }

}   // namespace

// classes: SMOOTH, SHARP, other edges
__global__ __launch_bounds__(256) void k_crs_classify(CreaseView v, uint32_t *par, uint32_t *eclass, uint32_t *classes)
{
	const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t cls = kNoElement, b = 0, end = 0;
	if (e < v.ne && side_segment(v, e, b, end) && end > b) {
		const uint32_t len = end - b, p = v.sides[b], q = len > 1 ? v.sides[b + 1] : 0;
		if (len == 1) cls = kBoundary;
		else if (len > 2) cls = kNonmanifold;
		else if (p >= v.n || q >= v.n) cls = kDegenerate;   // (no edges build writes such a side)
		else {
			const uint32_t a0 = vertex_of(v, v.indices[p]), a1 = vertex_of(v, v.indices[next_corner(p)]);
			if (a0 == a1) cls = kDegenerate;
			else if (same_direction(v, p, q)) cls = kMisoriented;
			else if (v.tri_face[p / 3] == v.tri_face[q / 3]) cls = kSmooth;   // a fan diagonal of a polygon
			else {
				const float c = v.edge_cos[e];
				cls = c == 2.0f ? kDegenerate : (double)c >= v.cos_limit ? kSmooth : kSharp;
			}
			if (cls == kSmooth) {
				uf_unite(par, slot_at(v, p, a0), slot_at(v, q, a0));
				uf_unite(par, slot_at(v, p, a1), slot_at(v, q, a1));
			}
		}
	}
	if (e < v.ne) eclass[e] = cls == kNoElement ? kDegenerate : cls;   // (an edge without sides: no edges build has one)
	const uint64_t smooth = __ballot(cls == kSmooth), sharp = __ballot(cls == kSharp), other = __ballot(e < v.ne && cls != kSmooth && cls != kSharp);
	if ((threadIdx.x & 63) == 0) {
		if (smooth) atomicAdd(&classes[0], (uint32_t)__popcll(smooth));
		if (sharp) atomicAdd(&classes[1], (uint32_t)__popcll(sharp));
		if (other) atomicAdd(&classes[2], (uint32_t)__popcll(other));
	}
}

__global__ __launch_bounds__(256) void k_crs_roots(uint32_t *par, uint32_t n, uint32_t *root, uint32_t *flag)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= n) return;
	const uint32_t r = uf_find(par, s);
	root[s] = r;
	flag[s] = r == s ? 1u : 0u;
}

// slot_group and edge_class; the groups per decoded vertex, the slots per group.  classes[3]: decoded vertices with more than one group
__global__ __launch_bounds__(256) void k_crs_labels(CreaseView v, const uint32_t *root, const uint32_t *num, const uint32_t *eclass, uint32_t *vgroups, uint32_t *count,
                                                    uint32_t *classes)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < v.ne) v.edge_class[i] = eclass[i];
	bool second = false;
	if (i < v.n) {
		const uint32_t r = root[i], g = r < v.n ? num[r] : kNoElement;
		v.slot_group[i] = g;
		if (g < v.ng) atomicAdd(&count[g], 1u);
		if (r == i) {
			const uint32_t x = vertex_of(v, v.indices[i]);
			if (x < v.nv) second = atomicAdd(&vgroups[x], 1u) == 1;   // exactly one root per such vertex finds one group before it
		}
	}
	const uint64_t split = __ballot(second);   // (every lane takes part)
	if ((threadIdx.x & 63) == 0 && split) atomicAdd(&classes[3], (uint32_t)__popcll(split));
}

__global__ __launch_bounds__(256) void k_crs_terms(CreaseView v, double *tn)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= v.ntri) return;
	const D3 p0 = position(v, v.indices[3 * t]);
	const D3 N = cross(sub(position(v, v.indices[3 * t + 1]), p0), sub(position(v, v.indices[3 * t + 2]), p0));
	const double len = length(N);
	const bool ok = usable(len);
	const D3 w = !ok ? D3{ 0.0, 0.0, 0.0 } : v.angle ? D3{ N.x / len, N.y / len, N.z / len } : N;
	tn[(size_t)t * 3] = w.x; tn[(size_t)t * 3 + 1] = w.y; tn[(size_t)t * 3 + 2] = w.z;
}

// (count[g] holds g's slots on entry and counts down: the last free place of the segment is taken first)
__global__ __launch_bounds__(256) void k_crs_scatter(const uint32_t *slot_group, uint32_t n, uint32_t ng, const uint32_t *start, uint32_t *count, uint32_t *seg)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= n) return;
	const uint32_t g = slot_group[s];
	if (g >= ng) return;
	const uint32_t k = atomicSub(&count[g], 1u);
	const uint64_t pos = (uint64_t)start[g] + k - 1;
	if (k && pos < n) seg[pos] = s;
}

__global__ __launch_bounds__(256) void k_crs_groups(CreaseView v, const uint32_t *start, uint32_t *seg, const double *tn, uint32_t *hubs, uint32_t hub_cap, float *gnormal)
{
	const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= v.ng) return;
	const uint32_t b = start[g], e = start[g + 1];
	const uint32_t len = e >= b && e <= v.n ? e - b : 0;
	if (len > kCreaseSegMax) {
		const uint32_t k = atomicAdd(&hubs[0], 1u);
		if (k < hub_cap) hubs[1 + k] = g;   // (hub_cap: every group that can have so many slots)
		return;
	}
	uint32_t *a = seg + b;
	for (uint32_t i = 1; i < len; ++i) {   // insertion sort by slot
		const uint32_t x = a[i];
		uint32_t j = i;
		while (j > 0 && a[j - 1] > x) { a[j] = a[j - 1]; --j; }
		a[j] = x;
	}
	D3 s{ 0.0, 0.0, 0.0 };
	for (uint32_t i = 0; i < len; ++i) add_slot(v, tn, a[i], s);
	write_unit(s, gnormal + (size_t)g * 3);
}

__global__ __launch_bounds__(256) void k_crs_hubs(CreaseView v, const uint32_t *start, uint32_t *seg, const double *tn, const uint32_t *hubs, uint32_t hub_cap, float *gnormal)
{
	__shared__ double part[3 * 256];
	const uint32_t listed = min(hubs[0], hub_cap), tid = threadIdx.x;
	for (uint32_t h = blockIdx.x; h < listed; h += gridDim.x) {
		const uint32_t g = hubs[1 + h];
		if (g >= v.ng) continue;
		const uint32_t b = start[g], e = start[g + 1];
		if (e < b || e > v.n) continue;
		const uint64_t len = e - b;
		uint32_t *a = seg + b;
		block_sort_segment(a, len, tid);
		const uint64_t chunk = (len + 255) / 256, lo = min(len, tid * chunk), hi = min(len, lo + chunk);
		D3 s{ 0.0, 0.0, 0.0 };
		for (uint64_t i = lo; i < hi; ++i) add_slot(v, tn, a[i], s);
		part[3 * tid] = s.x; part[3 * tid + 1] = s.y; part[3 * tid + 2] = s.z;
		__syncthreads();
		if (tid == 0) {
			for (uint32_t t = 1; t < 256; ++t) { s.x += part[3 * t]; s.y += part[3 * t + 1]; s.z += part[3 * t + 2]; }
			write_unit(s, gnormal + (size_t)g * 3);
		}
		__syncthreads();
	}
}

__global__ __launch_bounds__(256) void k_crs_expand(CreaseView v, const uint32_t *first_slot, const float *gnormal)
{
	const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
	if (w >= v.nw) return;
	const uint32_t s = first_slot[w], g = s < v.n ? v.slot_group[s] : kNoElement;
	v.vertex_source[w] = vertex_of(v, v.render_vertex[w]);
	float *o = v.normals + (size_t)w * 3;
	const float *gn = gnormal + (size_t)g * 3;
	const bool ok = g < v.ng;
	o[0] = ok ? gn[0] : 0.0f; o[1] = ok ? gn[1] : 0.0f; o[2] = ok ? gn[2] : 0.0f;
}

// ---- launchers
uint32_t creases_hub_capacity(uint32_t nslots) { return nslots / (kCreaseSegMax + 1) + 1; }

void launch_creases_groups(hipStream_t st, const CreaseView &v, const CreaseWork &w)
{
	launch_iota(st, v.n, w.par);
	if (v.ne) hipLaunchKernelGGL(k_crs_classify, dim3(blocks_for(v.ne, 256)), dim3(256), 0, st, v, w.par, w.eclass, w.classes);
	if (v.n) hipLaunchKernelGGL(k_crs_roots, dim3(blocks_for(v.n, 256)), dim3(256), 0, st, w.par, v.n, w.root, w.flag);
	launch_excl_scan(st, w.flag, v.n, w.sums, w.num);
}

void launch_creases_normals(hipStream_t st, const CreaseView &v, const CreaseWork &w)
{
	const uint32_t cap = creases_hub_capacity(v.n), items = std::max(v.n, v.ne);
	if (!items) return;
	hipLaunchKernelGGL(k_crs_labels, dim3(blocks_for(items, 256)), dim3(256), 0, st, v, (const uint32_t*)w.root, (const uint32_t*)w.num, (const uint32_t*)w.eclass, w.vgroups,
	                   w.count, w.classes);
	if (!v.n || !v.ng) return;
	hipLaunchKernelGGL(k_crs_terms, dim3(blocks_for(v.ntri, 256)), dim3(256), 0, st, v, w.terms);
	launch_excl_scan(st, w.count, v.ng, w.sums, w.start);
	hipLaunchKernelGGL(k_crs_scatter, dim3(blocks_for(v.n, 256)), dim3(256), 0, st, (const uint32_t*)v.slot_group, v.n, v.ng, (const uint32_t*)w.start, w.count, w.seg);
	hipLaunchKernelGGL(k_crs_groups, dim3(blocks_for(v.ng, 256)), dim3(256), 0, st, v, (const uint32_t*)w.start, w.seg, (const double*)w.terms, w.hubs, cap, w.gnormal);
	hipLaunchKernelGGL(k_crs_hubs, dim3(std::min<uint32_t>(cap, 1024)), dim3(256), 0, st, v, (const uint32_t*)w.start, w.seg, (const double*)w.terms, (const uint32_t*)w.hubs, cap,
	                   w.gnormal);
	if (v.nw) hipLaunchKernelGGL(k_crs_expand, dim3(blocks_for(v.nw, 256)), dim3(256), 0, st, v, (const uint32_t*)w.first_slot, (const float*)w.gnormal);
}

}   // namespace dev
}   // namespace hry
