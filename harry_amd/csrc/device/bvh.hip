// A linear bounding-volume hierarchy over the triangles of a render build, the closest-hit ray cast and the closest-point query over
// it, and the pairs of its triangles that pass through each other (driver: bvh.cpp; contract: include/harry_amd.h, hry_bvh_build,
// hry_bvh_cast, hry_bvh_nearest and hry_intersections_build; DESIGN.md "Bvh").  Every floating-point operation is an
// individually rounded IEEE double operation in the written order (the tree is built with -ffp-contract=off); the boxes are float
// minima and maxima, which are exact in any order; there are no floating-point atomics.  The bits of every buffer depend on the
// render build alone, those of a cast or a closest-point query on the hierarchy and the rays or points alone.
// The build, first stretch (grids sized by T; the number of leaves L is a device word until the stretch ends):
//   k_bvh_init      the counters and the empty scene box
//   k_bvh_live      a lane per triangle: live (nine finite floats) or dead; the scene box by a wavefront minimum / maximum of ordered
//                   words and one integer atomic per wavefront and bound (minima commute: the order decides nothing)
//   k_scan_*        exclusive scan of the live flags: a live triangle's rank in ascending t, and L (scan.hip: launch_excl_scan)
//   k_bvh_codes     a lane per triangle: the 30-bit code of a live one and its number, at its rank
//   k_radix_*       four stable 8-bit passes by code (radix_sort.hpp): ascending (code, t)
//   k_bvh_tree      a lane per internal node (Karras 2012): its range by two doubling / binary searches over the common prefixes of
//                   the keys code * 2^32 + i, its split by a third, its two children and their parents
//   k_bvh_depth     a lane per leaf: the internal nodes above it (at most 62: every level consumes one of the key's 62 significant
//                   bits), their maximum; and the distinct codes (a ballot per wavefront)
// Second stretch (L, the depth and the distinct codes have come down; the buffers are allocated):
//   k_bvh_emit      a lane per leaf: its triangle, code, three positions and box; a lane per node: its children; the scene box
//   k_bvh_fit       one launch per level, `depth` of them: a node whose children were finished by EARLIER launches takes the minimum
//                   / maximum of their boxes and notes its round.  Nothing is handed over inside a launch: a node that reads the
//                   round its child is writing in the same launch sees HRY_NO_ELEMENT or this round, and waits either way; what
//                   it reads of an earlier launch is visible because that launch has ended (DESIGN.md "Bvh" says why not the
//                   one-launch form with arrival counters)
// The cast:
//   k_bvh_cast      a ray per lane, a stack walk nearer child first.  The stack has kCastStack = 64 entries and cannot overflow: a pop
//                   pushes at most the two children of a node, so it holds at most one entry per level and one more, and depth <= 62.
//                   It lies in LDS interleaved by lane (a runtime-indexed private array would go to scratch): 64 entries * (a node
//                   and the float below its near bound) * 64 lanes = 32 KiB a workgroup of one wavefront
// The closest point:
//   k_bvh_nearest   a point per lane, the same stack and the same argument for its size: a node and the float below the bound of its
//                   box (rounded down it is still a lower bound, FLT_MAX where the double is beyond the floats).  Both children's
//                   bounds at a node, leaves answered at once, the nearer internal child popped first; whatever has a bound
//                   strictly greater than the best d2_t so far is skipped -- sound because d2_t is clamped from below by the bound
//                   of the triangle's own leaf box, and a box that contains another has a bound no greater (DESIGN.md "Bvh")
// The pairs that pass through each other (hry_intersections_build), in two stretches:
//   k_bvh_pairs     a leaf per lane, the same stack with node numbers alone (16 KiB): the lane's leaf box against both children's
//                   boxes, leaves answered at once, internal children pushed.  Every pair of leaves whose boxes overlap is met from
//                   both sides; the side of the lower triangle number answers it.  First it counts (a count per leaf; C, N, the
//                   box tests and P as integer atomics of wavefront sums), the counts are scanned, P comes down; then the same
//                   body fills each leaf's rows, (s, t | share << 31), and bumps tri_pairs
//   k_radix_*, k_pairs_turn   two stable sorts, by s, then -- key and payload exchanged -- by t: ascending (t, s)
//   k_pairs_emit    pairs and pair_shared from the sorted rows;  k_pairs_hit: H, the triangles with tri_pairs > 0
#include <hip/hip_runtime.h>

#include "dev_types.hpp"
#include "face_normal.hpp"
#include "kernels.hpp"
#include "radix_sort.hpp"
#include "wave.hpp"

namespace hry {
namespace dev {

namespace {

constexpr uint32_t kNone = 0xffffffffu, kLeafBit = 0x80000000u;
constexpr uint32_t kBvhBlock = 256, kCastBlock = 64, kCastStack = 64;
constexpr uint32_t kWordL = 0, kWordDistinct = 1, kWordDepth = 2, kWordBox = 4;

// floats as words whose unsigned order is the floats' order, -0 below +0: a total order, so the least of a set is one value
__device__ __forceinline__ uint32_t ordered(float f) { const uint32_t u = __float_as_uint(f); return u & 0x80000000u ? ~u : u | 0x80000000u; }
__device__ __forceinline__ float unordered(uint32_t w) { return __uint_as_float(w & 0x80000000u ? w ^ 0x80000000u : ~w); }
__device__ __forceinline__ float least(float a, float b) { return ordered(b) < ordered(a) ? b : a; }
__device__ __forceinline__ float greatest(float a, float b) { return ordered(b) > ordered(a) ? b : a; }
__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) < __builtin_inff(); }   // (false for NaN)
__device__ __forceinline__ bool finite_d(double x) { return fabs(x) < __builtin_inf(); }
__device__ __forceinline__ double dot_d(const D3 &a, const D3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// the nine floats of triangle t; false: an index no render build writes, or a float that is not finite
__device__ __forceinline__ bool triangle_of(const BvhWork &w, uint32_t t, float (&p)[9])
{
	bool live = true;
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		const uint32_t u = w.indices[3 * (size_t)t + k];
		if (u >= w.nout) { p[3 * k] = p[3 * k + 1] = p[3 * k + 2] = __builtin_nanf(""); live = false; continue; }
		const float *q = w.pos + (size_t)u * w.pos_stride;
#pragma unroll
		for (int c = 0; c < 3; ++c) { p[3 * k + c] = q[c]; live = live && finite_f(q[c]); }
	}
	return live;
}

__global__ void k_bvh_init(uint32_t *words)
{
	if (threadIdx.x < 4) words[threadIdx.x] = 0;
	if (threadIdx.x < 3) { words[kWordBox + threadIdx.x] = ordered(__builtin_inff()); words[kWordBox + 3 + threadIdx.x] = ordered(-__builtin_inff()); }
}

__global__ __launch_bounds__(kBvhBlock) void k_bvh_live(BvhWork w)
{
	const uint32_t t = blockIdx.x * kBvhBlock + threadIdx.x;
	float p[9];
	const bool live = t < w.T && triangle_of(w, t, p);
	if (t < w.T) w.flag[t] = live ? 1u : 0u;
#pragma unroll
	for (int c = 0; c < 3; ++c) {
		const uint32_t lo = wave_min(live ? ordered(least(least(p[c], p[3 + c]), p[6 + c])) : ordered(__builtin_inff()));
		const uint32_t hi = wave_max(live ? ordered(greatest(greatest(p[c], p[3 + c]), p[6 + c])) : ordered(-__builtin_inff()));
		if ((threadIdx.x & 63) == 0 && lo <= hi) { atomicMin(&w.words[kWordBox + c], lo); atomicMax(&w.words[kWordBox + 3 + c], hi); }
	}
}

__device__ __forceinline__ uint32_t cell_of(double c, float lo, float hi)
{
	if (hi == lo) return 0;
	const double x = ((c - (double)lo) / ((double)hi - (double)lo)) * 1024.0;
	return x >= 1023.0 ? 1023u : x > 0.0 ? (uint32_t)x : 0u;   // truncated toward zero, clamped to 0 .. 1023
}
__device__ __forceinline__ uint32_t spread3(uint32_t x)   // bit j to bit 3 j
{
	x = (x | (x << 16)) & 0x030000ffu;
	x = (x | (x << 8)) & 0x0300f00fu;
	x = (x | (x << 4)) & 0x030c30c3u;
	return (x | (x << 2)) & 0x09249249u;
}

__global__ __launch_bounds__(kBvhBlock) void k_bvh_codes(BvhWork w)
{
	const uint32_t t = blockIdx.x * kBvhBlock + threadIdx.x;
	if (t >= w.T || !w.flag[t]) return;
	float p[9];
	triangle_of(w, t, p);
	uint32_t cell[3];
#pragma unroll
	for (int c = 0; c < 3; ++c) {
		const double mid = (((double)p[c] + (double)p[3 + c]) + (double)p[6 + c]) / 3.0;
		cell[c] = cell_of(mid, unordered(w.words[kWordBox + c]), unordered(w.words[kWordBox + 3 + c]));
	}
	const uint32_t i = w.at[t];
	if (i >= w.T) return;   // (a rank is below L <= T)
	w.code_a[i] = (spread3(cell[0]) << 2) | (spread3(cell[1]) << 1) | spread3(cell[2]);
	w.tri_a[i] = t;
}

// the leading bits that the keys of leaves i and j share; -1 where j is no leaf.  The keys are distinct: they end in the leaf's number
__device__ __forceinline__ int common_prefix(const uint32_t *code, uint32_t L, int64_t i, int64_t j)
{
	if (j < 0 || j >= (int64_t)L) return -1;
	const unsigned long long a = ((unsigned long long)code[i] << 32) | (unsigned long long)i, b = ((unsigned long long)code[j] << 32) | (unsigned long long)j;
	return __clzll((long long)(a ^ b));
}

__global__ __launch_bounds__(kBvhBlock) void k_bvh_tree(BvhWork w)
{
	const uint32_t L = w.words[kWordL], node = blockIdx.x * kBvhBlock + threadIdx.x;
	if (L < 2 || node >= L - 1) return;
	const uint32_t *code = w.code_a;
	const int64_t i = node;
	const int64_t d = common_prefix(code, L, i, i + 1) > common_prefix(code, L, i, i - 1) ? 1 : -1;
	const int floor_ = common_prefix(code, L, i, i - d);
	int64_t reach = 2;
	while (common_prefix(code, L, i, i + reach * d) > floor_) reach *= 2;
	int64_t len = 0;
	for (int64_t step = reach / 2; step >= 1; step /= 2)
		if (common_prefix(code, L, i, i + (len + step) * d) > floor_) len += step;
	const int64_t j = i + len * d;
	const int within = common_prefix(code, L, i, j);
	int64_t s = 0, step = len;
	do {
		step = (step + 1) / 2;
		if (common_prefix(code, L, i, i + (s + step) * d) > within) s += step;
	} while (step > 1);
	const int64_t gamma = i + s * d + (d < 0 ? -1 : 0), a = i < j ? i : j, b = i < j ? j : i;
	const uint32_t left = (uint32_t)gamma, right = (uint32_t)gamma + 1;
	if (a == gamma) { w.children[2 * (size_t)node] = left | kLeafBit; w.leaf_parent[left] = node; }
	else { w.children[2 * (size_t)node] = left; w.node_parent[left] = node; }
	if (b == gamma + 1) { w.children[2 * (size_t)node + 1] = right | kLeafBit; w.leaf_parent[right] = node; }
	else { w.children[2 * (size_t)node + 1] = right; w.node_parent[right] = node; }
	if (node == 0) w.node_parent[0] = kNone;
}

__global__ __launch_bounds__(kBvhBlock) void k_bvh_depth(BvhWork w)
{
	const uint32_t L = w.words[kWordL], i = blockIdx.x * kBvhBlock + threadIdx.x;
	const bool have = i < L;
	uint32_t above = 0;
	if (have && L >= 2)
		for (uint32_t n = w.leaf_parent[i]; n != kNone && above < 64; n = w.node_parent[n]) ++above;   // (at most 62 levels)
	above = wave_max(above);
	const uint32_t first = (uint32_t)__popcll(__ballot(have && (i == 0 || w.code_a[i] != w.code_a[i - 1])));
	if ((threadIdx.x & 63) == 0) {
		if (above) atomicMax(&w.words[kWordDepth], above);
		if (first) atomicAdd(&w.words[kWordDistinct], first);
	}
}

__global__ __launch_bounds__(kBvhBlock) void k_bvh_emit(BvhWork w, BvhView v, uint32_t *round)
{
	const uint32_t i = blockIdx.x * kBvhBlock + threadIdx.x;
	if (i < 6) v.scene_box[i] = unordered(w.words[kWordBox + i]);
	if (i >= v.L) return;
	const uint32_t t = w.tri_a[i];
	float p[9];
	if (t < w.T) triangle_of(w, t, p);
	else for (int k = 0; k < 9; ++k) p[k] = 0.0f;   // (no sort leaves such a number)
	v.leaf_tri[i] = t;
	v.leaf_code[i] = w.code_a[i];
#pragma unroll
	for (int k = 0; k < 9; ++k) v.leaf_positions[9 * (size_t)i + k] = p[k];
#pragma unroll
	for (int c = 0; c < 3; ++c) {
		v.leaf_box[6 * (size_t)i + c] = least(least(p[c], p[3 + c]), p[6 + c]);
		v.leaf_box[6 * (size_t)i + 3 + c] = greatest(greatest(p[c], p[3 + c]), p[6 + c]);
	}
	if (i + 1 < v.L) {
		v.node_children[2 * (size_t)i] = w.children[2 * (size_t)i];
		v.node_children[2 * (size_t)i + 1] = w.children[2 * (size_t)i + 1];
		round[i] = kNone;
	}
}

__global__ __launch_bounds__(kBvhBlock) void k_bvh_fit(BvhView v, uint32_t *round, uint32_t r)
{
	const uint32_t i = blockIdx.x * kBvhBlock + threadIdx.x;
	if (i + 1 >= v.L || round[i] != kNone) return;
	const uint32_t c0 = v.node_children[2 * (size_t)i], c1 = v.node_children[2 * (size_t)i + 1];
	const uint32_t n0 = c0 & ~kLeafBit, n1 = c1 & ~kLeafBit;
	if (n0 >= v.L || n1 >= v.L) return;   // (no tree names such a child)
	// finished by an earlier launch?  A round written in this launch reads kNone or r: not below r either way
	if (!(c0 & kLeafBit) && !(round[n0] < r)) return;
	if (!(c1 & kLeafBit) && !(round[n1] < r)) return;
	const float *b0 = (c0 & kLeafBit ? v.leaf_box : v.node_box) + 6 * (size_t)n0, *b1 = (c1 & kLeafBit ? v.leaf_box : v.node_box) + 6 * (size_t)n1;
#pragma unroll
	for (int c = 0; c < 3; ++c) {
		v.node_box[6 * (size_t)i + c] = least(b0[c], b1[c]);
		v.node_box[6 * (size_t)i + 3 + c] = greatest(b0[3 + c], b1[3 + c]);
	}
	round[i] = r;
}

// ---- the cast
struct Ray { D3 o, d, inv; double tmin, tmax; };

// one axis of it: a direction of +-0 bounds nothing and fails the box where the origin lies outside [lo, hi]; otherwise n and f take
// the axis' nearer and farther crossing
__device__ __forceinline__ bool slab(double lo, double hi, double o, double d, double inv, double &n, double &f)
{
	if (d == 0.0) return !(o < lo || o > hi);
	const double a = (lo - o) * inv, c = (hi - o) * inv;
	const double nk = a < c ? a : c, fk = a < c ? c : a;
	n = nk > n ? nk : n;
	f = fk < f ? fk : f;
	return true;
}
// the interval of a box for a valid ray (the one rule, for leaf and node boxes alike); false: the box fails
__device__ __forceinline__ bool interval(const float *box, const Ray &ray, double &near, double &far)
{
	double n = -__builtin_inf(), f = __builtin_inf();
	if (!slab((double)box[0], (double)box[3], ray.o.x, ray.d.x, ray.inv.x, n, f) || !slab((double)box[1], (double)box[4], ray.o.y, ray.d.y, ray.inv.y, n, f) ||
	    !slab((double)box[2], (double)box[5], ray.o.z, ray.d.z, ray.inv.z, n, f))
		return false;
	const double n1 = n - fabs(n) * 0x1p-30, f1 = f + fabs(f) * 0x1p-30;
	near = ray.tmin > n1 ? ray.tmin : n1;
	far = ray.tmax < f1 ? ray.tmax : f1;
	return near <= far;
}

struct Best { double tt, u, v; uint32_t tri; };

// the line o + tt d against the triangle (p0, p1, p2) (Moeller, Trumbore), the one arithmetic of the cast's hit and of the segment
// test of k_bvh_pairs: inside -- det is finite and not zero, u >= 0, w >= 0, u + w <= 1; the caller bounds tt
struct Meet { double tt, u, w; bool inside; };
__device__ __forceinline__ Meet meet_of(const D3 &o, const D3 &d, const D3 &p0, const D3 &p1, const D3 &p2)
{
	const D3 e1 = sub3(p1, p0), e2 = sub3(p2, p0), pv = cross3(d, e2);
	const double det = dot_d(e1, pv);
	const D3 s = sub3(o, p0), q = cross3(s, e1);
	const double u = dot_d(s, pv) / det, w = dot_d(d, q) / det, tt = dot_d(e2, q) / det;
	return Meet{ tt, u, w, finite_d(det) && det != 0.0 && u >= 0.0 && w >= 0.0 && u + w <= 1.0 };
}

// leaf `leaf`, whose own box has passed with [near, far]
__device__ __forceinline__ void hit_leaf(const BvhView &v, uint32_t leaf, const Ray &ray, double near, double far, Best &best)
{
	const float *p = v.leaf_positions + 9 * (size_t)leaf;
	const D3 p0{ (double)p[0], (double)p[1], (double)p[2] }, p1{ (double)p[3], (double)p[4], (double)p[5] }, p2{ (double)p[6], (double)p[7], (double)p[8] };
	const Meet m = meet_of(ray.o, ray.d, p0, p1, p2);
	if (!(m.inside && near <= m.tt && m.tt <= far)) return;
	const uint32_t t = v.leaf_tri[leaf];
	if (m.tt < best.tt || (m.tt == best.tt && t < best.tri)) best = Best{ m.tt, m.u, m.w, t };
}

__global__ __launch_bounds__(kCastBlock) void k_bvh_cast(BvhView v, BvhCast c)
{
	__shared__ uint32_t s_node[kCastStack * kCastBlock];
	__shared__ float s_near[kCastStack * kCastBlock];
	const uint32_t lane = threadIdx.x;
	unsigned long long hits = 0, tests = 0;
	for (uint64_t base = (uint64_t)blockIdx.x * kCastBlock; base < c.n; base += (uint64_t)gridDim.x * kCastBlock) {
		const uint64_t i = base + lane;
		const bool have = i < c.n;
		Best best{ __builtin_inf(), 0.0, 0.0, kNone };
		uint32_t made = 0;
		if (have) {
			const float *po = (const float*)(c.o + i * c.o_stride), *pd = (const float*)(c.d + i * c.d_stride);
			Ray ray;
			ray.o = D3{ (double)po[0], (double)po[1], (double)po[2] };
			ray.d = D3{ (double)pd[0], (double)pd[1], (double)pd[2] };
			ray.inv = D3{ 1.0 / ray.d.x, 1.0 / ray.d.y, 1.0 / ray.d.z };
			ray.tmin = c.tmin; ray.tmax = c.tmax;
			const bool valid = finite_d(ray.o.x) && finite_d(ray.o.y) && finite_d(ray.o.z) && finite_d(ray.d.x) && finite_d(ray.d.y) && finite_d(ray.d.z) &&
			                   !(ray.d.x == 0.0 && ray.d.y == 0.0 && ray.d.z == 0.0);
			double near, far;
			if (valid && v.L == 1) {
				++made;
				if (interval(v.leaf_box, ray, near, far)) hit_leaf(v, 0, ray, near, far, best);
			} else if (valid && v.L > 1) {
				uint32_t sp = 1;
				s_node[lane] = 0; s_near[lane] = -__builtin_inff();
				while (sp) {
					--sp;
					const uint32_t node = s_node[sp * kCastBlock + lane];
					if ((double)s_near[sp * kCastBlock + lane] > best.tt || node + 1 >= v.L) continue;   // strict: an equal bound may hold a lower number
					const uint32_t c0 = v.node_children[2 * (size_t)node], c1 = v.node_children[2 * (size_t)node + 1];
					const uint32_t n0 = c0 & ~kLeafBit, n1 = c1 & ~kLeafBit;
					if (n0 >= v.L || n1 >= v.L) continue;   // (no tree names such a child)
					double near0, far0, near1, far1;
					bool go0 = interval((c0 & kLeafBit ? v.leaf_box : v.node_box) + 6 * (size_t)n0, ray, near0, far0);
					bool go1 = interval((c1 & kLeafBit ? v.leaf_box : v.node_box) + 6 * (size_t)n1, ray, near1, far1);
					made += 2;
					if (go0 && (c0 & kLeafBit)) { if (!(near0 > best.tt)) hit_leaf(v, n0, ray, near0, far0, best); go0 = false; }
					if (go1 && (c1 & kLeafBit)) { if (!(near1 > best.tt)) hit_leaf(v, n1, ray, near1, far1, best); go1 = false; }
					go0 = go0 && !(near0 > best.tt);
					go1 = go1 && !(near1 > best.tt);
					const bool first1 = go0 && go1 && near1 < near0;   // the nearer child is popped first: pushed last
					const uint32_t na = first1 ? n1 : n0, nb = first1 ? n0 : n1;
					const double ra = first1 ? near1 : near0, rb = first1 ? near0 : near1;
					const bool ga = first1 ? go1 : go0, gb = first1 ? go0 : go1;
					if (gb && sp < kCastStack) { s_node[sp * kCastBlock + lane] = nb; s_near[sp * kCastBlock + lane] = __double2float_rd(rb); ++sp; }
					if (ga && sp < kCastStack) { s_node[sp * kCastBlock + lane] = na; s_near[sp * kCastBlock + lane] = __double2float_rd(ra); ++sp; }
				}
			}
			const bool hit = best.tri != kNone;
			c.hit_tri[i] = best.tri;
			if (c.hit_t) c.hit_t[i] = hit ? (float)best.tt : __builtin_inff();
			if (c.hit_uv) { c.hit_uv[2 * i] = hit ? (float)best.u : 0.0f; c.hit_uv[2 * i + 1] = hit ? (float)best.v : 0.0f; }
		}
		hits += (unsigned long long)__popcll(__ballot(have && best.tri != kNone));
		tests += wave_sum((unsigned long long)made);
	}
	if (lane == 0 && c.stat) {
		if (hits) atomicAdd(&c.stat[0], hits);
		if (tests) atomicAdd(&c.stat[1], tests);
	}
}

// ---- the closest point
// the bound of a box for a point (the one rule, for leaf and node boxes alike): the squared distance to the box, monotone in lo
// downwards and in hi upwards, rounding included
__device__ __forceinline__ double gap(double lo, double hi, double q)
{
	const double a = lo - q, c = q - hi, g = a > c ? a : c;
	return g > 0.0 ? g : 0.0;
}
__device__ __forceinline__ double bound_of(const float *box, const D3 &q)
{
	const double gx = gap((double)box[0], (double)box[3], q.x), gy = gap((double)box[1], (double)box[4], q.y), gz = gap((double)box[2], (double)box[5], q.z);
	return (gx * gx + gy * gy) + gz * gz;
}
// where on the segment (a, a + d) the point with s = q - a lies nearest: 0 for a segment without length, clamped to [0, 1]
__device__ __forceinline__ double along(const D3 &s, const D3 &d)
{
	const double l = dot_d(d, d);
	if (l == 0.0) return 0.0;
	const double x = dot_d(s, d) / l;
	return x < 0.0 ? 0.0 : x > 1.0 ? 1.0 : x;
}

struct Near { double d2, u, v; D3 c; uint32_t tri; };

// leaf `leaf`, the bound of whose own box is b2
__device__ __forceinline__ void near_leaf(const BvhView &v, uint32_t leaf, const D3 &q, double b2, Near &best)
{
	const float *p = v.leaf_positions + 9 * (size_t)leaf;
	const D3 p0{ (double)p[0], (double)p[1], (double)p[2] }, p1{ (double)p[3], (double)p[4], (double)p[5] }, p2{ (double)p[6], (double)p[7], (double)p[8] };
	const D3 e1 = sub3(p1, p0), e2 = sub3(p2, p0), s = sub3(q, p0);
	double d2 = __builtin_inf(), bu = 0.0, bv = 0.0;
	D3 bc{ 0.0, 0.0, 0.0 };
	const auto candidate = [&](double u, double w) {
		const D3 c{ p0.x + (u * e1.x + w * e2.x), p0.y + (u * e1.y + w * e2.y), p0.z + (u * e1.z + w * e2.z) };
		const D3 r = sub3(q, c);
		const double d = dot_d(r, r);
		if (d < d2) { d2 = d; bu = u; bv = w; bc = c; }   // the first with the least: a later one only when strictly less
	};
	const D3 n = cross3(e1, e2);
	const double nn = dot_d(n, n);
	if (nn > 0.0) {
		const double u = dot_d(cross3(s, e2), n) / nn, w = dot_d(cross3(e1, s), n) / nn;
		if (u >= 0.0 && w >= 0.0 && u + w <= 1.0) candidate(u, w);
	}
	const double sb = along(s, e1), sc = along(sub3(q, p1), sub3(p2, p1)), sd = along(sub3(q, p2), sub3(p0, p2));
	candidate(sb, 0.0);
	candidate(1.0 - sc, sc);
	candidate(0.0, 1.0 - sd);
	if (b2 > d2) d2 = b2;   // rounding of c can put d2 an ulp below the box's bound: the skipping rests on d2_t >= that bound
	const uint32_t t = v.leaf_tri[leaf];
	if (d2 < best.d2 || (d2 == best.d2 && t < best.tri)) best = Near{ d2, bu, bv, bc, t };
}

__global__ __launch_bounds__(kCastBlock) void k_bvh_nearest(BvhView v, BvhNearest c)
{
	__shared__ uint32_t s_node[kCastStack * kCastBlock];
	__shared__ float s_bound[kCastStack * kCastBlock];
	const uint32_t lane = threadIdx.x;
	unsigned long long answered = 0, tests = 0, farthest = 0;
	for (uint64_t base = (uint64_t)blockIdx.x * kCastBlock; base < c.n; base += (uint64_t)gridDim.x * kCastBlock) {
		const uint64_t i = base + lane;
		const bool have = i < c.n;
		Near best{ c.r2, 0.0, 0.0, D3{ 0.0, 0.0, 0.0 }, kNone };   // an answer exactly at r2 is accepted: its number is below kNone
		uint32_t made = 0;
		if (have) {
			const float *pq = (const float*)(c.q + i * c.q_stride);
			const D3 q{ (double)pq[0], (double)pq[1], (double)pq[2] };
			const bool valid = c.any && finite_d(q.x) && finite_d(q.y) && finite_d(q.z);
			if (valid && v.L == 1) {
				++made;
				const double b = bound_of(v.leaf_box, q);
				if (!(b > best.d2)) near_leaf(v, 0, q, b, best);
			} else if (valid && v.L > 1) {
				uint32_t sp = 1;
				s_node[lane] = 0; s_bound[lane] = 0.0f;
				while (sp) {
					--sp;
					const uint32_t node = s_node[sp * kCastBlock + lane];
					if ((double)s_bound[sp * kCastBlock + lane] > best.d2 || node + 1 >= v.L) continue;   // strict: an equal bound may hold a lower number
					const uint32_t c0 = v.node_children[2 * (size_t)node], c1 = v.node_children[2 * (size_t)node + 1];
					const uint32_t n0 = c0 & ~kLeafBit, n1 = c1 & ~kLeafBit;
					if (n0 + (c0 & kLeafBit ? 0u : 1u) >= v.L || n1 + (c1 & kLeafBit ? 0u : 1u) >= v.L) continue;   // (no tree names such a child: a leaf below L, a node below L - 1)
					const double b0 = bound_of((c0 & kLeafBit ? v.leaf_box : v.node_box) + 6 * (size_t)n0, q);
					const double b1 = bound_of((c1 & kLeafBit ? v.leaf_box : v.node_box) + 6 * (size_t)n1, q);
					made += 2;
					bool go0 = !(c0 & kLeafBit), go1 = !(c1 & kLeafBit);
					if (!go0 && !(b0 > best.d2)) near_leaf(v, n0, q, b0, best);
					if (!go1 && !(b1 > best.d2)) near_leaf(v, n1, q, b1, best);
					go0 = go0 && !(b0 > best.d2);
					go1 = go1 && !(b1 > best.d2);
					const bool first1 = go0 && go1 && b1 < b0;   // the nearer child is popped first: pushed last
					const uint32_t na = first1 ? n1 : n0, nb = first1 ? n0 : n1;
					const double ra = first1 ? b1 : b0, rb = first1 ? b0 : b1;
					const bool ga = first1 ? go1 : go0, gb = first1 ? go0 : go1;
					if (gb && sp < kCastStack) { s_node[sp * kCastBlock + lane] = nb; s_bound[sp * kCastBlock + lane] = __double2float_rd(rb); ++sp; }
					if (ga && sp < kCastStack) { s_node[sp * kCastBlock + lane] = na; s_bound[sp * kCastBlock + lane] = __double2float_rd(ra); ++sp; }
				}
			}
			const bool hit = best.tri != kNone;
			c.near_tri[i] = best.tri;
			if (c.near_d2) c.near_d2[i] = hit ? best.d2 : __builtin_inf();
			if (c.near_uv) { c.near_uv[2 * i] = hit ? (float)best.u : 0.0f; c.near_uv[2 * i + 1] = hit ? (float)best.v : 0.0f; }
			if (c.near_point) { c.near_point[3 * i] = hit ? (float)best.c.x : 0.0f; c.near_point[3 * i + 1] = hit ? (float)best.c.y : 0.0f; c.near_point[3 * i + 2] = hit ? (float)best.c.z : 0.0f; }
		}
		const bool hit = have && best.tri != kNone;
		answered += (unsigned long long)__popcll(__ballot(hit));
		tests += wave_sum((unsigned long long)made);
		// non-negative doubles order as their words: an integer maximum, whatever the order
		farthest = max(farthest, wave_max(hit ? (unsigned long long)__double_as_longlong(best.d2) : 0ull));
	}
	if (lane == 0 && c.stat) {
		if (answered) atomicAdd(&c.stat[0], answered);
		if (tests) atomicAdd(&c.stat[1], tests);
		if (farthest) atomicMax(&c.stat[2], farthest);
	}
}

// ---- the pairs that pass through each other
struct Tri3 { D3 p[3]; };
__device__ __forceinline__ Tri3 corners_of(const BvhView &v, uint32_t leaf)
{
	const float *p = v.leaf_positions + 9 * (size_t)leaf;
	return Tri3{ { D3{ (double)p[0], (double)p[1], (double)p[2] }, D3{ (double)p[3], (double)p[4], (double)p[5] }, D3{ (double)p[6], (double)p[7], (double)p[8] } } };
}
// a triangle with a normal, as near_leaf asks for its face candidate
__device__ __forceinline__ bool proper(const Tri3 &a)
{
	const D3 n = cross3(sub3(a.p[1], a.p[0]), sub3(a.p[2], a.p[0]));
	return dot_d(n, n) > 0.0;
}
__device__ __forceinline__ bool same_corner(const D3 &a, const D3 &b) { return a.x == b.x && a.y == b.y && a.z == b.z; }   // (the widened floats: -0 equals +0)
// closed, on the floats: the one rule, for leaf and node boxes alike
__device__ __forceinline__ bool boxes_meet(const float (&a)[6], const float *b)
{
	return a[0] <= b[3] && b[0] <= a[3] && a[1] <= b[4] && b[1] <= a[4] && a[2] <= b[5] && b[2] <= a[5];
}
// the segment (a, b) against a triangle: the cast's arithmetic with o = a, d = b - a, and 0 <= tt <= 1
__device__ __forceinline__ bool meets(const D3 &a, const D3 &b, const Tri3 &tri)
{
	const Meet m = meet_of(a, sub3(b, a), tri.p[0], tri.p[1], tri.p[2]);
	return m.inside && 0.0 <= m.tt && m.tt <= 1.0;
}
// two proper triangles: share (0 .. 3) and, where it is 0 or 1, whether an admitted edge of one meets the other -- all six edges
// without a shared corner, with one the edge opposite it on either side.  Edge k is (P_k, P_(k + 1) % 3)
__device__ __forceinline__ bool pass_through(const Tri3 &a, const Tri3 &b, uint32_t &share)
{
	int ka = -1, kb = -1;
	share = 0;
#pragma unroll
	for (int i = 0; i < 3; ++i) {
		bool shared = false;
#pragma unroll
		for (int j = 0; j < 3; ++j)
			if (same_corner(a.p[i], b.p[j])) { shared = true; kb = j; }
		if (shared) { ++share; ka = i; }
	}
	if (share > 1) return false;
	const int ea = share ? (ka + 1) % 3 : -1, eb = share ? (kb + 1) % 3 : -1;   // the edge opposite corner k begins at corner k + 1
	bool any = false;
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		if (!any && (!share || k == ea)) any = meets(a.p[k], a.p[(k + 1) % 3], b);
		if (!any && (!share || k == eb)) any = meets(b.p[k], b.p[(k + 1) % 3], a);
	}
	return any;
}

// A leaf per lane, in leaf order (neighbours in space: the leaves are sorted by code); the cast's stack, node numbers alone.  Every
// leaf whose box meets the lane's is met -- its box lies inside every box above it --, so every pair is met from both sides, and
// the side of the lower triangle number answers it.  c.fill == 0 counts (count[leaf], and C, N, the box tests and P as 64-bit sums),
// c.fill == 1 walks again and writes the pairs where the scan of the counts says: one body, so both make the same decisions
__global__ __launch_bounds__(kCastBlock) void k_bvh_pairs(BvhView v, BvhPairs c)
{
	__shared__ uint32_t s_node[kCastStack * kCastBlock];
	const uint32_t lane = threadIdx.x;
	unsigned long long boxes = 0, tested = 0, made = 0, found = 0;
	for (uint64_t base = (uint64_t)blockIdx.x * kCastBlock; base < v.L; base += (uint64_t)gridDim.x * kCastBlock) {
		const uint64_t i = base + lane;
		uint32_t n_boxes = 0, n_tested = 0, n_made = 0, n_found = 0;
		if (i < v.L && v.L > 1) {
			const uint32_t t = v.leaf_tri[i];
			const Tri3 mine = corners_of(v, (uint32_t)i);
			const bool mine_proper = proper(mine);
			float box[6];
#pragma unroll
			for (int k = 0; k < 6; ++k) box[k] = v.leaf_box[6 * i + k];
			const uint64_t at = c.fill ? c.start[i] : 0;
			const auto leaf = [&](uint32_t j) {
				const uint32_t s = v.leaf_tri[j];
				if (!(t < s)) return;   // (itself, or the other side's pair)
				++n_boxes;
				if (!mine_proper) return;
				const Tri3 other = corners_of(v, j);
				if (!proper(other)) return;
				uint32_t share;
				const bool through = pass_through(mine, other, share);
				if (share > 1) return;
				++n_tested;
				if (!through) return;
				if (c.fill && at + n_found < c.P && t < c.T && s < c.T) {
					c.key[at + n_found] = s;
					c.val[at + n_found] = t | (share << 31);
					atomicAdd(&c.tri_pairs[t], 1u);
					atomicAdd(&c.tri_pairs[s], 1u);
				}
				++n_found;
			};
			uint32_t sp = 1;
			s_node[lane] = 0;
			while (sp) {
				--sp;
				const uint32_t node = s_node[sp * kCastBlock + lane];
				if (node + 1 >= v.L) continue;
				const uint32_t c0 = v.node_children[2 * (size_t)node], c1 = v.node_children[2 * (size_t)node + 1];
				const uint32_t n0 = c0 & ~kLeafBit, n1 = c1 & ~kLeafBit;
				if (n0 + (c0 & kLeafBit ? 0u : 1u) >= v.L || n1 + (c1 & kLeafBit ? 0u : 1u) >= v.L) continue;   // (no tree names such a child: a leaf below L, a node below L - 1)
				const bool go0 = boxes_meet(box, (c0 & kLeafBit ? v.leaf_box : v.node_box) + 6 * (size_t)n0);
				const bool go1 = boxes_meet(box, (c1 & kLeafBit ? v.leaf_box : v.node_box) + 6 * (size_t)n1);
				n_made += 2;
				if (go0 && (c0 & kLeafBit)) leaf(n0);
				if (go1 && (c1 & kLeafBit)) leaf(n1);
				// The two guards -- a child beyond L above, a push beyond the stack here -- keep a hierarchy that hry_bvh_build did not
				// make from reading or writing out of bounds, and nothing more: what they drop is dropped in both stretches alike,
				// so the result would be short and no check would notice.  A hierarchy of hry_bvh_build reaches neither (depth <= 62)
				if (go1 && !(c1 & kLeafBit) && sp < kCastStack) { s_node[sp * kCastBlock + lane] = n1; ++sp; }
				if (go0 && !(c0 & kLeafBit) && sp < kCastStack) { s_node[sp * kCastBlock + lane] = n0; ++sp; }
			}
			if (!c.fill) c.count[i] = n_found;
		} else if (i < v.L && !c.fill) c.count[i] = 0;
		if (!c.fill) {
			boxes += wave_sum((unsigned long long)n_boxes);
			tested += wave_sum((unsigned long long)n_tested);
			made += wave_sum((unsigned long long)n_made);
			found += wave_sum((unsigned long long)n_found);
		}
	}
	if (lane == 0 && !c.fill) {
		if (boxes) atomicAdd(&c.stat[0], boxes);
		if (tested) atomicAdd(&c.stat[1], tested);
		if (made) atomicAdd(&c.stat[2], made);
		if (found) atomicAdd(&c.stat[3], found);
	}
}

// between the two sorts: (s, t | share << 31) becomes (t, s | share << 31)
__global__ __launch_bounds__(kBvhBlock) void k_pairs_turn(uint32_t *key, uint32_t *val, uint32_t P)
{
	const uint32_t i = blockIdx.x * kBvhBlock + threadIdx.x;
	if (i >= P) return;
	const uint32_t s = key[i], packed = val[i];
	key[i] = packed & ~kLeafBit;
	val[i] = s | (packed & kLeafBit);
}
__global__ __launch_bounds__(kBvhBlock) void k_pairs_emit(const uint32_t *key, const uint32_t *val, uint32_t P, uint32_t *pairs, uint32_t *pair_shared)
{
	const uint32_t i = blockIdx.x * kBvhBlock + threadIdx.x;
	if (i >= P) return;
	pairs[2 * (size_t)i] = key[i];
	pairs[2 * (size_t)i + 1] = val[i] & ~kLeafBit;
	pair_shared[i] = val[i] >> 31;
}
// H: the triangles in a pair, a ballot and one integer atomic per wavefront
__global__ __launch_bounds__(kBvhBlock) void k_pairs_hit(const uint32_t *tri_pairs, uint32_t T, uint32_t *hit)
{
	const uint32_t t = blockIdx.x * kBvhBlock + threadIdx.x;
	const uint32_t n = (uint32_t)__popcll(__ballot(t < T && tri_pairs[t] > 0));
	if ((threadIdx.x & 63) == 0 && n) atomicAdd(hit, n);
}

}   // namespace

// ---- launchers (kernels.hpp)
size_t bvh_radix_words(uint32_t T) { return radix_scratch_words(T); }
void launch_bvh_first(hipStream_t st, const BvhWork &w)
{
	hipLaunchKernelGGL(k_bvh_init, dim3(1), dim3(64), 0, st, w.words);
	if (!w.T) return;
	const dim3 grid(blocks_for(w.T, kBvhBlock)), block(kBvhBlock);
	hipLaunchKernelGGL(k_bvh_live, grid, block, 0, st, w);
	launch_excl_scan(st, w.flag, w.T, w.sums, w.at, w.words + kWordL);
	hipLaunchKernelGGL(k_bvh_codes, grid, block, 0, st, w);
	launch_radix_sort(st, w.code_a, w.tri_a, w.code_b, w.tri_b, w.words + kWordL, w.T, 4, w.radix);   // (four passes: back in code_a / tri_a)
	hipLaunchKernelGGL(k_bvh_tree, grid, block, 0, st, w);
	hipLaunchKernelGGL(k_bvh_depth, grid, block, 0, st, w);
}

void launch_bvh_second(hipStream_t st, const BvhWork &w, const BvhView &v, uint32_t depth)
{
	uint32_t *round = w.flag;   // (the flags have served)
	hipLaunchKernelGGL(k_bvh_emit, dim3(blocks_for(v.L ? v.L : 1, kBvhBlock)), dim3(kBvhBlock), 0, st, w, v, round);
	if (v.L < 2) return;
	for (uint32_t r = 1; r <= depth; ++r) hipLaunchKernelGGL(k_bvh_fit, dim3(blocks_for(v.L - 1, kBvhBlock)), dim3(kBvhBlock), 0, st, v, round, r);
}

uint32_t bvh_cast_block() { return kCastBlock; }
void launch_bvh_cast(hipStream_t st, const BvhView &v, const BvhCast &c)
{
	if (!c.n) return;
	hipLaunchKernelGGL(k_bvh_cast, dim3(grid_for(c.n, kCastBlock)), dim3(kCastBlock), 0, st, v, c);
}

void launch_bvh_nearest(hipStream_t st, const BvhView &v, const BvhNearest &c)
{
	if (!c.n) return;
	hipLaunchKernelGGL(k_bvh_nearest, dim3(grid_for(c.n, kCastBlock)), dim3(kCastBlock), 0, st, v, c);
}

size_t bvh_pairs_radix_words(uint32_t P) { return radix_scratch_words(P); }
void launch_bvh_pairs_count(hipStream_t st, const BvhView &v, const BvhPairs &c, uint32_t *sums)
{
	if (v.L) hipLaunchKernelGGL(k_bvh_pairs, dim3(grid_for(v.L, kCastBlock)), dim3(kCastBlock), 0, st, v, c);
	launch_excl_scan(st, c.count, v.L, sums, c.start, c.words);
}

void launch_bvh_pairs_fill(hipStream_t st, const BvhView &v, const BvhPairs &c, uint32_t *key_b, uint32_t *val_b, uint32_t *radix, uint32_t *pairs, uint32_t *pair_shared)
{
	if (c.P) {
		hipLaunchKernelGGL(k_bvh_pairs, dim3(grid_for(v.L, kCastBlock)), dim3(kCastBlock), 0, st, v, c);
		// two stable sorts, by s and then by t, of as many 8-bit passes as the triangle numbers have bytes
		int passes = 1;
		while (passes < 4 && ((uint64_t)c.T - 1) >> (8 * passes)) ++passes;
		uint32_t *ka = c.key, *va = c.val, *kb = key_b, *vb = val_b;
		const dim3 grid(blocks_for(c.P, kBvhBlock)), block(kBvhBlock);
		for (int round = 0; round < 2; ++round) {
			launch_radix_sort(st, ka, va, kb, vb, c.words, c.P, passes, radix);
			if (passes & 1) { std::swap(ka, kb); std::swap(va, vb); }
			if (round == 0) hipLaunchKernelGGL(k_pairs_turn, grid, block, 0, st, ka, va, c.P);
		}
		hipLaunchKernelGGL(k_pairs_emit, grid, block, 0, st, (const uint32_t*)ka, (const uint32_t*)va, c.P, pairs, pair_shared);
	}
	if (c.T) hipLaunchKernelGGL(k_pairs_hit, dim3(blocks_for(c.T, kBvhBlock)), dim3(kBvhBlock), 0, st, (const uint32_t*)c.tri_pairs, c.T, c.words + 1);
}

}   // namespace dev
}   // namespace hry
