// The shading error of a quantisation: the angle between a face's normal before and after, as the chord between the two unit
// normals (contract: include/harry_amd.h, hry_normal_error; drivers: sweep.cpp, distortion.cpp).  A face's normal at
// width q depends only on its corners' raw position values and on the components' minimum and shared extent, none of which depends
// on q: one gather per face serves every width, the rest is arithmetic in registers.  Three kernels, wave64, a lane per face:
//   k_normal_sweep<T>     grid (blocks of kDistBlockRows faces, groups of kNormalGroup widths); T: the components' type.  A lane gathers the raw position
//                         values of its face's corners once per group, forms n_x once, and per width of the group takes the raws
//                         through quantise_raw -> stored_bits -> dequantise_bits (dequant.hpp's own functions), forms N_y and
//                         tallies.  Two shapes of the gather: an all-triangle mesh (no face offsets) keeps its nine raws in
//                         registers across the widths; with general degrees the corner loop is the outer loop, and per width only
//                         a FanSum (corner 0, the previous corner, the running N_y: face_normal.hpp) is kept, whatever the face's
//                         degree.  The width loop is unrolled with compile-time indices: no per-width array is indexed at run time.
//   k_distortion_normals  the same face function with "the value of b at the mapped row" in place of "quantise at q"; writes the
//                         per-face buffer on the way (lane t owns faces t, t + 256, ...: coalesced).
//   k_normal_fold         one block per slot: the blocks' records in block order (fold_slot).
// Lanes join by shuffles, wavefronts through LDS, blocks in k_normal_fold: the joins of dist_reduce.hpp over NormPart.  No
// floating-point atomics; every join in an order fixed by the face count alone.  Nothing is read out of bounds: a corner beyond
// the half-edges, a vertex beyond the row table and a row beyond the list make the face `skipped`.
#include <hip/hip_runtime.h>

#include "codec_math.hpp"
#include "dequant.hpp"
#include "dev_types.hpp"
#include "dist_reduce.hpp"
#include "face_normal.hpp"
#include "fan.hpp"
#include "kernels.hpp"

namespace hry {
namespace dev {

namespace {

constexpr int kLanes = 256, kWaves = kLanes / 64, kFacesPerLane = (int)(kDistBlockRows / kLanes);
static_assert(kFacesPerLane * kLanes == (int)kDistBlockRows, "a block's faces are a multiple of its lanes");

// the corners [lo, hi) of face f; false: the tables do not hold them
__device__ __forceinline__ bool face_span(const NormalFaces &F, uint32_t f, uint64_t &lo, uint64_t &hi)
{
	if (F.foff) { lo = F.foff[f]; hi = F.foff[f + 1]; }
	else { lo = 3ull * f; hi = lo + 3; }   // every face a triangle: no table
	return hi >= lo && hi <= F.ne;
}
// the record of the position list that corner k's vertex names, kDistNone: none
__device__ __forceinline__ uint32_t corner_row(const NormalFaces &F, uint64_t k)
{
	const uint32_t v = F.org[k];
	if (v >= F.nv) return kDistNone;
	const uint32_t row = F.rows ? F.rows[v] : v;
	return row < F.nrows ? row : kDistNone;
}
__device__ __forceinline__ bool finite3(const D3 &p) { return finite_f64(p.x) && finite_f64(p.y) && finite_f64(p.z); }

// face f into a lane's record, its classes tested in the contract's order.  have_x: the source face has a normal, n_x; returns the
// chord of a compared face, 0 otherwise
__device__ __forceinline__ double tally_face(NormPart &p, bool skip, bool finite, bool have_x, const D3 &nx, const D3 &Ny, uint32_t f)
{
	if (skip) { p.skipped += 1; return 0.0; }
	if (!finite) { p.nonfinite += 1; return 0.0; }
	if (!have_x) { p.degenerate += 1; return 0.0; }
	D3 ny;
	if (!unit_normal(Ny, ny)) { p.collapsed += 1; return 0.0; }
	const double c2 = chord_sq(nx, ny), chord = sqrt(c2);
	offer(p, chord, f);
	p.sum = p.sum + c2;
	p.compared += 1;
	return chord;
}

template <int T> __device__ __forceinline__ void sweep_faces(const NormalSweep &S, int q0, NormPart (&p)[kNormalGroup])
{
	const NormalFaces &F = S.F;
	const uint64_t base = (uint64_t)blockIdx.x * kDistBlockRows;
	const int t0 = T >= 0 ? T : S.c[0].dst_type, t1 = T >= 0 ? T : S.c[1].dst_type, t2 = T >= 0 ? T : S.c[2].dst_type;
#pragma unroll 1
	for (int r = 0; r < kFacesPerLane; ++r) {
		const uint64_t i = base + (uint64_t)r * kLanes + threadIdx.x;
		if (i >= F.nf) break;
		const uint32_t f = (uint32_t)i;
		uint64_t lo, hi;
		bool skip = !face_span(F, f, lo, hi);
		if (!F.foff) {
			// ---- triangles: nine raws stay in registers across the group's widths
			uint64_t raw[9];
			bool xfin = true;
			FanSum fx;
			fan_clear(fx);
#pragma unroll
			for (int k = 0; k < 3; ++k) {
				raw[3 * k] = raw[3 * k + 1] = raw[3 * k + 2] = 0;
				const uint32_t row = skip ? kDistNone : corner_row(F, lo + k);
				if (row == kDistNone) { skip = true; continue; }
				const uint8_t *rec = S.rec + (size_t)row * S.stride;
				raw[3 * k] = load_raw(rec + S.c[0].off, t0); raw[3 * k + 1] = load_raw(rec + S.c[1].off, t1); raw[3 * k + 2] = load_raw(rec + S.c[2].off, t2);
				const D3 x{ value_f64(raw[3 * k], t0), value_f64(raw[3 * k + 1], t1), value_f64(raw[3 * k + 2], t2) };
				xfin = xfin && finite3(x);
				fan_step(fx, x, (uint32_t)k);
			}
			D3 nx{ 0.0, 0.0, 0.0 };
			const bool have_x = unit_normal(fx.s, nx);
#pragma unroll
			for (int j = 0; j < kNormalGroup; ++j) {
				if (q0 + j > S.qmax) continue;
				FanSum fy;
				fan_clear(fy);
				bool fin = xfin;
				if (!skip) {
#pragma unroll
					for (int k = 0; k < 3; ++k) {
						const D3 y{ value_at<T>(raw[3 * k], S.c[0], q0 + j), value_at<T>(raw[3 * k + 1], S.c[1], q0 + j), value_at<T>(raw[3 * k + 2], S.c[2], q0 + j) };
						fin = fin && finite3(y);
						fan_step(fy, y, (uint32_t)k);
					}
				}
				(void)tally_face(p[j], skip, fin, have_x, nx, fy.s, f);
			}
			continue;
		}
		// ---- general degrees: the corner loop outside, one FanSum per width of the group
		FanSum fx, fy[kNormalGroup];
		bool fin[kNormalGroup];
		fan_clear(fx);
#pragma unroll
		for (int j = 0; j < kNormalGroup; ++j) { fan_clear(fy[j]); fin[j] = true; }
#pragma unroll 1
		for (uint64_t k = lo; k < hi && !skip; ++k) {
			const uint32_t row = corner_row(F, k);
			if (row == kDistNone) { skip = true; break; }
			const uint8_t *rec = S.rec + (size_t)row * S.stride;
			const uint64_t r0 = load_raw(rec + S.c[0].off, t0), r1 = load_raw(rec + S.c[1].off, t1), r2 = load_raw(rec + S.c[2].off, t2);
			const D3 x{ value_f64(r0, t0), value_f64(r1, t1), value_f64(r2, t2) };
			const bool xfin = finite3(x);
			const uint32_t at = (uint32_t)(k - lo);
			fan_step(fx, x, at);
#pragma unroll
			for (int j = 0; j < kNormalGroup; ++j) {
				if (q0 + j > S.qmax) continue;
				const D3 y{ value_at<T>(r0, S.c[0], q0 + j), value_at<T>(r1, S.c[1], q0 + j), value_at<T>(r2, S.c[2], q0 + j) };
				fin[j] = fin[j] && xfin && finite3(y);
				fan_step(fy[j], y, at);
			}
		}
		D3 nx{ 0.0, 0.0, 0.0 };
		const bool have_x = unit_normal(fx.s, nx);
#pragma unroll
		for (int j = 0; j < kNormalGroup; ++j) {
			if (q0 + j > S.qmax) continue;
			(void)tally_face(p[j], skip, fin[j], have_x, nx, fy[j].s, f);
		}
	}
}

}   // namespace

// T: the three components' common type (its switches in the shared functions fold away, and every type has the registers of its
// own arithmetic, not of the widest), or -1: they differ
template <int T> __global__ __launch_bounds__(256) void k_normal_sweep(NormalSweep S)
{
	__shared__ NormPart s_part[kNormalGroup][kWaves];
	const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const int q0 = (int)blockIdx.y * kNormalGroup + 1;
	if (q0 > S.qmax) return;   // (the whole block)
	NormPart p[kNormalGroup];
#pragma unroll
	for (int j = 0; j < kNormalGroup; ++j) clear(p[j]);
	sweep_faces<T>(S, q0, p);
#pragma unroll
	for (int j = 0; j < kNormalGroup; ++j) {
		wave_join(p[j]);
		if (lane == 0) s_part[j][wave] = p[j];
	}
	__syncthreads();
	if (t < (uint32_t)kNormalGroup && q0 + (int)t <= S.qmax)
		S.part[(size_t)blockIdx.x * (uint32_t)S.qmax + (uint32_t)(q0 - 1) + t] = block_join<kWaves>(s_part[t]);
}

__global__ __launch_bounds__(256) void k_distortion_normals(NormalPair P)
{
	__shared__ NormPart s_part[kWaves];
	const NormalFaces &F = P.F;
	const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const uint64_t base = (uint64_t)blockIdx.x * kDistBlockRows;
	NormPart p;
	clear(p);
#pragma unroll 1
	for (int r = 0; r < kFacesPerLane; ++r) {
		const uint64_t i = base + (uint64_t)r * kLanes + t;
		if (i >= F.nf) break;
		const uint32_t f = (uint32_t)i;
		uint64_t lo, hi;
		bool skip = !face_span(F, f, lo, hi), fin = true;
		FanSum fx, fy;
		fan_clear(fx); fan_clear(fy);
#pragma unroll 1
		for (uint64_t k = lo; k < hi && !skip; ++k) {
			const uint32_t row = corner_row(F, k);
			uint32_t j = row;
			if (row != kDistNone && P.map) j = P.map[row];
			if (j == kDistNone || j >= P.b_rows) { skip = true; break; }   // (never followed)
			const uint8_t *ra = P.a + (size_t)row * P.sa, *rb = P.b + (size_t)j * P.sb;
			const D3 x{ component_f64(ra + P.ca[0].off, P.ca[0]), component_f64(ra + P.ca[1].off, P.ca[1]), component_f64(ra + P.ca[2].off, P.ca[2]) };
			const D3 y{ component_f64(rb + P.cb[0].off, P.cb[0]), component_f64(rb + P.cb[1].off, P.cb[1]), component_f64(rb + P.cb[2].off, P.cb[2]) };
			fin = fin && finite3(x) && finite3(y);
			const uint32_t at = (uint32_t)(k - lo);
			fan_step(fx, x, at);
			fan_step(fy, y, at);
		}
		D3 nx{ 0.0, 0.0, 0.0 };
		const bool have_x = unit_normal(fx.s, nx);
		const double chord = tally_face(p, skip, fin, have_x, nx, fy.s, f);
		if (P.err) P.err[i] = (float)chord;
	}
	wave_join(p);
	if (lane == 0) s_part[wave] = p;
	__syncthreads();
	if (t == 0) P.part[blockIdx.x] = block_join<kWaves>(s_part);
}

__global__ __launch_bounds__(256) void k_normal_fold(const NormPart *part, uint32_t nb, uint32_t ns, NormFinal *out)
{
	__shared__ NormFinal s[kLanes];
	fold_slot<kLanes>(part, nb, ns, blockIdx.x, s, out + blockIdx.x);
}

void launch_normal_sweep(hipStream_t st, const NormalSweep &S)
{
	if (!S.F.nf || S.qmax <= 0) return;
	const dim3 grid(distortion_blocks(S.F.nf), (unsigned)((S.qmax + kNormalGroup - 1) / kNormalGroup));
	switch (S.type) {
	case 0: hipLaunchKernelGGL(k_normal_sweep<0>, grid, dim3(kLanes), 0, st, S); break;
	case 1: hipLaunchKernelGGL(k_normal_sweep<1>, grid, dim3(kLanes), 0, st, S); break;
	case 2: hipLaunchKernelGGL(k_normal_sweep<2>, grid, dim3(kLanes), 0, st, S); break;
	case 3: hipLaunchKernelGGL(k_normal_sweep<3>, grid, dim3(kLanes), 0, st, S); break;
	case 4: hipLaunchKernelGGL(k_normal_sweep<4>, grid, dim3(kLanes), 0, st, S); break;
	case 5: hipLaunchKernelGGL(k_normal_sweep<5>, grid, dim3(kLanes), 0, st, S); break;
	case 6: hipLaunchKernelGGL(k_normal_sweep<6>, grid, dim3(kLanes), 0, st, S); break;
	case 7: hipLaunchKernelGGL(k_normal_sweep<7>, grid, dim3(kLanes), 0, st, S); break;
	case 8: hipLaunchKernelGGL(k_normal_sweep<8>, grid, dim3(kLanes), 0, st, S); break;
	case 9: hipLaunchKernelGGL(k_normal_sweep<9>, grid, dim3(kLanes), 0, st, S); break;
	default: hipLaunchKernelGGL(k_normal_sweep<-1>, grid, dim3(kLanes), 0, st, S); break;
	}
}
void launch_distortion_normals(hipStream_t st, const NormalPair &P)
{
	if (P.F.nf) hipLaunchKernelGGL(k_distortion_normals, dim3(distortion_blocks(P.F.nf)), dim3(kLanes), 0, st, P);
}
void launch_normal_fold(hipStream_t st, const NormPart *part, uint32_t nblocks, uint32_t nslots, NormFinal *out)
{
	if (nslots) hipLaunchKernelGGL(k_normal_fold, dim3(nslots), dim3(kLanes), 0, st, part, nblocks, nslots, out);
}

}   // namespace dev
}   // namespace hry
