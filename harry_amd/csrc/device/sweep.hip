// The error of every quantisation width of a list's unquantised components in one pass (driver: sweep.cpp; contract:
// include/harry_amd.h, hry_quant_sweep_build).  The minimum and the shared extent of a component do not depend on the width, so a
// value is read once and, in registers, taken through k_requant's quantiser (quantise_raw, stored_bits) and the -c dequantiser
// (dequantise_bits) at every width: the functions of dequant.hpp themselves, not a restatement.  Two kernels, wave64:
//   k_quant_sweep       grid (blocks of kDistBlockRows rows, jobs, groups of kSweepGroup widths).  A job is one swept component, or
//                       -- one behind them -- the positions: the three position components at one width, (ex*ex + ey*ey) + ez*ez.
//                       A lane keeps one DistPart per width of its group: the width loop is unrolled with compile-time indices, so
//                       the kSweepGroup records stay in VGPRs (thirty of them would not: the widths are split over blockIdx.z, and
//                       a column is read again per group, from L2).  How many widths a block takes is a measured choice (DESIGN.md
//                       7f): fewer widths, fewer VGPRs, more wavefronts to overlap the chains of divisions.  The component's type
//                       is a template argument: the switches of the shared functions fold away.  Lanes join by shuffles,
//                       wavefronts through LDS: one DistPart per block, component and width -- k_distortion_rows' shape
//                       (dist_reduce.hpp).
//   k_quant_sweep_fold  one block per (component, width) record: the blocks' records in block order (fold_slot).
// No floating-point atomics; every join in an order fixed by the row count alone.  e*e is rounded on its own (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include "codec_math.hpp"
#include "dequant.hpp"
#include "dev_types.hpp"
#include "dist_reduce.hpp"
#include "fan.hpp"
#include "kernels.hpp"

namespace hry {
namespace dev {

namespace {

constexpr int kLanes = 256, kWaves = kLanes / 64, kRowsPerLane = (int)(kDistBlockRows / kLanes);
static_assert(kRowsPerLane * kLanes == (int)kDistBlockRows, "a block's rows are a multiple of its lanes");

template <int T> __device__ __forceinline__ void sweep_component(const SweepList &L, const SweepComp &sc, int q0, DistPart (&p)[kSweepGroup])
{
	const uint64_t base = (uint64_t)blockIdx.x * kDistBlockRows;
#pragma unroll 1
	for (int r = 0; r < kRowsPerLane; ++r) {
		const uint64_t i = base + (uint64_t)r * kLanes + threadIdx.x;
		if (i >= L.rows) break;
		const uint64_t raw = load_raw(L.rec + i * L.stride + sc.rc.off, T);
		const double x = value_f64(raw, T);
#pragma unroll
		for (int j = 0; j < kSweepGroup; ++j) {
			if (q0 + j > sc.qmax) continue;
			double sq;
			(void)tally(p[j], x, value_at<T>(raw, sc.rc, q0 + j), (uint32_t)i, sq);
		}
	}
}
// the three position components at one width each: a row is compared when all three pairs are finite
__device__ __forceinline__ void sweep_positions(const SweepList &L, int q0, DistPart (&p)[kSweepGroup])
{
	const uint64_t base = (uint64_t)blockIdx.x * kDistBlockRows;
#pragma unroll 1
	for (int r = 0; r < kRowsPerLane; ++r) {
		const uint64_t i = base + (uint64_t)r * kLanes + threadIdx.x;
		if (i >= L.rows) break;
		double d2[kSweepGroup];
		bool ok[kSweepGroup];
#pragma unroll
		for (int j = 0; j < kSweepGroup; ++j) { d2[j] = 0.0; ok[j] = true; }
#pragma unroll 1
		for (int a = 0; a < 3; ++a) {
			const RequantComp &c = L.c[L.pos + a].rc;
			const uint64_t raw = load_raw(L.rec + i * L.stride + c.off, c.dst_type);
			const double x = value_f64(raw, c.dst_type);
#pragma unroll
			for (int j = 0; j < kSweepGroup; ++j) {
				if (q0 + j > L.pos_qmax) continue;
				const double y = value_at<-1>(raw, c, q0 + j);
				if (finite_f64(x) && finite_f64(y)) {
					const double e = y - x, sq = e * e;
					d2[j] = a == 0 ? sq : d2[j] + sq;   // (ex*ex + ey*ey) + ez*ez
				} else ok[j] = false;
			}
		}
#pragma unroll
		for (int j = 0; j < kSweepGroup; ++j) {
			if (q0 + j > L.pos_qmax || !ok[j]) continue;
			offer(p[j], sqrt(d2[j]), (uint32_t)i);
			p[j].sum = p[j].sum + d2[j];
			p[j].compared += 1;
		}
	}
}

}   // namespace

__global__ __launch_bounds__(256) void k_quant_sweep(SweepList L)
{
	__shared__ DistPart s_part[kSweepGroup][kWaves];
	const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const int job = (int)blockIdx.y, q0 = (int)blockIdx.z * kSweepGroup + 1;
	const bool positions = job == L.n;
	const int qmax = positions ? L.pos_qmax : L.c[job].qmax;
	if (q0 > qmax) return;   // (the whole block: nothing of this group is ever read)
	DistPart p[kSweepGroup];
#pragma unroll
	for (int j = 0; j < kSweepGroup; ++j) clear(p[j]);
	if (positions) sweep_positions(L, q0, p);
	else {
		const SweepComp &sc = L.c[job];
		switch (sc.rc.dst_type) {
		case 0: sweep_component<0>(L, sc, q0, p); break;
		case 1: sweep_component<1>(L, sc, q0, p); break;
		case 2: sweep_component<2>(L, sc, q0, p); break;
		case 3: sweep_component<3>(L, sc, q0, p); break;
		case 4: sweep_component<4>(L, sc, q0, p); break;
		case 5: sweep_component<5>(L, sc, q0, p); break;
		case 6: sweep_component<6>(L, sc, q0, p); break;
		case 7: sweep_component<7>(L, sc, q0, p); break;
		case 8: sweep_component<8>(L, sc, q0, p); break;
		case 9: sweep_component<9>(L, sc, q0, p); break;
		default: break;
		}
	}
#pragma unroll
	for (int j = 0; j < kSweepGroup; ++j) {
		wave_join(p[j]);
		if (lane == 0) s_part[j][wave] = p[j];
	}
	__syncthreads();
	if (t < (uint32_t)kSweepGroup && q0 + (int)t <= qmax) {
		const uint32_t slot = (positions ? L.pos_slot : L.c[job].slot) + (uint32_t)(q0 - 1) + t;
		L.part[(size_t)blockIdx.x * L.ns + slot] = block_join<kWaves>(s_part[t]);
	}
}

__global__ __launch_bounds__(256) void k_quant_sweep_fold(DistFold f, DistFinal *out)
{
	__shared__ DistFinal s[kLanes];
	const uint32_t l = blockIdx.y, c = blockIdx.x;
	if (c >= f.nslots[l]) return;
	fold_slot<kLanes>(f.part[l], f.nblocks[l], f.nslots[l], c, s, out + f.out_at[l] + c);
}

void launch_quant_sweep(hipStream_t st, const SweepList &L)
{
	const int jobs = L.n + (L.pos >= 0 ? 1 : 0);
	int qmax = L.pos >= 0 ? L.pos_qmax : 0;
	for (int j = 0; j < L.n; ++j) qmax = std::max(qmax, (int)L.c[j].qmax);
	if (!L.rows || !jobs || qmax <= 0) return;
	const dim3 grid(distortion_blocks(L.rows), (unsigned)jobs, (unsigned)((qmax + kSweepGroup - 1) / kSweepGroup));
	hipLaunchKernelGGL(k_quant_sweep, grid, dim3(kLanes), 0, st, L);
}
void launch_quant_sweep_fold(hipStream_t st, const DistFold &f, DistFinal *out)
{
	uint32_t ns = 0;
	for (int l = 0; l < f.n; ++l) ns = std::max(ns, f.nslots[l]);
	if (f.n > 0 && ns) hipLaunchKernelGGL(k_quant_sweep_fold, dim3(ns, (unsigned)f.n), dim3(kLanes), 0, st, f, out);
}

}   // namespace dev
}   // namespace hry
