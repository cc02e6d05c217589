// Per-component error of one mesh against another through a numbering map (driver: distortion.cpp; contract: include/harry_amd.h,
// hry_distortion_build).  Two kernels, wave64:
//   k_distortion_rows  a block of 256 lanes owns kDistBlockRows consecutive rows of a, lane t the rows t, t + 256, ...: consecutive
//                      lanes read consecutive map entries and records of a (coalesced) and gather one whole record of b each, so a
//                      record's components come from one cache line.  Per component the lanes' (max |e|, lowest row), sum of e*e,
//                      range of a and counters are joined over the wavefront (__shfl_down), then over the block's four wavefronts
//                      through LDS: one DistPart per block and component, and one for the positions.  The per-row buffer is written
//                      on the way.  A map entry at or above b's count raises the status word (a vector atomic, once per wavefront)
//                      and is not followed.
//   k_distortion_fold  one block per list: lane t joins its contiguous span of the blocks' records, the lanes join pairwise in
//                      LDS -- always neighbours, so everything stays in block order.
// (The statistics and their joins: dist_reduce.hpp, shared with sweep.hip.)
// Every join is written out in one fixed order that depends on the row count alone: no floating-point atomics, the same bits
// from run to run.  e*e is rounded on its own (-ffp-contract=off).
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

constexpr uint32_t kNone = kDistNone;
constexpr int kLanes = 256, kWaves = kLanes / 64, kRowsPerLane = (int)(kDistBlockRows / kLanes);
static_assert(kRowsPerLane * kLanes == (int)kDistBlockRows, "a block's rows are a multiple of its lanes");

}   // namespace

__global__ __launch_bounds__(256) void k_distortion_rows(DistList L, RequantPlan pa, RequantPlan pb, uint32_t *status)
{
	__shared__ DistPart s_part[kMaxComp + 1][kWaves];
	const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const uint64_t base = (uint64_t)blockIdx.x * kDistBlockRows;
	const uint8_t *ra[kRowsPerLane], *rb[kRowsPerLane];
	bool live[kRowsPerLane], mapped[kRowsPerLane], pos_ok[kRowsPerLane];
	double esq[kRowsPerLane], d2[kRowsPerLane];
	uint32_t nskip = 0;
	bool bad = false;
#pragma unroll
	for (int k = 0; k < kRowsPerLane; ++k) {
		const uint64_t i = base + (uint64_t)k * kLanes + t;
		live[k] = i < L.rows;
		uint32_t j = kNone;
		if (live[k]) j = L.map ? L.map[i] : (uint32_t)i;
		if (j != kNone && j >= L.b_rows) { bad = true; j = kNone; }   // (never followed)
		mapped[k] = live[k] && j != kNone;
		nskip += live[k] && !mapped[k];
		ra[k] = L.a + (mapped[k] ? i : 0) * L.sa;
		rb[k] = L.b + (size_t)(mapped[k] ? j : 0) * L.sb;
		pos_ok[k] = mapped[k];
		esq[k] = 0.0; d2[k] = 0.0;
	}
	const uint64_t any_bad = __ballot(bad);
	if (any_bad && lane == (uint32_t)__ffsll((unsigned long long)any_bad) - 1) atomicOr(status, 1u);

	for (int c = 0; c < pa.n; ++c) {
		const RequantComp &ca = pa.c[c], &cb = pb.c[c];
		const bool is_pos = L.pos >= 0 && c >= L.pos && c < L.pos + 3;
		DistPart p;
		clear(p);
		p.skipped = nskip;
#pragma unroll
		for (int k = 0; k < kRowsPerLane; ++k) {
			if (!mapped[k]) continue;
			const double x = component_f64(ra[k] + ca.off, ca), y = component_f64(rb[k] + cb.off, cb);
			double sq;
			if (tally(p, x, y, (uint32_t)(base + (uint64_t)k * kLanes + t), sq)) {
				esq[k] = esq[k] + sq;
				if (is_pos) d2[k] = c == L.pos ? sq : d2[k] + sq;   // (ex*ex + ey*ey) + ez*ez
			} else if (is_pos) pos_ok[k] = false;
		}
		wave_join(p);
		if (lane == 0) s_part[c][wave] = p;
	}
	if (L.pos >= 0) {
		DistPart p;
		clear(p);
		p.skipped = nskip;
#pragma unroll
		for (int k = 0; k < kRowsPerLane; ++k) {
			if (!pos_ok[k]) continue;
			offer(p, sqrt(d2[k]), (uint32_t)(base + (uint64_t)k * kLanes + t));
			p.sum = p.sum + d2[k];
			p.compared += 1;
		}
		wave_join(p);
		if (lane == 0) s_part[pa.n][wave] = p;
	}
	if (L.err) {
#pragma unroll
		for (int k = 0; k < kRowsPerLane; ++k)
			if (live[k]) L.err[base + (uint64_t)k * kLanes + t] = mapped[k] ? (float)sqrt(esq[k]) : 0.0f;
	}
	__syncthreads();
	const uint32_t nslots = (uint32_t)pa.n + (L.pos >= 0 ? 1u : 0u);
	if (t < nslots) L.part[(size_t)blockIdx.x * nslots + t] = block_join<kWaves>(s_part[t]);
}

__global__ __launch_bounds__(256) void k_distortion_fold(DistFold f, DistFinal *out)
{
	__shared__ DistFinal s[kLanes];
	const uint32_t l = blockIdx.x;
	for (uint32_t c = 0; c < f.nslots[l]; ++c) fold_slot<kLanes>(f.part[l], f.nblocks[l], f.nslots[l], c, s, out + f.out_at[l] + c);
}

void launch_distortion_rows(hipStream_t st, const DistList &L, const RequantPlan &pa, const RequantPlan &pb, uint32_t *status)
{
	if (L.rows) hipLaunchKernelGGL(k_distortion_rows, dim3(distortion_blocks(L.rows)), dim3(kLanes), 0, st, L, pa, pb, status);
}
void launch_distortion_fold(hipStream_t st, const DistFold &f, DistFinal *out)
{
	if (f.n > 0) hipLaunchKernelGGL(k_distortion_fold, dim3((unsigned)f.n), dim3(kLanes), 0, st, f, out);
}

}   // namespace dev
}   // namespace hry
