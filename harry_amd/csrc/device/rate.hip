// The byte-plane histograms of the vertex attributes' residual codes at every quantisation width in one pass over the coding order
// (driver: rate.cpp; contract: include/harry_amd.h, hry_rate_sweep_build).  Neither the fan of a vertex nor the
// minimum and shared extent of a component depend on the width, so what k_predict_vtx does for the mesh as it stands is done here
// for every width: the shared functions themselves (predict.hpp, dequant.hpp, codec_math.hpp), not a restatement.
//   k_rate_sweep  grid (blocks of kRateBlock coded vertices in the encoder's XCD-aware map, 1 + groups of kRateGroup widths).  A
//                 lane walks the fan of its vertex once into LDS candidates.  Then, per component: the raw values of the vertex and
//                 of its candidates' corners are loaded once into registers, and per width of the block's group taken through
//                 k_requant's quantiser (quantise_raw, stored_bits), predicted in the storage type of that width and folded
//                 (residual_bits); every byte of the code is counted in an LDS histogram with LDS atomics.  The component's
//                 original type is a template argument: the quantiser's switch folds away.  Row 0 -- the component as it stands --
//                 is the same code with the stored value in place of the quantised one; it is the first group's only row, since
//                 a lossless 64-bit integer has eight planes where a quantised value has four at most.  After a component the
//                 block adds its non-zero bins to the table with atomicAdd on u32: integer sums, the same in any order.
// How many widths a block takes trades LDS (4 KiB a width beside the candidates' 24 KiB) against walking the fan again.
#include <hip/hip_runtime.h>

#include "codec_math.hpp"
#include "dequant.hpp"
#include "dev_types.hpp"
#include "fan.hpp"
#include "kernels.hpp"
#include "predict.hpp"

namespace hry {
namespace dev {

namespace {

constexpr int kRateGroup = 6;
static_assert(kRateGroup * kRatePlanes >= kRatePlanes0, "the histograms of a group of widths hold the eight planes of row 0");

typedef uint32_t RateHist[kRatePlanes][256];

// h: the planes of one row
template <typename T> __device__ __forceinline__ void count_code(typename cm::word<sizeof(T)>::u code, uint32_t (*h)[256])
{
#pragma unroll
	for (int b = 0; b < (int)sizeof(T); ++b) atomicAdd(&h[b][(uint32_t)(code >> (8 * b)) & 0xffu], 1u);
}

// what hry_requant to `bits` bits stores of the unquantised value raw of type SRC
template <int SRC> __device__ __forceinline__ uint32_t quantised(uint64_t raw, const RequantComp &c, int bits)
{
	RequantComp k = c;
	k.src_type = SRC; k.src_bits = 0; k.dst_bits = bits;
	return (uint32_t)stored_bits(quantise_raw(raw, k), bits);
}

// where the lane's vertex is in the walk: half-edge e, vertex v, rank k, nc candidates in the fan
struct RateVertex { uint32_t e, v, k; int nc; };

// the widths b0 .. b0 + kRateGroup - 1 (those in 1 .. qmax) of one swept component
template <int SRC>
__device__ __forceinline__ void rate_widths(const RateList &L, const RateComp &C, const Topo &tp, const uint32_t *rank, const RateVertex &x, int b0,
                                            uint32_t (*s_cand)[256], RateHist *s_hist)
{
	auto slot = [&](uint32_t v) { return load_raw(L.rec + (size_t)v * L.stride + C.rc.off, SRC); };
	const uint64_t self = slot(x.v);
	uint64_t raw[3 * kEncCand];
	if (x.nc <= kEncCand) {
#pragma unroll
		for (int i = 0; i < kEncCand; ++i)
			if (i < x.nc) {
#pragma unroll
				for (int j = 0; j < 3; ++j) raw[3 * i + j] = slot(s_cand[3 * i + j][threadIdx.x]);
			}
	}
#pragma unroll 1
	for (int g = 0; g < kRateGroup; ++g) {
		const int bits = b0 + g;
		if (bits < 1 || bits > C.qmax) continue;
		uint32_t qv[3 * kEncCand];
		if (x.nc <= kEncCand) {
#pragma unroll
			for (int i = 0; i < kEncCand; ++i)
				if (i < x.nc) {
#pragma unroll
					for (int j = 0; j < 3; ++j) qv[3 * i + j] = quantised<SRC>(raw[3 * i + j], C.rc, bits);
				}
		}
		const uint32_t qself = quantised<SRC>(self, C.rc, bits);
		auto in_type = [&](auto tag) {
			typedef decltype(tag) T;
			const T pred = x.nc > kEncCand ? predict_walked<T>(tp, rank, bits, x.e, x.k, 0, [&](uint32_t v) { return (T)quantised<SRC>(slot(v), C.rc, bits); })
			                               : predict_kept<T>(x.nc, bits, [&](int s) { return (T)qv[s]; });
			count_code<T>(cm::residual_bits<T>((T)qself, pred, bits), s_hist[g]);
		};
		if (bits <= 8) in_type(uint8_t()); else if (bits <= 16) in_type(uint16_t()); else in_type(uint32_t());
	}
}

// row 0: the component as it stands, in its storage type
template <typename T>
__device__ __forceinline__ void rate_as_stored(const RateList &L, const RateComp &C, const Topo &tp, const uint32_t *rank, const RateVertex &x,
                                               uint32_t (*s_cand)[256], uint32_t (*hist)[256])
{
	const int q = C.quant0;
	auto value = [&](uint32_t v) { return ldg<T>(L.rec + (size_t)v * L.stride + C.rc.off); };
	const T pred = x.nc > kEncCand ? predict_walked<T>(tp, rank, q, x.e, x.k, 0, value)
	                               : predict_kept<T>(x.nc, q, [&](int s) { return value(s_cand[s][threadIdx.x]); });
	count_code<T>(cm::residual_bits<T>(value(x.v), pred, q), hist);
}

}   // namespace

__global__ __launch_bounds__(kRateBlock) void k_rate_sweep(ConnView cv, const uint32_t *order_v, uint32_t n, const uint32_t *rank, RateList L, uint32_t blocks_per_xcd)
{
	__shared__ uint32_t s_cand[kEncCand * 3][256];
	__shared__ RateHist s_hist[kRateGroup];
	static_assert(kRateBlock == 256, "a lane's column of the candidates");
	const uint32_t vb = (blockIdx.x & 7u) * blocks_per_xcd + (blockIdx.x >> 3);
	const uint32_t k = vb * kRateBlock + threadIdx.x;
	const bool active = k < n;
	const bool first = blockIdx.y == 0;                                  // row 0 alone; then the widths in groups
	const int b0 = first ? 0 : ((int)blockIdx.y - 1) * kRateGroup + 1;
	uint32_t *const bins = &s_hist[0][0][0];
	constexpr uint32_t kBins = kRateGroup * kRatePlanes * 256, kRowBins = kRatePlanes * 256;
	for (uint32_t i = threadIdx.x; i < kBins; i += kRateBlock) bins[i] = 0;
	Topo tp{ cv };
	RateVertex x{ 0, 0, k, 0 };
	if (active) {
		x.e = order_v[k];
		x.v = cv.org[x.e];
		x.nc = keep_candidates(tp, rank, x.e, k, s_cand);
	}
	__syncthreads();
	for (int c = 0; c < L.n; ++c) {
		const RateComp &C = L.c[c];
		const bool row0 = first && C.row0 != 0;
		const bool widths = !first && b0 <= C.qmax;
		if (!row0 && !widths) continue;   // (the whole block)
		if (active) {
			if (row0) with_stype(C.stype0, [&](auto tag) { rate_as_stored<decltype(tag)>(L, C, tp, rank, x, s_cand, &s_hist[0][0]); });
			if (widths)
				switch (C.rc.src_type) {
				case 0: rate_widths<0>(L, C, tp, rank, x, b0, s_cand, s_hist); break;
				case 1: rate_widths<1>(L, C, tp, rank, x, b0, s_cand, s_hist); break;
				case 2: rate_widths<2>(L, C, tp, rank, x, b0, s_cand, s_hist); break;
				case 3: rate_widths<3>(L, C, tp, rank, x, b0, s_cand, s_hist); break;
				case 4: rate_widths<4>(L, C, tp, rank, x, b0, s_cand, s_hist); break;
				case 5: rate_widths<5>(L, C, tp, rank, x, b0, s_cand, s_hist); break;
				case 6: rate_widths<6>(L, C, tp, rank, x, b0, s_cand, s_hist); break;
				case 7: rate_widths<7>(L, C, tp, rank, x, b0, s_cand, s_hist); break;
				case 8: rate_widths<8>(L, C, tp, rank, x, b0, s_cand, s_hist); break;
				case 9: rate_widths<9>(L, C, tp, rank, x, b0, s_cand, s_hist); break;
				default: break;
				}
		}
		__syncthreads();
		// the component's rows in the table: two for row 0 (eight planes), then one per width 1 .. qmax.  A bin is non-zero only
		// where something was counted: in the first kRatePlanes0 planes of a row-0 block, else in the rows of widths <= qmax
		for (uint32_t i = threadIdx.x; i < kBins; i += kRateBlock) {
			const uint32_t cnt = bins[i];
			if (!cnt) continue;
			const size_t at = first ? (size_t)C.slot * kRowBins + i : (size_t)(C.slot + 1 + (uint32_t)b0 + i / kRowBins) * kRowBins + i % kRowBins;
			atomicAdd(L.table + at, cnt);
			bins[i] = 0;
		}
		__syncthreads();
	}
}

void launch_rate_sweep(hipStream_t st, const ConnView &cv, const uint32_t *order_v, uint32_t n, const uint32_t *rank, const RateList &L)
{
	int qmax = 0;   // the widest component's
	for (int c = 0; c < L.n; ++c) qmax = std::max(qmax, (int)L.c[c].qmax);
	if (!n || !L.n) return;
	const unsigned per = (blocks_for(n, kRateBlock) + 7) / 8;   // blocks per XCD; the grid is padded to 8 * per, surplus blocks find k >= n
	hipLaunchKernelGGL(k_rate_sweep, dim3(per * 8, 1u + (unsigned)((qmax + kRateGroup - 1) / kRateGroup)), dim3(kRateBlock), 0, st, cv, order_v, n, rank, L, per);
}

}   // namespace dev
}   // namespace hry
