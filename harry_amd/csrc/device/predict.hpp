// The prediction of one component of a coded vertex (attrcode.h:182-208), over "how a value is obtained": k_predict_vtx
// (kernels.hip) reads the records as they stand, k_rate_sweep (rate.hip) takes them through the quantiser at a run-time width first.
// The fan is walked ONCE per vertex: the (at most kEncCand) candidate triples that pass the rank filter are kept as vertex ids in
// LDS (keep_candidates) and every component is evaluated from them (predict_kept) -- the mean, and for floats the
// nearest-to-the-mean selection, which the reference evaluates in a second sweep over the same candidates.  A fan with more
// candidates (high-valence vertices) takes predict_walked, which walks again per component.
#pragma once
#include <hip/hip_runtime.h>

#include "codec_math.hpp"
#include "fan.hpp"

namespace hry {
namespace dev {

constexpr int kEncCand = 8;

// the candidates of the vertex at half-edge e (rank k) into the calling lane's column of s_cand, three vertex ids each; returns how
// many the fan has -- more than kEncCand: only the first kEncCand are kept
__device__ __forceinline__ int keep_candidates(const Topo &tp, const uint32_t *rank, uint32_t e, uint32_t k, uint32_t (*s_cand)[256])
{
	int nc = 0;
	fan_candidates(tp, rank, e, k, 0, [&](uint32_t v0, uint32_t v1, uint32_t vo) {
		if (nc < kEncCand) { s_cand[3 * nc][threadIdx.x] = v0; s_cand[3 * nc + 1][threadIdx.x] = v1; s_cand[3 * nc + 2][threadIdx.x] = vo; }
		++nc;
	});
	return nc;
}

// mean of candidate predictions in fan order (double / int64), integers take the mean, floats the candidate nearest to the mean
// (strict <, first wins).  value(v): component value of vertex v, as a T
template <typename T, typename V>
__device__ __forceinline__ T predict_walked(const Topo &tp, const uint32_t *rank, int q, uint32_t e, uint32_t my_rank, uint32_t lo, V &&value)
{
	typedef typename cm::wide<T>::type W;
	W acc = 0;
	uint32_t n = 0;
	fan_candidates(tp, rank, e, my_rank, lo, [&](uint32_t v0, uint32_t v1, uint32_t vo) {
		acc = acc + (W)cm::parallelogram<T>(value(v0), value(v1), value(vo), q);
		++n;
	});
	if (n == 0) return T(0);
	T avg = (T)cm::mean_of(acc, (W)n);
	if constexpr (!cm::is_fp<T>::value) return avg;
	else {
		T best = 3.402823466e+38f;   // numeric_limits<float>::max()
		fan_candidates(tp, rank, e, my_rank, lo, [&](uint32_t v0, uint32_t v1, uint32_t vo) {
			T p = cm::parallelogram<T>(value(v0), value(v1), value(vo), q);
			T db = avg > best ? avg - best : best - avg;
			T dp = avg > p ? avg - p : p - avg;
			best = db < dp ? best : p;
		});
		return best;
	}
}

// the same from nc <= kEncCand kept candidates.  kept(s): the value at kept vertex s = 3 * candidate + corner, as a T; s is a
// compile-time index once the loops are unrolled, so kept may read a register array
template <typename T, typename K>
__device__ __forceinline__ T predict_kept(int nc, int q, K &&kept)
{
	typedef typename cm::wide<T>::type W;
	if (nc == 0) return T(0);
	T p[kEncCand];
	W acc = 0;
#pragma unroll
	for (int i = 0; i < kEncCand; ++i)
		if (i < nc) {
			p[i] = cm::parallelogram<T>(kept(3 * i), kept(3 * i + 1), kept(3 * i + 2), q);
			acc = acc + (W)p[i];   // fan order (the float mean is a double sum in candidate order)
		}
	const T avg = (T)cm::mean_of(acc, (W)nc);
	if constexpr (!cm::is_fp<T>::value) return avg;
	else {
		T best = 3.402823466e+38f;   // numeric_limits<float>::max()
#pragma unroll
		for (int i = 0; i < kEncCand; ++i)
			if (i < nc) {
				T db = avg > best ? avg - best : best - avg;
				T dp = avg > p[i] ? avg - p[i] : p[i] - avg;
				best = db < dp ? best : p[i];
			}
		return best;
	}
}

}   // namespace dev
}   // namespace hry
