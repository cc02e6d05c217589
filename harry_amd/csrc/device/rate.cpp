// The coded size of the vertex attributes at every quantisation width (include/harry_amd.h: hry_rate_sweep_build; kernel:
// rate.hip): the byte-plane histograms of the residual codes hry_encode would write after a requant to each width,
// and the choice of a width from a byte budget on their entropies (host only).  The front half is the encoder's own: the mesh is
// made resident, walked by the plain cut-border walk, the coding order and the repaired twins go up and k_rank ranks the vertices
// (upload_coding_order / rank_coding_order, codec.cpp); then one kernel in place of k_predict_vtx.  The table lives in d_sweep.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "context.hpp"
#include "kernels.hpp"

namespace hry {

using namespace dev;

namespace {

constexpr size_t kRowWords = (size_t)kRatePlanes * 256;

const RateResult::Comp &rate_comp(const RateResult &s, int l, int c)
{
	if (l < 0 || (size_t)l >= s.comp.size()) throw Error(HRY_E_ARG, "Invalid list index");
	if (c < 0 || (size_t)c >= s.comp[l].size()) throw Error(HRY_E_ARG, "Invalid attribute index");
	return s.comp[l][c];
}
std::string not_swept(int l, int c, const std::string &why) { return "list " + std::to_string(l) + " attr " + std::to_string(c) + " was not swept: " + why; }

}   // namespace

void rate_sweep_build(Context &cx, Mesh &m, RateResult &out)
{
	if (m.partial) throw Error(HRY_E_ARG, "partially decoded mesh (a share of a sharded container): only its runs are real");
	if (m.general) throw Error(HRY_E_UNSUPPORTED, "general bindings: the rate sweep reads the PLY layout, one record per vertex");
	if (m.shard.active() || !m.shard.seeds.empty()) throw Error(HRY_E_UNSUPPORTED, "a shard of a larger mesh: the rate sweep walks a whole mesh");
	// what of the mesh as it stands hry_encode refuses: a lossless double only costs its component the row 0, anything else the build
	std::string no_double;
	try { check_codable(m); }
	catch (const Error &e) {
		bool dbl = false;
		for (const AttrList &L : m.lists) for (int c = 0; c < L.ncomp(); ++c) dbl = dbl || L.stype(c) == C_DOUBLE;
		if (!dbl) throw;
		no_double = e.what();
	}
	if (m.lists.size() < 2 || m.lists[0].count != m.nf || m.lists[1].count != m.nv) throw Error(HRY_E_UNSUPPORTED, "attribute lists must have one record per element");
	const AttrList &L = m.lists[1];
	if (L.ncomp() > dev::kMaxComp) throw Error(HRY_E_UNSUPPORTED, "more than 32 components in a list");
	if (L.data.size() < (size_t)L.count * L.stride()) throw Error(HRY_E_ARG, "list without its records");
	HIP_OK(hipSetDevice(cx.device));
	for (size_t l = 0; l < m.lists.size(); ++l) if (!m.lists[l].have_bounds && m.lists[l].ncomp()) { device_bounds(cx, m); break; }
	out.uploaded_bytes = 0;
	if (m.device_token == 0 || m.device_token != cx.resident_token) {
		for (const AttrList &A : m.lists) out.uploaded_bytes += A.data.size();
		out.uploaded_bytes += (uint64_t)m.ne() * 4 * (m.twins_pending ? 1 : 2) + ((uint64_t)m.nf + 1) * 4;
		cx.upload_mesh(m);
	}

	// ---- what is counted: list 1's components -- at 1 .. qmax where the error sweep sweeps them, as they stand where hry_encode codes them
	out.comp.assign(m.lists.size(), std::vector<RateResult::Comp>());
	for (size_t l = 0; l < m.lists.size(); ++l) {
		out.comp[l].resize(m.lists[l].ncomp());
		for (int c = 0; c < m.lists[l].ncomp(); ++c) {
			RateResult::Comp &C = out.comp[l][c];
			C.type = m.lists[l].type[c];
			if (l != 1) C.why = C.why0 = "list " + std::to_string(l) + " is not swept: only list 1, the vertex list, is";
		}
	}
	RateList J{};
	std::vector<int> job_of(L.ncomp(), -1);
	uint32_t rows = 0;
	for (int c = 0; c < L.ncomp(); ++c) {
		RateResult::Comp &C = out.comp[1][c];
		RequantComp rc{};
		C.qmax = swept_widths(m, 1, c, rc, C.why);
		C.row0 = L.stype(c) != C_DOUBLE;
		if (!C.row0) C.why0 = no_double;
		else C.planes0 = kTypeSize[L.stype(c)];
		if (!C.qmax && !C.row0) continue;
		RateComp &rj = J.c[J.n];
		rj = RateComp{};
		rj.rc = rc;
		if (!C.qmax) { rj.rc.off = L.offset[c]; rj.rc.src_type = rj.rc.dst_type = L.type[c]; }
		rj.qmax = C.qmax; rj.row0 = C.row0 ? 1 : 0; rj.slot = rows;
		rj.stype0 = (uint8_t)L.stype(c); rj.quant0 = L.quant[c];
		rows += (uint32_t)C.qmax + 2;
		job_of[c] = J.n++;
	}

	// ---- the encoder's front half: walk, coding order and repaired twins up, ranks
	auto t_walk = Clock::now();
	WalkResult w;
	if (m.nf) cut_border_walk(m, w, false);   // (a mesh without faces codes no vertex: the walk refuses it, the table is all zero)
	out.walk_ms = ms_since(t_walk);
	const uint32_t vc = (uint32_t)w.order_v.size();
	out.coded = vc;
	out.device_ms = 0;
	upload_coding_order(cx, m, w);
	rank_coding_order(cx, m, vc);

	// ---- the table
	const size_t tab_bytes = (size_t)rows * kRowWords * 4;
	std::vector<uint32_t> tab((size_t)rows * kRowWords, 0);
	if (rows && vc) {
		cx.d_sweep.ensure(tab_bytes);
		hipStream_t st = cx.stream;
		HIP_OK(hipMemsetAsync(cx.d_sweep.p, 0, tab_bytes, st));
		J.rec = cx.d_rec[1].as<uint8_t>();
		J.table = cx.d_sweep.as<uint32_t>();
		J.stride = (uint32_t)L.stride();
		TimedEvent ev[2];
		HIP_OK(hipEventRecord(ev[0], st));
		launch_rate_sweep(st, cx.conn_view(), cx.d_order_v.as<uint32_t>(), vc, cx.d_rank.as<uint32_t>(), J);
		HIP_OK(hipGetLastError());
		HIP_OK(hipEventRecord(ev[1], st));
		HIP_OK(hipMemcpyAsync(tab.data(), cx.d_sweep.p, tab_bytes, hipMemcpyDeviceToHost, st));
		HIP_OK(hipStreamSynchronize(st));
		float ms = 0;
		HIP_OK(hipEventElapsedTime(&ms, ev[0], ev[1]));
		out.device_ms = (double)ms;
	} else HIP_OK(hipStreamSynchronize(cx.stream));
	for (int c = 0; c < L.ncomp(); ++c) {
		if (job_of[c] < 0) continue;
		RateResult::Comp &C = out.comp[1][c];
		const uint32_t *from = tab.data() + (size_t)J.c[job_of[c]].slot * kRowWords;
		C.hist.assign(from, from + ((size_t)C.qmax + 2) * kRowWords);
	}
}

const uint32_t *rate_row(const RateResult::Comp &C, int bits) { return C.hist.data() + (bits ? (size_t)bits + 1 : 0) * kRowWords; }

double rate_hist_bytes(const uint32_t *hist)
{
	uint64_t n = 0;
	for (int s = 0; s < 256; ++s) n += hist[s];
	if (!n) return 0.0;
	double bits = 0.0;
	for (int s = 0; s < 256; ++s) if (hist[s]) bits += (double)hist[s] * std::log2((double)n / (double)hist[s]);
	return bits / 8.0;
}

int rate_planes(const RateResult &s, int l, int c, int bits)
{
	const RateResult::Comp &C = rate_comp(s, l, c);
	if (bits == 0) {
		if (!C.row0) throw Error(HRY_E_UNSUPPORTED, C.why0);
		return C.planes0;
	}
	if (!C.qmax) throw Error(HRY_E_UNSUPPORTED, not_swept(l, c, C.why));
	if (bits < 0 || bits > C.qmax) throw Error(HRY_E_ARG, "Invalid quantization bits");
	return bits <= 8 ? 1 : bits <= 16 ? 2 : 4;
}

double rate_bytes(const RateResult &s, int l, int c, int bits)
{
	const int np = rate_planes(s, l, c, bits);
	const uint32_t *row = rate_row(s.comp[l][c], bits);
	double sum = 0.0;
	for (int p = 0; p < np; ++p) sum += rate_hist_bytes(row + (size_t)p * 256);
	return sum;
}

int rate_pick(const double *bytes_by_bits, int n_bits, double budget)
{
	if (!(budget >= 0.0)) throw Error(HRY_E_ARG, "a budget is a number of bytes that is not negative");
	if (n_bits < 0 || (n_bits && !bytes_by_bits)) throw Error(HRY_E_ARG, "no table");
	for (int q = n_bits; q >= 1; --q) if (bytes_by_bits[q - 1] <= budget) return q;
	return 0;
}

int rate_choose(const RateResult &s, int l, int c, double budget, double *bytes)
{
	if (l < 0 || (size_t)l >= s.comp.size()) throw Error(HRY_E_ARG, "Invalid list index");
	std::vector<int> comps;
	if (c == -1) { for (size_t k = 0; k < s.comp[l].size(); ++k) if (s.comp[l][k].qmax) comps.push_back((int)k); }
	else {
		const RateResult::Comp &C = rate_comp(s, l, c);
		if (!C.qmax) throw Error(HRY_E_UNSUPPORTED, not_swept(l, c, C.why));
		comps.push_back(c);
	}
	if (comps.empty()) throw Error(HRY_E_UNSUPPORTED, "list " + std::to_string(l) + " has no swept component" + (s.comp[l].empty() ? std::string() : ": " + s.comp[l][0].why));
	int qmax = s.comp[l][comps[0]].qmax;
	for (int k : comps) qmax = std::min(qmax, s.comp[l][k].qmax);
	std::vector<double> sums((size_t)qmax, 0.0);
	for (int q = 1; q <= qmax; ++q) for (int k : comps) sums[q - 1] += rate_bytes(s, l, k, q);
	const int bits = rate_pick(sums.data(), qmax, budget);
	if (bytes) *bytes = bits ? sums[bits - 1] : 0.0;
	return bits;
}

}   // namespace hry
