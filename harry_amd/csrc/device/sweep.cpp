// The error of every quantisation width of a mesh's unquantised components (include/harry_amd.h: hry_quant_sweep_build; kernels:
// sweep.hip), and the choice of widths from tolerances on that table (host only).  Residency as in distortion.cpp:
// the records of the context's resident mesh are read in place, anything else goes up into the build's own working buffer
// (d_sweep), next to the blocks' partial records and the results: neither resident_token nor render_token is read for anything but
// the test, and neither is written -- unless the mesh has no bounds yet: then they are computed as hry_requant computes them.
// With HRY_SWEEP_NORMALS the faces' normal deviation at every width of the positions rides along (normal_sweep.hip):
// the connectivity is read in d_org / d_foff of the resident mesh or goes up too, and its records come down behind the table.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "codec_math.hpp"
#include "context.hpp"
#include "kernels.hpp"

namespace hry {

using namespace dev;

namespace {

bool meets(const hry_comp_error &e, int metric, double extent, double value)
{
	switch (metric) {
	case HRY_TOL_MAX_ABS: return e.max_abs <= value;
	case HRY_TOL_MAX_REL: return e.max_abs <= value * extent;
	case HRY_TOL_RMS: return e.compared != 0 && std::sqrt(e.sum_sq / (double)e.compared) <= value;
	default: return false;
	}
}
void check_tolerance_value(double value)
{
	if (!(value >= 0.0)) throw Error(HRY_E_ARG, "a tolerance is a number that is not negative");
}

}   // namespace

// Which widths component c of list l (bounds known) is swept at: 1 .. the result, 0: none and `why` says why.  The test is
// hry_requant's own, requant_plan on that one component; rc: what it gives (offset, minimum, shared extent), the bits left to the
// kernel.  One statement for the error sweep and the rate sweep (rate.cpp)
int swept_widths(const Mesh &m, size_t l, int c, dev::RequantComp &rc, std::string &why)
{
	const AttrList &L = m.lists[l];
	if (!distortion_compares(m, l)) { why = "list " + std::to_string(l) + " is not compared (no target, or beyond the PLY layout's two lists)"; return 0; }
	if (L.quant[c]) { why = "already quantised"; return 0; }
	std::vector<uint8_t> to = L.quant;
	to[c] = 1;
	RequantPlan one;
	try { one = requant_plan(L, to); } catch (const Error &e) { why = e.what(); return 0; }
	if (one.n != 1) throw Error(HRY_E_INTERNAL, "sweep: the plan of one component");
	rc = one.c[0];
	rc.src_bits = 0; rc.dst_bits = 0; rc.src_type = rc.dst_type = L.type[c];
	return std::min(kSweepMaxBits, 8 * (int)kTypeSize[L.type[c]]);
}

void quant_sweep_build(Context &cx, Mesh &m, uint32_t flags, SweepResult &out)
{
	if (flags & ~(uint32_t)HRY_SWEEP_NORMALS) throw Error(HRY_E_ARG, "unknown sweep flag");
	const bool want_normals = (flags & HRY_SWEEP_NORMALS) != 0;
	if (m.partial) throw Error(HRY_E_ARG, "partially decoded mesh (a share of a sharded container): only its runs are real");
	if (m.lists.size() > (size_t)kMaxLists) throw Error(HRY_E_UNSUPPORTED, "more than 16 attribute lists");
	const size_t nl = m.lists.size();
	for (size_t l = 0; l < nl; ++l) {
		const AttrList &L = m.lists[l];
		if (!distortion_compares(m, l)) continue;
		if (L.ncomp() > dev::kMaxComp) throw Error(HRY_E_UNSUPPORTED, "more than 32 components in a list");
		if (L.data.size() < (size_t)L.count * L.stride()) throw Error(HRY_E_ARG, "list without its records");
	}
	HIP_OK(hipSetDevice(cx.device));
	for (size_t l = 0; l < nl; ++l) if (!m.lists[l].have_bounds && m.lists[l].ncomp()) { device_bounds(cx, m); break; }

	// ---- what is swept: the unquantised components requant_plan accepts, at 1 .. min(30, the type's bits)
	out.comp.assign(nl, std::vector<SweepResult::Comp>());
	std::vector<SweepList> jobs(nl);
	std::vector<std::vector<int>> job_of(nl);
	for (size_t l = 0; l < nl; ++l) {
		const AttrList &L = m.lists[l];
		out.comp[l].resize(L.ncomp());
		job_of[l].assign(L.ncomp(), -1);
		SweepList &J = jobs[l];
		J = SweepList{};
		J.pos = -1;
		for (int c = 0; c < L.ncomp(); ++c) {
			SweepResult::Comp &C = out.comp[l][c];
			C.type = L.type[c];
			RequantComp rc;
			C.qmax = swept_widths(m, l, c, rc, C.why);
			if (!C.qmax) continue;
			C.extent = cm::value_f64(rc.scale, (int)L.type[c]);
			SweepComp &sc = J.c[J.n];
			sc.rc = rc;
			sc.qmax = C.qmax; sc.slot = J.ns;
			J.ns += (uint32_t)C.qmax;
			job_of[l][c] = J.n++;
		}
	}
	const int pl = distortion_position_list(m);
	out.pos_list = -1; out.pos_comp = -1; out.pos.clear();
	if (pl >= 0) {
		const int pc = m.lists[pl].interp_off[0];
		if (pc < 0 || pc + 3 > m.lists[pl].ncomp()) throw Error(HRY_E_INTERNAL, "position components outside their list");
		const std::vector<SweepResult::Comp> &C = out.comp[pl];
		if (C[pc].qmax && C[pc + 1].qmax && C[pc + 2].qmax) {   // (consecutive components, all swept: consecutive jobs)
			SweepList &J = jobs[pl];
			J.pos = job_of[pl][pc];
			J.pos_qmax = std::min(C[pc].qmax, std::min(C[pc + 1].qmax, C[pc + 2].qmax));
			J.pos_slot = J.ns;
			J.ns += (uint32_t)J.pos_qmax;
		}
		out.pos_list = pl; out.pos_comp = pc;
	}
	// ---- the faces' normal deviation at every width of the positions (HRY_SWEEP_NORMALS; normal_sweep.hip)
	out.nrm_asked = want_normals; out.nrm.clear(); out.nrm_why.clear();
	int nrm_qmax = 0;
	if (want_normals) {
		if (pl < 0 || jobs[pl].pos < 0) out.nrm_why = "the positions were not swept: their three components are not all swept";
		else if (normals_comparable(m, out.nrm_why)) nrm_qmax = jobs[pl].pos_qmax;
	}
	const uint32_t nf = m.nf, ne = m.ne();
	const bool tri = nrm_qmax && all_triangles(m);

	// ---- where the records are read: the resident mesh's, or uploads (d_rec holds one mesh at a time)
	bool res = cx.render_token == 0 && m.device_token != 0 && m.device_token == cx.resident_token;
	for (size_t l = 0; l < nl && res; ++l) res = !jobs[l].ns || cx.d_rec[l].cap >= m.lists[l].data.size();
	if (nrm_qmax && res) res = cx.res_nf == nf && cx.res_ne == ne && cx.d_org.cap >= (size_t)ne * 4 && (tri || cx.d_foff.cap >= ((size_t)nf + 1) * 4);
	Carve W;
	size_t ns_all = 0;
	std::vector<size_t> slot_at(nl, 0);
	std::vector<uint8_t*> up_rec(nl, nullptr);   // where a list's records go up, unless the mesh is resident (the vectors keep their size)
	std::vector<DistPart*> part(nl, nullptr);
	uint32_t *up_org, *up_foff;
	uint8_t *d_res;
	for (size_t l = 0; l < nl; ++l) {
		if (!jobs[l].ns) continue;
		slot_at[l] = ns_all;
		ns_all += jobs[l].ns;
		W.take(up_rec[l], res ? 0 : m.lists[l].data.size());
		W.take(part[l], (size_t)distortion_blocks(m.lists[l].count) * jobs[l].ns * sizeof(DistPart));
	}
	out.device_ms = 0; out.uploaded_bytes = 0;
	if (!ns_all) return;
	NormPart *npart;
	W.take(up_org, nrm_qmax && !res ? (size_t)ne * 4 : 0); W.take(up_foff, nrm_qmax && !res && !tri ? ((size_t)nf + 1) * 4 : 0);
	W.take(npart, nrm_qmax ?(size_t)distortion_blocks(nf) * nrm_qmax * sizeof(NormPart) : 0);
	VertexRows vrows;
	if (nrm_qmax) vrows.reserve(cx, m, pl, res, W);
	static_assert(sizeof(DistFinal) % 8 == 0 && sizeof(NormFinal) == sizeof(hry_normal_error) && sizeof(NormFinal) == 64, "the normals' records follow the table");
	const size_t dist_bytes = ns_all * sizeof(DistFinal), res_bytes = dist_bytes + (size_t)nrm_qmax * sizeof(NormFinal);   // one copy brings both down
	W.take(d_res, res_bytes);
	cx.d_sweep.ensure(W.total);
	void *wb = cx.d_sweep.p;
	W.bind(wb);

	hipStream_t st = cx.stream;
	uint64_t up = 0;
	DistFold fold{};
	for (size_t l = 0; l < nl; ++l) {
		SweepList &J = jobs[l];
		if (!J.ns) continue;
		const AttrList &L = m.lists[l];
		if (res) J.rec = cx.d_rec[l].as<uint8_t>();
		else {
			if (!L.data.empty()) HIP_OK(hipMemcpyAsync(up_rec[l], L.data.data(), L.data.size(), hipMemcpyHostToDevice, st));
			up += L.data.size();
			J.rec = up_rec[l];
		}
		J.part = part[l];
		J.rows = L.count; J.stride = (uint32_t)L.stride();
		const int k = fold.n++;
		fold.part[k] = J.part; fold.nblocks[k] = distortion_blocks(L.count); fold.nslots[k] = J.ns; fold.out_at[k] = (uint32_t)slot_at[l];
	}
	NormalSweep N{};
	if (nrm_qmax) {
		const SweepList &J = jobs[pl];
		if (res) { N.F.org = cx.d_org.as<uint32_t>(); N.F.foff = tri ? nullptr : cx.d_foff.as<uint32_t>(); }
		else {
			HIP_OK(hipMemcpyAsync(up_org, m.org.data(), (size_t)ne * 4, hipMemcpyHostToDevice, st));
			up += (size_t)ne * 4;
			N.F.org = up_org;
			if (!tri) {
				HIP_OK(hipMemcpyAsync(up_foff, m.face_off.data(), ((size_t)nf + 1) * 4, hipMemcpyHostToDevice, st));
				up += ((size_t)nf + 1) * 4;
				N.F.foff = up_foff;
			}
		}
		N.F.rows = nullptr; N.F.nf = nf; N.F.ne = ne; N.F.nv = m.general ? m.nv : J.rows; N.F.nrows = J.rows;
		N.rec = J.rec; N.part = npart; N.stride = J.stride; N.qmax = nrm_qmax;
		for (int a = 0; a < 3; ++a) N.c[a] = J.c[J.pos + a].rc;
		N.type = N.c[0].dst_type == N.c[1].dst_type && N.c[1].dst_type == N.c[2].dst_type ? N.c[0].dst_type : -1;
	}
	TimedEvent ev[2];
	HIP_OK(hipEventRecord(ev[0], st));
	for (size_t l = 0; l < nl; ++l) if (jobs[l].ns) launch_quant_sweep(st, jobs[l]);
	launch_quant_sweep_fold(st, fold, (DistFinal*)d_res);
	if (nrm_qmax) {
		N.F.rows = vrows.launch(cx, m, pl, W, wb, up);
		launch_normal_sweep(st, N);
		launch_normal_fold(st, N.part, distortion_blocks(nf), (uint32_t)nrm_qmax, (NormFinal*)(d_res + dist_bytes));
	}
	HIP_OK(hipGetLastError());
	HIP_OK(hipEventRecord(ev[1], st));
	std::vector<uint8_t> tab(res_bytes);
	HIP_OK(hipMemcpyAsync(tab.data(), d_res, res_bytes, hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	float ms = 0;
	HIP_OK(hipEventElapsedTime(&ms, ev[0], ev[1]));

	auto record = [&](size_t l, uint32_t slot) { DistFinal f; memcpy(&f, tab.data() + (slot_at[l] + slot) * sizeof(DistFinal), sizeof f); return f; };
	for (size_t l = 0; l < nl; ++l) {
		const SweepList &J = jobs[l];
		if (!J.ns) continue;
		for (int c = 0; c < m.lists[l].ncomp(); ++c) {
			if (job_of[l][c] < 0) continue;
			SweepResult::Comp &C = out.comp[l][c];
			C.by_bits.resize(C.qmax);
			for (int q = 1; q <= C.qmax; ++q) {
				const DistFinal f = record(l, J.c[job_of[l][c]].slot + (uint32_t)(q - 1));
				hry_comp_error &e = C.by_bits[q - 1];
				e.max_abs = f.mx; e.sum_sq = f.sum; e.a_min = f.mn; e.a_max = f.mxa;
				e.compared = f.compared; e.skipped = 0; e.nonfinite = f.nonfinite; e.changed = f.changed;
				e.argmax = f.row; e.reserved = 0;
			}
		}
		if (J.pos >= 0) {
			out.pos.resize(J.pos_qmax);
			for (int q = 1; q <= J.pos_qmax; ++q) {
				const DistFinal f = record(l, J.pos_slot + (uint32_t)(q - 1));
				out.pos[q - 1] = hry_pos_error{ f.mx, f.sum, f.compared, f.row, (int32_t)l };
			}
		}
	}
	if (nrm_qmax) {
		out.nrm.resize(nrm_qmax);
		memcpy(out.nrm.data(), tab.data() + dist_bytes, (size_t)nrm_qmax * sizeof(hry_normal_error));
		for (hry_normal_error &e : out.nrm) e.list = pl;
	}
	out.device_ms = (double)ms;
	out.uploaded_bytes = up;
}

int quant_pick(const hry_comp_error *by_bits, int n_bits, int metric, double extent, double value)
{
	check_tolerance_value(value);
	if (metric != HRY_TOL_MAX_ABS && metric != HRY_TOL_MAX_REL && metric != HRY_TOL_RMS) throw Error(HRY_E_ARG, "a component's tolerance is HRY_TOL_MAX_ABS, HRY_TOL_MAX_REL or HRY_TOL_RMS");
	if (n_bits < 0 || (n_bits && !by_bits)) throw Error(HRY_E_ARG, "no table");
	for (int q = 1; q <= n_bits; ++q) if (meets(by_bits[q - 1], metric, extent, value)) return q;
	return 0;
}

std::vector<hry_quant> quant_choose(const SweepResult &s, const hry_tolerance *t, size_t nt)
{
	struct Want { int l, c; std::vector<const hry_tolerance*> tol; };
	std::vector<Want> wants;   // in the order the tolerances first name a component
	auto want = [&](int l, int c, const hry_tolerance *tol) {
		for (Want &w : wants) if (w.l == l && w.c == c) { w.tol.push_back(tol); return; }
		wants.push_back(Want{ l, c, { tol } });
	};
	for (size_t i = 0; i < nt; ++i) {
		const hry_tolerance &T = t[i];
		check_tolerance_value(T.value);
		if (T.metric < HRY_TOL_MAX_ABS || T.metric > HRY_TOL_NORMAL_CHORD) throw Error(HRY_E_ARG, "unknown tolerance metric");
		if (T.list < 0 || (size_t)T.list >= s.comp.size()) throw Error(HRY_E_ARG, "Invalid list index");
		const std::vector<SweepResult::Comp> &C = s.comp[T.list];
		if (T.metric == HRY_TOL_POS_DIST) {
			if (T.comp != -1) throw Error(HRY_E_ARG, "HRY_TOL_POS_DIST names the position list with comp -1");
			if (T.list != s.pos_list) throw Error(HRY_E_ARG, "list " + std::to_string(T.list) + " is not the position list");
			if (s.pos.empty()) throw Error(HRY_E_UNSUPPORTED, "the positions were not swept: their three components are not all swept");
			for (int a = 0; a < 3; ++a) want(T.list, s.pos_comp + a, &T);
			continue;
		}
		if (T.metric == HRY_TOL_NORMAL_CHORD) {
			if (T.comp != -1) throw Error(HRY_E_ARG, "HRY_TOL_NORMAL_CHORD names the position list with comp -1");
			if (T.list != s.pos_list) throw Error(HRY_E_ARG, "list " + std::to_string(T.list) + " is not the position list");
			if (!s.nrm_asked) throw Error(HRY_E_UNSUPPORTED, "the normals were not swept: the sweep was built without HRY_SWEEP_NORMALS");
			if (s.nrm.empty()) throw Error(HRY_E_UNSUPPORTED, "the normals were not swept: " + s.nrm_why);
			for (int a = 0; a < 3; ++a) want(T.list, s.pos_comp + a, &T);
			continue;
		}
		if (T.comp == -1) {
			for (size_t c = 0; c < C.size(); ++c) if (C[c].qmax) want(T.list, (int)c, &T);
			continue;
		}
		if (T.comp < 0 || (size_t)T.comp >= C.size()) throw Error(HRY_E_ARG, "Invalid attribute index");
		if (!C[T.comp].qmax) throw Error(HRY_E_UNSUPPORTED, "list " + std::to_string(T.list) + " attr " + std::to_string(T.comp) + " was not swept: " + C[T.comp].why);
		want(T.list, T.comp, &T);
	}
	std::vector<hry_quant> out;
	for (const Want &w : wants) {
		const SweepResult::Comp &C = s.comp[w.l][w.c];
		int bits = 0;
		for (int q = 1; q <= C.qmax && !bits; ++q) {   // the smallest width that meets every tolerance on the component
			bool ok = true;
			for (const hry_tolerance *T : w.tol)
				ok = ok && (T->metric == HRY_TOL_POS_DIST ? q <= (int)s.pos.size() && s.pos[q - 1].max_dist <= T->value
				            : T->metric == HRY_TOL_NORMAL_CHORD ? q <= (int)s.nrm.size() && s.nrm[q - 1].max_chord <= T->value && s.nrm[q - 1].collapsed == 0
				                                                : meets(C.by_bits[q - 1], T->metric, C.extent, T->value));
			if (ok) bits = q;
		}
		if (!bits && C.type == C_DOUBLE)
			throw Error(HRY_E_UNSUPPORTED, "list " + std::to_string(w.l) + " attr " + std::to_string(w.c) + ": no width meets the tolerance, and a double cannot stay lossless");
		out.push_back(hry_quant{ w.l, w.c, bits });
	}
	return out;
}

}   // namespace hry
