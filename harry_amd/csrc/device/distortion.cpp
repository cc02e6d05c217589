// Per-component error of one mesh against another (include/harry_amd.h: hry_distortion_build; kernels: distortion.hip; DESIGN.md
// 7d).  Everything the comparison reads is usually in HBM already: the records a decode left (d_rec, under the token hry_render_build
// tests), the records of the context's resident mesh, and the numbering maps of the encode (a handle of their own).  What is not
// goes up into the build's own working buffer (d_distortion), next to the blocks' partial records, the results and the status word:
// neither the encoder's resident_token nor the decode's render_token is read for anything but the test, and neither is written.
// With HRY_DISTORTION_NORMALS the faces' normal deviation is taken over a's faces as well (normal_sweep.hip): a's
// connectivity is read in d_org / d_foff when a is the resident mesh, otherwise it goes up with the records.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "context.hpp"
#include "kernels.hpp"

namespace hry {

using namespace dev;

namespace {

bool compared(const Mesh &m, size_t l) { return m.lists[l].ncomp() > 0 && m.lists[l].target <= 2 && (m.general || l < 2); }
int npos(const AttrList &L) { return L.interp_len.empty() ? 0 : L.interp_len[0]; }

// the list whose first three POS components (mixing.h interpretation 0) are the positions, or -1
int position_list(const Mesh &m)
{
	if (!m.general) return m.lists.size() >= 2 && compared(m, 1) && npos(m.lists[1]) >= 3 ? 1 : -1;
	for (size_t l = 0; l < m.lists.size(); ++l)
		if (m.lists[l].target == 1 && compared(m, l) && npos(m.lists[l]) >= 3) return (int)l;
	return -1;
}

}   // namespace

bool distortion_compares(const Mesh &m, size_t l) { return compared(m, l); }
int distortion_position_list(const Mesh &m) { return position_list(m); }

bool normals_comparable(const Mesh &m, std::string &why)
{
	if (position_list(m) < 0) { why = "normals: no vertex list with three position components"; return false; }
	if (!m.nf) { why = "normals: the mesh has no faces"; return false; }
	if (m.face_off.size() != (size_t)m.nf + 1 || m.org.size() < m.ne()) { why = "normals: mesh without its connectivity"; return false; }
	if (m.general) {
		const Bindings &b = m.bind;
		const int pl = position_list(m);
		for (int r = 0; r < b.nregs_vtx(); ++r) {
			bool bound = false;
			for (int a = 0; a < b.nvtxlists(r); ++a) bound |= b.vtxlist(r, a) == pl;
			if (!bound) { why = "normals: a vertex region that does not bind the position list"; return false; }
		}
		if (b.vtx_reg.size() < m.nv || b.vtx_attr.size() < (size_t)m.nv * b.nb_vtx) { why = "normals: mesh without its binding tables"; return false; }
	}
	return true;
}
void VertexRows::reserve(const Context &cx, const Mesh &m, int pl, bool tables_there, Carve &W)
{
	general = m.general;
	if (!general) return;
	const Bindings &b = m.bind;
	slot.assign((size_t)std::max(b.nregs_vtx(), 1), -1);
	for (int r = 0; r < b.nregs_vtx(); ++r)
		for (int a = 0; a < b.nvtxlists(r); ++a) if (b.vtxlist(r, a) == pl) slot[r] = a;
	in_place = tables_there && cx.gen_token != 0 && cx.gen_token == m.device_token && cx.d_vreg.cap >= (size_t)m.nv * 2 && cx.d_vattr.cap >= (size_t)m.nv * b.nb_vtx * 4;
	w_slot = W.reserve(slot.size() * 4);
	w_vreg = W.reserve(in_place ? 0 : (size_t)m.nv * 2);
	w_vattr = W.reserve(in_place ? 0 : (size_t)m.nv * b.nb_vtx * 4);
	w_idx = W.reserve((size_t)m.nv * 4);
}
const uint32_t *VertexRows::launch(Context &cx, const Mesh &m, int pl, const Carve &W, void *wb, uint64_t &uploaded) const
{
	if (!general) return nullptr;
	const Bindings &b = m.bind;
	hipStream_t st = cx.stream;
	HIP_OK(hipMemcpyAsync(W.ptr<uint8_t>(wb, w_slot), slot.data(), slot.size() * 4, hipMemcpyHostToDevice, st));
	RowsView v{};
	v.slot = W.ptr<int32_t>(wb, w_slot); v.count = m.lists[pl].count;
	v.nowner = m.nv; v.nregs = (uint32_t)b.nregs_vtx(); v.nb = (uint32_t)b.nb_vtx; v.nelem = m.nv;
	if (in_place) { v.reg = cx.d_vreg.as<uint16_t>(); v.attr = cx.d_vattr.as<uint32_t>(); }
	else {
		HIP_OK(hipMemcpyAsync(W.ptr<uint8_t>(wb, w_vreg), b.vtx_reg.data(), (size_t)m.nv * 2, hipMemcpyHostToDevice, st));
		HIP_OK(hipMemcpyAsync(W.ptr<uint8_t>(wb, w_vattr), b.vtx_attr.data(), (size_t)m.nv * b.nb_vtx * 4, hipMemcpyHostToDevice, st));
		uploaded += (uint64_t)m.nv * 2 + (uint64_t)m.nv * b.nb_vtx * 4;
		v.reg = W.ptr<uint16_t>(wb, w_vreg); v.attr = W.ptr<uint32_t>(wb, w_vattr);
	}
	uint32_t *idx = W.ptr<uint32_t>(wb, w_idx);
	launch_rows_of(st, v, m.nv, idx);
	return idx;
}
bool all_triangles(const Mesh &m)
{
	bool tri = (uint64_t)m.ne() == 3ull * m.nf;
	for (size_t d = 4; d < m.have_degree.size(); ++d) tri = tri && !m.have_degree[d];
	return tri;
}

void distortion_build(Context &cx, const Mesh &a, const Mesh &b, const OrderResult *o, uint32_t flags, DistortionResult &out)
{
	if (flags & ~(uint32_t)(HRY_DISTORTION_ROWS | HRY_DISTORTION_NORMALS)) throw Error(HRY_E_ARG, "unknown distortion flag");
	const bool want_rows = (flags & HRY_DISTORTION_ROWS) != 0;
	if (a.partial || b.partial) throw Error(HRY_E_ARG, "partially decoded mesh (a share of a sharded container): only its runs are real");
	if (a.lists.size() != b.lists.size()) throw Error(HRY_E_ARG, "the meshes have different numbers of lists");
	if (a.lists.size() > (size_t)kMaxLists) throw Error(HRY_E_UNSUPPORTED, "more than 16 attribute lists");
	if (a.general != b.general) throw Error(HRY_E_ARG, "one mesh has the PLY layout, the other general bindings");
	const size_t nl = a.lists.size();
	const bool general = a.general;
	std::vector<RequantPlan> pa(nl), pb(nl);
	for (size_t l = 0; l < nl; ++l) {
		const AttrList &A = a.lists[l], &B = b.lists[l];
		if (A.target != B.target || A.ncomp() != B.ncomp() || A.type != B.type)
			throw Error(HRY_E_ARG, "list " + std::to_string(l) + ": the meshes differ in target, component count or component types");
		if (!compared(a, l)) continue;
		pa[l] = dequant_plan(A);
		pb[l] = dequant_plan(B);
		if (A.data.size() < (size_t)A.count * A.stride() || B.data.size() < (size_t)B.count * B.stride()) throw Error(HRY_E_ARG, "list without its records");
	}
	// ---- the maps
	std::vector<const uint32_t*> map(nl, nullptr);
	if (o && o->block.device != cx.device) throw Error(HRY_E_ARG, "the numbering maps live on another device than the context's");
	for (size_t l = 0; l < nl; ++l) {
		if (!compared(a, l)) continue;
		if (!o) {
			if (a.lists[l].count != b.lists[l].count) throw Error(HRY_E_ARG, "list " + std::to_string(l) + ": different counts and no order to pair the rows");
			continue;
		}
		const NamedBuf *m = o->find(general ? "list" + std::to_string(l) : l == 1 ? "vertex" : "face");
		if (!m || m->rows != a.lists[l].count) throw Error(HRY_E_ARG, "order does not fit the meshes");
		map[l] = (const uint32_t*)m->p;
	}
	const int pl = position_list(a);
	int pos_comp = -1;
	if (pl >= 0) {
		pos_comp = a.lists[pl].interp_off[0];
		if (pos_comp < 0 || pos_comp + 3 > a.lists[pl].ncomp()) throw Error(HRY_E_INTERNAL, "position components outside their list");
	}

	// ---- the faces' normal deviation (HRY_DISTORTION_NORMALS; normal_sweep.hip): a's faces, a's positions against b's at the mapped rows
	out.nrm = hry_normal_error{ 0, 0, 0, 0, 0, 0, 0, 0, -1 };
	bool want_normals = false;
	if (flags & HRY_DISTORTION_NORMALS) want_normals = normals_comparable(a, out.nrm_why);
	const uint32_t nf = a.nf, ne = a.ne();
	const bool tri = want_normals && all_triangles(a);

	HIP_OK(hipSetDevice(cx.device));
	// ---- where the records are read: the decode's buffers (holds_decode), the resident mesh's, or uploads
	bool b_res = holds_decode(cx, b);
	for (size_t l = 0; l < nl && b_res; ++l) b_res = !compared(b, l) || decoded_records(cx, l).cap >= b.lists[l].data.size();
	bool a_res = !b_res && cx.render_token == 0 && a.device_token != 0 && a.device_token == cx.resident_token;   // (d_rec holds one mesh at a time)
	for (size_t l = 0; l < nl && a_res; ++l) a_res = !compared(a, l) || cx.d_rec[l].cap >= a.lists[l].data.size();
	// (a's connectivity lies in d_org / d_foff when a is the resident mesh)
	const bool conn_res = want_normals && a_res && cx.res_nf == nf && cx.res_ne == ne && cx.d_org.cap >= (size_t)ne * 4 && (tri || cx.d_foff.cap >= ((size_t)nf + 1) * 4);

	Carve W;
	size_t nslots_all = 0;
	std::vector<size_t> slot_at(nl, 0), nslots(nl, 0);
	uint8_t *up_a[kMaxLists] = {}, *up_b[kMaxLists] = {}, *d_res;   // up_*: where a list's records go up, unless they are resident
	DistPart *part[kMaxLists] = {};
	uint32_t *up_org, *up_foff;
	NormPart *npart;
	for (size_t l = 0; l < nl; ++l) {
		if (!compared(a, l)) continue;
		nslots[l] = (size_t)a.lists[l].ncomp() + ((int)l == pl ? 1 : 0);
		slot_at[l] = nslots_all;
		nslots_all += nslots[l];
		W.take(up_a[l], a_res ? 0 : a.lists[l].data.size());
		W.take(up_b[l], b_res ? 0 : b.lists[l].data.size());
		W.take(part[l], (size_t)distortion_blocks(a.lists[l].count) * nslots[l] * sizeof(DistPart));
	}
	W.take(up_org, want_normals && !conn_res ? (size_t)ne * 4 : 0); W.take(up_foff, want_normals && !conn_res && !tri ? ((size_t)nf + 1) * 4 : 0);
	W.take(npart, want_normals ? (size_t)distortion_blocks(nf) * sizeof(NormPart) : 0);
	VertexRows vrows;
	if (want_normals) vrows.reserve(cx, a, pl, a_res, W);
	const size_t res_bytes = nslots_all * sizeof(DistFinal);
	static_assert(sizeof(NormFinal) == sizeof(hry_normal_error) && sizeof(NormFinal) == 64, "the normals' record is an hry_normal_error");
	W.take(d_res, res_bytes + 8 + (want_normals ? sizeof(NormFinal) : 0));   // the results, the status word, the normals' record: one copy brings all down
	cx.d_distortion.ensure(W.total);
	void *wb = cx.d_distortion.p;
	W.bind(wb);

	Carve O;
	std::vector<size_t> o_err(nl, 0);
	if (want_rows) for (size_t l = 0; l < nl; ++l) if (compared(a, l)) o_err[l] = O.reserve((size_t)a.lists[l].count * 4);
	const size_t o_nerr = O.reserve(want_rows && want_normals ? (size_t)nf * 4 : 0);
	out.block.alloc(cx.device, std::max<size_t>(O.total, 16));   // (without HRY_DISTORTION_ROWS there is no piece)

	hipStream_t st = cx.stream;
	uint64_t up = 0;
	auto put = [&](void *piece, const void *src, size_t bytes) {
		if (!bytes) return;
		HIP_OK(hipMemcpyAsync(piece, src, bytes, hipMemcpyHostToDevice, st));
		up += bytes;
	};
	uint32_t *d_status = (uint32_t*)(d_res + res_bytes);
	HIP_OK(hipMemsetAsync(d_status, 0, 8, st));
	DistFold fold{};
	std::vector<DistList> jobs;
	std::vector<size_t> job_list;
	for (size_t l = 0; l < nl; ++l) {
		if (!compared(a, l)) continue;
		const AttrList &A = a.lists[l], &B = b.lists[l];
		DistList J{};
		if (a_res) J.a = cx.d_rec[l].as<uint8_t>(); else { put(up_a[l], A.data.data(), A.data.size()); J.a = up_a[l]; }
		if (b_res) J.b = decoded_records(cx, l).as<uint8_t>(); else { put(up_b[l], B.data.data(), B.data.size()); J.b = up_b[l]; }
		J.map = map[l];
		J.err = want_rows ? O.ptr<float>(out.block.p, o_err[l]) : nullptr;
		J.part = part[l];
		J.rows = A.count; J.b_rows = B.count; J.sa = (uint32_t)A.stride(); J.sb = (uint32_t)B.stride();
		J.pos = (int)l == pl ? pos_comp : -1;
		jobs.push_back(J);
		job_list.push_back(l);
		const int k = fold.n++;
		fold.part[k] = J.part; fold.nblocks[k] = distortion_blocks(A.count); fold.nslots[k] = (uint32_t)nslots[l]; fold.out_at[k] = (uint32_t)slot_at[l];
	}

	NormalPair N{};
	if (want_normals) {
		if (conn_res) { N.F.org = cx.d_org.as<uint32_t>(); N.F.foff = tri ? nullptr : cx.d_foff.as<uint32_t>(); }
		else {
			put(up_org, a.org.data(), (size_t)ne * 4);
			N.F.org = up_org;
			if (!tri) { put(up_foff, a.face_off.data(), ((size_t)nf + 1) * 4); N.F.foff = up_foff; }
		}
		const AttrList &A = a.lists[pl], &B = b.lists[pl];
		for (size_t k = 0; k < jobs.size(); ++k) if (job_list[k] == (size_t)pl) { N.a = jobs[k].a; N.b = jobs[k].b; }
		N.F.rows = nullptr; N.F.nf = nf; N.F.ne = ne; N.F.nv = general ? a.nv : A.count; N.F.nrows = A.count;
		N.map = map[pl]; N.err = want_rows ? O.ptr<float>(out.block.p, o_nerr) : nullptr;
		N.part = npart;
		N.b_rows = B.count; N.sa = (uint32_t)A.stride(); N.sb = (uint32_t)B.stride();
		for (int c = 0; c < 3; ++c) { N.ca[c] = pa[pl].c[pos_comp + c]; N.cb[c] = pb[pl].c[pos_comp + c]; }
	}
	TimedEvent ev[2];
	HIP_OK(hipEventRecord(ev[0], st));
	for (size_t k = 0; k < jobs.size(); ++k) launch_distortion_rows(st, jobs[k], pa[job_list[k]], pb[job_list[k]], d_status);
	launch_distortion_fold(st, fold, (DistFinal*)d_res);
	if (want_normals) {
		N.F.rows = vrows.launch(cx, a, pl, W, wb, up);
		launch_distortion_normals(st, N);
		launch_normal_fold(st, N.part, distortion_blocks(nf), 1, (NormFinal*)(d_res + res_bytes + 8));
	}
	HIP_OK(hipGetLastError());
	HIP_OK(hipEventRecord(ev[1], st));
	std::vector<uint8_t> res(res_bytes + 8 + (want_normals ? sizeof(NormFinal) : 0));
	HIP_OK(hipMemcpyAsync(res.data(), d_res, res.size(), hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	uint32_t status = 0;
	memcpy(&status, res.data() + res_bytes, 4);
	if (status) throw Error(HRY_E_ARG, "order does not fit the meshes");
	float ms = 0;
	HIP_OK(hipEventElapsedTime(&ms, ev[0], ev[1]));

	static_assert(sizeof(DistFinal) == sizeof(hry_comp_error) && sizeof(hry_comp_error) == 72, "the results are hry_comp_error records");
	out.comp.assign(nl, std::vector<hry_comp_error>());
	out.pos = hry_pos_error{};
	out.pos.list = -1;
	out.pos_comp = pos_comp;
	for (size_t l = 0; l < nl; ++l) {
		if (!compared(a, l)) continue;
		const int nc = a.lists[l].ncomp();
		out.comp[l].resize(nc);
		for (int c = 0; c < nc; ++c) {
			DistFinal f;
			memcpy(&f, res.data() + (slot_at[l] + c) * sizeof(DistFinal), sizeof f);
			hry_comp_error &e = out.comp[l][c];
			e.max_abs = f.mx; e.sum_sq = f.sum; e.a_min = f.mn; e.a_max = f.mxa;
			e.compared = f.compared; e.skipped = f.skipped; e.nonfinite = f.nonfinite; e.changed = f.changed;
			e.argmax = f.row; e.reserved = 0;
		}
		if ((int)l == pl) {
			DistFinal f;
			memcpy(&f, res.data() + (slot_at[l] + nc) * sizeof(DistFinal), sizeof f);
			out.pos.max_dist = f.mx; out.pos.sum_sq_dist = f.sum; out.pos.compared = f.compared; out.pos.argmax = f.row; out.pos.list = pl;
		}
		if (want_rows) out.bufs.push_back(NamedBuf{ "error" + std::to_string(l), O.ptr<void>(out.block.p, o_err[l]), a.lists[l].count, 1, HRY_FLOAT });
	}
	if (want_normals) {
		memcpy(&out.nrm, res.data() + res_bytes + 8, sizeof out.nrm);
		out.nrm.list = pl;
		out.nrm_why.clear();
		if (want_rows) out.bufs.push_back(NamedBuf{ "normal_error", O.ptr<void>(out.block.p, o_nerr), nf, 1, HRY_FLOAT });
	}
	out.device_ms = (double)ms;
	out.uploaded_bytes = up;
}

}   // namespace hry
