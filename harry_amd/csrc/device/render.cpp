// A mesh as device buffers a GPU program draws: fan triangles, float attributes after the reference's `-c` dequantisation, and
// for general bindings with corner lists (OBJ vt / vn) one vertex per distinct corner key (include/harry_amd.h: hry_render_build;
// kernels: render.hip; DESIGN.md "Render-ready buffers").
//
// Residency: hry_decode leaves the decoded records (d_rec), the connectivity (d_foff / d_org) and the binding tables in HBM and
// marks the mesh and the context with one token (mark_decoded).  While both still carry it -- every other call on the context
// clears the context's, every call that changes the mesh clears the mesh's (api.cpp) -- the build reads them where they are.
// Otherwise it uploads what it needs into its own working buffer (d_render): the encoder's resident_token / gen_token are
// neither read nor written here.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>

#include "result_build.hpp"

namespace hry {

using namespace dev;

namespace {

// every component of list L, dequantised as hry_requant(clear) would (requant_plan: the quantised ones), the others as they are
RequantPlan gather_plan(const AttrList &L)
{
	if (L.ncomp() > dev::kMaxComp) throw Error(HRY_E_UNSUPPORTED, "more than 32 components in a list");
	bool quantised = false;
	for (int c = 0; c < L.ncomp(); ++c) quantised |= L.quant[c] != 0;
	if (quantised && !L.have_bounds) throw Error(HRY_E_ARG, "quantised list without bounds");
	const RequantPlan q = quantised ? requant_plan(L, std::vector<uint8_t>(L.ncomp(), 0)) : RequantPlan{};
	RequantPlan p{};
	p.n = L.ncomp();
	int k = 0;
	for (int c = 0; c < L.ncomp(); ++c) {
		RequantComp &rc = p.c[c];
		if (L.quant[c]) { rc = q.c[k++]; continue; }
		rc.off = L.offset[c]; rc.src_type = L.type[c]; rc.src_bits = 0; rc.dst_bits = 0; rc.dst_type = L.type[c];
	}
	return p;
}

bool rendered(const AttrList &L) { return L.ncomp() > 0 && L.target <= 2; }

}   // namespace

dev::RequantPlan dequant_plan(const AttrList &L) { return gather_plan(L); }

// the list whose first three POS components (mixing.h interpretation 0) are the positions the normals are computed from
static size_t position_list(const Mesh &m, const std::string &what = "normals")
{
	auto npos = [](const AttrList &L) { return L.interp_len.empty() ? 0 : L.interp_len[0]; };
	if (!m.general) {
		if (m.lists.size() < 2 || npos(m.lists[1]) < 3) throw Error(HRY_E_UNSUPPORTED, what + ": the vertex list has fewer than three position components");
		return 1;
	}
	size_t pl = m.lists.size();
	for (size_t l = 0; l < m.lists.size(); ++l) {
		if (m.lists[l].target != 1 || npos(m.lists[l]) < 3) continue;
		if (pl != m.lists.size()) throw Error(HRY_E_UNSUPPORTED, what + ": several vertex lists with three position components");
		pl = l;
	}
	if (pl == m.lists.size()) throw Error(HRY_E_UNSUPPORTED, what + ": no vertex list with three position components");
	for (int r = 0; r < m.bind.nregs_vtx(); ++r) {
		bool bound = false;
		for (int a = 0; a < m.bind.nvtxlists(r); ++a) bound |= (size_t)m.bind.vtxlist(r, a) == pl;
		if (!bound) throw Error(HRY_E_UNSUPPORTED, what + ": a vertex region that does not bind the position list");
	}
	return pl;
}

size_t render_position_list(const Mesh &m, const char *what) { return position_list(m, what); }

void render_build(Context &cx, const Mesh &m, uint32_t flags, RenderResult &out)
{
	if (flags & ~(uint32_t)(HRY_RENDER_VERTEX_NORMALS | HRY_RENDER_FACE_NORMALS | HRY_RENDER_ANGLE_WEIGHTED)) throw Error(HRY_E_ARG, "unknown render flag");
	if ((flags & HRY_RENDER_ANGLE_WEIGHTED) && !(flags & HRY_RENDER_VERTEX_NORMALS)) throw Error(HRY_E_ARG, "HRY_RENDER_ANGLE_WEIGHTED without HRY_RENDER_VERTEX_NORMALS");
	const bool want_vn = flags & HRY_RENDER_VERTEX_NORMALS, want_fn = flags & HRY_RENDER_FACE_NORMALS, want_n = want_vn || want_fn;
	if (m.partial) throw Error(HRY_E_ARG, "partially decoded mesh (a share of a sharded container): only its runs are real");
	if (m.lists.size() > (size_t)kMaxLists) throw Error(HRY_E_UNSUPPORTED, "more than 16 attribute lists");
	for (size_t d = 0; d < 3 && d < m.have_degree.size(); ++d)
		if (m.have_degree[d]) throw Error(HRY_E_INTERNAL, "a face with fewer than three corners (no reader or constructor builds one)");
	const uint32_t nv = m.nv, nf = m.nf, ne = m.ne();
	if (m.face_off.size() != (size_t)nf + 1 || m.org.size() < ne) throw Error(HRY_E_ARG, "mesh without its connectivity");
	const uint64_t ntri = m.ntri();
	HIP_OK(hipSetDevice(cx.device));
	const size_t nl = m.lists.size();
	const bool general = m.general;
	const Bindings &b = m.bind;
	const size_t pl = want_n ? position_list(m) : 0;
	for (size_t l = 0; l < nl; ++l)
		if (m.lists[l].data.size() < (size_t)m.lists[l].count * m.lists[l].stride()) throw Error(HRY_E_ARG, "list without its records");

	// ---- unwelded or not, and the small tables of the general bindings: which slot of a region binds a list
	std::vector<int> cpos(nl, -1);   // corner-target list -> its place among them
	uint32_t ncl = 0;
	for (size_t l = 0; l < nl; ++l) if (m.lists[l].target == 2) cpos[l] = (int)ncl++;
	bool unweld = false;
	std::vector<int32_t> small;   // cslot (face regions x corner lists), then per list its slot per region
	std::vector<size_t> slot_at(nl, 0);
	size_t cslot_at = 0;
	if (general) {
		for (int r = 0; r < b.nregs_face(); ++r) unweld |= b.ncornerlists(r) > 0;
		if (b.face_reg.size() < nf || b.vtx_reg.size() < nv || b.face_attr.size() < (size_t)nf * b.nb_face || b.vtx_attr.size() < (size_t)nv * b.nb_vtx ||
		    b.corner_attr.size() < (size_t)ne * b.nb_corner)
			throw Error(HRY_E_ARG, "mesh without its binding tables");
		cslot_at = small.size();
		small.resize(small.size() + (size_t)b.nregs_face() * ncl, -1);
		for (int r = 0; r < b.nregs_face(); ++r)
			for (int a = 0; a < b.ncornerlists(r); ++a) {
				const int l = b.cornerlist(r, a);
				if (l >= 0 && (size_t)l < nl && cpos[l] >= 0) small[cslot_at + (size_t)r * ncl + cpos[l]] = a;
			}
		for (size_t l = 0; l < nl; ++l) {
			const int t = m.lists[l].target;
			slot_at[l] = small.size();
			const int nr = t == 1 ? b.nregs_vtx() : b.nregs_face();
			small.resize(small.size() + (size_t)std::max(nr, 1), -1);
			for (int r = 0; r < nr; ++r) {
				const int n = t == 0 ? b.nfacelists(r) : t == 1 ? b.nvtxlists(r) : t == 2 ? b.ncornerlists(r) : 0;
				for (int a = 0; a < n; ++a) {
					const int bl = t == 0 ? b.facelist(r, a) : t == 1 ? b.vtxlist(r, a) : b.cornerlist(r, a);
					if ((size_t)bl == l) small[slot_at[l] + r] = a;
				}
			}
		}
	}

	// ---- where the mesh is read: the decode's buffers, or uploads
	// (a sharded container decoded here: d_whole_*, PLY layout only -- place_segment)
	const bool whole = cx.render_whole;
	const DevBuf &r_foff = whole ? cx.d_whole_foff : cx.d_foff, &r_org = whole ? cx.d_whole_org : cx.d_org;
	bool resident = holds_decode(cx, m) && r_foff.cap >= ((size_t)nf + 1) * 4 && r_org.cap >= (size_t)ne * 4;
	for (size_t l = 0; l < nl && resident; ++l) resident = !rendered(m.lists[l]) || decoded_records(cx, l).cap >= m.lists[l].data.size();
	if (general && resident)
		resident = cx.d_freg.cap >= (size_t)nf * 2 && cx.d_vreg.cap >= (size_t)nv * 2 && cx.d_fattr.cap >= b.face_attr.size() * 4 &&
		           cx.d_vattr.cap >= b.vtx_attr.size() * 4 && cx.d_cattr.cap >= b.corner_attr.size() * 4;

	// the working buffer: what goes up of a mesh that is not resident (up), the slot tables, the unweld's corner -> face table and
	// numbering, the rows of a list with general bindings, the normals' arrays (n)
	Carve W;
	struct { uint32_t *foff, *org, *fattr, *vattr, *cattr; uint8_t *rec[kMaxLists]; uint16_t *freg, *vreg; } up{};
	struct { double *fn; uint32_t *eface, *count, *fill, *start, *sums, *seg, *hubs; float *pos, *vn; } nw{};
	int32_t *d_small;
	uint32_t *eface, *idx;
	W.take(up.foff, resident ? 0 : ((size_t)nf + 1) * 4); W.take(up.org, resident ? 0 : (size_t)ne * 4);
	for (size_t l = 0; l < nl; ++l) W.take(up.rec[l], resident || !rendered(m.lists[l]) ? 0 : m.lists[l].data.size());
	const bool tables = general && !resident;
	W.take(up.freg, tables ? b.face_reg.size() * 2 : 0); W.take(up.vreg, tables ? b.vtx_reg.size() * 2 : 0);
	W.take(up.fattr, tables ? b.face_attr.size() * 4 : 0); W.take(up.vattr, tables ? b.vtx_attr.size() * 4 : 0);
	W.take(up.cattr, tables ? b.corner_attr.size() * 4 : 0);
	W.take(d_small, small.size() * 4);
	W.take(eface, unweld ? (size_t)ne * 4 : 0);
	DedupPlan D;   // the unweld's numbering of the corners (dedup.hip); D.ids: corner -> output vertex
	if (unweld) D.reserve(W, ne);
	W.take(idx, general ? (size_t)std::max(std::max(nf, nv), ne) * 4 : 0);
	// normals (normals.hip): N_f per face; per vertex its corners (counters, cursors, segment starts, the scan's sums, the segments,
	// the list of hubs); a corner -> face table for mixed degrees (the unweld's where there is one); unwelded meshes: the position
	// list per vertex and the normals per vertex
	bool all_tri = true;
	for (size_t d = 4; d < m.have_degree.size(); ++d) all_tri &= !m.have_degree[d];
	all_tri &= (uint64_t)ne == 3ull * nf;
	const bool n_eface = want_n && !all_tri && !unweld;
	const size_t pos_w = want_n ? (size_t)m.lists[pl].ncomp() : 0;
	W.take(nw.fn, want_n ? (size_t)nf * 24 : 0); W.take(nw.eface, n_eface ? (size_t)ne * 4 : 0);
	W.take(nw.count, want_vn ? (size_t)nv * 4 : 0); W.take(nw.fill, want_vn ? (size_t)nv * 4 : 0);
	W.take(nw.start, want_vn ? ((size_t)nv + 1) * 4 : 0); W.take(nw.sums, want_vn ? scan_sums_words(nv) * 4 : 0);
	W.take(nw.seg, want_vn ? (size_t)ne * 4 : 0); W.take(nw.hubs, want_vn ? ((size_t)normals_hub_capacity(ne) + 1) * 4 : 0);
	W.take(nw.pos, want_n && unweld ? (size_t)nv * pos_w * 4 : 0); W.take(nw.vn, want_vn && unweld ? (size_t)nv * 12 : 0);
	cx.d_render.ensure(W.total);
	W.bind(cx.d_render.p);
	if (unweld) D.bind(W, cx.d_render.p);

	hipStream_t st = cx.stream;
	uint64_t uploaded = 0;
	auto put = [&](void *piece, const void *src, size_t bytes) {
		if (!bytes) return;
		HIP_OK(hipMemcpyAsync(piece, src, bytes, hipMemcpyHostToDevice, st));
		uploaded += bytes;
	};
	const uint32_t *foff, *org;
	const uint8_t *rec[kMaxLists] = {};
	const uint16_t *freg = nullptr, *vreg = nullptr;
	const uint32_t *fattr = nullptr, *vattr = nullptr, *cattr = nullptr;
	if (resident) {
		foff = r_foff.as<uint32_t>(); org = r_org.as<uint32_t>();
		for (size_t l = 0; l < nl; ++l) rec[l] = decoded_records(cx, l).as<uint8_t>();
		if (general) {
			freg = cx.d_freg.as<uint16_t>(); vreg = cx.d_vreg.as<uint16_t>();
			fattr = cx.d_fattr.as<uint32_t>(); vattr = cx.d_vattr.as<uint32_t>(); cattr = cx.d_cattr.as<uint32_t>();
		}
	} else {
		put(up.foff, m.face_off.data(), ((size_t)nf + 1) * 4);
		put(up.org, m.org.data(), (size_t)ne * 4);
		foff = up.foff; org = up.org;
		for (size_t l = 0; l < nl; ++l) {
			if (rendered(m.lists[l])) put(up.rec[l], m.lists[l].data.data(), m.lists[l].data.size());
			rec[l] = up.rec[l];
		}
		if (general) {
			put(up.freg, b.face_reg.data(), b.face_reg.size() * 2); put(up.vreg, b.vtx_reg.data(), b.vtx_reg.size() * 2);
			put(up.fattr, b.face_attr.data(), b.face_attr.size() * 4); put(up.vattr, b.vtx_attr.data(), b.vtx_attr.size() * 4);
			put(up.cattr, b.corner_attr.data(), b.corner_attr.size() * 4);
			freg = up.freg; vreg = up.vreg; fattr = up.fattr; vattr = up.vattr; cattr = up.cattr;
		}
	}
	put(d_small, small.data(), small.size() * 4);

	StretchTimer timer;

	// ---- unweld: the number of output vertices comes down before the outputs are allocated (no corners: none).  The events
	// enclose kernels only: the table's fill and every copy lie outside them
	uint32_t nout = unweld ? 0 : nv;
	UnweldView u{};
	if (unweld && ne) {
		u.org = org; u.eface = eface; u.corner_attr = cattr; u.face_reg = freg; u.cslot = d_small + cslot_at;
		u.nf = nf; u.nregs = (uint32_t)b.nregs_face(); u.nlists = ncl; u.nb_corner = (uint32_t)b.nb_corner;
		HIP_OK(hipMemsetAsync(D.table, 0xff, D.table_bytes(), st));   // (launch_dedup_count gives u the plan's table, mask and count)
	}
	timer.mark(st);
	if (unweld && ne) {
		launch_edge_faces(st, foff, nf, eface);
		launch_dedup_count(st, u, D);
	}
	timer.mark(st);
	if (unweld && ne) HIP_OK(hipMemcpyAsync(&nout, D.total(), 4, hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	if (nout > ne && unweld) throw Error(HRY_E_INTERNAL, "unweld: more output vertices than corners");

	// ---- the outputs, in one allocation
	OutputPlan plan;
	plan.add("indices", ntri, 3, HRY_UINT);
	plan.add("tri_face", ntri, 1, HRY_UINT);
	plan.add("vertex_source", nout, 1, HRY_UINT);
	if (unweld) plan.add("corner_source", nout, 1, HRY_UINT);
	if (general) plan.add("face_region", nf, 1, HRY_USHORT);
	for (size_t l = 0; l < nl; ++l)
		if (rendered(m.lists[l])) plan.add("list" + std::to_string(l), m.lists[l].target == 0 ? nf : nout, m.lists[l].ncomp(), HRY_FLOAT);
	if (want_vn) plan.add("normals", nout, 3, HRY_FLOAT);
	if (want_fn) plan.add("face_normals", nf, 3, HRY_FLOAT);
	plan.alloc(cx.device, out);
	auto dst = [&](const char *name) { return out.ptr<uint32_t>(name); };
	auto list_rows = [&](size_t l) { return out.ptr<float>(("list" + std::to_string(l)).c_str()); };

	if (want_vn && nv) {   // (the counters' fill lies outside the events, like the table's)
		HIP_OK(hipMemsetAsync(nw.count, 0, (size_t)nv * 4, st));
		HIP_OK(hipMemsetAsync(nw.fill, 0, (size_t)nv * 4, st));
		HIP_OK(hipMemsetAsync(nw.hubs, 0, 4, st));
	}
	timer.mark(st);
	uint32_t *vsrc = dst("vertex_source");
	if (unweld && ne) launch_dedup_assign(st, D, nout, dst("corner_source"), org, vsrc);   // vertex_source = org of the first corner
	else if (!unweld) launch_iota(st, nv, vsrc);
	launch_fan(st, foff, nf, ntri, unweld ? D.ids : org, ne, dst("tri_face"), dst("indices"));
	for (size_t l = 0; l < nl; ++l) {
		const AttrList &L = m.lists[l];
		if (!rendered(L)) continue;
		const uint32_t rows = L.target == 0 ? nf : nout;
		const uint32_t *rows_idx = nullptr;
		if (general) {
			RowsView v{};
			v.slot = d_small + slot_at[l]; v.count = L.count;
			if (L.target == 0) { v.reg = freg; v.nowner = nf; v.nregs = (uint32_t)b.nregs_face(); v.attr = fattr; v.nb = (uint32_t)b.nb_face; v.nelem = nf; }
			else if (L.target == 1) { v.src = unweld ? vsrc : nullptr; v.reg = vreg; v.nowner = nv; v.nregs = (uint32_t)b.nregs_vtx(); v.attr = vattr; v.nb = (uint32_t)b.nb_vtx; v.nelem = nv; }
			else if (unweld) { v.src = dst("corner_source"); v.efc = eface; v.reg = freg; v.nowner = nf; v.nregs = (uint32_t)b.nregs_face(); v.attr = cattr; v.nb = (uint32_t)b.nb_corner; v.nelem = ne; }
			// (a corner list no region binds, identity layout: nelem 0, every row without a record)
			launch_rows_of(st, v, rows, idx);
			rows_idx = idx;
		}
		launch_render_gather(st, rec[l], L.stride(), L.count, rows_idx, rows, gather_plan(L), list_rows(l));
	}
	if (want_n) {
		const AttrList &L = m.lists[pl];
		NrmView n{};
		n.foff = foff; n.org = org; n.nv = nv; n.nf = nf; n.ne = ne; n.angle = (flags & HRY_RENDER_ANGLE_WEIGHTED) ? 1 : 0;
		n.pos_stride = (uint32_t)pos_w;
		const size_t pos_at = (size_t)L.interp_off[0];
		if (unweld) {   // the position list once more, a row per decoded vertex
			RowsView v{};
			v.slot = d_small + slot_at[pl]; v.count = L.count;
			v.reg = vreg; v.nowner = nv; v.nregs = (uint32_t)b.nregs_vtx(); v.attr = vattr; v.nb = (uint32_t)b.nb_vtx; v.nelem = nv;
			launch_rows_of(st, v, nv, idx);
			launch_render_gather(st, rec[pl], L.stride(), L.count, idx, nv, gather_plan(L), nw.pos);
			n.pos = nw.pos + pos_at;
		} else n.pos = list_rows(pl) + pos_at;   // identity layout: row v is vertex v
		if (!all_tri) {
			if (n_eface) launch_edge_faces(st, foff, nf, nw.eface);
			n.eface = n_eface ? nw.eface : eface;
		}
		launch_face_normals(st, n, nw.fn, want_fn ? out.ptr<float>("face_normals") : nullptr);
		if (want_vn) {
			float *vn = unweld ? nw.vn : out.ptr<float>("normals");
			launch_vertex_normals(st, n, nw.fn, nw.count, nw.fill, nw.start, nw.sums, nw.seg, nw.hubs, vn);
			if (unweld) launch_normals_expand(st, vn, vsrc, nout, nv, out.ptr<float>("normals"));
		}
	}
	timer.mark(st);
	if (general && nf) HIP_OK(hipMemcpyAsync(dst("face_region"), freg, (size_t)nf * 2, hipMemcpyDeviceToDevice, st));
	HIP_OK(hipStreamSynchronize(st));
	out.device_ms = timer.ms();
	out.uploaded_bytes = uploaded;
	out.nverts = nout;
	out.ntris = ntri;
}

// one counter for the whole process: a token names one decode on one context, whatever other contexts do
static std::atomic<uint64_t> g_render_tokens{ 1 };

void mark_decoded(Context &cx, Mesh &m, bool whole)
{
	m.render_token = 0;
	cx.render_token = 0;
	if (!whole && (cx.res_nf != m.nf || cx.res_ne != m.ne())) return;   // (the context's connectivity is not this mesh's)
	m.render_token = cx.render_token = g_render_tokens.fetch_add(1, std::memory_order_relaxed);
	cx.render_whole = whole;
	cx.render_nf = m.nf; cx.render_ne = m.ne();
}

bool holds_decode(const Context &cx, const Mesh &m)
{
	return m.render_token != 0 && m.render_token == cx.render_token && cx.render_nf == m.nf && cx.render_ne == m.ne() &&
	       !(cx.render_whole && (m.general || m.lists.size() > 2));
}

bool place_segment(Context &cx, const Mesh &seg, const std::vector<ShardRun> &runs, uint32_t gnv, uint32_t gnf, uint32_t gne)
{
	const uint32_t nlv = seg.nv, nlf = seg.nf, nle = seg.ne(), nr = (uint32_t)runs.size();
	const size_t vstride = (size_t)seg.lists[1].stride(), fstride = (size_t)seg.lists[0].stride();
	if (seg.general || seg.lists.size() != 2 || cx.res_nf != nlf || cx.res_ne != nle || cx.d_foff.cap < ((size_t)nlf + 1) * 4 || cx.d_org.cap < (size_t)nle * 4 ||
	    cx.d_rec[1].cap < (size_t)nlv * vstride || cx.d_rec[0].cap < (size_t)nlf * fstride)
		return false;
	std::vector<uint32_t> tab((size_t)6 * nr);
	uint32_t lv = 0, lf = 0, lh = 0;
	for (uint32_t j = 0; j < nr; ++j) {
		const ShardRun &r = runs[j];
		tab[j] = lv; tab[nr + j] = lf; tab[2 * nr + j] = lh;
		tab[3 * nr + j] = r.first_vertex; tab[4 * nr + j] = r.first_face; tab[5 * nr + j] = r.first_halfedge;
		lv += r.n_vertices; lf += r.n_faces; lh += r.n_halfedges;
	}
	if (lv != nlv || lf != nlf || lh != nle) return false;
	cx.d_whole_runs.ensure(std::max<size_t>(tab.size() * 4, 16));
	HIP_OK(hipMemcpyAsync(cx.d_whole_runs.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, cx.stream));
	const uint32_t *t = cx.d_whole_runs.as<uint32_t>();
	const RunPlace rp{ t, t + nr, t + 2 * nr, t + 3 * nr, t + 4 * nr, t + 5 * nr, nr, gnv, gnf, gne };
	launch_place_segment(cx.stream, rp, cx.d_rec[1].as<uint8_t>(), nlv, (uint32_t)vstride, cx.d_whole_rec[1].as<uint8_t>(),
	                     cx.d_rec[0].as<uint8_t>(), nlf, (uint32_t)fstride, cx.d_whole_rec[0].as<uint8_t>(), cx.d_org.as<uint32_t>(), nle, cx.d_whole_org.as<uint32_t>(),
	                     cx.d_foff.as<uint32_t>(), cx.d_whole_foff.as<uint32_t>());
	HIP_OK(hipStreamSynchronize(cx.stream));   // (the next segment's decode reuses d_rec / d_foff / d_org, on other streams too)
	return true;
}

void result_copy(Context &cx, const DeviceResult &r, const char *name, const char *what, void *dst, bool dst_is_device, bool same_device)
{
	const NamedBuf *b = r.find(name);
	if (!b) throw Error(HRY_E_ARG, std::string("no such ") + what + ": " + name);
	if (!b->bytes()) return;
	if (!dst) throw Error(HRY_E_ARG, "null destination");
	if (same_device && r.block.device != cx.device) throw Error(HRY_E_ARG, std::string("the ") + what + "s live on another device than the context's");
	HIP_OK(hipSetDevice(cx.device));
	HIP_OK(hipMemcpyAsync(dst, b->p, b->bytes(), dst_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, cx.stream));
	HIP_OK(hipStreamSynchronize(cx.stream));
}

}   // namespace hry
