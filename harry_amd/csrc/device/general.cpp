// The reference stream (.hry v0.1) of a mesh with GENERAL bindings: several regions, records
// shared between elements, corner attributes -- what the OBJ reader creates (formats/obj/reader.rl:108-277) and what
// formats/hry/attrcode.h:23-80,135-154,321-393,443-531 code.  The PLY layout keeps its own faster pipeline (codec.cpp).
//
// Division of labour, as everywhere in the compat profile:
//   host    the cut-border walk; which record every vertex / face / corner names and whether the stream says so with a new
//           record (DATA), a distance in creation order (HIST) or a distance in the vertex' own list of names (LHIST) --
//           integer bookkeeping along the coding order; the position of every symbol in the single stream
//   device  prediction + residuals of every record coded as DATA (general.hip), the adaptive models of every byte plane by
//           counting, the range coder (kernels.hip: the same kernels as the PLY layout; planes carry explicit positions)
// and for the decoder: host = serial entropy decode + replay + the same bookkeeping (compat_read.cpp), device = un-prediction.
// (The parallel container has no single sequence: there the bookkeeping is the device's too -- events.hip, general_planes_encode.)
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <functional>

#include "codec_math.hpp"
#include "context.hpp"
#include "kernels.hpp"

#include <exception>
#include <thread>

namespace hry {

using namespace dev;

bool reconstruct_vertex_list_fast(Context &cx, Mesh &m, int l, const OrderVec &order_v, const std::vector<uint32_t> &seg_start,
                                  const std::vector<uint32_t> &seg_level, const std::vector<uint8_t> &vplanes, const uint8_t *d_vplanes = nullptr);   // unchunk.cpp
bool vertex_list_fast_applicable(const Mesh &m, int l, size_t n_order);                                                                             // unchunk.cpp
void reconstruct_vertex_list_detached(Context &cx, Mesh &t, const Mesh &conn, const OrderVec &order_v, const std::vector<uint32_t> &seg_start,
                                      const std::vector<uint32_t> &seg_level, const uint8_t *d_vplanes, long long trace_origin);                    // unchunk.cpp
long long trace_origin_ns();                                                                                                                          // unchunk.cpp

void check_general(const Mesh &m)
{
	const Bindings &b = m.bind;
	if (m.lists.size() > (size_t)kMaxLists) throw Error(HRY_E_UNSUPPORTED, "more than 16 attribute lists");
	if (b.nregs_face() > 128 || b.nregs_vtx() > 128) throw Error(HRY_E_UNSUPPORTED, kTooManyRegionsText);
	if (b.nb_face > 255 || b.nb_vtx > 255 || b.nb_corner > 255) throw Error(HRY_E_UNSUPPORTED, "more than 255 lists bound to one region");
	if (b.face_reg.size() != m.nf || b.vtx_reg.size() != m.nv || b.face_attr.size() != (size_t)m.nf * b.nb_face ||
	    b.vtx_attr.size() != (size_t)m.nv * b.nb_vtx || b.corner_attr.size() != (size_t)m.ne() * b.nb_corner)
		throw Error(HRY_E_ARG, "binding tables do not match the element counts");
	auto bound = [&](int l, int want) {
		if (l < 0 || l >= (int)m.lists.size()) throw Error(HRY_E_ARG, "a region binds a list that does not exist");
		if (m.lists[l].target != want) throw Error(HRY_E_ARG, "a region binds a list of another kind");
	};
	for (int r = 0; r < b.nregs_face(); ++r) {
		for (int a = 0; a < b.nfacelists(r); ++a) bound(b.facelist(r, a), 0);
		for (int a = 0; a < b.ncornerlists(r); ++a) bound(b.cornerlist(r, a), 2);
	}
	for (int r = 0; r < b.nregs_vtx(); ++r) for (int a = 0; a < b.nvtxlists(r); ++a) bound(b.vtxlist(r, a), 1);
	for (uint32_t f = 0; f < m.nf; ++f) if (b.face_reg[f] >= b.nregs_face()) throw Error(HRY_E_ARG, "face region out of range");
	for (uint32_t v = 0; v < m.nv; ++v) if (b.vtx_reg[v] >= b.nregs_vtx()) throw Error(HRY_E_ARG, "vertex region out of range");
	// every record an element names exists (a decoded header may announce elements and an empty list)
	auto holds = [&](int l, uint32_t rec) { if (rec >= m.lists[l].count || (size_t)(rec + 1) * m.lists[l].stride() > m.lists[l].data.size()) throw Error(HRY_E_ARG, "an element names a record its list does not hold"); };
	for (uint32_t f = 0; f < m.nf; ++f) {
		const int r = b.face_reg[f];
		for (int a = 0; a < b.nfacelists(r); ++a) holds(b.facelist(r, a), b.face_attr[(size_t)f * b.nb_face + a]);
		for (uint32_t h = m.face_off[f]; h < m.face_off[f + 1]; ++h)
			for (int a = 0; a < b.ncornerlists(r); ++a) holds(b.cornerlist(r, a), b.corner_attr[(size_t)h * b.nb_corner + a]);
	}
	for (uint32_t v = 0; v < m.nv; ++v) { const int r = b.vtx_reg[v]; for (int a = 0; a < b.nvtxlists(r); ++a) holds(b.vtxlist(r, a), b.vtx_attr[(size_t)v * b.nb_vtx + a]); }
}

// connectivity + every list + the binding tables -> HBM
// (a mesh that hry_mesh_upload has made resident stays so, tables included, like a mesh in the PLY layout)
void upload_general(Context &cx, Mesh &m)
{
	const bool mesh_there = m.device_token != 0 && m.device_token == cx.resident_token && !m.twins_pending;
	if (mesh_there && cx.gen_token == m.device_token) return;
	if (!mesh_there) cx.upload_mesh(m);
	const Bindings &b = m.bind;
	auto put = [&](DevBuf &d, const void *src, size_t bytes) {
		d.ensure(std::max<size_t>(bytes, 16));
		if (bytes) HIP_OK(hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, cx.stream));
	};
	put(cx.d_vreg, b.vtx_reg.data(), b.vtx_reg.size() * 2);
	put(cx.d_freg, b.face_reg.data(), b.face_reg.size() * 2);
	put(cx.d_vattr, b.vtx_attr.data(), b.vtx_attr.size() * 4);
	put(cx.d_cattr, b.corner_attr.data(), b.corner_attr.size() * 4);
	put(cx.d_fattr, b.face_attr.data(), b.face_attr.size() * 4);
	HIP_OK(hipStreamSynchronize(cx.stream));
	cx.gen_token = m.device_token;
}
static GenView gen_view(const Context &cx, const Mesh &m)
{
	GenView gv;
	gv.vtx_reg = cx.d_vreg.as<uint16_t>(); gv.face_reg = cx.d_freg.as<uint16_t>();
	gv.vtx_attr = cx.d_vattr.as<uint32_t>(); gv.corner_attr = cx.d_cattr.as<uint32_t>();
	gv.nb_vtx = m.bind.nb_vtx; gv.nb_corner = m.bind.nb_corner;
	return gv;
}

namespace {

// a device arena filled from host vectors in one go: the pieces first, room for what kernels compute behind them; a piece or a
// room given a pointer of the caller's has it set to its place on the device by send()
struct Arena {
	struct Piece { const void *p; size_t bytes, at; };
	struct Slot { void *ptr; size_t at; };   // ptr: the caller's pointer variable
	std::vector<Piece> pieces;
	std::vector<Slot> slots;
	size_t bytes = 0, filled = 0;   // the whole arena / its pieces
	size_t room(size_t n)
	{
		const size_t at = (bytes + 15) & ~(size_t)15;
		bytes = at + n;
		return at;
	}
	template <typename T> void room(size_t n, T *&ptr) { slots.push_back(Slot{ &ptr, room(n) }); }
	size_t add(const void *p, size_t n)
	{
		pieces.push_back(Piece{ p, n, room(n) });
		filled = bytes;
		return pieces.back().at;
	}
	template <typename V> size_t add(const V &v) { return add(v.data(), v.size() * sizeof(typename V::value_type)); }
	template <typename V, typename T> void add(const V &v, T *&ptr) { slots.push_back(Slot{ &ptr, add(v) }); }
	// the pieces -> the context's pinned block -> HBM, behind everything on the stream; no wait: the block is the context's, and the
	// context's next call finds the stream drained.  (Until round 5 a pageable vector that grew piece by piece, its copy, and a wait
	// for it because the vector went out of scope: 4 of the 11 ms of a 180 000-triangle scene's encode.)
	void send(Context &cx, void *dst)
	{
		for (const Slot &s : slots) { void *at = (uint8_t*)dst + s.at; memcpy(s.ptr, &at, sizeof at); }
		if (!filled) return;
		cx.h_gen.ensure(filled);
		uint8_t *h = cx.h_gen.as<uint8_t>();
		for (const Piece &q : pieces) if (q.bytes) memcpy(h + q.at, q.p, q.bytes);
		HIP_OK(hipMemcpyAsync(dst, h, filled, hipMemcpyHostToDevice, cx.stream));
	}
};

// what the stream says about one list, on the device (in cx.d_gen): the kinds of its references, the distances in creation order
// and in the vertices' own names as 32-bit values, the records coded as data (which, at which half-edge / face, at which slot);
// *_pos: every symbol's position in the ONE sequence of the reference stream (the container has none); gh, lh, data: room for
// the distances' byte planes and the residuals' byte planes
struct ListSyms {
	uint32_t nt = 0, ng = 0, nlh = 0, nd = 0, nbytes = 0;
	uint8_t *type_sym = nullptr, *d_slot = nullptr;
	uint32_t *gh_vals = nullptr, *lh_vals = nullptr, *d_idx = nullptr, *d_he = nullptr;
	uint32_t *type_pos = nullptr, *gh_pos = nullptr, *lh_pos = nullptr, *d_pos = nullptr;
	uint8_t *gh = nullptr, *lh = nullptr, *data = nullptr;
};
struct RegionSyms { uint8_t *rv = nullptr, *rf = nullptr; uint32_t *rv_pos = nullptr, *rf_pos = nullptr; uint32_t n_rv = 0, n_rf = 0; };

// collect_events' arrays -> the arena (pinned, one copy, no wait: Arena::send), with room behind for the planes the kernels make
void send_events(Context &cx, const Events &E, bool positions, std::vector<ListSyms> &ls, RegionSyms &rg)
{
	Arena A;
	ls.assign(E.ls.size(), ListSyms());
	for (size_t l = 0; l < ls.size(); ++l) {
		const ListStream &S = E.ls[l];
		ListSyms &L = ls[l];
		L.nt = (uint32_t)S.type_sym.size(); L.ng = (uint32_t)S.gh_val.size(); L.nlh = (uint32_t)S.lh_val.size(); L.nd = (uint32_t)S.d_idx.size(); L.nbytes = S.nbytes;
		A.add(S.type_sym, L.type_sym); if (positions) A.add(S.type_pos, L.type_pos);
		// (the distances go up as 32-bit values and are split into their byte planes on the device, like the connectivity groups:
		// the host's byte loops were a millisecond of an 80 000-triangle scene)
		A.add(S.gh_val, L.gh_vals); if (positions) A.add(S.gh_pos, L.gh_pos);
		A.add(S.lh_val, L.lh_vals); if (positions) A.add(S.lh_pos, L.lh_pos);
		if (positions) A.add(S.d_pos, L.d_pos);
		A.add(S.d_idx, L.d_idx); A.add(S.d_he, L.d_he); A.add(S.d_slot, L.d_slot);
	}
	rg.n_rv = (uint32_t)E.rv_sym.size(); rg.n_rf = (uint32_t)E.rf_sym.size();
	A.add(E.rv_sym, rg.rv); if (positions) A.add(E.rv_pos, rg.rv_pos);
	A.add(E.rf_sym, rg.rf); if (positions) A.add(E.rf_pos, rg.rf_pos);
	for (ListSyms &L : ls) { A.room((size_t)L.nd * L.nbytes, L.data); A.room((size_t)L.ng * 4, L.gh); A.room((size_t)L.nlh * 2, L.lh); }
	cx.d_gen.ensure(std::max<size_t>(A.bytes, 16));
	A.send(cx, cx.d_gen.p);
}
// the distances of every list -> their byte planes
void split_histories(Context &cx, const std::vector<ListSyms> &ls)
{
	for (const ListSyms &L : ls) {
		launch_split_bytes(cx.stream, L.gh_vals, L.ng, 4, L.gh);
		launch_split_bytes(cx.stream, L.lh_vals, L.nlh, 2, L.lh);
	}
}
// ranks of vertices and faces along the coding order, then the residuals of every list's records coded as data
void general_residuals(Context &cx, const Mesh &m, uint32_t vc, uint32_t fc, const std::vector<ListSyms> &ls)
{
	cx.d_rank.ensure(std::max<size_t>((size_t)m.nv * 4 + (size_t)m.nf * 4, 16));
	const uint32_t *d_rank = cx.d_rank.as<uint32_t>();
	uint32_t *d_frank = cx.d_rank.as<uint32_t>() + m.nv;
	const ConnView cv = cx.conn_view();
	const GenView gv = gen_view(cx, m);
	rank_coding_order(cx, m, vc);
	launch_face_rank(cx.stream, cv, cx.d_order_f.as<uint32_t>(), fc, d_frank);
	for (size_t l = 0; l < ls.size(); ++l) {
		const ListSyms &L = ls[l];
		if (!L.nd || !L.nbytes) continue;
		const ListDesc ld = make_list_desc(m.lists[l]);
		const uint8_t *rec = cx.d_rec[l].as<uint8_t>();
		if (m.lists[l].target == 1) launch_gen_vtx_resid(cx.stream, cv, gv, d_rank, L.d_he, L.d_slot, L.d_idx, L.nd, rec, ld, L.data);
		else if (m.lists[l].target == 2) launch_gen_corner_resid(cx.stream, cv, gv, d_frank, L.d_he, L.d_slot, L.d_idx, L.nd, rec, ld, L.data);
		else launch_gen_face_resid(cx.stream, L.d_idx, L.nd, rec, ld, L.data);
	}
}
// where a plane of general_plane_layout lies, with the positions of its symbols in the reference stream (pos[j] + g.byte)
struct PlaneAt { const uint8_t *sym; uint32_t n; const uint32_t *pos; };
PlaneAt plane_at(const GenPlane &g, const std::vector<ListSyms> &ls, const RegionSyms &rg)
{
	if (g.what == GP_REGV) return PlaneAt{ rg.rv, rg.n_rv, rg.rv_pos };
	if (g.what == GP_REGF) return PlaneAt{ rg.rf, rg.n_rf, rg.rf_pos };
	const ListSyms &L = ls[g.list];
	switch (g.what) {
	case GP_TYPE: return PlaneAt{ L.type_sym, L.nt, L.type_pos };
	case GP_GHIST: return PlaneAt{ L.gh + (size_t)g.byte * L.ng, L.ng, L.gh_pos };
	case GP_LHIST: return PlaneAt{ L.lh + (size_t)g.byte * L.nlh, L.nlh, L.lh_pos };
	default: return PlaneAt{ L.data + (size_t)g.byte * L.nd, L.nd, L.d_pos };
	}
}

}   // namespace

void encode_general(Context &cx, Mesh &m, std::vector<uint8_t> &out)
{
	HIP_OK(hipSetDevice(cx.device));
	auto t_all = Clock::now();
	cx.timing = hry_timing{};
	check_codable(m);
	check_general(m);
	for (auto &L : m.lists) if (!L.have_bounds && L.ncomp()) { device_bounds(cx, m); break; }
	for (auto &L : m.lists) if (!L.have_bounds) { L.bmin.assign(L.stride(), 0); L.bmax.assign(L.stride(), 0); L.have_bounds = true; }
	upload_general(cx, m);

	out.clear();
	write_hry_header(m, 1, out);
	auto t_walk = Clock::now();
	WalkResult w;
	cut_border_walk(m, w, false);   // the operation model is evaluated on the device (k_opmodel_*), the groups' places in the ONE symbol sequence come out of the walk -- also from its threads (cbm_walk.cpp: the components' pieces are put in coding order)
	Events E;
	collect_events(m, w, w.n_conn, true, E);
	cx.timing.host_walk_ms = ms_since(t_walk);
	if ((uint64_t)E.end_pos + test_extra("HRY_TEST_EXTRA_SYMBOLS") >= (1ull << 31)) throw Error(HRY_E_UNSUPPORTED, "more than 2^31 symbols in one compat stream");
	const uint32_t ns = E.end_pos;
	const uint32_t vc = (uint32_t)w.order_v.size(), fc = (uint32_t)w.order_f.size();

	// ---- H2D: orders, repaired twins, connectivity symbols, then everything collect_events produced
	auto t_h2d = Clock::now();
	HIP_OK(hipEventRecord(cx.ev[0], cx.stream));
	cx.d_order_v.ensure(std::max<size_t>((size_t)vc * 4, 16));
	cx.d_order_f.ensure(std::max<size_t>((size_t)fc * 4, 16));
	if (vc) HIP_OK(hipMemcpyAsync(cx.d_order_v.p, w.order_v.data(), (size_t)vc * 4, hipMemcpyHostToDevice, cx.stream));
	if (fc) HIP_OK(hipMemcpyAsync(cx.d_order_f.p, w.order_f.data(), (size_t)fc * 4, hipMemcpyHostToDevice, cx.stream));
	upload_repaired_twins(cx, m, w);
	const ConnSymbols cs = upload_conn_symbols(cx, w);
	// the arena: symbol planes the host made, position tables, event tables; then room for the residual planes the kernels make
	std::vector<ListSyms> ls;
	RegionSyms rg;
	send_events(cx, E, true, ls, rg);
	split_histories(cx, ls);

	// ---- model jobs: the connectivity's, then the planes in the order of the layout (regions; per list kinds, history, per-vertex
	// history at corner lists, data).  collect_events makes no region symbols for one region and no per-vertex distances but at
	// corner lists: what the layout leaves out is empty
	ModelJobs J(cx, m);
	J.add_conn(w, cs);
	for (const GenPlane &g : general_plane_layout(m)) {
		const PlaneAt p = plane_at(g, ls, rg);
		J.add(p.sym, p.n, g.init, p.pos, (uint32_t)g.byte);
	}
	J.send(cs, ns);
	HIP_OK(hipStreamSynchronize(cx.stream));
	cx.timing.h2d_ms = ms_since(t_h2d);

	// ---- device: residuals of the records coded as data
	HIP_OK(hipEventRecord(cx.ev[1], cx.stream));
	general_residuals(cx, m, vc, fc, ls);
	HIP_OK(hipEventRecord(cx.ev[2], cx.stream));
	// ---- device: models -> per-symbol records in stream order
	launch_conn_models(cx, w, cs);
	J.run();

	if (cx.keep_stages) {
		cx.stage_put_host("order_v", w.order_v.data(), (size_t)vc * 4);
		cx.stage_put_host("order_f", w.order_f.data(), (size_t)fc * 4);
		cx.stage_put("rec", cx.d_rec_sym.p, (size_t)ns * sizeof(SymRec));
		cx.stage_put("sym_l", cx.d_sym_l.p, (size_t)ns * 4);
	}
	finish_compat_stream(cx, ns, t_all, out);
	if (cx.want_order) {   // HRY_FLAG_ORDER (order.cpp): the creation order of every list's records is the host's (collect_events), uploaded with the arena above
		cx.order_lists.assign(m.lists.size(), OrderListSource{});
		for (size_t l = 0; l < m.lists.size(); ++l) cx.order_lists[l] = OrderListSource{ ls[l].d_idx, ls[l].nd };
		order_build(cx, m, w, cx.d_order_v.as<uint32_t>(), cx.d_order_f.as<uint32_t>());
		cx.timing.total_ms = ms_since(t_all);   // (the maps' build counts into the encode's time)
	}
}

// Device part of a decode with general bindings: connectivity, bindings and the lists (holding residual codes in record layout,
// or -- chunked container -- zeros, the codes being scattered from the decoded planes by `fill`) go up; every list with records
// to reconstruct gets its source table and its chains.  ev[l] empty: the list is final already (vertex fast path) or has no records.
static void reconstruct_general(Context &cx, Mesh &m, const OrderVec &order_v, const std::vector<GenRecordEvents> &ev,
                                const std::function<void()> &fill)
{
	auto t_h2d = Clock::now();
	upload_general(cx, m);   // connectivity, bindings, and the residual codes in record layout
	if (fill) fill();
	const uint32_t vc = (uint32_t)order_v.size();
	cx.d_order_v.ensure(std::max<size_t>((size_t)vc * 4, 16));
	cx.d_rank.ensure(std::max<size_t>((size_t)m.nv * 4, 16));
	if (vc) HIP_OK(hipMemcpyAsync(cx.d_order_v.p, order_v.data(), (size_t)vc * 4, hipMemcpyHostToDevice, cx.stream));
	Arena A;
	const size_t nl = m.lists.size();
	std::vector<size_t> he_at(nl), slot_at(nl), src_at(nl), nsrc_at(nl);
	for (size_t l = 0; l < nl; ++l) { he_at[l] = A.add(ev[l].he); slot_at[l] = A.add(ev[l].slot); }
	size_t arena_bytes = (A.bytes + 15) & ~(size_t)15;
	for (size_t l = 0; l < nl; ++l) {
		if (m.lists[l].target != 1 && m.lists[l].target != 2) continue;
		const size_t nd = ev[l].he.size();
		src_at[l] = arena_bytes; arena_bytes += (nd * kSrcCap * 4 + 15) & ~(size_t)15;
		nsrc_at[l] = arena_bytes; arena_bytes += (nd + 15) & ~(size_t)15;
	}
	const size_t jobs_at = arena_bytes;
	size_t max_jobs = 0;
	for (const AttrList &L : m.lists) max_jobs += (size_t)L.ncomp();
	arena_bytes += (max_jobs + 1) * sizeof(GenChainJob);
	cx.d_gen.ensure(std::max<size_t>(arena_bytes, 16));
	A.send(cx, cx.d_gen.p);
	uint8_t *arena = cx.d_gen.as<uint8_t>();
	std::vector<GenChainJob> jobs, lead;   // lead: one per list (the source table is per record)
	for (size_t l = 0; l < nl; ++l) {
		const AttrList &L = m.lists[l];
		const uint32_t nd = (uint32_t)ev[l].he.size();
		if (!nd || !L.ncomp() || (L.target != 1 && L.target != 2)) continue;
		GenChainJob j{};
		j.kind = L.target == 1 ? 0 : 1; j.n = nd; j.rec = cx.d_rec[l].as<uint8_t>();
		j.src = (const uint32_t*)(arena + src_at[l]); j.nsrc = arena + nsrc_at[l];
		j.ev_he = (const uint32_t*)(arena + he_at[l]); j.ev_slot = arena + slot_at[l];
		j.ld = make_list_desc(L);
		lead.push_back(j);
		for (int c = 0; c < L.ncomp(); ++c) { j.comp = c; jobs.push_back(j); }   // the components of a record are predicted independently
	}
	// one launch per kind and storage type (the kernel is instantiated for each); inside a launch every job has its own wavefront
	std::stable_sort(jobs.begin(), jobs.end(), [](const GenChainJob &a, const GenChainJob &b) {
		return std::make_pair(a.kind, (int)a.ld.stype[a.comp]) < std::make_pair(b.kind, (int)b.ld.stype[b.comp]); });
	if (!jobs.empty()) HIP_OK(hipMemcpyAsync(arena + jobs_at, jobs.data(), jobs.size() * sizeof(GenChainJob), hipMemcpyHostToDevice, cx.stream));
	HIP_OK(hipStreamSynchronize(cx.stream));
	cx.timing.h2d_ms = ms_since(t_h2d);

	ConnView cv = cx.conn_view();
	const GenView gv = gen_view(cx, m);
	HIP_OK(hipEventRecord(cx.ev[3], cx.stream));
	rank_coding_order(cx, m, vc);
	for (const GenChainJob &j : lead)
		launch_gen_sources(cx.stream, j.kind, cv, gv, cx.d_rank.as<uint32_t>(), j.ev_he, j.ev_slot, j.n, const_cast<uint32_t*>(j.src), const_cast<uint8_t*>(j.nsrc));
	for (size_t l = 0; l < nl; ++l) {   // face lists: no prediction (attrcode.h:245-270)
		const AttrList &L = m.lists[l];
		if (L.target == 0 && L.ncomp() && !ev[l].he.empty()) launch_faces_unfold(cx.stream, (uint32_t)ev[l].he.size(), make_list_desc(L), cx.d_rec[l].as<uint8_t>());
	}
	HIP_OK(hipEventRecord(cx.ev[7], cx.stream));
	for (size_t a = 0; a < jobs.size();) {
		size_t e = a + 1;
		while (e < jobs.size() && jobs[e].kind == jobs[a].kind && jobs[e].ld.stype[jobs[e].comp] == jobs[a].ld.stype[jobs[a].comp]) ++e;
		launch_gen_chain(cx.stream, jobs[a].kind, jobs[a].ld.stype[jobs[a].comp], cv, gv, cx.d_rank.as<uint32_t>(), (const GenChainJob*)(arena + jobs_at) + a, (uint32_t)(e - a));
		a = e;
	}
	HIP_OK(hipEventRecord(cx.ev[4], cx.stream));
	for (size_t l = 0; l < nl; ++l)
		if (!m.lists[l].data.empty()) HIP_OK(hipMemcpyAsync(m.lists[l].data.data(), cx.d_rec[l].p, m.lists[l].data.size(), hipMemcpyDeviceToHost, cx.stream));
	HIP_OK(hipStreamSynchronize(cx.stream));
	cx.timing.k_chain_ms = cx.elapsed(7, 4);
}

// ---------------------------------------------------------------------------------------------------------
Mesh *decode_general(Context &cx, const uint8_t *p, size_t n, size_t hdr, std::unique_ptr<Mesh> m)
{
	HIP_OK(hipSetDevice(cx.device));
	auto t_all = Clock::now();
	cx.timing = hry_timing{};
	if (m->lists.size() > (size_t)kMaxLists) throw Error(HRY_E_UNSUPPORTED, "more than 16 attribute lists");
	for (const AttrList &L : m->lists)
		for (int c = 0; c < L.ncomp(); ++c) {
			if (L.stype(c) == C_DOUBLE) throw Error(HRY_E_UNSUPPORTED, "lossless double components are outside the supported subset");
			if (kTypeSize[L.stype(c)] == 8) throw Error(HRY_E_UNSUPPORTED, "8-byte storage types (more than 32 quantisation bits, lossless 64-bit integers) are outside the supported subset");   // (before the stream is read: the record chains have no such form)
		}
	auto t_walk = Clock::now();
	OrderVec order_v;
	std::vector<uint32_t> seg_start, seg_level;
	std::vector<GenRecordEvents> ev;
	std::vector<uint8_t> vplanes;
	// one vertex region with one list (every OBJ whose "v" lines have the same number of values): candidate for the vertex chains
	int fast_l = -1;
	if (m->bind.nregs_vtx() == 1 && m->bind.nvtxlists(0) == 1 && !env_on("HRY_GENERIC_VERTEX")) fast_l = m->bind.vtxlist(0, 0);
	read_general_stream(p + hdr, n - hdr, *m, order_v, ev, seg_start, seg_level, fast_l, vplanes);
	cx.timing.host_walk_ms = ms_since(t_walk);
	double fast_ms = 0;
	if (fast_l >= 0 && ev[fast_l].he.size() == order_v.size() && !order_v.empty()) {   // ... and every vertex created its own record
		if (reconstruct_vertex_list_fast(cx, *m, fast_l, order_v, seg_start, seg_level, vplanes)) { ev[fast_l].he.clear(); ev[fast_l].slot.clear(); fast_ms = cx.elapsed(3, 4); }
	}

	reconstruct_general(cx, *m, order_v, ev, nullptr);
	cx.timing.k_predict_ms = cx.elapsed(3, 4) + fast_ms;
	cx.timing.device_ms = cx.timing.k_predict_ms;
	cx.timing.payload_bytes = n - hdr;
	cx.timing.total_ms = ms_since(t_all);
	m->device_token = 0;
	mark_decoded(cx, *m);
	return m.release();
}


// ---------------------------------------------------------------------------------------------------------
// chunked container (.hry v0.2) with general bindings
// ---------------------------------------------------------------------------------------------------------
// The planes of a mesh with general bindings in the parallel container: which record every element names -- on the device
// (events.hip; HRY_HOST_EVENTS: the host's loop and an arena of its arrays, as until round 5) -- and the residuals of the records
// coded as data (general.hip).  Per list: kinds (one byte a reference), four planes of creation-order distances, two of per-vertex
// distances at corner lists, the data planes.
void general_planes_encode(Context &cx, Mesh &m, const WalkResult &w, std::vector<PlaneRef> &planes)
{
	const uint32_t vc = (uint32_t)w.order_v.size(), fc = (uint32_t)w.order_f.size();
	const size_t nl = m.lists.size();
	std::vector<ListSyms> ls;
	RegionSyms reg;
	ConnView cv = cx.conn_view();
	const GenView gv = gen_view(cx, m);
	const Bindings &b = m.bind;
	static const bool host_events_env = env_on("HRY_HOST_EVENTS");
	bool host_events = host_events_env;
again:
	if (host_events) {
		const auto t_events = Clock::now();
		Events E;   // (the host's arrays live until the arena has been copied into pinned memory: Arena::send)
		collect_events(m, w, 0, false, E);
		cx.timing.host_walk_ms += ms_since(t_events);   // (host bookkeeping along the coding order, like the walk: it was missing from the record)
		if (trace_on()) fprintf(stderr, "[hry enc] %8.3f ms  which record every element names (host)\n", ms_since(t_events));
		send_events(cx, E, false, ls, reg);
	} else {
		// ---- on the device.  Most references a list can get, without a pass over the orders: every coded element at every slot
		// of the region with the most slots for it (corner lists: every half-edge)
		std::vector<uint32_t> max_refs(nl, 0);
		for (size_t l = 0; l < nl; ++l) {
			const int tg = m.lists[l].target;
			if (tg == 3) continue;
			const int nreg = tg == 1 ? b.nregs_vtx() : b.nregs_face();
			uint32_t most = 0;
			for (int r = 0; r < nreg; ++r) {
				uint32_t c = 0;
				const int na = tg == 1 ? b.nvtxlists(r) : tg == 0 ? b.nfacelists(r) : b.ncornerlists(r);
				for (int a = 0; a < na; ++a) c += (uint32_t)(tg == 1 ? b.vtxlist(r, a) : tg == 0 ? b.facelist(r, a) : b.cornerlist(r, a)) == (uint32_t)l;
				most = std::max(most, c);
			}
			const uint64_t elems = tg == 1 ? vc : tg == 0 ? fc : m.ne();
			if (elems * most >= (1ull << 31)) throw Error(HRY_E_UNSUPPORTED, "more than 2^31 references to one list");
			max_refs[l] = (uint32_t)(elems * most);
		}
		// the regions' tables (a few words) through the context's pinned block
		Arena A;
		std::vector<int32_t> off_f(b.off_facelist.begin(), b.off_facelist.end()), off_v(b.off_vtxlist.begin(), b.off_vtxlist.end()), off_c(b.off_cornerlist.begin(), b.off_cornerlist.end());
		const size_t a_off_f = A.add(off_f), a_off_v = A.add(off_v), a_off_c = A.add(off_c);
		const size_t a_lf = A.add(b.reg_facelist), a_lv = A.add(b.reg_vtxlist), a_lc = A.add(b.reg_cornerlist);
		// (the vertices' names at the corner slots are shared by the corner lists: at most every half-edge at every corner slot)
		uint32_t most_corner_slots = 0;
		bool any_corner = false;
		for (int r = 0; r < b.nregs_face(); ++r) most_corner_slots = std::max(most_corner_slots, (uint32_t)b.ncornerlists(r));
		for (size_t l = 0; l < nl; ++l) any_corner |= m.lists[l].target == 2 && max_refs[l] != 0;
		if ((uint64_t)m.ne() * most_corner_slots >= (1ull << 31) || (uint64_t)b.nb_corner * m.nv >= (1ull << 31)) throw Error(HRY_E_UNSUPPORTED, "more than 2^31 corner references");
		const uint32_t corner_refs_max = any_corner ? m.ne() * most_corner_slots : 0u, head_words = any_corner ? (uint32_t)b.nb_corner * m.nv : 0u;
		ls.assign(nl, ListSyms());
		std::vector<uint8_t*> ws(nl, nullptr);
		for (size_t l = 0; l < nl; ++l) {
			const size_t r = max_refs[l];
			const uint32_t n_order = m.lists[l].target == 1 ? vc : fc;
			ListSyms &L = ls[l];
			L.nbytes = (uint32_t)m.lists[l].coded_bytes();
			A.room(r, L.type_sym); A.room(r * 4, L.gh_vals); A.room(m.lists[l].target == 2 ? r * 4 : 0, L.lh_vals);
			A.room(r * 4, L.d_idx); A.room(r * 4, L.d_he); A.room(r, L.d_slot);
			A.room(r * 4, L.gh); A.room(m.lists[l].target == 2 ? r * 2 : 0, L.lh); A.room(r * L.nbytes, L.data);
			A.room(r ? dev::events_list_workspace_bytes(n_order, (uint32_t)r, m.lists[l].count) : 0, ws[l]);
		}
		const size_t a_counts = A.room((nl * 4 + 4) * 4);
		A.room(vc, reg.rv); A.room(fc, reg.rf);
		const size_t a_names = A.room(dev::events_names_workspace_bytes(fc, corner_refs_max, head_words));
		// (the arena is sized from upper bounds -- every half-edge times the most slots a region binds to the list -- where the
		// host's loop needs the actual counts: a scene whose bounds do not fit the device's memory takes the host's loop)
		bool no_room = false;
		try { cx.d_gen.ensure(std::max<size_t>(A.bytes, 16)); } catch (const Error &) { (void)hipGetLastError(); no_room = true; }
		if (no_room) { host_events = true; goto again; }
		A.send(cx, cx.d_gen.p);
		uint8_t *arena = cx.d_gen.as<uint8_t>();
		EvRegions rg{ (const int32_t*)(arena + a_off_f), (const int32_t*)(arena + a_off_v), (const int32_t*)(arena + a_off_c),
		              (const uint16_t*)(arena + a_lf), (const uint16_t*)(arena + a_lv), (const uint16_t*)(arena + a_lc), cx.d_fattr.as<uint32_t>(), b.nb_face };
		uint32_t *d_counts = (uint32_t*)(arena + a_counts), *d_err = d_counts + nl * 4;
		HIP_OK(hipMemsetAsync(d_err, 0, 16, cx.stream));
		if (any_corner) dev::launch_corner_places(cx.stream, cv, gv, rg, cx.d_order_f.as<uint32_t>(), fc, corner_refs_max, head_words, m.nv, arena + a_names);
		for (int phase = 0; phase < 2; ++phase)
			for (size_t l = 0; l < nl; ++l) {
				const int tg = m.lists[l].target;
				if (tg == 3) { if (!phase) HIP_OK(hipMemsetAsync(d_counts + 4 * l, 0, 16, cx.stream)); continue; }
				const uint32_t *order = tg == 1 ? cx.d_order_v.as<uint32_t>() : cx.d_order_f.as<uint32_t>();
				const uint32_t n_order = tg == 1 ? vc : fc;
				ListSyms &L = ls[l];
				if (!phase) dev::launch_list_refs(cx.stream, tg, (uint32_t)l, m.lists[l].count, cv, gv, rg, order, n_order, max_refs[l], m.nv, fc, corner_refs_max, head_words, arena + a_names,
				                                  ws[l], d_counts + 4 * l, d_err);
				else dev::launch_list_kinds(cx.stream, tg, m.lists[l].count, cv, n_order, max_refs[l], m.nv, fc, corner_refs_max, head_words, arena + a_names, ws[l], L.type_sym,
				                            L.gh_vals, L.lh_vals, L.d_idx, L.d_he, L.d_slot, d_counts + 4 * l, d_err);
			}
		if (b.nregs_vtx() > 1) { dev::launch_region_symbols(cx.stream, 1, cv, gv, cx.d_order_v.as<uint32_t>(), vc, reg.rv); reg.n_rv = vc; }
		if (b.nregs_face() > 1) { dev::launch_region_symbols(cx.stream, 0, cv, gv, cx.d_order_f.as<uint32_t>(), fc, reg.rf); reg.n_rf = fc; }
		// how many of every kind: the one thing the host needs (the planes' lengths)
		cx.h_small.ensure(std::max<size_t>((nl * 4 + 4) * 4, 4096));
		uint32_t *h_counts = cx.h_small.as<uint32_t>();
		HIP_OK(hipMemcpyAsync(h_counts, d_counts, (nl * 4 + 4) * 4, hipMemcpyDeviceToHost, cx.stream));
		HIP_OK(hipStreamSynchronize(cx.stream));
		const uint32_t err = h_counts[nl * 4];
		if (err & 4u) { host_events = true; goto again; }   // a hub: a vertex with more names at a slot than a device thread walks (events.hip: kMaxNames) -- the host's loop
		if (err & 1u) throw Error(HRY_E_ARG, "an element names a record outside its list");
		if (err & 2u) throw Error(HRY_E_UNSUPPORTED, "more than 65536 different records of one list at one vertex (io.h:104 codes 16 bits)");
		for (size_t l = 0; l < nl; ++l) {
			ListSyms &L = ls[l];
			L.nt = h_counts[4 * l]; L.ng = h_counts[4 * l + 1]; L.nlh = h_counts[4 * l + 2]; L.nd = h_counts[4 * l + 3];
			if (L.nt > max_refs[l] || (uint64_t)L.ng + L.nlh + L.nd != L.nt) throw Error(HRY_E_INTERNAL, "references on the device: the kinds do not add up");
		}
	}
	if (cx.want_order) {   // HRY_FLAG_ORDER (order.cpp): every list's records in creation order stay where they are in the arena until the encode ends
		cx.order_lists.assign(nl, OrderListSource{});
		for (size_t l = 0; l < nl; ++l) cx.order_lists[l] = OrderListSource{ ls[l].d_idx, ls[l].nd };
	}
	split_histories(cx, ls);
	general_residuals(cx, m, vc, fc, ls);
	for (const GenPlane &g : general_plane_layout(m)) {
		const PlaneAt p = plane_at(g, ls, reg);
		planes.push_back(PlaneRef{ p.sym, p.n, g.init });
	}
}


void general_planes_decode(Context &cx, Mesh &m, const OrderVec &order_v, const std::vector<uint32_t> &seg_start,
                           const std::vector<uint32_t> &seg_level, const uint8_t *d_syms, const std::vector<uint64_t> &plane_off,
                           const std::vector<uint32_t> &nsym, uint32_t first)
{
	const std::vector<GenPlane> layout = general_plane_layout(m);
	// the planes that say which record every element names come down; the residual bytes stay where they are
	std::vector<std::vector<uint8_t>> host(layout.size());
	for (size_t q = 0; q < layout.size(); ++q) {
		if (layout[q].what == GP_DATA) continue;
		host[q].resize(nsym[first + q]);
		if (!host[q].empty()) HIP_OK(hipMemcpyAsync(host[q].data(), d_syms + plane_off[first + q], host[q].size(), hipMemcpyDeviceToHost, cx.stream));
	}
	HIP_OK(hipStreamSynchronize(cx.stream));
	GenHostPlanes hp;
	hp.lists.resize(m.lists.size());
	std::vector<size_t> data_plane0(m.lists.size(), 0);
	for (size_t q = 0; q < layout.size(); ++q) {
		const GenPlane &g = layout[q];
		const uint32_t n = nsym[first + q];
		switch (g.what) {
		case GP_REGV: hp.regv = host[q].data(); hp.n_regv = n; if (!hp.regv) hp.regv = (const uint8_t*)""; break;
		case GP_REGF: hp.regf = host[q].data(); hp.n_regf = n; if (!hp.regf) hp.regf = (const uint8_t*)""; break;
		case GP_TYPE: hp.lists[g.list].type = host[q].data(); hp.lists[g.list].n_type = n; break;
		case GP_GHIST:
			if (g.byte && n != hp.lists[g.list].n_gh) throw Error(HRY_E_FORMAT, "history planes of different length");
			hp.lists[g.list].gh[g.byte] = host[q].data(); hp.lists[g.list].n_gh = n; break;
		case GP_LHIST:
			if (g.byte && n != hp.lists[g.list].n_lh) throw Error(HRY_E_FORMAT, "history planes of different length");
			hp.lists[g.list].lh[g.byte] = host[q].data(); hp.lists[g.list].n_lh = n; break;
		default:
			if (g.byte == 0) { data_plane0[g.list] = first + q; hp.lists[g.list].n_data = n; }
			else if (n != hp.lists[g.list].n_data) throw Error(HRY_E_FORMAT, "residual planes of different length");
			break;
		}
	}
	std::vector<GenRecordEvents> ev;
	// A vertex list in which every vertex owns a record takes the PLY layout's chains, straight from the decoded planes -- and
	// BESIDE the host's bookkeeping of the other lists (which record every corner / face names: 6 ms per 180 000 triangles, as
	// long as the vertex chain): a helper thread drives the chain on copies of the connectivity and the list's records while this
	// thread reads the planes.  Whether the list qualifies is known from the planes' lengths (one residual symbol in the list's first
	// data plane per record coded as data).
	int fast_l = -1;
	if (m.bind.nregs_vtx() == 1 && m.bind.nvtxlists(0) == 1 && !env_on("HRY_GENERIC_VERTEX") && !order_v.empty()) {
		const int l = m.bind.vtxlist(0, 0);
		if (hp.lists[l].n_data == order_v.size() && m.lists[l].coded_bytes() > 0 && vertex_list_fast_applicable(m, l, order_v.size())) fast_l = l;
		// ... and from its reference kinds: every vertex must create its record (kind DATA).  A damaged stream whose data plane merely
		// has the right length would otherwise get a whole device reconstruction before the reader refuses it.
		if (fast_l >= 0) {
			const GenHostPlanes::L &P = hp.lists[l];
			bool all_data = P.n_type == order_v.size() && P.type != nullptr;
			for (uint32_t i = 0; all_data && i < P.n_type; ++i) all_data = P.type[i] == 0;
			if (!all_data) fast_l = -1;
		}
	}
	if (fast_l < 0) read_general_planes(m, order_v, hp, ev);
	else {
		Mesh t;
		t.nv = m.nv; t.nf = m.nf; t.declared_ne = m.declared_ne; t.have_degree = m.have_degree;   // (the connectivity itself is lent: both threads only read it)
		{
			BigVec<uint8_t> held;
			held.swap(m.lists[fast_l].data);
			t.lists[1] = m.lists[fast_l];      // the description; the records move
			t.lists[1].data.swap(held);
		}
		std::exception_ptr reader_error;
		const long long origin = trace_origin_ns();
		SideThreads chain;
		chain.spawn([&] { reconstruct_vertex_list_detached(cx, t, m, order_v, seg_start, seg_level, d_syms + plane_off[data_plane0[fast_l]], origin); });
		try { read_general_planes(m, order_v, hp, ev); } catch (...) { reader_error = std::current_exception(); }
		chain.join();
		t.lists[1].data.swap(m.lists[fast_l].data);
		if (reader_error) std::rethrow_exception(reader_error);   // (the reader's error wins over the chain's)
		chain.rethrow();
		ev[fast_l].he.clear(); ev[fast_l].slot.clear();
	}
	reconstruct_general(cx, m, order_v, ev, [&] {
		for (size_t l = 0; l < m.lists.size(); ++l) {
			const uint32_t nd = (uint32_t)ev[l].he.size();
			if (!nd || !m.lists[l].coded_bytes()) continue;
			launch_residuals_to_rec(cx.stream, d_syms + plane_off[data_plane0[l]], nd, make_list_desc(m.lists[l]), cx.d_rec[l].as<uint8_t>());
		}
	});
}

}   // namespace hry
