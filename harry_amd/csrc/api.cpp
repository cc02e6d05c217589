// C ABI of libharry_amd.so (include/harry_amd.h).  Thin: argument checks, exception -> status translation.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>

#include "device/context.hpp"
#include "device/result_build.hpp"

using namespace hry;

struct hry_ctx { Context cx; explicit hry_ctx(int d) : cx(d) {} };
struct hry_mesh { Mesh m; };
struct hry_plan { ShardPlan p; };
// the handles of the results with named buffers: one template over the result type, the member is `r` in every family
template <class R> struct ResultHandle { R r; };
struct hry_render : ResultHandle<RenderResult> {};
struct hry_edges : ResultHandle<EdgesResult> {};
struct hry_shells : ResultHandle<ShellsResult> {};
struct hry_orient : ResultHandle<OrientResult> {};
struct hry_tangents : ResultHandle<TangentsResult> {};
struct hry_creases : ResultHandle<CreasesResult> {};
struct hry_curvature : ResultHandle<CurvatureResult> {};
struct hry_bvh : ResultHandle<BvhResult> {};
struct hry_intersections : ResultHandle<IntersectionsResult> {};
struct hry_distortion : ResultHandle<DistortionResult> {};
struct hry_order : ResultHandle<std::unique_ptr<OrderResult>> {};   // (taken from the context whole: hry_order_take)
struct hry_sweep { SweepResult s; };
struct hry_rate_sweep { RateResult s; };
struct hry_walk {
	WalkResult w; uint32_t info[2]; std::vector<uint8_t> vplanes, fplanes; std::vector<uint32_t> seg_start, seg_level;
	mutable std::vector<uint8_t> op_sym, op_class;   // unpacked from w.op_sc on first request
	mutable std::vector<uint32_t> op_thr, op_cum;    // op_position_table, on first request
	mutable bool have_table = false;
	mutable std::vector<uint8_t> snap_section;       // the border snapshots as the chunked container's directory holds them, on first request
	std::map<std::string, std::vector<uint32_t>> tables;   // hry_analysis_tables: the arrays of a component analysis by name
	void table() const { if (!have_table) { op_position_table(w, op_thr, op_cum); have_table = true; } }
	void snapshots() const
	{
		if (!snap_section.empty() || w.snapshots.empty()) return;
		std::vector<RestartCounters> rc, sc;
		(void)select_restart_points(w.marks, w.named, rc, &w.snapshots, &sc);
		write_snapshot_section(w.snapshot_faces, w.snapshots, sc, snap_section);
	}
	void unpack_ops() const
	{
		if (op_sym.size() == w.op_sc.size()) return;
		op_sym.resize(w.op_sc.size()); op_class.resize(w.op_sc.size());
		for (size_t i = 0; i < w.op_sc.size(); ++i) { op_sym[i] = op_u8(w.op_sc[i]) & 7; op_class[i] = op_u8(w.op_sc[i]) >> 3; }
	}
};

static thread_local std::string g_last_error;

// the decode's buffers in HBM stop being the mesh's for hry_render_build (render.cpp) at the next call on the context, and at
// every call that changes the mesh
// ... and the numbering maps of an encode with HRY_FLAG_ORDER stop being hry_order_take's in the same way (order.cpp)
static void order_lost(hry_ctx *ctx) { if (ctx) { ctx->cx.order_token = 0; ctx->cx.want_order = false; ctx->cx.order.reset(); ctx->cx.order_lists.clear(); } }
static void touched(hry_ctx *ctx) { if (ctx) { ctx->cx.render_token = 0; order_lost(ctx); } }
static void touched(hry_mesh *m) { if (m) { m->m.render_token = 0; m->m.order_token = 0; } }
static std::atomic<uint64_t> g_order_tokens{ 1 };

template <typename F> static int guarded(F &&f)
{
	try { f(); return HRY_OK; }
	catch (const Error &e) { g_last_error = e.what(); return e.code; }
	catch (const std::bad_alloc &) { g_last_error = "out of memory"; return HRY_E_NOMEM; }
	catch (const std::exception &e) { g_last_error = e.what(); return HRY_E_INTERNAL; }
}
static uint8_t *dup_bytes(const std::vector<uint8_t> &v)
{
	uint8_t *p = (uint8_t*)malloc(v.size() ? v.size() : 1);
	if (!p) throw std::bad_alloc();
	if (!v.empty()) memcpy(p, v.data(), v.size());
	return p;
}

// ---- what the result handles share (context.hpp: DeviceResult; result_build.hpp).  r: the handle's result, nullptr for a null
// handle.  handle_get: *rows 0: no such buffer; *dev: its address, of a buffer without rows only where empty_has_address
// (hry_render_get gives it, the others give NULL: DESIGN.md 7e)
static int null_argument() { g_last_error = "null argument"; return HRY_E_ARG; }
static int handle_get(const DeviceResult *r, const char *name, const void **dev, uint64_t *rows, int *width, int *type, bool empty_has_address)
{
	if (!r || !name || !rows) return null_argument();
	const NamedBuf *b = r->find(name);
	*rows = b ? b->rows : 0;
	if (dev) *dev = b && (b->rows || empty_has_address) ? b->p : nullptr;
	if (width) *width = b ? b->width : 0;
	if (type) *type = b ? b->type : 0;
	return HRY_OK;
}
// what: what the handle calls a buffer, for the refusals; same_device: refuse a result on another device than the context's
static int handle_copy(hry_ctx *ctx, const DeviceResult *r, const char *name, const char *what, void *dst, int dst_is_device, bool same_device)
{
	if (!ctx || !r || !name) return null_argument();
	return guarded([&] { result_copy(ctx->cx, *r, name, what, dst, dst_is_device != 0, same_device); });
}
template <class R> static int handle_stat(const R *r, double *device_ms, uint64_t *uploaded_bytes)
{
	if (!r) return null_argument();
	if (device_ms) *device_ms = r->device_ms;
	if (uploaded_bytes) *uploaded_bytes = r->uploaded_bytes;
	return HRY_OK;
}
static int handle_summary(const TopologyResult *r, uint64_t *out, int n)
{
	if (!r || !out) return null_argument();
	for (int i = 0; i < n; ++i) out[i] = r->summary[i];
	return HRY_OK;
}
// a fresh handle H filled by build(H&); *out is NULL after every failure.  The builds leave the decode's token alone
template <class H, class F> static int handle_build(hry_ctx *ctx, bool have_arguments, H **out, F build)
{
	if (out) *out = nullptr;
	if (!ctx || !have_arguments || !out) return null_argument();
	order_lost(ctx);
	return guarded([&] {
		std::unique_ptr<H> h(new H());
		build(*h);
		*out = h.release();
	});
}
template <class R> static const R *result_of(const ResultHandle<R> *h) { return h ? &h->r : nullptr; }
static const OrderResult *result_of(const hry_order *o) { return o ? o->r.get() : nullptr; }
static uint64_t rows_of(const DeviceResult *r, const char *name) { const NamedBuf *b = r ? r->find(name) : nullptr; return b ? b->rows : 0; }   // (0: no such buffer)

extern "C" {

const char *hry_last_error(void) { return g_last_error.c_str(); }
int hry_abi_version(void) { return HRY_ABI_VERSION; }

int hry_device_count(void)
{
	int n = 0;
	return hipGetDeviceCount(&n) == hipSuccess && n > 0 ? n : 0;
}
int hry_ctx_create(int device, hry_ctx **out)
{
	if (!out) { g_last_error = "null argument"; return HRY_E_ARG; }
	*out = nullptr;
	return guarded([&] { *out = new hry_ctx(device); });
}
void hry_ctx_destroy(hry_ctx *ctx) { delete ctx; }
int hry_ctx_timing(const hry_ctx *ctx, hry_timing *out)
{
	if (!ctx || !out) { g_last_error = "null argument"; return HRY_E_ARG; }
	*out = ctx->cx.timing;
	return HRY_OK;
}
void *hry_ctx_stream(const hry_ctx *ctx) { return ctx ? (void*)ctx->cx.stream.s : nullptr; }   // (there since the context exists)

int hry_mesh_from_ply(const uint8_t *ply, size_t n, hry_mesh **out)
{
	if (!ply || !out) { g_last_error = "null argument"; return HRY_E_ARG; }
	*out = nullptr;
	return guarded([&] {
		std::unique_ptr<Mesh> m(mesh_from_ply(ply, n));
		*out = new hry_mesh{ std::move(*m) };
	});
}
int hry_mesh_from_arrays(uint32_t nv, const uint8_t *vrec, int v_ncomp, const uint8_t *v_types, const char *const *v_names,
                         uint32_t nf, const uint8_t *degrees, const uint32_t *indices,
                         const uint8_t *frec, int f_ncomp, const uint8_t *f_types, const char *const *f_names, hry_mesh **out)
{
	if (!out || (nf && (!degrees || !indices)) || (v_ncomp && (!v_types || !v_names || (nv && !vrec))) || (f_ncomp && (!f_types || !f_names || (nf && !frec)))) {
		g_last_error = "null argument";
		return HRY_E_ARG;
	}
	*out = nullptr;
	return guarded([&] {
		std::unique_ptr<Mesh> m(mesh_from_arrays(nv, vrec, v_ncomp, v_types, v_names, nf, degrees, indices, frec, f_ncomp, f_types, f_names));
		*out = new hry_mesh{ std::move(*m) };
	});
}
int hry_mesh_to_ply(const hry_mesh *m, int ascii, uint8_t **out, size_t *out_len)
{
	if (!m || !out || !out_len) { g_last_error = "null argument"; return HRY_E_ARG; }
	return guarded([&] {
		ByteSink v;
		mesh_to_ply(m->m, (ascii & HRY_PLY_ASCII) != 0, v, (ascii & HRY_PLY_PACKED) != 0);
		*out = v.release(out_len);
	});
}
int hry_mesh_from_obj(const uint8_t *obj, size_t n, const char *dir, hry_mesh **out)
{
	if (!obj || !out) { g_last_error = "null argument"; return HRY_E_ARG; }
	*out = nullptr;
	return guarded([&] {
		std::unique_ptr<Mesh> m(mesh_from_obj(obj, n, dir));
		*out = new hry_mesh{ std::move(*m) };
	});
}
int hry_mesh_to_obj(const hry_mesh *m, int, uint8_t **out, size_t *out_len)
{
	if (!m || !out || !out_len) { g_last_error = "null argument"; return HRY_E_ARG; }
	return guarded([&] {
		ByteSink v;
		mesh_to_obj(m->m, v);
		*out = v.release(out_len);
	});
}
int hry_mesh_general(const hry_mesh *m) { return m && m->m.general ? 1 : 0; }
int hry_list_target(const hry_mesh *m, int l) { return m && l >= 0 && (size_t)l < m->m.lists.size() ? m->m.lists[l].target : 3; }
int hry_mesh_nregions(const hry_mesh *m, int which)
{
	if (!m) return 0;
	if (!m->m.general) return 1;
	return which == 0 ? m->m.bind.nregs_face() : m->m.bind.nregs_vtx();
}
int hry_mesh_region_lists(const hry_mesh *m, int kind, int r, uint16_t *out, int cap)
{
	if (!m || r < 0) return 0;
	if (!m->m.general) { if (kind == 2 || r != 0) return 0; if (out && cap > 0) out[0] = kind == 0 ? 0 : 1; return 1; }
	const Bindings &b = m->m.bind;
	if (r >= (kind == 1 ? b.nregs_vtx() : b.nregs_face())) return 0;
	const int n = kind == 0 ? b.nfacelists(r) : kind == 1 ? b.nvtxlists(r) : b.ncornerlists(r);
	for (int a = 0; a < n && a < cap && out; ++a) out[a] = (uint16_t)(kind == 0 ? b.facelist(r, a) : kind == 1 ? b.vtxlist(r, a) : b.cornerlist(r, a));
	return n;
}
size_t hry_mesh_regions_of(const hry_mesh *m, int which, const uint16_t **out)
{
	if (!m || !out || !m->m.general) return 0;
	const BigVec<uint16_t> &v = which == 0 ? m->m.bind.face_reg : m->m.bind.vtx_reg;
	*out = v.data();
	return v.size();
}
size_t hry_mesh_bindings(const hry_mesh *m, int kind, const uint32_t **out, int *slots)
{
	if (!m || !out || !slots || !m->m.general) return 0;
	const Bindings &b = m->m.bind;
	const BigVec<uint32_t> &v = kind == 0 ? b.face_attr : kind == 1 ? b.vtx_attr : b.corner_attr;
	*slots = kind == 0 ? b.nb_face : kind == 1 ? b.nb_vtx : b.nb_corner;
	*out = v.data();
	return kind == 0 ? m->m.nf : kind == 1 ? m->m.nv : m->m.ne();
}
void hry_mesh_free(hry_mesh *m) { delete m; }
hry_mesh *hry_mesh_clone(const hry_mesh *m)
{
	if (!m) return nullptr;
	try { hry_mesh *c = new hry_mesh{ m->m }; c->m.device_token = 0; c->m.render_token = 0; c->m.order_token = 0; return c; }
	catch (...) { g_last_error = "out of memory"; return nullptr; }
}

uint32_t hry_mesh_nv(const hry_mesh *m) { return m->m.nv; }
uint32_t hry_mesh_nf(const hry_mesh *m) { return m->m.nf; }
uint32_t hry_mesh_ne(const hry_mesh *m) { return m->m.ne(); }
uint64_t hry_mesh_ntri(const hry_mesh *m) { return m->m.ntri(); }
const uint32_t *hry_mesh_face_offsets(const hry_mesh *m) { return m->m.face_off.data(); }
const uint32_t *hry_mesh_org(const hry_mesh *m) { return m->m.org.data(); }
const uint32_t *hry_mesh_twin(const hry_mesh *m)
{
	try { ensure_twins(m->m); } catch (...) { return nullptr; }
	return m->m.twin.data();
}
int hry_mesh_nlists(const hry_mesh *m) { return (int)m->m.lists.size(); }
int hry_list_ncomp(const hry_mesh *m, int l) { return m->m.lists[l].ncomp(); }
uint32_t hry_list_count(const hry_mesh *m, int l) { return m->m.lists[l].count; }
int hry_list_stride(const hry_mesh *m, int l) { return m->m.lists[l].stride(); }
int hry_list_type(const hry_mesh *m, int l, int c) { return m->m.lists[l].type[c]; }
int hry_list_quant(const hry_mesh *m, int l, int c) { return m->m.lists[l].quant[c]; }
int hry_list_offset(const hry_mesh *m, int l, int c) { return m->m.lists[l].offset[c]; }
int hry_list_interp_ncomp(const hry_mesh *m, int l, int interp)
{
	if (!m || l < 0 || (size_t)l >= m->m.lists.size() || interp < 0 || (size_t)interp >= m->m.lists[l].interp_len.size()) return 0;
	return m->m.lists[l].interp_len[interp];
}
int hry_list_interp_offset(const hry_mesh *m, int l, int interp)
{
	if (!hry_list_interp_ncomp(m, l, interp)) return -1;
	return m->m.lists[l].interp_off[interp];
}
const uint8_t *hry_list_data(const hry_mesh *m, int l) { return m->m.lists[l].data.data(); }
const uint8_t *hry_list_min(const hry_mesh *m, int l) { return m->m.lists[l].have_bounds ? m->m.lists[l].bmin.data() : nullptr; }
const uint8_t *hry_list_max(const hry_mesh *m, int l) { return m->m.lists[l].have_bounds ? m->m.lists[l].bmax.data() : nullptr; }

int hry_bounds(hry_ctx *ctx, hry_mesh *m)
{
	if (!ctx || !m) { g_last_error = "null argument"; return HRY_E_ARG; }
	touched(ctx); touched(m);
	return guarded([&] { device_bounds(ctx->cx, m->m); });
}
int hry_requant(hry_ctx *ctx, hry_mesh *m, const hry_quant *q, size_t nq, int clear)
{
	if (!ctx || !m || (nq && !q)) { g_last_error = "null argument"; return HRY_E_ARG; }
	touched(ctx); touched(m);
	return guarded([&] { device_requant(ctx->cx, m->m, q, nq, clear != 0); });
}
int hry_mesh_upload(hry_ctx *ctx, hry_mesh *m)
{
	if (!ctx || !m) { g_last_error = "null argument"; return HRY_E_ARG; }
	touched(ctx); touched(m);
	return guarded([&] { if (m->m.general) upload_general(ctx->cx, m->m); else ctx->cx.upload_mesh(m->m); });
}
int hry_encode(hry_ctx *ctx, hry_mesh *m, const hry_opts *opts, uint8_t **out, size_t *out_len)
{
	if (!ctx || !m || !out || !out_len) { g_last_error = "null argument"; return HRY_E_ARG; }
	*out = nullptr; *out_len = 0;
	touched(ctx); touched(m);
	return guarded([&] {
		hry_opts o = opts ? *opts : hry_opts{};
		ctx->cx.keep_stages = o.keep_stages != 0;
		ctx->cx.device_recurrence = (o.flags & HRY_FLAG_DEVICE_RECURRENCE) != 0;
		ctx->cx.stages.clear();
		if (o.flags & HRY_FLAG_ORDER) {
			if (m->m.shard.active() || !m->m.shard.seeds.empty()) throw Error(HRY_E_UNSUPPORTED, "HRY_FLAG_ORDER on a shard: the numbering maps describe a whole mesh");
			ctx->cx.want_order = true;
		}
		// the maps are the last thing an encode with the flag builds (order_build): on success ctx and m share a token until the next
		// call on either; an encode that throws leaves none
		struct OrderMark {
			hry_ctx *ctx; hry_mesh *m; bool ok = false;
			~OrderMark()
			{
				if (ok && ctx->cx.order) ctx->cx.order_token = m->m.order_token = g_order_tokens.fetch_add(1, std::memory_order_relaxed);
				else order_lost(ctx);
				ctx->cx.want_order = false;
				ctx->cx.order_lists.clear();
			}
		} mark{ ctx, m };
		if (o.profile == HRY_PROFILE_CHUNKED) {
			// straight into the buffer the caller gets: a vector first cost a zero fill, a second set of fresh pages and a copy --
			// 10 ms of a 75 ms encode of the 12.6 M-triangle share of configs[3] (39 MB of container)
			ByteSink sink;
			encode_chunked(ctx->cx, m->m, o.chunk_syms, sink);
			*out = sink.release(out_len);
			mark.ok = true;
			return;
		}
		std::vector<uint8_t> v;
		if (o.profile == HRY_PROFILE_COMPAT) encode_compat(ctx->cx, m->m, v);
		else throw Error(HRY_E_ARG, "unknown profile");
		*out = dup_bytes(v);
		*out_len = v.size();
		mark.ok = true;
	});
}
int hry_decode(hry_ctx *ctx, const uint8_t *hry, size_t n, const hry_opts *opts, hry_mesh **out)
{
	if (!ctx || !hry || !out) { g_last_error = "null argument"; return HRY_E_ARG; }
	*out = nullptr;
	touched(ctx);   // (the decode marks what it leaves in HBM: mark_decoded)
	return guarded([&] {
		hry_opts o = opts ? *opts : hry_opts{};
		ctx->cx.keep_stages = o.keep_stages != 0;
		ctx->cx.stages.clear();
		std::unique_ptr<Mesh> m(decode_any(ctx->cx, hry, n, o.shard_index, o.shard_count, (o.flags & HRY_FLAG_PARTIAL) != 0));
		*out = new hry_mesh{ std::move(*m) };
	});
}
int hry_encode_sharded(hry_ctx *const *ctx, int n_ctx, hry_mesh *m, const hry_quant *quant, size_t n_quant, int clear,
                       const hry_opts *opts, uint8_t **out, size_t *out_len, hry_shard_timing *timing)
{
	if (!ctx || n_ctx <= 0 || !m || !out || !out_len || (n_quant && !quant)) { g_last_error = "null argument"; return HRY_E_ARG; }
	*out = nullptr; *out_len = 0;
	for (int i = 0; i < n_ctx; ++i) touched(ctx[i]);
	touched(m);
	return guarded([&] {
		hry_opts o = opts ? *opts : hry_opts{};
		o.profile = opts ? o.profile : HRY_PROFILE_CHUNKED;
		if (o.flags & HRY_FLAG_ORDER) throw Error(HRY_E_UNSUPPORTED, "HRY_FLAG_ORDER with hry_encode_sharded: the numbering maps of a sharded encode are not built");
		if (o.profile != HRY_PROFILE_CHUNKED) throw Error(HRY_E_UNSUPPORTED, "the reference's single stream (compat) does not shard: one recurrence over the whole file");
		std::vector<Context*> cxs;
		for (int i = 0; i < n_ctx; ++i) { if (!ctx[i]) throw Error(HRY_E_ARG, "null context"); ctx[i]->cx.keep_stages = false; ctx[i]->cx.stages.clear(); cxs.push_back(&ctx[i]->cx); }
		ByteSink v;
		hry_shard_timing st{};
		encode_sharded(cxs.data(), n_ctx, m->m, quant, n_quant, clear != 0, o.shard_count, o.chunk_syms, v, st, (o.flags & HRY_FLAG_KEEP_MESH) == 0);
		if (timing) *timing = st;
		*out = v.release(out_len);
	});
}
int hry_decode_sharded(hry_ctx *const *ctx, int n_ctx, const uint8_t *hry, size_t n, const hry_opts *opts, hry_mesh **out, hry_shard_timing *timing)
{
	if (!ctx || n_ctx <= 0 || !hry || !out) { g_last_error = "null argument"; return HRY_E_ARG; }
	*out = nullptr;
	for (int i = 0; i < n_ctx; ++i) touched(ctx[i]);
	return guarded([&] {
		hry_opts o = opts ? *opts : hry_opts{};
		std::vector<Context*> cxs;
		for (int i = 0; i < n_ctx; ++i) { if (!ctx[i]) throw Error(HRY_E_ARG, "null context"); ctx[i]->cx.keep_stages = false; ctx[i]->cx.stages.clear(); cxs.push_back(&ctx[i]->cx); }
		std::unique_ptr<Mesh> g(new Mesh());
		int minor = 0;
		const bool sharded = n >= 6 && hry[4] == 0 && hry[5] == 3;
		if (!sharded) {   // an unsharded file: the first context decodes it
			std::unique_ptr<Mesh> m(decode_any(*cxs[0], hry, n, 0, 0, false));
			if (timing) { *timing = hry_shard_timing{}; timing->n_contexts = 1; timing->n_segments = 1; timing->total_ms = cxs[0]->timing.total_ms; }
			*out = new hry_mesh{ std::move(*m) };
			return;
		}
		const size_t hdr = read_hry_header(hry, n, *g, minor, false);
		std::unique_ptr<Mesh> m(decode_sharded(cxs.data(), n_ctx, hry, n, hdr, std::move(g), o.shard_index, o.shard_count,
		                                       (o.flags & HRY_FLAG_PARTIAL) != 0 || o.shard_count > 1, timing));
		*out = new hry_mesh{ std::move(*m) };
	});
}
int hry_container_check(const uint8_t *hry, size_t n, int *complete)
{
	if (!hry) { g_last_error = "null argument"; return HRY_E_ARG; }
	if (complete) *complete = 0;
	return guarded([&] {
		Mesh m;
		int minor = 0;
		const size_t hdr = read_hry_header(hry, n, m, minor, false);
		if (minor != 3) { if (complete) *complete = 1; return; }
		ShardedDirectory dir;
		std::vector<uint32_t> counts;
		for (const AttrList &L : m.lists) counts.push_back(L.count);
		parse_sharded_directory(hry, n, hdr, m.nv, m.nf, m.declared_ne, dir, true, m.general ? &counts : nullptr);
		if (complete) *complete = dir.complete ? 1 : 0;
	});
}
int hry_mesh_partial(const hry_mesh *m) { return m && m->m.partial ? 1 : 0; }
void hry_free(void *p) { BlockPool::give(p); }   // (a block of the recycling pool goes back to it, anything else to the C library)
int hry_container_info(const uint8_t *hry, size_t n, uint32_t info[8])
{
	if (!hry || !info) { g_last_error = "null argument"; return HRY_E_ARG; }
	return guarded([&] {
		Mesh m;
		int minor = 0;
		const size_t hdr = read_hry_header(hry, n, m, minor, false);
		for (int i = 0; i < 8; ++i) info[i] = 0;
		info[0] = (uint32_t)minor; info[1] = (uint32_t)hdr; info[2] = m.nv; info[3] = m.nf; info[4] = m.declared_ne; info[7] = 1;
		size_t body = hdr;
		if (minor == 3) {
			ShardedDirectory dir;
			std::vector<uint32_t> counts;
			for (const AttrList &L : m.lists) counts.push_back(L.count);
			parse_sharded_directory(hry, n, hdr, m.nv, m.nf, m.declared_ne, dir, true, m.general ? &counts : nullptr);
			info[7] = (uint32_t)dir.segments.size();
			if (dir.segments.empty()) return;
			body = dir.segments[0].offset + dir.segments[0].body_at;   // (general bindings: runs carry their record ranges)
		}
		if (minor >= 2) {
			if (n < body + 8) throw Error(HRY_E_FORMAT, "truncated chunked directory");
			memcpy(&info[5], hry + body, 4); memcpy(&info[6], hry + body + 4, 4);
		}
	});
}

int hry_shard_plan(const hry_mesh *m, int n_shards, hry_plan **out)
{
	if (!m || !out || n_shards <= 0) { g_last_error = "invalid argument"; return HRY_E_ARG; }
	*out = nullptr;
	return guarded([&] {
		std::unique_ptr<hry_plan> p(new hry_plan());
		shard_plan(m->m, (uint32_t)n_shards, p->p);
		*out = p.release();
	});
}
void hry_plan_free(hry_plan *p) { delete p; }
int hry_walk_run_shard(hry_mesh *m, const hry_plan *p, int shard, hry_walk **out)
{
	if (!m || !p || !out || shard < 0) { g_last_error = "invalid argument"; return HRY_E_ARG; }
	*out = nullptr;
	return guarded([&] {
		std::unique_ptr<hry_walk> w(new hry_walk());
		check_codable(m->m);
		ensure_twins(m->m);
		if (p->p.g_nv != m->m.nv || p->p.g_nf != m->m.nf || p->p.g_ne != m->m.ne()) throw Error(HRY_E_ARG, "the plan belongs to another mesh");
		ComponentAnalysis part;
		ShardInfo info;
		shard_components(p->p, (uint32_t)shard, part, info);
		int ud = 0;
		const bool uniform = m->m.uniform_degree(ud) && (ud == 3 || ud == 4);
		BigVec<uint32_t> eface;
		if (!uniform && p->p.A.eface.size() != m->m.ne()) {
			eface.resize(m->m.ne());
			for (uint32_t f = 0; f < m->m.nf; ++f) for (uint32_t h = m->m.face_off[f]; h < m->m.face_off[f + 1]; ++h) eface[h] = f;
		}
		WalkState marks(m->m.nv, m->m.nf);
		{ uint64_t nfs = 0; for (uint32_t k = 0; k < part.ncomp; ++k) nfs += part.n_faces[k]; w->w.snapshot_faces = snapshot_spacing((uint32_t)nfs); }   // (what an encode of the shard asks for)
		cut_border_walk_in_place(m->m, part, uniform ? nullptr : eface.empty() ? p->p.A.eface.data() : eface.data(), marks, w->w);
		w->info[0] = w->w.n_conn; w->info[1] = w->w.numtri_coded ? 1 : 0;
		*out = w.release();
	});
}
int hry_analysis_check(hry_ctx *ctx, hry_mesh *m)
{
	if (!ctx || !m) { g_last_error = "invalid argument"; return HRY_E_ARG; }
	touched(ctx); touched(m);
	return guarded([&] {
		check_codable(m->m);
		if (m->m.general || !m->m.shard.seeds.empty()) throw Error(HRY_E_ARG, "analysis check: a mesh in the PLY layout that is not a shard");
		if (m->m.device_token == 0 || m->m.device_token != ctx->cx.resident_token) ctx->cx.upload_mesh(m->m);
		ComponentAnalysis D, H;
		device_component_analysis(ctx->cx, m->m, D);
		analyse_components(m->m, H);
		if (D.ncomp != H.ncomp) throw Error(HRY_E_INTERNAL, "analysis: " + std::to_string(D.ncomp) + " components on the device, " + std::to_string(H.ncomp) + " on the host");
		if (D.ncomp < 2) return;
		auto same = [&](const char *what, const std::vector<uint32_t> &d, const std::vector<uint32_t> &h) {
			if (d.size() != h.size()) throw Error(HRY_E_INTERNAL, std::string("analysis: size of ") + what);
			for (size_t i = 0; i < d.size(); ++i)
				if (d[i] != h[i]) throw Error(HRY_E_INTERNAL, std::string("analysis: ") + what + "[" + std::to_string(i) + "] = " + std::to_string(d[i]) + " on the device, " + std::to_string(h[i]) + " on the host");
		};
		same("seed", D.seed, H.seed); same("n_faces", D.n_faces, H.n_faces); same("n_halfedges", D.n_halfedges, H.n_halfedges);
		same("fresh", D.fresh, H.fresh); same("group", D.group, H.group);
		same("face_lo", D.face_lo, H.face_lo); same("face_hi", D.face_hi, H.face_hi); same("vtx_lo", D.vtx_lo, H.vtx_lo); same("vtx_hi", D.vtx_hi, H.vtx_hi);
		// (component NUMBERS are the roots' order in both: by_rank / rank_of agree too)
		same("by_rank", D.by_rank, H.by_rank);
	});
}
int hry_analysis_tables(hry_ctx *ctx, hry_mesh *m, int on_device, hry_walk **out)
{
	if (!m || !out || (on_device && !ctx)) { g_last_error = "invalid argument"; return HRY_E_ARG; }
	*out = nullptr;
	if (on_device) touched(ctx);
	touched(m);
	return guarded([&] {
		std::unique_ptr<hry_walk> w(new hry_walk());
		check_codable(m->m);
		if (m->m.general || !m->m.shard.seeds.empty()) throw Error(HRY_E_ARG, "analysis tables: a mesh in the PLY layout that is not a shard");
		ComponentAnalysis A;
		if (on_device) {
			if (m->m.device_token == 0 || m->m.device_token != ctx->cx.resident_token) ctx->cx.upload_mesh(m->m);
			device_component_analysis(ctx->cx, m->m, A, true);
			w->tables["twin_over"] = { m->m.twin_over };
		} else analyse_components(m->m, A);
		auto &T = w->tables;
		T["ncomp"] = { A.ncomp };
		T["by_rank"] = A.by_rank; T["seed"] = A.seed; T["n_faces"] = A.n_faces; T["n_halfedges"] = A.n_halfedges; T["fresh"] = A.fresh; T["group"] = A.group;
		T["face_lo"] = A.face_lo; T["face_hi"] = A.face_hi; T["vtx_lo"] = A.vtx_lo; T["vtx_hi"] = A.vtx_hi;
		T["comp"].assign(A.comp.begin(), A.comp.end());
		start_face_spans(m->m.nf, T["spans"]);
		*out = w.release();
	});
}
uint32_t hry_plan_ncomponents(const hry_plan *p) { return p ? p->p.A.ncomp : 0; }
uint32_t hry_plan_ngroups(const hry_plan *p)
{
	uint32_t n = 0;
	if (p) for (uint32_t k = 0; k < p->p.A.ncomp; ++k) n += p->p.A.group[k] == k;
	return n;
}
uint64_t hry_plan_triangles(const hry_plan *p, int shard) { return p && shard >= 0 && (uint32_t)shard < p->p.n_shards ? p->p.shard_triangles[shard] : 0; }
int hry_shard_extract(const hry_mesh *m, const hry_plan *p, int shard, hry_mesh **out)
{
	if (!m || !p || !out || shard < 0) { g_last_error = "invalid argument"; return HRY_E_ARG; }
	*out = nullptr;
	return guarded([&] {
		std::unique_ptr<Mesh> s(shard_extract(m->m, p->p, (uint32_t)shard));
		*out = new hry_mesh{ std::move(*s) };
	});
}
int hry_merge(const uint8_t *const *parts, const size_t *sizes, size_t n, uint8_t **out, size_t *out_len)
{
	if (!parts || !sizes || !out || !out_len) { g_last_error = "null argument"; return HRY_E_ARG; }
	*out = nullptr; *out_len = 0;
	return guarded([&] {
		ByteSink v;
		merge_containers(parts, sizes, n, v);
		*out = v.release(out_len);
	});
}
size_t hry_mesh_runs(const hry_mesh *m, const uint32_t **runs)
{
	if (!m || !runs) return 0;
	const std::vector<ShardRun> &r = m->m.shard.active() ? m->m.shard.runs : m->m.covered;
	*runs = (const uint32_t*)r.data();
	return r.size();
}
size_t hry_shard_elements(const hry_mesh *m, int which, const uint32_t **idx)
{
	if (!m || !idx) return 0;
	if (which >= 16) {   // general bindings: input index in the whole mesh of every record of list which - 16
		if ((size_t)(which - 16) >= m->m.shard.record_of.size()) return 0;
		*idx = m->m.shard.record_of[which - 16].data();
		return m->m.shard.record_of[which - 16].size();
	}
	const std::vector<uint32_t> &v = which == 2 ? m->m.shard.seeds : which ? m->m.shard.vertex_of : m->m.shard.face_of;
	*idx = v.data();
	return v.size();
}
int hry_list_set_bounds(hry_mesh *m, int l, const uint8_t *min_rec, const uint8_t *max_rec)
{
	touched(m);
	if (!m || l < 0 || (size_t)l >= m->m.lists.size() || !min_rec || !max_rec) { g_last_error = "invalid argument"; return HRY_E_ARG; }
	AttrList &L = m->m.lists[l];
	for (int c = 0; c < L.ncomp(); ++c) if (L.quant[c]) { g_last_error = "bounds of an already quantised list come from its header"; return HRY_E_ARG; }
	L.bmin.assign(min_rec, min_rec + L.stride());
	L.bmax.assign(max_rec, max_rec + L.stride());
	L.bmin_at.clear(); L.bmax_at.clear();
	L.have_bounds = true;
	return HRY_OK;
}
uint32_t hry_list_min_at(const hry_mesh *m, int l, int c) { return m && l >= 0 && (size_t)l < m->m.lists.size() && c >= 0 && (size_t)c < m->m.lists[l].bmin_at.size() ? m->m.lists[l].bmin_at[c] : 0; }
uint32_t hry_list_max_at(const hry_mesh *m, int l, int c) { return m && l >= 0 && (size_t)l < m->m.lists.size() && c >= 0 && (size_t)c < m->m.lists[l].bmax_at.size() ? m->m.lists[l].bmax_at[c] : 0; }

int hry_stage_get(hry_ctx *ctx, const char *name, void **host_copy, size_t *bytes)
{
	if (!ctx || !name || !host_copy || !bytes) { g_last_error = "null argument"; return HRY_E_ARG; }
	auto it = ctx->cx.stages.find(name);
	if (it == ctx->cx.stages.end()) { g_last_error = std::string("no such stage: ") + name; return HRY_E_ARG; }
	return guarded([&] { *host_copy = dup_bytes(it->second); *bytes = it->second.size(); });
}
int hry_walk_run(hry_mesh *m, hry_walk **out)
{
	if (!m || !out) { g_last_error = "null argument"; return HRY_E_ARG; }
	*out = nullptr;
	return guarded([&] {
		std::unique_ptr<hry_walk> w(new hry_walk());
		check_codable(m->m);
		cut_border_walk(m->m, w->w);
		w->info[0] = w->w.n_conn; w->info[1] = w->w.numtri_coded ? 1 : 0;
		*out = w.release();
	});
}
int hry_walk_run_plain(hry_mesh *m, hry_walk **out)
{
	if (!m || !out) { g_last_error = "null argument"; return HRY_E_ARG; }
	*out = nullptr;
	return guarded([&] {
		std::unique_ptr<hry_walk> w(new hry_walk());
		check_codable(m->m);
		w->w.snapshot_faces = snapshot_spacing(m->m.nf);   // (what a chunked encode asks for)
		cut_border_walk(m->m, w->w, false);
		w->info[0] = w->w.n_conn; w->info[1] = w->w.numtri_coded ? 1 : 0;
		*out = w.release();
	});
}
size_t hry_walk_get(const hry_walk *w, const char *name, const void **ptr)
{
	if (!w || !name || !ptr) return 0;
	std::string n(name);
	const WalkResult &r = w->w;
	auto ret = [&](const auto &v) { *ptr = v.data(); return v.size(); };
	if (n == "order_v") return ret(r.order_v);
	if (n == "order_f") return ret(r.order_f);
	if (n == "op_sym") { w->unpack_ops(); return ret(w->op_sym); }
	if (n == "op_class") { w->unpack_ops(); return ret(w->op_class); }
	if (n == "op_l") return ret(r.op_l);
	if (n == "op_h") return ret(r.op_h);
	if (n == "op_t") return ret(r.op_t);
	if (n == "op_pos") return ret(r.op_pos);
	if (n == "op_thr") { w->table(); return ret(w->op_thr); }   // where the connectivity groups sit between the operations (what the
	if (n == "op_cum") { w->table(); return ret(w->op_cum); }   // device's operation model places its records with)
	if (n == "info") { *ptr = w->info; return 2; }
	if (n == "snap_section") { w->snapshots(); return ret(w->snap_section); }
	if (n == "marks") { *ptr = r.marks.data(); return r.marks.size() * (sizeof(ComponentMark) / 4); }
	if (n == "seg_start") return ret(w->seg_start);
	if (n == "seg_level") return ret(w->seg_level);
	if (n == "vplanes") return ret(w->vplanes);
	if (n == "fplanes") return ret(w->fplanes);
	if (n.size() == 8 && n.compare(0, 3, "grp") == 0 && n[3] >= '0' && n[3] < '0' + G_COUNT) {
		int g = n[3] - '0';
		if (n.compare(4, 4, "_val") == 0) return ret(r.grp_val[g]);
		if (n.compare(4, 4, "_pos") == 0) return ret(r.grp_pos[g]);
	}
	if (auto it = w->tables.find(n); it != w->tables.end()) return ret(it->second);
	*ptr = nullptr;
	return 0;
}
void hry_walk_free(hry_walk *w) { delete w; }

int hry_stream_read_host(const void *hry, size_t bytes, hry_mesh **mesh, hry_walk **out)
{
	if (!hry || !mesh || !out) { g_last_error = "null argument"; return HRY_E_ARG; }
	*mesh = nullptr; *out = nullptr;
	return guarded([&] {
		std::unique_ptr<hry_mesh> m(new hry_mesh());
		std::unique_ptr<hry_walk> w(new hry_walk());
		int minor = 0;
		size_t hdr = read_hry_header((const uint8_t*)hry, bytes, m->m, minor);
		if (minor != 1) throw Error(HRY_E_ARG, "not a single-stream (v0.1) file");
		if (m->m.general) throw Error(HRY_E_UNSUPPORTED, "hry_stream_read_host returns the planes of the PLY layout only");
		std::vector<uint32_t> seg_start, seg_level;
		OrderVec order_v;
		read_compat_stream((const uint8_t*)hry + hdr, bytes - hdr, m->m, order_v, seg_start, seg_level, w->vplanes, w->fplanes);
		w->w.order_v.assign(order_v.begin(), order_v.end());
		w->info[0] = w->info[1] = 0;
		*mesh = m.release();
		*out = w.release();
	});
}

int hry_walk_replay(const hry_mesh *src, const hry_walk *walk, int use_restart_points, hry_mesh **mesh, hry_walk **out)
{
	if (!src || !walk || !mesh || !out) { g_last_error = "null argument"; return HRY_E_ARG; }
	*mesh = nullptr; *out = nullptr;
	return guarded([&] {
		const WalkResult &r = walk->w;
		std::vector<uint8_t> planes[kConnPlanes];   // the chunked container's connectivity planes, built on the host
		walk_conn_planes(r, planes);
		std::unique_ptr<hry_mesh> m(new hry_mesh());
		std::unique_ptr<hry_walk> w(new hry_walk());
		m->m.nv = src->m.nv; m->m.nf = src->m.nf; m->m.declared_ne = src->m.ne(); m->m.have_degree = src->m.have_degree;
		// use_restart_points: 1 the restart points at component starts, 3 also the border snapshots inside components -- through the
		// directory's form and back, as a decoder receives them (the counters of a span depend on which points exist: never the snapshots alone)
		std::vector<RestartPoint> restarts;
		std::vector<RestartCounters> rcounters, scounters;
		std::vector<SnapshotPoint> snaps;
		const bool with_snaps = (use_restart_points & 2) != 0 && !r.snapshots.empty();
		if (use_restart_points & 3) restarts = select_restart_points(r.marks, r.named, rcounters, with_snaps ? &r.snapshots : nullptr, with_snaps ? &scounters : nullptr);
		if (use_restart_points == 2) throw Error(HRY_E_ARG, "replay: border snapshots go with the restart points");
		if (with_snaps) {
			std::vector<uint8_t> sec;
			write_snapshot_section(r.snapshot_faces, r.snapshots, scounters, sec);
			uint32_t spacing = 0;
			if (read_snapshot_section(sec.data(), sec.size(), m->m.nv, spacing, snaps) != sec.size() || spacing != r.snapshot_faces) throw Error(HRY_E_INTERNAL, "border snapshots: the section does not read back");
		}
		OrderVec order_v;
		PlaneView views[kConnPlanes];
		for (int k = 0; k < kConnPlanes; ++k) views[k] = PlaneView(planes[k]);
		cut_border_replay(m->m, views, restarts, rcounters, order_v, w->seg_start, w->seg_level, nullptr, with_snaps ? &snaps : nullptr);
		w->w.order_v.assign(order_v.begin(), order_v.end());
		w->info[0] = (uint32_t)restarts.size(); w->info[1] = (uint32_t)snaps.size();
		*mesh = m.release();
		*out = w.release();
	});
}

int hry_range_encode_lht(hry_ctx *ctx, const uint64_t *lht, size_t n, uint8_t **out, size_t *out_len)
{
	if (!ctx || (n && !lht) || !out || !out_len) { g_last_error = "null argument"; return HRY_E_ARG; }
	touched(ctx);
	return guarded([&] {
		std::vector<uint8_t> v;
		range_encode_lht(ctx->cx, lht, n, v);
		*out = dup_bytes(v);
		*out_len = v.size();
	});
}

// ---- render-ready device buffers (render.cpp)
int hry_render_build(hry_ctx *ctx, const hry_mesh *m, hry_render **out) { return hry_render_build_ex(ctx, m, 0, out); }
int hry_render_build_ex(hry_ctx *ctx, const hry_mesh *m, uint32_t flags, hry_render **out)
{
	return handle_build(ctx, m != nullptr, out, [&](hry_render &r) { render_build(ctx->cx, m->m, flags, r.r); });
}
uint32_t hry_render_nverts(const hry_render *r) { return r ? r->r.nverts : 0; }
uint64_t hry_render_ntris(const hry_render *r) { return r ? r->r.ntris : 0; }
int hry_render_get(const hry_render *r, const char *name, const void **dev, uint64_t *rows, int *width, int *type) { return handle_get(result_of(r), name, dev, rows, width, type, true); }
int hry_render_copy(hry_ctx *ctx, const hry_render *r, const char *name, void *dst, int dst_is_device) { return handle_copy(ctx, result_of(r), name, "render buffer", dst, dst_is_device, false); }
int hry_render_stat(const hry_render *r, double *device_ms, uint64_t *uploaded_bytes) { return handle_stat(result_of(r), device_ms, uploaded_bytes); }
void hry_render_free(hry_render *r) { delete r; }

// ---- the eight families behind a render build.  Their get, copy, summary, stat and free are one line each: the family, what its
// refusals call a buffer, the words of its summary.  What differs between them follows: build, count, and what only one has
#define HRY_RESULT_FAMILY(fam, noun, nsummary) \
	int hry_##fam##_get(const hry_##fam *h, const char *name, const void **dev, uint64_t *rows, int *width, int *type) { return handle_get(result_of(h), name, dev, rows, width, type, false); } \
	int hry_##fam##_copy(hry_ctx *ctx, const hry_##fam *h, const char *name, void *dst, int dst_is_device) { return handle_copy(ctx, result_of(h), name, noun, dst, dst_is_device, true); } \
	int hry_##fam##_summary(const hry_##fam *h, uint64_t out[nsummary]) { return handle_summary(result_of(h), out, nsummary); } \
	int hry_##fam##_stat(const hry_##fam *h, double *device_ms, uint64_t *uploaded_bytes) { return handle_stat(result_of(h), device_ms, uploaded_bytes); } \
	void hry_##fam##_free(hry_##fam *h) { delete h; }
HRY_RESULT_FAMILY(edges, "edge buffer", 4)
HRY_RESULT_FAMILY(shells, "shell buffer", 6)
HRY_RESULT_FAMILY(orient, "orientation buffer", 6)
HRY_RESULT_FAMILY(tangents, "tangent buffer", 6)
HRY_RESULT_FAMILY(creases, "crease buffer", 6)
HRY_RESULT_FAMILY(curvature, "curvature buffer", 6)
HRY_RESULT_FAMILY(bvh, "bvh buffer", 6)
HRY_RESULT_FAMILY(intersections, "intersection buffer", 6)
#undef HRY_RESULT_FAMILY

// unique edges and adjacency of a render build (edges.cpp)
int hry_edges_build(hry_ctx *ctx, const hry_mesh *m, const hry_render *r, uint32_t flags, hry_edges **out)
{
	return handle_build(ctx, m && r, out, [&](hry_edges &h) { edges_build(ctx->cx, m->m, r->r, flags, h.r); });
}
uint64_t hry_edges_count(const hry_edges *e) { return e ? e->r.summary[0] : 0; }
// shells of a render build behind its edges build (shells.cpp)
int hry_shells_build(hry_ctx *ctx, const hry_mesh *m, const hry_render *r, const hry_edges *e, uint32_t flags, hry_shells **out)
{
	return handle_build(ctx, m && r && e, out, [&](hry_shells &h) { shells_build(ctx->cx, m->m, r->r, e->r, flags, h.r); });
}
uint64_t hry_shells_count(const hry_shells *s) { return s ? s->r.summary[0] : 0; }
// a consistent winding per patch of a render build behind its edges build (orient.cpp)
int hry_orient_build(hry_ctx *ctx, const hry_mesh *m, const hry_render *r, const hry_edges *e, uint32_t flags, hry_orient **out)
{
	return handle_build(ctx, m && r && e, out, [&](hry_orient &h) { orient_build(ctx->cx, m->m, r->r, e->r, flags, h.r); });
}
uint64_t hry_orient_count(const hry_orient *o) { return o ? o->r.summary[0] : 0; }
// tangent frames of a render build (tangents.cpp)
int hry_tangents_build(hry_ctx *ctx, const hry_mesh *m, const hry_render *r, uint32_t flags, hry_tangents **out)
{
	return handle_build(ctx, m && r, out, [&](hry_tangents &h) { tangents_build(ctx->cx, m->m, r->r, flags, h.r); });
}
uint64_t hry_tangents_count(const hry_tangents *t) { return t ? t->r.summary[0] : 0; }
// hard edges and split normals of a render build (creases.cpp)
int hry_creases_build(hry_ctx *ctx, const hry_mesh *m, const hry_render *r, const hry_edges *e, double cos_limit, uint32_t flags, hry_creases **out)
{
	return handle_build(ctx, m && r && e, out, [&](hry_creases &h) { creases_build(ctx->cx, m->m, r->r, e->r, cos_limit, flags, h.r); });
}
uint64_t hry_creases_count(const hry_creases *c) { return c ? c->r.summary[0] : 0; }
// vertex areas and curvatures of a render build (curvature.cpp)
int hry_curvature_build(hry_ctx *ctx, const hry_mesh *m, const hry_render *r, const hry_edges *e, uint32_t flags, hry_curvature **out)
{
	return handle_build(ctx, m && r && e, out, [&](hry_curvature &h) { curvature_build(ctx->cx, m->m, r->r, e->r, flags, h.r); });
}
uint64_t hry_curvature_count(const hry_curvature *c) { return rows_of(result_of(c), "vertex_class"); }
int hry_curvature_totals(const hry_curvature *c, double out[3])
{
	if (!c || !out) return null_argument();
	for (int i = 0; i < 3; ++i) out[i] = c->r.totals[i];
	return HRY_OK;
}
// the hierarchy over the triangles of a render build, the cast and the closest-point query over it (bvh.cpp)
int hry_bvh_build(hry_ctx *ctx, const hry_mesh *m, const hry_render *r, uint32_t flags, hry_bvh **out)
{
	return handle_build(ctx, m && r, out, [&](hry_bvh &h) { bvh_build(ctx->cx, m->m, r->r, flags, h.r); });
}
uint64_t hry_bvh_count(const hry_bvh *b) { return rows_of(result_of(b), "leaf_tri"); }
int hry_bvh_cast(hry_ctx *ctx, const hry_bvh *b, uint64_t n_rays, const float *origins, uint64_t origin_stride, const float *dirs, uint64_t dir_stride, double tmin,
                 double tmax, uint32_t flags, uint32_t *hit_tri, float *hit_t, float *hit_uv, uint64_t stat[2], double *device_ms)
{
	if (!ctx || !b || (n_rays && (!origins || !dirs || !hit_tri))) return null_argument();
	return guarded([&] { bvh_cast(ctx->cx, b->r, n_rays, origins, origin_stride, dirs, dir_stride, tmin, tmax, flags, hit_tri, hit_t, hit_uv, stat, device_ms); });
}
int hry_bvh_nearest(hry_ctx *ctx, const hry_bvh *b, uint64_t n_points, const float *points, uint64_t point_stride, double max_dist, uint32_t flags, uint32_t *near_tri,
                    double *near_d2, float *near_uv, float *near_point, uint64_t stat[3], double *device_ms)
{
	if (!ctx || !b || (n_points && (!points || !near_tri))) return null_argument();
	return guarded([&] { bvh_nearest(ctx->cx, b->r, n_points, points, point_stride, max_dist, flags, near_tri, near_d2, near_uv, near_point, stat, device_ms); });
}
// ... and the pairs of its triangles that pass through each other: a build that reads the hierarchy alone
int hry_intersections_build(hry_ctx *ctx, const hry_bvh *b, uint32_t flags, hry_intersections **out)
{
	return handle_build(ctx, b != nullptr, out, [&](hry_intersections &h) { intersections_build(ctx->cx, b->r, flags, h.r); });
}
uint64_t hry_intersections_count(const hry_intersections *i) { return i ? i->r.summary[3] : 0; }
int hry_mesh_flip_faces(const hry_mesh *m, const uint32_t *face_flip, hry_mesh **out)
{
	if (out) *out = nullptr;
	if (!m || !face_flip || !out) { g_last_error = "null argument"; return HRY_E_ARG; }
	return guarded([&] {
		std::unique_ptr<Mesh> c(mesh_flip_faces(m->m, face_flip));
		*out = new hry_mesh{ std::move(*c) };
	});
}

// ---- numbering maps of an encode (order.cpp)
int hry_order_take(hry_ctx *ctx, const hry_mesh *m, hry_order **out)
{
	if (out) *out = nullptr;
	if (!ctx || !m || !out) { g_last_error = "null argument"; return HRY_E_ARG; }
	if (!ctx->cx.order || ctx->cx.order_token == 0 || ctx->cx.order_token != m->m.order_token) {
		g_last_error = "hry_order_take: the last call on this context was not a successful hry_encode of this mesh with HRY_FLAG_ORDER (or its maps have been taken)";
		return HRY_E_ARG;
	}
	return guarded([&] {
		std::unique_ptr<hry_order> o(new hry_order());
		o->r = std::move(ctx->cx.order);
		ctx->cx.order_token = 0;
		*out = o.release();
	});
}
int hry_order_get(const hry_order *o, const char *name, const void **dev, uint64_t *rows) { return handle_get(result_of(o), name, dev, rows, nullptr, nullptr, false); }
int hry_order_copy(hry_ctx *ctx, const hry_order *o, const char *name, void *dst, int dst_is_device) { return handle_copy(ctx, result_of(o), name, "numbering map", dst, dst_is_device, true); }
int hry_order_apply(hry_ctx *ctx, const hry_order *o, const char *kind, int direction, const void *d_src, uint64_t src_stride, void *d_dst, uint64_t dst_stride,
                    uint64_t row_bytes, uint64_t dst_rows)
{
	if (!ctx || !o || !o->r || !kind || !d_src || !d_dst) { g_last_error = "null argument"; return HRY_E_ARG; }
	return guarded([&] { order_apply(ctx->cx, *o->r, kind, direction, d_src, src_stride, d_dst, dst_stride, row_bytes, dst_rows); });
}
void hry_order_free(hry_order *o) { delete o; }

// ---- per-component error of one mesh against another (distortion.cpp).  Like hry_render_build it leaves the decode's token
// alone: b stays what the context holds, for this build and for a render build after it
int hry_distortion_build(hry_ctx *ctx, const hry_mesh *a, const hry_mesh *b, const hry_order *o, uint32_t flags, hry_distortion **out)
{
	return handle_build(ctx, a && b && !(o && !o->r), out, [&](hry_distortion &d) { distortion_build(ctx->cx, a->m, b->m, result_of(o), flags, d.r); });
}
int hry_distortion_component(const hry_distortion *d, int l, int c, hry_comp_error *out)
{
	if (!d || !out) { g_last_error = "null argument"; return HRY_E_ARG; }
	if (l < 0 || (size_t)l >= d->r.comp.size() || d->r.comp[l].empty()) { g_last_error = "no such compared list"; return HRY_E_ARG; }
	if (c < 0 || (size_t)c >= d->r.comp[l].size()) { g_last_error = "no such component"; return HRY_E_ARG; }
	*out = d->r.comp[l][c];
	return HRY_OK;
}
int hry_distortion_position(const hry_distortion *d, hry_pos_error *out)
{
	if (!d || !out) { g_last_error = "null argument"; return HRY_E_ARG; }
	*out = d->r.pos;
	return HRY_OK;
}
int hry_distortion_position_component(const hry_distortion *d) { return d ? d->r.pos_comp : -1; }
int hry_distortion_normals(const hry_distortion *d, hry_normal_error *out)
{
	if (!d || !out) { g_last_error = "null argument"; return HRY_E_ARG; }
	*out = d->r.nrm;
	if (out->list < 0) g_last_error = d->r.nrm_why;
	return HRY_OK;
}
int hry_distortion_get(const hry_distortion *d, const char *name, const void **dev, uint64_t *rows) { return handle_get(result_of(d), name, dev, rows, nullptr, nullptr, false); }
int hry_distortion_copy(hry_ctx *ctx, const hry_distortion *d, const char *name, void *dst, int dst_is_device) { return handle_copy(ctx, result_of(d), name, "distortion buffer", dst, dst_is_device, true); }
int hry_distortion_stat(const hry_distortion *d, double *device_ms, uint64_t *uploaded_bytes) { return handle_stat(result_of(d), device_ms, uploaded_bytes); }
void hry_distortion_free(hry_distortion *d) { delete d; }

// ---- the error of every quantisation width, and widths from tolerances (sweep.cpp).  With the bounds known it leaves the
// resident mesh and the decode's buffers alone, like hry_distortion_build; without, it computes them as hry_requant does
int hry_quant_sweep_build(hry_ctx *ctx, hry_mesh *m, hry_sweep **out) { return hry_quant_sweep_build_ex(ctx, m, 0, out); }
int hry_quant_sweep_build_ex(hry_ctx *ctx, hry_mesh *m, uint32_t flags, hry_sweep **out)
{
	if (out) *out = nullptr;
	if (!ctx || !m || !out) { g_last_error = "null argument"; return HRY_E_ARG; }
	order_lost(ctx);
	for (const AttrList &L : m->m.lists) if (!L.have_bounds && L.ncomp() && !m->m.partial) { touched(ctx); touched(m); break; }
	return guarded([&] {
		std::unique_ptr<hry_sweep> s(new hry_sweep());
		quant_sweep_build(ctx->cx, m->m, flags, s->s);
		*out = s.release();
	});
}
static const SweepResult::Comp *sweep_comp(const hry_sweep *s, int l, int c)
{
	if (!s) { g_last_error = "null argument"; return nullptr; }
	if (l < 0 || (size_t)l >= s->s.comp.size()) { g_last_error = "Invalid list index"; return nullptr; }
	if (c < 0 || (size_t)c >= s->s.comp[l].size()) { g_last_error = "Invalid attribute index"; return nullptr; }
	return &s->s.comp[l][c];
}
int hry_quant_sweep_bits(const hry_sweep *s, int l, int c)
{
	const SweepResult::Comp *C = sweep_comp(s, l, c);
	if (!C) return HRY_E_ARG;
	if (!C->qmax) g_last_error = C->why;
	return C->qmax;
}
int hry_quant_sweep_component(const hry_sweep *s, int l, int c, int bits, hry_comp_error *out)
{
	const SweepResult::Comp *C = sweep_comp(s, l, c);
	if (!C) return HRY_E_ARG;
	if (!out) { g_last_error = "null argument"; return HRY_E_ARG; }
	if (!C->qmax) { g_last_error = "list " + std::to_string(l) + " attr " + std::to_string(c) + " was not swept: " + C->why; return HRY_E_UNSUPPORTED; }
	if (bits < 1 || bits > C->qmax) { g_last_error = "Invalid quantization bits"; return HRY_E_ARG; }
	*out = C->by_bits[bits - 1];
	return HRY_OK;
}
int hry_quant_sweep_position(const hry_sweep *s, int bits, hry_pos_error *out)
{
	if (!s || !out) { g_last_error = "null argument"; return HRY_E_ARG; }
	if (s->s.pos.empty()) {   // no positions, or their three components are not all swept
		if (bits < 1 || bits > 30) { g_last_error = "Invalid quantization bits"; return HRY_E_ARG; }
		*out = hry_pos_error{};
		out->list = -1;
		return HRY_OK;
	}
	if (bits < 1 || (size_t)bits > s->s.pos.size()) { g_last_error = "Invalid quantization bits"; return HRY_E_ARG; }
	*out = s->s.pos[bits - 1];
	return HRY_OK;
}
int hry_quant_sweep_normals(const hry_sweep *s, int bits, hry_normal_error *out)
{
	if (!s || !out) { g_last_error = "null argument"; return HRY_E_ARG; }
	if (!s->s.nrm_asked) { g_last_error = "the normals were not swept: the sweep was built without HRY_SWEEP_NORMALS"; return HRY_E_UNSUPPORTED; }
	if (s->s.nrm.empty()) {
		if (bits < 1 || bits > 30) { g_last_error = "Invalid quantization bits"; return HRY_E_ARG; }
		*out = hry_normal_error{ 0, 0, 0, 0, 0, 0, 0, 0, -1 };
		g_last_error = s->s.nrm_why;
		return HRY_OK;
	}
	if (bits < 1 || (size_t)bits > s->s.nrm.size()) { g_last_error = "Invalid quantization bits"; return HRY_E_ARG; }
	*out = s->s.nrm[bits - 1];
	return HRY_OK;
}
int hry_chord_angle(double chord, double *radians)
{
	if (!radians) { g_last_error = "null argument"; return HRY_E_ARG; }
	if (!(chord >= 0.0)) { g_last_error = "a chord is a number that is not negative"; return HRY_E_ARG; }
	*radians = 2.0 * std::asin(std::min(chord / 2.0, 1.0));
	return HRY_OK;
}
int hry_angle_chord(double radians, double *chord)
{
	if (!chord) { g_last_error = "null argument"; return HRY_E_ARG; }
	if (!(radians >= 0.0) || radians > 3.14159265358979323846) { g_last_error = "an angle between normals lies in [0, pi]"; return HRY_E_ARG; }
	*chord = 2.0 * std::sin(radians / 2.0);
	return HRY_OK;
}
int hry_quant_sweep_stat(const hry_sweep *s, double *device_ms, uint64_t *uploaded_bytes)
{
	if (!s) { g_last_error = "null argument"; return HRY_E_ARG; }
	if (device_ms) *device_ms = s->s.device_ms;
	if (uploaded_bytes) *uploaded_bytes = s->s.uploaded_bytes;
	return HRY_OK;
}
void hry_quant_sweep_free(hry_sweep *s) { delete s; }
int hry_quant_choose(const hry_sweep *s, const hry_tolerance *t, size_t nt, hry_quant *out, size_t cap, size_t *n_out)
{
	if (n_out) *n_out = 0;
	if (!s || (nt && !t) || !n_out || (cap && !out)) { g_last_error = "null argument"; return HRY_E_ARG; }
	return guarded([&] {
		const std::vector<hry_quant> q = quant_choose(s->s, t, nt);
		*n_out = q.size();
		if (q.size() > cap) throw Error(HRY_E_ARG, "room for " + std::to_string(cap) + " requests, " + std::to_string(q.size()) + " chosen");
		for (size_t i = 0; i < q.size(); ++i) out[i] = q[i];
	});
}
int hry_quant_pick(const hry_comp_error *by_bits, int n_bits, int metric, double extent, double value)
{
	int bits = 0;
	const int rc = guarded([&] { bits = quant_pick(by_bits, n_bits, metric, extent, value); });
	return rc == HRY_OK ? bits : rc;
}

// ---- the coded size of list 1's components at every quantisation width, and a width from a byte budget (rate.cpp).  The build
// walks the mesh and makes it resident, as hry_encode does
int hry_rate_sweep_build(hry_ctx *ctx, hry_mesh *m, hry_rate_sweep **out)
{
	if (out) *out = nullptr;
	if (!ctx || !m || !out) { g_last_error = "null argument"; return HRY_E_ARG; }
	touched(ctx); touched(m);
	return guarded([&] {
		std::unique_ptr<hry_rate_sweep> s(new hry_rate_sweep());
		rate_sweep_build(ctx->cx, m->m, s->s);
		*out = s.release();
	});
}
uint32_t hry_rate_sweep_coded(const hry_rate_sweep *s) { return s ? s->s.coded : 0; }
int hry_rate_sweep_bits(const hry_rate_sweep *s, int l, int c)
{
	if (!s) { g_last_error = "null argument"; return HRY_E_ARG; }
	if (l < 0 || (size_t)l >= s->s.comp.size()) { g_last_error = "Invalid list index"; return HRY_E_ARG; }
	if (c < 0 || (size_t)c >= s->s.comp[l].size()) { g_last_error = "Invalid attribute index"; return HRY_E_ARG; }
	const RateResult::Comp &C = s->s.comp[l][c];
	if (!C.qmax) g_last_error = C.why;
	return C.qmax;
}
int hry_rate_sweep_planes(const hry_rate_sweep *s, int l, int c, int bits)
{
	if (!s) { g_last_error = "null argument"; return HRY_E_ARG; }
	int np = 0;
	const int rc = guarded([&] { np = rate_planes(s->s, l, c, bits); });
	return rc == HRY_OK ? np : rc;
}
int hry_rate_sweep_hist(const hry_rate_sweep *s, int l, int c, int bits, int plane, uint32_t out[256])
{
	if (!s || !out) { g_last_error = "null argument"; return HRY_E_ARG; }
	return guarded([&] {
		const int np = rate_planes(s->s, l, c, bits);
		if (plane < 0 || plane >= np) throw Error(HRY_E_ARG, "Invalid byte plane");
		memcpy(out, rate_row(s->s.comp[l][c], bits) + (size_t)plane * 256, 256 * sizeof(uint32_t));
	});
}
int hry_rate_sweep_bytes(const hry_rate_sweep *s, int l, int c, int bits, double *out)
{
	if (!s || !out) { g_last_error = "null argument"; return HRY_E_ARG; }
	return guarded([&] { *out = rate_bytes(s->s, l, c, bits); });
}
int hry_rate_sweep_stat(const hry_rate_sweep *s, double *device_ms, double *walk_ms, uint64_t *uploaded_bytes)
{
	if (!s) { g_last_error = "null argument"; return HRY_E_ARG; }
	if (device_ms) *device_ms = s->s.device_ms;
	if (walk_ms) *walk_ms = s->s.walk_ms;
	if (uploaded_bytes) *uploaded_bytes = s->s.uploaded_bytes;
	return HRY_OK;
}
void hry_rate_sweep_free(hry_rate_sweep *s) { delete s; }
int hry_rate_hist_bytes(const uint32_t hist[256], double *out)
{
	if (!hist || !out) { g_last_error = "null argument"; return HRY_E_ARG; }
	*out = rate_hist_bytes(hist);
	return HRY_OK;
}
int hry_rate_pick(const double *bytes_by_bits, int n_bits, double budget)
{
	int bits = 0;
	const int rc = guarded([&] { bits = rate_pick(bytes_by_bits, n_bits, budget); });
	return rc == HRY_OK ? bits : rc;
}
int hry_rate_choose(const hry_rate_sweep *s, int l, int c, double budget, int *bits, double *bytes)
{
	if (bits) *bits = 0;
	if (bytes) *bytes = 0.0;
	if (!s || !bits) { g_last_error = "null argument"; return HRY_E_ARG; }
	return guarded([&] { *bits = rate_choose(s->s, l, c, budget, bytes); });
}

// ---- meshes from device buffers (ingest.cpp)
int hry_mesh_from_device(hry_ctx *ctx, uint32_t nv, const hry_dev_column *vcols, int v_ncomp, uint32_t nf, const uint8_t *d_degrees,
                         const void *d_indices, int index_type, uint64_t n_indices, const hry_dev_column *fcols, int f_ncomp, int flags,
                         uint32_t *d_remap, hry_mesh **out)
{
	if (out) *out = nullptr;
	if (!ctx || !out || (v_ncomp > 0 && !vcols) || (f_ncomp > 0 && !fcols) || (n_indices && !d_indices)) { g_last_error = "null argument"; return HRY_E_ARG; }
	touched(ctx);
	return guarded([&] {
		std::unique_ptr<Mesh> m(mesh_from_device(ctx->cx, nv, vcols, v_ncomp, nf, d_degrees, d_indices, index_type, n_indices, fcols, f_ncomp, flags, d_remap));
		*out = new hry_mesh{ std::move(*m) };
	});
}
int hry_mesh_from_device_corners(hry_ctx *ctx, const hry_dev_rows *pos, const hry_dev_rows *tex, const hry_dev_rows *nrm, uint32_t nf,
                                 const uint8_t *d_degrees, int index_type, uint64_t n_indices, const uint16_t *d_face_material, int flags,
                                 uint32_t *const d_remap[3], hry_mesh **out)
{
	if (out) *out = nullptr;
	if (!ctx || !out || !pos) { g_last_error = "null argument"; return HRY_E_ARG; }
	touched(ctx);
	return guarded([&] {
		std::unique_ptr<Mesh> m(mesh_from_device_corners(ctx->cx, pos, tex, nrm, nf, d_degrees, index_type, n_indices, d_face_material, flags, d_remap));
		*out = new hry_mesh{ std::move(*m) };
	});
}
int hry_mesh_resident(const hry_ctx *ctx, const hry_mesh *m)
{
	return ctx && m && m->m.device_token != 0 && m->m.device_token == ctx->cx.resident_token ? 1 : 0;
}

}   // extern "C"
