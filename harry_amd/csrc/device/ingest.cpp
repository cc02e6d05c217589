// A mesh from device buffers (include/harry_amd.h: hry_mesh_from_device; kernels: ingest.hip; DESIGN.md "7b. Meshes from device
// buffers").  The result is what hry_mesh_from_arrays builds from the same values, and it is resident on the context exactly as after
// hry_mesh_upload: the kernels write the records, org and face offsets straight into d_rec / d_org / d_foff, the twins are matched
// there (Context::match_twins, the code an upload runs), and the host copies come down once.
#include <hip/hip_runtime.h>

#include <cstring>

#include "context.hpp"
#include "kernels.hpp"

namespace hry {

using namespace dev;

// the caller's buffer: device memory of the context's device, and (where the runtime can say) [p, p + bytes) inside one allocation
void check_device_memory(const Context &cx, const void *p, uint64_t bytes, const std::string &what)
{
	hipPointerAttribute_t a{};
	const hipError_t e = hipPointerGetAttributes(&a, p);
	if (e != hipSuccess) (void)hipGetLastError();
	if (e != hipSuccess || a.type != hipMemoryTypeDevice || a.device != cx.device)
		throw Error(HRY_E_ARG, what + ": not device memory of the context's device");
	hipDeviceptr_t base = nullptr;
	size_t size = 0;
	if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return; }
	if ((const uint8_t*)p + bytes > (const uint8_t*)base + size) throw Error(HRY_E_ARG, what + ": extends past the end of its allocation");
}

namespace {

// the layout of one list (layout_attr_list, as hry_mesh_from_arrays) and where each byte of its records comes from
PackCols list_from_columns(const Context &cx, AttrList &L, int target, const hry_dev_column *cols, int ncomp, uint32_t rows, const char *what)
{
	std::vector<std::string> nm;
	std::vector<CompType> ty;
	std::vector<bool> isl;
	for (int i = 0; i < ncomp; ++i) {
		const hry_dev_column &c = cols[i];
		if (c.type < 0 || c.type >= C_NONE) throw Error(HRY_E_ARG, "bad component type");
		if (!c.name) throw Error(HRY_E_ARG, "null component name");
		const std::string where = std::string(what) + " column " + c.name;
		const uint64_t sz = (uint64_t)kTypeSize[c.type];
		if (c.stride == 0 || c.stride % sz) throw Error(HRY_E_ARG, where + ": the stride is not a non-zero multiple of the type's size");
		if ((uintptr_t)c.data % sz) throw Error(HRY_E_ARG, where + ": misaligned");
		if (rows) check_device_memory(cx, c.data, (uint64_t)(rows - 1) * c.stride + sz, where);
		nm.push_back(c.name); ty.push_back((CompType)c.type); isl.push_back(false);
	}
	std::vector<int> slot;
	L.target = target;
	layout_attr_list(nm, ty, isl, L, slot);
	L.count = rows;
	PackCols p{};
	p.rec_stride = (uint32_t)L.stride();
	for (int i = 0; i < ncomp; ++i) {
		const int c = slot[i];
		p.src[c] = (const uint8_t*)cols[i].data;
		p.stride[c] = cols[i].stride;
		for (int b = 0; b < kTypeSize[ty[i]]; ++b) { p.comp_of[L.offset[c] + b] = (uint8_t)c; p.byte_of[L.offset[c] + b] = (uint8_t)b; }
	}
	return p;
}

}   // namespace

Mesh *mesh_from_device(Context &cx, uint32_t nv, const hry_dev_column *vcols, int v_ncomp, uint32_t nf, const uint8_t *d_degrees,
                       const void *d_indices, int index_type, uint64_t n_indices, const hry_dev_column *fcols, int f_ncomp, int flags,
                       uint32_t *d_remap)
{
	HIP_OK(hipSetDevice(cx.device));
	const bool weld = (flags & HRY_INGEST_WELD) != 0;
	if (flags & ~HRY_INGEST_WELD) throw Error(HRY_E_ARG, "unknown flags");
	if (index_type != HRY_UINT && index_type != HRY_LONG) throw Error(HRY_E_ARG, "index type must be HRY_UINT or HRY_LONG");
	if (v_ncomp < 0 || f_ncomp < 0) throw Error(HRY_E_ARG, "negative component count");
	if (weld && v_ncomp == 0) throw Error(HRY_E_ARG, "weld: vertices without components have no key");
	if (n_indices > 0xffffffffull) throw Error(HRY_E_UNSUPPORTED, "more than 2^32-1 half-edges");
	if (!d_degrees && n_indices != 3ull * nf) throw Error(HRY_E_ARG, "sum of degrees differs from the number of indices");
	const uint32_t ne = (uint32_t)n_indices;
	const bool idx64 = index_type == HRY_LONG;
	if (nf && d_degrees) check_device_memory(cx, d_degrees, nf, "degrees");
	if (ne) check_device_memory(cx, d_indices, (uint64_t)ne * (idx64 ? 8 : 4), "indices");
	if (d_remap && nv) check_device_memory(cx, d_remap, (uint64_t)nv * 4, "remap");

	std::unique_ptr<Mesh> m(new Mesh());
	const PackCols pf = list_from_columns(cx, m->lists[0], 0, fcols, f_ncomp, nf, "face");
	const PackCols pv = list_from_columns(cx, m->lists[1], 1, vcols, v_ncomp, nv, "vertex");
	const size_t sv = pv.rec_stride, sfc = pf.rec_stride;

	// ---- the context's resident buffers are rewritten from here on: whatever mesh they held is no longer resident
	cx.resident_token = 0;
	hipStream_t st = cx.stream;
	cx.d_foff.ensure(((size_t)nf + 1) * 4);
	cx.d_org.ensure(std::max<size_t>((size_t)ne * 4, 16));
	cx.d_twin.ensure(std::max<size_t>((size_t)ne * 4, 16));
	cx.d_rec[0].ensure(std::max<size_t>((size_t)nf * sfc, 16));
	cx.d_rec[1].ensure(std::max<size_t>((size_t)nv * sv, 16));

	Carve W;   // the working arrays, pieces of d_ingest
	const uint32_t nwf = (uint32_t)(((uint64_t)nf + 63) / 64);
	const size_t status_bytes = sizeof(IngestStatus) + 8;   // (+ the number of welded vertices)
	IngestStatus *status;
	uint32_t *fsum, *fstart, *frow;
	uint8_t *keys;
	W.take(status, status_bytes);
	W.take(fsum, d_degrees ? (size_t)nwf * 4 : 0); W.take(fstart, d_degrees ? ((size_t)nwf + 1) * 4 : 0);
	W.take(keys, weld ? (size_t)nv * sv : 0);
	DedupPlan D;   // the weld's numbering of the rows (dedup.hip); D.ids: row -> output vertex
	if (weld) D.reserve(W, nv);
	W.take(frow, weld ? (size_t)nv * 4 : 0);
	cx.d_ingest.ensure(W.total);
	W.bind(cx.d_ingest.p);
	if (weld) D.bind(W, cx.d_ingest.p);
	uint32_t *d_nout = (uint32_t*)((uint8_t*)status + sizeof(IngestStatus));
	HIP_OK(hipMemsetAsync(status, 0, status_bytes, st));

	// ---- every kernel up to the checks, then ONE read-back of the status word (and the welded count)
	launch_ingest_offsets(st, d_degrees, nf, fsum, fstart, cx.d_foff.as<uint32_t>(), status);
	const uint32_t *remap = nullptr;
	if (weld) {
		launch_ingest_pack(st, pv, nv, nullptr, nv, keys);
		HIP_OK(hipMemsetAsync(D.table, 0xff, D.table_bytes(), st));
		launch_dedup_count(st, WeldView{ keys, (uint32_t)sv }, D);
		launch_dedup_assign(st, D, nv, frow);
		if (nv) HIP_OK(hipMemcpyAsync(d_nout, D.total(), 4, hipMemcpyDeviceToDevice, st));
		remap = D.ids;
	} else launch_ingest_pack(st, pv, nv, nullptr, nv, cx.d_rec[1].as<uint8_t>());
	launch_ingest_org(st, d_indices, idx64, ne, nv, remap, cx.d_org.as<uint32_t>(), status);
	launch_ingest_pack(st, pf, nf, nullptr, nf, cx.d_rec[0].as<uint8_t>());
	cx.h_small.ensure(4096);
	HIP_OK(hipMemcpyAsync(cx.h_small.p, status, status_bytes, hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	IngestStatus s;
	uint32_t nout = nv;
	memcpy(&s, cx.h_small.p, sizeof s);
	if (weld) memcpy(&nout, cx.h_small.as<uint8_t>() + sizeof(IngestStatus), 4);
	if (s.err & kIngestBadDegree) throw Error(HRY_E_UNSUPPORTED, "polygon degree outside 3..255");
	if (d_degrees && s.total != n_indices) throw Error(HRY_E_ARG, "sum of degrees differs from the number of indices");
	if (s.err & kIngestBadIndex) throw Error(HRY_E_ARG, "vertex index out of range");
	if (nout > nv) throw Error(HRY_E_INTERNAL, "weld: more vertices than rows");

	// ---- welded: the records of the output vertices, gathered from the columns at each one's first row
	if (weld) {
		launch_ingest_pack(st, pv, nout, frow, nv, cx.d_rec[1].as<uint8_t>());
		if (d_remap && nv) HIP_OK(hipMemcpyAsync(d_remap, remap, (size_t)nv * 4, hipMemcpyDeviceToDevice, st));
	}
	m->nv = nout; m->nf = nf;
	m->lists[1].count = nout;
	if (d_degrees) {
		for (int d = 0; d < 256; ++d)
			if ((s.degmask[d >> 5] >> (d & 31)) & 1) { if (d >= (int)m->have_degree.size()) m->have_degree.resize(d + 1, 0); m->have_degree[d] = 1; }
	} else if (nf) {
		m->have_degree.assign(4, 0);
		m->have_degree[3] = 1;
	}

	// ---- the host copies, then the twins (hubs are matched on the host, from its connectivity)
	m->face_off.resize((size_t)nf + 1);
	m->org.resize(ne);
	for (int k = 0; k < 2; ++k) m->lists[k].data.resize((size_t)m->lists[k].count * m->lists[k].stride());
	fetch_to_host(cx, m->face_off.data(), cx.d_foff.p, ((size_t)nf + 1) * 4);
	fetch_to_host(cx, m->org.data(), cx.d_org.p, (size_t)ne * 4);
	for (int k = 0; k < 2; ++k) fetch_to_host(cx, m->lists[k].data.data(), cx.d_rec[k].p, m->lists[k].data.size());
	cx.conn_state(*m);
	m->twins_pending = true;
	cx.match_twins(*m);
	cx.make_resident(*m);
	return m.release();
}

// ---------------------------------------------------------------------------------------------------------
// hry_mesh_from_device_corners: the mesh hry_mesh_from_obj builds from the text of the same arrays (obj_io.cpp Loader), its tables
// written where upload_general puts them: d_rec[l], d_org, d_twin, d_foff, d_vreg, d_freg, d_vattr, d_cattr (d_fattr stays empty).
// ---------------------------------------------------------------------------------------------------------
namespace {

struct RowsIn {
	const hry_dev_rows *in = nullptr;
	const char *bad_index = "";   // the refusal's text for an index outside the rows
	int k = 0;                    // 0 pos, 1 tex, 2 nrm: d_remap's entry
	uint32_t bad_bit = 0;
	PackCols pack{};
	uint8_t *keys = nullptr;     // pieces of d_ingest (weld), with the numbering's
	uint32_t *frow = nullptr;
	DedupPlan dedup;
};

PackCols float_rows(const Context &cx, const hry_dev_rows &r, const char *what)
{
	if (r.ncomp > 0 && !r.cols) throw Error(HRY_E_ARG, std::string(what) + " rows: null columns");
	PackCols p{};
	p.rec_stride = 4u * (uint32_t)r.ncomp;
	for (int i = 0; i < r.ncomp; ++i) {
		const hry_dev_column &c = r.cols[i];
		const std::string where = std::string(what) + " column " + std::to_string(i);
		if (c.type != HRY_FLOAT) throw Error(HRY_E_ARG, where + ": the type must be HRY_FLOAT");
		if (c.stride == 0 || c.stride % 4) throw Error(HRY_E_ARG, where + ": the stride is not a non-zero multiple of the type's size");
		if ((uintptr_t)c.data % 4) throw Error(HRY_E_ARG, where + ": misaligned");
		if (r.rows) check_device_memory(cx, c.data, (uint64_t)(r.rows - 1) * c.stride + 4, where);
		p.src[i] = (const uint8_t*)c.data;
		p.stride[i] = c.stride;
		for (int b = 0; b < 4; ++b) { p.comp_of[4 * i + b] = (uint8_t)i; p.byte_of[4 * i + b] = (uint8_t)b; }
	}
	return p;
}

}   // namespace

Mesh *mesh_from_device_corners(Context &cx, const hry_dev_rows *pos, const hry_dev_rows *tex, const hry_dev_rows *nrm, uint32_t nf,
                               const uint8_t *d_degrees, int index_type, uint64_t n_indices, const uint16_t *d_face_material, int flags,
                               uint32_t *const d_remap[3])
{
	HIP_OK(hipSetDevice(cx.device));
	const bool weld = (flags & HRY_INGEST_WELD) != 0;
	if (flags & ~HRY_INGEST_WELD) throw Error(HRY_E_ARG, "unknown flags");
	if (!pos) throw Error(HRY_E_ARG, "null position rows");
	if (index_type != HRY_UINT && index_type != HRY_LONG) throw Error(HRY_E_ARG, "index type must be HRY_UINT or HRY_LONG");
	if (n_indices > 0xffffffffull) throw Error(HRY_E_UNSUPPORTED, "more than 2^32-1 half-edges");
	if (!d_degrees && n_indices != 3ull * nf) throw Error(HRY_E_ARG, "sum of degrees differs from the number of indices");
	const uint32_t ne = (uint32_t)n_indices;
	const bool idx64 = index_type == HRY_LONG;
	const int pn = pos->ncomp;
	if (!(pn == 3 || pn == 4 || (pn >= 6 && pn <= 8))) throw Error(HRY_E_ARG, "position rows: 3, 4, 6, 7 or 8 components");
	if (tex && tex->ncomp != 2 && tex->ncomp != 3) throw Error(HRY_E_ARG, "texture rows: 2 or 3 components");
	if (nrm && nrm->ncomp != 3) throw Error(HRY_E_ARG, "normal rows: 3 components");

	std::unique_ptr<Mesh> m(new Mesh());
	m->lists.clear();
	m->general = true;
	m->bind.nb_face = 0; m->bind.nb_vtx = 1; m->bind.nb_corner = 2;   // as the reader sets them
	RowsIn in[3];
	int nl = 0;
	auto add = [&](const hry_dev_rows *r, int kind, int k, const char *what, const char *bad_index, uint32_t bit) {
		if (!r) return;
		RowsIn &R = in[nl];
		R.in = r; R.k = k; R.bad_index = bad_index; R.bad_bit = bit;
		R.pack = float_rows(cx, *r, what);
		if (ne) {
			if (!r->indices) throw Error(HRY_E_ARG, std::string(what) + " indices: null");
			if ((uintptr_t)r->indices % (idx64 ? 8 : 4)) throw Error(HRY_E_ARG, std::string(what) + " indices: misaligned");
			check_device_memory(cx, r->indices, (uint64_t)ne * (idx64 ? 8 : 4), std::string(what) + " indices");
		}
		if (d_remap && d_remap[k] && r->rows) check_device_memory(cx, d_remap[k], (uint64_t)r->rows * 4, std::string(what) + " remap");
		m->lists.push_back(obj_list_layout(kind, r->ncomp));
		m->lists.back().count = r->rows;
		++nl;
	};
	add(pos, OBJ_VERTEX, 0, "position", "vertex index out of range", kIngestBadIndex);
	add(tex, OBJ_TEX, 1, "texture", "texture index out of range", kIngestBadTexIndex);
	add(nrm, OBJ_NORMAL, 2, "normal", "normal index out of range", kIngestBadNormalIndex);
	if (nf && d_degrees) check_device_memory(cx, d_degrees, nf, "degrees");
	if (nf && d_face_material) {
		if ((uintptr_t)d_face_material % 2) throw Error(HRY_E_ARG, "face materials: misaligned");
		check_device_memory(cx, d_face_material, (uint64_t)nf * 2, "face materials");
	}
	const uint32_t rows0 = pos->rows;

	// ---- the context's resident buffers are rewritten from here on: whatever mesh they held is no longer resident
	cx.resident_token = 0;
	cx.gen_token = 0;
	hipStream_t st = cx.stream;
	cx.d_foff.ensure(((size_t)nf + 1) * 4);
	cx.d_org.ensure(std::max<size_t>((size_t)ne * 4, 16));
	cx.d_twin.ensure(std::max<size_t>((size_t)ne * 4, 16));
	for (int l = 0; l < nl; ++l) cx.d_rec[l].ensure(std::max<size_t>((size_t)in[l].in->rows * in[l].pack.rec_stride, 16));
	cx.d_vreg.ensure(std::max<size_t>((size_t)rows0 * 2, 16));
	cx.d_vattr.ensure(std::max<size_t>((size_t)rows0 * 4, 16));
	cx.d_freg.ensure(std::max<size_t>((size_t)nf * 2, 16));
	cx.d_cattr.ensure(std::max<size_t>((size_t)ne * 8, 16));
	cx.d_fattr.ensure(16);

	Carve W;   // the working arrays, pieces of d_ingest
	const uint32_t nwf = (uint32_t)(((uint64_t)nf + 63) / 64);
	const size_t status_bytes = sizeof(IngestStatus) + 16;   // (+ the records of the three lists after the weld, the face regions)
	IngestStatus *status;
	uint32_t *fsum, *fstart, *mfirst, *mrank;
	W.take(status, status_bytes);
	W.take(fsum, d_degrees ? (size_t)nwf * 4 : 0); W.take(fstart, d_degrees ? ((size_t)nwf + 1) * 4 : 0);
	W.take(mfirst, d_face_material ? (size_t)kIngestMaterials * 4 : 0); W.take(mrank, d_face_material ? (size_t)kIngestMaterials * 4 : 0);
	for (int l = 0; l < nl && weld; ++l) {   // every welded list has its own keys and table
		RowsIn &R = in[l];
		const uint32_t n = R.in->rows;
		W.take(R.keys, (size_t)n * R.pack.rec_stride);
		R.dedup.reserve(W, n);
		W.take(R.frow, (size_t)n * 4);
	}
	cx.d_ingest.ensure(W.total);
	W.bind(cx.d_ingest.p);
	for (int l = 0; l < nl && weld; ++l) in[l].dedup.bind(W, cx.d_ingest.p);
	uint32_t *d_counts = (uint32_t*)((uint8_t*)status + sizeof(IngestStatus));   // [k]: records of list k after the weld; [3]: face regions
	HIP_OK(hipMemsetAsync(status, 0, status_bytes, st));

	// ---- every kernel up to the checks, then ONE read-back: the status word, the welded counts, the number of regions
	launch_ingest_offsets(st, d_degrees, nf, fsum, fstart, cx.d_foff.as<uint32_t>(), status);
	for (int l = 0; l < nl; ++l) {
		RowsIn &R = in[l];
		const uint32_t n = R.in->rows;
		if (!weld) { launch_ingest_pack(st, R.pack, n, nullptr, n, cx.d_rec[l].as<uint8_t>()); continue; }
		launch_ingest_pack(st, R.pack, n, nullptr, n, R.keys);
		HIP_OK(hipMemsetAsync(R.dedup.table, 0xff, R.dedup.table_bytes(), st));
		launch_dedup_count(st, WeldView{ R.keys, R.pack.rec_stride }, R.dedup);
		launch_dedup_assign(st, R.dedup, n, R.frow);
		if (n) HIP_OK(hipMemcpyAsync(d_counts + R.k, R.dedup.total(), 4, hipMemcpyDeviceToDevice, st));
	}
	auto remap_of = [&](const RowsIn &R) { return weld ? (const uint32_t*)R.dedup.ids : nullptr; };
	launch_ingest_org(st, pos->indices, idx64, ne, rows0, remap_of(in[0]), cx.d_org.as<uint32_t>(), status);
	CornerSlots cs{};
	for (int l = 1; l < nl; ++l) {   // slots are compacted: tex, then nrm, whichever are given
		cs.idx[l - 1] = in[l].in->indices; cs.remap[l - 1] = remap_of(in[l]); cs.rows[l - 1] = in[l].in->rows; cs.bad[l - 1] = in[l].bad_bit;
	}
	launch_ingest_corner_attr(st, cs, idx64, ne, cx.d_cattr.as<uint32_t>(), status);
	HIP_OK(hipMemsetAsync(cx.d_vreg.p, 0, std::max<size_t>((size_t)rows0 * 2, 16), st));   // one vertex region
	launch_iota(st, rows0, cx.d_vattr.as<uint32_t>());                                // vertex v owns record v
	if (d_face_material) {
		HIP_OK(hipMemsetAsync(mfirst, 0xff, (size_t)kIngestMaterials * 4, st));
		HIP_OK(hipMemsetAsync(mrank, 0, (size_t)kIngestMaterials * 4, st));
		launch_ingest_regions(st, d_face_material, nf, mfirst, mrank, d_counts + 3, cx.d_freg.as<uint16_t>(), status);
	} else HIP_OK(hipMemsetAsync(cx.d_freg.p, 0, std::max<size_t>((size_t)nf * 2, 16), st));
	cx.h_small.ensure(4096);
	HIP_OK(hipMemcpyAsync(cx.h_small.p, status, status_bytes, hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	IngestStatus s;
	uint32_t counts[4];
	memcpy(&s, cx.h_small.p, sizeof s);
	memcpy(counts, cx.h_small.as<uint8_t>() + sizeof(IngestStatus), sizeof counts);
	if (s.err & kIngestBadDegree) throw Error(HRY_E_UNSUPPORTED, "polygon degree outside 3..255");
	if (d_degrees && s.total != n_indices) throw Error(HRY_E_ARG, "sum of degrees differs from the number of indices");
	for (int l = 0; l < nl; ++l) if (s.err & in[l].bad_bit) throw Error(HRY_E_ARG, in[l].bad_index);
	if (s.err & kIngestManyRegions) throw Error(HRY_E_UNSUPPORTED, kTooManyRegionsText);
	const uint32_t nreg = d_face_material ? counts[3] : (nf ? 1u : 0u);
	for (int l = 0; l < nl; ++l) {
		RowsIn &R = in[l];
		const uint32_t n = R.in->rows, nout = weld ? counts[R.k] : n;
		if (nout > n) throw Error(HRY_E_INTERNAL, "weld: more records than rows");
		m->lists[l].count = nout;
		// ---- welded: the records of the output, gathered from the columns at each one's first row
		if (weld) launch_ingest_pack(st, R.pack, nout, R.frow, n, cx.d_rec[l].as<uint8_t>());
		if (d_remap && d_remap[R.k] && n) {
			if (weld) HIP_OK(hipMemcpyAsync(d_remap[R.k], R.dedup.ids, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
			else launch_iota(st, n, d_remap[R.k]);
		}
	}
	const uint32_t nv = m->lists[0].count;
	m->nv = nv; m->nf = nf;
	if (d_degrees) {
		for (int d = 0; d < 256; ++d)
			if ((s.degmask[d >> 5] >> (d & 31)) & 1) { if (d >= (int)m->have_degree.size()) m->have_degree.resize(d + 1, 0); m->have_degree[d] = 1; }
	} else if (nf) {
		m->have_degree.assign(4, 0);
		m->have_degree[3] = 1;
	}

	// ---- the regions' tables (the reader's: one vertex region on list 0, every face region on the corner lists given)
	Bindings &b = m->bind;
	if (nv) { const int r = b.add_vtx_region(1); b.reg_vtxlist[b.off_vtxlist[r]] = 0; }
	for (uint32_t r = 0; r < nreg; ++r) {
		const int q = b.add_face_region(0, nl - 1);
		for (int l = 1; l < nl; ++l) b.reg_cornerlist[b.off_cornerlist[q] + l - 1] = (uint16_t)l;
	}

	// ---- the host copies, then the twins (hubs are matched on the host, from its connectivity)
	m->face_off.resize((size_t)nf + 1);
	m->org.resize(ne);
	b.face_reg.resize(nf);
	b.corner_attr.resize((size_t)ne * 2);
	b.vtx_reg.assign(nv, 0);
	b.vtx_attr.resize(nv);
	for (int l = 0; l < nl; ++l) m->lists[l].data.resize((size_t)m->lists[l].count * m->lists[l].stride());
	fetch_to_host(cx, m->face_off.data(), cx.d_foff.p, ((size_t)nf + 1) * 4);
	fetch_to_host(cx, m->org.data(), cx.d_org.p, (size_t)ne * 4);
	fetch_to_host(cx, b.face_reg.data(), cx.d_freg.p, (size_t)nf * 2);
	fetch_to_host(cx, b.corner_attr.data(), cx.d_cattr.p, (size_t)ne * 8);
	fetch_to_host(cx, b.vtx_attr.data(), cx.d_vattr.p, (size_t)nv * 4);
	for (int l = 0; l < nl; ++l) fetch_to_host(cx, m->lists[l].data.data(), cx.d_rec[l].p, m->lists[l].data.size());
	cx.conn_state(*m);
	m->twins_pending = true;
	cx.match_twins(*m);
	cx.make_resident(*m);
	cx.gen_token = m->device_token;   // the binding tables are there too: upload_general finds nothing to do
	return m.release();
}

}   // namespace hry
