// What the two writers of the reference stream (.hry v0.1) share -- encode_compat (codec.cpp: the PLY layout's two lists, symbol
// positions as base + stride) and encode_general (general.cpp: the lists behind a mesh's bindings, explicit position tables):
//
//   upload_conn_symbols        the walk's connectivity groups with their positions and its operations -> HBM
//   ModelJobs                  every byte plane with its initial counts (models.h:197-218, model.h:38-55) and its place in the stream
//   launch_conn_models, run    groups -> byte planes, the operation model, the planes' models: (magic(t), x, l) per symbol
//   finish_compat_stream       finish_stream (codec.cpp) -> payload behind the header, the timing record
#include <algorithm>

#include "context.hpp"
#include "kernels.hpp"

namespace hry {

using namespace dev;

ConnSymbols upload_conn_symbols(Context &cx, const WalkResult &w)
{
	ConnSymbols cs{};
	size_t conn_plane_bytes = 0;
	for (int g = 0; g < G_COUNT; ++g) {
		cs.goff[g + 1] = cs.goff[g] + w.grp_val[g].size();
		conn_plane_bytes += w.grp_val[g].size() * kGroupBytes[g];
	}
	const size_t ngrp = cs.goff[G_COUNT], nop = w.op_sc.size();
	cx.d_grp_val.ensure(std::max<size_t>(ngrp * 4, 16));
	cx.d_grp_pos.ensure(std::max<size_t>(ngrp * 4, 16));
	cx.d_connplanes.ensure(std::max<size_t>(conn_plane_bytes, 16));
	// operations as the walk wrote them (symbol | order class << 3) + where the connectivity groups sit between them: the
	// device evaluates the operation model and places the records (k_opmodel_*)
	std::vector<uint32_t> op_thr, op_cum;
	op_position_table(w, op_thr, op_cum);
	const size_t op_bytes = (nop + 15) & ~(size_t)15, ngr = op_thr.size();
	cx.d_op.ensure(std::max<size_t>(op_bytes + ngr * 8 + dev::op_model_scratch_bytes((uint32_t)nop) + 64, 64));
	for (int g = 0; g < G_COUNT; ++g) {
		const size_t n = w.grp_val[g].size();
		if (!n) continue;
		HIP_OK(hipMemcpyAsync(cx.d_grp_val.as<uint32_t>() + cs.goff[g], w.grp_val[g].data(), n * 4, hipMemcpyHostToDevice, cx.stream));
		HIP_OK(hipMemcpyAsync(cx.d_grp_pos.as<uint32_t>() + cs.goff[g], w.grp_pos[g].data(), n * 4, hipMemcpyHostToDevice, cx.stream));
	}
	cs.nop = (uint32_t)nop; cs.ngr = (uint32_t)ngr;
	cs.d_opsc = cx.d_op.as<uint8_t>();
	cs.d_opthr = (uint32_t*)(cs.d_opsc + op_bytes); cs.d_opcum = cs.d_opthr + ngr;
	cs.d_opscratch = cs.d_opcum + ngr;
	if (nop) HIP_OK(hipMemcpyAsync(cs.d_opsc, w.op_sc.data(), nop, hipMemcpyHostToDevice, cx.stream));
	if (ngr) {
		HIP_OK(hipMemcpyAsync(cs.d_opthr, op_thr.data(), ngr * 4, hipMemcpyHostToDevice, cx.stream));
		HIP_OK(hipMemcpyAsync(cs.d_opcum, op_cum.data(), ngr * 4, hipMemcpyHostToDevice, cx.stream));
	}
	return cs;
}

void split_conn_groups(Context &cx, const WalkResult &w, bool numtri)
{
	size_t goff = 0, poff = 0;
	for (int g = 0; g < G_COUNT; ++g) {
		const uint32_t n = (uint32_t)w.grp_val[g].size();
		if (numtri || g != G_NUMTRI) launch_split_bytes(cx.stream, cx.d_grp_val.as<uint32_t>() + goff, n, kGroupBytes[g], cx.d_connplanes.as<uint8_t>() + poff);
		goff += n;
		poff += (size_t)n * kGroupBytes[g];
	}
}

void launch_conn_models(Context &cx, const WalkResult &w, const ConnSymbols &cs)
{
	split_conn_groups(cx, w);
	launch_op_model(cx.stream, cs.d_opsc, cs.nop, cs.d_opthr, cs.d_opcum, cs.ngr, cs.d_opscratch, cx.d_magic.as<MagicEnt>(), cx.d_rec_sym.as<SymRec>(), cx.d_sym_l.as<uint32_t>());
}

// (d_init is sized here: the jobs point into it)
ModelJobs::ModelJobs(Context &cx, const Mesh &m) : cx(cx)
{
	build_init_tables(m, inits);
	for (int k = 0; k < INIT_KINDS; ++k) for (int i = 0; i < 256; ++i) total[k] += inits[(size_t)k * 256 + i];
	cx.d_init.ensure(inits.size() * 4);
}
void ModelJobs::add(const uint8_t *sym, uint32_t n, int init, const uint32_t *pos_tab, uint32_t pos_add, uint32_t pos_base, uint32_t pos_stride)
{
	if (!n) return;
	PlaneJob j{};
	j.sym = sym; j.n = n; j.init = cx.d_init.as<uint32_t>() + (size_t)init * 256; j.t0 = total[init];
	j.pos_tab = pos_tab; j.pos_add = pos_add; j.pos_base = pos_base; j.pos_stride = pos_stride;
	j.chunk0 = (uint32_t)chunks.size();
	for (uint32_t f = 0; f < n; f += kChunk) chunks.push_back(ChunkRef{ (uint32_t)jobs.size(), f });
	jobs.push_back(j);
	max_total = std::max(max_total, j.t0 + n);
}
void ModelJobs::add_conn(const WalkResult &w, const ConnSymbols &cs)
{
	size_t poff = 0;
	for (int g = 0; g < G_COUNT; ++g) {
		const uint32_t n = (uint32_t)w.grp_val[g].size();
		for (int b = 0; b < kGroupBytes[g]; ++b)
			add(cx.d_connplanes.as<uint8_t>() + poff + (size_t)b * n, n, conn_plane_init(group_first_plane(g) + b), cx.d_grp_pos.as<uint32_t>() + cs.goff[g], (uint32_t)b);
		poff += (size_t)n * kGroupBytes[g];
	}
}
void ModelJobs::send(const ConnSymbols &cs, uint32_t ns)
{
	max_total = std::max(max_total, cs.nop + 8);   // the operation model's total: 7 + the operations so far
	HIP_OK(hipMemcpyAsync(cx.d_init.p, inits.data(), inits.size() * 4, hipMemcpyHostToDevice, cx.stream));
	cx.d_jobs.ensure(std::max<size_t>(jobs.size() * sizeof(PlaneJob), 16));
	cx.d_chunks.ensure(std::max<size_t>(chunks.size() * sizeof(ChunkRef), 16));
	cx.d_hist.ensure(std::max<size_t>(chunks.size() * 256 * 4, 16));
	if (!jobs.empty()) HIP_OK(hipMemcpyAsync(cx.d_jobs.p, jobs.data(), jobs.size() * sizeof(PlaneJob), hipMemcpyHostToDevice, cx.stream));
	if (!chunks.empty()) HIP_OK(hipMemcpyAsync(cx.d_chunks.p, chunks.data(), chunks.size() * sizeof(ChunkRef), hipMemcpyHostToDevice, cx.stream));
	cx.ensure_magic(max_total + 1);
	cx.d_rec_sym.ensure(std::max<size_t>((size_t)ns * sizeof(SymRec), 16));
	cx.d_sym_l.ensure(std::max<size_t>((size_t)ns * 4, 16));
}
void ModelJobs::run()
{
	launch_model(cx.stream, cx.d_jobs.as<PlaneJob>(), (uint32_t)jobs.size(), cx.d_chunks.as<ChunkRef>(), (uint32_t)chunks.size(), cx.d_hist.as<uint32_t>(),
	             cx.d_magic.as<MagicEnt>(), cx.d_rec_sym.as<SymRec>(), cx.d_sym_l.as<uint32_t>());
}

// ---- device: serial recurrence, big-number low register, carries; D2H
void finish_compat_stream(Context &cx, uint32_t ns, Clock::time_point t_all, std::vector<uint8_t> &out)
{
	std::vector<uint8_t> payload;
	finish_stream(cx, ns, payload);
	out.insert(out.end(), payload.begin(), payload.end());
	cx.stage_put_host("payload", payload.data(), payload.size());
	cx.timing.k_predict_ms = cx.elapsed(1, 2);
	cx.timing.k_model_ms = cx.elapsed(2, 3);
	cx.timing.k_rchain_ms = cx.elapsed(3, 4);
	cx.timing.device_ms = cx.elapsed(1, 5);
	cx.timing.n_symbols = ns;
	cx.timing.payload_bytes = payload.size();
	cx.timing.total_ms = ms_since(t_all);
}

}   // namespace hry
