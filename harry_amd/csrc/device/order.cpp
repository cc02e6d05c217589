// Numbering maps of an encode (include/harry_amd.h: hry_order_take; kernels: order.hip).  An encode with HRY_FLAG_ORDER calls
// order_build once its container is written: everything the maps need is in HBM by then -- the connectivity (d_foff / d_org / d_eface),
// the walk's orders where the encode's own kernels read them, and, with general bindings, every list's records in creation order
// (d_idx in the events' arena, whether the host's loop or events.hip made it).  What a path did not bring up whole goes up here from
// the walk's host arrays: order_f when no face plane reads it, both orders behind the pipelined chunked encode (which sends them
// run by run inside its batches).  The vertex map is computed from order_v like k_rank's table, not adopted from d_rank: the
// general paths keep the faces' ranks behind it and the pipelined path fills it by runs, and a scatter of 4 bytes a vertex is not
// worth a dependency on either.  The result owns one allocation (DeviceBlock) that no later call on the context touches.
#include <hip/hip_runtime.h>

#include <string>

#include "context.hpp"
#include "kernels.hpp"

namespace hry {

using namespace dev;

void order_build(Context &cx, const Mesh &m, const WalkResult &w, const uint32_t *d_order_v, const uint32_t *d_order_f)
{
	HIP_OK(hipSetDevice(cx.device));
	cx.order.reset();
	const uint32_t nv = m.nv, nf = m.nf, ne = m.ne();
	const uint32_t vc = (uint32_t)w.order_v.size(), fc = (uint32_t)w.order_f.size();
	const ConnView cv = cx.conn_view();
	if (cv.nf != nf || cv.ne != ne) throw Error(HRY_E_INTERNAL, "numbering maps: the context's connectivity is not the encoded mesh's");
	if (vc > nv || fc > nf) throw Error(HRY_E_INTERNAL, "numbering maps: more coded elements than the mesh has");
	if (m.general && cx.order_lists.size() != m.lists.size()) throw Error(HRY_E_INTERNAL, "numbering maps: the encode left no record tables");
	const bool mixed = cv.eface != nullptr;

	// ---- the result: every map and its inverse in one block, filled with HRY_NO_ELEMENT
	std::unique_ptr<OrderResult> R(new OrderResult());
	Carve O;   // piece k is bufs[k]
	auto add = [&](const std::string &name, uint64_t rows) {
		for (int inv = 0; inv < 2; ++inv) {
			R->bufs.push_back(NamedBuf{ inv ? name + "_inv" : name, nullptr, rows, 1, HRY_UINT });
			O.reserve((size_t)rows * 4);
		}
	};
	add("vertex", nv); add("face", nf); add("corner", ne);
	if (m.general) for (size_t l = 0; l < m.lists.size(); ++l) add("list" + std::to_string(l), m.lists[l].count);
	R->block.alloc(cx.device, O.total);
	for (size_t k = 0; k < R->bufs.size(); ++k) R->bufs[k].p = O.ptr<void>(R->block.p, k);
	HIP_OK(hipMemsetAsync(R->block.p, 0xff, O.total, cx.stream));
	auto map = [&](size_t k) { return (uint32_t*)R->bufs[k].p; };
	uint32_t *vertex = map(0), *vertex_inv = map(1), *face = map(2), *face_inv = map(3), *corner = map(4), *corner_inv = map(5);

	// ---- working arrays: the orders the encode did not leave whole in HBM, the coded faces' degrees, their scan
	Carve W;
	uint32_t *up_v, *up_f, *deg, *doff, *sums;
	W.take(up_v, d_order_v ? 0 : (size_t)vc * 4); W.take(up_f, d_order_f ? 0 : (size_t)fc * 4);
	W.take(deg, mixed ? (size_t)fc * 4 : 0); W.take(doff, mixed ? ((size_t)fc + 1) * 4 : 0); W.take(sums, mixed ? scan_sums_words(fc) * 4 : 0);
	cx.d_order_ws.ensure(W.total);
	W.bind(cx.d_order_ws.p);
	if (!d_order_v) {
		if (vc) HIP_OK(hipMemcpyAsync(up_v, w.order_v.data(), (size_t)vc * 4, hipMemcpyHostToDevice, cx.stream));
		d_order_v = up_v;
	}
	if (!d_order_f) {
		if (fc) HIP_OK(hipMemcpyAsync(up_f, w.order_f.data(), (size_t)fc * 4, hipMemcpyHostToDevice, cx.stream));
		d_order_f = up_f;
	}
	if (!mixed) deg = doff = nullptr;   // (one degree: nothing to count or to scan)

	launch_order_vertex(cx.stream, d_order_v, vc, cv.org, nv, vertex, vertex_inv);
	launch_order_face(cx.stream, cv, d_order_f, fc, face, face_inv, deg);
	if (mixed && fc) launch_excl_scan(cx.stream, deg, fc, sums, doff);
	if (fc) launch_order_corner(cx.stream, cv, d_order_f, face, doff, corner, corner_inv);
	if (m.general)
		for (size_t l = 0; l < m.lists.size(); ++l) {
			const OrderListSource &S = cx.order_lists[l];
			if (S.nd > m.lists[l].count) throw Error(HRY_E_INTERNAL, "numbering maps: more records created than the list has");
			launch_order_records(cx.stream, S.d_idx, S.nd, m.lists[l].count, map(6 + 2 * l), map(7 + 2 * l));
		}
	HIP_OK(hipGetLastError());
	HIP_OK(hipStreamSynchronize(cx.stream));   // (the pageable host arrays above are the walk's: they go with the encode)
	cx.order = std::move(R);
}

void order_apply(Context &cx, const OrderResult &o, const char *kind, int direction, const void *d_src, uint64_t src_stride, void *d_dst, uint64_t dst_stride,
                 uint64_t row_bytes, uint64_t dst_rows)
{
	if (direction != HRY_ORDER_TO_DECODED && direction != HRY_ORDER_TO_SOURCE) throw Error(HRY_E_ARG, "unknown direction: HRY_ORDER_TO_DECODED or HRY_ORDER_TO_SOURCE");
	const std::string k(kind);
	if (k.size() >= 4 && k.compare(k.size() - 4, 4, "_inv") == 0) throw Error(HRY_E_ARG, "unknown kind: " + k + " (the direction selects the inverse)");
	// TO_DECODED: dst is indexed by decoded elements, dst row j = src row kind_inv[j]; TO_SOURCE: dst row i = src row kind[i]
	const NamedBuf *map = o.find(direction == HRY_ORDER_TO_DECODED ? k + "_inv" : k);
	if (!map) throw Error(HRY_E_ARG, "unknown kind: " + k);
	if (o.block.device != cx.device) throw Error(HRY_E_ARG, "the numbering maps live on another device than the context's");
	if (row_bytes == 0) throw Error(HRY_E_ARG, "row_bytes is 0");
	if (src_stride < row_bytes || dst_stride < row_bytes) throw Error(HRY_E_ARG, "a stride below row_bytes");
	if (dst_rows != map->rows) throw Error(HRY_E_ARG, "dst_rows is " + std::to_string(dst_rows) + ", the map \"" + map->name + "\" has " + std::to_string(map->rows) + " rows");
	if (!dst_rows) return;
	if (src_stride > (1ull << 31) || dst_stride > (1ull << 31)) throw Error(HRY_E_ARG, "a stride above 2^31 bytes");   // (rows x stride stays below 2^63)
	HIP_OK(hipSetDevice(cx.device));
	const uint64_t src_span = (dst_rows - 1) * src_stride + row_bytes, dst_span = (dst_rows - 1) * dst_stride + row_bytes;
	check_device_memory(cx, d_src, src_span, "src");
	check_device_memory(cx, d_dst, dst_span, "dst");
	const uintptr_t s0 = (uintptr_t)d_src, d0 = (uintptr_t)d_dst;
	if (s0 < d0 + dst_span && d0 < s0 + src_span) throw Error(HRY_E_ARG, "src and dst overlap");
	if (!launch_order_rows(cx.stream, (const uint32_t*)map->p, dst_rows, d_src, src_stride, d_dst, dst_stride, row_bytes)) throw Error(HRY_E_UNSUPPORTED, "more than 2^39 words in one move");
	HIP_OK(hipGetLastError());
	HIP_OK(hipStreamSynchronize(cx.stream));
}

}   // namespace hry
