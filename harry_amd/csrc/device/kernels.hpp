// Launch wrappers of the HIP kernels (kernels.hip, chunked.hip, ...).  Everything is enqueued on the given stream.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "dev_types.hpp"

namespace hry {
struct Carve;   // hip_handles.hpp
namespace dev {

// grids: blocks of `per` items that cover n; grid_for: at most 2^20 of them, for kernels that stride over the grid
inline unsigned blocks_for(uint64_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }
inline unsigned grid_for(uint64_t n, unsigned per) { return (unsigned)std::min<uint64_t>((n + per - 1) / per, 1u << 20); }

// every component of a list in two launches; out: 24 bytes per component { u64 min, u64 max, u32 min_at, u32 max_at }
void launch_bounds(hipStream_t st, const uint8_t *rec, uint32_t count, const BoundsPlan &plan,
                   uint8_t *part_min, uint8_t *part_max, uint32_t *part_idx, int nparts, uint8_t *out);
void launch_requant(hipStream_t st, uint8_t *rec, uint32_t count, int stride, const RequantPlan &plan);
void launch_rank(hipStream_t st, const uint32_t *order_v, uint32_t n, const uint32_t *org, uint32_t *rank);
void launch_predict_vtx(hipStream_t st, const ConnView &cv, const uint32_t *order_v, uint32_t n, const uint32_t *rank, const uint8_t *rec,
                        const ListDesc &ld, uint8_t *planes);
void launch_face_planes(hipStream_t st, const ConnView &cv, const uint32_t *order_f, uint32_t n, const uint8_t *rec, const ListDesc &ld, uint8_t *planes);
// the same over a batch of runs of the coding order (chunked.cpp: EncodePipeline): start = exclusive scan of the runs' lengths
// (nruns + 1 entries, device), first = where each run begins in the coding order, total = start[nruns]; n = all coded elements;
// packed = the runs' entries of the host array back to back (they take their places in order_v / order_f on the way)
void launch_rank_runs(hipStream_t st, const uint32_t *start, const uint32_t *first, uint32_t nruns, uint32_t total, const uint32_t *packed, uint32_t *order_v, const uint32_t *org, uint32_t *rank);
void launch_predict_vtx_runs(hipStream_t st, const ConnView &cv, const uint32_t *start, const uint32_t *first, uint32_t nruns, uint32_t total, const uint32_t *order_v, uint32_t n,
                             const uint32_t *rank, const uint8_t *rec, const ListDesc &ld, uint8_t *planes);
void launch_face_planes_runs(hipStream_t st, const ConnView &cv, const uint32_t *start, const uint32_t *first, uint32_t nruns, uint32_t total, const uint32_t *packed, uint32_t *order_f, uint32_t n,
                             const uint8_t *rec, const ListDesc &ld, uint8_t *planes);
void launch_split_bytes_runs(hipStream_t st, const uint32_t *start, const uint32_t *first, uint32_t nruns, uint32_t total, const uint32_t *packed, const uint32_t *val, uint32_t n, int nbytes, uint8_t *planes);
// (packed == nullptr in any of them: the runs' entries were copied to their places in order_v / order_f / val run by run)
void launch_edge_faces(hipStream_t st, const uint32_t *foff, uint32_t nf, uint32_t *eface, uint32_t first = 0);   // faces [first, nf)
void launch_magic_table(hipStream_t st, MagicEnt *tab, uint32_t from, uint32_t to);
void launch_split_bytes(hipStream_t st, const uint32_t *val, uint32_t n, int nbytes, uint8_t *planes);
// the order-conditioned operation model of the reference stream, by counting; op: symbol | class << 3 per operation, thr / cum: op_position_table
size_t op_model_scratch_bytes(uint32_t n);
void launch_op_model(hipStream_t st, const uint8_t *op, uint32_t n, const uint32_t *thr, const uint32_t *cum, uint32_t ngroups, void *scratch,
                     const MagicEnt *magic, SymRec *rec, uint32_t *sym_l);
void launch_op_records(hipStream_t st, const uint32_t *l, const uint32_t *h, const uint32_t *t, const uint32_t *pos, uint32_t n,
                       const MagicEnt *magic, SymRec *rec, uint32_t *sym_l);
void launch_type_records(hipStream_t st, uint32_t n, uint32_t pos_base, uint32_t pos_stride, const MagicEnt *magic, SymRec *rec, uint32_t *sym_l);
void launch_model(hipStream_t st, const PlaneJob *jobs, uint32_t njobs, const ChunkRef *chunks, uint32_t nchunks, uint32_t *hist,
                  const MagicEnt *magic, SymRec *rec, uint32_t *sym_l);
void launch_rchain(hipStream_t st, const SymRec *rec, uint32_t n, uint64_t *r_out, uint32_t *s_out, uint64_t *state);
void launch_low_accumulate(hipStream_t st, const uint64_t *r, const uint32_t *s, const uint32_t *sym_l, uint32_t n, uint64_t *acc);
struct PullRanges { uint32_t *dst[4]; const uint32_t *src[4]; uint32_t words[4]; };   // device destinations, pinned host sources (device-visible), 32-bit words each
void launch_pull_ranges(hipStream_t st, const PullRanges &r);
void launch_carry(hipStream_t st, const uint64_t *acc, uint32_t nw, uint64_t *v, uint32_t *summary, uint8_t *bytes, const StreamJob *jobs = nullptr, const uint32_t *stream_bits = nullptr, uint32_t ns = 0);

// attribute records from the decoded residual planes (unpredict.hip; driver: unchunk.cpp)
void launch_residuals_to_rec(hipStream_t st, const uint8_t *planes, uint32_t n, const ListDesc &ld, uint8_t *rec);
void launch_faces_unfold(hipStream_t st, uint32_t n, const ListDesc &ld, uint8_t *rec);
bool unpredict2_applicable(const ListDesc &ld);
// plan (keep_stages: the stage "chain_plan"): a row of six words per chain kernel launched -- kind (2 k_unpredict2, 3 k_unpredict3,
// 4 k_unpredict3_range, 5 k_unpredict2 in its exact form for signed sources), storage type, work lists, components of that type,
// wavefronts per chain, bytes of the LDS ring.  Filled on the host where the launch is decided; the kernels know nothing of it.
constexpr uint32_t kChainPlanWords = 6;
void launch_chain_records(hipStream_t st, const uint32_t *cand, const uint8_t *ncand, uint32_t nvtx, const uint32_t *seg_start, uint32_t nseg, void *crec);
bool unpredict3_wanted(const ListDesc &ld);
void launch_unpredict2(hipStream_t st, const ConnView &cv, const uint32_t *order_v, uint32_t nvtx, uint32_t *cand, uint8_t *ncand, const void *crec,
                       const uint8_t *planes, const ListDesc &ld, uint8_t *rec, const uint32_t *segs, const uint32_t *list_off, uint32_t n_lists,
                       const uint32_t *seg_start, uint32_t nseg, uint32_t *done, std::vector<uint32_t> *plan = nullptr);
void launch_candidates_ids(hipStream_t st, const ConnView &cv, const uint32_t *order_v, uint32_t nvtx, uint32_t *cand, uint8_t *ncand);
bool unpredict3_covers(const ListDesc &ld);
void launch_slice_prepare(hipStream_t st, const ConnView &cv, const uint32_t *order_v, uint32_t nvtx, uint32_t v_begin, uint32_t v_end, uint32_t *cand, uint8_t *ncand, void *crec);
size_t cand_table_words(uint32_t nvtx);
void cand_table_reset(hipStream_t st, uint32_t *cand, uint32_t nvtx);
void launch_slice_chain(hipStream_t st, const ConnView &cv, const uint32_t *order_v, uint32_t nvtx, uint32_t v_begin, uint32_t v_end, const uint32_t *cand, const uint8_t *ncand,
                        const void *crec, const uint8_t *planes, const ListDesc &ld, uint8_t *rec, std::vector<uint32_t> *plan = nullptr);
void launch_scatter_u32(hipStream_t st, const uint32_t *pairs, uint32_t n, uint32_t *dst);
uint32_t chain_timeout_flags(hipStream_t st, const uint32_t *gave_up = nullptr);

// records of a mesh with general bindings (general.hip; driver: general.cpp)
constexpr int kSrcCap = 24;   // most sources a vertex record keeps (general.hip: SrcCap)
struct GenChainJob {
	int32_t kind, comp;        // one job = one component of one list (the components of a record are predicted independently)
	uint32_t n, pad2;
	uint8_t *rec;
	const uint32_t *src, *ev_he;
	const uint8_t *nsrc, *ev_slot;
	ListDesc ld;
};
void launch_face_rank(hipStream_t st, const ConnView &cv, const uint32_t *order_f, uint32_t n, uint32_t *frank);
void launch_gen_vtx_resid(hipStream_t st, const ConnView &cv, const GenView &gv, const uint32_t *rank, const uint32_t *ev_he, const uint8_t *ev_slot,
                          const uint32_t *ev_idx, uint32_t n, const uint8_t *rec, const ListDesc &ld, uint8_t *planes);
void launch_gen_face_resid(hipStream_t st, const uint32_t *ev_idx, uint32_t n, const uint8_t *rec, const ListDesc &ld, uint8_t *planes);
void launch_gen_corner_resid(hipStream_t st, const ConnView &cv, const GenView &gv, const uint32_t *frank, const uint32_t *ev_he, const uint8_t *ev_slot,
                             const uint32_t *ev_idx, uint32_t n, const uint8_t *rec, const ListDesc &ld, uint8_t *planes);
void launch_gen_sources(hipStream_t st, int kind, const ConnView &cv, const GenView &gv, const uint32_t *rank, const uint32_t *ev_he, const uint8_t *ev_slot,
                        uint32_t n, uint32_t *src, uint8_t *nsrc);
void launch_gen_chain(hipStream_t st, int kind, int stype, const ConnView &cv, const GenView &gv, const uint32_t *rank, const GenChainJob *jobs, uint32_t njobs);

// half-edge twin matching (twins.hip): conn.org / foff (/ eface) resident, twin = output; ws: twin_workspace_bytes
size_t twin_workspace_bytes(uint32_t nv, uint32_t ne);
uint32_t twin_overflow_capacity();
// *over: device pointer (inside ws) of the list of vertices with too many half-edges for the kernel: count, then vertex ids
void launch_twins(hipStream_t st, const ConnView &cv, uint32_t nv, uint32_t *twin, void *ws, const uint32_t **over);

// the grid-level exclusive scans (scan.hip; the wavefront and block levels under them: wave.hpp).  launch_excl_scan: n counters in
// three launches, sums: scan_sums_words(n) words of scratch.  total_out == nullptr: out[n + 1], out[n] = total; otherwise out[n]
// and *total_out = total.  No counters: the total alone, 0
size_t scan_sums_words(uint32_t n);
void launch_excl_scan(hipStream_t st, const uint32_t *in, uint32_t n, uint32_t *sums, uint32_t *out, uint32_t *total_out = nullptr);
void launch_scan_counts(hipStream_t st, const uint32_t *counts, uint32_t n, uint32_t *out);   // k_scan_counts (one block): out[n + 1], out[n] = total

// order.hip: the numbering maps of an encode; every table pre-filled with 0xFF (kNoRank) by the caller
void launch_order_vertex(hipStream_t st, const uint32_t *order_v, uint32_t n, const uint32_t *org, uint32_t nv, uint32_t *vertex, uint32_t *vertex_inv);
// deg: the coded faces' degrees in coding order (mixed degrees), or nullptr
void launch_order_face(hipStream_t st, const ConnView &cv, const uint32_t *order_f, uint32_t n, uint32_t *face, uint32_t *face_inv, uint32_t *deg);
// doff: exclusive scan of deg (mixed degrees), or nullptr: decoded face j begins at j * cv.udeg
void launch_order_corner(hipStream_t st, const ConnView &cv, const uint32_t *order_f, const uint32_t *face, const uint32_t *doff, uint32_t *corner, uint32_t *corner_inv);
void launch_order_records(hipStream_t st, const uint32_t *d_idx, uint32_t nd, uint32_t count, uint32_t *list, uint32_t *list_inv);
// dst row i = src row map[i] (zero where map[i] is kNoRank), row_bytes of every row; false: more words than one launch covers
bool launch_order_rows(hipStream_t st, const uint32_t *map, uint64_t rows, const void *src, uint64_t src_stride, void *dst, uint64_t dst_stride, uint64_t row_bytes);
// connected components of the faces and their tables for the walk on several host threads (twins.hip; driver: analysis.cpp)
size_t components_workspace_bytes(uint32_t nv, uint32_t nf);
// where the workspace's parts lie (twins.hip decides; nobody else computes an offset into it): per face the component label (a
// root face after stage 1), the root flags, their exclusive scan (num[nf] = components) and the scan's block sums; per vertex the
// first component in coding order (stage 3); the list of (component, component) ties with its counter
struct ComponentsWorkspace { uint32_t *label, *flag, *num, *sums, *vfirst, *tie_count, *tie_pairs; };
ComponentsWorkspace components_workspace(void *ws, uint32_t nv, uint32_t nf);
void launch_components_label(hipStream_t st, const ConnView &cv, const ComponentsWorkspace &w);
void launch_components_faces(hipStream_t st, const ConnView &cv, uint32_t *label, const uint32_t *num, const uint32_t *spans, uint32_t nspans,
                             uint32_t *nfaces, uint32_t *nhe, uint32_t *flo, uint32_t *fhi, uint64_t *first_key);
void launch_components_vertices(hipStream_t st, const ConnView &cv, uint32_t nv, uint32_t ncomp, const ComponentsWorkspace &w, const uint32_t *rank_of,
                                uint32_t *tie, uint32_t *fresh, uint32_t *vlo, uint32_t *vhi);

// chunked profile (chunked.hip)
void launch_chunk_encode(hipStream_t st, const StreamJob *jobs, uint32_t nstreams, const uint32_t *inits, const MagicEnt *magic, uint64_t *acc, uint32_t *stream_bits);
// the same streams in two kernels (thousands of streams: the model a wavefront per stream, the range registers a lane per stream):
// rec = 8 bytes per symbol of all streams (every stream: t0 + n <= 65535), rec_off[j] = symbols of the streams before j,
// order = stream indices, longest first
void launch_chunk_encode_split(hipStream_t st, const StreamJob *jobs, uint32_t nstreams, const uint32_t *inits, const MagicEnt *magic, uint64_t *acc, uint32_t *stream_bits,
                               const uint64_t *rec_off, void *rec, const uint32_t *order);
void launch_stream_pack(hipStream_t st, const StreamJob *jobs, uint32_t nstreams, const uint32_t *stream_bits, const uint8_t *bytes,
                        uint32_t *nbytes, uint64_t *offsets, uint8_t *out, bool pack);
// stable partition of the operation bytes (symbol | class << 3) into one plane of symbols per class; base[c] = first byte of
// plane c in `planes`, scratch: 8 counters per unit of kSplitUnit operations
constexpr uint32_t kSplitUnit = 1024;
void launch_split_classes(hipStream_t st, const uint8_t *ops, uint32_t n, const uint32_t base[8], uint32_t *scratch, uint8_t *planes);
void launch_plane_hist(hipStream_t st, const HistSlice *slices, uint32_t nslices, uint32_t *hist);
void launch_scatter_u8(hipStream_t st, const uint8_t *src, const uint32_t *dst_index, uint32_t n, uint8_t *dst);
void launch_chunk_decode(hipStream_t st, const StreamJob *jobs, uint32_t nstreams, const uint32_t *inits, const MagicEnt *magic,
                         const uint8_t *payload, const uint64_t *offsets, const uint32_t *nbytes);
void launch_chunk_decode_lanes(hipStream_t st, const StreamJob *jobs, uint32_t nstreams, const uint32_t *inits, const MagicEnt *magic,
                               const uint8_t *payload, const uint64_t *offsets, const uint32_t *nbytes, bool counts16);   // one lane per stream; every job with t0 > 128 (counts16: and t0 + n <= 65535)

// events.hip: which record every element names, per list, on the device (the host's loop: host/general_events.cpp)
size_t events_list_workspace_bytes(uint32_t n_order, uint32_t max_refs, uint32_t list_count);
size_t events_names_workspace_bytes(uint32_t fc, uint32_t corner_refs_max, uint32_t head_words);
void launch_corner_places(hipStream_t st, const ConnView &cv, const GenView &gv, const EvRegions &rg, const uint32_t *order_f, uint32_t fc, uint32_t corner_refs_max,
                          uint32_t head_words, uint32_t nv, void *names_ws);
void launch_list_refs(hipStream_t st, int kind, uint32_t list, uint32_t list_count, const ConnView &cv, const GenView &gv, const EvRegions &rg,
                      const uint32_t *order, uint32_t n_order, uint32_t max_refs, uint32_t nv, uint32_t fc, uint32_t corner_refs_max, uint32_t head_words, void *names_ws, void *list_ws,
                      uint32_t *counts, uint32_t *err);
void launch_list_kinds(hipStream_t st, int kind, uint32_t list_count, const ConnView &cv, uint32_t n_order, uint32_t max_refs, uint32_t nv, uint32_t fc, uint32_t corner_refs_max,
                       uint32_t head_words, void *names_ws, void *list_ws, uint8_t *type_sym, uint32_t *gh_val, uint32_t *lh_val, uint32_t *d_idx, uint32_t *d_he, uint8_t *d_slot,
                       uint32_t *counts, uint32_t *err);
void launch_region_symbols(hipStream_t st, int kind, const ConnView &cv, const GenView &gv, const uint32_t *order, uint32_t n, uint8_t *out);

// first-occurrence numbering (dedup.hip): item i gets the id of its key, ids numbered by the key's first item.  The keys of the
// unweld are an UnweldView's corners (dev_types.hpp), the weld's the packed records of a WeldView
struct WeldView { const uint8_t *rec; uint32_t stride, n, mask; uint32_t *table; };
// the working arrays of one numbering of n items: reserve() its pieces in a Carve while sizing, bind() after the allocation.
// table: mask + 1 slots (a power of two >= 2 n), filled with 0xff by the caller before launch_dedup_count; first_of / ids[n],
// masks / counts[nw], wave_start[nw + 1]; *total(): the number of distinct keys, on the device
struct DedupPlan {
	uint32_t n = 0, nw = 0, mask = 0;
	uint32_t *table = nullptr, *first_of = nullptr, *counts = nullptr, *wave_start = nullptr, *ids = nullptr;
	uint64_t *masks = nullptr;
	size_t at_table = 0, at_first_of = 0, at_masks = 0, at_counts = 0, at_wave_start = 0, at_ids = 0;   // pieces of the Carve
	size_t table_bytes() const { return ((size_t)mask + 1) * 4; }
	const uint32_t *total() const { return wave_start + nw; }
	bool own_ids = true;
	void reserve(Carve &W, uint32_t items, bool with_ids = true);   // with_ids false: the caller points `ids` at n words of its own after bind()
	void bind(const Carve &W, void *base);
};
// insert, find, scan over the keys of u; the launcher takes u's table, mask and item count from the plan.  Fills first_of, masks,
// counts, wave_start
void launch_dedup_count(hipStream_t st, UnweldView u, const DedupPlan &p);
void launch_dedup_count(hipStream_t st, WeldView u, const DedupPlan &p);
void launch_dedup_count(hipStream_t st, EdgeView u, const DedupPlan &p);   // the sides of a render build's triangles (edges.cpp)
void launch_dedup_count(hipStream_t st, ShellVertexView u, const DedupPlan &p);   // the corners of its triangles by (shell, decoded vertex) (shells.cpp)
void launch_dedup_count(hipStream_t st, CreaseSlotView u, const DedupPlan &p);   // their index slots by (output vertex, smooth group) (creases.cpp)
// p.ids[i] = id of item i; per id below nout: first_item[id] = its first item, via_out[id] = via[that item] (via == nullptr: none)
void launch_dedup_assign(hipStream_t st, const DedupPlan &p, uint32_t nout, uint32_t *first_item, const uint32_t *via = nullptr, uint32_t *via_out = nullptr);
void launch_iota(hipStream_t st, uint32_t n, uint32_t *out);   // out[i] = i

// render-ready buffers (render.hip; driver: render.cpp).  launch_fan: tri_face[T] and indices[3T] of the fan triangulation,
// corners mapped through vmap (org, or the unweld's corner -> output vertex map)
void launch_fan(hipStream_t st, const uint32_t *foff, uint32_t nf, uint64_t ntri, const uint32_t *vmap, uint32_t ne, uint32_t *tri_face, uint32_t *indices);
void launch_rows_of(hipStream_t st, const RowsView &v, uint32_t rows, uint32_t *idx);
// plan: every component of the list (dst_bits 0; src_bits = its quantisation), idx == nullptr: row u is record u
// a decoded segment into the whole numbering (render.cpp: place_segment): records (stride bytes each) of nl local vertices / faces,
// origins of ne local half-edges (vertex ids mapped too), face offsets of nf local faces
void launch_place_segment(hipStream_t st, const RunPlace &r, const uint8_t *vrec, uint32_t nlv, uint32_t vstride, uint8_t *whole_vrec,
                          const uint8_t *frec, uint32_t nlf, uint32_t fstride, uint8_t *whole_frec, const uint32_t *org, uint32_t nle, uint32_t *whole_org,
                          const uint32_t *foff, uint32_t *whole_foff);
void launch_render_gather(hipStream_t st, const uint8_t *rec, int stride, uint32_t count, const uint32_t *idx, uint64_t rows, const RequantPlan &plan, float *out);

// normals of a render build (normals.hip; driver: render.cpp).  fn: 3 doubles per face (working buffer); count / fill: nv zeroed
// counters each; start: nv + 1; sums: scan_sums_words(nv); seg: ne; hubs: 1 + normals_hub_capacity(ne) words, the first zeroed;
// out: nv rows of 3 floats, every row written
uint32_t normals_hub_capacity(uint32_t ne);
void launch_face_normals(hipStream_t st, const NrmView &n, double *fn, float *face_normals /* nf x 3, or nullptr */);
void launch_vertex_normals(hipStream_t st, const NrmView &n, const double *fn, uint32_t *count, uint32_t *fill, uint32_t *start, uint32_t *sums, uint32_t *seg,
                           uint32_t *hubs, float *out);
void launch_normals_expand(hipStream_t st, const float *vn, const uint32_t *vsrc, uint32_t nout, uint32_t nv, float *out);   // out[u] = vn[vsrc[u]]

// edges of a render build (edges.hip; driver: edges.cpp), behind the numbering of the sides (v.tri_edges).  count: v.ne zeroed
// counters (the scatter's cursors afterwards); sums: scan_sums_words(v.ne); hubs: 1 + edges_hub_capacity(v.n) words, the first
// zeroed; classes: 3 zeroed counters -- edges with one side, with two, with more.  Every row of every buffer of v is written
uint32_t edges_hub_capacity(uint32_t nsides);
void launch_edges(hipStream_t st, const EdgesView &v, uint32_t *count, uint32_t *sums, uint32_t *hubs, uint32_t *classes);

// tangent frames of a render build (tangents.hip; driver: tangents.cpp).  The working arrays and what is zeroed: TanWork
// (dev_types.hpp).  Every row of v.tangents and, where given, v.bitangents is written
uint32_t tangents_hub_capacity(uint32_t nslots);
void launch_tangents(hipStream_t st, const TanView &v, const TanWork &w);

// hard edges and split normals of a render build (creases.hip; driver: creases.cpp), behind its edges build with geometry.  The
// working arrays and what is zeroed: CreaseWork (dev_types.hpp).  launch_creases_groups: w.eclass, the classes' counters, the
// union-find over the slots, w.root and the scan of the root flags: w.num[n] = the number of groups, on the device.
// launch_creases_normals (v.ng and v.nw known, the outputs allocated, v.ids and v.render_vertex numbered, w.first_slot filled):
// every row of edge_class, slot_group, vertex_source and normals
uint32_t creases_hub_capacity(uint32_t nslots);
void launch_creases_groups(hipStream_t st, const CreaseView &v, const CreaseWork &w);
void launch_creases_normals(hipStream_t st, const CreaseView &v, const CreaseWork &w);

// vertex areas and curvatures of a render build (curvature.hip; driver: curvature.cpp), behind its edges build.  The working arrays
// and what is zeroed: CurvWork (dev_types.hpp).  Every row of the six buffers of v is written; returns where the totals' one row of
// three doubles will lie on the device (nullptr: no decoded vertex).  curvature_fold_rows: the rows one round of the totals'
// reduction leaves of `rows`
uint32_t curvature_hub_capacity(uint32_t nslots);
uint32_t curvature_fold_rows(uint32_t rows);
const double *launch_curvature(hipStream_t st, const CurvView &v, const CurvWork &w);

// the hierarchy of a render build and the cast over it (bvh.hip; driver: bvh.cpp).  launch_bvh_first: live flags, codes, the sort, the
// tree and its depth, everything in BvhWork (dev_types.hpp); w.words[0 .. 2] = L, distinct codes, depth afterwards.
// launch_bvh_second (L and the depth known, the buffers of v allocated): every buffer of v, the node boxes in `depth` launches.
// launch_bvh_cast: c.n rays against v; bvh_cast_block: the rays of one workgroup; bvh_radix_words: the words of w.radix for T triangles
// launch_bvh_nearest: the closest point of v's triangles to each of c.n points, in workgroups of the cast's size
size_t bvh_radix_words(uint32_t T);
void launch_bvh_first(hipStream_t st, const BvhWork &w);
void launch_bvh_second(hipStream_t st, const BvhWork &w, const BvhView &v, uint32_t depth);
void launch_bvh_cast(hipStream_t st, const BvhView &v, const BvhCast &c);
uint32_t bvh_cast_block();
void launch_bvh_nearest(hipStream_t st, const BvhView &v, const BvhNearest &c);
// launch_bvh_pairs_count (c.fill == 0): the walk of every leaf against the hierarchy, counting, and the scan of the counts into
// c.start and c.words[0]; sums: scan_sums_words(v.L).  launch_bvh_pairs_fill (c.fill == 1, c.P known): the walk again, the two sorts
// (key_b / val_b: the other side, P words each; radix: bvh_pairs_radix_words(P)), pairs and pair_shared, and H into c.words[1]
size_t bvh_pairs_radix_words(uint32_t P);
void launch_bvh_pairs_count(hipStream_t st, const BvhView &v, const BvhPairs &c, uint32_t *sums);
void launch_bvh_pairs_fill(hipStream_t st, const BvhView &v, const BvhPairs &c, uint32_t *key_b, uint32_t *val_b, uint32_t *radix, uint32_t *pairs, uint32_t *pair_shared);

// shells of a render build (shells.hip; driver: shells.cpp), behind its edges build.  launch_shells_roots: the union-find over the
// triangles, the root flags and their scan: w.num[T] = the number of shells, on the device.  launch_shells_label (v.ns known, the
// outputs allocated, counts zeroed, face_shell filled with 0xff): tri_shell, face_shell, shell_first, the triangle and face columns.
// launch_shells_counts, behind the numbering of the corners by (shell, decoded vertex) (w.pair_id, w.pair_first_of): edge_shell, the
// other six columns, and the five reductions of the summary behind S (w.summary: closed, nonmanifold, misoriented, loops, largest)
void launch_shells_roots(hipStream_t st, const ShellsView &v, const ShellsWork &w);
void launch_shells_label(hipStream_t st, const ShellsView &v, const ShellsWork &w);
void launch_shells_counts(hipStream_t st, const ShellsView &v, const ShellsWork &w);

// consistent winding per patch of a render build (orient.hip; driver: orient.cpp), behind its edges build.  launch_orient_roots: the
// union-find over the orientation double cover, the root flags and their scan: w.num[T] = the number of patches, on the device.
// launch_orient_flips (v.np known, the outputs allocated, counts / face_flip / w.turn zeroed): every integer buffer, the flips
// relative to each patch's lowest triangle, inverted by majority where asked.  launch_orient_outward, behind launch_measures over
// the patches and oriented_indices (v.measures): closed orientable patches of negative volume turned as a whole.
// launch_orient_summary: the five reductions of the summary behind P (w.summary: orientable, flipped, inverted, against, remaining)
void launch_orient_roots(hipStream_t st, const OrientView &v, const OrientWork &w);
void launch_orient_flips(hipStream_t st, const OrientView &v, const OrientWork &w, bool majority);
void launch_orient_outward(hipStream_t st, const OrientView &v, const OrientWork &w);
void launch_orient_summary(hipStream_t st, const OrientView &v, const OrientWork &w);

// area, signed volume and box per label -- a shell, a patch -- of a render build's triangles (measures.hip; drivers: shells.cpp,
// orient.cpp).  The scratch: measures_reserve its seven arrays in a Carve for T triangles (the first piece comes back),
// measures_bind them behind the allocation, with the caller's flag [T] and sums (free by then), measures_clear them for nl labels
uint32_t shells_hub_capacity(uint32_t ntri);
size_t measures_reserve(Carve &W, uint32_t ntri);
MeasuresWork measures_bind(const Carve &W, void *base, size_t first, uint32_t *flag, uint32_t *sums);
void measures_clear(hipStream_t st, const MeasuresWork &w, uint32_t nl);
void launch_measures(hipStream_t st, const MeasuresView &v, const MeasuresWork &w);

// per-component error of one mesh against another (distortion.hip; driver: distortion.cpp).  launch_distortion_rows: one DistPart
// per block of kDistBlockRows rows and slot (pa.n components, then the positions when L.pos >= 0) into L.part; a map entry at or
// above L.b_rows raises *status (nothing is read there).  launch_distortion_fold: the blocks' records in block order, one block per
// list, into out[f.out_at[l] + slot]
constexpr uint32_t kDistBlockRows = 1024;
inline uint32_t distortion_blocks(uint32_t rows) { return (uint32_t)(((uint64_t)rows + kDistBlockRows - 1) / kDistBlockRows); }
void launch_distortion_rows(hipStream_t st, const DistList &L, const RequantPlan &pa, const RequantPlan &pb, uint32_t *status);
void launch_distortion_fold(hipStream_t st, const DistFold &f, DistFinal *out);
// the error of every quantisation width of a list's unquantised components in one pass (sweep.hip; driver: sweep.cpp): blocks of
// kDistBlockRows rows x jobs x groups of kSweepGroup widths leave one DistPart per block and (component, width) in L.part;
// launch_quant_sweep_fold: one block per record of f's lists (nslots = a list's ns), the blocks' records in block order
constexpr int kSweepGroup = 2, kSweepMaxBits = 30;
void launch_quant_sweep(hipStream_t st, const SweepList &L);
void launch_quant_sweep_fold(hipStream_t st, const DistFold &f, DistFinal *out);

// the faces' normal deviation (normal_sweep.hip; drivers: sweep.cpp, distortion.cpp).  launch_normal_sweep: blocks of
// kDistBlockRows faces x groups of kNormalGroup widths leave one NormPart per block and width in S.part; launch_distortion_normals:
// one NormPart per block in P.part; launch_normal_fold: one block per slot, the blocks' records in block order, into out[slot].
// kNormalGroup is a measured choice
constexpr int kNormalGroup = 2;
void launch_normal_sweep(hipStream_t st, const NormalSweep &S);
void launch_distortion_normals(hipStream_t st, const NormalPair &P);
void launch_normal_fold(hipStream_t st, const NormPart *part, uint32_t nblocks, uint32_t nslots, NormFinal *out);

// the byte-plane histograms of the residual codes of list 1's components at every quantisation width (rate.hip; driver: rate.cpp):
// blocks of kRateBlock coded vertices x groups of table rows (row = width, 0: as it stands); L.table is zeroed before
constexpr int kRateBlock = 256;
void launch_rate_sweep(hipStream_t st, const ConnView &cv, const uint32_t *order_v, uint32_t n, const uint32_t *rank, const RateList &L);

// meshes from device buffers (ingest.hip; driver: ingest.cpp).  The checks raise bits of err; total = sum of the degrees (64-bit),
// degmask = the set of degrees present (bit d)
constexpr uint32_t kIngestBadDegree = 1, kIngestBadIndex = 2;
struct IngestStatus { uint32_t err, pad; unsigned long long total; uint32_t degmask[8]; };
// the columns of one list and where their bytes go in its records: byte k of a record is byte byte_of[k] of column comp_of[k]
struct PackCols {
	const uint8_t *src[kMaxComp];
	uint64_t stride[kMaxComp];
	uint8_t comp_of[8 * kMaxComp], byte_of[8 * kMaxComp];
	uint32_t rec_stride;
};
// face_off[nf + 1] into foff; deg == nullptr: every face a triangle.  wave_sums / wave_start: (nf + 63) / 64 (+ 1) words
void launch_ingest_offsets(hipStream_t st, const uint8_t *deg, uint32_t nf, uint32_t *wave_sums, uint32_t *wave_start, uint32_t *foff, IngestStatus *status);
void launch_ingest_org(hipStream_t st, const void *idx, bool idx64, uint32_t ne, uint32_t nv, const uint32_t *remap, uint32_t *org, IngestStatus *status);
// n records of p.rec_stride bytes into out; record r from row rows[r] (rows == nullptr: row r) of columns with nsrc rows
void launch_ingest_pack(hipStream_t st, const PackCols &p, uint32_t n, const uint32_t *rows, uint32_t nsrc, uint8_t *out);
// ... with corner lists (hry_mesh_from_device_corners): further bits of IngestStatus::err
constexpr uint32_t kIngestBadTexIndex = 4, kIngestBadNormalIndex = 8, kIngestManyRegions = 16;
constexpr uint32_t kIngestMaterials = 65536, kIngestMaxRegions = 128;
// the two slots of corner_attr: the index buffer of the slot's list (nullptr: unused, the slot holds 0), its rows, the weld's map of
// the list (or nullptr) and the bit an index outside [0, rows) raises
struct CornerSlots { const void *idx[2]; const uint32_t *remap[2]; uint32_t rows[2], bad[2]; };
void launch_ingest_corner_attr(hipStream_t st, const CornerSlots &cs, bool idx64, uint32_t ne, uint32_t *corner_attr, IngestStatus *status);
// face regions from a material per face: first[kIngestMaterials] filled with 0xff and rank[kIngestMaterials] zeroed before; the
// number of distinct materials goes to *n_regions, more than kIngestMaxRegions raises kIngestManyRegions
void launch_ingest_regions(hipStream_t st, const uint16_t *mat, uint32_t nf, uint32_t *first, uint32_t *rank, uint32_t *n_regions, uint16_t *face_reg,
                           IngestStatus *status);

}   // namespace dev
}   // namespace hry
