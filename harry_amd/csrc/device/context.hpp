// Device context of the codec: HIP device, one stream, grow-only workspace buffers, resident mesh.
#pragma once
#include <chrono>
#include <cstdio>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../host/host.hpp"
#include "dev_types.hpp"
#include "hip_handles.hpp"

namespace hry {

typedef std::chrono::steady_clock Clock;
inline double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }
// HRY_TRACE's time line: ms since t0, after the prefix the file names (kMarkPrefix: "[hry enc]" for the encoder, "[hry]" for the decoder)
#define HRY_MARK(t0, what) do { if (trace_on()) fprintf(stderr, "%s %8.3f ms  %s\n", kMarkPrefix, ms_since(t0), what); } while (0)

constexpr int kMaxLists = 16;   // attribute lists of one mesh kept in HBM (the OBJ reader creates at most 8)

// A result handle's buffers (render.cpp, order.cpp, distortion.cpp): pieces (hip_handles.hpp: Carve) of the one allocation the
// handle owns, found by name
struct NamedBuf {
	std::string name;
	void *p = nullptr;
	uint64_t rows = 0;
	int width = 0, type = 0;   // components a row, HRY_FLOAT / HRY_UINT / HRY_USHORT
	size_t bytes() const { return (size_t)rows * (size_t)width * (type == HRY_USHORT ? 2u : 4u); }
};
struct DeviceResult {
	DeviceBlock block;
	std::vector<NamedBuf> bufs;
	const NamedBuf *find(const std::string &name) const { for (const NamedBuf &b : bufs) if (b.name == name) return &b; return nullptr; }
	template <typename T> T *ptr(const char *name) const { return (T*)find(name)->p; }   // of a buffer the result is known to have
};
// a named buffer of any of the three results to dst (device or host memory), on cx's stream, waited for (defined in render.cpp).
// what: what the handle calls a buffer ("numbering map"), for the refusals.  same_device: refuse a result that lives on another
// device than cx's -- hry_order_copy and hry_distortion_copy ask for it, hry_render_copy does not
struct Context;
void result_copy(Context &cx, const DeviceResult &r, const char *name, const char *what, void *dst, bool dst_is_device, bool same_device);
// order.cpp: the numbering maps of one encode (include/harry_amd.h: hry_order_take), width 1 HRY_UINT
typedef DeviceResult OrderResult;
// general bindings: where an encode left the records of a list that it coded as data, in creation order (d_idx, in cx.d_gen)
struct OrderListSource { const uint32_t *d_idx = nullptr; uint32_t nd = 0; };

struct Context {
	int device = 0;
	// Streams and events own themselves (hip_handles.hpp) and, but for the main stream, are created when they are first used --
	// by the thread that drives the context: a handle that a side thread uses is touched before that thread starts
	Stream stream;    // (created with the context, at the highest priority)
	Stream stream2;   // uploads and connectivity-only kernels of the pipelined decode
	Stream stream3;   // attribute streams' entropy decode, next to the connectivity streams'
	static constexpr int kUploadStreams = 2;
	Stream up_stream[kUploadStreams];   // further uploaders of finished spans beside stream2 (unchunk.cpp: SpanUploader)
	Event up_ev[kUploadStreams];
	Event ev_x[2];                   // cross-stream ordering events
	Event ev_payload;                // chunked decode: the attribute streams' part of a large payload is on the device
	// chunked decode: the attribute streams are launched in groups by how far into their plane they end (unchunk.cpp); group g
	// runs on attr_stream(g) -- stream3 for the first group -- and raises attr_ev[g]
	static constexpr int kAttrGroups = 3;   // (+ the codec's three streams: more streams than hardware queues serialise)
	Stream attr_more[kAttrGroups - 1];
	hipStream_t attr_stream(int g) { return g ? attr_more[g - 1].get() : stream3.get(); }
	Event attr_ev[kAttrGroups];
	PinBuf h_down;                   // pinned landing buffer for the vertex records of the pipelined decode (device -> host per slice)
	PinBuf h_mirror;                 // pipelined decode with border snapshots: pinned copies of the helper threads' stretches (face offsets, origins, twins, decode order), made by the helpers themselves
	PinBuf h_stage;                  // pinned staging memory for uploads that run next to a busy host thread (copies from pageable
	                                 // memory make the runtime pin and unpin pages: TLB shootdowns for every thread; unchunk.cpp: Stager)
	Stream pipe_stream;              // chunked encode: what finished groups of a walk on several threads have coded goes to the planes beside the walk (chunked.cpp: EncodePipeline)
	Event pipe_ev;
	static constexpr int kPipeSlots = 3;
	Event pipe_slot_ev[kPipeSlots];   // a slot of h_pipe / d_pipe is free again
	TimedEvent ev[8];
	// the float chains of a large mesh run in batches (unchunk.cpp: ChainBatches): a pair of timing events around every batch's
	// launches, so that hry_timing.k_chain_ms is the sum over the batches of a decode
	static constexpr int kChainBatchEvents = 16;
	TimedEvent chain_ev[2 * kChainBatchEvents];
	hry_timing timing{};

	// resident mesh (hry_mesh_upload): attribute records and connectivity stay in HBM across encodes
	uint64_t resident_token = 0;
	uint64_t gen_token = 0;          // the mesh whose binding tables (d_vreg .. d_cattr) are in HBM (general.cpp: upload_general)
	uint64_t render_token = 0;       // the mesh the last hry_decode returned, while d_rec / d_foff / d_org (and the binding tables) still
	                                 // hold it: hry_render_build reads them instead of uploading (render.cpp); any other call clears it.
	                                 // Drawn from ONE counter of the process (mark_decoded): no two contexts ever hand out the same token
	bool render_whole = false;       // ... the mesh is a sharded container decoded here: its records and connectivity are in d_whole_*
	uint32_t render_nf = 0, render_ne = 0;
	DevBuf d_whole_rec[2], d_whole_foff, d_whole_org, d_whole_runs;   // decode_sharded on ONE context, PLY layout: the segments' device results placed into the whole numbering (render.cpp: place_segment)
	DevBuf d_rec[kMaxLists], d_org, d_twin, d_foff, d_eface;
	DevBuf d_vreg, d_freg, d_vattr, d_cattr, d_fattr, d_gen;   // general bindings (general.cpp): region and record tables, event arena
	uint32_t res_nv = 0, res_nf = 0, res_ne = 0, res_udeg = 0;
	bool res_has_eface = false;

	// reciprocal table, valid for totals < magic_n
	DevBuf d_magic;
	uint32_t magic_n = 0;

	// workspace
	DevBuf d_order_v, d_order_f, d_rank, d_vplanes, d_fplanes, d_connplanes, d_grp_val, d_grp_pos, d_op, d_jobs, d_chunks, d_hist, d_init,
	       d_rec_sym, d_sym_l, d_r, d_s, d_state, d_acc, d_v, d_summary, d_bytes, d_small;
	// chunked profile
	DevBuf d_cjobs, d_cscratch, d_csizes, d_coffs, d_cout, d_csyms, d_patch;
	DevBuf d_render;   // hry_render_build: its uploads (a mesh that is not resident) and working arrays (render.cpp)
	DevBuf d_edges;    // hry_edges_build: the numbering's table and working arrays, counters, the list of long segments (edges.cpp)
	DevBuf d_orient;   // hry_orient_build: the double cover's union-find, the scan, the patches' turns, the measures' working arrays (orient.cpp)
	DevBuf d_tangents; // hry_tangents_build: the triangles' terms and signs, counters, segment starts, the segments, the list of long segments (tangents.cpp)
	DevBuf d_creases;  // hry_creases_build: the slots' union-find, roots and scan, the numbering's table, the triangles' terms, the groups' segments and normals (creases.cpp)
	DevBuf d_curvature;   // hry_curvature_build: the ends' flags, counters, segment starts, the segments, the list of long segments, the decoded vertices' rows and the totals' rounds (curvature.cpp)
	DevBuf d_bvh;   // hry_bvh_build: the live flags and their scan, the sort's two sides and counters, the tree's children and parents; hry_bvh_cast / hry_bvh_nearest: the staged rays or points and results of a host query, the counters; hry_intersections_build: the words that come down, the leaves' counts and their scan, the sort's two sides (bvh.cpp)
	DevBuf d_shells;   // hry_shells_build: the union-finds, the pairs' numbering, the chunks' partial sums and their segments (shells.cpp)
	DevBuf d_distortion;   // hry_distortion_build: its uploads (what is not resident), the blocks' records, results and status word (distortion.cpp)
	DevBuf d_sweep;   // hry_quant_sweep_build: its uploads (a mesh that is not resident), the blocks' records and the results (sweep.cpp)
	DevBuf d_ingest;   // hry_mesh_from_device: status word, scans, the weld's keys and table (ingest.cpp)
	DevBuf d_split;   // chunked encode in two kernels: per stream the place of its records and the streams' order, longest first (the records: d_rec_sym)
	DevBuf d_pipe, d_nt_val, d_nt_planes;   // EncodePipeline: run tables and twin pairs of the batches; the polygons' triangle counts and their two byte planes
	std::vector<uint32_t> h_twin_patch;   // (half-edge, twin) pairs on their way to d_patch (upload_repaired_twins)
	std::vector<uint32_t> inplace_twin_patches;   // a shard coded in place: the half-edges whose twins its walks repaired in the WHOLE mesh's host array (sharded.cpp brings them to the resident copy on another device)

	// HRY_FLAG_ORDER: the running hry_encode builds the numbering maps behind its own work (order.cpp: order_build) and leaves them
	// in `order` under order_token, which the mesh shares until any other call on the context or the mesh clears it (api.cpp)
	bool want_order = false;
	uint64_t order_token = 0;
	std::unique_ptr<OrderResult> order;
	std::vector<OrderListSource> order_lists;   // general bindings: filled by the encode's reference pass, read by order_build
	DevBuf d_order_ws;                          // order_build: orders that the encode did not bring up, degrees, offsets, scan sums

	bool keep_stages = false;
	bool device_recurrence = false; // HRY_FLAG_DEVICE_RECURRENCE: k_rchain instead of the host core
	PinBuf h_pipe;                  // chunked encode: the pipeline's staging slots (run tables + the runs' entries, gathered)
	PinBuf h_fetch;                 // large results on their way down: a ring of pinned slots (fetch_to_host, codec.cpp)
	Event stage_ev[8];              // ... and an event per slot
	PinBuf h_gen;                   // general bindings: the events' arena on its way up (general.cpp)
	PinBuf h_small;                 // a few words that come down asynchronously (a copy into pageable memory keeps its caller until it has happened)
	PinBuf h_conn;                  // chunked decode: the connectivity planes, down for the host's replay
	PinBuf h_rec, h_r, h_s;         // compat: symbol records down, (r, S) up, slice by slice (codec.cpp finish_stream)
	std::vector<Event> slice_ev;
	std::map<std::string, std::vector<uint8_t>> stages;

	explicit Context(int dev);
	~Context();
	void stage_put(const char *name, const void *dptr, size_t bytes);
	void stage_put_host(const char *name, const void *hptr, size_t bytes);
	void ensure_magic(uint32_t n);
	void upload_mesh(Mesh &m, bool with_records = true);
	void adopt_conn(Mesh &m);        // the connectivity is in d_foff / d_org / d_twin already (unchunk.cpp: SpanUploader): the rest of upload_mesh
	void conn_state(const Mesh &m);  // d_foff / d_org hold m's connectivity: the face of every half-edge (mixed degrees) and res_*
	// m.twins_pending, its connectivity in d_foff / d_org (conn_state done) and every index below nv: the twins matched on the
	// device (twins.hip; hubs on the host, from m's host arrays) into d_twin and m.twin
	void match_twins(Mesh &m);
	void make_resident(Mesh &m);     // m and this context share a new token (drawn from one counter of the process): m is resident here
	dev::ConnView conn_view() const;
	float elapsed(int a, int b);
};

// ---- planes of the chunked container (chunked.cpp, unchunk.cpp, general.cpp; their layout: host.hpp)
struct PlaneRef { const uint8_t *dptr; uint32_t n; int init; };
// encode: collects the references on the host, computes the residuals on the device, returns the planes (device pointers into
// cx.d_gen) in layout order; order_v / order_f / repaired twins must be resident (d_order_v, d_order_f, d_twin)
void general_planes_encode(Context &cx, Mesh &m, const WalkResult &w, std::vector<PlaneRef> &planes);
// decode: the decoded planes (device, plane k at d_syms + plane_off[k], nsym[k] symbols; first = index of the first attribute
// plane) -> bindings + records of m
void general_planes_decode(Context &cx, Mesh &m, const OrderVec &order_v, const std::vector<uint32_t> &seg_start,
                           const std::vector<uint32_t> &seg_level, const uint8_t *d_syms, const std::vector<uint64_t> &plane_off,
                           const std::vector<uint32_t> &nsym, uint32_t first);

void check_general(const Mesh &m);             // general.cpp
// device -> pageable host memory, behind everything on cx.stream; returns when the bytes are there (codec.cpp)
void fetch_to_host(Context &cx, void *dst, const void *d_src, size_t bytes);
void upload_general(Context &cx, Mesh &m);     // connectivity + every list + the binding tables -> HBM

// codec entry points (codec.cpp / chunked.cpp)
// records: m holds the lists' formats and counts only, their records are those of *records and nothing else travels to the device
void device_bounds(Context &cx, Mesh &m, const Mesh *records = nullptr);
// analysis.cpp: host/cbm_walk.cpp's analyse_components on the device, for a mesh resident on cx (every table but the per-face labels)
// everything: for tests -- no early return for a mesh of one component, and the labels copied down into A.comp
void device_component_analysis(Context &cx, const Mesh &m, ComponentAnalysis &A, bool everything = false);
void device_requant(Context &cx, Mesh &m, const hry_quant *q, size_t nq, bool clear);
std::vector<std::vector<uint8_t>> requant_targets(const Mesh &m, const hry_quant *q, size_t nq, bool clear);   // validated request -> quantisation of every component
dev::RequantPlan requant_plan(const AttrList &L, const std::vector<uint8_t> &to);
// the twins the walk repaired (cbm/encoder.h:150,193-198) into the resident copy: the few entries it names, else the whole array
void upload_repaired_twins(Context &cx, const Mesh &host, const WalkResult &w, bool patches_only = false);
// the front half of the vertex attributes' pass (codec.cpp; shared by encode_compat and rate_sweep_build): the walk's order_v into
// d_order_v with its repaired twins; then the rank of every vertex in it into d_rank
void upload_coding_order(Context &cx, const Mesh &m, const WalkResult &w);
void rank_coding_order(Context &cx, const Mesh &m, uint32_t vc);
uint64_t test_extra(const char *name);   // HRY_TEST_EXTRA_SYMBOLS / _BITS: counted on top of a reference stream's own (tests of the format's limits)
void encode_compat(Context &cx, Mesh &m, std::vector<uint8_t> &out);
// ---- compat_stream.cpp: what encode_compat and encode_general share of the reference stream
// the connectivity symbols of a walk on the device: group g's values and positions at d_grp_val / d_grp_pos + goff[g] (room for
// their byte planes in d_connplanes), in d_op the operation bytes, op_position_table's thr / cum and the operation model's scratch
struct ConnSymbols {
	size_t goff[G_COUNT + 1];
	uint32_t nop, ngr;
	uint8_t *d_opsc;
	uint32_t *d_opthr, *d_opcum;
	void *d_opscratch;
};
ConnSymbols upload_conn_symbols(Context &cx, const WalkResult &w);
// the groups' values in d_grp_val -> their byte planes in d_connplanes (numtri false: but for the polygons' triangle counts --
// chunked.cpp: its pipeline has split them already)
void split_conn_groups(Context &cx, const WalkResult &w, bool numtri = true);
void launch_conn_models(Context &cx, const WalkResult &w, const ConnSymbols &cs);   // split_conn_groups, then the operation model's records
// the model jobs of one stream: every byte plane with its initial counts (an INIT_* kind of build_init_tables) and the position of
// its symbols in the stream -- pos_tab[j] + pos_add, or with no table pos_base + j * pos_stride; empty planes are skipped
struct ModelJobs {
	Context &cx;
	std::vector<uint32_t> inits;
	uint32_t total[INIT_KINDS] = {};
	std::vector<dev::PlaneJob> jobs;
	std::vector<dev::ChunkRef> chunks;
	uint32_t max_total = 2;   // the largest total a model of the stream reaches: the reciprocal table covers it
	ModelJobs(Context &cx, const Mesh &m);
	void add(const uint8_t *sym, uint32_t n, int init, const uint32_t *pos_tab, uint32_t pos_add, uint32_t pos_base = 0, uint32_t pos_stride = 0);
	void add_conn(const WalkResult &w, const ConnSymbols &cs);   // the planes of the connectivity groups
	void send(const ConnSymbols &cs, uint32_t ns);               // tables, jobs and chunks -> HBM; reciprocals and the records of ns symbols sized
	void run();                                                  // launch_model on the jobs
};
// finish_stream, the payload behind what `out` holds, the timing record of an encode that began at t_all
void finish_compat_stream(Context &cx, uint32_t ns, Clock::time_point t_all, std::vector<uint8_t> &out);
// A shard coded where it lies in the whole mesh (sharded.cpp: the in-process executor): the mesh handed to encode_chunked is a
// SKELETON -- the shard's sizes, the lists' formats and bounds, its runs, no arrays; the context's connectivity and record arrays
// are those of the whole mesh in the whole mesh's numbering, filled over the shard's index intervals; the walk goes over the
// whole mesh's host arrays with the shard's components.
struct InPlaceShard {
	Mesh *whole;
	const ComponentAnalysis *part;                                   // the shard's components (shard_components)
	const uint32_t *eface;                                           // face of every half-edge of the whole mesh (mixed degrees), else nullptr
	WalkState *marks;                                                // of the whole mesh; shared by the workers
	const std::vector<std::pair<uint32_t, uint32_t>> *face_intervals;   // the shard's faces, as uploaded (repaired twins go up over the same intervals)
	std::function<void()> arrays_ready;                              // called after the walk, before anything touches the device: returns when the
	                                                                 // shard's intervals are in HBM (and quantised, if the caller quantises)
};
void encode_chunked(Context &cx, Mesh &m, int chunk_syms, ByteSink &out, const InPlaceShard *in_place = nullptr);   // (bytes that are not zero-filled first and go to the caller as they are)
void encode_general(Context &cx, Mesh &m, std::vector<uint8_t> &out);   // general.cpp: regions, shared records, corner lists (reference stream only)
Mesh *decode_general(Context &cx, const uint8_t *p, size_t n, size_t hdr, std::unique_ptr<Mesh> m);
void finish_stream(Context &cx, uint32_t ns, std::vector<uint8_t> &payload);
Mesh *decode_any(Context &cx, const uint8_t *p, size_t n, int shard_index = 0, int shard_count = 0, bool allow_partial = false);
// sharded.cpp: one mesh over several contexts (devices) from one process
void encode_sharded(Context *const *cxs, int n_ctx, Mesh &m, const hry_quant *q, size_t nq, bool clear, int n_shards, int chunk_syms,
                    ByteSink &out, hry_shard_timing &st, bool store_bounds = true);
Mesh *decode_sharded(Context *const *cxs, int n_ctx, const uint8_t *p, size_t n, size_t hdr, std::unique_ptr<Mesh> g, int shard_index, int shard_count,
                     bool allow_partial, hry_shard_timing *st);
void range_encode_lht(Context &cx, const uint64_t *lht, size_t n, std::vector<uint8_t> &out);

// render.cpp: a mesh as device buffers a GPU program draws (include/harry_amd.h: hry_render_build); the result owns its memory
struct RenderResult : DeviceResult {
	uint32_t nverts = 0;
	uint64_t ntris = 0;
	double device_ms = 0;
	uint64_t uploaded_bytes = 0;
};
// marks m as what cx holds in HBM after a decode (unchunk.cpp, general.cpp; whole: sharded.cpp, the mesh is in d_whole_*), with a
// token unique in the process; a mesh whose connectivity the context does not hold stays unmarked
void mark_decoded(Context &cx, Mesh &m, bool whole = false);
// decode_sharded on one context (PLY layout): the segment just decoded (cx's d_rec / d_foff / d_org, the segment's numbering) into
// d_whole_* at its runs' places in the whole numbering; false (nothing placed) when the context does not hold the segment
bool place_segment(Context &cx, const Mesh &seg, const std::vector<ShardRun> &runs, uint32_t gnv, uint32_t gnf, uint32_t gne);
// cx still holds the decode of m (mark_decoded's token on both, the same connectivity; of a sharded container only the PLY layout
// is placed whole); then list l's records are in decoded_records(cx, l) -- whose capacity the caller checks for the lists it reads
bool holds_decode(const Context &cx, const Mesh &m);
inline const DevBuf &decoded_records(const Context &cx, size_t l) { return cx.render_whole ? cx.d_whole_rec[l] : cx.d_rec[l]; }
void render_build(Context &cx, const Mesh &m, uint32_t flags, RenderResult &out);   // flags: HRY_RENDER_*
// the list whose first three POS components are the positions the normals (and the edges' geometry) are computed from; `what`
// opens the refusals' text (HRY_E_UNSUPPORTED)
size_t render_position_list(const Mesh &m, const char *what);   // (render.cpp: position_list)

// (the edges, shells and orient builds behind a render build: result_build.hpp)

// every component of list L as hry_requant(clear) would leave it, for a kernel that reads the records in place (render.cpp): the
// quantised ones dequantised, the others as they are.  More than 32 components: HRY_E_UNSUPPORTED; quantised without bounds: HRY_E_ARG
dev::RequantPlan dequant_plan(const AttrList &L);

// distortion.cpp: per-component error of one mesh against another (include/harry_amd.h: hry_distortion_build).  The result owns the
// per-row buffers (one allocation) and the host copy of the statistics
struct DistortionResult : DeviceResult {             // bufs: "error<l>" with HRY_DISTORTION_ROWS, width 1 HRY_FLOAT
	std::vector<std::vector<hry_comp_error>> comp;   // per list; empty: the list is not compared
	hry_pos_error pos{};
	int pos_comp = -1;                               // the first of the three position components in list pos.list
	hry_normal_error nrm{ 0, 0, 0, 0, 0, 0, 0, 0, -1 };   // HRY_DISTORTION_NORMALS: the faces' normal deviation; list -1: nrm_why says why not
	std::string nrm_why = "HRY_DISTORTION_NORMALS was not set";
	double device_ms = 0;
	uint64_t uploaded_bytes = 0;
};
// the normal deviation can be taken over m's faces (normal_sweep.hip): a position list, faces, the PLY layout; why: why not
bool normals_comparable(const Mesh &m, std::string &why);
// m's connectivity for k_normal_sweep / k_distortion_normals: every face a triangle (no face offsets are read)
bool all_triangles(const Mesh &m);
// general bindings: the record of the position list pl that every vertex names, by one k_rows_of pass into a build's working buffer.
// reserve() while sizing (tables_there: m is the resident mesh -- its binding tables are read in place where the context holds
// them), launch() on the stream: the table's device address, nullptr in the PLY layout (row v is vertex v)
struct VertexRows {
	bool general = false, in_place = false;
	std::vector<int32_t> slot;   // per vertex region: the slot that binds pl
	size_t w_slot = 0, w_vreg = 0, w_vattr = 0, w_idx = 0;
	void reserve(const Context &cx, const Mesh &m, int pl, bool tables_there, Carve &W);
	const uint32_t *launch(Context &cx, const Mesh &m, int pl, const Carve &W, void *wb, uint64_t &uploaded) const;
};
void distortion_build(Context &cx, const Mesh &a, const Mesh &b, const OrderResult *o, uint32_t flags, DistortionResult &out);
bool distortion_compares(const Mesh &m, size_t l);   // list l is one hry_distortion_build compares
int distortion_position_list(const Mesh &m);         // the list whose first three POS components are the positions, or -1

// sweep.cpp: the error of every quantisation width of m's unquantised components (include/harry_amd.h: hry_quant_sweep_build).
// The result is the host table only
struct SweepResult {
	struct Comp {
		int qmax = 0, type = 0;          // swept at 1 .. qmax bits; 0: not swept, `why` says why
		std::string why;
		double extent = 0;               // the shared extent (requant_plan's scale) as a double
		std::vector<hry_comp_error> by_bits;   // [qmax], index bits - 1
	};
	std::vector<std::vector<Comp>> comp;   // per list and component
	int pos_list = -1, pos_comp = -1;      // the position list and the first of its three components (-1: none)
	std::vector<hry_pos_error> pos;        // [min of the three qmax], index bits - 1; empty: the three are not all swept
	bool nrm_asked = false;                // built with HRY_SWEEP_NORMALS
	std::vector<hry_normal_error> nrm;     // [pos.size()], index bits - 1; empty: nrm_why says why
	std::string nrm_why;
	double device_ms = 0;
	uint64_t uploaded_bytes = 0;
};
int swept_widths(const Mesh &m, size_t l, int c, dev::RequantComp &rc, std::string &why);   // 1 .. the result; 0: not swept, why says why
void quant_sweep_build(Context &cx, Mesh &m, uint32_t flags, SweepResult &out);   // flags: HRY_SWEEP_*; (computes bounds where unset, as device_requant does)
// host only: the smallest width whose record meets (metric, value), 0: none; and the requests that meet a set of tolerances
int quant_pick(const hry_comp_error *by_bits, int n_bits, int metric, double extent, double value);
std::vector<hry_quant> quant_choose(const SweepResult &s, const hry_tolerance *t, size_t nt);

// rate.cpp: the byte-plane histograms of list 1's residual codes at every quantisation width (include/harry_amd.h:
// hry_rate_sweep_build).  The result is the host table only
struct RateResult {
	struct Comp {
		int qmax = 0, type = 0;          // swept at 1 .. qmax bits; 0: not swept, `why` says why
		bool row0 = false;               // the component as it stands is counted; else why0 says why not
		int planes0 = 0;                 // ... in that many byte planes
		std::string why, why0;
		std::vector<uint32_t> hist;      // rows of 4 x 256 counters: as it stands (two rows, eight planes), then one per width (rate_row)
	};
	std::vector<std::vector<Comp>> comp;   // per list and component
	uint32_t coded = 0;
	double device_ms = 0, walk_ms = 0;
	uint64_t uploaded_bytes = 0;
};
void rate_sweep_build(Context &cx, Mesh &m, RateResult &out);
// host only.  rate_hist_bytes: the zeroth-order entropy of a histogram in bytes; rate_planes: byte planes of a component at `bits`;
// rate_bytes: the sum over the planes of one row; rate_pick: the LARGEST width whose bytes fit the budget, 0: none;
// rate_choose: one common width for component c of list l (-1: every swept one)
double rate_hist_bytes(const uint32_t *hist);
const uint32_t *rate_row(const RateResult::Comp &C, int bits);   // the planes of one row, 256 counters each
int rate_planes(const RateResult &s, int l, int c, int bits);
double rate_bytes(const RateResult &s, int l, int c, int bits);
int rate_pick(const double *bytes_by_bits, int n_bits, double budget);
int rate_choose(const RateResult &s, int l, int c, double budget, double *bytes);

// order.cpp.  order_build: at the end of an encode with cx.want_order -- m's connectivity is in d_foff / d_org (conn_view), w is the
// encode's walk; d_order_v / d_order_f: the walk's orders where the encode has them whole in HBM, else nullptr (they go up from w);
// general bindings: cx.order_lists names every list's records in creation order.  Leaves the maps in cx.order, waited for.
void order_build(Context &cx, const Mesh &m, const WalkResult &w, const uint32_t *d_order_v, const uint32_t *d_order_f);
void order_apply(Context &cx, const OrderResult &o, const char *kind, int direction, const void *d_src, uint64_t src_stride, void *d_dst, uint64_t dst_stride,
                 uint64_t row_bytes, uint64_t dst_rows);

// ingest.cpp: hry_mesh_from_device (include/harry_amd.h); the result is resident on cx
// a caller's buffer is device memory of cx's device and, where the runtime can say, [p, p + bytes) lies inside one allocation: else HRY_E_ARG
void check_device_memory(const Context &cx, const void *p, uint64_t bytes, const std::string &what);
Mesh *mesh_from_device(Context &cx, uint32_t nv, const hry_dev_column *vcols, int v_ncomp, uint32_t nf, const uint8_t *d_degrees,
                       const void *d_indices, int index_type, uint64_t n_indices, const hry_dev_column *fcols, int f_ncomp, int flags,
                       uint32_t *d_remap);
// ... hry_mesh_from_device_corners: general bindings as the OBJ reader creates them, resident with their tables (as after upload_general)
Mesh *mesh_from_device_corners(Context &cx, const hry_dev_rows *pos, const hry_dev_rows *tex, const hry_dev_rows *nrm, uint32_t nf,
                               const uint8_t *d_degrees, int index_type, uint64_t n_indices, const uint16_t *d_face_material, int flags,
                               uint32_t *const d_remap[3]);
constexpr const char *kTooManyRegionsText = "more than 128 regions: the reference seeds its region models out of bounds (model.h:49-55)";   // check_general

dev::ListDesc make_list_desc(const AttrList &L);
void check_codable(const Mesh &m);

}   // namespace hry
