// Plain structs shared between host launch code and HIP kernels (the adjacency of a render build's triangles: tri_adjacency.hpp).
#pragma once
#include <cstdint>

#include "tri_adjacency.hpp"

namespace hry {
namespace dev {

constexpr int kMaxComp = 32;
constexpr int kChunk = 2048;        // symbols per model-evaluation chunk (one wavefront walks one chunk)
constexpr uint32_t kNoRank = 0xffffffffu;

// one attribute list as the kernels see it
struct ListDesc {
	int32_t ncomp, stride, nplanes;
	uint8_t stype[kMaxComp];   // storage type (mixing::Type value) of each component
	uint8_t otype[kMaxComp];   // original type
	uint8_t quant[kMaxComp];
	uint16_t off[kMaxComp];    // byte offset of the component's slot in a record
	uint16_t plane[kMaxComp];  // index of the component's first byte plane
};

struct ConnView {
	const uint32_t *org, *twin, *foff, *eface;   // eface == nullptr when every polygon has udeg edges
	uint32_t udeg, nf, ne;
};

// general bindings as the kernels see them (mesh.hpp Bindings): element -> region, element x slot -> record of the bound list
struct GenView {
	const uint16_t *vtx_reg, *face_reg;
	const uint32_t *vtx_attr, *corner_attr;
	int32_t nb_vtx, nb_corner;
};
// which lists a region binds at its slots (Bindings: off_* / reg_*: region r's slots are [off[r], off[r + 1])), and the faces' own
// records -- what the device needs beside GenView to say which record every element names (events.hip)
struct EvRegions {
	const int32_t *off_face, *off_vtx, *off_corner;
	const uint16_t *face_lists, *vtx_lists, *corner_lists;
	const uint32_t *face_attr;
	int32_t nb_face;
};

// dedup.hip (UnweldKey): the corner keys of the render build's unweld (general bindings with corner lists); cslot[r * nlists + k] = slot of the k-th corner
// list in face region r's corner slots, -1 where the region does not bind it; n, mask and table (mask + 1 slots, kNone = empty) are the launcher's, from its DedupPlan
struct UnweldView {
	const uint32_t *org, *eface, *corner_attr;
	const uint16_t *face_reg;
	const int32_t *cslot;
	uint32_t n, nf, nregs, nlists, nb_corner, mask;   // n: corners
	uint32_t *table;
};
// dedup.hip (EdgeKey): the sides of a render build's triangles (edges.cpp).  Side s = 3 t + k joins indices[s] to
// indices[3 t + (k + 1) % 3]; its key is the unordered pair of their vertex_source entries.  nout: rows of vsrc; n (sides), mask and
// table are the launcher's, from its DedupPlan
struct EdgeView {
	const uint32_t *indices, *vsrc;
	uint32_t n, nout, mask;
	uint32_t *table;
};
// edges.hip: what the kernels behind the numbering read and write.  indices / vsrc as above; tri_edges[n]: the edge of every side;
// offsets[ne + 1] / sides[n]: the CSR of the edges' sides; pos: float rows of pos_stride floats whose first three are an output
// vertex's position, nullptr: no geometry (length / cot / cos are not written)
struct EdgesView {
	const uint32_t *indices, *vsrc, *tri_edges;
	uint32_t *offsets, *sides, *edges, *neighbours;
	const float *pos;
	float *length, *cot, *cos;
	uint32_t n, nout, ne, pos_stride;
};
// dedup.hip (ShellVertexKey): the 3 T corners of a render build's triangles (shells.cpp).  The key of corner c is the pair (shell of
// its triangle, decoded vertex vsrc[indices[c]]): the same decoded vertex within the same shell.  n (corners), mask and table are
// the launcher's, from its DedupPlan
struct ShellVertexView {
	const uint32_t *indices, *vsrc, *tri_shell;
	uint32_t n, nout, mask;
	uint32_t *table;
};
// shells.hip: the adjacency it reads (tri_adjacency.hpp) and what it writes.  ns shells (0 until they are counted); counts: ns rows of 8
struct ShellsView : TriAdjacency {
	uint32_t *tri_shell, *face_shell, *edge_shell, *first, *counts;
	uint32_t ns;
};
// the working arrays of shells.hip, laid out by shells.cpp: par / flag [T], num [T + 1], sums: scan_sums_words(T) (it serves the
// scan over the T flags and the measures' over the ns <= T counters); pair_id / pair_first_of: the ids and first_of of the corners'
// numbering [3 T]; slot [3 T] filled with 0xff; loop_par [ne]; summary: 8 zeroed words
struct ShellsWork {
	uint32_t *par, *flag, *num, *sums, *pair_id, *slot, *loop_par, *summary;
	const uint32_t *pair_first_of;
};
// orient.hip: the adjacency it reads and what it writes.  np patches (0 until they are counted); counts: np rows of 8; oriented: T
// rows of 3; measures: np rows of 8 as measures.hip leaves them, nullptr: none
struct OrientView : TriAdjacency {
	uint32_t *tri_patch, *tri_flip, *face_flip, *oriented, *first, *counts;
	float *measures;
	uint32_t np;
};
// the working arrays of orient.hip, laid out by orient.cpp: par [2 T] (the double cover: node 2 t is triangle t as wound, 2 t + 1
// turned), flag [T], num [T + 1], sums: scan_sums_words(T), turn [np] zeroed, summary: 8 zeroed words
struct OrientWork {
	uint32_t *par, *flag, *num, *sums, *turn, *summary;
};
// measures.hip: exactly what its kernels read and write.  indices: ntri rows of 3 output vertices; label[ntri]: the shell or patch
// of every triangle, below nl; first[nl]: the lowest triangle of every label; pos: float rows of pos_stride floats whose first three
// are an output vertex's position (nout rows); measures: nl rows of 8 (area, signed volume, min x y z, max x y z)
struct MeasuresView {
	const uint32_t *indices, *label, *first;
	const float *pos;
	float *measures;
	uint32_t ntri, nout, nl, pos_stride;
};
// ... and their scratch (kernels.hpp: measures_reserve / measures_bind / measures_clear): flag [T] and sums, scan_sums_words(T),
// lent by the caller; partial [T] pairs of doubles, pcount [nl] zeroed, pstart [nl + 1], pseg [T], box_lo / box_hi [nl, 3] filled
// with 0xff / 0, hubs: 1 + shells_hub_capacity(T) words, the first zeroed
struct MeasuresWork {
	uint32_t *flag, *sums;
	double *partial;
	uint32_t *pcount, *pstart, *pseg, *box_lo, *box_hi, *hubs;
};
// render.hip: which record of one list every output row names.  Row u -> element src[u] (or u) -> the region of efc[element]
// (or of the element) -> slot[region] (-1: unbound) -> attr[element * nb + slot]
struct RowsView {
	const uint32_t *src, *efc, *attr;
	const uint16_t *reg;
	const int32_t *slot;
	uint32_t nelem, nowner, nregs, nb, count;
};

// normals.hip: what the normals of a render build read.  pos: float rows of pos_stride floats whose first three are a vertex's
// position; eface == nullptr: every face is a triangle (corner c belongs to face c / 3, foff is not read); angle: corner-angle weights
struct NrmView {
	const uint32_t *foff, *org, *eface;
	const float *pos;
	uint32_t pos_stride, nv, nf, ne;
	int32_t angle;
};

// tangents.hip: what the tangent frames of a render build read and write.  indices[n]: the n = 3 T index slots; pos / uv / nrm: float
// rows of *_stride floats per output vertex (nout rows) whose first three / two / three are its position, texture coordinates and
// normal; angle: corner-angle weights; tangents: nout rows of 4; bitangents: nout rows of 3, nullptr: none
struct TanView {
	const uint32_t *indices;
	const float *pos, *uv, *nrm;
	float *tangents, *bitangents;
	uint32_t n, nout, pos_stride, uv_stride, nrm_stride;
	int32_t angle;
};
// ... and their working arrays, laid out by tangents.cpp: terms [T] rows of 6 doubles, sign [T], count [nout] zeroed (the scatter's
// cursors afterwards), start [nout + 1], sums: scan_sums_words(nout), seg [n], hubs: 1 + tangents_hub_capacity(n) words, the first
// zeroed, classes: 4 zeroed counters -- framed, mirrored, mixed vertices, uv-degenerate triangles
struct TanWork {
	double *terms;
	uint32_t *sign, *count, *start, *sums, *seg, *hubs, *classes;
};

// dedup.hip (CreaseKey): the 3 T index slots of a render build's triangles (creases.cpp).  The key of slot s is the pair (the output
// vertex indices[s], the root root[s] of the slot's smooth group).  n (slots), mask and table are the launcher's
struct CreaseSlotView {
	const uint32_t *indices, *root;
	uint32_t n, mask;
	uint32_t *table;
};
// creases.hip: the adjacency it reads (tri_adjacency.hpp), the edges' cosines, the float rows of the positions (pos_stride floats per
// output vertex) and what it writes.  nv: decoded vertices; ng groups and nw split vertices (0 until they are counted); angle:
// corner-angle weights; ids: the slots' split vertices ("indices" of the result)
struct CreaseView : TriAdjacency {
	const float *edge_cos, *pos;
	const uint32_t *ids;
	uint32_t *edge_class, *slot_group, *render_vertex, *vertex_source;
	float *normals;
	double cos_limit;
	uint32_t pos_stride, nv, ng, nw;
	int32_t angle;
};
// ... and its working arrays, laid out by creases.cpp: par / root / flag [n], num [n + 1], sums: scan_sums_words(n) (it serves the
// scan over the n flags and the one over the ng <= n counters); eclass [ne]; first_slot [n] (nw <= n used); terms [T] rows of 3
// doubles; count: ng <= n zeroed counters (the scatter's cursors afterwards; they lie where flag lay); start [n + 1]; seg [n] (where
// par lay); gnormal [n] rows of 3 floats (ng used); vgroups [nv] zeroed; hubs: 1 + creases_hub_capacity(n) words, the first zeroed;
// classes: 4 zeroed counters -- SMOOTH, SHARP, other edges, decoded vertices with more than one group
struct CreaseWork {
	uint32_t *par, *root, *flag, *num, *sums, *eclass, *first_slot, *count, *start, *seg, *vgroups, *hubs, *classes;
	double *terms;
	float *gnormal;
};

// curvature.hip: the adjacency it reads (tri_adjacency.hpp), the float rows of the positions (pos_stride floats per output vertex)
// and the six buffers it writes, nout rows each.  nv: decoded vertices
struct CurvView : TriAdjacency {
	const float *pos;
	uint32_t *vertex_class;
	float *area, *defect, *gaussian, *mean_normal, *mean;
	uint32_t pos_stride, nv;
};
// ... and its working arrays, laid out by curvature.cpp: ends [nv] zeroed (bit 0: an end of an edge with one side, bit 1: of one with
// more than two); count [nv] zeroed (the scatter's cursors afterwards); start [nv + 1]; sums: scan_sums_words(nv); seg [n]; hubs:
// 1 + curvature_hub_capacity(n) words, the first zeroed; cls [nv] and rows [nv] rows of 7 floats: what the expansion copies (area,
// defect, gaussian, mean_normal x y z, mean); terms [nv] rows of 3 doubles: what a vertex adds to the totals; fold_a / fold_b: the
// rounds of the totals' reduction, ceil(nv / 256) and ceil(ceil(nv / 256) / 256) rows of 3 doubles; classes: 8 zeroed counters --
// interior, boundary, irregular, isolated vertices, vertices with bit 8
struct CurvWork {
	uint32_t *ends, *count, *start, *sums, *seg, *hubs, *cls, *classes;
	float *rows;
	double *terms, *fold_a, *fold_b;
};

// bvh.hip: what the hierarchy's build reads of a render build -- the indices of its T triangles and the float rows of the positions
// (pos_stride floats per output vertex, nout of them) -- and its working arrays, laid out by bvh.cpp, T entries each unless said:
// flag (1: live) and at [T + 1] (its exclusive scan: a live triangle's rank); code_a / tri_a / code_b / tri_b: the sort's two sides;
// children [T, 2]; leaf_parent / node_parent; sums: scan_sums_words(T); radix: radix_scratch_words(T) (radix_sort.hpp); words: 16
// words -- [0] L, [1] distinct codes, [2] depth, [4 .. 9] the scene box as ordered words (k_bvh_init sets them)
struct BvhWork {
	const uint32_t *indices;
	const float *pos;
	uint32_t T, nout, pos_stride;
	uint32_t *flag, *at, *code_a, *tri_a, *code_b, *tri_b, *children, *leaf_parent, *node_parent, *sums, *radix, *words;
};
// ... and the finished hierarchy: what the second stretch writes and the cast reads (L leaves, L - 1 nodes).  round [L - 1]: the
// round of the box fit that finished a node, HRY_NO_ELEMENT before (working memory, not a buffer of the handle)
struct BvhView {
	uint32_t L;
	uint32_t *leaf_tri, *leaf_code, *node_children;
	float *leaf_box, *leaf_positions, *node_box, *scene_box;
};
// one cast: n rays, origin / direction of ray i at byte i * stride of o / d (stride 0: one for all); dense outputs, t and uv may be
// null; stat: two zeroed 64-bit counters (rays that hit, box tests)
struct BvhCast {
	uint64_t n, o_stride, d_stride;
	const uint8_t *o, *d;
	double tmin, tmax;
	uint32_t *hit_tri;
	float *hit_t, *hit_uv;
	unsigned long long *stat;
};
// one closest-point query: n points, point i at byte i * q_stride of q (stride 0: one for all); r2: the squared radius; any: 0 where
// the radius is negative and no point is answered; dense outputs, all but near_tri may be null; stat: three zeroed 64-bit words
// (points answered, bounds evaluated, the bits of the largest near_d2)
struct BvhNearest {
	uint64_t n, q_stride;
	const uint8_t *q;
	double r2;
	uint32_t any;
	uint32_t *near_tri;
	double *near_d2;
	float *near_uv, *near_point;
	unsigned long long *stat;
};
// the pairs of leaves that pass through each other, one walk of two: fill == 0 writes count [L] and adds to stat, four zeroed 64-bit
// words (pairs of leaves whose boxes overlap, pairs that reach the segment tests, box tests of the walk, pairs found); fill == 1
// reads start [L], the exclusive scan of count, and writes P rows of key (s) and val (t | share << 31) and bumps tri_pairs [T],
// zeroed.  words: [0] P as the scan gave it (the sorts' length), [1] H, zeroed; T: the triangles of the render build
struct BvhPairs {
	uint32_t fill, P, T;
	uint32_t *count, *start, *key, *val, *tri_pairs, *words;
	unsigned long long *stat;
};

// render.hip: the runs of one segment of a sharded container, local first element (l*) and first element in the whole mesh (g*)
// per run and kind (vertices, faces, half-edges); gn*: sizes of the whole mesh
struct RunPlace {
	const uint32_t *lv, *lf, *lh, *gv, *gf, *gh;
	uint32_t nr, gnv, gnf, gne;
};

// per-symbol record consumed by the serial range recurrence (16 bytes, one dwordx4 per lane)
struct alignas(16) SymRec {
	uint64_t magic;    // reciprocal of the context total t (round-up method, 65-bit magic with implicit top bit)
	uint32_t x;        // multiplier: h - l, or l when the symbol is the last one with non-zero count (h == t)
	uint32_t meta;     // bits 0-5: post-shift, bit 6: h == t form (R' = R - r*x), bit 7: exact no-op (l == 0 && h == t)
};
constexpr uint32_t kMetaSub = 1u << 6, kMetaNoop = 1u << 7;

// reciprocals of a context total t: 65-bit magic + shift for 64-bit coder registers (reference stream), and m32 / sh32
// (cm::make_magic32) for the 32-bit registers of the chunked container's streams
struct alignas(16) MagicEnt { uint64_t magic; uint32_t shift; uint32_t m32; };
constexpr uint32_t kMagicSh32Shift = 8;   // MagicEnt::shift bits 8..15 hold sh32

// a byte plane whose adaptive model is evaluated by counting
struct PlaneJob {
	const uint8_t *sym;        // n symbols
	const uint32_t *pos_tab;   // global position of symbol j is pos_tab[j] + pos_add, or pos_base + j * pos_stride when null
	const uint32_t *init;      // 256 initial counts
	uint32_t n, t0;            // t0 = sum of init
	uint32_t pos_add, pos_base, pos_stride;
	uint32_t chunk0;           // index of this job's first chunk in the global chunk list
};
struct ChunkRef { uint32_t job, first; };

// chunked profile: one independent stream = one chunk of one context plane
struct StreamJob {
	const uint8_t *sym;    // symbols of the chunk (encode: input, decode: output)
	uint32_t n;            // symbols in the chunk
	uint32_t init;         // index of the 256-entry initial count table
	uint32_t t0;           // sum of the initial counts
	uint32_t word_base;    // first 32-bit word of this stream's big-number accumulator / byte image
};

// a slice of a plane for the histogram pass (static priors)
struct HistSlice { const uint8_t *sym; uint32_t n, plane; };

struct SplitBase { uint32_t b[8]; };

// the components of a list for the bounds reduction
struct BoundsPlan { int32_t n, stride; uint16_t off[kMaxComp]; uint8_t type[kMaxComp]; };

// one component of an in-place requantisation: mn / scale carry the raw bits of the component's original type
struct RequantComp { int32_t off, src_type, src_bits, dst_bits, dst_type, pad; uint64_t mn, scale; };   // dst_bits 0: dequantise into dst_type
struct RequantPlan { int32_t n; int32_t pad; RequantComp c[kMaxComp]; };

// distortion.hip: what one block of k_distortion_rows leaves per component (and, one slot behind the components, for the
// positions: mx = the largest distance, sum = the squared distances), and what k_distortion_fold makes of the blocks' records --
// the layout of hry_comp_error (include/harry_amd.h)
struct alignas(16) DistPart {
	double mx, sum, mn, mxa;
	uint32_t row, compared, skipped, nonfinite, changed, pad[3];
};   // 64 bytes
struct DistFinal {
	double mx, sum, mn, mxa;
	uint64_t compared, skipped, nonfinite, changed;
	uint32_t row, reserved;
};   // 72 bytes
// one list of a comparison: rows of a (stride sa) against rows map[i] of b (stride sb; map == nullptr: row i); pos: the first of
// the three position components, or -1; err: the per-row buffer, or nullptr
struct DistList {
	const uint8_t *a, *b;
	const uint32_t *map;
	float *err;
	DistPart *part;
	uint32_t rows, b_rows, sa, sb;
	int32_t pos, pad;
};
struct DistFold {
	const DistPart *part[16];
	uint32_t nblocks[16], nslots[16], out_at[16];   // out_at: the list's first record in the results
	int32_t n, pad;
};

// sweep.hip: one swept (unquantised) component of a list -- rc as requant_plan gives it (offset, type, minimum, shared extent; the
// bits are the kernel's) -- swept at 1 .. qmax bits; its record of width q is slot + q - 1 of the list's ns
struct SweepComp { RequantComp rc; int32_t qmax; uint32_t slot; };
// one list of a sweep: job j < n is component c[j]; job n (pos >= 0) the positions, components c[pos .. pos + 2] at one width
struct SweepList {
	const uint8_t *rec;
	DistPart *part;      // [blocks][ns]
	uint32_t rows, stride, ns, pos_slot;
	int32_t n, pos, pos_qmax, pad;
	SweepComp c[kMaxComp];
};

// normal_sweep.hip: what one block leaves per slot for the faces' normal deviation (mx = the largest chord, sum = the squared
// chords), and what k_normal_fold makes of the blocks' records -- the layout of hry_normal_error (include/harry_amd.h)
struct alignas(16) NormPart {
	double mx, sum;
	uint32_t row, compared, skipped, nonfinite, degenerate, collapsed, pad[2];
};   // 48 bytes
struct NormFinal {
	double mx, sum;
	uint64_t compared, skipped, nonfinite, degenerate, collapsed;
	uint32_t row;
	int32_t list;
};   // 64 bytes
// the faces of a mesh and where a corner's position lies: corner k names vertex org[k], whose record in the position list is row
// rows[v] (rows == nullptr: row v; kNoRank: none).  foff == nullptr: every face is a triangle (corner c belongs to face c / 3)
struct NormalFaces {
	const uint32_t *org, *foff, *rows;
	uint32_t nf, ne, nv, nrows;   // nrows: records of the position list
};
// k_normal_sweep: the three position components (rc as in SweepComp, consecutive in a record of `stride` bytes at rec) at every
// width 1 .. qmax; block b's record of width q is part[b * qmax + q - 1].  type: the components' common type, -1: they differ
struct NormalSweep {
	NormalFaces F;
	const uint8_t *rec;
	NormPart *part;
	uint32_t stride;
	int32_t qmax, type, pad;
	RequantComp c[3];
};
// k_distortion_normals: positions of a (components ca of a record at a + row * sa) against b's at row map[row] (map == nullptr: the
// same row; an entry at or above b_rows is never followed: k_distortion_rows has raised the status word for it); err: the per-face
// buffer, or nullptr
struct NormalPair {
	NormalFaces F;
	const uint8_t *a, *b;
	const uint32_t *map;
	float *err;
	NormPart *part;      // [blocks]
	uint32_t b_rows, sa, sb, pad;
	RequantComp ca[3], cb[3];
};

// rate.hip: one component of list 1 in a rate sweep.  rc.off / rc.src_type (the original type) / rc.mn / rc.scale as requant_plan
// gives them; swept at 1 .. qmax bits (0: not swept); row0: the component as it stands is counted too, in its storage type stype0 at
// quant0 bits.  The table is made of rows of kRatePlanes x 256 counters; the component's are slot .. slot + qmax + 1: two for row 0
// (kRatePlanes0 planes: a lossless 64-bit integer has eight), then row slot + 1 + bits for every width
constexpr int kRatePlanes = 4, kRatePlanes0 = 8;
struct RateComp { RequantComp rc; int32_t qmax, row0; uint32_t slot; uint8_t stype0, quant0, pad[2]; };
struct RateList {
	const uint8_t *rec;
	uint32_t *table;     // [rows][kRatePlanes][256], zeroed
	uint32_t stride;
	int32_t n;
	RateComp c[kMaxComp];
};

}   // namespace dev
}   // namespace hry
