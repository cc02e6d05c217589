// harry -- the reference's command line (main.cc:23-123) on top of the C ABI of libharry_amd.so (include/harry_amd.h):
//     harry [OPTIONS] INPUT OUTPUT      -f/--format hry|ply|obj   -l/--list L   -a/--attr A   -q/--quant Q   -c/--clear-quant
//                                       --ply-ascii   -h/--help
// Same flag state machine (-l sets the list, -a the component for the next -q only, main.cc:47-71), same phase prints
// (main.cc:99-120), same error texts; an error ends the program the way the reference's uncaught std::runtime_error does
// (message of std::terminate on stderr, status 134).  Input kind by magic number, output kind by extension
// (formats/unified_reader.h:33-56, unified_writer.h:31-47): .hry, .ply and .obj both ways.
// Additive options (the reference rejects them as invalid): --profile compat|chunked (default compat = the reference's own
// v0.1 stream), --chunk N, --device D, --gpus N (N device contexts behind this one command, devices D, D+1, ... -- more
// contexts than devices share them: the mesh shards by connected component, every context codes / decodes its shards on a
// worker thread of its own, one sharded container comes out; hry_encode_sharded / hry_decode_sharded), --shards N (number of
// shards, default one per context; both imply --profile chunked, the reference's single stream does not shard), --ply-packed
// (binary PLY of a quantised mesh with every value in the width its header declares; the reference's writer dumps the
// original-width records, formats/ply/writer.cc:72-75), --report (after the quantisation phase, what it cost: one line per component,
// "Distortion: list L attr C bits Q max M rms R changed N", the quantised mesh against a clone taken before -- hry_distortion_build
// with the identity map, since a decode returns the quantised values exactly), --max-error V / --max-error-rel V (a tolerance in
// place of -q, bound to the preceding -l / -a the same way: the largest error of the component, absolute or as a fraction of its
// shared extent; the mesh is swept once -- hry_quant_sweep_build -- and the smallest width that meets the tolerance is applied,
// "Chosen: list L attr C bits Q max M" per component; with -c the mesh is cleared first, swept, and every width is applied to the
// cleared values; without -a every component of the list is named, as by -q, and one that cannot take a tolerance -- quantised
// already and no -c, a constant integer -- ends the run with its reason), --max-bytes N (a byte budget for the written .hry in place
// of -q, bound to the preceding -l / -a: ONE common width for the named component, or every swept component of the list, such that
// the file is at most N bytes.  The mesh -- after the other quantisations -- is swept once, hry_rate_sweep_build; hry_rate_choose
// picks the starting width from N minus the fixed part, which is 0 before the first encode and afterwards the real size minus the
// estimate at the width just encoded; then real encodes step down until the file fits and up while the next width still fits:
// "Budget: list L attr C bits Q estimated E bytes" per component and "Budget: output S of N bytes after K encodes"),
// --max-normal-angle DEG (in place of -q for the position components of the preceding -l, which must be the position list; no -a: the
// smallest width at which no face's normal turns by more than DEG degrees and no face loses its normal -- the same sweep with
// HRY_SWEEP_NORMALS, HRY_TOL_NORMAL_CHORD; "Chosen: list L attr C bits Q max-angle A deg" per position component; same refusals and
// -c handling as --max-error); --report then adds, after its Distortion: lines and when the mesh has positions and faces,
// "Normals: faces F max-angle A deg rms R deg collapsed K degenerate G" (hry_distortion_build with HRY_DISTORTION_NORMALS; rms: the
// angle of the rms chord); --topology (with or without OUTPUT: after the quantisation phase one line, "Topology: vertices V faces F
// triangles T edges E boundary B manifold M nonmanifold N euler X" -- hry_render_build, hry_edges_build and hry_edges_summary: E the
// unique edges of the fan triangles over the decoded vertices, B / M / N those with one, two and more sides, X = V - E + F, which is
// the Euler characteristic for all-triangle meshes; without OUTPUT the run ends there); --shells (with or without OUTPUT, after
// --topology's line: "Shells: shells S closed C nonmanifold N misoriented M loops L largest K", then for the first 16 shells
// "Shell: I triangles T vertices V edges E boundary B loops L euler X genus G" -- hry_shells_build, hry_shells_summary and the first rows
// of "shell_counts"; X = V - E + T of the shell, G = (2 - X - L) / 2, or - where the shell has non-manifold or misoriented edges);
// --orient / --orient-outward (with or without OUTPUT, after those lines, which keep describing the source mesh: "Orientation: patches
// P orientable O flipped F inverted I against A remaining R" -- hry_orient_build with HRY_ORIENT_MAJORITY, and HRY_ORIENT_OUTWARD for
// the second, and hry_orient_summary; with OUTPUT and F > 0 the mesh that is written is hry_mesh_flip_faces(mesh, "face_flip"));
// --tangents (with or without OUTPUT, after those lines: "Tangents: vertices U framed F unframed Z mirrored M mixed X degenerate D" --
// hry_tangents_build over a render build of the mesh and hry_tangents_summary; the normals are the file's where the mesh has a
// normal list, HRY_TANGENTS_STORED_NORMALS, and the area-weighted ones of HRY_RENDER_VERTEX_NORMALS otherwise; a mesh without
// texture coordinates ends with the library's refusal);
// --creases DEG (with or without OUTPUT, after those lines: "Creases: angle DEG vertices W groups G smooth S sharp H split V other O" --
// hry_creases_build at cos(DEG degrees) over a render build of the mesh and its edges build with geometry, and hry_creases_summary;
// it describes the mesh that is written: after --orient, the oriented one.  Nothing else about the output changes);
// --curvature (with or without OUTPUT, after those lines: "Curvature: vertices D interior I boundary B irregular N isolated Z
// degenerate G area A defect X turns K mean-integral M" -- hry_curvature_build over a render build of the mesh and its edges build,
// hry_curvature_summary and hry_curvature_totals; turns = defect / (2 pi), on a closed manifold mesh its Euler characteristic; it
// describes the mesh that is written, like --creases.  Nothing else about the output changes);
// --bvh (with or without OUTPUT, after those lines: "Bvh: triangles T leaves L dead Z distinct-codes C depth D" -- hry_bvh_build over a
// render build of the mesh, and hry_bvh_summary; it describes the mesh that is written, like --creases.  Nothing else about the
// output changes);
// --deviation OTHER (with or without OUTPUT, after those lines; OTHER is a .ply, .obj or .hry: "Deviation: forward points N answered
// A max M rms R" -- the position rows of a render build of the mesh that is written against the closest points of OTHER's triangles,
// hry_bvh_build over a render build of OTHER and hry_bvh_nearest; M the largest distance, R the square root of the mean squared
// distance over the A rows that were answered --, "Deviation: backward ..." -- OTHER's rows against the triangles of the mesh that is
// written --, and "Deviation: hausdorff H diagonal D relative H/D": H the larger M, D the diagonal of the scene box of the mesh that
// is written.  Nothing else about the output changes: harry in.ply out.hry -l1 -q10 && harry out.hry --deviation in.ply);
// --intersections (with or without OUTPUT, after those lines: "Intersections: triangles T candidates C tested N pairs P triangles-hit H"
// -- hry_bvh_build over a render build of the mesh, hry_intersections_build and hry_intersections_summary; it describes the mesh that
// is written, like --bvh.  Nothing else about the output changes: harry in.ply out.hry -l1 -q10 && harry out.hry --intersections
// against harry in.ply --intersections tells what the quantisation folded).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <thread>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/harry_amd.h"
#include "../host/env.hpp"
#include "../host/side_threads.hpp"

using hry::env_on;
using hry::trace_on;
using hry::SideThreads;

namespace {

const std::chrono::steady_clock::time_point g_start = std::chrono::steady_clock::now();   // (static initialisation: as early as this program can look)
long long since_start_ms() { return (long long)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - g_start).count(); }
struct QuantArg { int l, o, q; };
struct ToleranceArg { int l, o, metric; double value; };
struct BudgetArg { int l = -1, o = -1; long long bytes = -1; };   // bytes < 0: none
struct Args {
	std::string in, out, fmt, profile, deviation;   // profile empty: compat, unless --gpus / --shards ask for the sharded container
	std::vector<QuantArg> quant;
	std::vector<ToleranceArg> tolerance;
	BudgetArg budget;
	bool clearquant = false, ply_ascii = false, ply_packed = false, report = false, topology = false, shells = false, orient = false, orient_outward = false, tangents = false, creases = false, curvature = false, bvh = false, intersections = false;
	double crease_angle = 0.0;
	std::string crease_text;   // DEG as it was given
	int chunk = 0, device = 0, shards = 0, gpus = 0;
};

struct Opt { char s; const char *l; const char *descr; bool has_val; };
const Opt kOpts[] = {
	{ 'h', "help", "Print this dialogue.", false }, { 'f', "format", "Enforce output format", true }, { 'l', "list", "Select attribute list", true },
	{ 'a', "attr", "Select attribute", true }, { 'q', "quant", "Quantization bits", true }, { 'c', "clear-quant", "Clear all quantization first", false },
	{ 0, "ply-ascii", "PLY writer: Use ASCII format", false }, { 0, "ply-packed", "PLY writer: quantised values in their declared width", false }, { 0, "profile", "compat (reference stream, default) or chunked", true },
	{ 0, "chunk", "chunked: symbols per chunk", true }, { 0, "device", "GPU index (first one with --gpus)", true }, { 0, "gpus", "N device contexts, one worker thread each", true },
	{ 0, "shards", "chunked: code as N shards (default: one per context)", true }, { 0, "report", "Print the error of the quantization per component", false },
	{ 0, "max-error", "Quantization bits from the largest error allowed", true }, { 0, "max-error-rel", "... as a fraction of the extent", true },
	{ 0, "max-bytes", "Quantization bits from the largest .hry allowed", true },
	{ 0, "max-normal-angle", "Position bits from the largest turn of a face normal, degrees", true },
	{ 0, "topology", "Print edge counts and V - E + F (OUTPUT may be left out)", false },
	{ 0, "shells", "Print the connected shells, their counts, loops and genus (OUTPUT may be left out)", false },
	{ 0, "orient", "Wind the faces of every patch consistently, the smaller side turned (OUTPUT may be left out)", false },
	{ 0, "orient-outward", "... and closed patches so that they enclose a positive volume", false },
	{ 0, "tangents", "Print how many vertices get a tangent frame from positions, uv and normals (OUTPUT may be left out)", false },
	{ 0, "creases", "Print how many vertices and hard edges a crease angle of DEG degrees gives (OUTPUT may be left out)", true },
	{ 0, "curvature", "Print the vertex classes, the surface area, the total angle defect and the integral of the mean curvature (OUTPUT may be left out)", false },
	{ 0, "bvh", "Print the leaves, dead triangles, distinct codes and depth of a bounding-volume hierarchy over the triangles (OUTPUT may be left out)", false },
	{ 0, "deviation", "Print the surface deviation, one-sided both ways and symmetric, against the mesh in FILE (OUTPUT may be left out)", true },
	{ 0, "intersections", "Print the triangle pairs that pass through each other: an edge of one meets the other (OUTPUT may be left out)", false } };

void usage(const char *argv0)
{
	std::cout << "Harry mesh compressor" << std::endl << std::endl << "Usage: " << argv0 << " [OPTIONS] INPUT OUTPUT" << std::endl;
	for (const Opt &o : kOpts) {
		std::cout << "  ";
		if (o.s) std::cout << '-' << o.s << ", "; else std::cout << "    ";
		char buf[64];
		snprintf(buf, sizeof buf, "--%-13s%s", o.l, strlen(o.l) >= 13 ? " " : "");   // (a name that fills the column keeps a space behind it)
		std::cout << buf << o.descr << std::endl;
	}
}
[[noreturn]] void arg_error(const char *argv0, const std::string &what)
{
	usage(argv0);
	std::cout << std::endl;
	std::cerr << "Error: " << what << std::endl;
	std::exit(EXIT_FAILURE);
}
int to_int(const char *argv0, const std::string &v)
{
	char *end = nullptr;
	long x = strtol(v.c_str(), &end, 10);
	if (v.empty() || *end) arg_error(argv0, "Invalid cast");
	return (int)x;
}

double to_double(const char *argv0, const std::string &v)
{
	char *end = nullptr;
	const double x = strtod(v.c_str(), &end);
	if (v.empty() || *end) arg_error(argv0, "Invalid cast");
	return x;
}

Args parse(int argc, const char **argv)
{
	Args a;
	int cur_l = -1, cur_a = -1;   // (the reference leaves cur_l uninitialised, main.cc:48: -q without -l is reported instead)
	bool have_l = false;
	std::vector<std::string> pos;
	for (int i = 1; i < argc; ++i) {
		std::string s = argv[i];
		const Opt *o = nullptr;
		std::string val;
		bool inline_val = false;
		if (s.size() > 2 && s[0] == '-' && s[1] == '-') {
			std::string name = s.substr(2);
			size_t eq = name.find('=');
			if (eq != std::string::npos) { val = name.substr(eq + 1); name = name.substr(0, eq); inline_val = true; }
			for (const Opt &k : kOpts) if (name == k.l) o = &k;
			if (!o) arg_error(argv[0], "Invalid option " + name);
		} else if (s.size() >= 2 && s[0] == '-' && s[1] != '-') {
			for (const Opt &k : kOpts) if (k.s && k.s == s[1]) o = &k;
			if (!o) arg_error(argv[0], std::string("Invalid option ") + s[1]);
			if (s.size() > 2) { val = s.substr(2); inline_val = true; }
		} else { pos.push_back(s); continue; }
		if (o->has_val && !inline_val) {
			if (i + 1 >= argc) arg_error(argv[0], "Too few non-optional arguments");
			val = argv[++i];
		}
		const std::string n = o->l;
		if (n == "help") { usage(argv[0]); std::exit(EXIT_SUCCESS); }
		else if (n == "format") { if (val != "hry" && val != "ply" && val != "obj") arg_error(argv[0], "Invalid enum value"); a.fmt = val; }
		else if (n == "list") { cur_l = to_int(argv[0], val); have_l = true; }
		else if (n == "attr") cur_a = to_int(argv[0], val);
		else if (n == "quant") {
			if (!have_l) arg_error(argv[0], "-q needs a preceding -l (the reference reads an uninitialised list index here)");
			a.quant.push_back(QuantArg{ cur_l, cur_a, to_int(argv[0], val) });
			cur_a = -1;
		}
		else if (n == "clear-quant") a.clearquant = true;
		else if (n == "ply-ascii") a.ply_ascii = true;
		else if (n == "ply-packed") a.ply_packed = true;
		else if (n == "profile") { if (val != "compat" && val != "chunked") arg_error(argv[0], "Invalid enum value"); a.profile = val; }
		else if (n == "chunk") a.chunk = to_int(argv[0], val);
		else if (n == "device") a.device = to_int(argv[0], val);
		else if (n == "shards") a.shards = to_int(argv[0], val);
		else if (n == "gpus") a.gpus = to_int(argv[0], val);
		else if (n == "report") a.report = true;
		else if (n == "topology") a.topology = true;
		else if (n == "shells") a.shells = true;
		else if (n == "orient") a.orient = true;
		else if (n == "orient-outward") a.orient = a.orient_outward = true;
		else if (n == "tangents") a.tangents = true;
		else if (n == "curvature") a.curvature = true;
		else if (n == "bvh") a.bvh = true;
		else if (n == "intersections") a.intersections = true;
		else if (n == "deviation") { if (val.empty()) arg_error(argv[0], "Invalid file name"); a.deviation = val; }
		else if (n == "creases") {
			a.crease_angle = to_double(argv[0], val);
			if (std::isnan(a.crease_angle)) arg_error(argv[0], "Invalid angle");
			a.creases = true; a.crease_text = val;
		}
		else if (n == "max-error" || n == "max-error-rel") {
			if (!have_l) arg_error(argv[0], "--" + n + " needs a preceding -l");
			const double v = to_double(argv[0], val);
			if (!(v >= 0.0)) arg_error(argv[0], "Invalid tolerance");
			a.tolerance.push_back(ToleranceArg{ cur_l, cur_a, n == "max-error" ? HRY_TOL_MAX_ABS : HRY_TOL_MAX_REL, v });
			cur_a = -1;
		}
		else if (n == "max-normal-angle") {
			if (!have_l) arg_error(argv[0], "--max-normal-angle needs a preceding -l");
			if (cur_a != -1) arg_error(argv[0], "Invalid option: --max-normal-angle names the position components itself: no -a");
			const double v = to_double(argv[0], val);
			if (!(v >= 0.0) || v > 180.0) arg_error(argv[0], "Invalid tolerance");
			a.tolerance.push_back(ToleranceArg{ cur_l, -1, HRY_TOL_NORMAL_CHORD, v });
		}
		else if (n == "max-bytes") {
			if (!have_l) arg_error(argv[0], "--max-bytes needs a preceding -l");
			if (a.budget.bytes >= 0) arg_error(argv[0], "Invalid option: --max-bytes given twice");
			char *end = nullptr;
			const long long v = strtoll(val.c_str(), &end, 10);
			if (val.empty() || *end || v < 0) arg_error(argv[0], "Invalid budget");
			a.budget.l = cur_l; a.budget.o = cur_a; a.budget.bytes = v;
			cur_a = -1;
		}
	}
	if (a.budget.bytes >= 0) {
		const BudgetArg &b = a.budget;
		for (const QuantArg &q : a.quant)
			if (b.l == q.l && (b.o == q.o || b.o == -1 || q.o == -1))
				arg_error(argv[0], "Invalid option: list " + std::to_string(b.l) + " attr " + std::to_string(b.o == -1 ? q.o : b.o) + " has both -q and a budget");
		for (const ToleranceArg &t : a.tolerance)
			if (b.l == t.l && (b.o == t.o || b.o == -1 || t.o == -1))
				arg_error(argv[0], "Invalid option: list " + std::to_string(b.l) + " attr " + std::to_string(b.o == -1 ? t.o : b.o) + " has both a tolerance and a budget");
		if (a.gpus > 1 || a.shards > 1) arg_error(argv[0], "--max-bytes sweeps and encodes the whole mesh on one context: not with --gpus / --shards");
	}
	for (const ToleranceArg &t : a.tolerance)
		for (const QuantArg &q : a.quant)
			if (t.l == q.l && t.metric == HRY_TOL_NORMAL_CHORD ? q.o == -1 : t.l == q.l && (t.o == q.o || t.o == -1 || q.o == -1))   // (an angle against -q on a named component: when the position components are known)
				arg_error(argv[0], "Invalid option: list " + std::to_string(t.l) + " attr " + std::to_string(t.o == -1 ? q.o : t.o) + " has both -q and a tolerance");
	if (a.gpus < 0 || a.shards < 0 || a.gpus > 64) arg_error(argv[0], "Invalid number of contexts / shards");
	if ((a.gpus > 1 || a.shards > 1) && a.profile == "compat") arg_error(argv[0], "--gpus / --shards need --profile chunked: the reference's single stream does not shard");
	if (a.profile.empty()) a.profile = a.gpus > 1 || a.shards > 1 ? "chunked" : "compat";
	if (pos.size() < (a.topology || a.shells || a.orient || a.tangents || a.creases || a.curvature || a.bvh || !a.deviation.empty() || a.intersections ? 1u : 2u)) arg_error(argv[0], "Too few non-optional arguments");
	if (pos.size() > 2) arg_error(argv[0], "Too much non-optional arguments");
	a.in = pos[0];
	if (pos.size() > 1) a.out = pos[1];
	else if (a.budget.bytes >= 0) arg_error(argv[0], "--max-bytes is a budget for an OUTPUT");
	return a;
}

void ok(int rc) { if (rc != HRY_OK) throw std::runtime_error(hry_last_error()); }

std::string ext_of(const std::string &fn)
{
	std::string e = fn.size() >= 4 ? fn.substr(fn.size() - 4) : std::string();
	std::transform(e.begin(), e.end(), e.begin(), ::tolower);
	return e;
}

// the input file, mapped read-only (an empty file, or one that cannot be mapped, is read the plain way)
struct MappedFile {
	const uint8_t *p = nullptr;
	size_t n = 0;
	bool mapped = false;
	std::vector<uint8_t> copy;
	explicit MappedFile(const std::string &path)
	{
		const int fd = open(path.c_str(), O_RDONLY);
		if (fd < 0) throw std::runtime_error("cannot open " + path);
		struct stat sb;
		if (fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode) && sb.st_size > 0) {
			void *q = mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
			if (q != MAP_FAILED) { p = (const uint8_t*)q; n = (size_t)sb.st_size; mapped = true; (void)madvise(q, n, MADV_WILLNEED); }
		}
		if (!mapped) {
			uint8_t buf[1 << 16];
			for (;;) { const ssize_t k = read(fd, buf, sizeof buf); if (k <= 0) break; copy.insert(copy.end(), buf, buf + k); }
			p = copy.data(); n = copy.size();
		}
		close(fd);
	}
	~MappedFile() { if (mapped) munmap((void*)p, n); }
	MappedFile(const MappedFile&) = delete;
	size_t size() const { return n; }
	const uint8_t *data() const { return p; }
	uint8_t operator[](size_t i) const { return p[i]; }
};

// the output file; a large one is written by a few threads, each its own range (the copy into the page cache is the work:
// 1.7 GB of PLY took 0.4 s on one thread)
void write_file(const std::string &path, const uint8_t *p, size_t n)
{
	const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
	if (fd < 0) throw std::runtime_error("cannot write " + path);
	const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
	const unsigned nt = n >= ((size_t)64 << 20) ? std::min(8u, hw) : 1u;
	std::vector<char> failed(nt, 0);
	auto part = [&](unsigned t) {
		size_t at = n * t / nt;
		const size_t end = n * (t + 1) / nt;
		while (at < end) {
			const ssize_t k = pwrite(fd, p + at, std::min<size_t>(end - at, (size_t)64 << 20), (off_t)at);
			if (k <= 0) { failed[t] = 1; return; }
			at += (size_t)k;
		}
	};
	SideThreads th;
	for (unsigned t = 1; t < nt; ++t) th.spawn([&part, t] { part(t); });
	part(0);
	th.join();
	const bool bad = std::find(failed.begin(), failed.end(), (char)1) != failed.end();
	if (close(fd) != 0 || bad) throw std::runtime_error("cannot write " + path);
}

struct Handles {   // released on every path
	std::vector<hry_ctx*> cx;   // [0]: the context of every single-device step
	hry_mesh *mesh = nullptr, *before = nullptr;   // before: --report's clone of the mesh as it was read
	hry_distortion *dist = nullptr;
	hry_render *render = nullptr;   // --topology, --shells, --orient
	hry_edges *edges = nullptr;
	hry_shells *shells = nullptr;
	hry_orient *orient = nullptr;   // --orient, --orient-outward
	hry_tangents *tangents = nullptr;   // --tangents, over a render build of its own
	hry_creases *creases = nullptr;   // --creases, over a render build and an edges build with geometry of its own
	hry_curvature *curvature = nullptr;   // --curvature, over a render build and an edges build of its own
	hry_bvh *bvh = nullptr;   // --bvh, --deviation, --intersections, over a render build of its own
	hry_intersections *intersections = nullptr;   // --intersections, over that hierarchy
	hry_mesh *other = nullptr;   // --deviation: the mesh to compare with, its render build and the hierarchy over it
	hry_render *other_render = nullptr;
	hry_bvh *other_bvh = nullptr;
	hry_sweep *sweep = nullptr;
	hry_rate_sweep *rate = nullptr;
	hry_mesh *trial = nullptr;   // --max-bytes: the clone one width is encoded from
	std::vector<uint8_t*> bufs;
	// the render build of the mesh and the edges build behind it; what was built from them goes with them
	void build_adjacency()
	{
		ok(hry_render_build(cx[0], mesh, &render));
		ok(hry_edges_build(cx[0], mesh, render, 0, &edges));
	}
	void drop_adjacency()
	{
		if (intersections) hry_intersections_free(intersections);
		if (bvh) hry_bvh_free(bvh);
		if (curvature) hry_curvature_free(curvature);
		if (creases) hry_creases_free(creases);
		if (tangents) hry_tangents_free(tangents);
		if (orient) hry_orient_free(orient);
		if (shells) hry_shells_free(shells);
		if (edges) hry_edges_free(edges);
		if (render) hry_render_free(render);
		intersections = nullptr; bvh = nullptr; curvature = nullptr; creases = nullptr; tangents = nullptr; orient = nullptr; shells = nullptr; edges = nullptr; render = nullptr;
	}
	void drop_other()
	{
		if (other_bvh) hry_bvh_free(other_bvh);
		if (other_render) hry_render_free(other_render);
		if (other) hry_mesh_free(other);
		other_bvh = nullptr; other_render = nullptr; other = nullptr;
	}
	~Handles()
	{
		for (uint8_t *b : bufs) hry_free(b);
		drop_adjacency();
		drop_other();
		if (dist) hry_distortion_free(dist);
		if (sweep) hry_quant_sweep_free(sweep);
		if (rate) hry_rate_sweep_free(rate);
		if (trial) hry_mesh_free(trial);
		if (before) hry_mesh_free(before);
		if (mesh) hry_mesh_free(mesh);
		for (hry_ctx *c : cx) hry_ctx_destroy(c);
	}
};

// --max-bytes: the widest common width of the budget's components whose .hry (options o) is at most the budget; the container
// comes back in *out (released with h.bufs)
void encode_within_budget(Handles &h, const BudgetArg &b, const hry_opts &o, uint8_t **out, size_t *out_len)
{
	ok(hry_rate_sweep_build(h.cx[0], h.mesh, &h.rate));
	std::vector<int> comps;
	if (b.l < 0 || b.l >= hry_mesh_nlists(h.mesh)) throw std::runtime_error("Invalid list index");
	if (b.o == -1) { for (int c = 0; c < hry_list_ncomp(h.mesh, b.l); ++c) if (hry_rate_sweep_bits(h.rate, b.l, c) > 0) comps.push_back(c); }
	else comps.push_back(b.o);
	int qmax = 0;
	for (int c : comps) {
		const int q = hry_rate_sweep_bits(h.rate, b.l, c);
		if (q < 0) throw std::runtime_error(hry_last_error());
		if (q == 0) throw std::runtime_error("list " + std::to_string(b.l) + " attr " + std::to_string(c) + " cannot take a budget: " + hry_last_error());
		qmax = qmax ? std::min(qmax, q) : q;
	}
	if (comps.empty()) {
		std::string why = "it has no components";
		if (hry_list_ncomp(h.mesh, b.l) > 0 && hry_rate_sweep_bits(h.rate, b.l, 0) == 0) why = hry_last_error();
		throw std::runtime_error("list " + std::to_string(b.l) + " has no component that can take a budget: " + why);
	}
	auto estimate = [&](int bits) {
		double sum = 0;
		for (int c : comps) { double e = 0; ok(hry_rate_sweep_bytes(h.rate, b.l, c, bits, &e)); sum += e; }
		return sum;
	};
	std::map<int, std::pair<uint8_t*, size_t>> coded;   // width -> its container
	auto size_at = [&](int bits) {
		auto it = coded.find(bits);
		if (it != coded.end()) return it->second.second;
		if (!(h.trial = hry_mesh_clone(h.mesh))) throw std::runtime_error(hry_last_error());
		std::vector<hry_quant> q;
		for (int c : comps) q.push_back(hry_quant{ b.l, c, bits });
		ok(hry_requant(h.cx[0], h.trial, q.data(), q.size(), 0));
		uint8_t *p = nullptr;
		size_t n = 0;
		ok(hry_encode(h.cx[0], h.trial, &o, &p, &n));
		h.bufs.push_back(p);
		hry_mesh_free(h.trial); h.trial = nullptr;
		coded[bits] = std::make_pair(p, n);
		return n;
	};
	const size_t N = (size_t)b.bytes;
	auto start = [&](double fixed) {   // hry_rate_choose on what the budget leaves beside the fixed part; nothing fits: 1 bit
		int bits = 0;
		const double left = (double)N - fixed;
		if (left >= 0) ok(hry_rate_choose(h.rate, b.l, b.o, left, &bits, nullptr));
		return std::max(1, std::min(bits, qmax));
	};
	int bits = start(0.0);
	const size_t first = size_at(bits);
	bits = start((double)first - estimate(bits));
	while (size_at(bits) > N) {
		if (bits == 1) throw std::runtime_error("--max-bytes " + std::to_string(N) + ": the output is " + std::to_string(size_at(1)) + " bytes at 1 bit");
		--bits;
	}
	while (bits < qmax && size_at(bits + 1) <= N) ++bits;
	for (int c : comps) {
		double e = 0;
		ok(hry_rate_sweep_bytes(h.rate, b.l, c, bits, &e));
		char line[160];
		snprintf(line, sizeof line, "Budget: list %d attr %d bits %d estimated %.0f bytes", b.l, c, bits, e);
		std::cout << line << std::endl;
	}
	std::cout << "Budget: output " << coded[bits].second << " of " << N << " bytes after " << coded.size() << " encodes" << std::endl;
	*out = coded[bits].first; *out_len = coded[bits].second;
	hry_rate_sweep_free(h.rate); h.rate = nullptr;
}

// --deviation: one direction.  The position rows of r, a render build of m, against the triangles of `surface`
struct Deviation { uint64_t points = 0, answered = 0; double max = 0.0, rms = 0.0; };
Deviation deviation_of(hry_ctx *cx, const hry_mesh *m, const hry_render *r, const hry_bvh *surface)
{
	int pl = -1;
	for (int l = 0; l < hry_mesh_nlists(m) && pl < 0; ++l)
		if (hry_list_target(m, l) == 1 && hry_list_interp_ncomp(m, l, 0) >= 3) pl = l;
	if (pl < 0) throw std::runtime_error("deviation: no vertex list with three position components");
	const std::string name = "list" + std::to_string(pl);
	uint64_t rows = 0;
	int width = 0, type = 0;
	ok(hry_render_get(r, name.c_str(), nullptr, &rows, &width, &type));
	Deviation d;
	d.points = rows;
	if (!rows) return d;
	std::vector<float> values((size_t)rows * (size_t)width);
	ok(hry_render_copy(cx, r, name.c_str(), values.data(), 0));
	std::vector<uint32_t> tri(rows);
	std::vector<double> d2(rows);
	uint64_t stat[3] = {};
	ok(hry_bvh_nearest(cx, surface, rows, values.data() + hry_list_interp_offset(m, pl, 0), (uint64_t)width * 4, HUGE_VAL, HRY_NEAREST_HOST, tri.data(), d2.data(), nullptr,
	                   nullptr, stat, nullptr));
	double sum = 0.0, largest = 0.0;
	for (uint64_t i = 0; i < rows; ++i) if (tri[i] != HRY_NO_ELEMENT) sum += d2[i];   // in index order
	memcpy(&largest, &stat[2], 8);
	d.answered = stat[0];
	if (d.answered) { d.max = std::sqrt(largest); d.rms = std::sqrt(sum / (double)d.answered); }
	return d;
}

int run(const Args &args)
{
	typedef std::chrono::high_resolution_clock Clock;
	auto ms = [](Clock::time_point a, Clock::time_point b) { return (long long)std::chrono::duration_cast<std::chrono::milliseconds>(b - a).count(); };
	Handles h;
	const int n_ctx = std::max(1, args.gpus);
	const int n_dev = hry_device_count();
	// The device contexts come up (runtime start, code objects: a few hundred milliseconds) while the input is read and parsed on the
	// host; whoever needs one first waits for them.
	SideThreads ctx_thread;
	ctx_thread.spawn([&] {
		for (int i = 0; i < n_ctx; ++i) {
			hry_ctx *c = nullptr;
			if (hry_ctx_create(n_dev > 0 && i > 0 ? (args.device + i) % n_dev : args.device, &c) != HRY_OK) throw std::runtime_error(hry_last_error());
			h.cx.push_back(c);
		}
	});
	const bool trace = trace_on();
	bool ctx_ready = false;
	auto contexts = [&] {
		if (!ctx_ready) { ctx_ready = true; ctx_thread.join(); if (trace) std::cerr << "[harry] " << since_start_ms() << " ms  contexts ready" << std::endl; }
		ctx_thread.rethrow();
	};
	if (trace) std::cerr << "[harry] " << since_start_ms() << " ms  arguments parsed" << std::endl;
	const bool sharded = n_ctx > 1 || args.shards > 1;

	std::cout << "Reading input..." << std::endl;
	Clock::time_point t0 = Clock::now();
	// the file is mapped, not copied: the parser's threads fault its pages in as they go (a 1.6 GB PLY read into a zero-filled
	// vector first was 0.6 s before the first byte was looked at)
	MappedFile in(args.in);
	if (in.size() >= 4 && in[0] == 0xfa && in[1] == 0xff && in[2] == 0xaf && in[3] == 0xaf) {
		contexts();
		if (n_ctx > 1) {
			hry_shard_timing st{};
			ok(hry_decode_sharded(h.cx.data(), n_ctx, in.data(), in.size(), nullptr, &h.mesh, &st));
			std::cout << "  " << st.n_segments << " segment(s) on " << st.n_contexts << " context(s), " << std::min(n_ctx, std::max(1, n_dev)) << " device(s): decode "
			          << (long long)st.encode_ms << " ms, placement " << (long long)st.extract_ms << " ms" << std::endl;
		} else ok(hry_decode(h.cx[0], in.data(), in.size(), nullptr, &h.mesh));
	}
	else if (in.size() >= 3 && in[0] == 'p' && in[1] == 'l' && in[2] == 'y') ok(hry_mesh_from_ply(in.data(), in.size(), &h.mesh));
	else if (ext_of(args.in) == ".obj") {
		// material libraries are looked up in the input path up to its last separator -- the whole path when there is none, as
		// the reference computes it (formats/unified_reader.h:56)
		const std::string dir = args.in.substr(0, args.in.find_last_of("/\\"));
		ok(hry_mesh_from_obj(in.data(), in.size(), dir.c_str(), &h.mesh));
		std::cout << "Used face regions: " << hry_mesh_nregions(h.mesh, 0) << std::endl;     // formats/obj/reader.rl:296-297
		std::cout << "Used vertex regions: " << hry_mesh_nregions(h.mesh, 1) << std::endl;
	}
	else throw std::runtime_error("Not a mesh file");
	if (trace) std::cerr << "[harry] " << since_start_ms() << " ms  input parsed" << std::endl;
	contexts();
	Clock::time_point t1 = Clock::now();
	std::cout << "Reading input took " << ms(t0, t1) << " ms." << std::endl;

	std::string type = args.fmt;
	if (type.empty()) {
		const std::string e = ext_of(args.out);
		type = e == ".hry" ? "hry" : e == ".ply" ? "ply" : e == ".obj" ? "obj" : "";
	}
	std::vector<hry_quant> q;
	for (const QuantArg &x : args.quant) q.push_back(hry_quant{ x.l, x.o, x.q });
	// a sharded .hry quantises shard by shard on the workers (the bounds of the whole mesh are combined from the shards'): the
	// whole mesh never sits on one device
	const bool quant_in_encode = sharded && type == "hry";
	if (!args.tolerance.empty() && quant_in_encode) throw std::runtime_error("--max-error / --max-normal-angle sweep the whole mesh on one context: not with --gpus / --shards");
	const bool budget = args.budget.bytes >= 0;
	if (budget && quant_in_encode) throw std::runtime_error("--max-bytes sweeps and encodes the whole mesh on one context: not with --gpus / --shards");
	if (budget && type != "hry") throw std::runtime_error("--max-bytes is a budget for a .hry output");
	const bool quant_phase = (!q.empty() || !args.tolerance.empty() || args.clearquant) && !quant_in_encode;
	if (quant_phase) {
		std::cout << "Quantization..." << std::endl;
		if (args.report && !(h.before = hry_mesh_clone(h.mesh))) throw std::runtime_error(hry_last_error());
		bool cleared = false;
		if (!args.tolerance.empty()) {
			// the widths the tolerances need, from one sweep of the mesh as the quantisation finds it.  With -c that is the cleared mesh:
			// it is cleared here, on its own, and every width -- chosen or explicit -- is then applied to the cleared values, so what is
			// applied is what was swept (a direct q -> q' rescale of a quantised source truncates: up to a whole step, not the table's)
			if (args.clearquant) { ok(hry_requant(h.cx[0], h.mesh, nullptr, 0, 1)); cleared = true; }
			bool angles = false;
			for (const ToleranceArg &t : args.tolerance) angles = angles || t.metric == HRY_TOL_NORMAL_CHORD;
			ok(hry_quant_sweep_build_ex(h.cx[0], h.mesh, angles ? HRY_SWEEP_NORMALS : 0u, &h.sweep));
			std::vector<hry_tolerance> tol, tol_angle;
			// a tolerance without -a names every component of its list, as -q does: one that cannot take it (quantised already, a
			// constant integer) is an error with its reason, where the library's comp -1 would leave it out
			for (const ToleranceArg &t : args.tolerance) {
				if (t.metric == HRY_TOL_NORMAL_CHORD) {   // degrees -> the chord the table is in; the library names the three components
					double chord = 0.0;
					ok(hry_angle_chord(t.value * (3.14159265358979323846 / 180.0), &chord));
					tol.push_back(hry_tolerance{ t.l, -1, t.metric, 0, chord });
					tol_angle.push_back(tol.back());
					continue;
				}
				const bool all = t.o == -1 && t.l >= 0 && t.l < hry_mesh_nlists(h.mesh);
				if (!all) tol.push_back(hry_tolerance{ t.l, t.o, t.metric, 0, t.value });
				else for (int c = 0; c < hry_list_ncomp(h.mesh, t.l); ++c) tol.push_back(hry_tolerance{ t.l, c, t.metric, 0, t.value });
			}
			size_t n = 0;
			std::vector<hry_quant> chosen((size_t)16 * 32);
			ok(hry_quant_choose(h.sweep, tol.data(), tol.size(), chosen.data(), chosen.size(), &n));
			size_t n_angle = 0;   // the components an angle names: the position components
			std::vector<hry_quant> by_angle((size_t)16 * 32);
			if (!tol_angle.empty()) ok(hry_quant_choose(h.sweep, tol_angle.data(), tol_angle.size(), by_angle.data(), by_angle.size(), &n_angle));
			for (size_t i = 0; i < n; ++i) {
				bool angle = false;
				for (size_t k = 0; k < n_angle; ++k) angle = angle || (by_angle[k].list == chosen[i].list && by_angle[k].comp == chosen[i].comp);
				char line[160];
				if (angle) {
					for (const hry_quant &x : q)
						if (x.list == chosen[i].list && (x.comp == -1 || x.comp == chosen[i].comp))
							throw std::runtime_error("list " + std::to_string(x.list) + " attr " + std::to_string(chosen[i].comp) + " has both -q and --max-normal-angle");
					hry_normal_error ne{};
					double rad = 0.0;
					if (chosen[i].bits) { ok(hry_quant_sweep_normals(h.sweep, chosen[i].bits, &ne)); ok(hry_chord_angle(ne.max_chord, &rad)); }
					snprintf(line, sizeof line, "Chosen: list %d attr %d bits %d max-angle %.9g deg", chosen[i].list, chosen[i].comp, chosen[i].bits, rad * (180.0 / 3.14159265358979323846));
				} else {
					hry_comp_error e{};
					if (chosen[i].bits) ok(hry_quant_sweep_component(h.sweep, chosen[i].list, chosen[i].comp, chosen[i].bits, &e));
					snprintf(line, sizeof line, "Chosen: list %d attr %d bits %d max %.9g", chosen[i].list, chosen[i].comp, chosen[i].bits, e.max_abs);
				}
				std::cout << line << std::endl;
			}
			for (size_t i = 0; i < n; ++i) q.push_back(chosen[i]);
			hry_quant_sweep_free(h.sweep); h.sweep = nullptr;
		}
		ok(hry_requant(h.cx[0], h.mesh, q.data(), q.size(), args.clearquant && !cleared ? 1 : 0));   // validation and texts of main.cc:74-91 inside
	}
	Clock::time_point t2 = Clock::now();
	if (quant_phase) std::cout << "Quantization took " << ms(t1, t2) << " ms." << std::endl;
	if (h.before) {
		ok(hry_distortion_build(h.cx[0], h.before, h.mesh, nullptr, HRY_DISTORTION_NORMALS, &h.dist));
		for (int l = 0; l < hry_mesh_nlists(h.mesh); ++l)
			for (int c = 0; c < hry_list_ncomp(h.mesh, l); ++c) {
				hry_comp_error e;
				if (hry_distortion_component(h.dist, l, c, &e) != HRY_OK) continue;   // (a list that is not compared)
				char line[256];
				snprintf(line, sizeof line, "Distortion: list %d attr %d bits %d max %.9g rms %.9g changed %llu", l, c, hry_list_quant(h.mesh, l, c), e.max_abs,
				         e.compared ? std::sqrt(e.sum_sq / (double)e.compared) : 0.0, (unsigned long long)e.changed);
				std::cout << line << std::endl;
			}
		hry_normal_error ne{};
		if (hry_distortion_normals(h.dist, &ne) == HRY_OK && ne.list >= 0) {   // (a mesh with positions and faces)
			double mx = 0.0, rms = 0.0;
			ok(hry_chord_angle(ne.max_chord, &mx));
			if (ne.compared) ok(hry_chord_angle(std::sqrt(ne.sum_sq_chord / (double)ne.compared), &rms));
			const double deg = 180.0 / 3.14159265358979323846;
			char line[256];
			snprintf(line, sizeof line, "Normals: faces %llu max-angle %.9g deg rms %.9g deg collapsed %llu degenerate %llu",
			         (unsigned long long)(ne.compared + ne.skipped + ne.nonfinite + ne.degenerate + ne.collapsed), mx * deg, rms * deg,
			         (unsigned long long)ne.collapsed, (unsigned long long)ne.degenerate);
			std::cout << line << std::endl;
		}
		hry_distortion_free(h.dist); h.dist = nullptr;
		hry_mesh_free(h.before); h.before = nullptr;
		t2 = Clock::now();   // (the report is no part of the writing phase)
	}

	if (args.topology) {
		h.build_adjacency();
		uint64_t s[4];
		ok(hry_edges_summary(h.edges, s));
		const long long V = hry_mesh_nv(h.mesh), F = hry_mesh_nf(h.mesh);
		std::cout << "Topology: vertices " << V << " faces " << F << " triangles " << hry_mesh_ntri(h.mesh) << " edges " << s[0] << " boundary " << s[1] << " manifold " << s[2]
		          << " nonmanifold " << s[3] << " euler " << V - (long long)s[0] + F << std::endl;
		h.drop_adjacency();
		t2 = Clock::now();   // (no part of the writing phase)
	}
	if (args.shells) {
		h.build_adjacency();
		ok(hry_shells_build(h.cx[0], h.mesh, h.render, h.edges, 0, &h.shells));
		uint64_t s[6];
		ok(hry_shells_summary(h.shells, s));
		std::cout << "Shells: shells " << s[0] << " closed " << s[1] << " nonmanifold " << s[2] << " misoriented " << s[3] << " loops " << s[4] << " largest " << s[5] << std::endl;
		const uint64_t shown = std::min<uint64_t>(s[0], 16);
		std::vector<uint32_t> c(8 * s[0]);   // (the whole buffer comes down: the handle copies buffers, not rows)
		if (s[0]) ok(hry_shells_copy(h.cx[0], h.shells, "shell_counts", c.data(), 0));
		for (uint64_t i = 0; i < shown; ++i) {
			const uint32_t *k = &c[8 * i];   // triangles, faces, vertices, edges, boundary, nonmanifold, misoriented, loops
			const long long euler = (long long)k[2] - (long long)k[3] + (long long)k[0];
			std::cout << "Shell: " << i << " triangles " << k[0] << " vertices " << k[2] << " edges " << k[3] << " boundary " << k[4] << " loops " << k[7] << " euler " << euler << " genus ";
			if (k[5] || k[6]) std::cout << "-";
			else std::cout << (2 - euler - (long long)k[7]) / 2;
			std::cout << std::endl;
		}
		h.drop_adjacency();
		t2 = Clock::now();   // (no part of the writing phase)
	}
	if (args.orient) {
		h.build_adjacency();
		ok(hry_orient_build(h.cx[0], h.mesh, h.render, h.edges, HRY_ORIENT_MAJORITY | (args.orient_outward ? HRY_ORIENT_OUTWARD : 0u), &h.orient));
		uint64_t s[6];
		ok(hry_orient_summary(h.orient, s));
		std::cout << "Orientation: patches " << s[0] << " orientable " << s[1] << " flipped " << s[2] << " inverted " << s[3] << " against " << s[4] << " remaining " << s[5] << std::endl;
		if (s[2] && !args.out.empty()) {   // (nothing flipped: the mesh is written as it is)
			std::vector<uint32_t> flip(hry_mesh_nf(h.mesh));
			ok(hry_orient_copy(h.cx[0], h.orient, "face_flip", flip.data(), 0));
			hry_mesh *turned = nullptr;
			ok(hry_mesh_flip_faces(h.mesh, flip.data(), &turned));
			hry_mesh_free(h.mesh); h.mesh = turned;
		}
		h.drop_adjacency();
		t2 = Clock::now();   // (no part of the writing phase)
	}
	if (args.tangents) {
		bool stored = false;   // a normal list: a vertex or corner list with three NORMAL components
		for (int l = 0; l < hry_mesh_nlists(h.mesh); ++l) stored |= (hry_list_target(h.mesh, l) == 1 || hry_list_target(h.mesh, l) == 2) && hry_list_interp_ncomp(h.mesh, l, 1) >= 3;
		ok(hry_render_build_ex(h.cx[0], h.mesh, stored ? 0u : HRY_RENDER_VERTEX_NORMALS, &h.render));
		ok(hry_tangents_build(h.cx[0], h.mesh, h.render, stored ? HRY_TANGENTS_STORED_NORMALS : 0u, &h.tangents));
		uint64_t s[6];
		ok(hry_tangents_summary(h.tangents, s));
		std::cout << "Tangents: vertices " << hry_render_nverts(h.render) << " framed " << s[0] << " unframed " << s[1] << " mirrored " << s[2] << " mixed " << s[3] << " degenerate " << s[4] << std::endl;
		h.drop_adjacency();
		t2 = Clock::now();   // (no part of the writing phase)
	}
	if (args.creases) {
		ok(hry_render_build(h.cx[0], h.mesh, &h.render));
		ok(hry_edges_build(h.cx[0], h.mesh, h.render, HRY_EDGES_GEOMETRY, &h.edges));
		ok(hry_creases_build(h.cx[0], h.mesh, h.render, h.edges, std::cos(args.crease_angle * (3.14159265358979323846 / 180.0)), 0u, &h.creases));
		uint64_t s[6];
		ok(hry_creases_summary(h.creases, s));
		std::cout << "Creases: angle " << args.crease_text << " vertices " << s[0] << " groups " << s[1] << " smooth " << s[2] << " sharp " << s[3] << " split " << s[4] << " other " << s[5] << std::endl;
		h.drop_adjacency();
		t2 = Clock::now();   // (no part of the writing phase)
	}
	if (args.curvature) {
		h.build_adjacency();
		ok(hry_curvature_build(h.cx[0], h.mesh, h.render, h.edges, 0u, &h.curvature));
		uint64_t s[6];
		double t[3];
		ok(hry_curvature_summary(h.curvature, s));
		ok(hry_curvature_totals(h.curvature, t));
		char line[512];
		snprintf(line, sizeof line, "Curvature: vertices %llu interior %llu boundary %llu irregular %llu isolated %llu degenerate %llu area %.9g defect %.9g turns %.9g mean-integral %.9g",
		         (unsigned long long)s[0], (unsigned long long)s[1], (unsigned long long)s[2], (unsigned long long)s[3], (unsigned long long)s[4], (unsigned long long)s[5], t[0], t[1],
		         t[1] / (2.0 * 3.14159265358979323846), t[2]);
		std::cout << line << std::endl;
		h.drop_adjacency();
		t2 = Clock::now();   // (no part of the writing phase)
	}
	// --bvh, --deviation and --intersections read one hierarchy over one render build of the mesh: built by the first of them
	// that runs, dropped behind the last
	const auto hierarchy = [&] {
		if (h.bvh) return;
		ok(hry_render_build(h.cx[0], h.mesh, &h.render));
		ok(hry_bvh_build(h.cx[0], h.mesh, h.render, 0u, &h.bvh));
	};
	if (args.bvh) {
		hierarchy();
		uint64_t s[6];
		ok(hry_bvh_summary(h.bvh, s));
		std::cout << "Bvh: triangles " << s[0] << " leaves " << s[1] << " dead " << s[2] << " distinct-codes " << s[3] << " depth " << s[4] << std::endl;
	}
	if (!args.deviation.empty()) {
		MappedFile of(args.deviation);
		if (of.size() >= 4 && of[0] == 0xfa && of[1] == 0xff && of[2] == 0xaf && of[3] == 0xaf) ok(hry_decode(h.cx[0], of.data(), of.size(), nullptr, &h.other));
		else if (of.size() >= 3 && of[0] == 'p' && of[1] == 'l' && of[2] == 'y') ok(hry_mesh_from_ply(of.data(), of.size(), &h.other));
		else if (ext_of(args.deviation) == ".obj") ok(hry_mesh_from_obj(of.data(), of.size(), args.deviation.substr(0, args.deviation.find_last_of("/\\")).c_str(), &h.other));
		else throw std::runtime_error("Not a mesh file");
		hierarchy();
		ok(hry_render_build(h.cx[0], h.other, &h.other_render));
		ok(hry_bvh_build(h.cx[0], h.other, h.other_render, 0u, &h.other_bvh));
		const Deviation side[2] = { deviation_of(h.cx[0], h.mesh, h.render, h.other_bvh), deviation_of(h.cx[0], h.other, h.other_render, h.bvh) };
		for (int k = 0; k < 2; ++k) {
			char line[256];
			snprintf(line, sizeof line, "Deviation: %s points %llu answered %llu max %.9g rms %.9g", k ? "backward" : "forward", (unsigned long long)side[k].points,
			         (unsigned long long)side[k].answered, side[k].max, side[k].rms);
			std::cout << line << std::endl;
		}
		float box[6];
		ok(hry_bvh_copy(h.cx[0], h.bvh, "scene_box", box, 0));
		const double dx = (double)box[3] - (double)box[0], dy = (double)box[4] - (double)box[1], dz = (double)box[5] - (double)box[2];
		const double hausdorff = std::max(side[0].max, side[1].max), diagonal = hry_bvh_count(h.bvh) ? std::sqrt((dx * dx + dy * dy) + dz * dz) : 0.0;
		char line[256];
		snprintf(line, sizeof line, "Deviation: hausdorff %.9g diagonal %.9g relative %.9g", hausdorff, diagonal, diagonal > 0.0 ? hausdorff / diagonal : 0.0);
		std::cout << line << std::endl;
		h.drop_other();
	}
	if (args.intersections) {
		hierarchy();
		ok(hry_intersections_build(h.cx[0], h.bvh, 0u, &h.intersections));
		uint64_t s[6];
		ok(hry_intersections_summary(h.intersections, s));
		std::cout << "Intersections: triangles " << s[0] << " candidates " << s[1] << " tested " << s[2] << " pairs " << s[3] << " triangles-hit " << s[4] << std::endl;
	}
	if (h.bvh) {
		h.drop_adjacency();
		t2 = Clock::now();   // (no part of the writing phase)
	}
	if ((args.topology || args.shells || args.orient || args.tangents || args.creases || args.curvature || args.bvh || !args.deviation.empty() || args.intersections) && args.out.empty()) {
		if (!env_on("HRY_ORDERLY_EXIT")) { std::cout.flush(); std::cerr.flush(); fflush(nullptr); _exit(EXIT_SUCCESS); }
		return EXIT_SUCCESS;
	}

	std::cout << "Writing output..." << std::endl;
	if (type.empty()) throw std::runtime_error("Unknown file extension");
	uint8_t *out = nullptr;
	size_t out_len = 0;
	if (type == "hry") {
		hry_opts o{};
		o.profile = args.profile == "chunked" ? HRY_PROFILE_CHUNKED : HRY_PROFILE_COMPAT;
		o.chunk_syms = args.chunk;
		if (quant_in_encode) {
			if (o.profile != HRY_PROFILE_CHUNKED) throw std::runtime_error("--gpus / --shards need --profile chunked");
			o.shard_count = args.shards;
			hry_shard_timing st{};
			ok(hry_encode_sharded(h.cx.data(), n_ctx, h.mesh, q.data(), q.size(), args.clearquant ? 1 : 0, &o, &out, &out_len, &st));
			std::cout << "  " << st.n_shards << " shard(s) of " << st.n_components << " component(s) on " << st.n_contexts << " context(s), " << std::min(n_ctx, std::max(1, n_dev))
			          << " device(s): plan " << (long long)st.plan_ms << " ms, extract " << (long long)st.extract_ms << " ms, bounds " << (long long)(st.bounds_ms + st.combine_ms)
			          << " ms, quantization " << (long long)st.quant_ms << " ms, encode " << (long long)st.encode_ms << " ms, merge " << (long long)st.merge_ms << " ms" << std::endl;
		} else if (budget) encode_within_budget(h, args.budget, o, &out, &out_len);
		else ok(hry_encode(h.cx[0], h.mesh, &o, &out, &out_len));
	} else if (type == "ply") ok(hry_mesh_to_ply(h.mesh, (args.ply_ascii ? HRY_PLY_ASCII : 0) | (args.ply_packed ? HRY_PLY_PACKED : 0), &out, &out_len));
	else ok(hry_mesh_to_obj(h.mesh, 0, &out, &out_len));
	if (!budget) h.bufs.push_back(out);   // (a budget's containers are in h.bufs already)
	write_file(args.out, out, out_len);
	Clock::time_point t3 = Clock::now();
	std::cout << "Writing output took " << ms(t2, t3) << " ms." << std::endl;
	std::cout << "Total compression time: " << ms(t0, t3) << " ms" << std::endl;
	std::cout << "Total input size: " << in.size() << " Bytes" << std::endl;
	std::cout << "Total output size: " << out_len << " Bytes" << std::endl;
	if (trace) std::cerr << "[harry] " << since_start_ms() << " ms  done" << std::endl;
	// Everything is written.  Gigabytes of host arrays, the device contexts and the runtime itself would now be taken apart piece by
	// piece (0.5 s for the configs[3] mesh) only for the process to end: it ends here instead, and the system takes it all back at
	// once.  HRY_ORDERLY_EXIT=1 keeps the long way (leak checkers, tests of the destructors).
	if (!env_on("HRY_ORDERLY_EXIT")) { std::cout.flush(); std::cerr.flush(); fflush(nullptr); _exit(EXIT_SUCCESS); }
	return EXIT_SUCCESS;
}

}   // namespace

int main(int argc, const char **argv)
{
	const Args args = parse(argc, argv);
	try {
		const int rc = run(args);
		if (trace_on()) std::cerr << "[harry] " << since_start_ms() << " ms  handles released" << std::endl;
		return rc;
	} catch (const std::exception &e) {
		// what the reference's uncaught exception prints through std::terminate, and the status abort() leaves
		std::cout.flush();
		std::cerr << "terminate called after throwing an instance of 'std::runtime_error'" << std::endl << "  what():  " << e.what() << std::endl;
		return 134;
	}
}
