"""Designed meshes for the decoder's reconstruction: the candidate table (k_candidates_ids) and the chains (k_chain_records,
k_unpredict3, k_unpredict3_range, k_unpredict2<T>).  What each mesh demands is counted by tests/chain_ref.py from the CPU oracle's
vertex trace and is a CONDITION of the case (tests/test_chain_cpu.py, no GPU): at least MIN_VERTICES vertices of every vertex class
the case is there for and at least MIN_TILES tiles of every tile class, at every team size the case runs at.

Run as a program (tests/test_gpu_chain.py: one process per setting of HRY_CHAIN_WAVES, which is read once per process) every case
goes through the GPU, every check exact against the oracle:
  1. quantised by the product and by the oracle; the reference-format stream and the chunked container equal the oracle's;
  2. both decoded in one launch (HRY_NO_PIPELINE=1) and -- the container of a case that qualifies -- pipelined in forced slices;
     every decode equals the oracle's decode of the reference-format stream;
  3. the stages "ncand", "cand" and "cand_over" against the oracle's trace: counts (0xff above eight), compact rows, overflow rows;
  4. the stage "chain_plan": the kernel, the ring and the team size the case was meant for did run.
One line per case, then "all equal"; the first mismatch ends the run, named by case, class and vertex.
    HRY_CHAIN_WAVES=4 python tests/tools/chain_cases.py [case ...]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from harry_amd import meshgen as mg
from oracle import oracle_py as op   # checker only
from tests import chain_ref as cr

MIN_VERTICES, MIN_TILES = 32, 4
TEAMS = (1, 4, 8, 12)
SLICES = ((64, 64), (1000, 4096), (3000, 16448))   # (faces between two publications, vertices of a slice); 16 448: a tile more than the ring
K2, K3, K3_RANGE = 2, 3, 4
F32, U32, U16, U8 = 0, 4, 6, 8                     # storage types (mixing::Type)
RING_FULL, RING_HALF = 32 * 1024, 16 * 1024
ENV = ("HRY_NO_PIPELINE", "HRY_PIPELINE_MIN_VERTICES", "HRY_PIPELINE_FACES", "HRY_PIPELINE_SLICE", "HRY_PIPELINE_LAST_PIECE")


# ---- the meshes
def _hubs():
    # a torus of triangles, quads and pentagons (the (a, b, b) offer of a polygon of degree above 4; 3 - 6 candidates where the walk
    # closes) with discs around new vertices of 3 .. 14 faces: every source of theirs belongs to the torus, an earlier component
    return mg.with_shared_discs(mg.torus(40, 40, polys="mixed"), list(range(3, 15)) * 6)


def _shared():
    # the same discs on a triangle torus, and the slivers of non-manifold edges and vertices (tiny components that share work lists)
    return mg.with_nonmanifold(mg.with_shared_discs(mg.torus(60, 60), list(range(3, 15)) * 6), 60, 40)


def _ribbon():
    return mg.ribbon(8400, 3)   # 25 200 vertices, one component: a third of them reads more than 8 192 back, 486 more than 16 320 (68 by less than a tile)


def _ribbon_and_many():
    # 350 components of 64 vertices beside a ribbon that reads 4 096 and more back: more than 1 024 chains, rings of half the size
    return mg.concat([mg.ribbon(3000, 3)] + [mg.torus(8, 8, seed=20 + c, center=(3.0 * (c % 32), 3.0 + 3.0 * (c // 32), 0.0)) for c in range(350)])


def _heads():
    # a long regular torus (tiles without heads, stretches of 17 and more two-candidate vertices, gaps past 64 x 11 for the team of
    # twelve) with 16 small holes whose borders the walk goes round: tiles of 1, 2 - 8, 9 - 12 and more heads at every team size.
    # One component of triangles: the pipelined decode takes it, and with it the team of twelve
    return mg.with_holes(mg.torus(264, 264), 16)


def _pieces():
    # narrow strips and small irregular pieces: nearly every source is recent, the tiles are cut into runs as they come
    parts = [mg.grid(40, 5, seed=30 + c) for c in range(6)] + [mg.grid(9, 9, seed=40 + c, quads=True) for c in range(6)]
    parts += [mg.torus(12, 14, seed=50 + c, polys="mixed", center=(3.0 * c, 4.0, 0.0)) for c in range(6)] + [mg.icosphere(2, seed=60 + c, extra_props=False) for c in range(4)]
    return mg.concat(parts)


def _noisy():
    # heavy noise: parallelograms past both ends of the range and residual codes in their far form at every width; z cut off at a
    # floor and a ceiling: stretches of the smallest and the largest value (predictions of 0: raw codes; of the top: no room above)
    m = mg.torus(100, 100, sigma=0.08)
    v = m.verts.copy()
    v["z"] = np.clip(v["z"], np.float32(-0.2), np.float32(0.2))
    return mg.Mesh(v, m.degrees, m.indices)


def _ties():
    return mg.snapped(mg.torus(64, 64, sigma=0.0), 1.0 / 32)


_V_COUNTS = ("cand0", "cand1", "cand2", "cand3_8", "cand9p")
_V_NOISE = ("clamp0", "clamptop", "far_code", "raw", "near", "chained", "constant")
_T_HEADS = ("heads0", "heads1", "heads2_8", "heads9_12", "heads13p", "rowheads9p", "late", "dense", "stretch17p")
_T_NOISE = ("run_leaves0", "run_leaves1", "run_leaves2p")

# name, mesh, q (0: lossless), kernel, storage type, ring bytes, pipelined decode qualifies, vertex classes, tile classes
CASES = (
    ("hubs_q8", _hubs, 8, K3, U8, cr.RING3, False, _V_COUNTS + ("cross", "cross_many"), ()),
    ("hubs_q12", _hubs, 12, K3, U16, 2 * cr.RING3, False, _V_COUNTS + ("cross", "cross_many"), ()),
    ("hubs_f32", _hubs, 0, K2, F32, RING_FULL, False, _V_COUNTS + ("cross", "cross_many"), ()),
    ("long_rows_q12", _ribbon, 12, K3, U16, 2 * cr.RING3, True, (f"older{cr.RING3_NEAR}", "ring_edge"), ("heads0", "dense", "stretch17p")),
    ("long_rows_f32", _ribbon, 0, K2, F32, RING_FULL, False, ("older8192",), ()),
    ("long_rows_f32_half", _ribbon_and_many, 0, K2, F32, RING_HALF, False, ("older4096",), ()),
    ("shared_q12", _shared, 12, K3, U16, 2 * cr.RING3, False, ("cross", "cross_many", "cand3_8", "cand9p"), ()),
    ("heads_q12", _heads, 12, K3, U16, 2 * cr.RING3, True, ("chained", "constant"), _T_HEADS),
    ("pieces_q12", _pieces, 12, K3, U16, 2 * cr.RING3, False, _V_COUNTS[:4], ("heads13p", "rowheads9p", "late", "dense")),
    ("noisy_q1", _noisy, 1, K3, U8, cr.RING3, True, ("clamp0", "clamptop", "raw", "chained", "constant"), _T_NOISE),
    ("noisy_q2", _noisy, 2, K3, U8, cr.RING3, True, _V_NOISE, _T_NOISE),
    ("noisy_q8", _noisy, 8, K3, U8, cr.RING3, True, _V_NOISE, _T_NOISE),
    ("noisy_q9", _noisy, 9, K3, U16, 2 * cr.RING3, True, _V_NOISE, _T_NOISE),
    ("noisy_q16", _noisy, 16, K3, U16, 2 * cr.RING3, True, _V_NOISE, _T_NOISE),
    ("wide_q17", _noisy, 17, K2, U32, RING_FULL, False, ("clamp0", "clamptop", "far_code", "raw", "near"), ()),
    ("wide_q24", _noisy, 24, K2, U32, RING_FULL, False, ("clamp0", "clamptop", "far_code", "raw", "near"), ()),
    ("ties_f32", _ties, 0, K2, F32, RING_FULL, False, ("float_tie",), ()),
)


class Built:
    """a case's mesh and the oracle's side of it: streams, decode, trace and classes (made once, read only)"""

    def __init__(self, mesh_fn, q):
        self.ply = mesh_fn().to_ply()
        self.q = q
        self.quant = [(1, -1, q)] if q else []
        o = op.Mesh.from_ply(self.ply)
        if q:
            o.requant(self.quant)
        self.quantised = o
        self.compat = o.clone().encode().data
        self.ref = op.Mesh.from_hry_traced(self.compat)
        self.trace = self.ref.vertex_trace()
        self.ncomp = len(self.ref.list_fmt(1))

    def classes(self, comp):
        return cr.classify_vertices(self.trace, self.ref.component(1, comp), self.q, self.trace["comp_first"], comp)


_PER_VALUE = ("clamp0", "clamptop", "near", "far_code", "raw", "float_tie", "leaves", "run_leaves0", "run_leaves1", "run_leaves2p")


def teams_of(sliced: bool):
    """the team sizes a case's k_unpredict3 chains run at: k_unpredict3 itself holds at most eight wavefronts (HRY_CHAIN_WAVES=12
    gives it eight), k_unpredict3_range -- the pipelined decode's, for the cases that qualify -- takes all twelve"""
    return TEAMS if sliced else TEAMS[:3]


def census(b: Built, scanned: bool):
    """({vertex class: vertices}, {team size: {tile class: tiles}}): what the connectivity decides is counted once, what the values
    decide (clamps, residual codes, ties, vertices that leave the speculated form) is summed over the list's components"""
    vsum, tsum = {}, {W: {} for W in TEAMS}
    for c in range(b.ncomp):
        vc = b.classes(c)
        for k, n in cr.vertex_census(vc).items():
            vsum[k] = vsum.get(k, 0) + n if k in _PER_VALUE else n
        for W in TEAMS if scanned else ():
            for k, n in cr.tile_census(vc, W).items():
                tsum[W][k] = tsum[W].get(k, 0) + n if k in _PER_VALUE else n
    return vsum, tsum


# ---------------------------------------------------------------------------------------------------------------------------
def main():
    from harry_amd import codec as hc

    class Mismatch(Exception):
        pass

    def check(case, cond, what):
        if not cond:
            raise Mismatch(f"{case}: {what}")

    def same(case, what, dec, ref):
        check(case, (dec.nv, dec.nf, dec.ne) == (ref.nv, ref.nf, ref.ne), f"{what}: sizes")
        check(case, np.array_equal(dec.org(), ref.org()), f"{what}: connectivity")
        for l in (0, 1):
            x, y = dec.list_data(l), ref.list_data(l)
            if not np.array_equal(x, y):
                bad = np.flatnonzero((x != y).any(axis=1))
                raise Mismatch(f"{case}: {what}: list {l}: {len(bad)} records differ, first {bad[:6].tolist()}, byte columns {np.flatnonzero((x != y).any(axis=0)).tolist()}")

    def table(case, what, b, cx):
        """the staged candidate table against the oracle's trace"""
        count, tri = b.trace["count"], b.trace["triples"]
        n = len(count)
        ncand = cx.stage("ncand")[:n]
        cand = cx.stage("cand", np.uint32).reshape(-1, 6)[:n]
        over = cx.stage("cand_over", np.uint32)
        want_n = np.where(count > 8, 0xff, count).astype(np.uint8)
        bad = np.flatnonzero(ncand != want_n)
        check(case, not len(bad), f"{what}: ncand of vertex {bad[:1].tolist()}: {ncand[bad[:1]].tolist()}, the oracle counts {count[bad[:1]].tolist()} ({len(bad)} differ)")
        small = count <= 2
        want_row = np.where((np.arange(6)[None, :] < 3 * count[:, None]) & small[:, None], tri[:, :2].reshape(n, 6), 0)
        bad = np.flatnonzero(small & (cand != want_row).any(axis=1))
        check(case, not len(bad), f"{what}: compact row of vertex {bad[:1].tolist()} ({int(count[bad[0]]) if len(bad) else 0} candidates): {cand[bad[:1]].tolist()}, expected {want_row[bad[:1]].tolist()} ({len(bad)} differ)")
        wide = np.flatnonzero((count >= 3) & (count <= 8))
        rows = int(over[0])
        check(case, rows == len(wide) and len(over) == 16 + 24 * rows, f"{what}: {rows} overflow rows handed out ({len(over)} words staged) for {len(wide)} vertices of 3 .. 8 candidates")
        check(case, not over[1:16].any(), f"{what}: the overflow area's header behind its counter is not zero")
        slots = cand[wide, 0]
        check(case, len(np.unique(slots)) == len(wide) and (not len(wide) or int(slots.max()) < rows), f"{what}: overflow slots are not distinct numbers below {rows}")
        got = over[16:].reshape(-1, 24)[slots]
        want = np.where(np.arange(8)[None, :, None] < count[wide][:, None, None], tri[wide], 0).reshape(-1, 24)
        bad = np.flatnonzero((got != want).any(axis=1))
        check(case, not len(bad), f"{what}: overflow row of vertex {wide[bad[:1]].tolist()} ({count[wide[bad[:1]]].tolist()} candidates): {got[bad[:1]].tolist()}, expected {want[bad[:1]].tolist()} ({len(bad)} differ)")
        return len(wide), int((count > 8).sum())

    def plan_rows(cx):
        return cx.stage("chain_plan", np.uint32).reshape(-1, 6)

    def run_case(case, mesh_fn, q, kernel, stype, ring, sliced, built):
        key = (mesh_fn, q)
        if key not in built:
            built.clear()   # (one mesh at a time)
            built[key] = Built(mesh_fn, q)
        b = built[key]
        for k in ENV:
            os.environ.pop(k, None)
        # 1. quantised by the product: both profiles' bytes are the oracle's
        a = hc.Mesh.from_ply(b.ply)
        if b.quant:
            cx.requant(a, b.quant)
        check(case, cx.write_hry(a.clone(), profile=hc.PROFILE_COMPAT) == b.compat, "reference-format stream differs from the oracle's")
        chunked = cx.write_hry(a.clone(), profile=hc.PROFILE_CHUNKED)
        check(case, chunked == b.quantised.clone().encode_chunked(hc.container_info(chunked)["chunk_syms"]).data, "chunked container differs from the oracle's")
        # 2. - 4. one launch, from both formats
        n_nv = b.ref.nv
        team = forced if forced else 12 if n_nv >= 1 << 18 else 8 if n_nv >= 1 << 16 else 4
        seen = []
        os.environ["HRY_NO_PIPELINE"] = "1"
        for what, data in (("reference format", b.compat), ("container", chunked)):
            dec = cx.read_hry(data, keep_stages=True)
            n_wide, n_big = table(case, what, b, cx)   # (first: a wrong table is the better message than the values it leads to)
            same(case, f"{what}, one launch", dec, b.ref)
            plan = plan_rows(cx)
            check(case, len(plan) >= 1 and all(int(r[0]) == kernel and int(r[1]) == stype for r in plan), f"{what}: chain_plan {plan.tolist()}, expected kernel {kernel} on storage type {stype}")
            check(case, all(int(r[3]) == b.ncomp and int(r[5]) == ring for r in plan), f"{what}: chain_plan {plan.tolist()}, expected {b.ncomp} components and rings of {ring} bytes")
            check(case, all(int(r[4]) == (min(8, team) if kernel == K3 else 1) for r in plan), f"{what}: chain_plan {plan.tolist()}, expected teams of {min(8, team) if kernel == K3 else 1}")
            seen.append(plan[0].tolist())
        os.environ.pop("HRY_NO_PIPELINE")
        # ... and the container in forced slices, where the pipelined decode takes the mesh
        if sliced:
            for faces, slice_ in SLICES:
                # (what is left when the replay is done goes in pieces of HRY_PIPELINE_LAST_PIECE once it is more than three of them:
                # with the slice's size there too, a mesh of more than three slices is cut however fast the replay was)
                os.environ.update(HRY_PIPELINE_MIN_VERTICES="0", HRY_PIPELINE_FACES=str(faces), HRY_PIPELINE_SLICE=str(slice_), HRY_PIPELINE_LAST_PIECE=str(slice_))
                what = f"container, slices of {slice_} vertices"
                dec = cx.read_hry(chunked, keep_stages=True)
                table(case, what, b, cx)
                same(case, what, dec, b.ref)
                plan = plan_rows(cx)
                check(case, len(plan) >= 1 and all(int(r[0]) == K3_RANGE and int(r[1]) == stype and int(r[4]) == team and int(r[5]) == ring for r in plan),
                      f"{what}: chain_plan {plan[:3].tolist()}, expected the range kernel on storage type {stype} with teams of {team}")
                check(case, n_nv <= 3 * slice_ or len(plan) >= 2, f"{what}: one slice only")
                seen.append(plan[0].tolist() + [len(plan)])
            for k in ENV:
                os.environ.pop(k, None)
        return f"nv {n_nv} rows {n_wide} above-eight {n_big} plan {seen}"

    forced = min(16, int(os.environ.get("HRY_CHAIN_WAVES", "0") or 0))
    only = sys.argv[1:]
    cx = hc.Codec(0)
    t_start = time.time()
    built = {}
    try:
        for case, mesh_fn, q, kernel, stype, ring, sliced, _, _ in CASES:
            if only and case not in only:
                continue
            t = time.time()
            line = run_case(case, mesh_fn, q, kernel, stype, ring, sliced, built)
            print(f"{case:20s} waves {forced or 'unset':5} {line}  ({time.time() - t:.1f} s)", flush=True)
    except Mismatch as e:
        print("MISMATCH", e, flush=True)
        sys.exit(1)
    finally:
        for k in ENV:
            os.environ.pop(k, None)
    cx.close()
    print(f"total {time.time() - t_start:.1f} s")
    print("all equal")


if __name__ == "__main__":
    main()
