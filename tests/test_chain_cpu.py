"""What the designed meshes of tests/tools/chain_cases.py demand of the decoder's reconstruction, counted from the CPU oracle alone
(tests/chain_ref.py over oracle_py.Mesh.vertex_trace()); no GPU.  A case is there for its classes: at least 32 vertices of every vertex
class and at least 4 tiles of every tile class it names, at every team size W its chains run at (k_unpredict3 holds at most eight
wavefronts; the pipelined decode's k_unpredict3_range, for the cases that qualify, takes twelve).  The minima are conditions of the
cases, not measurements; the meshes are the smallest found that meet them.  The census as it stands (vertex classes that the values
decide -- clamps, residual codes, ties -- and the run classes are summed over x, y, z; what the connectivity decides is counted once):

    hubs_q8               1672 vertices,  73 components | cand0 128, cand1 624, cand2 689, cand3_8 195, cand9p 36, cross 72, cross_many 72
    hubs_q12              1672 vertices,  73 components | cand0 128, cand1 624, cand2 689, cand3_8 195, cand9p 36, cross 72, cross_many 72
    hubs_f32              1672 vertices,  73 components | cand0 128, cand1 624, cand2 689, cand3_8 195, cand9p 36, cross 72, cross_many 72
    long_rows_q12        25200 vertices,   1 components | older16320 486, ring_edge 68
                        W =  1: heads0 130, dense 263, stretch17p 131
                        W =  4: heads0 130, dense 263, stretch17p 131
                        W =  8: heads0 130, dense 263, stretch17p 131
                        W = 12: heads0 130, dense 263, stretch17p 131
    long_rows_f32        25200 vertices,   1 components | older8192 8401
    long_rows_f32_half   31400 vertices, 351 components | older4096 1910
    shared_q12            3812 vertices, 173 components | cross 67, cross_many 67, cand3_8 150, cand9p 32
    heads_q12            69696 vertices,   1 components | chained 68091, constant 1605
                        W =  1: heads0 111, heads1 290, heads2_8 670, heads9_12 7, heads13p 11, rowheads9p 8, late 7, dense 11, stretch17p 1059
                        W =  4: heads0 102, heads1 270, heads2_8 527, heads9_12 11, heads13p 179, rowheads9p 8, late 179, dense 11, stretch17p 1059
                        W =  8: heads0 78, heads1 119, heads2_8 305, heads9_12 6, heads13p 581, rowheads9p 8, late 576, dense 11, stretch17p 1059
                        W = 12: heads0 5, heads1 12, heads2_8 68, heads9_12 11, heads13p 993, rowheads9p 8, late 993, dense 11, stretch17p 1059
    pieces_q12            3342 vertices,  22 components | cand0 329, cand1 1660, cand2 913, cand3_8 440
                        W =  1: heads13p 60, rowheads9p 19, late 4, dense 60
                        W =  4: heads13p 63, rowheads9p 19, late 6, dense 60
                        W =  8: heads13p 63, rowheads9p 19, late 6, dense 60
    noisy_q1             10000 vertices,   1 components | clamp0 390, clamptop 261, raw 19640, chained 9802, constant 198
                        W =  1: run_leaves0 50, run_leaves1 52, run_leaves2p 387
                        W =  4: run_leaves0 50, run_leaves1 59, run_leaves2p 387
                        W =  8: run_leaves0 50, run_leaves1 52, run_leaves2p 387
                        W = 12: run_leaves0 50, run_leaves1 52, run_leaves2p 387
    noisy_q2             10000 vertices,   1 components | clamp0 240, clamptop 221, far_code 306, raw 11573, near 18121, chained 9802, constant 198
                        W =  1: run_leaves0 54, run_leaves1 145, run_leaves2p 306
                        W =  4: run_leaves0 54, run_leaves1 149, run_leaves2p 306
                        W =  8: run_leaves0 54, run_leaves1 145, run_leaves2p 306
                        W = 12: run_leaves0 54, run_leaves1 145, run_leaves2p 306
    noisy_q8             10000 vertices,   1 components | clamp0 1294, clamptop 53, far_code 916, raw 2441, near 26643, chained 9802, constant 198
                        W =  1: run_leaves0 186, run_leaves1 120, run_leaves2p 200
                        W =  4: run_leaves0 186, run_leaves1 121, run_leaves2p 200
                        W =  8: run_leaves0 186, run_leaves1 120, run_leaves2p 200
                        W = 12: run_leaves0 186, run_leaves1 120, run_leaves2p 200
    noisy_q9             10000 vertices,   1 components | clamp0 1348, clamptop 55, far_code 941, raw 2381, near 26678, chained 9802, constant 198
                        W =  1: run_leaves0 180, run_leaves1 132, run_leaves2p 200
                        W =  4: run_leaves0 180, run_leaves1 133, run_leaves2p 200
                        W =  8: run_leaves0 180, run_leaves1 132, run_leaves2p 200
                        W = 12: run_leaves0 180, run_leaves1 132, run_leaves2p 200
    noisy_q16            10000 vertices,   1 components | clamp0 1404, clamptop 61, far_code 966, raw 2327, near 26707, chained 9802, constant 198
                        W =  1: run_leaves0 177, run_leaves1 131, run_leaves2p 201
                        W =  4: run_leaves0 177, run_leaves1 132, run_leaves2p 201
                        W =  8: run_leaves0 177, run_leaves1 131, run_leaves2p 201
                        W = 12: run_leaves0 177, run_leaves1 131, run_leaves2p 201
    wide_q17             10000 vertices,   1 components | clamp0 1404, clamptop 61, far_code 967, raw 2327, near 26706
    wide_q24             10000 vertices,   1 components | clamp0 1404, clamptop 56, far_code 956, raw 2327, near 26717
    ties_f32              4096 vertices,   1 components | float_tie 3421

The classes nothing here reaches: a vertex with more than eight candidates whose sources lie in its OWN component (the walk hands a
vertex out when it meets its first face, never behind all of its neighbours: the many-candidate centres are single new vertices of
components that name an earlier one's), and, for the team of twelve, a mesh other than heads_q12 with tiles of 1 .. 12 heads (a
source must lie more than 64 x 11 vertices back, and the front of a regular mesh of n vertices is about 2 sqrt(n) long)."""
import numpy as np
import pytest

from oracle import oracle_py as op
from tests import chain_ref as cr
from tests.tools import chain_cases as cc

_built = {}


def built(fn, q):
    if (fn, q) not in _built:
        _built[(fn, q)] = cc.Built(fn, q)
    return _built[(fn, q)]


@pytest.mark.parametrize("case", cc.CASES, ids=[c[0] for c in cc.CASES])
def test_case_meets_its_census(case):
    name, fn, q, kernel, stype, ring, sliced, vertex_classes, tile_classes = case
    b = built(fn, q)
    assert b.ref.nv <= 70000
    vs, ts = cc.census(b, kernel == cc.K3)
    short = {k: vs[k] for k in vertex_classes if vs[k] < cc.MIN_VERTICES}
    assert not short, f"{name}: vertex classes below {cc.MIN_VERTICES}: {short}"
    for W in cc.teams_of(sliced) if tile_classes else ():
        short = {k: ts[W][k] for k in tile_classes if ts[W][k] < cc.MIN_TILES}
        assert not short, f"{name}: tile classes below {cc.MIN_TILES} with teams of {W}: {short}"
    # where the case is meant to run: storage type and kernel follow from q as the product decides them
    fmt = b.ref.list_fmt(1)
    assert all(op.stype_of(t, qq) == stype for t, qq, _ in fmt)
    assert (kernel == cc.K3) == (stype in (cc.U16, cc.U8))
    if kernel == cc.K2:   # the rule of launch_unpredict2: rings of half the size for more than 1 024 chains
        first = np.append(b.trace["comp_first"], b.ref.nv)
        owners = np.diff(first)
        owners = owners[owners > 0]
        tiny, lists, run = owners < 64, 0, 0
        for t in tiny:   # (consecutive tiny components share a work list, up to 64 of them: group_chain_lists)
            if not t or run == 0 or run >= 64:
                lists, run = lists + 1, 0
            run = run + 1 if t else 0
        assert (cc.RING_HALF if lists * len(fmt) > 1024 else cc.RING_FULL) == ring


@pytest.mark.parametrize("case", [c for c in cc.CASES if c[0] in ("hubs_q12", "hubs_f32", "noisy_q2", "wide_q17")], ids=lambda c: c[0])
def test_recording_changes_nothing_and_agrees_with_itself(case):
    name, fn, q = case[:3]
    b = built(fn, q)
    plain = op.Mesh.from_hry(b.compat)
    assert np.array_equal(plain.org(), b.ref.org())
    for l in (0, 1):
        assert np.array_equal(plain.list_data(l), b.ref.list_data(l))
    assert plain.vertex_trace()["count"].size == 0
    tr = b.trace
    n = b.ref.nv
    assert tr["count"].shape == (n,) and tr["triples"].shape == (n, 8, 3) and tr["pred"].shape == (n, b.ncomp)
    v = np.arange(n)[:, None, None]
    have = np.broadcast_to((np.arange(8)[None, :] < np.minimum(tr["count"], 8)[:, None])[:, :, None], tr["triples"].shape)
    assert (tr["triples"][have] < np.broadcast_to(v, have.shape)[have]).all(), "a source that is not decoded before its vertex"
    assert not tr["triples"][~have].any()
    first = tr["comp_first"]
    assert first[0] == 0 and (np.diff(first.astype(np.int64)) >= 0).all() and first[-1] <= n
    if q == 0:
        return
    # the prediction the oracle says it used is the rounded mean of the recorded triples' saturated parallelograms
    # (attrcode.h:182-208, prediction.h:121-138) over the decoded values -- for every vertex whose triples are all recorded
    top = (1 << q) - 1
    full = tr["count"] <= 8
    for c in range(b.ncomp):
        val = b.ref.component(1, c).astype(np.int64)
        t = tr["triples"].astype(np.int64)
        p = np.clip(val[t[:, :, 0]] + val[t[:, :, 1]] - val[t[:, :, 2]], 0, top)
        cnt = tr["count"].astype(np.int64)
        s = np.where(np.arange(8)[None, :] < cnt[:, None], p, 0).sum(axis=1)
        want = np.where(cnt > 0, (s + cnt // 2) // np.maximum(cnt, 1), 0)
        bad = np.flatnonzero(full & (want != tr["pred"][:, c].astype(np.int64)))
        assert not len(bad), f"{name}: component {c}, vertex {bad[:4].tolist()}"


@pytest.mark.parametrize("bits,q", [(8, 1), (8, 2), (8, 8), (16, 9), (16, 16), (32, 17), (32, 24), (32, 0)])
def test_code_classes_are_the_forms_of_the_reference_code(bits, q):
    """NEAR: value = pred + ((code >> 1) ^ -(code & 1)); RAW: the code is the value and the prediction 0; FAR: neither
    (prediction.h:46-64), with the code the oracle writes (prediction.h:81-99)"""
    L = op.lib()
    rng = np.random.default_rng(bits * 100 + q)
    top = (1 << (q or bits)) - 1
    n = 3000
    value = rng.integers(0, top + 1, n, dtype=np.int64)
    pred = np.clip(value + rng.integers(-40, 41, n) * rng.integers(0, 2, n) + (rng.integers(0, 8, n) == 0) * rng.integers(-top, top + 1, n), 0, top)
    pred[::17] = 0
    pred[5::19] = top
    cls = cr.code_class(value, pred, top)
    assert ({cr.NEAR, cr.RAW} if q == 1 else {cr.NEAR, cr.FAR, cr.RAW}) <= set(cls.tolist())   # (one bit: no room for a far code)
    for v, p, k in zip(value.tolist(), pred.tolist(), cls.tolist()):
        code = L.ho_kat_encode_delta_u(v, p, bits // 8, q)
        assert L.ho_kat_decode_delta_u(code, p, bits // 8, q) == v
        near_form = p + ((code >> 1) ^ -(code & 1))
        if k == cr.RAW:
            assert p == 0 and code == v
        elif k == cr.NEAR:
            assert near_form == v
        else:
            assert p != 0 and (code >> 1) > min(p - 1, top - p)


def test_classes_of_a_hand_made_trace():
    """eight vertices of one component and two of a second one, the rules of tests/chain_ref.py spelled out on them"""
    count = np.array([0, 0, 0, 1, 2, 3, 1, 9, 1, 2], np.uint32)
    tri = np.zeros((10, 8, 3), np.uint32)
    tri[3, 0] = (2, 1, 0)          # chained through a = v - 1
    tri[4, :2] = ((0, 1, 2), (1, 3, 2))   # chained through b of the second candidate; the others' latest is 2
    tri[5, :3] = ((4, 3, 2), (3, 2, 1), (2, 1, 0))
    tri[6, 0] = (1, 2, 5)          # o = v - 1 is no chained source
    tri[7, :8] = [(6, 5, 4)] * 8
    tri[8, 0] = (7, 6, 5)          # first vertex of its component: never chained, every source of an earlier component
    tri[9, :2] = ((8, 3, 2), (2, 8, 1))
    trace = {"count": count, "triples": tri, "pred": np.zeros((10, 1), np.uint64)}
    values = np.array([5, 6, 7, 8, 200, 9, 250, 10, 11, 12], np.uint8)
    vc = cr.classify_vertices(trace, values, 8, [0, 8], 0)
    assert vc["chained"].tolist() == [False, False, False, True, True, False, False, False, False, True]
    assert vc["pos"].tolist() == [7, 7, 7, 0, 4, 7, 7, 7, 7, 0]
    assert vc["gap"].tolist() == [65535, 65535, 65535, 2, 2, 65535, 1, 65535, 1, 1]
    assert vc["cross"].tolist() == [False] * 8 + [True, True]
    assert vc["cross_many"].sum() == 0 and vc["cand3_8"].tolist()[5] and vc["cand9p"].tolist()[7]
    # vertex 4: 5 + 6 - 7 = 4 and 6 + 8 - 7 = 7; vertex 6: 6 + 7 - 9 = 4; vertex 9: 11 + 8 - 7 = 12 and 7 + 11 - 6 = 12; vertex 5: 200 + 8 - 7
    assert not vc["clamp0"].any() and vc["clamptop"].tolist() == [False] * 10
    tc = cr.classify_tiles(vc, 1)
    assert tc["nheads"].tolist() == [5, 2]   # vertices 3, 4, 6 (recent sources), 5 and 7 (many candidates); 8 and 9
