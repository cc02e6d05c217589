"""The twin matching and the component analysis of a mesh (twins.hip: k_twin_*, k_cc_*; analysis.cpp; host/cbm_walk.cpp: analyse_impl)
restated in plain numpy, for tests/test_analysis_cpu.py and tests/test_gpu_analysis.py.  The one thing taken from the library is the
start-face sequence (the spans of hry_analysis_tables): its order is that of a libstdc++ hash set and is pinned against the oracle's
traced encode on its own (test_analysis_cpu.py: test_start_face_sequence_equals_the_oracles_order)."""
from __future__ import annotations

import numpy as np

try:
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components as _cc
except ImportError:   # the same partition by pointer jumping
    _cc = None

NONE = 0xFFFFFFFF
PER_RANK = ("by_rank", "seed", "n_faces", "n_halfedges", "fresh", "group", "face_lo", "face_hi", "vtx_lo", "vtx_hi")


def partition(n, a, b):
    """the sets of 0 .. n-1 under the undirected relations (a[i], b[i]) -> a label per element, in no particular numbering"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if _cc is not None:
        g = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n, n))
        return _cc(g, directed=False)[1].astype(np.int64)
    lab = np.arange(n, dtype=np.int64)
    while True:   # every element takes the smallest label among its neighbours' until nothing moves, the labels jumping to their own
        m = lab.copy()
        np.minimum.at(m, a, lab[b])
        np.minimum.at(m, b, lab[a])
        m = m[m]
        if np.array_equal(m, lab):
            return lab
        lab = m


def by_first_occurrence(lab):
    """labels renumbered densely in the order of their first elements: what "numbered in face order of the roots" is when a root is
    the smallest element of its set"""
    _, first, inv = np.unique(lab, return_index=True, return_inverse=True)
    new = np.empty(len(first), np.int64)
    new[np.argsort(first, kind="stable")] = np.arange(len(first))
    return new[inv.reshape(-1)]


def same_partition(x, y):
    """do two labellings of the same elements describe one partition, whatever their numbers"""
    x, y = np.asarray(x, np.int64).reshape(-1), np.asarray(y, np.int64).reshape(-1)
    if len(x) != len(y):
        return False
    if len(x) == 0:
        return True
    pairs = np.unique(np.stack([x, y], axis=1), axis=0)
    return len(pairs) == len(np.unique(x)) == len(np.unique(y))


def faces_of_halfedges(face_offsets):
    foff = np.asarray(face_offsets, np.int64)
    return np.repeat(np.arange(len(foff) - 1, dtype=np.int64), np.diff(foff))


def next_halfedge(face_offsets):
    """next(h): the half-edge after h around its face"""
    foff = np.asarray(face_offsets, np.int64)
    nxt = np.arange(1, foff[-1] + 1, dtype=np.int64)
    nxt[foff[1:] - 1] = foff[:-1]
    return nxt


def positions(spans, faces):
    """the place of every face of `faces` in the start-face sequence the spans describe (lowest face, highest face, position of the
    span's first face, ascending) sorted by the lowest face"""
    sp = np.asarray(spans, np.int64).reshape(-1, 4)
    f = np.asarray(faces, np.int64)
    i = np.searchsorted(sp[:, 0], f, side="right") - 1
    return sp[i, 2] + np.where(sp[i, 3] != 0, f - sp[i, 0], sp[i, 1] - f)


def sequence(spans):
    """the start-face sequence itself: face at every position"""
    sp = np.asarray(spans, np.int64).reshape(-1, 4)
    nf = int((sp[:, 1] - sp[:, 0] + 1).sum())
    seq = np.full(nf, -1, np.int64)
    f = np.arange(nf, dtype=np.int64)
    seq[positions(sp, f)] = f
    return seq


def analysis(face_offsets, org, twin, nv, spans):
    """-> the tables of hry_analysis_tables by name ("ncomp", the per-rank arrays, "comp"), plus "vfirst" [nv] (the first rank at every
    vertex, NONE: unreferenced), "rank_of_face" [nf] and "hit" [ne] (the corners whose vertex another rank reached first: what
    k_cc_vertex_ties notes)"""
    foff = np.asarray(face_offsets, np.int64)
    org, twin = np.asarray(org, np.int64), np.asarray(twin, np.int64)
    nf, ne = len(foff) - 1, len(org)
    fh = faces_of_halfedges(foff)
    # components: f and face(twin[h]) for every half-edge h of f with a twin, undirected
    h = np.flatnonzero(twin != np.arange(ne))
    comp = by_first_occurrence(partition(nf, fh[h], fh[twin[h]]))
    ncomp = int(comp.max()) + 1 if nf else 0
    # keys: face 0 first, the others by their place in the start-face sequence
    f = np.arange(nf, dtype=np.int64)
    key = ((positions(spans, f) + 1) << 32) | f
    key[:1] = 0
    ckey = np.full(ncomp, np.iinfo(np.int64).max)
    np.minimum.at(ckey, comp, key)
    by_rank = np.argsort(ckey, kind="stable")
    rank_of = np.empty(ncomp, np.int64)
    rank_of[by_rank] = np.arange(ncomp)
    kf = rank_of[comp]
    out = {"ncomp": np.array([ncomp]), "comp": comp, "by_rank": by_rank, "seed": ckey[by_rank] & 0xFFFFFFFF, "rank_of_face": kf}
    out["n_faces"] = np.bincount(kf, minlength=ncomp)
    out["n_halfedges"] = np.bincount(kf, weights=np.diff(foff), minlength=ncomp).astype(np.int64)
    lo, hi = np.full(ncomp, NONE, np.int64), np.zeros(ncomp, np.int64)
    np.minimum.at(lo, kf, f)
    np.maximum.at(hi, kf, f + 1)
    out["face_lo"], out["face_hi"] = lo, hi
    # the first rank at every vertex, and what each rank is first at
    kh = kf[fh]
    vfirst = np.full(nv, NONE, np.int64)
    np.minimum.at(vfirst, org, kh)
    used = np.flatnonzero(vfirst != NONE)
    out["vfirst"] = vfirst
    out["fresh"] = np.bincount(vfirst[used], minlength=ncomp)
    lo, hi = np.full(ncomp, NONE, np.int64), np.zeros(ncomp, np.int64)
    np.minimum.at(lo, vfirst[used], used)
    np.maximum.at(hi, vfirst[used], used + 1)
    out["vtx_lo"], out["vtx_hi"] = lo, hi
    # groups: ranks that share a vertex, transitively; a group is named by its smallest rank
    hit = vfirst[org] != kh
    out["hit"] = hit
    sets = partition(ncomp, vfirst[org[hit]], kh[hit])
    smallest = np.full(int(sets.max()) + 1 if ncomp else 0, NONE, np.int64)
    np.minimum.at(smallest, sets, np.arange(ncomp))
    out["group"] = smallest[sets]
    return out


def match_twins(face_offsets, org):
    """the reference's matching rule (structs/conn.h:201-214) as a dictionary loop over the half-edges in index order: a directed edge
    (a, b) takes the pending (b, a) if there is one; otherwise it becomes pending itself, unless an (a, b) is pending already -- then
    it stays without a twin for good.  For small meshes."""
    org = np.asarray(org, np.int64)
    nxt = next_halfedge(face_offsets)
    twin = np.arange(len(org), dtype=np.int64)
    pending = {}
    for h in range(len(org)):
        a, b = int(org[h]), int(org[nxt[h]])
        o = pending.pop((b, a), None)
        if o is not None:
            twin[h], twin[o] = o, h
        else:
            pending.setdefault((a, b), h)
    return twin


def compare(got, want, what):
    """every table of `got` (hry_analysis_tables) against the restatement `want`: the labels as a partition first, then as numbers"""
    assert int(got["ncomp"][0]) == int(want["ncomp"][0]), f"{what}: ncomp {int(got['ncomp'][0])}, restated {int(want['ncomp'][0])}"
    assert same_partition(got["comp"], want["comp"]), f"{what}: comp is another PARTITION of the faces"
    assert np.array_equal(got["comp"], want["comp"]), f"{what}: comp is the same partition under other NUMBERS"
    for name in PER_RANK:
        g, w = np.asarray(got[name], np.int64), np.asarray(want[name], np.int64)
        assert g.shape == w.shape, f"{what}: {name} has {g.shape} entries, restated {w.shape}"
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, f"{what}: {name} differs at {len(bad)} ranks, first {int(bad[0])}: {int(g[bad[0]])}, restated {int(w[bad[0]])}"
