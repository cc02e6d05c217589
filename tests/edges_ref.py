"""numpy restatement of hry_edges_build (include/harry_amd.h): unique edges, adjacency and per-edge geometry of a render build, from
its `indices`, `vertex_source` and the float32 position rows of its output vertices.  The topology is np.unique over the keys,
renumbered by first index, and a stable argsort; the geometry is float64 with every operation rounded on its own, in the order the
header writes them -- numpy's elementwise products, sums, quotients and square roots are exactly that -- and the cotangent sum is a
plain loop over the edge's sides in ascending order."""
from __future__ import annotations

import numpy as np

NO_ELEMENT = 0xFFFFFFFF
FIXED = ("edges", "tri_edges", "edge_offsets", "edge_sides", "tri_neighbours")
GEOMETRY = ("edge_length", "edge_cot", "edge_cos")


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _norm(a):
    return np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])


def _usable(x):
    return (x > 0.0) & (x < np.inf)   # (false for NaN)


def build(indices, vertex_source, positions=None) -> dict:
    """indices u32 [T, 3], vertex_source u32 [U], positions f32 [U, 3] or None -> the buffers of hry_edges_build by name, plus
    "summary" = (E, edges with one side, with two, with more)"""
    I = np.asarray(indices, np.int64).reshape(-1, 3)
    vs = np.asarray(vertex_source, np.int64)
    T = len(I)
    frm, to, oth = I.reshape(-1), I[:, [1, 2, 0]].reshape(-1), I[:, [2, 0, 1]].reshape(-1)
    a, b = vs[frm], vs[to]
    key = (np.minimum(a, b).astype(np.uint64) << np.uint64(32)) | np.maximum(a, b).astype(np.uint64)
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")            # edges in order of their first side
    rank = np.empty(len(first), np.int64)
    rank[order] = np.arange(len(first))
    tri_edges = rank[inv.reshape(-1)]
    E = len(first)
    s0 = first[order]
    swap = a[s0] > b[s0]
    edges = np.stack([np.where(swap, to[s0], frm[s0]), np.where(swap, frm[s0], to[s0])], axis=1) if E else np.zeros((0, 2), np.int64)
    sides = np.argsort(tri_edges, kind="stable")        # per edge its sides, ascending
    counts = np.bincount(tri_edges, minlength=E)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    nb = np.full(3 * T, NO_ELEMENT, np.int64)
    two = np.flatnonzero(counts == 2)
    p, q = sides[offsets[two]], sides[offsets[two] + 1]
    nb[p], nb[q] = q // 3, p // 3
    out = {
        "edges": edges.astype(np.uint32), "tri_edges": tri_edges.astype(np.uint32).reshape(T, 3), "edge_offsets": offsets.astype(np.uint32),
        "edge_sides": sides.astype(np.uint32), "tri_neighbours": nb.astype(np.uint32).reshape(T, 3),
        "summary": (E, int((counts == 1).sum()), int((counts == 2).sum()), int((counts > 2).sum())),
    }
    if positions is None:
        return out
    P = np.asarray(positions, np.float32)[:, :3].astype(np.float64)
    with np.errstate(all="ignore"):
        length = _norm(P[edges[:, 1]] - P[edges[:, 0]]).astype(np.float32)
        u, v = P[frm] - P[oth], P[to] - P[oth]
        l = _norm(_cross(u, v))
        c = _dot(u, v) / l
        c = np.where(_usable(l) & np.isfinite(c), c, 0.0)
        S = np.zeros(E, np.float64)
        for e in range(E):                              # strictly in order, one after the other
            acc = np.float64(0.0)
            for s in sides[offsets[e]:offsets[e + 1]]:
                acc = acc + c[s]
            S[e] = acc
        cot = (0.5 * S).astype(np.float32)
        N = _cross(P[I[:, 1]] - P[I[:, 0]], P[I[:, 2]] - P[I[:, 0]])
        ln = _norm(N)
        n = N / ln[:, None]
        cos = np.full(E, 2.0, np.float32)
        t0, t1 = p // 3, q // 3
        d = _dot(n[t0], n[t1])
        d = np.where((a[p] == a[q]) & (b[p] == b[q]), -d, d)
        ok = _usable(ln[t0]) & _usable(ln[t1])
        cos[two[ok]] = d[ok].astype(np.float32)
    out.update(edge_length=length, edge_cot=cot, edge_cos=cos)
    return out


def float_steps(got, want):
    """(values that are not bit-equal, the largest distance in float32 steps); NaN equals NaN, and a NaN against a number is infinitely far"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)

    def ordered(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    both_nan = np.isnan(got) & np.isnan(want)
    d = np.abs(ordered(got) - ordered(want)).astype(np.float64)
    d[both_nan] = 0
    d[np.isnan(got) != np.isnan(want)] = np.inf
    differ = (got.view(np.uint32) != want.view(np.uint32)) & ~both_nan
    return int(differ.sum()), (float(d.max()) if d.size else 0.0)
