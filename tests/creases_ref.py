"""A numpy restatement of the creases contract of include/harry_amd.h (hry_creases_build) over tests/edges_ref.py: the classes of the
edges, the groups of the index slots (a union-find whose root is the smallest member), the split vertices (first occurrence of
(index, group) over ascending slot) and the normals, in float64 with every operation rounded on its own in the written order: a
group's sum starts from +0 and adds the terms of its slots in ascending slot, one after the other (in rounds: round r adds the r-th
slot of every group that has one); a group of more than 32 slots sums 256 consecutive ranges of ceil(n / 256) slots each in that way,
each from +0, and adds the 256 partial sums in range order.  Results are rounded to float32 once.

Tolerance of a comparison against the device, by the argument of tests/normals_ref.py: both sides evaluate in double, in the same
order and association, and round to float once; they differ by a last place in sqrt, the division and atan2 -- relative errors of
order 2^-50 before the rounding, so a component is the same float or its neighbour, and with |component| <= 1 neighbours are at most
2^-24 apart: normals_ref.TOL.  That holds only where the sum does not cancel: `guard[w]` says |S_g| >= 2^-20 * sum |terms| of the
group of split vertex w (a group without terms, or with a sum that is not finite, is admitted: its row is zeros on both sides).  A
test compares guarded vertices only, and asserts that the guard excluded none."""
from __future__ import annotations

import numpy as np

from tests import edges_ref as er
from tests.normals_ref import TOL  # noqa: F401  (the comparison's tolerance, by name)

SMOOTH, SHARP, BOUNDARY, NONMANIFOLD, MISORIENTED, DEGENERATE = 0, 1, 2, 3, 4, 5
INTEGER = ("indices", "render_vertex", "vertex_source", "slot_group", "edge_class")
SUMMARY = ("vertices", "groups", "smooth", "sharp", "split", "other")
SEG_MAX, RANGES = 32, 256


def _next(s):
    return s - 2 if s % 3 == 2 else s + 1


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _length(a):
    return np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])


def _usable(n):
    return (n > 0) & (n < np.inf)   # (false for NaN)


def classify(indices, vertex_source, tri_face, edges, cos_limit):
    """edge_class [E], and the pairs of slots the SMOOTH edges unite [R, 2]"""
    flat = np.asarray(indices, np.int64).reshape(-1)
    vs = np.asarray(vertex_source, np.int64)
    tf = np.asarray(tri_face, np.int64)
    off, sides, cos = edges["edge_offsets"].astype(np.int64), edges["edge_sides"].astype(np.int64), edges["edge_cos"]
    cls = np.zeros(len(off) - 1, np.uint32)
    pairs = []
    for e in range(len(cls)):
        seg = sides[off[e]:off[e + 1]]
        if len(seg) == 1:
            cls[e] = BOUNDARY
            continue
        if len(seg) > 2:
            cls[e] = NONMANIFOLD
            continue
        p, q = int(seg[0]), int(seg[1])
        a0, a1, b0, b1 = vs[flat[p]], vs[flat[_next(p)]], vs[flat[q]], vs[flat[_next(q)]]
        if a0 == a1:
            cls[e] = DEGENERATE
        elif a0 == b0 and a1 == b1:
            cls[e] = MISORIENTED
        elif tf[p // 3] == tf[q // 3]:
            cls[e] = SMOOTH
        elif cos[e] == np.float32(2.0):
            cls[e] = DEGENERATE
        else:
            cls[e] = SMOOTH if np.float64(cos[e]) >= cos_limit else SHARP
        if cls[e] == SMOOTH:
            for v in (a0, a1):
                pairs.append((p if vs[flat[p]] == v else _next(p), q if vs[flat[q]] == v else _next(q)))
    return cls, np.array(pairs, np.int64).reshape(-1, 2)


def roots_of(n, pairs):
    """the smallest member of every slot's set"""
    par = np.arange(n)

    def find(x):
        while par[x] != x:
            par[x] = par[par[x]]
            x = par[x]
        return x
    for a, b in pairs:
        a, b = find(int(a)), find(int(b))
        if a != b:
            par[max(a, b)] = min(a, b)
    return np.array([find(s) for s in range(n)], np.int64)


def _sum_in_order(owner, nown, term, live):
    """per owner the sum of its live items' terms in ascending item, from +0, one after the other (in rounds)"""
    S = np.zeros((nown,) + term.shape[1:])
    order = np.argsort(owner, kind="stable")
    ov = owner[order]
    first = np.concatenate([[0], np.cumsum(np.bincount(ov, minlength=nown))])[:-1]
    rank = np.arange(len(ov)) - first[ov]
    by_rank = np.argsort(rank, kind="stable")
    cuts = np.concatenate([[0], np.cumsum(np.bincount(rank, minlength=1))])
    for r in range(len(cuts) - 1):
        sel = by_rank[cuts[r]:cuts[r + 1]]
        sel = sel[live[order[sel]]]   # (a triangle without a normal adds nothing: not even +0 to a -0)
        S[ov[sel]] += term[order[sel]]
    return S


def topology(indices, vertex_source, tri_face, positions, cos_limit, edges=None):
    """what the weights do not change: (edge_class [E], the root of every slot [3 T]); edges: edges_ref.build's, where at hand"""
    I = np.asarray(indices, np.int64).reshape(-1, 3)
    if edges is None:
        edges = er.build(I, vertex_source, positions)
    cls, pairs = classify(I, vertex_source, tri_face, edges, cos_limit)
    return cls, roots_of(3 * len(I), pairs)


def build(indices, vertex_source, tri_face, positions, cos_limit, weights="area", edges=None, topo=None) -> dict:
    """indices u32 [T, 3], vertex_source u32 [U], tri_face u32 [T], positions f32 [U, 3]: what the render build holds -> the buffers of
    hry_creases_build by name, plus "summary" (SUMMARY's counts), "guard" bool [W] and "group_slots" (slots per group).  topo:
    topology()'s result for the same arguments, where at hand"""
    assert weights in ("area", "angle") and not np.isnan(cos_limit)
    I = np.asarray(indices, np.int64).reshape(-1, 3)
    vs = np.asarray(vertex_source, np.int64)
    T, n = len(I), 3 * len(I)
    flat = I.reshape(-1)
    cls, root = topology(I, vs, tri_face, positions, cos_limit, edges) if topo is None else topo
    firsts, group = np.unique(root, return_inverse=True)   # (ascending smallest slot)
    group = group.reshape(-1)
    G = len(firsts)
    # ---- split vertices: first occurrence of (index, group) over ascending slot
    key = flat.astype(np.uint64) << np.uint64(32) | group.astype(np.uint64)
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(first), np.int64)
    rank[order] = np.arange(len(first))
    ids = rank[inv.reshape(-1)]
    W = len(first)
    first_slot = first[order]
    render_vertex = flat[first_slot]
    # ---- terms
    with np.errstate(all="ignore"):
        P = np.asarray(positions, np.float32)[:, :3].astype(np.float64)
        N = _cross(P[I[:, 1]] - P[I[:, 0]], P[I[:, 2]] - P[I[:, 0]])
        ln = _length(N)
        ok = _usable(ln)
        tri = np.repeat(np.arange(T), 3)
        if weights == "area":
            term, mag = N[tri], ln[tri]
        else:
            k = np.tile(np.arange(3), T)
            a, b = P[I[tri, (k + 1) % 3]] - P[flat], P[I[tri, (k + 2) % 3]] - P[flat]
            theta = np.arctan2(_length(_cross(a, b)), _dot(a, b))
            term, mag = theta[:, None] * (N / ln[:, None])[tri], np.abs(theta)
        live = ok[tri]
        term = np.where(live[:, None], term, 0.0)
        mag = np.where(live, mag, 0.0)
        # ---- S_g: the lane's order up to 32 slots, 256 ranges beyond
        sizes = np.bincount(group, minlength=G)
        by_group = np.argsort(group, kind="stable")
        place = np.empty(n, np.int64)   # the place of slot s within its group, ascending
        place[by_group] = np.arange(n) - np.concatenate([[0], np.cumsum(sizes)])[:-1][group[by_group]]
        S = _sum_in_order(group, G, term, live)
        for g in np.flatnonzero(sizes > SEG_MAX):
            slots = np.flatnonzero(group == g)
            chunk = -(-len(slots) // RANGES)
            part = _sum_in_order(place[slots] // chunk, RANGES, term[slots], live[slots])
            acc = part[0].copy()
            for r in range(1, RANGES):
                acc = acc + part[r]
            S[g] = acc
        A = np.bincount(group, weights=mag, minlength=G)
        lg = _length(S)
        gok = _usable(lg)
        gn = np.zeros((G, 3), np.float32)
        gn[gok] = (S[gok] / lg[gok][:, None]).astype(np.float32)
        gguard = ~(lg < 2.0 ** -20 * A)
    wgroup = group[first_slot]
    per_vertex = np.bincount(vs[flat[firsts]], minlength=1)   # groups per decoded vertex: a group lies at one decoded vertex
    summary = (W, G, int((cls == SMOOTH).sum()), int((cls == SHARP).sum()), int((per_vertex > 1).sum()), int((cls >= BOUNDARY).sum()))
    return {
        "indices": ids.astype(np.uint32).reshape(T, 3), "render_vertex": render_vertex.astype(np.uint32), "vertex_source": vs[render_vertex].astype(np.uint32),
        "normals": gn[wgroup].reshape(W, 3), "slot_group": group.astype(np.uint32).reshape(T, 3), "edge_class": cls,
        "summary": summary, "guard": gguard[wgroup], "group_slots": sizes,
    }


def of_arrays(positions, degrees, corners, cos_limit, weights="area", vertex_source=None):
    """the restatement of a mesh in the PLY layout: the fan of shells_ref.fan, vertex_source the identity unless given"""
    from tests import shells_ref as sr
    I, tf = sr.fan(degrees, corners)
    pos = np.asarray(positions, np.float32)
    return build(I, np.arange(len(pos)) if vertex_source is None else vertex_source, tf, pos, cos_limit, weights)


def of_mesh(m, cos_limit, weights="area"):
    """the same for a meshgen mesh (fields x, y, z)"""
    return of_arrays(np.stack([m.verts["x"], m.verts["y"], m.verts["z"]], axis=1), m.degrees, m.indices, cos_limit, weights)


def from_render(rn, positions, cos_limit, weights="area"):
    """the restatement from a render build's host arrays (Codec.render_numpy) and the float rows of its positions"""
    return build(rn["indices"], rn["vertex_source"], rn["tri_face"], positions, cos_limit, weights)
