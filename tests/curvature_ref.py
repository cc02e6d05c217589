"""A numpy restatement of the curvature contract of include/harry_amd.h (hry_curvature_build) over tests/edges_ref.py: per slot the
angle, the share of the mixed area, the Laplace vector and the triangle's normal, in float64 with every operation rounded on its own
in the written order; per decoded vertex the eight sums from +0 over its slots in ascending slot, one after the other (in rounds:
round r adds the r-th slot of every vertex that has one), and beyond 32 slots as 256 consecutive ranges of ceil(n / 256) slots, each
from +0, whose partial sums are added in range order; the classes from the edges' side counts; the totals in rounds of 256 rows.
Results are rounded to float32 once.

Tolerance of a comparison against the device -- derived, not measured: |got - want| <= one float32 step of want + 2^-40 * scale.
Both sides evaluate in double, in the same order and association, and round to float once; they differ only by last places of sqrt,
the division and atan2: a few 2^-52 of a term's magnitude per term.  With at most about 2^10 terms a vertex that stays below 2^-42
of `scale`, the sum of the absolute values of the terms behind the value (tau included for the defect) divided by the absolute
denominator where there is one; 2^-40 leaves a factor of four and is still 2^16 below the float32 resolution of the terms, so a wrong
order, a float atomic or a float32 intermediate fails.  A flat vertex, whose defect and Laplace vector cancel, is covered by the
scale term and not excluded by a guard: no value is left out of a comparison.
The scale of "mean": H = (L . S) / (|S| * 4 A).  An error e_j of S_j (at most a few 2^-52 of sum |N_sj|) moves |S| by at most
sum_j e_j and H by |H| sum_j e_j / |S| <= sum_j |L_j| sum_k e_k / (|S| 4 A), since |H| |S| <= sum_j |L_j| |S_j| / (4 A) and
|S_j| <= |S|; the errors of L and of the products in the numerator are bounded by the same form.  So the scale is
(sum over components and slots of |L_s|) * (sum over components and slots of |N_t|) / (|S| * 4 A), and sum |L_s| / (4 A) where |S|
is not usable.  The scale of a total is the sum of its rows' scales (for the third: the row's scale of H times A)."""
from __future__ import annotations

import numpy as np

from tests import edges_ref as er
from tests.creases_ref import _sum_in_order

ISOLATED, INTERIOR, BOUNDARY, IRREGULAR, DEGENERATE = 0, 1, 2, 3, 8
FLOATS = ("vertex_area", "angle_defect", "gaussian", "mean_normal", "mean")
BUFFERS = ("vertex_class",) + FLOATS
SUMMARY = ("vertices", "interior", "boundary", "irregular", "isolated", "degenerate")
TOTALS = ("area", "defect", "mean_integral")
SEG_MAX, RANGES, FOLD = 32, 256, 256
PI, TWO_PI = float(np.pi), float(2 * np.pi)   # the doubles nearest pi and 2 pi
EPS = 2.0 ** -40


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


_cross, _norm, _usable = er._cross, er._norm, er._usable


def slot_terms(I, P):
    """per slot s = 3 t + k: (live [n], terms [n, 8] = theta, A_s, L_s x y z, N_t x y z, branch [n]: 0 the cotangent formula, 1 the
    obtuse corner of an obtuse triangle, 2 another corner of one)"""
    T = len(I)
    p = [P[I[:, k]] for k in range(3)]
    N = _cross(p[1] - p[0], p[2] - p[0])
    ln = _norm(N)
    a = [p[(k + 1) % 3] - p[k] for k in range(3)]
    b = [p[(k + 2) % 3] - p[k] for k in range(3)]
    x = [_norm(_cross(a[k], b[k])) for k in range(3)]
    d = [_dot(a[k], b[k]) for k in range(3)]
    c = []
    for k in range(3):
        q = d[k] / x[k]
        c.append(np.where(_usable(x[k]) & np.isfinite(q), q, 0.0))
    area_t = 0.5 * ln
    obtuse = (d[0] < 0.0) | (d[1] < 0.0) | (d[2] < 0.0)
    terms = np.zeros((T, 3, 8))
    branch = np.zeros((T, 3), np.int64)
    for k in range(3):
        cn, cp = c[(k + 1) % 3], c[(k + 2) % 3]
        share = np.where(obtuse, np.where(d[k] < 0.0, 0.5 * area_t, 0.25 * area_t), 0.125 * (_dot(a[k], a[k]) * cp + _dot(b[k], b[k]) * cn))
        terms[:, k, 0] = np.arctan2(x[k], d[k])
        terms[:, k, 1] = share
        terms[:, k, 2:5] = -(cp[:, None] * a[k] + cn[:, None] * b[k])
        terms[:, k, 5:8] = N
        branch[:, k] = np.where(obtuse, np.where(d[k] < 0.0, 1, 2), 0)
    live = np.repeat(_usable(ln), 3)
    return live, terms.reshape(3 * T, 8), branch.reshape(-1)


def vertex_sums(owner, D, terms, live):
    """the eight sums per decoded vertex [D, 8], by the 32 / 256-range rule, and the slots per vertex"""
    n = len(owner)
    sizes = np.bincount(owner, minlength=D)
    S = _sum_in_order(owner, D, terms, live)
    by_owner = np.argsort(owner, kind="stable")
    place = np.empty(n, np.int64)   # the place of slot s within its vertex, ascending
    place[by_owner] = np.arange(n) - np.concatenate([[0], np.cumsum(sizes)])[:-1][owner[by_owner]]
    for v in np.flatnonzero(sizes > SEG_MAX):
        slots = np.flatnonzero(owner == v)
        chunk = -(-len(slots) // RANGES)
        part = _sum_in_order(place[slots] // chunk, RANGES, terms[slots], live[slots])
        acc = part[0].copy()
        for r in range(1, RANGES):
            acc = acc + part[r]
        S[v] = acc
    return S, sizes


def fold(rows):
    """the totals: rounds of 256 rows into one, each chunk from +0 in row order, at least one round, until one row is left"""
    rows = np.asarray(rows, np.float64).reshape(-1, 3)
    if not len(rows):
        return np.zeros(3)
    while True:
        chunks = -(-len(rows) // FOLD)
        padded = np.zeros((chunks * FOLD, 3))   # (a +0 behind the last row changes no bit: a sum that starts from +0 is never -0)
        padded[:len(rows)] = rows
        padded = padded.reshape(chunks, FOLD, 3)
        acc = np.zeros((chunks, 3))
        for i in range(FOLD):
            acc = acc + padded[:, i]
        rows = acc
        if len(rows) == 1:
            return rows[0]


def vertex_classes(flat, vs, D, edges, sizes):
    """the class of every decoded vertex, bit 8 aside"""
    off, sides = edges["edge_offsets"].astype(np.int64), edges["edge_sides"].astype(np.int64)
    count = np.diff(off)
    first = sides[off[:-1]]
    nxt = np.where(first % 3 == 2, first - 2, first + 1)
    ends = np.zeros(D, np.int64)
    for bit, sel in ((1, count == 1), (2, count > 2)):
        for s in (first[sel], nxt[sel]):
            ends[vs[flat[s]]] |= bit
    return np.where(sizes == 0, ISOLATED, np.where(ends & 2, IRREGULAR, np.where(ends & 1, BOUNDARY, INTERIOR)))


def build(indices, vertex_source, positions, nv, edges=None) -> dict:
    """indices u32 [T, 3], vertex_source u32 [U], positions f32 [U, 3], nv = D decoded vertices -> the buffers of
    hry_curvature_build by name, "summary" (SUMMARY's counts), "totals" [3], "scale": the scale of every float buffer's values, by
    name, and of the totals ("totals"); "decoded": the doubles per decoded vertex (Theta, A, L [D, 3], S [D, 3], defect, H, class),
    "branch" [3 T] and "slot_area" [3 T] (0 for a slot without terms), "tri_area" [T]"""
    I = np.asarray(indices, np.int64).reshape(-1, 3)
    vs = np.asarray(vertex_source, np.int64)
    flat = I.reshape(-1)
    D = int(nv)
    P = np.asarray(positions, np.float32)[:, :3].astype(np.float64)
    if edges is None:
        edges = er.build(I, vs)
    owner = vs[flat]
    with np.errstate(all="ignore"):
        live, terms, branch = slot_terms(I, P)
        S8, sizes = vertex_sums(owner, D, terms, live)
        absum = np.zeros((D, 8))
        np.add.at(absum, owner[live], np.abs(terms[live]))
        base = vertex_classes(flat, vs, D, edges, sizes)
        Theta, A, L, S = S8[:, 0], S8[:, 1], S8[:, 2:5], S8[:, 5:8]
        ok = _usable(A)
        tau = np.where(base == BOUNDARY, PI, TWO_PI)
        defect = np.where(base == ISOLATED, 0.0, tau - Theta)
        four = 4.0 * A
        ls = _norm(S)
        H = np.where(_usable(ls), _dot(L, S) / (ls * four), _norm(L) / four)
        K = defect / A
        Hn = L / four[:, None]
        cls = (base | np.where(ok, 0, DEGENERATE)).astype(np.uint32)
        f32 = lambda x, keep: np.where(keep, x, 0.0).astype(np.float32)
        dec = {"vertex_class": cls, "vertex_area": f32(A, ok), "angle_defect": defect.astype(np.float32), "gaussian": f32(K, ok),
               "mean_normal": f32(Hn, ok[:, None]), "mean": f32(H, ok)}
        # ---- the scales
        s_theta = np.where(base == ISOLATED, 0.0, tau + absum[:, 0])
        s_L = absum[:, 2:5]
        s_H = np.where(_usable(ls), s_L.sum(axis=1) * absum[:, 5:8].sum(axis=1) / (ls * np.abs(four)), s_L.sum(axis=1) / np.abs(four))
        zero = lambda x, keep: np.where(keep, x, 0.0)   # (a row written as +0 has nothing behind it)
        scale = {"vertex_area": zero(absum[:, 1], ok), "angle_defect": s_theta, "gaussian": zero(s_theta / np.abs(A), ok),
                 "mean_normal": zero(s_L / np.abs(four)[:, None], ok[:, None]), "mean": zero(s_H, ok)}
        livev = (base != ISOLATED) & ok
        rows = np.where(livev[:, None], np.stack([A, defect, H * A], axis=1), 0.0)
        totals = fold(rows)
        tscale = np.where(livev[:, None], np.stack([absum[:, 1], s_theta, s_H * np.abs(A)], axis=1), 0.0).sum(axis=0)
    out = {name: np.ascontiguousarray(dec[name][vs]) for name in BUFFERS}
    out["scale"] = {name: scale[name][vs] for name in FLOATS}
    out["scale"]["totals"] = tscale
    out["totals"] = totals
    low = cls & 7
    out["summary"] = (D, int((low == INTERIOR).sum()), int((low == BOUNDARY).sum()), int((low == IRREGULAR).sum()), int((low == ISOLATED).sum()),
                      int((cls & DEGENERATE != 0).sum()))
    out["decoded"] = {"Theta": Theta, "A": A, "L": L, "S": S, "defect": defect, "H": H, "class": cls, "slots": sizes, "scale_L": s_L, "scale_theta": s_theta,
                      "scale_A": absum[:, 1]}
    out["branch"] = np.where(live, branch, -1)
    out["slot_area"] = np.where(live, terms[:, 1], 0.0)
    out["tri_area"] = 0.5 * _norm(_cross(P[I[:, 1]] - P[I[:, 0]], P[I[:, 2]] - P[I[:, 0]]))
    return out


def of_arrays(positions, degrees, corners, vertex_source=None):
    """the restatement of a mesh in the PLY layout: the fan of shells_ref.fan, vertex_source the identity unless given"""
    from tests import shells_ref as sr
    I, _ = sr.fan(degrees, corners)
    pos = np.asarray(positions, np.float32)
    return build(I, np.arange(len(pos)) if vertex_source is None else vertex_source, pos, len(pos))


def of_mesh(m):
    """the same for a meshgen mesh (fields x, y, z)"""
    return of_arrays(np.stack([m.verts["x"], m.verts["y"], m.verts["z"]], axis=1), m.degrees, m.indices)


def from_render(rn, positions, nv):
    """the restatement from a render build's host arrays (Codec.render_numpy), the float rows of its positions and the mesh's nv"""
    return build(rn["indices"], rn["vertex_source"], positions, nv)


def bound(want, scale):
    """the tolerance of a comparison: one float32 step of want + 2^-40 * scale; of doubles (the totals, which are not rounded to
    float32): 2^-40 * scale alone"""
    w = np.asarray(want)
    if w.dtype == np.float64:
        return EPS * np.asarray(scale, np.float64)
    with np.errstate(all="ignore"):
        step = np.abs(np.spacing(w.astype(np.float32))).astype(np.float64)
    return np.where(np.isfinite(w), step, 0.0) + EPS * np.asarray(scale, np.float64)


def compare(got, want, scale, label):
    """asserts |got - want| <= bound, values that are not finite being equal; prints and returns (values not bit-equal, the largest
    difference in units of the bound)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, want.shape, got.dtype, want.dtype)
    finite = np.isfinite(want)
    assert np.array_equal(got[~finite], want[~finite], equal_nan=True), (label, "values that are not finite differ")
    b = np.broadcast_to(bound(want, scale), want.shape)
    diff = np.abs(got[finite].astype(np.float64) - want[finite].astype(np.float64))
    with np.errstate(all="ignore"):
        units = float(np.max(np.where(diff == 0, 0.0, diff / b[finite]))) if diff.size else 0.0
    view = np.uint32 if want.dtype == np.float32 else np.uint64
    differ = int((np.ascontiguousarray(got).view(view) != np.ascontiguousarray(want).view(view)).sum())
    print("CURVATURE", label, "values not bit-equal:", differ, "of", want.size, "largest difference in units of the bound:", units)
    assert np.isfinite(got[finite]).all() and units <= 1.0, (label, units)
    return differ, units
