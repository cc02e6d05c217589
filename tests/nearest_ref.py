"""The numpy restatement of hry_bvh_nearest (include/harry_amd.h): the closest point of the hierarchy's triangles to every query
point, as a brute force of every point against every leaf -- the candidates of the triangle, the clamp by the bound of its own leaf
box, the least with ties to the least triangle number.  Nothing here walks a tree to answer a point but `walk`, the reference stack
walk the CPU tests compare with the brute force and count bound evaluations with; it is written in plain Python floats (IEEE
doubles, one rounding an operation), a second statement of the same rules.  Every floating-point operation is a double operation of
its own, in the order the contract writes them, so the device must agree bit for bit.  The hierarchy itself is tests/bvh_ref.py's."""
import numpy as np

from tests import bvh_ref as br
from tests.bvh_ref import LEAF, NO_ELEMENT, cross, dot


def valid_points(Q):
    return np.isfinite(Q).all(axis=1)


def bound(box, Q):
    """box f32 [m, 6] against points Q f64 [n, 3] -> b2 [n, m]: the one rule, for leaf and node boxes alike"""
    lo, hi = box[None, :, :3].astype(np.float64), box[None, :, 3:].astype(np.float64)
    q = Q[:, None, :]
    g = np.maximum(np.maximum(lo - q, q - hi), 0.0)
    return (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]


def clamp01(s):
    return np.where(s < 0, 0.0, np.where(s > 1, 1.0, s))   # (a NaN stays one)


def segment(A, B, Q):
    d = B - A
    l = dot(d, d)
    with np.errstate(all="ignore"):
        return np.where(l == 0, 0.0, clamp01(dot(Q - A, d) / np.where(l == 0, 1.0, l)))


def candidates(leaf_positions, Q):
    """the four candidates of every (point, leaf), in the contract's order: a list of (is a candidate, u, v) [n, m], and the
    triangles' P0, e1, e2 [1, m, 3]"""
    P = leaf_positions.astype(np.float64).reshape(1, -1, 3, 3)
    P0, P1, P2 = P[:, :, 0], P[:, :, 1], P[:, :, 2]
    q = Q[:, None, :]
    e1, e2, s = P1 - P0, P2 - P0, q - P0
    n = cross(e1, e2)
    nn = dot(n, n)
    with np.errstate(all="ignore"):
        safe = np.where(nn > 0, nn, 1.0)
        u, v = dot(cross(s, e2), n) / safe, dot(cross(e1, s), n) / safe
        face = (nn > 0) & (u >= 0) & (v >= 0) & (u + v <= 1)
    sb, sc, sd = segment(P0, P1, q), segment(P1, P2, q), segment(P2, P0, q)
    always, zero = np.ones(sb.shape, bool), np.zeros(sb.shape)
    return [(face, u, v), (always, sb, zero), (always, 1.0 - sc, sc), (always, zero, 1.0 - sd)], (P0, e1, e2)


def triangle(leaf_positions, leaf_box, Q):
    """every (point, leaf): (d2_t, u, v, C) [n, m] (C [n, m, 3]) -- the first candidate with the least d2, clamped from below by the
    bound of the leaf's own box"""
    cands, (P0, e1, e2) = candidates(leaf_positions, Q)
    q = Q[:, None, :]
    shape = cands[1][1].shape
    best, bu, bv, bc = np.full(shape, np.inf), np.zeros(shape), np.zeros(shape), np.zeros(shape + (3,))
    for ok, u, v in cands:
        with np.errstate(all="ignore"):
            c = P0 + (u[..., None] * e1 + v[..., None] * e2)
            d2 = dot(q - c, q - c)
            take = ok & (d2 < best)
        best, bu, bv, bc = np.where(take, d2, best), np.where(take, u, bu), np.where(take, v, bv), np.where(take[..., None], c, bc)
    b2 = bound(leaf_box, Q)
    return np.where(b2 > best, b2, best), bu, bv, bc


def nearest(bvh, points, max_dist=np.inf, chunk=256):
    """every point against every leaf -> {"tri" u32 [n], "d2" f64 [n], "uv" f32 [n, 2], "point" f32 [n, 3], "answered", "max_bits":
    the third stat word}"""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    n, L = len(points), len(bvh["leaf_tri"])
    tri, d2 = np.full(n, NO_ELEMENT, np.uint32), np.full(n, np.inf, np.float64)
    uv, point = np.zeros((n, 2), np.float32), np.zeros((n, 3), np.float32)
    r2 = np.float64(max_dist) * np.float64(max_dist)
    good = np.flatnonzero(valid_points(points)) if L and not max_dist < 0 else np.zeros(0, np.int64)
    numbers = bvh["leaf_tri"][None, :].astype(np.int64)
    for at in range(0, len(good), chunk):
        rows = good[at:at + chunk]
        Q = points[rows].astype(np.float64)
        dt, u, v, c = triangle(bvh["leaf_positions"], bvh["leaf_box"], Q)
        ok = dt <= r2
        dt = np.where(ok, dt, np.inf)
        least = dt.min(axis=1)
        leaf = np.where(ok & (dt == least[:, None]), numbers, 1 << 40).argmin(axis=1)
        hit = ok.any(axis=1)
        k = np.arange(len(rows))
        tri[rows[hit]] = bvh["leaf_tri"][leaf[hit]]
        d2[rows[hit]] = dt[k, leaf][hit]
        uv[rows[hit]] = np.stack([u[k, leaf], v[k, leaf]], axis=1)[hit].astype(np.float32)
        with np.errstate(over="ignore"):
            point[rows[hit]] = c[k, leaf][hit].astype(np.float32)
    answered = tri != NO_ELEMENT
    return {"tri": tri, "d2": d2, "uv": uv, "point": point, "answered": int(answered.sum()),
            "max_bits": int(d2[answered].max().view(np.uint64)) if answered.any() else 0}


# ---- the reference walk, in plain Python floats
def _bound(box, q):
    b = []
    for k in range(3):
        a, c = box[k] - q[k], q[k] - box[3 + k]
        g = a if a > c else c
        b.append(g if g > 0.0 else 0.0)
    return (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _segment(a, b, q):
    d = _sub(b, a)
    l = _dot(d, d)
    if l == 0.0:
        return 0.0
    s = _dot(_sub(q, a), d) / l
    return 0.0 if s < 0.0 else 1.0 if s > 1.0 else s


def _triangle(p, box, q):
    """(d2_t, u, v, C) of one triangle (nine floats) whose leaf box is `box`"""
    p0, p1, p2 = p[0:3], p[3:6], p[6:9]
    e1, e2, s = _sub(p1, p0), _sub(p2, p0), _sub(q, p0)
    n = _cross(e1, e2)
    nn = _dot(n, n)
    cands = []
    if nn > 0.0:
        u, v = _dot(_cross(s, e2), n) / nn, _dot(_cross(e1, s), n) / nn
        if u >= 0.0 and v >= 0.0 and u + v <= 1.0:
            cands.append((u, v))
    sb, sc, sd = _segment(p0, p1, q), _segment(p1, p2, q), _segment(p2, p0, q)
    cands += [(sb, 0.0), (1.0 - sc, sc), (0.0, 1.0 - sd)]
    best = (float("inf"), 0.0, 0.0, (0.0, 0.0, 0.0))
    for u, v in cands:
        c = tuple(p0[k] + (u * e1[k] + v * e2[k]) for k in range(3))
        r = _sub(q, c)
        d2 = _dot(r, r)
        if d2 < best[0]:
            best = (d2, u, v, c)
    b2 = _bound(box, q)
    return (b2 if b2 > best[0] else best[0],) + best[1:]


def walk(bvh, point, max_dist=np.inf):
    """one point down the tree with a stack, the nearer child first, skipping what has a bound strictly greater than the best d2_t
    so far -> (tri, d2, u, v, C, bounds evaluated)"""
    q = tuple(float(x) for x in np.asarray(point, np.float32))
    L = len(bvh["leaf_tri"])
    none = (NO_ELEMENT, np.float64(np.inf), np.float32(0), np.float32(0), np.zeros(3, np.float32), 0)
    if not L or not all(np.isfinite(q)) or max_dist < 0:
        return none
    lists = bvh.get("_lists")   # (the buffers as Python lists, made once a hierarchy)
    if lists is None:
        lists = bvh["_lists"] = tuple(bvh[k].astype(np.float64).tolist() if bvh[k].dtype == np.float32 else bvh[k].tolist()
                                          for k in ("leaf_positions", "leaf_box", "node_box", "node_children", "leaf_tri"))
    leaf_positions, leaf_box, node_box, children, leaf_tri = lists
    r2 = float(max_dist) * float(max_dist)
    best, tests = (r2, NO_ELEMENT, 0.0, 0.0, (0.0, 0.0, 0.0)), 0

    def leaf(i):
        nonlocal best
        d2, u, v, c = _triangle(leaf_positions[i], leaf_box[i], q)
        t = leaf_tri[i]
        if d2 < best[0] or (d2 == best[0] and t < best[1]):
            best = (d2, t, u, v, c)

    if L == 1:
        tests += 1
        if not _bound(leaf_box[0], q) > best[0]:
            leaf(0)
    stack = [(0, 0.0)] if L > 1 else []
    deepest = 0
    while stack:
        deepest = max(deepest, len(stack))
        node, b2 = stack.pop()
        if b2 > best[0]:
            continue
        kids = []
        for c in children[node]:
            n = c & ~LEAF
            tests += 1
            b2 = _bound((leaf_box if c & LEAF else node_box)[n], q)
            if not b2 > best[0]:
                if c & LEAF:
                    leaf(n)
                else:
                    kids.append((n, b2))
        kids = [k for k in kids if not k[1] > best[0]]
        if len(kids) == 2 and kids[1][1] < kids[0][1]:
            kids.reverse()   # the nearer one is pushed last: on top
        stack.extend(reversed(kids))
    assert deepest <= 64
    if best[1] == NO_ELEMENT:
        return none[:5] + (tests,)
    with np.errstate(over="ignore"):
        return (best[1], np.float64(best[0]), np.float32(best[2]), np.float32(best[3]), np.array(best[4], np.float64).astype(np.float32), tests)


def point_set(bvh, n, seed):
    """n points about the hierarchy's scene, float32 [n, 3], in four quarters: random in the scene box grown by a half; exactly at
    corners of leaves (the distance is 0 and several triangles tie); midpoints of leaf edges; points on faces displaced by
    N(0, 0.05)"""
    rng = np.random.default_rng(seed)
    L = len(bvh["leaf_tri"])
    box = bvh["scene_box"][0].astype(np.float64) if L else np.array([0.0, 0, 0, 1, 1, 1])
    lo, hi = box[:3], box[3:]
    mid, half = (lo + hi) / 2, np.maximum((hi - lo) / 2, 1e-3)
    tris = bvh["leaf_positions"].reshape(-1, 3, 3).astype(np.float64) if L else np.zeros((1, 3, 3))
    quarter = n // 4
    a = mid + 1.5 * half * rng.uniform(-1, 1, (quarter, 3))
    b = tris[rng.integers(0, len(tris), quarter), rng.integers(0, 3, quarter)]
    t, k = rng.integers(0, len(tris), quarter), rng.integers(0, 3, quarter)
    c = (tris[t, k] + tris[t, (k + 1) % 3]) / 2
    rest = n - 3 * quarter
    t, w = rng.integers(0, len(tris), rest), rng.dirichlet([1, 1, 1], rest)
    d = (tris[t] * w[:, :, None]).sum(axis=1) + rng.normal(0, 0.05, (rest, 3))
    return np.concatenate([a, b, c, d]).astype(np.float32)
