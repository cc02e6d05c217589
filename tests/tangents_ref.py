"""A numpy float64 restatement of the tangents contract of include/harry_amd.h (hry_tangents_build): every operation is an
individually rounded double operation in the written order; a vertex's sums run over its index slots in ascending slot, starting from
+0 (in rounds: round r adds the r-th slot of every vertex that has one).  Results are rounded to float32 once.

Tolerance of a comparison against the device, by the argument of tests/normals_ref.py: both sides evaluate in double and round to
float once; they differ by the association of the sums of hubs (vertices with more than 32 slots, which the device sums in 256
ranges) and by a last place in sqrt, the division and atan2 -- relative errors of order 2^-50 before the rounding, so a component is
the same float or its neighbour, and with |component| <= 1 for t and for w (n x t) neighbours are at most 2^-24 apart: TOL.
That holds only where nothing cancels.  `guard[u]` is true where all three hold:
    |S_T| >= 2^-20 * sum |T terms|,   |R| >= 2^-20 * |S_T|,   |(n x t) . S_B| >= 2^-20 * sum |B terms|   (the last for w);
a test compares guarded vertices only, and asserts that the guard excluded none.  w is expected equal exactly, and so are the
summary's counts."""
import numpy as np

TOL = 2.0 ** -24


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _length(a):
    return np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])


def _usable(n):
    return (n > 0) & np.isfinite(n)


def tangents(pos, uv, nrm, indices, weights="area"):
    """pos f32 [U, 3], uv f32 [U, 2], nrm f32 [U, 3]: what the render build holds per output vertex; indices: its triangles [T, 3].
    Returns a dict: tangents f32 [U, 4], bitangents f32 [U, 3], guard bool [U], summary (framed, unframed, mirrored, mixed,
    degenerate), mixed bool [U], degenerate bool [T]."""
    assert weights in ("area", "angle")
    with np.errstate(all="ignore"):
        P = np.asarray(pos, np.float32).astype(np.float64).reshape(-1, 3)
        Q = np.asarray(uv, np.float32).astype(np.float64).reshape(-1, 2)
        N = np.asarray(nrm, np.float32).astype(np.float64).reshape(-1, 3)
        I = np.asarray(indices).astype(np.int64).reshape(-1, 3)
        U, T = len(P), len(I)
        i0, i1, i2 = I[:, 0], I[:, 1], I[:, 2]
        # ---- per triangle
        e1, e2 = P[i1] - P[i0], P[i2] - P[i0]
        a1, b1 = Q[i1, 0] - Q[i0, 0], Q[i1, 1] - Q[i0, 1]
        a2, b2 = Q[i2, 0] - Q[i0, 0], Q[i2, 1] - Q[i0, 1]
        det = a1 * b2 - a2 * b1
        Tr = e1 * b2[:, None] - e2 * b1[:, None]
        Br = e2 * a1[:, None] - e1 * a2[:, None]
        neg = det < 0
        Tr[neg] = -Tr[neg]
        Br[neg] = -Br[neg]
        ok = (det != 0) & np.isfinite(det) & np.isfinite(Tr).all(axis=1) & np.isfinite(Br).all(axis=1)
        lt, lb = _length(Tr), _length(Br)
        if weights == "angle":
            ok &= (lt != 0) & (lb != 0)
            Tr, Br = Tr / lt[:, None], Br / lb[:, None]
        # ---- per slot s = 3 t + k
        tri = np.repeat(np.arange(T), 3)
        k = np.tile(np.arange(3), T)
        own = I.reshape(-1)
        if weights == "area":
            wgt = np.ones(3 * T)
            mag_t, mag_b = lt[tri], lb[tri]
        else:
            p = P[own]
            a, b = P[I[tri, (k + 1) % 3]] - p, P[I[tri, (k + 2) % 3]] - p
            wgt = np.arctan2(_length(_cross(a, b)), _dot(a, b))
            mag_t = mag_b = np.abs(wgt)
        live = ok[tri]
        term_t = np.where(live[:, None], Tr[tri] if weights == "area" else wgt[:, None] * Tr[tri], 0.0)
        term_b = np.where(live[:, None], Br[tri] if weights == "area" else wgt[:, None] * Br[tri], 0.0)
        mag_t, mag_b = np.where(live, mag_t, 0.0), np.where(live, mag_b, 0.0)
        # ---- the sums: ascending slot, one after the other (round r adds the r-th slot of every vertex that has one)
        S_T, S_B, A_T, A_B = np.zeros((U, 3)), np.zeros((U, 3)), np.zeros(U), np.zeros(U)
        terms, pos_sign, neg_sign = np.zeros(U, np.int64), np.zeros(U, bool), np.zeros(U, bool)
        order = np.argsort(own, kind="stable")
        ov = own[order]
        first = np.concatenate([[0], np.cumsum(np.bincount(ov, minlength=U))])[:-1]
        rank = np.arange(len(ov)) - first[ov]
        by_rank = np.argsort(rank, kind="stable")
        cuts = np.concatenate([[0], np.cumsum(np.bincount(rank, minlength=1))])
        for r in range(len(cuts) - 1):
            sel = by_rank[cuts[r]:cuts[r + 1]]
            sel = sel[live[order[sel]]]   # (a uv-degenerate triangle adds nothing: not even +0 to a -0)
            u, s = ov[sel], order[sel]
            S_T[u] += term_t[s]
            S_B[u] += term_b[s]
            A_T[u] += mag_t[s]
            A_B[u] += mag_b[s]
            terms[u] += 1
            pos_sign[u] |= ~neg[tri[s]]
            neg_sign[u] |= neg[tri[s]]
        # ---- per output vertex
        nl = _length(N)
        n = N / nl[:, None]
        d = _dot(n, S_T)
        R = S_T - n * d[:, None]
        rl = _length(R)
        framed = (terms > 0) & _usable(nl) & _usable(rl)
        t = R / rl[:, None]
        c = _cross(n, t)
        h = _dot(c, S_B)
        w = np.where(h < 0, -1.0, 1.0)
        tan = np.zeros((U, 4), np.float32)
        tan[framed, :3] = t[framed].astype(np.float32)
        tan[framed, 3] = w[framed].astype(np.float32)
        bit = np.zeros((U, 3), np.float32)
        bit[framed] = (w[framed][:, None] * c[framed]).astype(np.float32)
        lim = 2.0 ** -20
        guard = ~framed | (~(_length(S_T) < lim * A_T) & ~(rl < lim * _length(S_T)) & ~(np.abs(h) < lim * A_B))
        mixed = pos_sign & neg_sign
        summary = (int(framed.sum()), int(U - framed.sum()), int((framed & (w < 0)).sum()), int(mixed.sum()), int((~ok).sum()))
        return {"tangents": tan, "bitangents": bit, "guard": guard, "summary": summary, "mixed": mixed, "degenerate": ~ok}
