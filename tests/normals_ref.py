"""A numpy float64 restatement of the normals contract of include/harry_amd.h (hry_render_build_ex): every operation is an
individually rounded double operation in the written order; a vertex's sum runs over its corners in ascending half-edge id, starting
from +0.  Results are rounded to float32 once.

Tolerance of a comparison against the device: both sides evaluate in double and round to float once; they differ by the association of
the sums of hubs (vertices with more than 32 corners) and by a last place in sqrt / atan2 -- relative errors of order 2^-50 before the
rounding, so a component is the same float or its neighbour, and with |component| <= 1 neighbours are at most 2^-24 apart: TOL.
That holds only where the sum does not cancel: `guard[v]` says |S_v| >= 2^-20 * sum |terms|, and a test compares guarded vertices only
(and asserts how many the guard excluded)."""
import numpy as np

TOL = 2.0 ** -24


def positions_of(verts) -> np.ndarray:
    """float32 [nv, 3] from a structured vertex array with fields x, y, z"""
    return np.stack([np.asarray(verts[k], np.float32) for k in "xyz"], axis=1)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _length(a):
    return np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])


def _usable(n):
    return (n > 0) & np.isfinite(n)


def _unit32(s):
    n = _length(s)
    ok = _usable(n)
    out = np.zeros(s.shape, np.float32)
    out[ok] = (s[ok] / n[ok][:, None]).astype(np.float32)
    return out


def normals(pos, degrees, indices, mode="area"):
    """pos: float32 [nv, 3] (what the build's list buffer holds); degrees u8 [nf]; indices: the flattened corners.
    Returns (face_normals f32 [nf, 3], normals f32 [nv, 3], guard bool [nv])."""
    assert mode in ("area", "angle")
    with np.errstate(all="ignore"):
        P = np.asarray(pos, np.float32).astype(np.float64)
        nv = len(P)
        deg = np.asarray(degrees).astype(np.int64)
        org = np.asarray(indices).astype(np.int64)
        nf = len(deg)
        off = np.concatenate([[0], np.cumsum(deg)])
        lo = off[:-1]
        # ---- N_f: the fan triangles' cross products relative to corner 0, in order
        N = np.zeros((nf, 3))
        if nf:
            p0 = P[org[lo]]
            for k in range(1, int(deg.max()) - 1):
                sel = np.nonzero(deg > k + 1)[0]
                t = _cross(P[org[lo[sel] + k]] - p0[sel], P[org[lo[sel] + k + 1]] - p0[sel])
                N[sel] = t if k == 1 else N[sel] + t
        flen = _length(N)
        fok = _usable(flen)
        unit = np.zeros((nf, 3))
        unit[fok] = N[fok] / flen[fok][:, None]
        face_normals = unit.astype(np.float32)
        # ---- per corner: its face's contribution
        face = np.repeat(np.arange(nf), deg)
        if mode == "area":
            term = np.where(fok[face][:, None], N[face], 0.0)
            mag = np.where(fok[face], flen[face], 0.0)
        else:
            c = np.arange(len(org))
            nxt = np.where(c + 1 == off[1:][face], lo[face], c + 1)
            prv = np.where(c == lo[face], off[1:][face] - 1, c - 1)
            a, b = P[org[nxt]] - P[org], P[org[prv]] - P[org]
            theta = np.arctan2(_length(_cross(a, b)), (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2])
            term = np.where(fok[face][:, None], theta[:, None] * unit[face], 0.0)
            mag = np.where(fok[face], np.abs(theta), 0.0)
        # ---- S_v: ascending corner id, one after the other (round r adds the r-th corner of every vertex that has one)
        S = np.zeros((nv, 3))
        A = np.zeros(nv)
        order = np.argsort(org, kind="stable")
        ov = org[order]
        first = np.concatenate([[0], np.cumsum(np.bincount(ov, minlength=nv))])[:-1]
        rank = np.arange(len(ov)) - first[ov]
        by_rank = np.argsort(rank, kind="stable")
        cuts = np.concatenate([[0], np.cumsum(np.bincount(rank, minlength=1))])
        for r in range(len(cuts) - 1):
            sel = by_rank[cuts[r]:cuts[r + 1]]
            S[ov[sel]] += term[order[sel]]
            A[ov[sel]] += mag[order[sel]]
        guard = ~(_length(S) < 2.0 ** -20 * A)
        return face_normals, _unit32(S), guard


def of_mesh(m, mode="area"):
    """the same for a meshgen mesh (fields x, y, z)"""
    return normals(positions_of(m.verts), m.degrees, m.indices, mode)
