"""numpy restatement of hry_shells_build (include/harry_amd.h) from the output of edges_ref.build: a plain union-find over the triangles
along the edges' side lists, shells numbered by their lowest triangle, the per-shell counts, the loops rule (boundary edges of one
shell joined where they share a decoded vertex) and -- from the float32 position rows -- area, signed volume and box in float64 with
exactly the association the header writes: per chunk of 256 triangles a partial from +0 in ascending t, then the chunks' partials from
+0 in ascending chunk."""
from __future__ import annotations

import numpy as np

from tests import edges_ref as er

FIXED = ("tri_shell", "face_shell", "edge_shell", "shell_first", "shell_counts")
GEOMETRY = ("shell_measures",)
COLUMNS = ("triangles", "faces", "vertices", "edges", "boundary", "nonmanifold", "misoriented", "loops")
CHUNK = 256


class _UnionFind:
    def __init__(self, n):
        self.p = list(range(n))

    def find(self, x):
        p = self.p
        while p[x] != x:
            p[x] = p[p[x]]
            x = p[x]
        return x

    def unite(self, a, b):
        a, b = self.find(a), self.find(b)
        if a != b:
            self.p[max(a, b)] = min(a, b)   # the root is the smallest member


def _float_key(x):
    """float32 -> uint32 in the floats' order, -0 below +0"""
    b = np.asarray(x, np.float32).view(np.uint32)
    return np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)


def build(indices, vertex_source, tri_face, nf, edges, positions=None) -> dict:
    """indices u32 [T, 3], vertex_source u32 [U], tri_face u32 [T], nf, edges = edges_ref.build(indices, vertex_source), positions
    f32 [U, 3] or None -> the buffers of hry_shells_build by name, plus "summary" = (S, closed, nonmanifold, misoriented, loops, largest)"""
    I = np.asarray(indices, np.int64).reshape(-1, 3)
    vs = np.asarray(vertex_source, np.int64)
    tf = np.asarray(tri_face, np.int64)
    T = len(I)
    off, sides = edges["edge_offsets"].astype(np.int64), edges["edge_sides"].astype(np.int64)
    E = len(off) - 1
    lens = np.diff(off)
    uf = _UnionFind(T)
    for e in range(E):
        first = sides[off[e]]
        for s in sides[off[e] + 1:off[e + 1]]:
            uf.unite(int(s) // 3, int(first) // 3)
    root = np.array([uf.find(t) for t in range(T)], np.int64)
    firsts = np.flatnonzero(root == np.arange(T))                      # ascending: shells by their lowest triangle
    S = len(firsts)
    number = np.full(T + 1, -1, np.int64)
    number[firsts] = np.arange(S)
    tri_shell = number[root] if T else np.zeros(0, np.int64)
    face_shell = np.full(nf if T else 0, er.NO_ELEMENT, np.int64)
    face_shell[tf] = tri_shell
    edge_shell = tri_shell[sides[off[:-1]] // 3] if E else np.zeros(0, np.int64)
    counts = np.zeros((S, 8), np.int64)
    counts[:, 0] = np.bincount(tri_shell, minlength=S)
    counts[:, 1] = np.bincount(face_shell[face_shell != er.NO_ELEMENT], minlength=S)
    pairs = np.unique(np.stack([np.repeat(tri_shell, 3), vs[I.reshape(-1)]], axis=1), axis=0) if T else np.zeros((0, 2), np.int64)
    counts[:, 2] = np.bincount(pairs[:, 0], minlength=S)
    counts[:, 3] = np.bincount(edge_shell, minlength=S)
    counts[:, 4] = np.bincount(edge_shell[lens == 1], minlength=S)
    counts[:, 5] = np.bincount(edge_shell[lens > 2], minlength=S)
    frm, to = vs[I.reshape(-1)], vs[I[:, [1, 2, 0]].reshape(-1)]
    two = np.flatnonzero(lens == 2)
    p, q = sides[off[two]], sides[off[two] + 1]
    counts[:, 6] = np.bincount(edge_shell[two[(frm[p] == frm[q]) & (to[p] == to[q])]], minlength=S)
    # loops: the boundary edges of a shell, joined where two of them share a decoded vertex
    boundary = np.flatnonzero(lens == 1)
    lf = _UnionFind(E)
    seen = {}
    for e in boundary:
        s = sides[off[e]]
        for vtx in (frm[s], to[s]):
            k = (int(edge_shell[e]), int(vtx))
            if k in seen:
                lf.unite(int(e), seen[k])
            else:
                seen[k] = int(e)
    loop_roots = [e for e in boundary if lf.find(int(e)) == e]
    counts[:, 7] = np.bincount(edge_shell[loop_roots], minlength=S) if len(loop_roots) else 0
    out = {
        "tri_shell": tri_shell.astype(np.uint32), "face_shell": face_shell.astype(np.uint32), "edge_shell": edge_shell.astype(np.uint32),
        "shell_first": firsts.astype(np.uint32), "shell_counts": counts.astype(np.uint32),
        "summary": (S, int(((counts[:, 4] == 0) & (counts[:, 5] == 0)).sum()), int((counts[:, 5] > 0).sum()), int((counts[:, 6] > 0).sum()),
                    int(counts[:, 7].sum()), int(counts[:, 0].max()) if S else 0),
    }
    if positions is None:
        return out
    P32 = np.asarray(positions, np.float32)[:, :3]
    P = P32.astype(np.float64)
    M = np.zeros((S, 8), np.float32)
    with np.errstate(all="ignore"):
        p0, p1, p2 = P[I[:, 0]], P[I[:, 1]], P[I[:, 2]]
        area = er._norm(er._cross(p1 - p0, p2 - p0))
        area = np.where(np.isfinite(area), area, 0.0)
        O = P[I[firsts[tri_shell], 0]] if T else np.zeros((0, 3))
        vol = er._dot(p0 - O, er._cross(p1 - O, p2 - O))
        vol = np.where(np.isfinite(vol), vol, 0.0)
        A, V = np.zeros(S, np.float64), np.zeros(S, np.float64)
        for c in range(0, T, CHUNK):                                   # strictly in the order of the contract
            pa, pv = {}, {}
            for t in range(c, min(c + CHUNK, T)):
                s = int(tri_shell[t])
                pa[s] = pa.get(s, np.float64(0.0)) + area[t]
                pv[s] = pv.get(s, np.float64(0.0)) + vol[t]
            for s in pa:
                A[s] = A[s] + pa[s]
                V[s] = V[s] + pv[s]
        M[:, 0] = (0.5 * A).astype(np.float32)
        M[:, 1] = (V / 6.0).astype(np.float32)
    key = _float_key(P32)
    finite = np.isfinite(P32)
    corner_shell = np.repeat(tri_shell, 3)
    corner = I.reshape(-1)
    for k in range(3):
        lo, hi = np.full(S, 0xFFFFFFFF, np.uint32), np.zeros(S, np.uint32)
        ok = finite[corner, k]
        np.minimum.at(lo, corner_shell[ok], key[corner[ok], k])
        np.maximum.at(hi, corner_shell[ok], key[corner[ok], k])
        unkey = lambda x: np.where(x & 0x80000000, x & 0x7FFFFFFF, ~x).astype(np.uint32).view(np.float32)
        M[:, 2 + k] = np.where(lo == 0xFFFFFFFF, np.float32(np.inf), unkey(lo))
        M[:, 5 + k] = np.where(hi == 0, np.float32(-np.inf), unkey(hi))
    out["shell_measures"] = M
    return out


def fan(degrees, indices):
    """the fan triangulation of a render build, on the host: (indices [T, 3], tri_face [T]); triangle k of a face joins its corners
    0, k + 1, k + 2"""
    deg = np.asarray(degrees, np.int64)
    idx = np.asarray(indices, np.int64)
    start = np.concatenate([[0], np.cumsum(deg)])[:-1]
    tri_face = np.repeat(np.arange(len(deg)), deg - 2)
    k = np.arange(len(tri_face)) - np.repeat(np.cumsum(deg - 2) - (deg - 2), deg - 2)
    c0 = start[tri_face]
    return np.stack([idx[c0], idx[c0 + k + 1], idx[c0 + k + 2]], axis=1), tri_face


def of_mesh(m, geometry=True):
    """the restatement of a meshgen mesh in the PLY layout (vertex_source is the identity)"""
    I, tf = fan(m.degrees, m.indices)
    vs = np.arange(len(m.verts))
    pos = np.stack([m.verts["x"], m.verts["y"], m.verts["z"]], axis=1).astype(np.float32)
    return build(I, vs, tf, len(m.degrees), er.build(I, vs), pos if geometry else None)


def from_render(rn, nf, positions=None, geometry=True):
    """the restatement from a render build's host arrays (Codec.render_numpy) and the mesh's face count"""
    e = er.build(rn["indices"], rn["vertex_source"])
    return build(rn["indices"], rn["vertex_source"], rn["tri_face"], nf, e, positions if geometry else None)


def euler(row) -> int:
    return int(row[2]) - int(row[3]) + int(row[0])


def genus(row):
    """(2 - euler - loops) / 2 where the row has no non-manifold and no misoriented edge, else None"""
    if row[5] or row[6]:
        return None
    return (2 - euler(row) - int(row[7])) // 2
