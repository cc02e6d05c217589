"""numpy / pure-Python restatement of hry_orient_build (include/harry_amd.h) from the output of edges_ref.build: the relations (joining
edges, along or against; consecutive fan triangles of one face, along), a sequential breadth-first pass over them that carries the
parity of the flips and notices a contradiction, patches numbered by their lowest triangle, the majority and outward rules, the
per-patch counts.  patch_measures comes from shells_ref.build over oriented_indices, with the patches handed to it as the sets its
union-find joins: the same float64 sums in the same order."""
from __future__ import annotations

from collections import deque

import numpy as np

from tests import edges_ref as er
from tests import shells_ref as sr

FIXED = ("tri_patch", "tri_flip", "face_flip", "oriented_indices", "patch_first", "patch_counts")
OUTWARD = ("patch_measures",)
COLUMNS = ("triangles", "faces", "flipped", "flipped_faces", "against", "open", "orientable", "inverted")
SUMMARY = ("patches", "orientable", "flipped", "inverted", "against", "remaining")


def relations(indices, vertex_source, tri_face, edges):
    """-> (list of (t0, t1, against), joining [3 T] bool: the side's edge is a joining edge, how many relations -- the first ones -- come
    from an edge)"""
    I = np.asarray(indices, np.int64).reshape(-1, 3)
    vs = np.asarray(vertex_source, np.int64)
    tf = np.asarray(tri_face, np.int64)
    T = len(I)
    off, sides = edges["edge_offsets"].astype(np.int64), edges["edge_sides"].astype(np.int64)
    frm, to = vs[I.reshape(-1)], vs[I[:, [1, 2, 0]].reshape(-1)]
    joining = np.zeros(3 * T, bool)
    rel = []
    for e in range(len(off) - 1):
        if off[e + 1] - off[e] != 2:
            continue
        s0, s1 = int(sides[off[e]]), int(sides[off[e] + 1])
        if s0 // 3 == s1 // 3 or frm[s0] == to[s0]:
            continue
        joining[s0] = joining[s1] = True
        rel.append((s0 // 3, s1 // 3, bool(frm[s0] == frm[s1] and to[s0] == to[s1])))
    n_edge = len(rel)
    for t in range(T - 1):
        if tf[t] == tf[t + 1]:
            rel.append((t, t + 1, False))
    return rel, joining, n_edge


def analyse(indices, vertex_source, tri_face, edges):
    """the part of build() that no flag changes: the relations and the breadth-first pass -- (relations, joining, relations from edges,
    tri_patch, relative flips, patch_first, orientable)"""
    I = np.asarray(indices, np.int64).reshape(-1, 3)
    tf = np.asarray(tri_face, np.int64)
    T = len(I)
    rel, joining, n_edge = relations(I, vertex_source, tf, edges)
    adj = [[] for _ in range(T)]
    for a, b, against in rel:
        adj[a].append((b, against))
        adj[b].append((a, against))
    patch = np.full(T, -1, np.int64)
    flip = np.zeros(T, np.int64)
    firsts, orientable = [], []
    for t in range(T):                                                 # ascending: patches by their lowest triangle
        if patch[t] >= 0:
            continue
        p = len(firsts)
        firsts.append(t)
        ok = True
        patch[t] = p
        queue = deque([t])
        while queue:
            a = queue.popleft()
            for b, against in adj[a]:
                want = flip[a] ^ int(against)
                if patch[b] < 0:
                    patch[b], flip[b] = p, want
                    queue.append(b)
                elif flip[b] != want:
                    ok = False
        orientable.append(ok)
    P = len(firsts)
    orientable = np.array(orientable, bool)
    firsts = np.array(firsts, np.int64)
    if T:
        flip[~orientable[patch]] = 0
    return rel, joining, n_edge, patch, flip, firsts, orientable


def build(indices, vertex_source, tri_face, nf, edges, positions=None, majority=False, outward=False, analysis=None) -> dict:
    """the buffers of hry_orient_build by name, plus "summary" = (P, orientable, flipped, inverted, against, remaining); positions f32
    [U, 3] are needed with outward; analysis: analyse() of the same arrays, where several flag combinations share it"""
    I = np.asarray(indices, np.int64).reshape(-1, 3)
    tf = np.asarray(tri_face, np.int64)
    T = len(I)
    rel, joining, n_edge, patch, flip, firsts, orientable = analysis if analysis is not None else analyse(I, vertex_source, tf, edges)
    flip = flip.copy()
    P = len(firsts)
    tris = np.bincount(patch, minlength=P) if T else np.zeros(0, np.int64)
    if majority and T:
        turn = orientable & (2 * np.bincount(patch, weights=flip, minlength=P).astype(np.int64) > tris)
        flip ^= turn[patch].astype(np.int64)
    oriented = np.where(flip[:, None] != 0, I[:, [0, 2, 1]], I)
    counts = np.zeros((P, 8), np.int64)
    counts[:, 0] = tris
    new_face = np.ones(T, bool)
    new_face[1:] = tf[1:] != tf[:-1]
    if T:
        counts[:, 1] = np.bincount(patch[new_face], minlength=P)
        counts[:, 4] = np.bincount([patch[a] for a, _, against in rel[:n_edge] if against], minlength=P)
        counts[:, 5] = np.bincount(np.repeat(patch, 3)[~joining], minlength=P)
    counts[:, 6] = orientable
    out = {}
    if outward and not T:
        out["patch_measures"] = np.zeros((0, 8), np.float32)
    elif outward:
        # the patches as the shells of shells_ref.build: one made-up edge per patch whose sides are the first sides of its triangles
        order = np.argsort(patch, kind="stable")
        fake = {"edge_offsets": np.concatenate([[0], np.cumsum(tris)]).astype(np.uint32), "edge_sides": (3 * order).astype(np.uint32)}
        s = sr.build(oriented, vertex_source, tf, nf, fake, positions)
        assert np.array_equal(s["tri_shell"], patch) and np.array_equal(s["shell_first"], firsts)
        M = s["shell_measures"].copy()
        inv = orientable & (counts[:, 5] == 0) & (M[:, 1] < 0)
        M[inv, 1] = -M[inv, 1]
        counts[:, 7] = inv
        if T:
            flip ^= inv[patch].astype(np.int64)
        oriented = np.where(flip[:, None] != 0, I[:, [0, 2, 1]], I)
        out["patch_measures"] = M
    if T:
        counts[:, 2] = np.bincount(patch, weights=flip, minlength=P).astype(np.int64)
        counts[:, 3] = np.bincount(patch[new_face], weights=flip[new_face], minlength=P).astype(np.int64)
    face_flip = np.zeros(nf if T else 0, np.int64)
    face_flip[tf] = flip
    out.update({
        "tri_patch": patch.astype(np.uint32), "tri_flip": flip.astype(np.uint32), "face_flip": face_flip.astype(np.uint32),
        "oriented_indices": oriented.astype(np.uint32).reshape(-1, 3), "patch_first": firsts.astype(np.uint32), "patch_counts": counts.astype(np.uint32),
        "summary": (P, int(orientable.sum()), int(flip.sum()), int(counts[:, 7].sum()), int(counts[:, 4].sum()), int(counts[~orientable, 4].sum())),
    })
    return out


def of_arrays(positions, degrees, indices, majority=False, outward=False):
    """the restatement of a mesh in the PLY layout (vertex_source is the identity): positions [nv, 3] or None, the faces' degrees and
    corners"""
    I, tf = sr.fan(degrees, indices)
    nv = int(np.max(indices)) + 1 if len(indices) else 0
    if positions is not None:
        nv = len(positions)
    vs = np.arange(nv)
    pos = None if positions is None else np.asarray(positions, np.float32)
    return build(I, vs, tf, len(degrees), er.build(I, vs), pos, majority, outward)


def of_mesh(m, majority=False, outward=False):
    """... of a meshgen mesh"""
    pos = np.stack([m.verts["x"], m.verts["y"], m.verts["z"]], axis=1).astype(np.float32)
    return of_arrays(pos, m.degrees, m.indices, majority, outward)


def from_render(rn, nf, positions=None):
    """the restatements from a render build's host arrays (Codec.render_numpy) and the mesh's face count: a function of (majority,
    outward); the four share one analysis"""
    e = er.build(rn["indices"], rn["vertex_source"])
    a = analyse(rn["indices"], rn["vertex_source"], rn["tri_face"], e)
    return lambda majority=False, outward=False: build(rn["indices"], rn["vertex_source"], rn["tri_face"], nf, e, positions, majority, outward, a)


def flip_faces(degrees, indices, face_flip):
    """the flip rule of hry_mesh_flip_faces on a corner array: a flagged face (v0, v1, ..., vk-1) becomes (v0, vk-1, ..., v1)"""
    out = np.array(indices).copy()
    start = 0
    for f, k in enumerate(np.asarray(degrees, np.int64)):
        if face_flip[f] and k > 1:
            out[start + 1:start + k] = out[start + 1:start + k][::-1]
        start += k
    return out


# ---- designed meshes: (positions [nv, 3], degrees, corners)
def tris_mesh(pos, tris):
    tris = np.asarray(tris, np.uint32).reshape(-1, 3)
    return np.asarray(pos, np.float32), np.full(len(tris), 3, np.uint8), tris.reshape(-1)


def turned(mesh, which):
    """the mesh with the faces `which` (indices, or a bool per face) turned by the flip rule"""
    pos, deg, idx = mesh
    flags = np.zeros(len(deg), bool)
    flags[which] = True
    return pos, deg, flip_faces(deg, idx, flags)


def random_turns(mesh, fraction=0.3, seed=5):
    """... with that fraction of the faces, chosen with a fixed seed; -> (mesh, the flags)"""
    flags = np.random.default_rng(seed).random(len(mesh[1])) < fraction
    return turned(mesh, flags), flags


TETRA_POS = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]
TETRA_TRIS = [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]             # counter-clockwise seen from outside: volume + 1 / 6


def tetra():
    return tris_mesh(TETRA_POS, TETRA_TRIS)


def two_tetrahedra():
    """two tetrahedra that share the edge 0 - 1 and nothing else: the edge has four sides"""
    pos = TETRA_POS + [[0, -1, 0], [0, 0, -1]]
    return tris_mesh(pos, TETRA_TRIS + [[0, 1, 4], [0, 5, 1], [0, 4, 5], [1, 5, 4]])


def book3():
    """three triangles on the edge 0 - 1"""
    return tris_mesh([[0, 0, 0], [0, 0, 1], [1, 0, 0], [0, 1, 0], [-1, -1, 0]], [[0, 1, 2], [0, 1, 3], [1, 0, 4]])


def band(n=8, twist=False):
    """a closed strip of 2 n triangles round the z axis; twist: the last quad joins the two rows crosswise, a Moebius strip"""
    a = 2 * np.pi * np.arange(n) / n
    half = a / 2 if twist else 0 * a
    mid = np.stack([np.cos(a), np.sin(a), 0 * a], axis=1)
    across = np.stack([np.cos(half) * np.cos(a), np.cos(half) * np.sin(a), np.sin(half)], axis=1) * 0.3
    pos = np.concatenate([mid - across, mid + across])                # row a: 0 .. n - 1, row b: n .. 2 n - 1
    tris = []
    for i in range(n):
        a0, b0 = i, n + i
        a1, b1 = (i + 1, n + i + 1) if i + 1 < n else ((n, 0) if twist else (0, n))
        tris += [[a0, a1, b1], [a0, b1, b0]]
    return tris_mesh(pos, tris)


def closed_grid(n=6, m=6, klein=False, quads=False):
    """an n x m grid of quads closed in both directions: a torus, or with klein a Klein bottle (column n is column 0 upside down)"""
    def v(i, j):
        if i == n:
            i, j = 0, ((m - j) % m if klein else j)
        return i * m + j % m
    u, w = np.meshgrid(2 * np.pi * np.arange(n) / n, 2 * np.pi * np.arange(m) / m, indexing="ij")
    pos = np.stack([(2 + np.cos(w)) * np.cos(u), (2 + np.cos(w)) * np.sin(u), np.sin(w)], axis=2).reshape(-1, 3)
    faces = []
    for i in range(n):
        for j in range(m):
            q = [v(i, j), v(i + 1, j), v(i + 1, j + 1), v(i, j + 1)]
            faces += [q] if quads else [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    k = 4 if quads else 3
    return np.asarray(pos, np.float32), np.full(len(faces), k, np.uint8), np.asarray(faces, np.uint32).reshape(-1)


def quad_with_fins():
    """a quad (a, b, c, d) and the triangles (a, c, x), (c, a, y) on its diagonal, which has four sides"""
    pos = [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1], [0.5, 0.5, -1]]
    return np.asarray(pos, np.float32), np.array([4, 3, 3], np.uint8), np.array([0, 1, 2, 3, 0, 2, 4, 2, 0, 5], np.uint32)


def repeated_vertex():
    """two ordinary triangles, then two that repeat vertex 3: their 3 - 3 edge has two sides in two triangles and relates nothing"""
    pos = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [2, 0, 0], [2, 1, 0]]
    return tris_mesh(pos, [[0, 1, 2], [2, 1, 3], [3, 3, 4], [3, 3, 5]])
