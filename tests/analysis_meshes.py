"""Meshes designed for the seams of twins.hip -- the twin matcher (k_twin_*) and the component analysis (k_cc_*, analysis.cpp) -- as
(positions [nv, 3] float32, degrees, corners), and for each the function that counts, on plain arrays, the condition the mesh
exists for.  A test asserts a case's condition twice: with the host's twins (tests/test_analysis_cpu.py) and with the twins that came
down from the device (tests/test_gpu_analysis.py).  The constants are read from twins.hip; the cases follow them by name."""
from __future__ import annotations

import itertools

import numpy as np

from harry_amd import meshgen as mg
from tests import analysis_ref as ar
from tests import seam_meshes as sm
from tests import util

TWIN_SEG_MAX = 48        # twins.hip: kTwinSegMax, the entries one thread of k_twin_match sorts; a vertex above is left to the host
TWIN_OVER_MAX = 4096     # twins.hip: kTwinOverMax, the vertices the list of k_twin_match holds; above, the host matches everything
HOOK_FACES = 16384       # twins.hip: kHookFaces, the faces a workgroup of k_cc_hook_local unites in LDS
STATS_BLOCK = 256        # twins.hip: the threads of k_cc_face_stats / k_cc_vertex_stats / k_cc_vertex_ties and the entries of their LDS lists
WAVE = 64
TIE_LISTS = 64           # twins.hip: kTieLists, the sub-lists of the tie list (a workgroup appends to the one of its index)
TIE_PAIRS = 1 << 22      # twins.hip: kTiePairs, the pairs of all sub-lists together
TIE_SUB = TIE_PAIRS // TIE_LISTS
SCAN_BLOCK = 1024        # scan.hip: kScanBlock


def positions(nv, seed=1):
    return np.random.default_rng(seed).random((nv, 3), dtype=np.float32)


def mesh(deg, idx, nv=None, seed=1):
    idx = np.ascontiguousarray(idx, np.uint32).reshape(-1)
    nv = int(idx.max()) + 1 if nv is None else nv
    return positions(nv, seed), np.ascontiguousarray(deg, np.uint8), idx


def tri_mesh(tris, nv=None, seed=1):
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    return mesh(np.full(len(tris), 3, np.uint8), tris, nv, seed)


def to_hc(m):
    """the mesh in the library (twins pending)"""
    from harry_amd import codec as hc
    return hc.Mesh.from_arrays(util.xyz(m[0]), m[1], m[2])


def to_ply(m):
    return mg.Mesh(util.xyz(m[0]), m[1], m[2]).to_ply()


def offsets(m):
    return np.concatenate(([0], np.cumsum(np.asarray(m[1], np.int64))))


def shuffled_faces(m, seed):
    """the faces of a mesh in a random order"""
    pos, deg, idx = m
    off = offsets(m)
    perm = np.random.default_rng(seed).permutation(len(deg))
    d = np.asarray(deg, np.int64)[perm]
    at = np.repeat(off[perm], d) + (np.arange(int(d.sum())) - np.repeat(np.concatenate(([0], np.cumsum(d)))[:-1], d))
    return pos, np.asarray(deg)[perm], np.asarray(idx)[at]


# ---- what a case is there for
def segment_lengths(face_offsets, org, nv):
    """per vertex the half-edges whose smaller endpoint it is: the segment k_twin_match sorts"""
    org = np.asarray(org, np.int64)
    return np.bincount(np.minimum(org, org[ar.next_halfedge(face_offsets)]), minlength=nv)


def vertices_over(face_offsets, org, nv):
    """how many vertices k_twin_match must leave to the host"""
    return int((segment_lengths(face_offsets, org, nv) > TWIN_SEG_MAX).sum())


def twin_path(reported):
    """which path an upload took, from the count k_twin_match reported"""
    return "device" if reported == 0 else "patched" if reported <= TWIN_OVER_MAX else "host"


def runs_of(face_offsets, org, vertex):
    """the lengths of the runs of equal larger endpoints in a vertex' segment"""
    org = np.asarray(org, np.int64)
    other = org[ar.next_halfedge(face_offsets)]
    lo, hi = np.minimum(org, other), np.maximum(org, other)
    return np.sort(np.unique(hi[lo == vertex], return_counts=True)[1])


def direction_sequences(face_offsets, org):
    """for every undirected edge the directions of its half-edges in index order (True: from the smaller endpoint) -> the set of them"""
    org = np.asarray(org, np.int64)
    other = org[ar.next_halfedge(face_offsets)]
    seqs = {}
    for h in range(len(org)):
        a, b = int(org[h]), int(other[h])
        seqs.setdefault((min(a, b), max(a, b)), []).append(a < b if a != b else None)
    return seqs


def face_pairs(face_offsets, twin):
    """the unions of k_cc_hook_local / k_cc_hook as (face, other face) [R, 2]: a two-sided edge once, from its larger face; a one-sided
    twin from the side that has it"""
    twin = np.asarray(twin, np.int64)
    fh = ar.faces_of_halfedges(face_offsets)
    h = np.flatnonzero(twin != np.arange(len(twin)))
    f, b = fh[h], fh[twin[h]]
    keep = (b != f) & ~((b > f) & (twin[twin[h]] == h))
    return np.stack([f[keep], b[keep]], axis=1)


def leaving(pairs, tile=HOOK_FACES):
    """how many of the pairs leave the tile their face lies in: the ones k_cc_hook takes"""
    return sm.leaving(pairs, tile)


def one_sided(twin):
    """half-edges with a twin that does not point back"""
    twin = np.asarray(twin, np.int64)
    return int(((twin != np.arange(len(twin))) & (twin[twin] != np.arange(len(twin)))).sum())


def repaired_leaving(face_offsets, before, after, tile=HOOK_FACES):
    """half-edges that a walk gave another twin, between faces of different tiles"""
    before, after = np.asarray(before, np.int64), np.asarray(after, np.int64)
    fh = ar.faces_of_halfedges(face_offsets)
    h = np.flatnonzero((before != after) & (after != np.arange(len(after))))
    return int((fh[h] // tile != fh[after[h]] // tile).sum())


def labels_per_group(labels, size):
    """(fewest, most) different labels among the `size` consecutive elements of every whole group"""
    lab = np.asarray(labels, np.int64)
    rows = np.sort(lab[:len(lab) // size * size].reshape(-1, size), axis=1)
    n = 1 + (np.diff(rows, axis=1) != 0).sum(axis=1)
    return int(n.min()), int(n.max())


def tie_hits(hit, face_offsets):
    """the pairs k_cc_vertex_ties notes per sub-list of the tie list, from the restated `hit` corners: a workgroup of 256 faces appends
    to the list of its index"""
    fh = ar.faces_of_halfedges(face_offsets)
    sub = (fh[np.asarray(hit, bool)] // STATS_BLOCK) % TIE_LISTS
    return np.bincount(sub, minlength=TIE_LISTS)


def vertex_sets(face_offsets, org):
    """how many sets the faces form when faces with a common vertex are joined"""
    fh = ar.faces_of_halfedges(face_offsets)
    org = np.asarray(org, np.int64)
    first = np.full(int(org.max()) + 1, len(fh), np.int64)
    np.minimum.at(first, org, fh)
    return len(np.unique(ar.partition(len(face_offsets) - 1, fh, first[org])))


# ---- the twin matcher
def segment_fan(entries):
    """one vertex (number 1) whose segment holds `entries` half-edges.  Every triangle of a fan brings two, so an odd count takes an open
    fan whose first spoke ends at vertex 0, below the hub: that spoke lies in vertex 0's segment"""
    t = (entries + 1) // 2
    rim = np.arange(2, t + 3)
    if entries & 1:
        rim[0] = 0
    return tri_mesh(np.stack([np.full(t, 1), rim[:-1], rim[1:]], axis=1), nv=t + 3)


def fans(n, t=25):
    """n open fans of t triangles, each on vertices of its own with the hub first: n vertices with 2 t entries"""
    base = np.arange(n)[:, None] * (t + 2)
    i = np.arange(t)[None, :]
    return tri_mesh(np.stack([base + 0 * i, base + 1 + i, base + 2 + i], axis=2))


def direction_mesh(self_twin=False):
    """one undirected edge shared by k faces for k = 1 .. 6, in every sequence of directions (126 edges), each on a pair of vertices of
    its own; the faces of all edges dealt round-robin, so that an edge's half-edges keep their order and lie far apart.  Every second
    pair has its smaller vertex second.  self_twin: also two faces that repeat a vertex at consecutive corners (an edge that is
    its own reverse), once alone and once twice on the same vertex"""
    cases = [s for k in range(1, 7) for s in itertools.product((True, False), repeat=k)]
    faces, nv = [[] for _ in cases], 0
    for c, seq in enumerate(cases):
        a, b = (nv, nv + 1) if c % 2 == 0 else (nv + 1, nv)
        nv += 2
        for out in seq:
            faces[c].append((a, b, nv) if out == (a < b) else (b, a, nv))
            nv += 1
    if self_twin:
        faces.append([(nv, nv, nv + 1)])
        faces.append([(nv + 2, nv + 2, nv + 3), (nv + 2, nv + 2, nv + 4)])
        nv += 5
    tris = [f[i] for i in range(6) for f in faces if len(f) > i]
    return tri_mesh(tris, nv=nv), cases


def books(pages=(48, 49), seed=3):
    """books: an edge (a, b) with `pages` triangles in random directions, the third vertices numbered BELOW a, so that a's segment is
    the run of its pages and nothing else -> (mesh, the vertices a)"""
    rng = np.random.default_rng(seed)
    third = np.arange(sum(pages))
    tris, spines, at = [], [], 0
    for k, p in enumerate(pages):
        a, b = len(third) + 2 * k, len(third) + 2 * k + 1
        spines.append(a)
        for c in third[at:at + p]:
            tris.append((a, b, c) if rng.random() < 0.5 else (b, a, c))
        at += p
    return tri_mesh(tris), spines


# ---- the labelling
def strip(ntri, reverse=False):
    return sm.strip(ntri, reverse)


def alternating_strips(ntri):
    """two strips of ntri triangles, the even faces one strip and the odd faces the other"""
    a, b = sm.strip(ntri), sm.strip(ntri, at=5.0)
    tris = np.empty((2 * ntri, 3), np.int64)
    tris[0::2] = np.asarray(a[2], np.int64).reshape(-1, 3)
    tris[1::2] = np.asarray(b[2], np.int64).reshape(-1, 3) + len(a[0])
    return np.concatenate([a[0], b[0]]), np.full(2 * ntri, 3, np.uint8), tris.reshape(-1).astype(np.uint32)


def shuffled_tori(n=100, seed=5):
    """two tori of 2 n^2 triangles each, all faces in one random order"""
    return shuffled_faces(sm.gen_arrays(mg.concat([mg.torus(n, n, seed=2), mg.torus(n, n, seed=3, center=(4.0, 0.0, 0.0))])), seed)


def repairing(seed=16, split=60):
    """a mesh of more than kHookFaces faces whose walk repairs twins (cbm/encoder.h:150,193-198): one of the soups meshgen.py lists as
    repairing, its first `split` faces in front of a torus that fills a tile and the others behind it, so that half-edges the walk
    pairs anew lie in different tiles"""
    tor, s = sm.gen_arrays(mg.torus(96, 90)), sm.gen_arrays(mg.soup(seed=seed))
    st, tt = np.asarray(s[2], np.int64).reshape(-1, 3) + len(tor[0]), np.asarray(tor[2], np.int64).reshape(-1, 3)
    return tri_mesh(np.concatenate([st[:split], tt, st[split:]]), nv=len(tor[0]) + len(s[0]))


# ---- the per-component sums
def confetti(nf, spare=False):
    """nf lone triangles: every face a component.  spare: an unreferenced vertex behind every triangle's three"""
    per = 4 if spare else 3
    v = np.arange(nf)[:, None] * per + np.arange(3)[None, :]
    return tri_mesh(v, nv=nf * per)


STRIP_DEGREES = (3, 4, 3, 3, 4, 3, 3, 9)


def interleaved_strips(nstrips=64, cycles=3):
    """nstrips chains of polygons, each sharing an edge with the next, faces and vertices dealt round-robin: face j of strip s is face
    j * nstrips + s, its vertex i is vertex i * nstrips + s.  Strip s runs through STRIP_DEGREES from place s on, so the 64 faces of a
    wavefront are of all the degrees, and every strip has the same number of corners"""
    P, L = len(STRIP_DEGREES), len(STRIP_DEGREES) * cycles
    nloc = sum(d - 2 for d in STRIP_DEGREES) * cycles + 2
    deg = np.empty((L, nstrips), np.uint8)
    corners = [[None] * nstrips for _ in range(L)]
    for s in range(nstrips):
        prev, used = None, 0
        for j in range(L):
            d = STRIP_DEGREES[(j + s) % P]
            if prev is None:
                cur, used = list(range(d)), d
            else:   # the shared edge: the previous polygon's last listed edge after an even polygon, its closing edge after an odd one
                x, y = (prev[-2], prev[-1]) if j % 2 == 1 else (prev[-1], prev[0])
                cur = [y, x] + list(range(used, used + d - 2))
                used += d - 2
            deg[j, s], corners[j][s], prev = d, [v * nstrips + s for v in cur], cur
        assert used == nloc
    return mesh(deg.reshape(-1), np.concatenate([np.asarray(c, np.int64) for row in corners for c in row]), nv=nloc * nstrips)


def face0_last():
    """a lone triangle as face 0 in front of three strips: the start-face sequence of so few faces is descending, so face 0's component
    would be coded last if the reference did not take face 0 first whatever the sequence says"""
    parts = [sm.strip(1)] + [sm.strip(3, at=float(k)) for k in range(1, 4)]
    return sm.join(parts)


# ---- the ties
def chain(n=5000, seed=9):
    """n triangles, each sharing ONE vertex (no edge) with the next, faces and vertices in a random order"""
    i = np.arange(n)
    tris = np.stack([i, n + 1 + i, i + 1], axis=1)   # (s_i, u_i, s_i+1)
    rng = np.random.default_rng(seed)
    relabel = rng.permutation(2 * n + 1)
    return tri_mesh(relabel[tris][rng.permutation(n)], nv=2 * n + 1)


def hub_and_pairs(n=300, seed=4):
    """vertex 0 shared by n lone triangles, and n more lone triangles tied in pairs by one vertex each; faces in a random order"""
    i = np.arange(n)
    hub = np.stack([0 * i, 1 + 2 * i, 2 + 2 * i], axis=1)
    base = 1 + 2 * n
    j = np.arange(n // 2)
    first = np.stack([base + 5 * j, base + 5 * j + 1, base + 5 * j + 2], axis=1)
    second = np.stack([base + 5 * j, base + 5 * j + 3, base + 5 * j + 4], axis=1)
    tris = np.concatenate([hub, first, second])
    return tri_mesh(tris[np.random.default_rng(seed).permutation(len(tris))])


OVERFLOW_POOL = 739                                                  # a prime: every 2 x 2 matrix below is invertible modulo it
OVERFLOW_STEPS = ((1, 0), (0, 1), (1, 1), (1, 2), (2, 3), (3, 5), (5, 8), (8, 13))   # consecutive rows (and the last with the first) have determinant +-1, -13


def overflow(n=OVERFLOW_POOL):
    """n^2 lone octagons whose corner m comes from pool m of n vertices: octagon (i, j) takes vertex (a i + b j) mod n of pool m with
    (a, b) = OVERFLOW_STEPS[m].  Two octagons never agree in two consecutive corners (the steps of consecutive corners are
    independent modulo n), so no edge is shared and every face is a component -- and every corner but a pool vertex' first is a hit
    of k_cc_vertex_ties: 2048 a workgroup.  The even pools are numbered below the odd ones: 4 n hubs for the twin matcher"""
    i, j = np.meshgrid(np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64), indexing="ij")
    i, j = i.reshape(-1), j.reshape(-1)
    base = [(m // 2 + (4 if m % 2 else 0)) * n for m in range(8)]
    idx = np.stack([base[m] + (a * i + b * j) % n for m, (a, b) in enumerate(OVERFLOW_STEPS)], axis=1)
    return mesh(np.full(n * n, 8, np.uint8), idx, nv=8 * n)
