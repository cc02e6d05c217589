"""Meshes designed for the seams of the analysis kernels -- the sizes at which orient.hip, shells.hip, edges.hip and normals.hip change
strategy -- as (positions [nv, 3] float32, degrees, corners), and for each the function that counts what the case is there for.  The
counting functions take the arrays of a render build (indices [T, 3], vertex_source, tri_face) and the restatements' outputs, so a
test asserts a case's condition twice: on the arrays themselves (tests/test_seams_cpu.py) and on the same run's render buffers
(tests/test_gpu_seams.py).  The constants are read from the .hip files; the cases follow them by name."""
from __future__ import annotations

import numpy as np

from harry_amd import meshgen as mg
from tests import orient_ref as orf
from tests import shells_ref as sr

COVER_TRIS = 4096    # orient.hip: a tile of k_hook_local<CoverGraph> (hook.hpp), the triangles a workgroup unites in LDS
HOOK_TRIS = 8192     # shells.hip: ... of k_hook_local<ShellGraph>
CHUNK = 256          # measures.hip: kShellChunk, the triangles of one partial sum
SEG_MAX = 32         # measures.hip: kSegMax; edges.hip: kEdgeSegMax; normals.hip: kNrmSegMax -- a lane above, a workgroup beyond
SORT_BLOCK = 256     # seg_sort.hpp: the threads of block_sort_segment; k_sh_hubs' tile of partials
WAVE = 64
LABEL_BLOCK = 256    # the threads of a block of the per-label kernels (k_sh_summary, k_or_decide, k_or_outward, k_sh_sums)
SCAN_BLOCK = 1024    # scan.hip: kScanBlock, the flags one block of launch_excl_scan holds


# ---- render-build arrays of a mesh in the PLY layout
def arrays_of(mesh):
    """(indices [T, 3], vertex_source, tri_face, nf) as a render build of hc.Mesh.from_arrays(mesh) has them: the fan, no vertex split"""
    pos, deg, idx = mesh
    I, tf = sr.fan(deg, idx)
    return I, np.arange(len(pos)), tf, len(deg)


def gen_arrays(m):
    """a meshgen mesh as (positions, degrees, corners)"""
    return np.stack([m.verts["x"], m.verts["y"], m.verts["z"]], axis=1).astype(np.float32), m.degrees, m.indices


def join(meshes):
    """the disjoint union of (positions, degrees, corners) meshes, faces in the order given"""
    base = np.cumsum([0] + [len(m[0]) for m in meshes])[:-1]
    return (np.concatenate([np.asarray(m[0], np.float32) for m in meshes]), np.concatenate([np.asarray(m[1], np.uint8) for m in meshes]),
            np.concatenate([np.asarray(m[2], np.int64) + b for m, b in zip(meshes, base)]).astype(np.uint32))


def reordered(mesh, order):
    """a triangle mesh with its triangles in the order given"""
    pos, deg, idx = mesh
    assert (np.asarray(deg) == 3).all()
    return pos, deg, np.ascontiguousarray(np.asarray(idx).reshape(-1, 3)[order]).reshape(-1)


# ---- what a case is there for
def leaving(pairs, tile):
    """how many of the relations (t, other) [R, 2] leave the tile of `tile` triangles that t lies in: the ones the second hook pass takes"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    return int((pairs[:, 0] // tile != pairs[:, 1] // tile).sum())


def shell_pairs(edges):
    """the unions of k_sh_hook_local / k_sh_hook: every side but the first of an edge, with the first side's triangle -- [R, 2]"""
    off, sides = edges["edge_offsets"].astype(np.int64), edges["edge_sides"].astype(np.int64)
    first = np.repeat(sides[off[:-1]], np.diff(off))
    keep = sides // 3 != first // 3
    return np.stack([sides[keep] // 3, first[keep] // 3], axis=1)


def orient_pairs(indices, vertex_source, tri_face, edges):
    """the relations of k_or_hook_local / k_or_hook: ([R, 2], how many of them -- the first -- come from a joining edge)"""
    rel, _, n_edge = orf.relations(indices, vertex_source, tri_face, edges)
    return np.array([(a, b) for a, b, _ in rel], np.int64).reshape(-1, 2), n_edge


def fan_on_seam_counts(indices, vertex_source, tri_face, edges, seam):
    """(the triangles either side of `seam` belong to one face, the triangles of that face, how many of their sides are joining sides)"""
    tf = np.asarray(tri_face, np.int64)
    _, joining, _ = orf.relations(indices, vertex_source, tf, edges)
    fan = np.flatnonzero(tf == tf[seam])
    return bool(tf[seam - 1] == tf[seam]), fan, int(joining.reshape(-1, 3)[fan].sum())


def chunk_entries(tri_label):
    """per label (how many chunks of 256 triangles hold it: its partials; the chunks from its first to its last)"""
    lab = np.asarray(tri_label, np.int64)
    pairs = np.unique(np.stack([lab, np.arange(len(lab)) // CHUNK], axis=1), axis=0)
    n = int(lab.max()) + 1 if len(lab) else 0
    entries = np.bincount(pairs[:, 0], minlength=n)
    lo, hi = np.full(n, len(lab)), np.zeros(n, np.int64)
    np.minimum.at(lo, pairs[:, 0], pairs[:, 1])
    np.maximum.at(hi, pairs[:, 0], pairs[:, 1])
    return entries, hi - lo + 1


def segment_lengths(edges):
    """the sides per edge"""
    return np.diff(edges["edge_offsets"].astype(np.int64))


def corners_per_vertex(indices, vertex_source, nv):
    """the corners per decoded vertex: the terms of a vertex normal's sum"""
    return np.bincount(np.asarray(vertex_source, np.int64)[np.asarray(indices, np.int64).reshape(-1)], minlength=nv)


def labels_per_wavefront(tri_label):
    """the fewest different labels among the 64 triangles of a whole wavefront"""
    lab = np.asarray(tri_label, np.int64)
    rows = lab[:len(lab) // WAVE * WAVE].reshape(-1, WAVE)
    return min(len(set(r.tolist())) for r in rows)


# ---- strips
def strip(ntri, reverse=False, at=0.0):
    """the first ntri triangles of a two-row grid, each next to the one before; reverse: listed from the far end"""
    m = mg.grid(ntri // 2 + 2, 2)
    tris = m.indices.reshape(-1, 3)[:ntri]
    assert len(tris) == ntri
    pos = np.stack([m.verts["x"] + at, m.verts["y"], m.verts["z"]], axis=1).astype(np.float32)
    return pos, np.full(ntri, 3, np.uint8), np.ascontiguousarray(tris[::-1] if reverse else tris).reshape(-1)


def turned_strip(ntri, reverse=False):
    """... with random_turns: -> (mesh, the flags)"""
    return orf.random_turns(strip(ntri, reverse))


# ---- 1. a polygon whose fan lies across a tile seam and is held together by the same-face rule alone
def fan_on_seam(degree, lead, tile=COVER_TRIS):
    """a strip of tile - lead triangles, a polygon of `degree` corners on vertices of its own, and on every diagonal v0 - vd of its fan
    the two fin triangles of orf.quad_with_fins: the diagonal has four sides and joins nothing, the polygon's rim has one.  The fan is
    the triangles tile - lead .. tile - lead + degree - 3, so with lead in 1 .. degree - 2 it crosses `tile`"""
    assert 1 <= lead <= degree - 2
    a = 2 * np.pi * np.arange(degree) / degree
    ring = np.stack([3 + np.cos(a), 3 + np.sin(a), 0.1 * np.cos(2 * a)], axis=1)
    fins_pos, fins = [], []
    for d in range(2, degree - 1):
        mid = 0.5 * (ring[0] + ring[d])
        k = degree + len(fins_pos)
        fins_pos += [mid + [0, 0, 1], mid - [0, 0, 1]]
        fins += [[0, d, k], [d, 0, k + 1]]
    poly = (np.concatenate([ring, np.array(fins_pos).reshape(-1, 3)]), np.array([degree] + [3] * len(fins), np.uint8),
            np.concatenate([np.arange(degree), np.array(fins, np.int64).reshape(-1)]))
    return join([strip(tile - lead), poly])


# ---- 7. two shells in alternating blocks of one chunk
def alternating_blocks(blocks=40):
    """two strips of blocks x 256 triangles laid out in alternating blocks of 256: each shell has `blocks` partials over a span of
    2 blocks - 1 chunks, so every second slot of its span holds no partial of the shell"""
    n = blocks * CHUNK
    both = join([strip(n), strip(n, at=50.0)])
    order = np.stack([np.arange(n).reshape(blocks, CHUNK), n + np.arange(n).reshape(blocks, CHUNK)], axis=1).reshape(-1)
    return reordered(both, order)


# ---- 9. many labels
def confetti(n=3000, seed=41):
    """n triangles on vertices of their own at random float32 positions: n shells, n patches"""
    pos = np.random.default_rng(seed).random((3 * n, 3)).astype(np.float32) * 10
    return pos, np.full(n, 3, np.uint8), np.arange(3 * n, dtype=np.uint32)


def interleaved_strips(strips=WAVE, each=48):
    """`strips` strips of `each` triangles, triangle i belonging to strip i % strips: every wavefront holds `strips` labels, and every
    label recurs in every tile"""
    both = join([strip(each, at=3.0 * k) for k in range(strips)])
    order = (np.arange(strips)[None, :] * each + np.arange(each)[:, None]).reshape(-1)
    return reordered(both, order)


# ---- 10. long edge segments
def book(pages, at=0.0):
    """`pages` triangles round one shared edge (the spine 0 - 1), their winding alternating so that the spine's sides run both ways,
    with a strip of ordinary triangles behind them"""
    a = 2 * np.pi * np.arange(pages) / pages
    pos = np.concatenate([[[0, 0, 0], [0, 0, 1]], np.stack([np.cos(a), np.sin(a), 0.5 + 0.25 * np.cos(3 * a)], axis=1)])
    tris = [(0, 1, 2 + i) if i % 3 else (1, 0, 2 + i) for i in range(pages)]
    tail = mg.grid(6, 2)
    tpos = np.stack([tail.verts["x"] + 5, tail.verts["y"], tail.verts["z"]], axis=1)
    tris = np.concatenate([np.array(tris), tail.indices.reshape(-1, 3) + len(pos)])
    pos = np.concatenate([pos, tpos]) + [at, 0, 0]
    return pos.astype(np.float32), np.full(len(tris), 3, np.uint8), tris.astype(np.uint32).reshape(-1)


def shelf(books=20, pages=33):
    """`books` books of `pages` pages in one mesh: as many long segments"""
    return join([book(pages, at=10.0 * k) for k in range(books)])


# ---- 11. vertices either side of 32 and 256 corners
HUB_VALENCES = [31, 32, 33, 34, 255, 256, 257]


def hub_discs():
    return gen_arrays(mg.hub_discs(HUB_VALENCES))


# ---- 6. a closed surface in a hostile order
def shuffled_torus(nu=96, nv=128, seed=23):
    """mg.torus with its triangles shuffled: most relations leave their tile"""
    m = gen_arrays(mg.torus(nu, nv))
    return reordered(m, np.random.default_rng(seed).permutation(len(m[1])))


# ---- the cases, shared by the CPU and the GPU test
FANS = {   # name: (degree, lead, tile) -- the fan of the polygon is the triangles tile - lead ..
    "quad_4095": (4, 1, COVER_TRIS), "pentagon_4095": (5, 1, COVER_TRIS), "pentagon_4094": (5, 2, COVER_TRIS),
    "pentagon_8191": (5, 1, HOOK_TRIS), "pentagon_8190": (5, 2, HOOK_TRIS),   # orient's second seam is the shells' first
}
TWO_TILES = {   # name: (mesh, (patches, orientable, inverted) of the restatement's summary) -- 4200 and 4608 triangles, one patch
    "moebius": (lambda: orf.band(2100, twist=True), (1, 0, 0)),
    "band_turned": (lambda: orf.random_turns(orf.band(2100))[0], (1, 1, 0)),
    "klein": (lambda: orf.closed_grid(48, 48, klein=True), (1, 0, 0)),
    "torus_quads_turned": (lambda: orf.random_turns(orf.closed_grid(48, 48, quads=True))[0], (1, 1, 0)),
}
ORIENT_STRIPS = [COVER_TRIS - 1, COVER_TRIS, COVER_TRIS + 1]
SHELL_STRIPS = [HOOK_TRIS - 1, HOOK_TRIS, HOOK_TRIS + 1, 16400]   # 8192 and 8193 triangles are 32 and 33 partials: either side of kSegMax
LONG_STRIP = (SORT_BLOCK + 1) * CHUNK + 3                           # 258 partials: the second tile of k_sh_hubs' left-to-right sum
BOOK_PAGES = [SEG_MAX - 1, SEG_MAX, SEG_MAX + 1, SORT_BLOCK - 1, SORT_BLOCK, SORT_BLOCK + 1]
