"""Inputs for the first-occurrence numbering (harry_amd/csrc/device/dedup.hip) chosen for where their keys hash: every case puts
its keys' home slots at the end of the table, so that the cluster they build wraps from the last slot to slot 0 and the probe paths
are as long as the case has keys.  The inputs are found by search with the restated hashes of tests/dedup_ref.py: a fixed range of
candidates, the lowest qualifying ones taken in order, so a case is the same on every run -- and loses its property if a hash or the
table's size changes, which tests/test_dedup_cpu.py then reports by the case's name.  Every generator returns the input and the
census (dedup_ref.table_census of its distinct keys' homes, plus "slots", "items" and "keys") the case is there for."""
from __future__ import annotations

import functools

import numpy as np

from tests import dedup_ref as dr
from tests import ingest_ref as ir

LAST = 4   # the home slots of a case are the last LAST slots of its table


def census_of(hashes_of_distinct_keys, items: int) -> dict:
    """the census of a table for `items` items whose distinct keys, in order of first occurrence, have these hashes"""
    slots = dr.slots_for(items)
    c = dr.table_census(np.asarray(hashes_of_distinct_keys, np.uint32) & np.uint32(slots - 1), slots, LAST)
    c.update(slots=slots, items=int(items), keys=len(hashes_of_distinct_keys))
    return c


def _lowest(want: int, limit: int, block: int, qualifies):
    """the lowest `want` candidates of 0 .. limit - 1 for which qualifies(candidates u32 [m]) -> bool [m] holds"""
    found, have = [], 0
    for lo in range(0, limit, block):
        cand = np.arange(lo, min(lo + block, limit), dtype=np.uint32)
        hit = cand[qualifies(cand)]
        found.append(hit)
        have += len(hit)
        if have >= want:
            break
    found = np.concatenate(found)[:want]
    assert len(found) == want, (want, len(found), limit)
    return found


# ---- weld: float32 rows; the candidates are the floats 0 .. 2^24 - 1, all exact and distinct
WELD_LIMIT = 1 << 24


def _weld_values(want, slots, first_home, records_of):
    mask = np.uint32(slots - 1)
    return _lowest(want, WELD_LIMIT, 1 << 20, lambda c: (dr.weld_hash(records_of(c.astype(np.float32))) & mask) >= first_home).astype(np.float32)


def weld_census(columns) -> dict:
    """the census of the weld of these columns' rows"""
    rec = ir.packed_records(columns)
    _, first = ir.weld(rec)
    return census_of(dr.weld_hash(rec[first]), len(rec))


@functools.lru_cache(maxsize=None)
def weld_one_home(n: int):
    """n distinct rows of one float32 column, every home the last slot: one run of n slots from slot `slots - 1` on, and the row
    that comes last probes all of it.  -> ([x], census)"""
    slots = dr.slots_for(n)
    x = _weld_values(n, slots, slots - 1, lambda v: ir.packed_records([v]))
    return [x], weld_census([x])


@functools.lru_cache(maxsize=None)
def weld_last_slots_dups(keys: int = 2048, seed: int = 5):
    """`keys` distinct rows with their homes in the last LAST slots of the table of 2 * keys rows, every one present twice, the rows
    shuffled: duplicates of many keys interleaved on one cluster.  -> ([x], census)"""
    slots = dr.slots_for(2 * keys)
    v = _weld_values(keys, slots, slots - LAST, lambda v: ir.packed_records([v]))
    x = np.random.default_rng(seed).permutation(np.concatenate([v, v]))
    return [x], weld_census([x])


WIDE_COLUMNS, WIDE_SEARCHED = 9, 4


@functools.lru_cache(maxsize=None)
def weld_stride36_one_home(n: int = 512):
    """weld_one_home(n) with records of nine float32 columns (stride 36): the search varies column WIDE_SEARCHED, the other eight
    hold one non-zero value each.  -> (the nine columns, census)"""
    slots = dr.slots_for(n)

    def columns(v):
        return [v if k == WIDE_SEARCHED else np.full(len(v), k + 0.5, np.float32) for k in range(WIDE_COLUMNS)]

    x = _weld_values(n, slots, slots - 1, lambda v: ir.packed_records(columns(v)))
    cols = columns(x)
    return cols, weld_census(cols)


# ---- edges: a closed fan round vertex 0 whose spokes (0, b) all have their homes in the last LAST slots
def edge_keys(tris, vertex_source=None):
    """(lo, hi) u32 [3 T, 2] of every side, in side order"""
    I = np.asarray(tris, np.int64).reshape(-1, 3)
    if vertex_source is not None:
        I = np.asarray(vertex_source, np.int64)[I]
    a, b = I.reshape(-1), I[:, [1, 2, 0]].reshape(-1)
    return np.stack([np.minimum(a, b), np.maximum(a, b)], axis=1).astype(np.uint32)


def edges_census(tris, vertex_source=None) -> dict:
    """the census of the sides' table, plus "spokes_in_last": the keys (0, b) among those with their homes in the last slots, and
    "spoke_sides": the set of side counts of the keys (0, b)"""
    keys = edge_keys(tris, vertex_source)
    ids, first = dr.first_occurrence(keys)
    distinct = keys[first]
    h = dr.edge_hash(distinct[:, 0], distinct[:, 1])
    c = census_of(h, len(keys))
    spoke = distinct[:, 0] == 0
    c["spokes_in_last"] = int((spoke & ((h & np.uint32(c["slots"] - 1)) >= c["slots"] - LAST)).sum())
    c["spoke_sides"] = sorted(set(np.bincount(ids, minlength=len(first))[spoke].tolist()))
    return c


EDGE_FAN_T = 1100        # 3 T = 3300 sides: a table of 8192 slots
EDGE_LIMIT = 1 << 23     # (a slot in 2048 is a home: some 2^21.1 ids hold 1100 rim vertices)


@functools.lru_cache(maxsize=None)
def edge_fan_one_cluster(T: int = EDGE_FAN_T):
    """T triangles (0, r[i], r[i + 1]) round vertex 0, the rim r the lowest T ids b > 0 whose key (0, b) has its home in the last
    LAST slots of the table of 3 T sides.  The hub lies above the centre of a unit circle that carries the rim; every other
    vertex lies on a line outside it, so all positions are finite and distinct.  -> (positions f32 [nv, 3], triangles, census)"""
    slots = dr.slots_for(3 * T)
    mask = np.uint32(slots - 1)
    rim = _lowest(T, EDGE_LIMIT, 1 << 20, lambda b: (b > 0) & ((dr.edge_hash(np.zeros(len(b), np.uint32), b) & mask) >= slots - LAST)).astype(np.int64)
    nv = int(rim[-1]) + 1
    pos = np.zeros((nv, 3), np.float32)
    pos[:, 0] = 2.0 + np.arange(nv)
    a = 2 * np.pi * np.arange(T) / T
    pos[rim] = np.stack([np.cos(a), np.sin(a), np.zeros(T)], axis=1)
    pos[0] = (0, 0, 0.5)
    tris = np.stack([np.zeros(T, np.int64), rim, np.roll(rim, -1)], axis=1).astype(np.uint32)
    return pos, tris, edges_census(tris)


# ---- unweld: an OBJ scene `f v/vt/` (the reader takes a bare `v/vt` for a normal's index too) whose corner keys (org, vt record) all have their homes in the last LAST slots
UNWELD_CORNERS, UNWELD_VT = 2048, 1 << 15


def unweld_census(corner_keys) -> dict:
    """the census of the corners' table from tests/render_ref.py: corner_keys(mesh)"""
    keys = np.asarray(corner_keys, np.uint32)
    _, first = dr.first_occurrence(keys)
    return census_of(dr.unweld_hash(keys[first]), len(keys))


@functools.lru_cache(maxsize=None)
def unweld_one_home(seed: int = 7):
    """2048 corners -- a table of 4096 slots at load 1/2, as full as a table gets.  Vertex k (k < 1024) is used with the lowest
    texture record t[k] < 2^15 for which the key (k, t[k]) has its home in the last LAST slots; corners 0 .. 1023 name the
    pairs in order, corners 1024 .. 2047 name them again in a shuffle, so every output vertex is shared by two corners.  2048 is no
    multiple of 3: each half is one quad and 340 triangles, and no face names a vertex twice.
    -> (OBJ text, the pair (v, vt) of every corner i64 [2048, 2], census)"""
    K = UNWELD_CORNERS // 2
    slots = dr.slots_for(UNWELD_CORNERS)
    mask = np.uint32(slots - 1)
    vt = np.zeros(K, np.int64)
    for k in range(K):
        vt[k] = _lowest(1, UNWELD_VT, 1 << 12, lambda t: (dr.unweld_hash(np.stack([np.full(len(t), k, np.uint32), t], axis=1)) & mask) >= slots - LAST)[0]
    rng = np.random.default_rng(seed)
    order = np.concatenate([np.arange(K), rng.permutation(K)])
    pairs = np.stack([order, vt[order]], axis=1)
    pos = rng.uniform(-1, 1, (K, 3)).astype(np.float32)
    lines = ["v %.8f %.8f %.8f" % tuple(float(c) for c in p) for p in pos]
    lines += ["vt %.8f %.8f" % (a / UNWELD_VT, (a * 37) % UNWELD_VT / UNWELD_VT) for a in range(UNWELD_VT)]   # (distinct rows)
    at = 0
    for half in range(2):
        for deg in [4] + [3] * ((K - 4) // 3):
            lines.append("f " + " ".join("%d/%d/" % (v + 1, t + 1) for v, t in pairs[at:at + deg]))
            at += deg
    assert at == UNWELD_CORNERS
    keys = pairs.astype(np.uint32)
    return ("\n".join(lines) + "\n").encode(), pairs, unweld_census(keys)


# ---- shells: strips whose corners' keys (shell, vertex) all have their homes in the last LAST slots
SHELL_LIMIT = 1 << 22


def shell_keys(indices, vertex_source, tri_shell):
    """(shell, vertex) u32 [3 T, 2] of every corner, in corner order"""
    I = np.asarray(indices, np.int64).reshape(-1)
    return np.stack([np.repeat(np.asarray(tri_shell, np.int64), 3), np.asarray(vertex_source, np.int64)[I]], axis=1).astype(np.uint32)


def shells_census(keys) -> dict:
    """the census of the corners' table, plus "corners_in_last": the corners whose key has its home in the last slots"""
    keys = np.asarray(keys, np.uint32)
    ids, first = dr.first_occurrence(keys)
    h = dr.shell_vertex_hash(keys[first, 0], keys[first, 1])
    c = census_of(h, len(keys))
    c["corners_in_last"] = int(((h & np.uint32(c["slots"] - 1)) >= c["slots"] - LAST)[ids].sum())
    return c


def _strip(ids, at):
    """len(ids) - 2 triangles along ids, wound alike; positions of the ids: a zigzag from x = at"""
    n = len(ids) - 2
    i = np.arange(n)
    a, b = np.where(i % 2 == 0, i, i + 1), np.where(i % 2 == 0, i + 1, i)
    tris = np.stack([ids[a], ids[b], ids[i + 2]], axis=1)
    j = np.arange(len(ids))
    return tris, np.stack([at + j // 2 * 1.0, j % 2 * 1.0, np.zeros(len(ids))], axis=1)


@functools.lru_cache(maxsize=None)
def shell_vertex_one_home(shells: int = 1, T: int = 680):
    """T triangles (3 T = 2040 corners: a table of 4096 slots, all but at load 1/2) in `shells` strips of T / shells triangles.
    Strip s takes its T / shells + 2 vertex ids, ascending, from the lowest unused ids whose key (s, id) has its home in the
    last LAST slots.  The strips share no vertex, and strip s begins at triangle s * T / shells, so the shell of strip s is s:
    shells are numbered by their lowest triangle.  Every other vertex lies on a line far from the strips.
    -> (positions f32 [nv, 3], triangles, census)"""
    assert T % shells == 0
    slots = dr.slots_for(3 * T)
    mask = np.uint32(slots - 1)
    used = np.zeros(SHELL_LIMIT, bool)
    tris, where = [], []
    for s in range(shells):
        ids = _lowest(T // shells + 2, SHELL_LIMIT, 1 << 20,
                      lambda v: ~used[v] & ((dr.shell_vertex_hash(np.full(len(v), s, np.uint32), v) & mask) >= slots - LAST)).astype(np.int64)
        used[ids] = True
        t, p = _strip(ids, 1000.0 * s)
        tris.append(t)
        where.append((ids, p))
    nv = int(np.flatnonzero(used)[-1]) + 1
    pos = np.zeros((nv, 3), np.float32)
    pos[:, 0] = -2.0 - np.arange(nv)
    for ids, p in where:
        pos[ids] = p
    tris = np.concatenate(tris).astype(np.uint32)
    keys = shell_keys(tris, np.arange(nv), np.repeat(np.arange(shells), T // shells))
    return pos, tris, shells_census(keys)


# ---- creases: a triangle soup whose slots' keys (output vertex, smooth-group root) all have their homes in the last LAST slots
CREASE_LIMIT = 1 << 16
CREASE_COS_LIMIT = 2.0   # above every cosine: every real edge is sharp


def crease_keys(indices, slot_group):
    """(output vertex, root) u32 [3 T, 2] of every slot: the root of a group is its smallest slot"""
    I, g = np.asarray(indices, np.int64).reshape(-1), np.asarray(slot_group, np.int64).reshape(-1)
    root = np.full(int(g.max()) + 1 if len(g) else 0, len(g), np.int64)
    np.minimum.at(root, g, np.arange(len(g)))
    return np.stack([I, root[g]], axis=1).astype(np.uint32)


def creases_census(keys) -> dict:
    keys = np.asarray(keys, np.uint32)
    _, first = dr.first_occurrence(keys)
    return census_of(dr.crease_hash(keys[first, 0], keys[first, 1]), len(keys))


@functools.lru_cache(maxsize=None)
def crease_soup_one_home(T: int = 682, seed: int = 9):
    """T triangles that share no vertex (3 T = 2046 slots: a table of 4096 slots).  Why the roots are known: the contract of
    hry_creases_build unites slots across SMOOTH edges only and names a group by its smallest slot; in a soup of triangles every
    edge has one side (BOUNDARY), so at any limit -- the case is built at CREASE_COS_LIMIT, where even a shared edge would be
    sharp -- every slot is a group of its own and its root is the slot itself.  A PLY-layout mesh's output vertices are its
    vertices, so the key of slot s is (the vertex it names, s): slot s names the lowest unused vertex v < 2^16 for which the key
    (v, s) has its home in the last LAST slots.  All 3 T keys are distinct and lie in one run.  Positions: seeded, uniform in a
    cube.  -> (positions f32 [nv, 3], triangles, census)"""
    n = 3 * T
    slots = dr.slots_for(n)
    mask = np.uint32(slots - 1)
    used = np.zeros(CREASE_LIMIT, bool)
    names = np.zeros(n, np.int64)
    for s in range(n):
        names[s] = _lowest(1, CREASE_LIMIT, 1 << 12, lambda v: ~used[v] & ((dr.crease_hash(v, np.full(len(v), s, np.uint32)) & mask) >= slots - LAST))[0]
        used[names[s]] = True
    nv = int(names.max()) + 1
    pos = np.random.default_rng(seed).uniform(-1, 1, (nv, 3)).astype(np.float32)
    tris = names.reshape(T, 3).astype(np.uint32)
    return pos, tris, creases_census(crease_keys(tris, np.arange(n)))
