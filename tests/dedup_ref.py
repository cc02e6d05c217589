"""numpy restatement of what decides the probe paths of the first-occurrence numbering (harry_amd/csrc/device/dedup.hip): the five
key policies' hashes (dedup_hash.hpp; tied to the source by tests/test_dedup_cpu.py through tests/native/dedup_hash_check.cpp), the
table's size (DedupPlan::reserve), and a census of an open-addressing table with linear probing from the home slots of its distinct
keys.  Shared by tests/dedup_cases.py, tests/test_dedup_cpu.py and tests/test_gpu_dedup.py."""
from __future__ import annotations

import numpy as np

NONE = 0xFFFFFFFF


def _u32(a) -> np.ndarray:
    return np.atleast_1d(np.asarray(a)).astype(np.uint32)


# ---- the hashes (uint32 arrays: products and sums wrap)
def fmix(h: np.ndarray) -> np.ndarray:
    """murmur3's finaliser"""
    h = _u32(h).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def mix_part(h: np.ndarray, part) -> np.ndarray:
    """one more key part into a running value, then the finaliser"""
    h = _u32(h)
    return fmix(h ^ (_u32(part) + np.uint32(0x7F4A7C15) + (h << np.uint32(6)) + (h >> np.uint32(2))))


def hash_bytes(records: np.ndarray) -> np.ndarray:
    """uint8 [n, stride] -> u32 [n]: FNV-1a over the record, then the finaliser"""
    records = np.asarray(records, np.uint8)
    h = np.full(len(records), 0x811C9DC5, np.uint32)
    for k in range(records.shape[1]):
        h = (h ^ records[:, k]) * np.uint32(0x01000193)
    return fmix(h)


def hash_pair(first, second) -> np.ndarray:
    return mix_part(fmix(_u32(first) * np.uint32(0x9E3779B1)), second)


def hash_parts(keys: np.ndarray) -> np.ndarray:
    """u32 [n, parts] -> u32 [n]: the running value over the parts in order"""
    keys = np.asarray(keys, np.uint32)
    h = np.full(len(keys), 0x9E3779B9, np.uint32)
    for i in range(keys.shape[1]):
        h = mix_part(h, keys[:, i])
    return h


def weld_hash(records):
    """WeldKey: the packed record of a row (tests/ingest_ref.py: packed_records)"""
    return hash_bytes(records)


def edge_hash(lo, hi):
    """EdgeKey: the decoded vertices a side joins, lo <= hi"""
    return hash_pair(lo, hi)


def shell_vertex_hash(shell, vertex):
    """ShellVertexKey: the vertex goes in first"""
    return hash_pair(vertex, shell)


def crease_hash(vertex, root):
    """CreaseKey: the root goes in first"""
    return hash_pair(root, vertex)


def unweld_hash(keys):
    """UnweldKey: the rows of tests/render_ref.py: corner_keys (org, then a part per corner-target list)"""
    return hash_parts(keys)


# ---- the table
def slots_for(n: int) -> int:
    """DedupPlan::reserve: a power of two >= 2 n, 64 at least"""
    slots = 64
    while slots < 2 * n:
        slots <<= 1
    return slots


def table_census(homes, slots: int, k: int = 4) -> dict:
    """The table after the distinct keys with these home slots are in it (homes in ascending order of the keys' first items):
    "occupied": the sorted occupied slots -- with linear probing the set does not depend on the order of insertion;
    "longest_run": the longest cyclic run of occupied slots; "wraps": whether that run holds both slot slots - 1 and slot 0;
    "homes_in_last": the keys whose home is one of the last k slots; "max_displacement": the greatest distance from home of a key
    when the keys go in one after the other in the order given."""
    homes = np.asarray(homes, np.int64)
    assert slots & (slots - 1) == 0 and len(homes) < slots and (len(homes) == 0 or (0 <= homes.min() and homes.max() < slots))
    nxt = list(range(slots))   # nxt[s]: a slot at or cyclically after s that may be free (a union-find with path compression)

    def free_from(s):
        path = []
        while nxt[s] != s:
            path.append(s)
            s = nxt[s]
        for p in path:
            nxt[p] = s
        return s

    taken = np.zeros(slots, bool)
    worst = 0
    for h in homes.tolist():
        s = free_from(h)
        taken[s] = True
        nxt[s] = (s + 1) & (slots - 1)
        worst = max(worst, (s - h) & (slots - 1))
    longest, wraps = 0, False
    if taken.any():
        start = int(np.flatnonzero(~taken)[0])              # an empty slot: no run crosses it
        rolled = np.roll(taken, -start)
        edges = np.diff(np.concatenate([[0], rolled.astype(np.int8), [0]]))
        begin, end = np.flatnonzero(edges == 1), np.flatnonzero(edges == -1)
        i = int(np.argmax(end - begin))
        longest = int(end[i] - begin[i])
        first = (int(begin[i]) + start) % slots
        wraps = first != 0 and first + longest > slots
    return {"occupied": np.flatnonzero(taken), "longest_run": longest, "wraps": bool(wraps),
            "homes_in_last": int((homes >= slots - k).sum()), "max_displacement": int(worst)}


# ---- the numbering
def first_occurrence(keys):
    """rows (or items of a 1-D array) with equal keys share one id, ids in order of first occurrence, as tests/ingest_ref.py: weld
    numbers records: (id of every item u32 [n], first item of every id u32 [ids])"""
    keys = np.ascontiguousarray(keys)
    if len(keys) == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    if keys.ndim == 1:
        _, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    else:
        _, first, inv = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    return rank[inv.reshape(-1)].astype(np.uint32), first[order].astype(np.uint32)
