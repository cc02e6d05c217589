"""The first-occurrence numbering's probe paths, without a GPU: the numpy restatement of the five hashes (tests/dedup_ref.py) against
harry_amd/csrc/device/dedup_hash.hpp itself, compiled into tests/native/dedup_hash_check.cpp; the census and the table size of
dedup_ref on tables small enough to follow by hand; and the census every designed input of tests/dedup_cases.py is there for, so that
a change of a hash or of the table's size names the case that lost its property (tests/test_gpu_dedup.py runs them)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from harry_amd import codec as hc
from tests import dedup_cases as dc
from tests import dedup_ref as dr
from tests import ingest_ref as ir
from tests import render_ref as rr
from tests import util

FULL = 0xFFFFFFFF


# ---- 1. the restatement against the source
def _special_pairs():
    v = [0, 1, FULL, FULL - 1, 0x80000000, 0x9E3779B1, 12345]
    return np.array([(a, b) for a in v for b in v], np.uint32)   # (holds (0, 0), (FULL, FULL) and every other pair of equal parts)


def _records(rng):
    """records of many strides, as lists of uint8 arrays [n, stride]: random ones of stride 1, 4, 12, 36 and 7, and the special ones"""
    out = [rng.integers(0, 256, (3000, s), dtype=np.uint8) for s in (1, 4, 12, 36)] + [rng.integers(0, 256, (500, 7), dtype=np.uint8)]
    out.append(np.arange(256, dtype=np.uint8).reshape(256, 1))                    # every record of stride 1
    for s in (1, 4, 36):
        out.append(np.stack([np.zeros(s, np.uint8), np.full(s, 255, np.uint8), np.full(s, 0x5A, np.uint8)]))   # 0, all ones, equal bytes
    out.append(ir.packed_records([np.array([0.0, -0.0, 1.0, np.inf, np.nan], np.float32)] * 9))   # stride 36, equal parts
    out.append(np.zeros((1, 0), np.uint8))                                        # the empty record
    return out


def test_hashes_equal_the_source(tmp_path):
    """every form of dedup_hash.hpp on at least 10 000 random keys and on the special ones: 0, 0xffffffff, equal parts, records of
    stride 1 and of stride 36"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "dedup_hash_check")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(util.ROOT, "harry_amd", "csrc", "device"),
                        os.path.join(util.ROOT, "tests", "native", "dedup_hash_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rng = np.random.default_rng(11)
    lines, want, forms = [], [], []

    def add(form, text, hashes):
        assert len(text) == len(hashes)
        lines.extend(text)
        want.append(np.asarray(hashes, np.uint32))
        forms.extend([form] * len(text))

    for rec in _records(rng):
        add("weld", ["w " + (bytes(row).hex() or "-") for row in rec], dr.weld_hash(rec))
    pairs = np.concatenate([rng.integers(0, 1 << 32, (10000, 2), dtype=np.uint64).astype(np.uint32),
                            rng.integers(0, 5000, (2000, 2)).astype(np.uint32), _special_pairs()])
    for form, letter, fn in (("edge", "e", dr.edge_hash), ("shell_vertex", "s", dr.shell_vertex_hash), ("crease", "c", dr.crease_hash)):
        add(form, ["%s %d %d" % (letter, a, b) for a, b in pairs.tolist()], fn(pairs[:, 0], pairs[:, 1]))
    for parts in (1, 2, 3, 5):
        keys = np.concatenate([rng.integers(0, 1 << 32, (3000, parts), dtype=np.uint64).astype(np.uint32),
                               np.array([[0] * parts, [FULL] * parts, [7] * parts], np.uint32)])
        add("unweld", ["u %d %s" % (parts, " ".join(map(str, row))) for row in keys.tolist()], dr.unweld_hash(keys))
    add("unweld", ["u 2 %d %d" % (a, b) for a, b in _special_pairs().tolist()], dr.unweld_hash(_special_pairs()))
    counts = {f: forms.count(f) for f in set(forms)}
    assert sorted(counts) == ["crease", "edge", "shell_vertex", "unweld", "weld"] and min(counts.values()) >= 10000, counts
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.array(r.stdout.split(), np.uint64)
    want = np.concatenate(want)
    assert len(got) == len(want) == len(lines)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, [(forms[i], lines[i], int(got[i]), int(want[i])) for i in bad[:5]]
    # the three pair forms take their parts in different orders: the restatement has not collapsed them
    a, b = pairs[:, 0], pairs[:, 1]
    assert (dr.edge_hash(a, b) != dr.shell_vertex_hash(a, b))[a != b].all() and np.array_equal(dr.shell_vertex_hash(a, b), dr.crease_hash(a, b))
    assert np.array_equal(dr.edge_hash(a, b), dr.shell_vertex_hash(b, a))


# ---- 2. the table's size and the census, by hand
def test_slots_for_steps():
    """64 slots at least; the load is exactly 1/2 at n = 32, 2048, ... and 1/4 one item later"""
    assert [dr.slots_for(n) for n in (0, 1, 3, 32, 33, 64, 65, 2047, 2048, 2049, 4096, 4097)] == [64, 64, 64, 64, 128, 128, 256, 4096, 4096, 8192, 8192, 16384]
    for n in range(1, 5000):
        s = dr.slots_for(n)
        assert s >= 64 and s >= 2 * n and s & (s - 1) == 0 and (s == 64 or s // 2 < 2 * n)


def test_census_by_hand():
    c = dr.table_census([], 8)
    assert (len(c["occupied"]), c["longest_run"], c["wraps"], c["homes_in_last"], c["max_displacement"]) == (0, 0, False, 0, 0)
    c = dr.table_census([7, 7, 7], 8)                       # slots 7, 0, 1
    assert (c["occupied"].tolist(), c["longest_run"], c["wraps"], c["homes_in_last"], c["max_displacement"]) == ([0, 1, 7], 3, True, 3, 2)
    c = dr.table_census([0, 0, 5, 1], 8)                    # slots 0, 1, 5, 2: the run begins at slot 0 and does not wrap
    assert (c["occupied"].tolist(), c["longest_run"], c["wraps"], c["homes_in_last"], c["max_displacement"]) == ([0, 1, 2, 5], 3, False, 1, 1)
    c = dr.table_census([6, 2, 2, 6, 2, 6, 3], 8, 2)        # 6, 2, 3, 7, 4, 0, 5: slot 1 alone is free, the run goes from 2 round to 0
    assert (c["occupied"].tolist(), c["longest_run"], c["wraps"], c["homes_in_last"], c["max_displacement"]) == ([0, 2, 3, 4, 5, 6, 7], 7, True, 3, 2)
    c = dr.table_census([1, 1, 6], 8)                       # slots 1, 2, 6: nothing near the end
    assert (c["occupied"].tolist(), c["longest_run"], c["wraps"], c["homes_in_last"], c["max_displacement"]) == ([1, 2, 6], 2, False, 1, 1)
    c = dr.table_census([3, 7, 3, 7], 8)                    # two runs of two, the first found wins; the set is the same in any order
    assert c["occupied"].tolist() == dr.table_census([7, 7, 3, 3], 8)["occupied"].tolist() == [0, 3, 4, 7] and c["longest_run"] == 2
    rng = np.random.default_rng(2)
    homes = rng.integers(0, 64, 40)
    sets = [dr.table_census(rng.permutation(homes), 64)["occupied"].tolist() for _ in range(5)]
    assert all(s == sets[0] for s in sets) and len(sets[0]) == 40


def test_first_occurrence():
    ids, first = dr.first_occurrence(np.array([[5, 1], [2, 2], [5, 1], [0, 9], [2, 2]], np.uint32))
    assert ids.tolist() == [0, 1, 0, 2, 1] and first.tolist() == [0, 1, 3]
    ids, first = dr.first_occurrence(np.array([9, 9, 3, 9, 3], np.uint32))
    assert ids.tolist() == [0, 0, 1, 0, 1] and first.tolist() == [0, 2]
    rec = np.random.default_rng(1).integers(0, 3, (200, 4), dtype=np.uint8)
    a, b = dr.first_occurrence(rec), ir.weld(rec)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 3. the designed inputs have the properties they are there for
def one_wrapping_run(c, keys, items, slots):
    """all `keys` distinct keys of `items` items in a table of `slots` slots, one run from the last slots across slot 0"""
    assert (c["items"], c["keys"], c["slots"]) == (items, keys, slots), c
    assert c["homes_in_last"] == keys and c["longest_run"] == keys == len(c["occupied"]) and c["wraps"], c
    assert c["max_displacement"] >= keys - dc.LAST, c


@pytest.mark.parametrize("n,slots", [(3, 64), (32, 64), (33, 128), (2048, 4096)])
def test_case_weld_one_home(n, slots):
    (x,), c = dc.weld_one_home(n)
    assert x.dtype == np.float32 and len(np.unique(x)) == n and (x == np.floor(x)).all() and x.max() < dc.WELD_LIMIT
    one_wrapping_run(c, n, n, slots)
    assert c["max_displacement"] == n - 1 and c["occupied"].tolist() == sorted([slots - 1] + list(range(n - 1)))
    assert ((dr.weld_hash(ir.packed_records([x])) & np.uint32(slots - 1)) == slots - 1).all()


def test_case_weld_last_slots_dups():
    (x,), c = dc.weld_last_slots_dups()
    one_wrapping_run(c, 2048, 4096, 8192)
    ids, first = ir.weld(ir.packed_records([x]))
    assert np.bincount(ids).tolist() == [2] * 2048
    order = np.argsort(ids, kind="stable").reshape(2048, 2)           # the two rows of every key
    apart = int((order[:, 0] // 64 != order[:, 1] // 64).sum())
    print("keys whose two rows lie in different wavefronts:", apart)
    assert apart >= 1900
    assert len(np.unique(order // 64)) == 64 and (np.diff(first.astype(np.int64)) > 0).all() and first[-1] > 2048   # interleaved


def test_case_weld_stride36_one_home():
    cols, c = dc.weld_stride36_one_home()
    rec = ir.packed_records(cols)
    assert rec.shape == (512, 36) and len(cols) == 9
    one_wrapping_run(c, 512, 512, 1024)
    assert c["max_displacement"] == 511
    for k, col in enumerate(cols):
        assert col.dtype == np.float32 and (len(np.unique(col)) == 512 if k == dc.WIDE_SEARCHED else (col == col[0]).all() and col[0] != 0)


def test_case_edge_fan_one_cluster():
    pos, tris, c = dc.edge_fan_one_cluster()
    T = len(tris)
    assert (c["items"], c["slots"], c["keys"]) == (3 * T, 8192, 2 * T) and T >= 1024
    assert c["spokes_in_last"] == T and c["spoke_sides"] == [2]
    assert c["longest_run"] >= T and c["wraps"] and c["max_displacement"] >= T - dc.LAST, c
    assert np.isfinite(pos).all() and len(np.unique(pos[np.unique(tris)], axis=0)) == T + 1
    assert (tris[:, 0] == 0).all() and np.array_equal(tris[:, 2], np.roll(tris[:, 1], -1)) and (np.diff(tris[:, 1].astype(np.int64)) > 0).all()


@pytest.mark.parametrize("shells", [1, 2])
def test_case_shell_vertex_one_home(shells):
    pos, tris, c = dc.shell_vertex_one_home(shells)
    T = len(tris)
    assert (T, c["items"], c["slots"]) == (680, 2040, 4096)
    assert c["keys"] == T + 2 * shells == len(np.unique(tris)) and c["corners_in_last"] == 3 * T >= 1024
    one_wrapping_run(c, c["keys"], 3 * T, 4096)
    half = T // shells
    for s in range(shells):      # the strips: connected along their triangles, sharing no vertex with each other
        mine = tris[s * half:(s + 1) * half]
        assert all(len(set(mine[i]) & set(mine[i + 1])) == 2 for i in range(half - 1))
        assert not set(mine.reshape(-1).tolist()) & set(np.delete(tris, np.s_[s * half:(s + 1) * half], axis=0).reshape(-1).tolist())
    assert np.isfinite(pos).all() and len(np.unique(pos[np.unique(tris)], axis=0)) == c["keys"]


def test_case_unweld_one_home():
    obj, pairs, c = dc.unweld_one_home()
    one_wrapping_run(c, 1024, 2048, 4096)
    assert c["max_displacement"] == 1023
    assert pairs.shape == (2048, 2) and np.array_equal(pairs[:1024, 0], np.arange(1024)) and sorted(pairs[1024:, 0].tolist()) == list(range(1024))
    # ... and from the render build's own inputs: the keys the unweld's view derives from the mesh the reader made of the text
    mesh = hc.Mesh.from_obj(obj, "")
    assert rr.unwelded(mesh) and mesh.ne == 2048 and mesh.nf == 682
    keys = rr.corner_keys(mesh)
    assert keys.shape == (2048, 2) and np.array_equal(keys, pairs.astype(np.uint32))
    seen = dc.unweld_census(keys)
    assert {k: v for k, v in seen.items() if k != "occupied"} == {k: v for k, v in c.items() if k != "occupied"}
    assert np.array_equal(seen["occupied"], c["occupied"])
    faces = np.split(pairs[:, 0], np.cumsum(np.diff(mesh.face_offsets().astype(np.int64)))[:-1])
    assert all(len(set(f.tolist())) == len(f) for f in faces)


def test_case_crease_soup_one_home():
    pos, tris, c = dc.crease_soup_one_home()
    T = len(tris)
    one_wrapping_run(c, 3 * T, 3 * T, 4096)
    assert 3 * T == 2046 and len(np.unique(tris)) == 3 * T and tris.max() < dc.CREASE_LIMIT and np.isfinite(pos).all()
    keys = dc.crease_keys(tris, np.arange(3 * T))
    assert np.array_equal(keys[:, 1], np.arange(3 * T)) and np.array_equal(keys[:, 0], tris.reshape(-1))
    assert np.array_equal(dc.crease_keys([[4, 5, 6], [7, 5, 6]], [0, 1, 2, 3, 1, 2]), [[4, 0], [5, 1], [6, 2], [7, 3], [5, 1], [6, 2]])
