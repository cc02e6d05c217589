"""What of the self-intersection build needs no GPU: the entry points of hry_intersections_build (include/harry_amd.h), and the
restatement of its contract (tests/intersections_ref.py) against closed forms and a reference stack walk against the brute force.
tests/test_gpu_intersections.py holds the device to the same restatement, bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import cli
from harry_amd import meshgen as mg
from tests import bvh_ref as br
from tests import intersections_ref as ir
from tests import seam_meshes as sm
from tests import util

HEADER = os.path.join(util.ROOT, "include", "harry_amd.h")


def test_header_declares_and_library_exports():
    text = open(HEADER).read()
    L = nat.load()
    assert re.search(r"\bint hry_intersections_build\(hry_ctx \*ctx, const hry_bvh \*b, uint32_t flags, hry_intersections \*\*out\);", text)
    for what in ("build", "count", "get", "copy", "summary", "stat", "free"):
        assert re.search(r"\bhry_intersections_%s\(" % what, text) and hasattr(L, "hry_intersections_" + what), what
    assert re.search(r"hry_intersections_build\s+\(no counterpart:", text)
    assert "lo_t <= hi_s and lo_s <= hi_t" in text and "coplanar overlaps are not found" in text and "touching counts" in text


def test_the_abi_version_stays():
    text = open(HEADER).read()
    assert re.search(r"#define HRY_ABI_VERSION\s+6\b", text) and nat.load().hry_abi_version() == 6   # additive: the ABI stays
    assert hasattr(nat.load(), "hry_intersections_build")


def test_null_arguments_without_a_device():
    import ctypes as C
    L = nat.load()
    out = C.c_void_p(77)
    assert L.hry_intersections_build(None, None, 0, C.byref(out)) == nat.E_ARG and out.value is None
    assert "null argument" in L.hry_last_error().decode()
    assert L.hry_intersections_build(None, None, 0, None) == nat.E_ARG
    assert L.hry_intersections_count(None) == 0
    assert L.hry_intersections_summary(None, (C.c_uint64 * 6)()) == nat.E_ARG and "null argument" in L.hry_last_error().decode()
    L.hry_intersections_free(None)


def test_the_option_is_in_the_usage_text():
    r = subprocess.run([cli.HARRY], capture_output=True, text=True, timeout=60)
    assert re.search(r"--intersections\s+Print the triangle pairs that pass through each other", r.stdout), r.stdout


# ---- closed forms, all exact
A = [0, 0, 0, 2, 0, 0, 0, 2, 0]


def both(bvh):
    """the brute force -- and the walk must say the same"""
    got = ir.intersections(bvh)
    w, tests = ir.walk(bvh)
    for k in ir.BUFFERS:
        assert np.array_equal(got[k], w[k]), k
    assert got["summary"] == w["summary"]
    return got


def against_a(second, first=A):
    got = both(ir.of_triangles([first, second]))
    T, C, N, P, H = got["summary"]
    assert T == 2 and P == len(got["pairs"]) == len(got["pair_shared"]) and H == (2 if P else 0) and got["tri_pairs"].tolist() == [P, P]
    assert got["pairs"].tolist() == ([[0, 1]] if P else [])
    swapped = ir.intersections(ir.of_triangles([second, first]))   # no test depends on which triangle is called the first
    assert swapped["summary"] == got["summary"] and np.array_equal(swapped["pair_shared"], got["pair_shared"])
    return C, N, P, got["pair_shared"].tolist()


CLOSED = {
    "pierced": ([.5, .5, -1, .5, .5, 1, 3, 3, .5], (1, 1, 1, [0])),
    "one_corner_opposite_edge_through": ([0, 0, 0, .5, .5, -1, .5, .5, 1], (1, 1, 1, [1])),
    "one_corner_written_with_negative_zeros": ([-0.0, 0, -0.0, .5, .5, -1, .5, .5, 1], (1, 1, 1, [1])),
    "one_corner_leaning_away": ([0, 0, 0, -1, -1, -1, -1, -1, 1], (1, 1, 0, [])),
    "an_edge_shared_folded_flat": ([0, 0, 0, 2, 0, 0, 0, 1, 0], (1, 0, 0, [])),
    "coplanar_overlap": ([.5, .5, 0, 3, .5, 0, .5, 3, 0], (1, 1, 0, [])),
    "a_corner_on_the_face": ([.5, .5, 0, .5, .5, 1, 1, 1, 1], (1, 1, 1, [0])),
    "boxes_overlap_only": ([1.9, 1.9, -1, 1.9, 1.9, 1, 1.5, 1.9, 0], (1, 1, 0, [])),
    "improper_segment_through": ([.5, .5, -1, .5, .5, 1, .5, .5, 1], (1, 0, 0, [])),
}


@pytest.mark.parametrize("name", sorted(CLOSED))
def test_closed_forms(name):
    second, want = CLOSED[name]
    assert against_a(second) == want


def test_more_closed_forms():
    assert against_a([5, 5, 5, 6, 5, 5, 5, 6, 5]) == (0, 0, 0, [])                          # boxes apart
    assert against_a(A) == (1, 0, 0, [])                                                  # all three corners shared: never tested
    assert against_a([0, 2, 0, 2, 0, 0, 0, 0, 0]) == (1, 0, 0, [])                         # ... in another order
    assert against_a([1, -1, -1, 1, -1, 1, 1, 1, 0]) == (1, 1, 1, [0])                     # an edge of A through the other's face ... corner (1, 1, 0) on A's edge
    assert against_a([1, 0, -1, 1, 0, 1, 1, -3, 0]) == (1, 1, 1, [0])                      # edge against edge: touching counts
    none = ir.intersections(ir.of_triangles(np.zeros((0, 9))))
    assert none["summary"] == (0, 0, 0, 0, 0) and none["pairs"].shape == (0, 2) and none["tri_pairs"].shape == (0,)
    dead = ir.intersections(ir.of_triangles([A, [.5, .5, -1, .5, .5, np.nan, 3, 3, .5]]))   # a dead triangle is no leaf
    assert dead["summary"] == (2, 0, 0, 0, 0) and dead["tri_pairs"].tolist() == [0, 0]


# ---- the walk
def torus_pos(n=24, m=16):
    pos, deg, idx = sm.gen_arrays(mg.torus(n, m))
    return np.asarray(pos, np.float32), br.fan_triangles(deg, np.asarray(idx, np.uint32))


def two_tori(kind):
    """the torus beside its copy: "rings" -- the axes cycled (z, x, y) and moved by (1, 0, 0), two linked rings --, "shifted" -- moved
    by (0.3, 0.1, 0.05)"""
    pos, tri = torus_pos()
    other = (pos[:, [2, 0, 1]] + np.float32([1, 0, 0])) if kind == "rings" else (pos + np.float32([0.3, 0.1, 0.05]))
    return np.concatenate([pos, other.astype(np.float32)]), np.concatenate([tri, tri + np.uint32(len(pos))])


@pytest.mark.parametrize("kind", ["torus", "rings"])
def test_the_walk_agrees_with_the_brute_force_and_prunes(kind):
    if kind == "torus":
        pos, tri = torus_pos()
    else:
        pos, tri = two_tori(kind)
    b = br.build(tri, pos)
    want = ir.intersections(b)
    got, tests = ir.walk(b)
    for k in ir.BUFFERS:
        assert np.array_equal(got[k], want[k]), k
    assert got["summary"] == want["summary"]
    L = b["summary"][1]
    print(kind, "summary", want["summary"], "box tests per leaf", tests / L, "of", 2 * L - 1, "nodes")
    assert L == len(tri) and 0 < tests / L <= (2 * L - 1) / 8, tests / L   # a walk that prunes nothing makes 2 L - 2 a leaf
    T, C, N, P, H = want["summary"]
    assert (P, C) == ((0, 4903) if kind == "torus" else (152, 10562)), want["summary"]
    assert (want["pairs"][:, 0] < want["pairs"][:, 1]).all() and want["tri_pairs"].sum() == 2 * P
    if kind == "rings":   # every pair has a triangle of either ring, and the order is the lexicographic one
        assert (want["pairs"][:, 0] < T // 2).all() and (want["pairs"][:, 1] >= T // 2).all() and not want["pair_shared"].any()
        keys = want["pairs"][:, 0].astype(np.uint64) << np.uint64(32) | want["pairs"][:, 1]
        assert (np.diff(keys.astype(np.int64)) > 0).all()
