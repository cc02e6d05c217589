"""What of the hierarchy and the cast needs no GPU: the entry points of hry_bvh_build and hry_bvh_cast (include/harry_amd.h), and
the restatement of their contract (tests/bvh_ref.py) against closed forms, the tree's invariants, the monotonicity the skipping of
subtrees rests on, and a reference stack walk against the brute force.  tests/test_gpu_bvh.py holds the device to the same
restatement, bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import cli
from harry_amd import meshgen as mg
from tests import bvh_ref as br
from tests import seam_meshes as sm
from tests import util
from tests.test_creases_cpu import cube_triangles

HEADER = os.path.join(util.ROOT, "include", "harry_amd.h")
NAMES = ("build", "count", "get", "copy", "summary", "stat", "free", "cast")


def test_header_declares_and_library_exports():
    text = open(HEADER).read()
    L = nat.load()
    for name in NAMES:
        assert re.search(r"\bhry_bvh_%s\(" % name, text), name
        assert hasattr(L, "hry_bvh_" + name), name
    assert "typedef struct hry_bvh hry_bvh;" in text
    assert re.search(r"hry_bvh_build, hry_bvh_cast\s+\(no counterpart:", text)
    assert re.search(r"#define HRY_CAST_HOST\s+1u\b", text) and nat.CAST_HOST == 1
    assert re.search(r"#define HRY_ABI_VERSION\s+6\b", text) and L.hry_abi_version() == 6   # additive: the ABI stays
    assert "Not promised: watertightness" in text


def test_null_arguments_without_a_device():
    L = nat.load()
    out = C.c_void_p(1)
    assert L.hry_bvh_build(None, None, None, 0, C.byref(out)) == nat.E_ARG and not out.value
    assert L.hry_bvh_build(None, None, None, 0, None) == nat.E_ARG
    assert L.hry_bvh_count(None) == 0
    s = (C.c_uint64 * 6)()
    assert L.hry_bvh_summary(None, s) == nat.E_ARG and L.hry_bvh_stat(None, None, None) == nat.E_ARG
    rows = C.c_uint64()
    assert L.hry_bvh_get(None, b"leaf_tri", None, C.byref(rows), None, None) == nat.E_ARG
    assert L.hry_bvh_cast(None, None, 0, None, 0, None, 0, 0.0, 1.0, 0, None, None, None, None, None) == nat.E_ARG
    L.hry_bvh_free(None)


def test_the_option_is_in_the_usage_text():
    r = subprocess.run([cli.HARRY], capture_output=True, text=True, timeout=60)
    assert re.search(r"--bvh\s+Print the leaves", r.stdout), r.stdout


# ---- closed forms
def test_axis_ray_into_the_unit_cube():
    b = br.of_arrays(*cube_triangles())
    assert b["summary"] == (12, 12, 0, len(np.unique(b["leaf_code"])), b["summary"][4]) and 4 <= b["summary"][4] <= 11   # (twelve leaves: at least four levels)
    # from below at (3/4, 1/4): the bottom quad 0 2 3 1 is triangles 0 = (0, 2, 3) and 1 = (0, 3, 1); the point is 1/4 of the way to
    # corner 3 = (1, 1, 0) and 1/2 of the way to corner 1 = (1, 0, 0) from corner 0, inside triangle 1, one unit away -- all exact
    got = br.cast(b, [[0.75, 0.25, -1.0]], [[0.0, 0.0, 1.0]])
    assert got["tri"].tolist() == [1] and got["t"].tolist() == [1.0] and got["uv"].tolist() == [[0.25, 0.5]] and got["hits"] == 1
    # a window behind the near face: the far face, z = 1, two units away (the top quad 4 5 7 6: triangles 2 = (4, 5, 7), 3 = (4, 7, 6))
    got = br.cast(b, [[0.75, 0.25, -1.0]], [[0.0, 0.0, 1.0]], tmin=1.5)
    assert got["tri"].tolist() == [2] and got["t"].tolist() == [2.0] and got["uv"].tolist() == [[0.5, 0.25]]
    # from inside, and the other facing; the same ray with a -0 in a flat axis
    for d in ([0.0, 0.0, -1.0], [-0.0, 0.0, -1.0]):
        got = br.cast(b, [[0.75, 0.25, 0.5]], [d])
        assert got["tri"].tolist() == [1] and got["t"].tolist() == [0.5]
    # outside the cube's shadow, an empty window, a window that ends before the cube, invalid rays
    assert br.cast(b, [[1.5, 0.25, -1.0]], [[0.0, 0.0, 1.0]])["tri"].tolist() == [br.NO_ELEMENT]
    assert br.cast(b, [[0.75, 0.25, -1.0]], [[0.0, 0.0, 1.0]], tmin=3.0, tmax=2.0)["hits"] == 0
    assert br.cast(b, [[0.75, 0.25, -1.0]], [[0.0, 0.0, 1.0]], tmax=0.5)["hits"] == 0
    bad = br.cast(b, [[np.nan, 0.25, -1.0], [0.75, 0.25, -1.0], [0.75, 0.25, -1.0]], [[0.0, 0.0, 1.0], [0.0, -0.0, 0.0], [0.0, 0.0, np.inf]])
    assert bad["hits"] == 0 and np.isinf(bad["t"]).all() and not bad["uv"].any()


def test_one_triangle_and_two_coincident_ones():
    pos = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    one = br.build([[0, 1, 2]], pos)
    assert one["summary"] == (1, 1, 0, 1, 0) and one["node_children"].shape == (0, 2)
    cell = int(br.spread3(np.array([341]))[0])   # the centroid (1/3, 1/3, 0) in the box (0, 0, 0) .. (1, 1, 0): cells 341, 341 and, without extent, 0
    assert one["leaf_code"].tolist() == [cell << 2 | cell << 1]
    got = br.cast(one, [[0.25, 0.5, 2.0]], [[0.0, 0.0, -4.0]])
    assert got["tri"].tolist() == [0] and got["t"].tolist() == [0.5] and got["uv"].tolist() == [[0.25, 0.5]]
    assert br.walk(one, [0.25, 0.5, 2.0], [0.0, 0.0, -4.0])[:4] == (0, 0.5, 0.25, 0.5)
    two = br.build([[0, 1, 2], [0, 1, 2]], pos)   # the same code, the same box: the lower number wins, whichever leaf is met first
    assert two["summary"] == (2, 2, 0, 1, 1) and two["node_children"].tolist() == [[br.LEAF, br.LEAF | 1]]
    assert br.cast(two, [[0.25, 0.5, 2.0]], [[0.0, 0.0, -4.0]])["tri"].tolist() == [0]
    assert br.walk(two, [0.25, 0.5, 2.0], [0.0, 0.0, -4.0])[0] == 0
    flipped = br.build([[2, 1, 0], [0, 1, 2]], pos)   # both facings count
    assert br.cast(flipped, [[0.25, 0.5, 2.0]], [[0.0, 0.0, -4.0]])["tri"].tolist() == [0]
    none = br.build(np.zeros((0, 3), np.uint32), pos)
    assert none["summary"] == (0, 0, 0, 0, 0) and none["scene_box"].tolist() == [[np.inf] * 3 + [-np.inf] * 3]
    assert br.cast(none, [[0.25, 0.5, 2.0]], [[0.0, 0.0, -4.0]])["hits"] == 0


def test_dead_triangles_are_in_no_leaf():
    pos = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [0, np.inf, 1]])
    b = br.build([[0, 1, 3], [0, 1, 2], [4, 1, 2], [2, 1, 0]], pos)
    assert b["summary"] == (4, 2, 2, 1, 1) and b["leaf_tri"].tolist() == [1, 3] and np.isfinite(b["scene_box"]).all()


def test_codes_interleave_x_above_y_above_z():
    lo, hi = np.float32([0, 0, 0]), np.float32([1024, 1024, 1024])
    at = lambda x, y, z: int(br.codes_of(np.float32([[[x, y, z]] * 3]), lo, hi)[0])
    assert at(1, 0, 0) == 4 and at(0, 1, 0) == 2 and at(0, 0, 1) == 1 and at(2, 0, 0) == 32 and at(1023, 1023, 1023) == (1 << 30) - 1
    assert at(1024, 1024, 1024) == (1 << 30) - 1 and at(512.5, 0, 0) == 4 << 27   # the far face is clamped into the last cell
    flat = br.codes_of(np.float32([[[5, 7, 7]] * 3]), np.float32([0, 7, 7]), np.float32([10, 7, 7]))   # no extent: cell 0
    assert int(flat[0]) == int(br.spread3(np.array([512]))[0]) << 2


# ---- the tree
MESHES = {
    "torus": lambda: sm.gen_arrays(mg.torus(24, 16)),
    "flat_grid": lambda: (np.float32([[x, y, 0] for y in range(9) for x in range(9)]), np.full(128, 3, np.uint8),
                          np.array([t for y in range(8) for x in range(8) for t in ([9 * y + x, 9 * y + x + 1, 9 * y + x + 10], [9 * y + x, 9 * y + x + 10, 9 * y + x + 9])],
                                   np.uint32).reshape(-1)),
    "copies": lambda: (np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.full(70, 3, np.uint8), np.tile(np.arange(3, dtype=np.uint32), 70)),
}


def nan_torus():
    pos, deg, idx = MESHES["torus"]()
    pos = pos.copy()
    pos[100, 1] = np.nan
    return pos, deg, idx


@pytest.mark.parametrize("name", sorted(MESHES) + ["nan_torus"])
def test_tree_invariants(name):
    b = br.of_arrays(*(nan_torus() if name == "nan_torus" else MESHES[name]()))
    T, L, dead, distinct, depth = b["summary"]
    assert L == T - dead and (dead > 0) == (name == "nan_torus") and len(b["node_children"]) == L - 1 and 1 <= depth <= 62
    assert (np.diff(b["leaf_code"].astype(np.int64) * (1 << 32) + b["leaf_tri"]) > 0).all()   # ascending (code, t)
    kids, ranges = b["node_children"], b["ranges"]
    leaves = kids[(kids & br.LEAF) != 0] & ~np.uint32(br.LEAF)
    inner = kids[(kids & br.LEAF) == 0]
    assert sorted(leaves.tolist()) == list(range(L)) and sorted(inner.tolist()) == list(range(1, L - 1))   # each once; the root is no child
    assert ranges[0].tolist() == [0, L - 1]
    for node, (a, z) in enumerate(ranges.tolist()):
        assert node in (a, z)   # Karras: a node's number is an end of its range ...
        (l, r) = kids[node].tolist()
        gamma = l & ~br.LEAF
        assert r & ~br.LEAF == gamma + 1 and a <= gamma < z   # ... and its children's numbers are its split
        assert (ranges[gamma].tolist() == [a, gamma]) if not l & br.LEAF else a == gamma
        assert (ranges[gamma + 1].tolist() == [gamma + 1, z]) if not r & br.LEAF else gamma + 1 == z
        box = np.concatenate([b["leaf_box"][a:z + 1, :3].min(axis=0), b["leaf_box"][a:z + 1, 3:].max(axis=0)])
        assert np.array_equal(b["node_box"][node], box)   # the box of a node is the box of its leaves
    assert np.array_equal(b["node_box"][0], b["scene_box"][0])
    if name == "copies":   # one code: the tree rests on the position bits alone, and is balanced over them
        assert distinct == 1 and depth == 7


# ---- the interval
def test_the_interval_is_monotone_on_nested_boxes():
    """a box that contains another has a near no greater and a far no smaller, exactly, and passes wherever the inner one does: what
    lets the walk skip a subtree (DESIGN.md "Bvh")"""
    rng = np.random.default_rng(11)
    n = 4000
    c, h = rng.normal(size=(n, 3)), rng.uniform(0, 1, (n, 3)) * rng.choice([0.0, 1e-6, 1.0], (n, 3))
    inner = np.concatenate([c - h, c + h], axis=1).astype(np.float32)
    grow = rng.uniform(0, 1, (n, 6)) * rng.choice([0.0, 1e-7, 1.0], (n, 6))
    outer = np.concatenate([np.minimum(inner[:, :3], (inner[:, :3] - grow[:, :3]).astype(np.float32)),
                            np.maximum(inner[:, 3:], (inner[:, 3:] + grow[:, 3:]).astype(np.float32))], axis=1)
    O = (c + rng.normal(size=(n, 3)) * rng.choice([0.0, 1.0, 30.0], (n, 1))).astype(np.float32)
    O[::7] = inner[::7, :3]   # origins on a face, an edge, a corner
    D = (rng.normal(size=(n, 3)) * rng.choice([0.0, 1e-30, 1.0], (n, 3))).astype(np.float32)
    D[::2][(rng.uniform(size=(len(D[::2]), 3)) < 0.3)] = -0.0
    D[~(D != 0).any(axis=1)] = np.float32([0, 1, 0])
    assert br.valid_rays(O, D).all()
    seen = 0
    for tmin, tmax in ((0.0, np.inf), (-np.inf, np.inf), (0.5, 2.0)):
        for i in range(n):
            pi, ni, fi = br.interval(inner[i:i + 1], O[i:i + 1].astype(np.float64), D[i:i + 1].astype(np.float64), tmin, tmax)
            po, no, fo = br.interval(outer[i:i + 1], O[i:i + 1].astype(np.float64), D[i:i + 1].astype(np.float64), tmin, tmax)
            assert not np.isnan([ni[0, 0], fi[0, 0], no[0, 0], fo[0, 0]]).any()
            if pi[0, 0]:
                assert po[0, 0] and no[0, 0] <= ni[0, 0] and fo[0, 0] >= fi[0, 0], (i, inner[i], outer[i], O[i], D[i])
                seen += 1
    assert seen > n // 2   # the inner box passes often enough for the comparison to mean something


# ---- the walk
@pytest.mark.parametrize("name", ["torus", "flat_grid", "nan_torus"])
def test_the_walk_agrees_with_the_brute_force_and_prunes(name):
    b = br.of_arrays(*(nan_torus() if name == "nan_torus" else MESHES[name]()))
    L = b["summary"][1]
    o, d = br.ray_set(b, 3000, seed=3)
    want = br.cast(b, o, d)
    assert 3000 // 4 <= want["hits"] <= 3000 - 3000 // 4, want["hits"]   # the set hits with a quarter of its rays and misses with a quarter
    some = np.arange(0, 3000, 10)
    tests = []
    for i in some:
        tri, t, u, v, made = br.walk(b, o[i], d[i])
        assert (tri, t.view(np.uint32), u.view(np.uint32), v.view(np.uint32)) == \
               (want["tri"][i], want["t"][i].view(np.uint32), want["uv"][i, 0].view(np.uint32), want["uv"][i, 1].view(np.uint32)), i
        tests.append(made)
    assert np.mean(tests) <= (2 * L - 1) / 4, np.mean(tests)   # a walk that prunes nothing makes 2 L - 2 of them
    print(name, "hits", want["hits"], "box tests per ray", np.mean(tests), "of", 2 * L - 1, "nodes")


def test_a_window_returns_the_second_hit():
    b = br.of_arrays(*MESHES["torus"]())
    o, d = br.ray_set(b, 600, seed=5)
    first = br.cast(b, o, d)
    cut = float(np.median(first["t"][first["tri"] != br.NO_ELEMENT]))
    second = br.cast(b, o, d, tmin=cut)
    moved = (first["tri"] != br.NO_ELEMENT) & (first["t"] < cut)
    assert moved.sum() > 50 and (second["tri"][moved] != first["tri"][moved]).all() and (second["tri"][moved] != br.NO_ELEMENT).sum() > 25
    assert (second["t"][second["tri"] != br.NO_ELEMENT] >= np.float32(cut)).all()
    kept = first["t"] > cut   # (the misses too; the ray whose rounded t is the cut itself may lie on either side)
    assert np.array_equal(second["tri"][kept], first["tri"][kept])
