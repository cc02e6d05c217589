"""What of the closest-point query needs no GPU: the entry point of hry_bvh_nearest (include/harry_amd.h), and the restatement of
its contract (tests/nearest_ref.py) against closed forms, degenerate triangles, the monotonicity of the bound that the skipping of
subtrees rests on, and a reference stack walk against the brute force.  tests/test_gpu_nearest.py holds the device to the same
restatement, bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import cli
from tests import bvh_ref as br
from tests import nearest_ref as nr
from tests import util
from tests.test_bvh_cpu import MESHES, nan_torus
from tests.test_creases_cpu import cube_triangles

HEADER = os.path.join(util.ROOT, "include", "harry_amd.h")


def test_header_declares_and_library_exports():
    text = open(HEADER).read()
    L = nat.load()
    assert re.search(r"\bint hry_bvh_nearest\(hry_ctx \*ctx, const hry_bvh \*b, uint64_t n_points, const float \*points, uint64_t point_stride,", text)
    assert hasattr(L, "hry_bvh_nearest")
    assert re.search(r"#define HRY_NEAREST_HOST\s+1u\b", text) and nat.NEAREST_HOST == 1
    assert re.search(r"hry_bvh_nearest\s+\(no counterpart:", text)
    assert "ties to the least triangle number" in text and "d2_t = max(that d2, the bound of t's own leaf box)" in text


def test_the_abi_version_stays():
    text = open(HEADER).read()
    assert re.search(r"#define HRY_ABI_VERSION\s+6\b", text) and nat.load().hry_abi_version() == 6   # additive: the ABI stays


def test_null_arguments_without_a_device():
    L = nat.load()
    assert L.hry_bvh_nearest(None, None, 0, None, 0, 1.0, 0, None, None, None, None, None, None) == nat.E_ARG
    assert L.hry_bvh_nearest(None, None, 4, None, 12, float("inf"), nat.NEAREST_HOST, None, None, None, None, None, None) == nat.E_ARG
    assert "null argument" in L.hry_last_error().decode()


def test_the_option_is_in_the_usage_text():
    r = subprocess.run([cli.HARRY], capture_output=True, text=True, timeout=60)
    assert re.search(r"--deviation\s+Print the surface deviation", r.stdout), r.stdout


# ---- closed forms, all exact
def one(bvh, q, max_dist=np.inf):
    """(tri, d2, uv, point) of one point, by the brute force -- and the walk must say the same"""
    got = nr.nearest(bvh, [q], max_dist)
    w = nr.walk(bvh, q, max_dist)
    assert (w[0], float(w[1]), [float(w[2]), float(w[3])], w[4].tolist()) == (int(got["tri"][0]), float(got["d2"][0]), got["uv"][0].tolist(), got["point"][0].tolist())
    return int(got["tri"][0]), float(got["d2"][0]), got["uv"][0].tolist(), got["point"][0].tolist()


def test_points_about_the_unit_cube():
    b = br.of_arrays(*cube_triangles())
    # the bottom quad 0 2 3 1 is triangles 0 = (0, 2, 3) and 1 = (0, 3, 1); the top quad 4 5 7 6 is 2 = (4, 5, 7) and 3 = (4, 7, 6)
    # below the bottom face at (3/4, 1/4): inside triangle 1, 1/4 of the way to corner 3 and 1/2 of the way to corner 1, one unit away
    assert one(b, [0.75, 0.25, -1.0]) == (1, 1.0, [0.25, 0.5], [0.75, 0.25, 0.0])
    # beyond the edge from corner 0 to corner 1 = (1, 0, 0): its midpoint, on segment (P2, P0) of triangle 1 -- the side face at y = 0
    # shares the edge and the distance, and has the greater numbers
    assert one(b, [0.5, -1.0, -1.0]) == (1, 2.0, [0.0, 0.5], [0.5, 0.0, 0.0])
    # beyond corner 0: the corner itself, P0 of triangle 0
    assert one(b, [-1.0, -1.0, -1.0]) == (0, 3.0, [0.0, 0.0], [0.0, 0.0, 0.0])
    # on corner 7 = (1, 1, 1), which six triangles share: the least number, the top's triangle 2, whose P2 it is
    assert one(b, [1.0, 1.0, 1.0]) == (2, 0.0, [0.0, 1.0], [1.0, 1.0, 1.0])
    # inside the cube: the nearest face
    assert one(b, [0.75, 0.25, 0.125])[:2] == (1, 0.015625)
    # the radius: an answer exactly at it is accepted, one beyond it is not; a negative radius answers nothing; invalid points
    assert one(b, [0.75, 0.25, -1.0], 1.0)[0] == 1 and one(b, [0.75, 0.25, -1.0], 0.999)[0] == br.NO_ELEMENT
    assert one(b, [1.0, 1.0, 1.0], 0.0)[:2] == (2, 0.0) and one(b, [1.0, 1.0, 1.0], -1.0)[0] == br.NO_ELEMENT
    bad = nr.nearest(b, [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]])
    assert bad["answered"] == 0 and bad["max_bits"] == 0 and np.isinf(bad["d2"]).all() and not bad["uv"].any() and not bad["point"].any()
    assert (bad["tri"] == br.NO_ELEMENT).all()
    far = nr.nearest(b, [[0.75, 0.25, -1.0], [0.5, -1.0, -1.0], [np.nan, 0, 0]])
    assert far["answered"] == 2 and far["max_bits"] == int(np.float64(2.0).view(np.uint64))


def test_one_triangle():
    pos = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    b = br.build([[0, 1, 2]], pos)
    assert one(b, [0.25, 0.5, 2.0]) == (0, 4.0, [0.25, 0.5], [0.25, 0.5, 0.0])      # above the face
    assert one(b, [0.25, 0.5, -2.0]) == (0, 4.0, [0.25, 0.5], [0.25, 0.5, 0.0])     # ... and below: both facings
    assert one(b, [0.5, -1.0, 0.0]) == (0, 1.0, [0.5, 0.0], [0.5, 0.0, 0.0])        # beyond the edge (P0, P1)
    assert one(b, [1.0, 1.0, 0.0]) == (0, 0.5, [0.5, 0.5], [0.5, 0.5, 0.0])         # beyond the edge (P1, P2)
    assert one(b, [-1.0, 0.25, 0.0]) == (0, 1.0, [0.0, 0.25], [0.0, 0.25, 0.0])     # beyond the edge (P2, P0)
    assert one(b, [2.0, 0.0, 0.0]) == (0, 1.0, [1.0, 0.0], [1.0, 0.0, 0.0])         # beyond the corner P1: segment (P0, P1) comes first
    assert one(b, [0.0, 3.0, 0.0]) == (0, 4.0, [0.0, 1.0], [0.0, 1.0, 0.0])         # beyond the corner P2
    none = br.build(np.zeros((0, 3), np.uint32), pos)
    assert one(none, [0.25, 0.5, 2.0]) == (br.NO_ELEMENT, np.inf, [0.0, 0.0], [0.0, 0.0, 0.0])
    two = br.build([[0, 1, 2], [0, 1, 2]], pos)   # the same triangle twice: the lower number, whichever leaf is met first
    assert one(two, [0.25, 0.5, 2.0])[0] == 0
    flipped = br.build([[2, 1, 0], [0, 1, 2]], pos)
    assert one(flipped, [0.25, 0.5, 2.0])[:2] == (0, 4.0)


def test_degenerate_triangles_answer_as_what_they_are():
    pos = np.float32([[0, 0, 0], [0, 0, 0], [1, 0, 0]])   # two equal corners: the segment from (0, 0, 0) to (1, 0, 0)
    seg = br.build([[0, 1, 2]], pos)
    assert one(seg, [0.5, 1.0, 0.0]) == (0, 1.0, [0.5, 0.5], [0.5, 0.0, 0.0])       # segment (P1, P2) at s = 1/2: (u, v) = (1 - s, s)
    assert one(seg, [-1.0, 0.0, 0.0]) == (0, 1.0, [0.0, 0.0], [0.0, 0.0, 0.0])      # segment (P0, P1) has no length: s = 0
    assert one(seg, [3.0, 0.0, 0.0]) == (0, 4.0, [0.0, 1.0], [1.0, 0.0, 0.0])
    thin = br.build([[0, 1, 2]], np.float32([[0, 0, 0], [2, 0, 0], [1, 0, 0]]))     # three corners in a line: no normal either
    assert one(thin, [1.5, 2.0, 0.0])[:2] == (0, 4.0) and one(thin, [1.5, 2.0, 0.0])[3] == [1.5, 0.0, 0.0]
    pt = br.build([[0, 1, 2]], np.float32([[1, 2, 3]] * 3))                        # three equal corners: a point
    assert one(pt, [1.0, 2.0, 5.0]) == (0, 4.0, [0.0, 0.0], [1.0, 2.0, 3.0])
    assert one(pt, [1.0, 2.0, 3.0]) == (0, 0.0, [0.0, 0.0], [1.0, 2.0, 3.0])


# ---- the bound
def test_the_bound_is_monotone_on_nested_boxes():
    """a box that contains another has a bound no greater, exactly: what lets the walk skip a subtree (DESIGN.md "Bvh")"""
    rng = np.random.default_rng(11)
    n = 4000
    c, h = rng.normal(size=(n, 3)), rng.uniform(0, 1, (n, 3)) * rng.choice([0.0, 1e-6, 1.0], (n, 3))
    inner = np.concatenate([c - h, c + h], axis=1).astype(np.float32)
    grow = rng.uniform(0, 1, (n, 6)) * rng.choice([0.0, 1e-7, 1.0], (n, 6))
    outer = np.concatenate([np.minimum(inner[:, :3], (inner[:, :3] - grow[:, :3]).astype(np.float32)),
                            np.maximum(inner[:, 3:], (inner[:, 3:] + grow[:, 3:]).astype(np.float32))], axis=1)
    Q = (c + rng.normal(size=(n, 3)) * rng.choice([0.0, 1.0, 30.0, 1e30], (n, 1))).astype(np.float32)
    Q[::7] = inner[::7, :3]   # points on a face, an edge, a corner
    assert nr.valid_points(Q).all()
    bi = np.array([nr.bound(inner[i:i + 1], Q[i:i + 1].astype(np.float64))[0, 0] for i in range(n)])
    bo = np.array([nr.bound(outer[i:i + 1], Q[i:i + 1].astype(np.float64))[0, 0] for i in range(n)])
    assert not np.isnan(bi).any() and not np.isnan(bo).any() and (bo <= bi).all() and (bi >= 0).all()
    assert (bi > 0).sum() > n // 2 and (bo < bi).sum() > n // 8 and (bi == 0).sum() > n // 16   # the comparison means something
    assert [nr._bound(inner[i].astype(np.float64).tolist(), Q[i].astype(np.float64).tolist()) for i in range(0, n, 40)] == bi[::40].tolist()
    huge = nr.bound(np.float32([[-3e38, -3e38, -3e38, -3e38, -3e38, -3e38]]), np.float64([[3e38, 3e38, 3e38]]))[0, 0]
    assert np.isfinite(huge) and huge > 1e78   # beyond the floats, far inside the doubles


def test_a_triangle_is_never_nearer_than_its_box():
    """d2_t >= the bound of its own leaf box >= the bound of every box above: the chain the skipping rests on, on a real tree"""
    b = br.of_arrays(*MESHES["torus"]())
    pts = nr.point_set(b, 400, seed=5).astype(np.float64)
    dt = nr.triangle(b["leaf_positions"], b["leaf_box"], pts)[0]
    leaf_bound, node_bound = nr.bound(b["leaf_box"], pts), nr.bound(b["node_box"], pts)
    assert (dt >= leaf_bound).all()
    for node, (a, z) in enumerate(b["ranges"].tolist()):
        assert (node_bound[:, node:node + 1] <= leaf_bound[:, a:z + 1]).all(), node


# ---- the walk
@pytest.fixture(scope="module")
def torus_set():
    b = br.of_arrays(*MESHES["torus"]())
    pts = nr.point_set(b, 2000, seed=3)
    return b, pts, nr.nearest(b, pts)


def same_answer(w, want, i):
    return (w[0], w[1].view(np.uint64), w[2].view(np.uint32), w[3].view(np.uint32), w[4].view(np.uint32).tolist()) == \
           (want["tri"][i], want["d2"][i].view(np.uint64), want["uv"][i, 0].view(np.uint32), want["uv"][i, 1].view(np.uint32), want["point"][i].view(np.uint32).tolist())


@pytest.mark.parametrize("name", ["torus", "flat_grid", "nan_torus"])
def test_the_walk_agrees_with_the_brute_force_and_prunes(name, torus_set):
    if name == "torus":
        b, pts, want = torus_set
    else:
        b = br.of_arrays(*(nan_torus() if name == "nan_torus" else MESHES[name]()))
        pts = nr.point_set(b, 2000, seed=3)
        want = nr.nearest(b, pts)
    L = b["summary"][1]
    assert want["answered"] == len(pts)
    tests = []
    for i in range(len(pts)):
        w = nr.walk(b, pts[i])
        assert same_answer(w, want, i), (i, w, want["tri"][i], want["d2"][i])
        tests.append(w[5])
    print(name, "bounds per point", np.mean(tests), "of", 2 * L - 1, "nodes")
    if name == "torus":
        assert np.mean(tests) <= (2 * L - 1) / 4, np.mean(tests)   # a walk that prunes nothing evaluates 2 L - 2


def test_the_set_and_a_radius(torus_set):
    b, pts, want = torus_set
    assert (want["d2"] == 0).sum() >= len(pts) // 8, (want["d2"] == 0).sum()   # the corners, where several triangles tie
    radius = float(np.sqrt(np.median(want["d2"][want["d2"] > 0])))
    within = nr.nearest(b, pts, radius)
    assert len(pts) // 4 <= within["answered"] <= len(pts) - len(pts) // 4, within["answered"]
    keep = want["d2"] <= np.float64(radius) * np.float64(radius)
    assert np.array_equal(within["tri"], np.where(keep, want["tri"], br.NO_ELEMENT)) and np.array_equal(within["d2"], np.where(keep, want["d2"], np.inf))
    for i in range(0, len(pts), 5):
        assert same_answer(nr.walk(b, pts[i], radius), within, i), i
    none = nr.nearest(b, pts, -1.0)
    assert none["answered"] == 0 and none["max_bits"] == 0
    zero = nr.nearest(b, pts, 0.0)
    assert zero["answered"] == int((want["d2"] == 0).sum()) and zero["max_bits"] == 0
    print("answered within the median radius", within["answered"], "at distance 0", zero["answered"])
