"""The pairs of triangles that pass through each other (include/harry_amd.h: hry_intersections_build; kernel:
harry_amd/csrc/device/bvh.hip, k_bvh_pairs) against the numpy restatement of tests/intersections_ref.py, which tests every leaf
against every leaf.  The pairs, the corners they share, the counts per triangle and T, C, N, P, H are compared bit for bit; nothing
is left out and nothing has a tolerance (the sixth summary word, which depends on the walk, is held to the pruning bound instead)."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import cli
from harry_amd import codec as hc
from harry_amd import meshgen as mg
from tests import bvh_ref as br
from tests import intersections_ref as ir
from tests import nearest_ref as nr
from tests import util
from tests.test_creases_cpu import CUBE_POS, CUBE_QUADS
from tests.test_gpu_bvh import MESHES as BVH_MESHES
from tests.test_gpu_bvh import check_build, same_bits
from tests.test_gpu_creases import gen, mesh_of
from tests.test_intersections_cpu import CLOSED, A, two_tori

pytestmark = pytest.mark.gpu

PAIRS_BLOCK = 64   # bvh.hip: kCastBlock, the leaves of one workgroup of the walk


@pytest.fixture(scope="module")
def cx():
    c = hc.Codec(0)
    yield c
    c.close()


def soup(triangles):
    """triangles given as nine floats each, on vertices of their own"""
    pos = np.asarray(triangles, np.float32).reshape(-1, 3)
    return mesh_of((pos, np.full(len(pos) // 3, 3, np.uint8), np.arange(len(pos), dtype=np.uint32)))


def check_intersections(b, want, label, ref=None):
    """one build against the restatement: every buffer and the summary; returns (the restatement, the Intersections)"""
    x = b.intersections()
    got = x.buffers_numpy()
    ref = ir.intersections(want) if ref is None else ref
    assert sorted(got) == sorted(hc.Intersections.BUFFERS) == sorted(ir.BUFFERS)
    for k in ir.BUFFERS:
        assert same_bits(got[k], ref[k]), (label, k, got[k].shape, ref[k].shape)
    st = x.stat()
    assert (x.triangles, x.candidates, x.tested, x.pairs, x.triangles_hit) == ref["summary"] == tuple(st[k] for k in ir.SUMMARY), (label, st, ref["summary"])
    assert x.count() == ref["summary"][3] and st["uploaded_bytes"] == 0 and x.device_ms > 0 and st["box_tests"] == x.box_tests
    return ref, x


def run_mesh(cx, mesh, label):
    want, b = check_build(cx, mesh, label)
    ref, x = check_intersections(b, want, label)
    b.close()
    return want, ref, x


# ---- 1. nothing to find: empty results with the right shapes
@pytest.mark.parametrize("name", ["no_leaf", "one_leaf", "two_leaves", "three_leaves", "a_point", "dead_in_a_tile"])
def test_empty_results(cx, name):
    want, ref, x = run_mesh(cx, BVH_MESHES[name](), name)
    T, L = want["summary"][:2]
    got = x.buffers_numpy()
    assert ref["summary"][3] == 0 and got["pairs"].shape == (0, 2) and got["pair_shared"].shape == (0,) and got["tri_pairs"].shape == (T,) and not got["tri_pairs"].any()
    assert x.triangles == T and x.triangles_hit == 0 and (x.box_tests > 0) == (L > 1)
    if name == "a_point":
        assert x.candidates == L * (L - 1) // 2 and x.tested == 0   # five coincident points: every box overlaps, none is proper
    x.close()


def test_one_code(cx):
    """1 025 coincident triangles: the walk prunes nothing here and must still end"""
    want, ref, x = run_mesh(cx, BVH_MESHES["one_code"](), "one_code")
    assert (x.candidates, x.tested, x.pairs) == (1025 * 1024 // 2, 0, 0)
    x.close()


# ---- 2. the closed forms through the device
@pytest.mark.parametrize("name", sorted(CLOSED))
def test_closed_forms(cx, name):
    second, (c, n, p, shared) = CLOSED[name]
    for label, tris in ((name, [A, second]), (name + " swapped", [second, A])):
        want, ref, x = run_mesh(cx, soup(tris), label)
        got = x.buffers_numpy()
        assert (x.candidates, x.tested, x.pairs) == (c, n, p) and got["pair_shared"].tolist() == shared and got["pairs"].tolist() == [[0, 1]] * p
        x.close()


def cube_obj():
    """the cube with a normal per face: every corner is written three times, so the render build is unwelded"""
    lines = ["v %g %g %g" % tuple(p) for p in CUBE_POS]
    normals = []
    for q in CUBE_QUADS:
        p = np.float64([CUBE_POS[k] for k in q])
        n = np.cross(p[1] - p[0], p[2] - p[0])
        normals.append(n / np.linalg.norm(n))
    lines += ["vn %.6f %.6f %.6f" % tuple(n + 0.0) for n in normals]
    lines += ["f " + " ".join("%d//%d" % (k + 1, f + 1) for k in q) for f, q in enumerate(CUBE_QUADS)]
    return ("\n".join(lines) + "\n").encode()


def test_sharing_is_by_position(cx):
    mesh = hc.Mesh.from_obj(cube_obj(), "")
    assert len(cx.render_numpy(mesh)["vertex_source"]) == 24 > mesh.nv   # neighbours share positions, not numbers
    want, ref, x = run_mesh(cx, mesh, "cube obj")
    assert x.triangles == 12 and x.pairs == 0 and x.candidates > x.tested > 0   # pairs with a shared edge are never tested, those with a corner are
    x.close()


# ---- 3. tori
def tori_mesh(kind):
    pos, tri = two_tori(kind)
    return mesh_of((pos, np.full(len(tri), 3, np.uint8), tri.reshape(-1)))


@pytest.fixture(scope="module")
def rings(cx):
    want, b = check_build(cx, tori_mesh("rings"), "rings")
    yield want, b, ir.intersections(want)
    b.close()


def pruned(x, L):
    print("box tests per leaf", x.box_tests / L, "of", 2 * L - 1, "nodes; build", x.device_ms, "ms")
    assert 0 < x.box_tests / L <= (2 * L - 1) / 4, x.box_tests / L   # a walk that prunes nothing makes 2 L - 2 a leaf


def test_the_torus(cx):
    want, ref, x = run_mesh(cx, gen(mg.torus(24, 16)), "torus")
    assert (x.pairs, x.candidates) == (0, 4903)
    pruned(x, want["summary"][1])
    x.close()


def test_the_linked_rings(rings):
    want, b, ref = rings
    ref, x = check_intersections(b, want, "rings", ref)
    assert (x.triangles, x.pairs, x.candidates) == (1536, 152, 10562) and not ref["pair_shared"].any()
    pruned(x, want["summary"][1])
    x.close()


def test_the_shifted_copy(cx):
    want, ref, x = run_mesh(cx, tori_mesh("shifted"), "shifted")
    assert x.pairs == 276 and ref["tri_pairs"].max() == 4
    x.close()


# ---- 4. the comb: rows longer than a wavefront and a block, leaf counts at the workgroup seams
def comb(n, needle_first=False, needles=1):
    teeth = [[k + .5, -1, -1, k + .5, 1, -1, k + .5, 0, 1] for k in range(n)]
    needle = [[-1, 0, -.5 - .004 * j, n + 1, 0, -.5 - .004 * j, n + 1, .01, -.25 - .004 * j] for j in range(needles)]   # (parallel: no two meet)
    return needle + teeth if needle_first else teeth + needle


@pytest.mark.parametrize("needle_first", [False, True])
@pytest.mark.parametrize("n", [PAIRS_BLOCK - 1, PAIRS_BLOCK, PAIRS_BLOCK + 1, 200, 257])
def test_the_comb(cx, n, needle_first):
    want, ref, x = run_mesh(cx, soup(comb(n, needle_first)), f"comb {n}")
    got = x.buffers_numpy()
    assert x.pairs == n and x.triangles_hit == n + 1 and not got["pair_shared"].any()
    if needle_first:   # every pair begins with the needle: one leaf's row holds all n
        assert got["pairs"].tolist() == [[0, k + 1] for k in range(n)] and got["tri_pairs"].tolist() == [n] + [1] * n
    else:               # every pair ends in the needle
        assert got["pairs"].tolist() == [[k, n] for k in range(n)] and got["tri_pairs"].tolist() == [1] * n + [n]
    x.close()


def test_more_pairs_than_the_build_left_room_for():
    """100 needles through 100 teeth on a fresh codec: 10 000 pairs of 200 triangles, so the working buffer the hierarchy's build
    left has to grow between the two stretches with the counts and their scan in it: the sort's four sides alone are 4 * 4 P =
    160 000 bytes, while the build over T = 200 triangles asks for a dozen pieces of 4 T or 8 T bytes and the counters of one sort
    tile, under 20 000 bytes together.  This is the growth end to end; no entry point tells whether the buffer grew, so what the
    helper copies and frees is held by itself in tests/test_grow_keeping_cpu.py"""
    n = 100
    P, T = n * n, 2 * n
    fresh = hc.Codec(0)
    try:
        want, ref, x = run_mesh(fresh, soup(comb(n, needles=n)), "needles")
        assert x.pairs == P and x.triangles_hit == T and ref["tri_pairs"].tolist() == [n] * T
        again = fresh.intersections(soup(comb(n, needles=n)))   # ... and with the room there already: the same bytes
        for k in ir.BUFFERS:
            assert same_bits(again.buffers_numpy()[k], ref[k]), k
        again.close()
        x.close()
    finally:
        fresh.close()


# ---- 5. determinism, and the working buffer shared with the queries
def test_two_builds_are_bit_identical(cx, rings):
    want, b, ref = rings
    again = cx.bvh(tori_mesh("rings"))
    x, y = b.intersections(), again.intersections()
    bx, by = x.buffers_numpy(), y.buffers_numpy()
    for k in ir.BUFFERS:
        assert same_bits(bx[k], by[k]), k
    assert x.stat()["box_tests"] == y.stat()["box_tests"]
    for h in (x, y, again):
        h.close()


def test_behind_a_cast_and_a_nearest(rings):
    want, b, ref = rings
    o, d = br.ray_set(want, 300, seed=3)
    assert same_bits(b.cast_numpy(o, d)["tri"], br.cast(want, o, d)["tri"])
    pts = nr.point_set(want, 300, seed=3)
    assert same_bits(b.nearest_numpy(pts)["tri"], nr.nearest(want, pts)["tri"])
    ref, x = check_intersections(b, want, "behind the queries", ref)   # all three use the context's one working buffer
    x.close()
    assert same_bits(b.cast_numpy(o, d)["tri"], br.cast(want, o, d)["tri"])


def test_the_result_outlives_the_hierarchy(cx):
    mesh = tori_mesh("rings")
    x = cx.intersections(mesh)   # renders, builds the hierarchy, queries and frees both
    del mesh
    assert x.pairs == 152 and x.buffers_numpy()["pairs"].shape == (152, 2)
    x.close()
    x.close()


TORCH_CHILD = r"""
import sys
import numpy as np
import torch
torch.cuda.init()   # a PyTorch program: torch holds the device before the codec starts
sys.path.insert(0, sys.argv[1])
from harry_amd import codec as hc
from tests.test_intersections_cpu import two_tori
pos, tri = two_tori("rings")
v = np.zeros(len(pos), np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")]))
v["x"], v["y"], v["z"] = pos[:, 0], pos[:, 1], pos[:, 2]
c = hc.Codec(0)
x = c.intersections(hc.Mesh.from_arrays(v, np.full(len(tri), 3, np.uint8), tri.reshape(-1)))
host, dev = x.buffers_numpy(), x.buffers()
assert tuple(dev["pairs"].shape) == (152, 2) and tuple(dev["pair_shared"].shape) == (152,) and tuple(dev["tri_pairs"].shape) == (1536,)
for k in host:
    assert dev[k].dtype == torch.int32 and dev[k].is_cuda and np.array_equal(dev[k].cpu().numpy().view(np.uint32), host[k]), k
x.close()
c.close()
print("torch ok")
"""


def test_torch_tensors():
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD, util.ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "torch ok" in r.stdout, r.stdout + r.stderr


# ---- 6. refusals
def test_refusals(cx, rings):
    want, b, ref = rings
    L = nat.load()
    out = C.c_void_p(77)
    for args, words in (((cx.h, None, 0), "null argument"), ((None, b.h, 0), "null argument"), ((cx.h, b.h, 1), "unknown intersections flag"),
                        ((cx.h, b.h, 0x80000000), "unknown intersections flag")):
        out.value = 77
        assert L.hry_intersections_build(*args, C.byref(out)) == nat.E_ARG and words in L.hry_last_error().decode() and out.value is None, args
    assert L.hry_intersections_build(cx.h, b.h, 0, None) == nat.E_ARG
    ref, x = check_intersections(b, want, "after the refusals", ref)   # the context is as usable as before
    rows, width, typ = C.c_uint64(), C.c_int(), C.c_int()
    nat.check(L.hry_intersections_get(x.h, b"pairs", None, C.byref(rows), C.byref(width), C.byref(typ)))
    assert (rows.value, width.value) == (152, 2)
    nat.check(L.hry_intersections_get(x.h, b"leaf_tri", None, C.byref(rows), C.byref(width), C.byref(typ)))
    assert (rows.value, width.value) == (0, 0)   # no such buffer
    x.close()


# ---- 7. the command line
def run(*args):
    r = subprocess.run([cli.HARRY] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.splitlines()


def test_the_command_line(rings, tmp_path):
    want, b, ref = rings
    pos, tri = two_tori("rings")
    (tmp_path / "rings.ply").write_bytes(mg.Mesh(util.xyz(pos), np.full(len(tri), 3, np.uint8), tri.reshape(-1)).to_ply())
    lines = run(tmp_path / "rings.ply", "--intersections", "--bvh")
    (at,) = [i for i, l in enumerate(lines) if l.startswith("Intersections:")]
    assert lines[at] == "Intersections: triangles %d candidates %d tested %d pairs %d triangles-hit %d" % ref["summary"] and "pairs 152 " in lines[at]
    assert lines[at - 1].startswith("Bvh:") and "Writing output..." not in lines   # after the --bvh line; OUTPUT may be left out
    with_option = run(tmp_path / "rings.ply", tmp_path / "a.hry", "-l1", "-q14", "--intersections")
    without = run(tmp_path / "rings.ply", tmp_path / "b.hry", "-l1", "-q14")
    assert (tmp_path / "a.hry").read_bytes() == (tmp_path / "b.hry").read_bytes() and not [l for l in without if l.startswith("Intersections:")]
    (line,) = [l for l in with_option if l.startswith("Intersections:")]
    assert line.startswith("Intersections: triangles 1536 ") and with_option.index("Writing output...") > with_option.index(line)
    again = run(tmp_path / "a.hry", "--intersections")   # of the decode: what the quantisation left of them
    assert len([l for l in again if l.startswith("Intersections: triangles 1536 ")]) == 1
