"""The closest-point query over the hierarchy (include/harry_amd.h: hry_bvh_nearest; kernel: harry_amd/csrc/device/bvh.hip,
k_bvh_nearest) against the numpy restatement of tests/nearest_ref.py, which tests every point against every leaf.  The triangle, the
squared distance, the barycentric pair, the point and the three stat words are compared bit for bit; no value is left out and
nothing has a tolerance (the second stat word, which depends on the walk, is held to the pruning bound instead)."""
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
from tests import nearest_ref as nr
from tests import util
from tests.test_creases_cpu import cube_quads
from tests.test_gpu_bvh import MESHES as BVH_MESHES
from tests.test_gpu_bvh import check_build, same_bits
from tests.test_gpu_creases import gen, mesh_of, render_inputs

pytestmark = pytest.mark.gpu

NEAREST_BLOCK = 64   # bvh.hip: kCastBlock, the points of one workgroup of the query
POINT_COUNTS = [0, 1, NEAREST_BLOCK - 1, NEAREST_BLOCK, NEAREST_BLOCK + 1, 2 * NEAREST_BLOCK + 1]
MESHES = {name: BVH_MESHES[name] for name in ("no_leaf", "one_leaf", "two_leaves", "three_leaves", "one_code", "a_point", "flat", "dead_in_a_tile", "torus_mixed")}
MESHES["torus"] = lambda: gen(mg.torus(24, 16))
KEYS = ("tri", "d2", "uv", "point")
FLAT = (np.float32([[x, y, 0] for y in range(9) for x in range(9)]), np.full(64, 4, np.uint8),   # the grid of "flat": 8 x 8 quads in z = 0
        np.array([[9 * y + x, 9 * y + x + 1, 9 * y + x + 10, 9 * y + x + 9] for y in range(8) for x in range(8)], np.uint32).reshape(-1))
BAD = np.float32([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan]])


@pytest.fixture(scope="module")
def cx():
    c = hc.Codec(0)
    yield c
    c.close()


def bits_of(x):
    return int(np.float64(x).view(np.uint64))


def check_nearest(b, want, points, label, max_dist=np.inf, ref=None):
    """one query against the restatement (or against `ref`, rows of a restatement made before): every output and the stat"""
    got = b.nearest_numpy(points, max_dist)
    ref = nr.nearest(want, points, max_dist) if ref is None else ref
    for k in KEYS:
        assert same_bits(got[k], ref[k]), (label, k, int((got[k] != ref[k]).sum()))
    answered = ref["tri"] != br.NO_ELEMENT
    assert b.answered == int(answered.sum()), (label, b.answered)
    assert bits_of(b.max_d2) == (bits_of(ref["d2"][answered].max()) if answered.any() else 0), (label, b.max_d2)
    assert b.device_ms > 0 or not len(ref["tri"])
    return ref


def rows_of(ref, pick):
    return {k: ref[k][pick] for k in KEYS}


# ---- 1. meshes: a query against the restatement
@pytest.mark.parametrize("name", sorted(MESHES))
def test_against_the_restatement(cx, name):
    want, b = check_build(cx, MESHES[name](), name)
    L = want["summary"][1]
    pts = np.concatenate([nr.point_set(want, 240, seed=len(name)), BAD])
    ref = check_nearest(b, want, pts, name)
    assert ref["answered"] == (240 if L else 0)
    if name == "one_code":
        assert L == 1025 and set(ref["tri"][:240].tolist()) == {0}   # coincident triangles: every answer is a tie, and goes to number 0
    if name == "a_point":
        assert (ref["uv"] == 0).all() and (ref["point"][:240] == np.float32([1, 2, 3])).all()
    if L:
        assert (ref["d2"][:240] == 0).sum() >= 30
        radius = float(np.sqrt(np.median(ref["d2"][:240])))
        within = check_nearest(b, want, pts, name + " within a radius", radius)
        assert 60 <= within["answered"] <= 240
    b.close()


# ---- 2. points
@pytest.fixture(scope="module")
def torus(cx):
    want, b = check_build(cx, MESHES["torus"](), "torus")
    pts = nr.point_set(want, 2000, seed=3)
    yield want, b, pts, nr.nearest(want, pts)
    b.close()


def test_the_torus_set_and_the_pruning(torus):
    want, b, pts, ref = torus
    n, L = len(pts), want["summary"][1]
    check_nearest(b, want, pts, "torus", ref=ref)
    assert ref["answered"] == n and (ref["d2"] == 0).sum() >= n // 8
    print("bounds per point", b.bound_tests / n, "of", 2 * L - 1, "nodes; query", b.device_ms, "ms")
    assert 0 < b.bound_tests / n <= (2 * L - 1) / 4, b.bound_tests / n   # a walk that prunes nothing evaluates 2 L - 2


def test_the_flat_grid_set(cx):
    want, b = check_build(cx, MESHES["flat"](), "flat")
    check_nearest(b, want, nr.point_set(want, 2000, seed=3), "flat")
    b.close()


@pytest.mark.parametrize("n", POINT_COUNTS)
def test_point_counts(torus, n):
    want, b, pts, ref = torus
    pick = np.arange(n) * 7 % len(pts)
    got = b.nearest_numpy(pts[pick])
    assert got["tri"].shape == (n,) and got["d2"].shape == (n,) and got["uv"].shape == (n, 2) and got["point"].shape == (n, 3)
    for k in KEYS:
        assert same_bits(got[k], ref[k][pick]), k
    assert b.answered == n and (b.bound_tests > 0) == (n > 0)
    assert bits_of(b.max_d2) == (bits_of(ref["d2"][pick].max()) if n else 0)


@pytest.mark.parametrize("stride", [12, 16, 32, 0])
def test_strides(torus, stride):
    want, b, pts, ref = torus
    n = 500
    if stride:
        wide = np.full((n + 1, stride // 4), 7, np.float32)
        wide[1:, -3:] = pts[:n]
        view = wide[1:, -3:]
        expect = rows_of(ref, slice(0, n))
    else:   # one point for all
        view = np.broadcast_to(pts[7], (n, 3))
        expect = {k: np.repeat(ref[k][7:8], n, axis=0) for k in KEYS}
    assert view.strides[0] == stride
    check_nearest(b, want, view, f"stride {stride}", ref=expect)


def test_invalid_points_among_valid_ones(torus):
    want, b, pts, ref = torus
    mixed = pts[:200].copy()
    at = np.arange(3, 200, 9)
    mixed[at] = BAD[np.arange(len(at)) % len(BAD)]
    expect = {k: ref[k][:200].copy() for k in KEYS}
    expect["tri"][at], expect["d2"][at], expect["uv"][at], expect["point"][at] = br.NO_ELEMENT, np.inf, 0, 0
    check_nearest(b, want, mixed, "invalid among valid", ref=expect)
    assert b.answered == 200 - len(at)
    assert check_nearest(b, want, BAD, "only invalid")["answered"] == 0


def test_radii(torus):
    want, b, pts, ref = torus
    pts = pts[:1200:2]
    mine = rows_of(ref, slice(0, 1200, 2))
    radius = float(np.sqrt(np.median(mine["d2"][mine["d2"] > 0])))
    within = check_nearest(b, want, pts, "the median radius", radius)
    assert len(pts) // 4 <= within["answered"] <= len(pts) - len(pts) // 4
    zero = check_nearest(b, want, pts, "radius 0", 0.0)
    assert zero["answered"] == int((mine["d2"] == 0).sum()) > 0 and b.max_d2 == 0.0   # only the points on the surface answer
    assert check_nearest(b, want, pts, "a negative radius", -1.0)["answered"] == 0 and b.bound_tests == 0
    check_nearest(b, want, pts, "an infinite radius", np.inf, ref=mine)


def test_an_answer_exactly_at_the_radius(cx):
    want, b = check_build(cx, mesh_of(cube_quads()), "cube")
    q = np.float32([[0.75, 0.25, -1.0], [0.5, -2.0, 0.0]])   # 1 and 2 away: d2 = 1 and 4, squares of the radii below
    for radius, answered in ((1.0, 1), (2.0, 2), (0.9999999, 0), (1.9999999, 1)):
        assert check_nearest(b, want, q, f"radius {radius}", radius)["answered"] == answered
    b.close()


def test_two_queries_are_bit_identical(cx, torus):
    want, b, pts, ref = torus
    again = cx.bvh(MESHES["torus"]())
    x, y, z = b.nearest_numpy(pts[:700]), again.nearest_numpy(pts[:700]), b.nearest_numpy(pts[:700])
    for k in KEYS:
        assert same_bits(x[k], y[k]) and same_bits(x[k], z[k]), k
    again.close()


# ---- 3. device pointers, torch
TORCH_CHILD = r"""
import sys
import numpy as np
import torch
torch.cuda.init()   # a PyTorch program: torch holds the device before the codec starts
sys.path.insert(0, sys.argv[1])
from harry_amd import codec as hc
from harry_amd import meshgen as mg
from tests import nearest_ref as nr
m = mg.torus(24, 16)
mesh = hc.Mesh.from_arrays(m.verts, m.degrees, m.indices)
c = hc.Codec(0)
b = c.bvh(mesh)
host = b.buffers_numpy()
p = nr.point_set(host, 1000, seed=3)
p[5::50] = np.nan
ref = b.nearest_numpy(p)
answered, tests, largest = b.answered, b.bound_tests, b.max_d2
assert answered == 1000 - 20 and largest > 0
KEYS = ("tri", "d2", "uv", "point")
def same(got, want=ref, n=len(p)):
    assert got["tri"].dtype == torch.int32 and got["d2"].dtype == torch.float64 and got["uv"].dtype == got["point"].dtype == torch.float32
    assert tuple(got["tri"].shape) == (n,) and tuple(got["d2"].shape) == (n,) and tuple(got["uv"].shape) == (n, 2) and tuple(got["point"].shape) == (n, 3)
    for k in KEYS:
        assert np.array_equal(got[k].cpu().numpy().view(np.uint8), np.ascontiguousarray(want[k][:n]).view(np.uint8)), k
tp = torch.from_numpy(p).cuda()
same(b.nearest(tp))                                    # HRY_NEAREST_HOST and device pointers: the same bits
assert b.answered == answered and b.bound_tests == tests and b.max_d2 == largest and b.device_ms > 0
assert int((b.nearest(tp)["tri"] == -1).sum()) == 20
for width in (4, 8):                                   # strides of 16 and 32 bytes
    wide = torch.full((len(p), width), 7.0, device="cuda")
    wide[:, -3:] = tp
    same(b.nearest(wide[:, -3:]))
half = b.nearest(tp[::2])                              # a stride of 24 bytes
assert np.array_equal(half["d2"].cpu().numpy().view(np.uint64), ref["d2"][::2].view(np.uint64))
one = b.nearest(tp[7])                                 # one point
same(one, {k: ref[k][7:8] for k in KEYS}, 1)
wide = b.nearest(tp[7].expand(300, 3))                 # ... and as an expanded tensor: stride 0
same(wide, {k: np.repeat(ref[k][7:8], 300, axis=0) for k in KEYS}, 300)
radius = float(np.sqrt(np.median(ref["d2"][np.isfinite(ref["d2"]) & (ref["d2"] > 0)])))
same(b.nearest(tp, radius), b.nearest_numpy(p, radius))
assert 250 < b.answered < 750
assert tuple(b.nearest(tp[:0])["tri"].shape) == (0,)
b.close()
c.close()
print("torch ok")
"""


def test_torch_tensors_and_device_pointers():
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD, util.ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "torch ok" in r.stdout, r.stdout + r.stderr


# ---- 4. refusals
def test_refusals(cx):
    """every refusal returns its code, writes nothing, and leaves the context as usable as before"""
    L = nat.load()
    good = mesh_of(cube_quads())
    b = cx.bvh(good)
    q = np.float32([[0.75, 0.25, -1.0]] * 4)
    tri, d2, uv, point = np.zeros(4, np.uint32), np.zeros(5, np.float64), np.zeros((4, 2), np.float32), np.zeros((4, 3), np.float32)
    stat, ms = (C.c_uint64 * 3)(), C.c_double()

    def nearest(n=4, q_ptr=q.ctypes.data, stride=12, max_dist=np.inf, flags=nat.NEAREST_HOST, tri_ptr=tri.ctypes.data, d2_ptr=d2.ctypes.data, handle=b.h):
        return L.hry_bvh_nearest(cx.h, handle, n, q_ptr, stride, max_dist, flags, tri_ptr, d2_ptr, uv.ctypes.data, point.ctypes.data, stat, C.byref(ms))

    def usable():
        other = cx.bvh(good)
        assert other.count() == 12 and other.nearest_numpy([0.75, 0.25, -1.0])["d2"].tolist() == [1.0]
        other.close()

    assert nearest() == 0 and tri.tolist() == [1] * 4 and d2[:4].tolist() == [1.0] * 4 and uv.tolist() == [[0.25, 0.5]] * 4
    assert point.tolist() == [[0.75, 0.25, 0.0]] * 4 and list(stat)[0] == 4 and list(stat)[2] == bits_of(1.0) and ms.value > 0
    dev = C.c_void_p()
    nat.check(L.hry_bvh_get(b.h, b"leaf_positions", C.byref(dev), C.byref(C.c_uint64()), None, None))
    for kw, words in ((dict(handle=None), "null argument"), (dict(tri_ptr=None), "null argument"), (dict(q_ptr=None), "null argument"),
                      (dict(flags=2), "unknown nearest flag"), (dict(flags=3), "unknown nearest flag"),
                      (dict(stride=6), "multiple of 4"), (dict(stride=13), "multiple of 4"),
                      (dict(max_dist=np.nan), "NaN"),
                      (dict(flags=0), "not device memory"),                                       # host memory in a device query
                      (dict(q_ptr=dev.value), "device memory in a closest-point query with"),     # device memory in a host query
                      (dict(d2_ptr=d2.ctypes.data + 4), "misaligned"), (dict(q_ptr=q.ctypes.data + 2), "misaligned")):
        tri[:], d2[:], uv[:], point[:], ms.value = 77, 77, 77, 77, 77
        stat[0] = stat[1] = stat[2] = 77
        assert nearest(**kw) == nat.E_ARG and words in L.hry_last_error().decode(), (kw, L.hry_last_error())
        assert tri.tolist() == [77] * 4 and d2.tolist() == [77] * 5 and (uv == 77).all() and (point == 77).all() and list(stat) == [77] * 3 and ms.value == 77   # nothing was written
        usable()
    tri[:] = 77
    assert nearest(n=0, q_ptr=None, tri_ptr=None) == 0 and tri.tolist() == [77] * 4 and list(stat) == [0, 0, 0]   # no points: nothing is touched
    assert nearest(max_dist=-1.0) == 0 and tri.tolist() == [br.NO_ELEMENT] * 4 and np.isinf(d2[:4]).all() and not uv.any() and not point.any()   # no error
    assert list(stat) == [0, 0, 0]
    assert L.hry_bvh_nearest(cx.h, b.h, 4, q.ctypes.data, 12, np.inf, nat.NEAREST_HOST, tri.ctypes.data, None, None, None, None, None) == 0
    assert tri.tolist() == [1] * 4   # d2, uv, point, stat and device_ms may be left out
    b.close()


# ---- 5. Codec.deviation and the command line
def deviation_by_the_restatement(cx, a, b):
    """Codec.deviation's dict from the restatement: the position rows of each mesh's render build against the other's leaves"""
    sides = []
    for mesh in (a, b):
        rn, pos = render_inputs(cx, mesh)
        sides.append((br.build(rn["indices"], pos), pos))

    def one_way(points, surface):
        ref = nr.nearest(surface, points)
        d2 = ref["d2"][ref["tri"] != br.NO_ELEMENT]
        total = 0.0
        for x in d2.tolist():
            total += x
        return {"points": len(points), "answered": len(d2), "max": float(np.sqrt(d2.max())) if len(d2) else 0.0, "rms": float(np.sqrt(total / len(d2))) if len(d2) else 0.0}

    out = {"forward": one_way(sides[0][1], sides[1][0]), "backward": one_way(sides[1][1], sides[0][0])}
    out["hausdorff"] = max(out["forward"]["max"], out["backward"]["max"])
    return out, sides[0][0]["scene_box"][0].astype(np.float64)


def lines_of(dev, box):
    diagonal = float(np.sqrt(((box[3] - box[0]) * (box[3] - box[0]) + (box[4] - box[1]) * (box[4] - box[1])) + (box[5] - box[2]) * (box[5] - box[2])))
    out = ["Deviation: %s points %d answered %d max %.9g rms %.9g" % (k, dev[k]["points"], dev[k]["answered"], dev[k]["max"], dev[k]["rms"]) for k in ("forward", "backward")]
    return out + ["Deviation: hausdorff %.9g diagonal %.9g relative %.9g" % (dev["hausdorff"], diagonal, dev["hausdorff"] / diagonal)]


def run(*args):
    r = subprocess.run([cli.HARRY] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.splitlines()


def deviation_lines(lines):
    return [l for l in lines if l.startswith("Deviation:")]


def test_deviation_of_a_mesh_against_itself_and_a_moved_copy(cx, tmp_path):
    torus = mg.torus(24, 16)
    (tmp_path / "torus.ply").write_bytes(torus.to_ply())
    lines = run(tmp_path / "torus.ply", "--deviation", tmp_path / "torus.ply", "--bvh")
    got = deviation_lines(lines)
    n = len(torus.verts)
    assert got[:2] == [f"Deviation: forward points {n} answered {n} max 0 rms 0", f"Deviation: backward points {n} answered {n} max 0 rms 0"]
    assert got[2].startswith("Deviation: hausdorff 0 diagonal ") and got[2].endswith(" relative 0") and len(got) == 3
    (at,) = [i for i, l in enumerate(lines) if l.startswith("Bvh:")]
    assert lines[at + 1:at + 4] == got and "Writing output..." not in lines   # after the --bvh line; OUTPUT may be left out
    pos, deg, idx = FLAT
    (tmp_path / "flat.ply").write_bytes(mg.Mesh(util.xyz(pos), deg, idx).to_ply())
    (tmp_path / "moved.ply").write_bytes(mg.Mesh(util.xyz(pos + np.float32([0, 0, 0.5])), deg, idx).to_ply())
    got = deviation_lines(run(tmp_path / "flat.ply", "--deviation", tmp_path / "moved.ply"))
    assert got == ["Deviation: forward points 81 answered 81 max 0.5 rms 0.5", "Deviation: backward points 81 answered 81 max 0.5 rms 0.5",
                   "Deviation: hausdorff 0.5 diagonal %.9g relative %.9g" % (np.sqrt(128.0), 0.5 / np.sqrt(128.0))]
    d = cx.deviation(mesh_of((pos, deg, idx)), mesh_of((pos + np.float32([0, 0, 0.5]), deg, idx)))
    assert d == {"forward": {"points": 81, "answered": 81, "max": 0.5, "rms": 0.5}, "backward": {"points": 81, "answered": 81, "max": 0.5, "rms": 0.5}, "hausdorff": 0.5}


def test_deviation_of_a_quantised_decode(cx, tmp_path):
    torus = mg.torus(24, 16)
    (tmp_path / "in.ply").write_bytes(torus.to_ply())
    with_option = run(tmp_path / "in.ply", tmp_path / "a.hry", "-l1", "-q8", "--deviation", tmp_path / "in.ply")
    without = run(tmp_path / "in.ply", tmp_path / "b.hry", "-l1", "-q8")
    assert (tmp_path / "a.hry").read_bytes() == (tmp_path / "b.hry").read_bytes() and not deviation_lines(without)
    assert with_option.index("Writing output...") > max(i for i, l in enumerate(with_option) if l.startswith("Deviation:"))
    got = deviation_lines(run(tmp_path / "a.hry", "--deviation", tmp_path / "in.ply"))
    decoded, source = cx.read_hry((tmp_path / "a.hry").read_bytes()), hc.Mesh.from_ply(torus.to_ply())
    dev = cx.deviation(decoded, source)
    want, box = deviation_by_the_restatement(cx, decoded, source)
    assert dev == want, (dev, want)
    assert got == lines_of(want, box), (got, lines_of(want, box))
    assert len(deviation_lines(with_option)) == 3   # (of the quantised mesh in its source order: the sums may differ in their last bits)
    n = len(torus.verts)
    assert dev["forward"]["points"] == dev["forward"]["answered"] == n and dev["backward"]["answered"] == n
    # 8 bits over the extent of an axis: no coordinate moves by more than a step, so no vertex by more than sqrt(3) steps, and its
    # own moved copy lies on the other surface
    step = float((np.stack([torus.verts[k] for k in "xyz"]).max(axis=1) - np.stack([torus.verts[k] for k in "xyz"]).min(axis=1)).max()) / 255
    assert 0 < dev["forward"]["rms"] <= dev["forward"]["max"] <= dev["hausdorff"] <= np.sqrt(3) * step
