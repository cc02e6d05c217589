"""Vertex areas and curvatures of a render build (include/harry_amd.h: hry_curvature_build; kernels: harry_amd/csrc/device/curvature.hip)
against the numpy restatement of tests/curvature_ref.py, which reads what the render build holds.  The classes and the summary's
counts are compared exactly; every float value within one float32 step of the restatement's + 2^-40 of its scale, the totals within
2^-40 of theirs (curvature_ref's docstring derives the bound); no value is left out.  Every comparison prints how many values are not
bit-equal and the largest difference in units of the bound (DESIGN.md "Curvature" has the table)."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import cli
from harry_amd import codec as hc
from harry_amd import meshgen as mg
from tests import curvature_ref as cv
from tests import seam_meshes as sm
from tests import util
from tests.test_creases_cpu import cube_quads, cube_triangles
from tests.test_curvature_cpu import obtuse_sheet
from tests.test_gpu_creases import gen, mesh_of, not_bit_equal, render_inputs

pytestmark = pytest.mark.gpu

# the sizes at which curvature.hip changes strategy, and the ones it shares (tests/seam_meshes.py)
CURV_SEG_MAX = 32    # kCurvSegMax: a lane sums a vertex of up to so many slots, a workgroup a longer one
CURV_RANGES = 256    # the ranges of a workgroup's sum (the threads of k_cur_hubs)
CURV_BLOCK = 256     # the threads of a block of the per-edge, per-slot, per-decoded-vertex and per-output-vertex kernels
CURV_FOLD = 256      # kCurvFold: the rows one block of the totals' reduction adds


@pytest.fixture(scope="module")
def cx():
    c = hc.Codec(0)
    yield c
    c.close()


def compare(got, st, want, label):
    """the buffers and the stat of one build against the restatement"""
    assert sorted(got) == sorted(hc.Codec.CURVATURE_BUFFERS) == sorted(cv.BUFFERS)
    assert got["vertex_class"].dtype == np.uint32 and np.array_equal(got["vertex_class"], want["vertex_class"]), (label, "vertex_class")
    assert tuple(st[k] for k in cv.SUMMARY) == want["summary"], (label, st, want["summary"])
    worst = {}
    for name in cv.FLOATS:
        worst[name] = cv.compare(got[name], want[name], want["scale"][name], f"{label} {name}")
        zero = want[name].view(np.uint32) == 0   # a row written as +0 is +0, bit for bit
        assert not got[name].view(np.uint32)[zero & (want["scale"][name] == 0)].any(), (label, name)
    totals = np.array([st[k] for k in cv.TOTALS])
    worst["totals"] = cv.compare(totals, want["totals"], want["scale"]["totals"], f"{label} totals")
    tb = cv.EPS * want["scale"]["totals"]
    assert (np.abs(totals - want["totals"]) <= tb)[np.isfinite(want["totals"])].all(), (label, totals, want["totals"], tb)
    return worst


def check(cx, mesh, label):
    """the build against the restatement, with the summary, the totals and the stat; returns (the restatement, the buffers, the stat)"""
    rn, pos = render_inputs(cx, mesh)
    want = cv.from_render(rn, pos, mesh.nv)
    got = cx.curvature_numpy(mesh)
    st = cx.curvature_stat()
    assert st["uploaded_bytes"] == 0 and st["device_ms"] > 0 and st["edges_device_ms"] > 0 and st["vertices"] == mesh.nv
    compare(got, st, want, label)
    return want, got, st


# ---- 1. against the restatement
def torus_obj_mesh():
    from tests.test_gpu_tangents import torus_obj   # an OBJ torus whose vt seams unweld the wrap's vertices
    return hc.Mesh.from_obj(torus_obj(), "")


def degenerate_mesh():
    pos = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.1],      # a proper pair of triangles
           [1, 0.5, 0.05],                                     # ... and a sliver on their edge 1 - 3 with no area: 1, 3 and their midpoint
           [3, 0, 0], [4, 0, 0], [5, 0, 0],                    # three points on a line
           [7, 0, 0], [7, 0, 0], [8, 1, 0]]                    # two corners in one place
    return util.xyz_mesh(pos, [[0, 1, 2], [1, 3, 2], [3, 1, 4], [5, 6, 7], [8, 9, 10]])


NAN_VERTEX = 14


def nan_mesh():
    m = mg.grid(6, 6)
    verts = m.verts.copy()
    verts["x"][NAN_VERTEX] = np.nan
    return hc.Mesh.from_arrays(verts, m.degrees, m.indices)


MESHES = {
    "grid_triangles": lambda: gen(mg.grid(9, 8)),
    "grid_quads": lambda: gen(mg.grid(9, 8, quads=True)),
    "icosphere": lambda: gen(mg.icosphere(2)),
    "torus": lambda: gen(mg.torus(24, 16)),
    "torus_mixed": lambda: gen(mg.torus(24, 16, polys="mixed")),
    "torus_nonmanifold": lambda: gen(mg.with_nonmanifold(mg.torus(24, 16))),
    "soup": lambda: gen(mg.soup(seed=7)),
    "one_triangle": lambda: util.xyz_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]]),
    "cube_quads": lambda: mesh_of(cube_quads()),
    "cube_triangles": lambda: mesh_of(cube_triangles()),
    "obj_torus": torus_obj_mesh,
    "obtuse_sheet": lambda: mesh_of(obtuse_sheet()),
    "degenerate": degenerate_mesh,
    "nan_position": nan_mesh,
}


@pytest.mark.parametrize("name", sorted(MESHES))
def test_against_the_restatement(cx, name):
    mesh = MESHES[name]()
    want, got, st = check(cx, mesh, name)
    turns = st["defect"] / cv.TWO_PI
    if name in ("cube_quads", "cube_triangles"):
        assert want["summary"] == (8, 8, 0, 0, 0, 0) and abs(turns - 2) < 1e-12 and abs(st["area"] - 6) < 1e-12
        assert np.abs(got["angle_defect"] - np.float32(np.pi / 2)).max() <= np.spacing(np.float32(np.pi / 2))
    if name in ("torus", "torus_mixed"):
        assert want["summary"][1] == mesh.nv and abs(turns) < 1e-9
    if name == "icosphere":
        assert abs(turns - 2) < 1e-9 and (got["mean"] > 0).all() and (got["gaussian"] > 0).all()
    if name in ("grid_triangles", "grid_quads"):
        assert want["summary"][2] == 2 * (9 + 8) - 4 and abs(turns - 1) < 1e-9
    if name in ("torus_nonmanifold", "soup"):
        assert want["summary"][3] > 0
    if name == "one_triangle":
        assert want["summary"] == (3, 0, 3, 0, 0, 0) and abs(st["area"] - 0.5) < 1e-15
    if name == "obtuse_sheet":
        assert sorted(set(want["branch"].tolist())) == [0, 1, 2]
    if name == "obj_torus":   # the seams split output vertices, not the rings: the rows of one decoded vertex are bit-equal
        vs = cx.render_numpy(mesh)["vertex_source"]
        assert len(vs) > mesh.nv and want["summary"][1] == mesh.nv
        first = np.full(mesh.nv, -1)
        first[vs[::-1]] = np.arange(len(vs))[::-1]
        for k in cv.BUFFERS:
            assert not_bit_equal(got[k], got[k][first[vs]]) == 0, k
    if name == "degenerate":   # the triangles without area give their corners nothing: the vertices only they name have bit 8
        assert (got["vertex_class"][4:] & 8).all() and not (got["vertex_class"][:4] & 8).any() and want["summary"][5] == 7
        assert not got["vertex_area"][4:].any() and (got["vertex_area"][:4] > 0).all()
    if name == "nan_position":   # the NaN poisons its own triangles only; no NaN comes out
        assert got["vertex_class"][NAN_VERTEX] == (cv.INTERIOR | cv.DEGENERATE) and want["summary"][5] == 1
        for k in cv.FLOATS:
            assert np.isfinite(got[k]).all(), k


@pytest.mark.parametrize("profile", [hc.PROFILE_COMPAT, hc.PROFILE_CHUNKED], ids=["compat", "chunked"])
@pytest.mark.parametrize("bits", [0, 12], ids=["lossless", "q12"])
def test_decoded_meshes(cx, profile, bits):
    m = gen(mg.torus(24, 16, polys="mixed"))
    if bits:
        cx.requant(m, [(1, -1, bits)])
    dec = cx.read_hry(cx.write_hry(m, profile=profile))
    want, got, st = check(cx, dec, f"decoded {bits}")   # (resident: a render build leaves the decode's buffers where they are)
    assert want["summary"][1] == dec.nv and abs(st["defect"]) < 1e-9
    up = dec.clone()
    again = cx.curvature_numpy(up)
    for k in cv.BUFFERS:
        assert not_bit_equal(again[k], got[k]) == 0, k


# ---- 2. the seams of the kernels
def test_hub_discs(cx):
    """centres of 31 .. 34 and 255 .. 257 slots: the lane's sum up to CURV_SEG_MAX, the workgroup's CURV_RANGES ranges beyond -- of
    one slot up to 256 of them, of two from 257 on"""
    assert sm.HUB_VALENCES == [CURV_SEG_MAX - 1, CURV_SEG_MAX, CURV_SEG_MAX + 1, CURV_SEG_MAX + 2, CURV_RANGES - 1, CURV_RANGES, CURV_RANGES + 1]
    mesh = sm.hub_discs()
    want, got, st = check(cx, mesh_of(mesh), "hub discs")
    slots = want["decoded"]["slots"]
    centres = np.flatnonzero(slots > 6)
    assert slots[centres].tolist() == sm.HUB_VALENCES and (want["decoded"]["class"][centres] == cv.INTERIOR).all()
    assert want["summary"][1:] == (sum(sm.HUB_VALENCES) + len(sm.HUB_VALENCES), sum(sm.HUB_VALENCES), 0, 0, 0)   # the rims are boundary
    assert (got["vertex_area"][centres] > 0).all() and (got["mean"][centres] != 0).all()


@pytest.mark.parametrize("ntri", [85, 86, 255, 256, 257])
def test_strips(cx, ntri):
    """255 and 258 slots, 255 .. 257 triangles: either side of CURV_BLOCK slots; the vertices the strip leaves out are isolated"""
    mesh = sm.strip(ntri)
    want, got, st = check(cx, mesh_of(mesh), f"strip {ntri}")
    assert want["summary"][2] == ntri + 2 and want["summary"][4] == len(mesh[0]) - ntri - 2 == want["summary"][5]


def straddling(nv):
    """a two-row grid and, last, a triangle on vertices of its own: nv decoded vertices"""
    tri = (np.float32([[0, 5, 0], [1, 5, 0], [0, 6, 0.5]]), np.full(1, 3, np.uint8), np.arange(3, dtype=np.uint32))
    k, rest = divmod(nv, 2)
    return sm.join([sm.gen_arrays(mg.grid(k - 1, 2)), tri]) if rest else sm.gen_arrays(mg.grid(k, 2))


@pytest.mark.parametrize("nv", [CURV_BLOCK - 1, CURV_BLOCK, CURV_BLOCK + 1])
def test_vertex_count_straddles_a_block(cx, nv):
    """one block of k_cur_vertices and one chunk of k_cur_fold hold CURV_BLOCK = CURV_FOLD decoded vertices: one less, as many, one
    more -- the last one a corner of a real triangle, and the totals of the third a second round"""
    assert CURV_BLOCK == CURV_FOLD
    mesh = straddling(nv)
    assert len(mesh[0]) == nv
    want, got, st = check(cx, mesh_of(mesh), f"{nv} vertices")
    assert want["summary"][0] == nv and want["summary"][4] == 0 and got["vertex_area"][nv - 1] > 0


def test_shuffled_torus(cx):
    """neighbours lie far apart: a vertex's slots come from all over the slot range, in whatever order the scatter leaves them"""
    mesh = sm.shuffled_torus()
    assert len(mesh[1]) == 24576
    want, got, st = check(cx, mesh_of(mesh), "shuffled torus")
    assert want["summary"] == (len(mesh[0]), len(mesh[0]), 0, 0, 0, 0) and abs(st["defect"]) < 1e-8


# ---- 3. determinism and ownership
def test_two_builds_are_bit_identical(cx):
    mesh = mesh_of(sm.join([sm.hub_discs(), sm.gen_arrays(mg.torus(24, 16))]))
    first, st = cx.curvature_numpy(mesh), cx.curvature_stat()
    again, st2 = cx.curvature_numpy(mesh), cx.curvature_stat()
    for k in cv.BUFFERS:
        assert not_bit_equal(again[k], first[k]) == 0, k
    for k in cv.SUMMARY + cv.TOTALS:
        assert np.array_equal(np.float64(st[k]).view(np.uint64), np.float64(st2[k]).view(np.uint64)), k


def test_inputs_freed_before_the_buffers_are_read(cx):
    L = nat.load()
    mesh = mesh_of(sm.hub_discs())
    want = cx.curvature_numpy(mesh)
    r, e, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
    nat.check(L.hry_render_build(cx.h, mesh.h, C.byref(r)))
    nat.check(L.hry_edges_build(cx.h, mesh.h, r, 0, C.byref(e)))
    nat.check(L.hry_curvature_build(cx.h, mesh.h, r, e, 0, C.byref(c)))
    L.hry_edges_free(e)
    L.hry_render_free(r)
    try:
        assert L.hry_curvature_count(c) == len(want["mean"])
        d, up = C.c_double(), C.c_uint64(7)
        nat.check(L.hry_curvature_stat(c, C.byref(d), C.byref(up)))
        assert up.value == 0 and d.value > 0
        for name in hc.Codec.CURVATURE_BUFFERS:
            rows, width, typ = C.c_uint64(), C.c_int(), C.c_int()
            nat.check(L.hry_curvature_get(c, name.encode(), None, C.byref(rows), C.byref(width), C.byref(typ)))
            a = np.empty((rows.value, width.value) if width.value > 1 else (rows.value,), np.float32 if typ.value == 0 else np.uint32)
            nat.check(L.hry_curvature_copy(cx.h, c, name.encode(), a.ctypes.data, 0))
            assert a.shape == want[name].shape and np.array_equal(a.view(np.uint32), want[name].view(np.uint32)), name
    finally:
        L.hry_curvature_free(c)


# ---- 4. refusals: *out stays NULL and a good build follows
def test_refusals(cx):
    L = nat.load()
    good, other = mesh_of(cube_quads()), mesh_of(obtuse_sheet())
    held = []

    def build(fam, mesh, *args):
        h = C.c_void_p()
        nat.check(getattr(L, f"hry_{fam}_build")(cx.h, mesh.h, *args, C.byref(h)))
        held.append((fam, h))
        return h

    def refused(mesh, r, e, flags, code, *words):
        out = C.c_void_p(1)
        assert L.hry_curvature_build(cx.h, mesh.h if mesh is not None else None, r, e, flags, C.byref(out)) == code and not out.value
        text = L.hry_last_error().decode()
        assert all(w in text for w in words), text
        assert cx.curvature_numpy(good)["mean"].shape == (8,) and cx.curvature_stat()["interior"] == 8   # the context is as usable as before

    try:
        r = build("render", good)
        e = build("edges", good, r, 0)
        r2 = build("render", other)
        e2 = build("edges", other, r2, 0)
        refused(good, r, e, 1, nat.E_ARG, "unknown curvature flag")
        refused(good, r, e2, 0, nat.E_ARG, "not an edges build")
        refused(good, r2, e, 0, nat.E_ARG, "not a render build of this mesh")
        refused(good, None, e, 0, nat.E_ARG, "null argument")
        refused(good, r, None, 0, nat.E_ARG, "null argument")
        refused(None, r, e, 0, nat.E_ARG, "null argument")
        assert L.hry_curvature_build(cx.h, good.h, r, e, 0, None) == nat.E_ARG
        c = build("curvature", good, r, e, 0)
        assert L.hry_curvature_count(c) == 8
    finally:
        for fam, h in reversed(held):
            getattr(L, f"hry_{fam}_free")(h)


# ---- 5. the wrapper and the command line
def principal_of(mean, gaussian):
    r = np.sqrt(np.maximum(mean * mean - gaussian, np.float32(0)))
    return np.stack([mean + r, mean - r], axis=1)


def test_principal_numpy(cx):
    got = cx.curvature_numpy(gen(mg.icosphere(2)), principal=True)
    assert sorted(got) == sorted(hc.Codec.CURVATURE_BUFFERS + ("principal",)) and got["principal"].dtype == np.float32
    assert np.array_equal(got["principal"], principal_of(got["mean"], got["gaussian"])) and (got["principal"][:, 0] >= got["principal"][:, 1]).all()


TORCH_CHILD = r"""
import sys
import numpy as np
import torch
torch.cuda.init()   # a PyTorch program: torch holds the device before the codec starts
sys.path.insert(0, sys.argv[1])
from harry_amd import codec as hc
from harry_amd import meshgen as mg
from tests.test_gpu_curvature import principal_of
m = mg.with_nonmanifold(mg.torus(24, 16))
mesh = hc.Mesh.from_arrays(m.verts, m.degrees, m.indices)
c = hc.Codec(0)
ref = c.curvature_numpy(mesh)
got = c.curvature(mesh, principal=True)
st = c.curvature_stat()
assert sorted(got) == sorted(hc.Codec.CURVATURE_BUFFERS + ("principal",))
for k, a in ref.items():
    t = got[k]
    assert t.device == torch.device("cuda", 0) and t.dtype == (torch.float32 if a.dtype == np.float32 else torch.int32), k
    assert tuple(t.shape) == a.shape and np.array_equal(t.cpu().numpy().view(np.uint8), a.view(np.uint8)), k
# float32 products and differences are the same on both sides (separate kernels: nothing contracts); a device square root may differ
# from numpy's in its last place, so r does by one step of r and either row by that and its own rounding
p, want = got["principal"].cpu().numpy(), principal_of(ref["mean"], ref["gaussian"])
assert p.dtype == np.float32 and p.shape == want.shape
r = (want[:, 0] - want[:, 1]) / 2
assert (np.abs(p.astype(np.float64) - want) <= 2.0 ** -22 * (np.abs(ref["mean"]) + np.abs(r))[:, None]).all()
assert st["uploaded_bytes"] == 0 and st["vertices"] == mesh.nv and st["irregular"] > 0
c.close()
print("torch ok")
"""


def test_torch_tensors():
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD, util.ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "torch ok" in r.stdout, r.stdout + r.stderr


def test_curvature_option(tmp_path):
    pos, deg, idx = sm.hub_discs()
    want = cv.of_arrays(pos, deg, idx)
    (tmp_path / "in.ply").write_bytes(mg.Mesh(util.xyz(pos), deg, idx).to_ply())
    run = lambda *args: subprocess.run([cli.HARRY, str(tmp_path / "in.ply")] + list(args), capture_output=True, text=True, timeout=300)
    with_option, without = run(str(tmp_path / "a.hry"), "--curvature", "--creases", "30"), run(str(tmp_path / "b.hry"))
    assert with_option.returncode == 0 and without.returncode == 0, with_option.stdout + with_option.stderr + without.stderr
    lines = with_option.stdout.splitlines()
    (at,) = [i for i, l in enumerate(lines) if l.startswith("Curvature:")]
    (creases_at,) = [i for i, l in enumerate(lines) if l.startswith("Creases:")]
    assert creases_at < at < lines.index("Writing output...") and "Curvature:" not in without.stdout
    assert (tmp_path / "a.hry").read_bytes() == (tmp_path / "b.hry").read_bytes()
    alone = run("--curvature")
    assert alone.returncode == 0 and "Writing output" not in alone.stdout
    assert [l for l in alone.stdout.splitlines() if l.startswith("Curvature:")] == [lines[at]]
    words = lines[at].split()
    assert words[1::2] == ["vertices", "interior", "boundary", "irregular", "isolated", "degenerate", "area", "defect", "turns", "mean-integral"]
    assert tuple(int(w) for w in words[2:14:2]) == want["summary"]
    area, defect, turns, integral = (float(w) for w in words[14::2])
    # nine significant digits of a value within 2^-40 of its scale of the restatement's
    for printed, value, scale in ((area, want["totals"][0], want["scale"]["totals"][0]), (defect, want["totals"][1], want["scale"]["totals"][1]),
                                  (turns, want["totals"][1] / cv.TWO_PI, want["scale"]["totals"][1] / cv.TWO_PI), (integral, want["totals"][2], want["scale"]["totals"][2])):
        assert abs(printed - value) <= 5e-9 * abs(value) + cv.EPS * scale, (printed, value)
