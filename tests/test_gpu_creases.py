"""Hard edges and split normals of a render build (include/harry_amd.h: hry_creases_build; kernels: harry_amd/csrc/device/creases.hip,
dedup.hip with CreaseKey) against the numpy restatement of tests/creases_ref.py, which reads what the render build holds.  Integer
buffers and the summary's counts are compared exactly; normal components within creases_ref.TOL (2^-24, normals_ref's) on the
vertices the restatement's guard admits -- every test but the designed zeros asserts that it admits all.  Every comparison prints how
many values are not bit-equal (DESIGN.md "Creases" has the table)."""
import ctypes as C
import math
import subprocess
import sys

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import cli
from harry_amd import codec as hc
from harry_amd import meshgen as mg
from tests import creases_ref as cr
from tests import edges_ref as er
from tests import seam_meshes as sm
from tests import util
from tests.test_creases_cpu import cube_quads, cube_triangles, prism, prism_limits

pytestmark = pytest.mark.gpu

WEIGHTS = ("area", "angle")
COS30 = math.cos(math.radians(30.0))
LIMITS = (-1.0, COS30, 2.0)
# the sizes at which creases.hip changes strategy, and the ones it shares (tests/seam_meshes.py: WAVE, SCAN_BLOCK)
CREASE_SEG_MAX = 32    # kCreaseSegMax: a lane sums a group of up to so many slots, a workgroup a longer one
CREASE_RANGES = 256    # the ranges of a workgroup's sum (the threads of k_crs_hubs)
CREASE_BLOCK = 256     # the threads of a block of the per-edge, per-slot, per-triangle, per-group and per-split-vertex kernels


@pytest.fixture(scope="module")
def cx():
    c = hc.Codec(0)
    yield c
    c.close()


def mesh_of(arrays):
    pos, deg, idx = arrays
    return hc.Mesh.from_arrays(util.xyz(pos), np.asarray(deg, np.uint8), np.asarray(idx, np.uint32))


def gen(m):
    return hc.Mesh.from_arrays(m.verts, m.degrees, m.indices)


def render_inputs(cx, mesh):
    """what the contract reads of the mesh's render build: (its host arrays, the float rows of the positions [U, 3])"""
    L = nat.load()
    rn = cx.render_numpy(mesh)
    (pl,) = [l for l in range(mesh.nlists) if mesh.list_target(l) == 1 and L.hry_list_interp_ncomp(mesh.h, l, 0) >= 3]
    at = L.hry_list_interp_offset(mesh.h, pl, 0)
    return rn, np.ascontiguousarray(rn[f"list{pl}"][:, at:at + 3])


def not_bit_equal(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


def compare(got, want, label, zeros_by_design=False):
    for name in cr.INTEGER:
        assert got[name].dtype == np.uint32 and got[name].shape == want[name].shape, (label, name, got[name].shape, want[name].shape)
        assert np.array_equal(got[name], want[name]), (label, name)
    g, w, guard = got["normals"], want["normals"], want["guard"]
    assert g.dtype == np.float32 and g.shape == w.shape
    if zeros_by_design:   # an exact cancellation is exact on both sides: zero rows, bit for bit
        assert not guard.all() and not g[~guard].view(np.uint32).any() and not w[~guard].view(np.uint32).any(), label
    else:
        assert guard.all(), (label, "the guard excludes", int((~guard).sum()))
    zero = ~w.any(axis=1)
    assert np.array_equal(~g.any(axis=1), zero) and not g[zero].view(np.uint32).any(), label
    err = float(np.abs(g[guard].astype(np.float64) - w[guard]).max()) if guard.any() else 0.0
    print("CREASES", label, "normals: values not bit-equal:", not_bit_equal(g, w), "of", g.size, "largest difference:", err)
    assert err <= cr.TOL, (label, err)


def check(cx, mesh, label, cases=None, zeros_by_design=False):
    """the build against the restatement at every (weights, limit) of `cases` (default: both weightings at LIMITS), with the
    summary, the stat and the gathered positions; returns {(weights, limit): (the restatement, the buffers)}"""
    rn, pos = render_inputs(cx, mesh)
    edges = er.build(rn["indices"], rn["vertex_source"], pos)
    out, topo = {}, {}
    for weights, limit in cases or [(w, l) for l in LIMITS for w in WEIGHTS]:
        if limit not in topo:
            topo[limit] = cr.topology(rn["indices"], rn["vertex_source"], rn["tri_face"], pos, limit, edges)
        want = cr.build(rn["indices"], rn["vertex_source"], rn["tri_face"], pos, limit, weights, topo=topo[limit])
        got = cx.creases_numpy(mesh, cos_limit=limit, weights=weights)
        st = cx.creases_stat()
        assert sorted(got) == sorted(hc.Codec.CREASES_BUFFERS + ("positions",))
        assert st["uploaded_bytes"] == 0 and (st["device_ms"] > 0 or not len(rn["indices"])) and st["cos_limit"] == limit
        assert tuple(st[k] for k in cr.SUMMARY) == want["summary"], (label, weights, limit, st, want["summary"])
        compare(got, want, f"{label} {weights} {limit:.3g}", zeros_by_design)
        assert np.array_equal(got["positions"].view(np.uint32), pos[got["render_vertex"]].view(np.uint32))
        out[weights, limit] = (want, got)
    return out


# ---- 1. against the restatement: both weightings at the limits -1, cos 30 degrees and 2
def torus_obj_mesh():
    from tests.test_gpu_tangents import torus_obj   # an OBJ torus whose vt seams unweld the wrap's vertices
    return hc.Mesh.from_obj(torus_obj(), "")


MESHES = {
    "grid_triangles": lambda: gen(mg.grid(9, 8)),
    "grid_quads": lambda: gen(mg.grid(9, 8, quads=True)),
    "icosphere": lambda: gen(mg.icosphere(2)),
    "torus": lambda: gen(mg.torus(24, 16)),
    "torus_mixed": lambda: gen(mg.torus(24, 16, polys="mixed")),
    "torus_nonmanifold": lambda: gen(mg.with_nonmanifold(mg.torus(24, 16))),
    "soup": lambda: gen(mg.soup(seed=7)),   # (the default seed folds three fans so sharply that their sums nearly cancel: the guard's case)
    "one_triangle": lambda: util.xyz_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]]),
    "cube_quads": lambda: mesh_of(cube_quads()),
    "cube_triangles": lambda: mesh_of(cube_triangles()),
    "prism6": lambda: mesh_of(prism(6)),
    "prism32": lambda: mesh_of(prism(32)),
    "prism33": lambda: mesh_of(prism(33)),
    "prism40": lambda: mesh_of(prism(40)),
    "obj_torus": torus_obj_mesh,
}


@pytest.mark.parametrize("name", sorted(MESHES))
def test_against_the_restatement(cx, name):
    mesh = MESHES[name]()
    r = check(cx, mesh, name)
    flat = r["area", 2.0][0]["summary"]
    assert flat[0] == flat[1]   # flat shading: only the corners of one polygon share a vertex, and those share a group
    if name == "cube_quads":
        assert r["area", -1.0][0]["summary"] == (8, 8, 18, 0, 0, 0) and r["area", COS30][0]["summary"] == (24, 24, 6, 12, 8, 0)
    if name == "obj_torus":   # the seams split vertices, not normals: W = U, and fewer groups than vertices
        s = r["area", -1.0][0]["summary"]
        assert s[0] == cx.render_numpy(mesh)["vertex_source"].shape[0] > mesh.nv == s[1] and s[3:] == (0, 0, 0)
    if name in ("torus_nonmanifold", "soup"):
        assert r["area", -1.0][0]["summary"][5] > 0


def test_cube_and_prisms_have_the_closed_forms(cx):
    r = check(cx, mesh_of(cube_quads()), "cube at equality", [(w, l) for w in WEIGHTS for l in (0.0, float(np.nextafter(0.0, 1.0)), math.cos(math.radians(90)))])
    for w in WEIGHTS:
        assert r[w, 0.0][0]["summary"] == (8, 8, 18, 0, 0, 0)
        for l in (float(np.nextafter(0.0, 1.0)), math.cos(math.radians(90))):
            assert r[w, l][0]["summary"] == (24, 24, 6, 12, 8, 0)
            assert np.array_equal(np.abs(r[w, l][1]["normals"]).sum(axis=1), np.ones(24)) and (np.abs(r[w, l][1]["normals"]).max(axis=1) == 1).all()
    r = check(cx, mesh_of(cube_triangles()), "cube of triangles", [("area", 1.0), ("area", 2.0)])
    assert r["area", 1.0][0]["summary"][0] == 24 and r["area", 2.0][0]["summary"][0] == 36
    for n in (6, 32, 33, 40):
        smooth_sides, sharp_sides = prism_limits(n)
        r = check(cx, mesh_of(prism(n)), f"prism {n}", [("area", smooth_sides), ("angle", sharp_sides)])
        assert r["area", smooth_sides][1]["normals"].shape[0] == 4 * n + 2 and r["angle", sharp_sides][1]["normals"].shape[0] == 6 * n + 2
        for want, got in r.values():
            assert np.array_equal(got["normals"][got["indices"][:n].reshape(-1)], np.tile(np.float32([0, 0, -1]), (3 * n, 1)))
            assert np.array_equal(got["normals"][got["indices"][n:2 * n].reshape(-1)], np.tile(np.float32([0, 0, 1]), (3 * n, 1)))


# ---- 2. the seams of the kernels
SEAM_CASES = [("area", -1.0), ("angle", -1.0), ("area", COS30)]
STRIPS = {                                # triangles: what lies either side of which size
    21: "63 slots", 22: "66 slots: a dedup wavefront",
    85: "255 slots", 86: "258 slots: CREASE_BLOCK slots",
    127: "255 edges", 128: "257 edges: CREASE_BLOCK edges",
    254: "256 groups", 255: "257 groups: CREASE_BLOCK groups and split vertices",
    256: "256 triangles", 257: "257 triangles: CREASE_BLOCK triangles",
    341: "1023 slots", 342: "1026 slots: the scan block of sm.SCAN_BLOCK flags",
}
CAP_SLOTS = [CREASE_SEG_MAX - 1, CREASE_SEG_MAX, CREASE_SEG_MAX + 1, CREASE_RANGES - 1, CREASE_RANGES, CREASE_RANGES + 1, 300]


@pytest.mark.parametrize("ntri", sorted(STRIPS))
def test_strips(cx, ntri):
    r = check(cx, mesh_of(sm.strip(ntri)), f"strip {ntri}", SEAM_CASES)
    s = r["area", -1.0][0]["summary"]
    assert s[:2] == (ntri + 2, ntri + 2) and s[2] + s[5] == 2 * ntri + 1   # a vertex per group; the edges of a strip


@pytest.mark.parametrize("n", CAP_SLOTS)
def test_cap_centres(cx, n):
    """the centre of a prism's cap is one smooth group of n slots: the lane's sum up to 32, the workgroup's ranges beyond -- of one
    slot up to 256 of them, of two from 257 on"""
    limit = prism_limits(n)[0]
    r = check(cx, mesh_of(prism(n)), f"cap {n}", [("area", limit), ("angle", limit)])
    for want, got in r.values():
        assert sorted(want["group_slots"].tolist())[-2:] == [n, n] and sorted(want["group_slots"].tolist())[-3] <= 3
        assert np.array_equal(got["normals"][got["indices"][:n, 0]], np.tile(np.float32([0, 0, -1]), (n, 1)))
        assert np.array_equal(got["normals"][got["indices"][n:2 * n, 0]], np.tile(np.float32([0, 0, 1]), (n, 1)))


def test_shuffled_torus(cx):
    """neighbours lie far apart: every union leaves its tile, and the groups' slots come from all over the slot range"""
    mesh = sm.shuffled_torus()
    r = check(cx, mesh_of(mesh), "shuffled torus", [("area", -1.0), ("angle", COS30)])
    assert r["area", -1.0][0]["summary"][:2] == (len(mesh[0]), len(mesh[0]))


# ---- 3. designed zeros
def test_opposed_triangles_cancel_exactly(cx):
    # two triangles folded onto each other across the edge 0 - 1: edge_cos is exactly -1, smooth at the limit -1, and the two normals
    # at either end of the edge cancel exactly (integer coordinates: every product and sum is exact)
    mesh = util.xyz_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 1, 0]], [[0, 1, 2], [1, 0, 3]])
    for (weights, _), (want, got) in check(cx, mesh, "opposed", [("area", -1.0), ("angle", -1.0)], zeros_by_design=True).items():
        assert want["summary"] == (4, 4, 1, 0, 0, 4)
        zero = ~got["normals"].any(axis=1)
        assert sorted(got["vertex_source"][zero].tolist()) == [0, 1] and np.array_equal(np.abs(got["normals"][~zero]), np.tile(np.float32([0, 0, 1]), (2, 1)))
    sharp = check(cx, mesh, "opposed, sharp", [("area", float(np.nextafter(-1.0, 0.0)))])["area", float(np.nextafter(-1.0, 0.0))][1]
    assert sharp["normals"].any(axis=1).all() and len(sharp["normals"]) == 6


def test_degenerate_triangles(cx):
    pos = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.1],      # a proper pair of triangles
           [2, 2, 0],                                          # ... and a sliver on their edge 1 - 3 with no area: 1, 3 and their midpoint
           [3, 0, 0], [4, 0, 0], [5, 0, 0],                    # three points on a line
           [7, 0, 0], [7, 0, 0], [8, 1, 0]]                    # two corners in one place
    pos[4] = [1, 0.5, 0.05]
    mesh = util.xyz_mesh(pos, [[0, 1, 2], [1, 3, 2], [3, 1, 4], [5, 6, 7], [8, 9, 10]])
    for (weights, limit), (want, got) in check(cx, mesh, "degenerate").items():
        assert (want["edge_class"] == cr.DEGENERATE).sum() == 1   # the edge 1 - 3: one of its triangles has no normal
        zero = ~got["normals"].any(axis=1)
        # the sliver's corners stand alone (at 1 and 3 beside the proper triangles' split vertices), like the other triangles without area
        assert set(got["vertex_source"][zero].tolist()) == {1, 3, 4, 5, 6, 7, 8, 9, 10} and set(got["vertex_source"][~zero].tolist()) == {0, 1, 2, 3}


def test_nan_position_poisons_only_its_own_groups(cx):
    m = mg.grid(6, 6)
    clean = check(cx, gen(m), "grid 6 x 6", [("area", -1.0)])["area", -1.0][1]
    bad = 14
    verts = m.verts.copy()
    verts["x"][bad] = np.nan
    r = check(cx, hc.Mesh.from_arrays(verts, m.degrees, m.indices), "grid 6 x 6 with a NaN")
    tris = m.indices.reshape(-1, 3)
    poisoned = (tris == bad).any(axis=1)
    near = np.isin(tris, np.unique(tris[poisoned]))   # slots at a vertex of a poisoned triangle
    for (weights, limit), (want, got) in r.items():
        assert not np.isnan(got["normals"]).any()
        assert not got["normals"][got["indices"][poisoned].reshape(-1)].any()          # the poisoned triangles' own corners: zeros
        assert got["normals"][got["indices"][~poisoned].reshape(-1)].any(axis=1).all()  # every other corner has a normal
        assert (want["edge_class"] == cr.DEGENERATE).sum() == 12   # the six spokes at the vertex and the rim of its fan
    got = r["area", -1.0][1]
    away = ~near
    assert away.any() and np.array_equal(got["normals"][got["indices"][away]].view(np.uint32), clean["normals"][clean["indices"][away]].view(np.uint32))


# ---- 4. determinism and residency
def same_bits(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_three_builds_are_bit_identical(cx):
    mesh = mesh_of(sm.join([prism(300), sm.gen_arrays(mg.torus(24, 16))]))
    for weights in WEIGHTS:
        for limit in (-1.0, COS30):
            first = cx.creases_numpy(mesh, cos_limit=limit, weights=weights)
            for _ in range(2):
                same_bits(cx.creases_numpy(mesh, cos_limit=limit, weights=weights), first)


@pytest.mark.parametrize("profile", [hc.PROFILE_COMPAT, hc.PROFILE_CHUNKED], ids=["compat", "chunked"])
@pytest.mark.parametrize("bits", [0, 12], ids=["lossless", "q12"])
def test_resident_and_uploaded(cx, profile, bits):
    m = gen(mg.torus(24, 16, polys="mixed"))
    if bits:
        cx.requant(m, [(1, -1, bits)])
    dec = cx.read_hry(cx.write_hry(m, profile=profile))
    resident = cx.creases_numpy(dec, angle=20.0)   # (a render build leaves the decode's buffers where they are)
    assert cx.creases_stat()["render_uploaded_bytes"] == 0 and cx.creases_stat()["uploaded_bytes"] == 0
    rn, pos = render_inputs(cx, dec)
    compare(resident, cr.build(rn["indices"], rn["vertex_source"], rn["tri_face"], pos, math.cos(math.radians(20.0))), f"resident {bits}")
    up = dec.clone()
    same_bits(cx.creases_numpy(up, angle=20.0), resident)
    assert cx.creases_stat()["render_uploaded_bytes"] > 0 and cx.creases_stat()["uploaded_bytes"] == 0


def test_inputs_freed_before_the_buffers_are_read(cx):
    L = nat.load()
    mesh = mesh_of(prism(40))
    want = cx.creases_numpy(mesh, cos_limit=0.5)
    r, e, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
    nat.check(L.hry_render_build(cx.h, mesh.h, C.byref(r)))
    nat.check(L.hry_edges_build(cx.h, mesh.h, r, nat.EDGES_GEOMETRY, C.byref(e)))
    nat.check(L.hry_creases_build(cx.h, mesh.h, r, e, 0.5, 0, C.byref(c)))
    L.hry_edges_free(e)
    L.hry_render_free(r)
    try:
        assert L.hry_creases_count(c) == len(want["normals"])
        d, up = C.c_double(), C.c_uint64(7)
        nat.check(L.hry_creases_stat(c, C.byref(d), C.byref(up)))
        assert up.value == 0 and d.value > 0
        for name in hc.Codec.CREASES_BUFFERS:
            rows, width, typ = C.c_uint64(), C.c_int(), C.c_int()
            nat.check(L.hry_creases_get(c, name.encode(), None, C.byref(rows), C.byref(width), C.byref(typ)))
            a = np.empty((rows.value, width.value) if width.value > 1 else (rows.value,), np.float32 if typ.value == 0 else np.uint32)
            nat.check(L.hry_creases_copy(cx.h, c, name.encode(), a.ctypes.data, 0))
            assert a.shape == want[name].shape and np.array_equal(a.view(np.uint32), want[name].view(np.uint32)), name
    finally:
        L.hry_creases_free(c)


# ---- 5. refusals: *out stays NULL and a good build follows
def test_refusals(cx):
    L = nat.load()
    good, other = mesh_of(cube_quads()), mesh_of(prism(6))
    held = []

    def build(fam, mesh, *args):
        h = C.c_void_p()
        nat.check(getattr(L, f"hry_{fam}_build")(cx.h, mesh.h, *args, C.byref(h)))
        held.append((fam, h))
        return h

    def refused(mesh, r, e, limit, flags, code, *words):
        out = C.c_void_p(1)
        assert L.hry_creases_build(cx.h, mesh.h, r, e, limit, flags, C.byref(out)) == code and not out.value
        text = L.hry_last_error().decode()
        assert all(w in text for w in words), text
        assert cx.creases_numpy(good, cos_limit=0.5)["normals"].shape == (24, 3)   # the context is as usable as before

    try:
        r = build("render", good)
        plain, geo = build("edges", good, r, 0), build("edges", good, r, nat.EDGES_GEOMETRY)
        r2 = build("render", other)
        geo2 = build("edges", other, r2, nat.EDGES_GEOMETRY)
        refused(good, r, plain, 0.5, 0, nat.E_ARG, "HRY_EDGES_GEOMETRY")
        refused(good, r, geo, float("nan"), 0, nat.E_ARG, "limit")
        refused(good, r, geo, 0.5, 2, nat.E_ARG, "unknown creases flag")
        refused(good, r2, geo, 0.5, 0, nat.E_ARG, "not a render build of this mesh")
        refused(good, r, geo2, 0.5, 0, nat.E_ARG, "not an edges build")
        refused(other, r, geo, 0.5, 0, nat.E_ARG, "not a render build of this mesh")
        out = C.c_void_p(1)
        assert L.hry_creases_build(cx.h, good.h, r, None, 0.5, 0, C.byref(out)) == nat.E_ARG and not out.value
        for limit in (-np.inf, np.inf, -1.0, 2.0):   # every limit but NaN is legal
            c = build("creases", good, r, geo, limit, 0)
            assert L.hry_creases_count(c) == (8 if limit < 0 else 24)
    finally:
        for fam, h in reversed(held):
            getattr(L, f"hry_{fam}_free")(h)


# ---- 6. torch tensors
TORCH_CHILD = r"""
import sys
import numpy as np
import torch
torch.cuda.init()   # a PyTorch program: torch holds the device before the codec starts
sys.path.insert(0, sys.argv[1])
from harry_amd import codec as hc
from tests.test_creases_cpu import prism
from tests.test_gpu_creases import mesh_of
mesh = mesh_of(prism(40))
c = hc.Codec(0)
for weights in ("area", "angle"):
    ref = c.creases_numpy(mesh, angle=30.0, weights=weights)
    got = c.creases(mesh, angle=30.0, weights=weights)
    assert sorted(got) == sorted(ref) == sorted(hc.Codec.CREASES_BUFFERS + ("positions",))
    for k, t in got.items():
        assert t.device == torch.device("cuda", 0) and t.dtype == (torch.float32 if ref[k].dtype == np.float32 else torch.int32), k
        assert tuple(t.shape) == ref[k].shape and np.array_equal(t.cpu().numpy().view(np.uint8), ref[k].view(np.uint8)), k
    rows = c.render(mesh)["list1"]
    assert torch.equal(got["positions"], rows[got["render_vertex"].long(), :3])
st = c.creases_stat()
assert st["vertices"] == 4 * 40 + 2 == len(got["normals"]) and st["uploaded_bytes"] == 0
c.close()
print("torch ok")
"""


def test_torch_tensors():
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD, util.ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "torch ok" in r.stdout, r.stdout + r.stderr


# ---- 7. the command line
def test_creases_option(tmp_path):
    pos, deg, idx = cube_quads()
    (tmp_path / "cube.ply").write_bytes(mg.Mesh(util.xyz(pos), deg, idx).to_ply())
    with_option = subprocess.run([cli.HARRY, str(tmp_path / "cube.ply"), str(tmp_path / "a.hry"), "--creases", "30"], capture_output=True, text=True, timeout=300)
    without = subprocess.run([cli.HARRY, str(tmp_path / "cube.ply"), str(tmp_path / "b.hry")], capture_output=True, text=True, timeout=300)
    assert with_option.returncode == 0 and without.returncode == 0, with_option.stdout + with_option.stderr + without.stderr
    lines = [l for l in with_option.stdout.splitlines() if l.startswith("Creases:")]
    assert lines == ["Creases: angle 30 vertices 24 groups 24 smooth 6 sharp 12 split 8 other 0"] and "Creases:" not in without.stdout
    assert (tmp_path / "a.hry").read_bytes() == (tmp_path / "b.hry").read_bytes()
    alone = subprocess.run([cli.HARRY, str(tmp_path / "cube.ply"), "--creases=90"], capture_output=True, text=True, timeout=300)
    assert alone.returncode == 0 and "Writing output" not in alone.stdout
    assert [l for l in alone.stdout.splitlines() if l.startswith("Creases:")] == ["Creases: angle 90 vertices 24 groups 24 smooth 6 sharp 12 split 8 other 0"]
