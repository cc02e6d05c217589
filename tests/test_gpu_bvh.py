"""The hierarchy over a render build and the cast over it (include/harry_amd.h: hry_bvh_build, hry_bvh_cast; kernels:
harry_amd/csrc/device/bvh.hip, radix_sort.hpp) against the numpy restatement of tests/bvh_ref.py, which reads what the render build
holds and tests every ray against every leaf.  Every buffer, the summary and every cast output are compared bit for bit; no value is
left out and nothing has a tolerance."""
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
from tests import seam_meshes as sm
from tests import util
from tests.test_creases_cpu import cube_quads, cube_triangles
from tests.test_gpu_creases import gen, mesh_of, render_inputs

pytestmark = pytest.mark.gpu

# the sizes at which the kernels change strategy
SORT_TILE = 1024               # radix_sort.hpp: kRadixTile, the items one workgroup counts and scatters (four rounds of 256)
SCAN_BLOCK = sm.SCAN_BLOCK     # scan.hip: the counters one block of launch_excl_scan holds; a pass scans 256 per tile
BVH_BLOCK = 256                # bvh.hip: the threads of a block of the per-triangle, per-leaf and per-node kernels
CAST_BLOCK = 64                # bvh.hip: kCastBlock, the rays of one workgroup of the cast
RAY_COUNTS = [0, 1, 63, 64, 65, CAST_BLOCK - 1, CAST_BLOCK, CAST_BLOCK + 1, 2 * CAST_BLOCK + 1]


@pytest.fixture(scope="module")
def cx():
    c = hc.Codec(0)
    yield c
    c.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_build(cx, mesh, label):
    """the build against the restatement: every buffer, the summary and the stat; returns (the restatement, the Bvh)"""
    rn, pos = render_inputs(cx, mesh)
    want = br.build(rn["indices"], pos)
    b = cx.bvh(mesh)
    got, st = b.buffers_numpy(), cx.bvh_stat()
    assert sorted(got) == sorted(hc.Bvh.BUFFERS) == sorted(br.BUFFERS)
    for name in br.BUFFERS:
        assert same_bits(got[name], want[name]), (label, name, got[name].shape, want[name].shape)
    assert tuple(st[k] for k in br.SUMMARY) == want["summary"] == tuple(b.stat()[k] for k in br.SUMMARY), (label, st, want["summary"])
    assert st["uploaded_bytes"] == 0 and st["device_ms"] > 0 and b.count() == want["summary"][1]
    return want, b


def check_cast(b, want, origins, dirs, label, tmin=0.0, tmax=np.inf):
    got, ref = b.cast_numpy(origins, dirs, tmin, tmax), br.cast(want, origins, dirs, tmin, tmax)
    for k in ("tri", "t", "uv"):
        assert same_bits(got[k], ref[k]), (label, k, int((got[k] != ref[k]).sum()))
    assert b.hits == ref["hits"] and b.device_ms > 0, (label, b.hits, ref["hits"])
    return ref


def rays_for(want, n, seed):
    """the set of tests/bvh_ref.py, and behind it three rays that are not valid and eight from inside the scene box"""
    o, d = br.ray_set(want, n, seed)
    rng = np.random.default_rng(seed + 1)
    box = want["scene_box"][0] if want["summary"][1] else np.float32([0, 0, 0, 1, 1, 1])
    inside = ((box[:3] + box[3:]) / 2 + (box[3:] - box[:3]) * rng.uniform(-0.3, 0.3, (8, 3))).astype(np.float32)
    bad_o, bad_d = np.float32([[np.nan, 0, 0], [0, 0, 0], [0, 0, 0]]), np.float32([[0, 0, 1], [0, -0.0, 0], [0, np.inf, 1]])
    return np.concatenate([o, bad_o, inside]), np.concatenate([d, bad_d, rng.normal(size=(8, 3)).astype(np.float32)])


# ---- 1. meshes: every buffer and a cast, against the restatement
def copies(n):
    """n triangles in one place, on vertices of their own: one code, one digit bucket in every pass"""
    pos = np.tile(np.float32([[0.5, 0, 0], [1, 0.25, 0], [0, 1, 0.5]]), (n, 1))
    return pos, np.full(n, 3, np.uint8), np.arange(3 * n, dtype=np.uint32)


def with_dead(arrays, rows):
    pos, deg, idx = arrays
    pos = pos.copy()
    for i, (row, value) in enumerate(rows):
        pos[row, i % 3] = value
    return pos, deg, idx


def torus_obj_mesh():
    from tests.test_gpu_tangents import torus_obj   # an OBJ torus whose vt seams unweld the wrap's vertices
    return hc.Mesh.from_obj(torus_obj(), "")


MESHES = {
    "no_leaf": lambda: mesh_of(with_dead(sm.strip(1), [(0, np.nan)])),
    "one_leaf": lambda: mesh_of(sm.strip(1)),
    "two_leaves": lambda: mesh_of(sm.strip(2)),
    "three_leaves": lambda: mesh_of(sm.strip(3)),
    "tile_less_one": lambda: mesh_of(sm.strip(SORT_TILE - 1)),
    "tile": lambda: mesh_of(sm.strip(SORT_TILE)),
    "tile_and_one": lambda: mesh_of(sm.strip(SORT_TILE + 1)),
    "two_tiles_and_one": lambda: mesh_of(sm.strip(2 * SORT_TILE + 1)),
    "past_a_scan_block": lambda: gen(mg.torus(48, 44)),          # 4224 triangles: five tiles, 1280 counters a pass
    "one_code": lambda: mesh_of(copies(SORT_TILE + 1)),
    "distinct_codes": lambda: gen(mg.grid(5, 5)),
    "dead_in_a_tile": lambda: mesh_of(with_dead(sm.gen_arrays(mg.torus(24, 16)), [(100, np.nan), (101, np.inf), (230, -np.inf)])),
    "flat": lambda: mesh_of((np.float32([[x, y, 0] for y in range(9) for x in range(9)]), np.full(64, 4, np.uint8),
                             np.array([[9 * y + x, 9 * y + x + 1, 9 * y + x + 10, 9 * y + x + 9] for y in range(8) for x in range(8)], np.uint32).reshape(-1))),
    "a_point": lambda: mesh_of((np.tile(np.float32([[1, 2, 3]]), (7, 1)), np.full(5, 3, np.uint8), np.array([0, 1, 2, 2, 3, 4, 4, 5, 6, 0, 2, 4, 1, 3, 5], np.uint32))),
    "grid_quads": lambda: gen(mg.grid(9, 8, quads=True)),
    "torus_mixed": lambda: gen(mg.torus(24, 16, polys="mixed")),
    "obj_torus": torus_obj_mesh,
    "torus_nonmanifold": lambda: gen(mg.with_nonmanifold(mg.torus(24, 16))),
    "soup": lambda: gen(mg.soup(seed=7)),
    "cube_quads": lambda: mesh_of(cube_quads()),
}


@pytest.mark.parametrize("name", sorted(MESHES))
def test_against_the_restatement(cx, name):
    mesh = MESHES[name]()
    want, b = check_build(cx, mesh, name)
    T, L, dead, distinct, depth = want["summary"]
    o, d = rays_for(want, 240, seed=len(name))
    ref = check_cast(b, want, o, d, name)
    leaves = {"no_leaf": 0, "one_leaf": 1, "two_leaves": 2, "three_leaves": 3, "tile_less_one": SORT_TILE - 1, "tile": SORT_TILE, "tile_and_one": SORT_TILE + 1,
              "two_tiles_and_one": 2 * SORT_TILE + 1, "one_code": SORT_TILE + 1}
    if name in leaves:
        assert L == leaves[name] and dead == T - L
    if name == "no_leaf":
        assert T == 1 and ref["hits"] == 0 and not np.isfinite(want["scene_box"]).any()
    if name == "past_a_scan_block":
        assert 256 * -(-L // SORT_TILE) > SCAN_BLOCK and T > 4 * SCAN_BLOCK
    if name == "one_code":
        assert distinct == 1 and depth == 11   # 1025 equal codes: the tree rests on the eleven position bits
    if name == "distinct_codes":
        assert distinct == L > 1
    if name == "dead_in_a_tile":
        assert dead > 6 and L + dead == T and np.isfinite(want["scene_box"]).all()
    if name == "flat":
        assert want["scene_box"][0, 2] == want["scene_box"][0, 5] == 0 and (want["leaf_code"] & 0x09249249 == 0).all() and T == 128
    if name == "a_point":
        assert L == 5 and distinct == 1 and not want["leaf_code"].any()
    if name in ("grid_quads", "torus_mixed"):
        assert T > mesh.nf
    if name == "obj_torus":
        assert len(cx.render_numpy(mesh)["vertex_source"]) > mesh.nv
    if name not in ("no_leaf", "a_point", "one_leaf", "two_leaves", "three_leaves"):
        assert ref["hits"] > 20, ref["hits"]
    b.close()


# ---- 2. rays
@pytest.fixture(scope="module")
def torus(cx):
    want, b = check_build(cx, gen(mg.torus(24, 16)), "torus")
    o, d = br.ray_set(want, 3000, seed=3)
    yield want, b, o, d, br.cast(want, o, d)
    b.close()


def test_the_torus_set_and_the_pruning(torus):
    want, b, o, d, ref = torus
    n, L = len(o), want["summary"][1]
    assert n // 4 <= ref["hits"] <= n - n // 4   # of the restatement alone: the set hits with a quarter of its rays and misses with a quarter
    got = b.cast_numpy(o, d)
    for k in ("tri", "t", "uv"):
        assert same_bits(got[k], ref[k]), (k, int((got[k] != ref[k]).sum()))
    assert b.hits == ref["hits"]
    print("box tests per ray", b.box_tests / n, "of", 2 * L - 1, "nodes; cast", b.device_ms, "ms")
    assert 0 < b.box_tests / n <= (2 * L - 1) / 4, b.box_tests / n   # a walk that prunes nothing makes 2 L - 2


def test_the_flat_grid_set(cx):
    want, b = check_build(cx, MESHES["flat"](), "flat")
    o, d = br.ray_set(want, 3000, seed=3)
    ref = check_cast(b, want, o, d, "flat")
    assert 3000 // 4 <= ref["hits"] <= 3000 - 3000 // 4
    b.close()


@pytest.mark.parametrize("n", RAY_COUNTS)
def test_ray_counts(torus, n):
    want, b, o, d, ref = torus
    pick = np.arange(n) * 7 % len(o)
    got = b.cast_numpy(o[pick], d[pick])
    assert got["tri"].shape == (n,) and got["uv"].shape == (n, 2)
    assert same_bits(got["tri"], ref["tri"][pick]) and same_bits(got["t"], ref["t"][pick]) and same_bits(got["uv"], ref["uv"][pick])
    assert b.hits == int((ref["tri"][pick] != br.NO_ELEMENT).sum()) and (b.box_tests > 0) == (n > 0)


@pytest.mark.parametrize("stride", [12, 16, 32])
def test_strides_and_one_origin(torus, stride):
    want, b, o, d, ref = torus
    n = 500
    wide_o, wide_d = np.full((n, stride // 4), 7, np.float32), np.full((n + 1, stride // 4), 7, np.float32)
    wide_o[:, :3], wide_d[1:, -3:] = o[:n], d[:n]
    got = b.cast_numpy(wide_o[:, :3], wide_d[1:, -3:])
    assert wide_d[1:, -3:].strides[0] == stride
    assert same_bits(got["tri"], ref["tri"][:n]) and same_bits(got["t"], ref["t"][:n]) and same_bits(got["uv"], ref["uv"][:n])
    eye = np.float32([0.2, -0.1, 3.0])   # stride 0: one origin for all rays, towards points about the leaves' corners
    rng = np.random.default_rng(stride)
    aim = want["leaf_positions"].reshape(-1, 3)[rng.integers(0, 3 * len(want["leaf_tri"]), n)] + rng.normal(size=(n, 3)) * 0.2
    wide_d[1:, -3:] = (aim - eye).astype(np.float32)
    seen = check_cast(b, want, eye, wide_d[1:, -3:], f"one origin, stride {stride}")
    assert n // 4 <= seen["hits"] <= n - n // 8, seen["hits"]


def test_windows(torus):
    want, b, o, d, ref = torus
    o, d, first = o[:900], d[:900], ref["tri"][:900]
    cut = float(np.median(ref["t"][:900][first != br.NO_ELEMENT]))
    second = check_cast(b, want, o, d, "behind the cut", tmin=cut)
    moved = (first != br.NO_ELEMENT) & (ref["t"][:900] < cut)
    assert (second["tri"][moved] != first[moved]).all() and (second["tri"][moved] != br.NO_ELEMENT).sum() > 50   # the first hit is cut off: the second comes back
    check_cast(b, want, o, d, "before the cut", tmax=cut)
    check_cast(b, want, o, d, "a slab", tmin=cut * 0.9, tmax=cut * 1.1)
    check_cast(b, want, o, d, "behind the origin too", tmin=-np.inf)
    assert check_cast(b, want, o, d, "tmin > tmax", tmin=2.0, tmax=1.0)["hits"] == 0
    assert check_cast(b, want, o, d, "an infinite tmin", tmin=np.inf)["hits"] == 0


def test_origins_inside_the_mesh(torus):
    want, b, o, d, ref = torus
    rng = np.random.default_rng(9)
    a = rng.uniform(0, 2 * np.pi, 400)
    inside = np.stack([np.cos(a), np.sin(a), np.zeros(400)], axis=1).astype(np.float32)   # on the tube's centre circle
    r = check_cast(b, want, inside, rng.normal(size=(400, 3)).astype(np.float32), "from the tube")
    assert r["hits"] >= 399   # a closed tube (watertightness is not promised: a ray through an edge may slip out)


def test_two_builds_and_two_casts_are_bit_identical(cx, torus):
    want, b, o, d, ref = torus
    again = cx.bvh(gen(mg.torus(24, 16)))
    one, two = b.buffers_numpy(), again.buffers_numpy()
    for k in br.BUFFERS:
        assert same_bits(one[k], two[k]), k
    x, y = b.cast_numpy(o[:700], d[:700]), again.cast_numpy(o[:700], d[:700])
    for k in ("tri", "t", "uv"):
        assert same_bits(x[k], y[k]), k
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
from tests import bvh_ref as br
m = mg.torus(24, 16)
mesh = hc.Mesh.from_arrays(m.verts, m.degrees, m.indices)
c = hc.Codec(0)
b = c.bvh(mesh)
host = b.buffers_numpy()
dev = b.buffers()
for k, a in host.items():
    t = dev[k]
    assert t.device == torch.device("cuda", 0) and t.dtype == (torch.float32 if a.dtype == np.float32 else torch.int32), k
    assert tuple(t.shape) == a.shape and np.array_equal(t.cpu().numpy().view(np.uint8), a.view(np.uint8)), k
o, d = br.ray_set(host, 1000, seed=3)
ref = b.cast_numpy(o, d)
hits, tests = b.hits, b.box_tests
assert hits > 250
def same(got, n=len(o)):
    assert got["tri"].dtype == torch.int32 and got["t"].dtype == torch.float32 and tuple(got["uv"].shape) == (n, 2)
    for k in ("tri", "t", "uv"):
        assert np.array_equal(got[k].cpu().numpy().view(np.uint8), ref[k][:n].view(np.uint8)), k
to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
same(b.cast(to, td))                                   # HRY_CAST_HOST and device pointers: the same bits
assert b.hits == hits and b.box_tests == tests and b.device_ms > 0
assert int((b.cast(to, td)["tri"] == -1).sum()) == len(o) - hits
for width in (4, 8):                                   # strides of 16 and 32 bytes
    wo, wd = torch.full((len(o), width), 7.0, device="cuda"), torch.full((len(o), width), 7.0, device="cuda")
    wo[:, :3], wd[:, -3:] = to, td
    same(b.cast(wo[:, :3], wd[:, -3:]))
half = b.cast(to[::2], td[::2])                        # a stride of 24 bytes
assert np.array_equal(half["tri"].cpu().numpy().view(np.uint32), ref["tri"][::2])
eye = torch.tensor([0.2, -0.1, 3.0], device="cuda")    # stride 0
one = b.cast(eye, td)
want = b.cast_numpy(eye.cpu().numpy(), d)
for k in ("tri", "t", "uv"):
    assert np.array_equal(one[k].cpu().numpy().view(np.uint8), want[k].view(np.uint8)), k
wide = b.cast(eye.expand(len(o), 3), td)             # ... and as an expanded tensor
assert np.array_equal(wide["t"].cpu().numpy().view(np.uint8), want["t"].view(np.uint8))
assert tuple(b.cast(to[:0], td[:0])["tri"].shape) == (0,)
b.close()
c.close()
print("torch ok")
"""


def test_torch_tensors_and_device_pointers():
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD, util.ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "torch ok" in r.stdout, r.stdout + r.stderr


# ---- 4. ownership and refusals
def test_refusals(cx):
    """every refusal returns its code, *out stays NULL, and the context is as usable as before; the cast works after hry_render_free"""
    L = nat.load()
    good, other = mesh_of(cube_quads()), mesh_of(sm.strip(5))
    held = []

    def build(fam, mesh, *args):
        h = C.c_void_p()
        nat.check(getattr(L, f"hry_{fam}_build")(cx.h, mesh.h, *args, C.byref(h)))
        held.append((fam, h))
        return h

    def usable():
        b = cx.bvh(good)
        assert b.count() == 12 and b.cast_numpy([0.75, 0.25, -1.0], [[0.0, 0.0, 1.0]])["t"].tolist() == [1.0]
        b.close()

    def refused(mesh, r, flags, code, *words):
        out = C.c_void_p(1)
        assert L.hry_bvh_build(cx.h, mesh.h if mesh is not None else None, r, flags, C.byref(out)) == code and not out.value
        text = L.hry_last_error().decode()
        assert all(w in text for w in words), text
        usable()

    try:
        r, r2 = build("render", good), build("render", other)
        refused(good, r, 1, nat.E_ARG, "unknown bvh flag")
        refused(good, r2, 0, nat.E_ARG, "not a render build of this mesh")
        refused(good, None, 0, nat.E_ARG, "null argument")
        refused(None, r, 0, nat.E_ARG, "null argument")
        assert L.hry_bvh_build(cx.h, good.h, r, 0, None) == nat.E_ARG
        b = build("bvh", good, r, 0)
        L.hry_render_free(held.pop(0)[1])   # r: the hierarchy keeps its own positions
        o, d = np.float32([[0.75, 0.25, -1.0]] * 4), np.float32([[0, 0, 1]] * 4)
        tri, t, uv = np.zeros(4, np.uint32), np.zeros(4, np.float32), np.zeros((4, 2), np.float32)
        stat, ms = (C.c_uint64 * 2)(), C.c_double()

        def cast(n=4, o_ptr=o.ctypes.data, so=12, d_ptr=d.ctypes.data, sd=12, tmin=0.0, tmax=np.inf, flags=nat.CAST_HOST, tri_ptr=tri.ctypes.data, handle=b):
            return L.hry_bvh_cast(cx.h, handle, n, o_ptr, so, d_ptr, sd, tmin, tmax, flags, tri_ptr, t.ctypes.data, uv.ctypes.data, stat, C.byref(ms))

        assert cast() == 0 and tri.tolist() == [1] * 4 and t.tolist() == [1.0] * 4 and uv.tolist() == [[0.25, 0.5]] * 4 and list(stat)[0] == 4
        dev, rows = C.c_void_p(), C.c_uint64()
        nat.check(L.hry_bvh_get(b, b"leaf_positions", C.byref(dev), C.byref(rows), None, None))
        for code, kw, words in ((nat.E_ARG, dict(handle=None), "null argument"), (nat.E_ARG, dict(tri_ptr=None), "null argument"),
                                (nat.E_ARG, dict(o_ptr=None), "null argument"), (nat.E_ARG, dict(d_ptr=None), "null argument"),
                                (nat.E_ARG, dict(flags=2), "unknown cast flag"), (nat.E_ARG, dict(flags=3), "unknown cast flag"),
                                (nat.E_ARG, dict(so=6), "multiple of 4"), (nat.E_ARG, dict(sd=13), "multiple of 4"),
                                (nat.E_ARG, dict(tmin=np.nan), "NaN"), (nat.E_ARG, dict(tmax=np.nan), "NaN"),
                                (nat.E_ARG, dict(flags=0), "not device memory"),                       # host memory in a device cast
                                (nat.E_ARG, dict(o_ptr=dev.value), "device memory in a cast with")):   # device memory in a host cast
            tri[:] = 77
            assert cast(**kw) == code and all(w in L.hry_last_error().decode() for w in [words]), (kw, L.hry_last_error())
            assert tri.tolist() == [77] * 4   # nothing was written
            usable()
        tri[:] = 77
        assert cast(n=0, o_ptr=None, d_ptr=None, tri_ptr=None) == 0 and tri.tolist() == [77] * 4 and list(stat) == [0, 0]   # no rays: nothing is touched
        assert cast(tmin=2.0, tmax=1.0) == 0 and tri.tolist() == [br.NO_ELEMENT] * 4 and np.isinf(t).all()                 # no error: every ray misses
        assert L.hry_bvh_cast(cx.h, b, 4, o.ctypes.data, 12, d.ctypes.data, 12, 0.0, np.inf, nat.CAST_HOST, tri.ctypes.data, None, None, None, None) == 0
        assert tri.tolist() == [1] * 4   # t, uv, stat and device_ms may be left out
    finally:
        for fam, h in reversed(held):
            getattr(L, f"hry_{fam}_free")(h)


def test_a_mesh_without_positions_is_refused(cx):
    flat = np.zeros(3, np.dtype([("x", "<f4"), ("y", "<f4")]))   # no z: the position list the normals' rule refuses
    flat["x"], flat["y"] = [0, 1, 0], [0, 0, 1]
    mesh = hc.Mesh.from_arrays(flat, np.array([3], np.uint8), np.array([0, 1, 2], np.uint32))
    with pytest.raises(hc.HryError) as e:
        cx.bvh(mesh)
    assert e.value.code == nat.E_UNSUPPORTED and "position" in str(e.value)
    assert cx.bvh(mesh_of(cube_triangles())).count() == 12


# ---- 5. the command line
def test_bvh_option(cx, tmp_path):
    arrays = with_dead(sm.gen_arrays(mg.torus(24, 16)), [(100, np.nan)])
    want = br.of_arrays(*arrays)
    (tmp_path / "in.ply").write_bytes(mg.Mesh(util.xyz(arrays[0]), arrays[1], arrays[2]).to_ply())
    run = lambda *args: subprocess.run([cli.HARRY, str(tmp_path / "in.ply")] + list(args), capture_output=True, text=True, timeout=300)
    with_option, without = run(str(tmp_path / "a.hry"), "--bvh", "--curvature"), run(str(tmp_path / "b.hry"))
    assert with_option.returncode == 0 and without.returncode == 0, with_option.stdout + with_option.stderr + without.stderr
    lines = with_option.stdout.splitlines()
    (at,) = [i for i, l in enumerate(lines) if l.startswith("Bvh:")]
    (curvature_at,) = [i for i, l in enumerate(lines) if l.startswith("Curvature:")]
    assert curvature_at < at < lines.index("Writing output...") and "Bvh:" not in without.stdout
    assert (tmp_path / "a.hry").read_bytes() == (tmp_path / "b.hry").read_bytes()
    alone = run("--bvh")
    assert alone.returncode == 0 and "Writing output" not in alone.stdout
    assert [l for l in alone.stdout.splitlines() if l.startswith("Bvh:")] == [lines[at]]
    words = lines[at].split()
    assert words[1::2] == ["triangles", "leaves", "dead", "distinct-codes", "depth"]
    T, L, dead, distinct, depth = (int(w) for w in words[2::2])
    st = cx.bvh(mesh_of(arrays)).stat()
    assert (T, L, dead, distinct, depth) == want["summary"] == tuple(st[k] for k in br.SUMMARY) and dead > 0 and 1 <= depth <= 62
