"""The rate sweep on the GPU (include/harry_amd.h: hry_rate_sweep_build; kernel: harry_amd/csrc/device/rate.hip) through
Codec.rate_sweep.  The yardstick is the encoder itself, which is pinned to the reference's bytes: Codec.requant of a clone to a width,
Codec.write_hry(clone, keep_stages=True), and np.bincount of the rows of its "vplanes" stage must EQUAL the sweep's histograms --
counts, no tolerance.  bytes() against the numpy entropy of tests/rate_sweep_ref.py within 1e-12 relative (derived there)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import cli
from harry_amd import codec as hc
from harry_amd import meshgen as mg
from tests import rate_sweep_ref as rref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
PROFILES = {"compat": hc.PROFILE_COMPAT, "chunked": hc.PROFILE_CHUNKED}
WIDTHS = (1, 7, 8, 9, 16, 17, 24, 25, 30)   # where the storage type changes, and where float(2^q - 1) stops being exact
BLOCK = 256                                  # coded vertices per block (kRateBlock)
ENC_CAND = 8                                 # candidates kept per vertex (kEncCand): a fan with more walks again per component
NO_FACES = (np.zeros(0, np.uint8), np.zeros(0, np.uint32))
REL = 1e-12


@pytest.fixture(scope="module")
def cx():
    c = hc.Codec(0)
    yield c
    c.close()


def refused(code, fn, *args, **kw):
    with pytest.raises(hc.HryError) as e:
        fn(*args, **kw)
    assert e.value.code == code, e.value
    return e.value


def encoder_hists(cx, m: hc.Mesh, quants=(), profile="compat"):
    """(coded, {component: [planes, 256] counts}) of list 1 from the encoder's own byte planes for a clone of m after `quants`"""
    clone = m.clone()
    if quants:
        cx.requant(clone, list(quants))
    cx.write_hry(clone, profile=PROFILES[profile], keep_stages=True)
    sizes = [hc.TYPE_SIZE[hc.storage_type(t, q)] for t, q, _ in clone.list_fmt(1)]
    nplanes = sum(sizes)
    coded = len(cx.stage("order_v", np.uint32))
    planes = cx.stage("vplanes").reshape(nplanes, coded)
    out, first = {}, 0
    for c, n in enumerate(sizes):
        out[c] = np.stack([np.bincount(planes[first + b], minlength=256) for b in range(n)]).astype(np.uint32)
        first += n
    return coded, out


def check_width(cx, m, s, q, comps=None, profile="compat"):
    """the table at q bits against the encoder: every swept component of list 1 (or `comps`) that has the width goes to q on one clone"""
    comps = [c for c in (range(len(m.list_fmt(1))) if comps is None else comps) if s.bits(1, c) >= q]
    assert comps
    coded, want = encoder_hists(cx, m, [(1, c, q) for c in comps], profile)
    assert coded == s.coded
    for c in comps:
        got = s.hist(1, c, q)
        assert got.shape == (rref.planes_at(q), 256) == want[c].shape and got.dtype == np.uint32
        assert np.array_equal(got, want[c]), (c, q, np.argwhere(got != want[c])[:4])
        assert (got.sum(axis=1) == coded).all()
    return len(comps)


def check_row0(cx, m, s, comps=None, profile="compat"):
    coded, want = encoder_hists(cx, m, (), profile)
    assert coded == s.coded
    for c in (range(len(m.list_fmt(1))) if comps is None else comps):
        got = s.hist(1, c, 0)
        assert got.shape == want[c].shape and np.array_equal(got, want[c]), (c, np.argwhere(got != want[c])[:4])
        assert (got.sum(axis=1) == coded).all()


def tables(s, m) -> list:
    return [s.hist(1, c, q) for c in range(len(m.list_fmt(1))) for q in range(0, s.bits(1, c) + 1) if q or s.planes(1, c, 0)]


def with_unreferenced(gen: mg.Mesh, extra: int) -> mg.Mesh:
    v = np.concatenate([gen.verts, np.zeros(extra, gen.verts.dtype)])
    for k, n in enumerate(v.dtype.names):
        v[n][gen.nv:] = np.linspace(-2.0 - k, 2.0 + k, extra)
    return mg.Mesh(v, gen.degrees, gen.indices, gen.face_props)


HUB = 40
MESHES = {
    "torus": lambda: mg.torus(24, 16),
    "mixed": lambda: mg.torus(24, 16, polys="mixed"),
    "grid_quads": lambda: mg.grid(9, 8, quads=True),
    "nonmanifold": lambda: mg.with_nonmanifold(mg.torus(12, 10)),
    "multi_unreferenced": lambda: with_unreferenced(mg.multi_component(5, 8, 9), 7),
    "soup": lambda: mg.soup(),
    "hubs": lambda: mg.hub_discs([HUB, 5, 3 * ENC_CAND]),
}


@pytest.fixture(scope="module")
def swept(cx):
    """every mesh of MESHES with its sweep, built once"""
    out = {}
    for name, make in MESHES.items():
        gen = make()
        m = hc.Mesh.from_ply(gen.to_ply())
        out[name] = (gen, m, cx.rate_sweep(m))
    yield out
    for _, _, s in out.values():
        s.close()


# ---- 1. every mesh at the widths where something changes; all three position components on one clone: one encode per width
@pytest.mark.parametrize("name", sorted(MESHES))
def test_histograms_equal_the_encoders_planes(cx, swept, name):
    gen, m, s = swept[name]
    assert [s.bits(1, c) for c in range(3)] == [30, 30, 30] and 0 < s.coded <= m.nv
    for q in WIDTHS:
        assert check_width(cx, m, s, q) == 3
    check_row0(cx, m, s)
    if name == "multi_unreferenced":
        assert s.coded == m.nv - 7 < m.nv                 # vertices no face names are not coded
    if name == "hubs":
        valence = np.bincount(gen.indices.astype(np.int64))
        assert valence.max() == HUB > ENC_CAND            # the hub's fan holds more candidates than are kept: it walks again per component
    for t in tables(s, m):
        assert (t.sum(axis=1) == s.coded).all()


def test_every_width_on_the_smallest_mesh(cx, swept):
    _, m, s = swept["soup"]
    for q in range(1, 31):
        assert check_width(cx, m, s, q) == 3
    refused(nat.E_ARG, s.hist, 1, 0, 31)


def test_one_component_quantised_alone(cx, swept):
    """the components of a vertex are predicted independently: the table of y holds with x and z lossless, and beside other widths"""
    _, m, s = swept["torus"]
    for q in (7, 12, 17):
        assert check_width(cx, m, s, q, comps=[1]) == 1
    coded, want = encoder_hists(cx, m, [(1, 0, 5), (1, 1, 12), (1, 2, 20)])
    for c, q in ((0, 5), (1, 12), (2, 20)):
        assert np.array_equal(s.hist(1, c, q), want[c])


@pytest.mark.parametrize("name", ["mixed", "multi_unreferenced"])
def test_the_other_profile_writes_the_same_planes(cx, swept, name):
    _, m, s = swept[name]
    for q in (8, 9, 17):
        assert check_width(cx, m, s, q, profile="chunked") == 3
    check_row0(cx, m, s, profile="chunked")


# ---- 2. row 0: the mesh as it stands
def test_row_0_with_colours_integer_properties_and_a_quantised_component(cx):
    gen = mg.with_integer_props(mg.with_colors(mg.torus(12, 10)))
    m = hc.Mesh.from_ply(gen.to_ply())
    cx.requant(m, [(1, 1, 11)])                      # y is quantised already: not swept, but counted as it stands
    s = cx.rate_sweep(m)
    ncomp = len(m.list_fmt(1))
    assert ncomp == 12
    assert s.bits(1, 1) == 0 and s.reason(1, 1) == "already quantised" and s.planes(1, 1, 0) == 2
    assert [s.planes(1, c, 0) for c in range(ncomp)] == [hc.TYPE_SIZE[hc.storage_type(t, q)] for t, q, _ in m.list_fmt(1)]
    check_row0(cx, m, s)
    check_row0(cx, m, s, profile="chunked")
    swept_comps = [c for c in range(ncomp) if s.bits(1, c)]
    assert 0 in swept_comps and 3 in swept_comps and 1 not in swept_comps
    for q in (1, 8):
        assert check_width(cx, m, s, q) == len(swept_comps)
    refused(nat.E_UNSUPPORTED, s.hist, 1, 1, 4)
    refused(nat.E_UNSUPPORTED, s.choose, 1, 1, 1e9)
    s.close()


# ---- 3. a component of each of the ten types on a torus, at the boundary widths each type has
TYPES = [("f", "<f4"), ("d", "<f8"), ("ul", "<u8"), ("l", "<i8"), ("ui", "<u4"), ("i", "<i4"), ("us", "<u2"), ("s", "<i2"), ("uc", "u1"), ("c", "i1")]
RANGES = {"ul": (0, 10 ** 6), "l": (-10 ** 6, 10 ** 6), "ui": (0, 50000), "i": (-1000, 1000), "us": (0, 1000), "s": (-300, 300), "uc": (0, 200), "c": (-50, 50)}
QMAX = [30, 30, 30, 30, 30, 30, 16, 16, 8, 8]


@pytest.fixture(scope="module")
def typed(cx):
    gen = mg.torus(12, 10)
    rng = np.random.default_rng(11)
    v = np.zeros(gen.nv, np.dtype([(n, gen.verts.dtype[n]) for n in gen.verts.dtype.names] + TYPES + [("ci", "<i4")]))
    for n in gen.verts.dtype.names:
        v[n] = gen.verts[n]
    v["f"] = rng.normal(0.0, 3.0, gen.nv)
    v["d"] = rng.normal(0.0, 100.0, gen.nv)
    for n, (lo, hi) in RANGES.items():
        v[n] = rng.integers(lo, hi + 1, gen.nv)
    v["ci"] = -17
    m = hc.Mesh.from_arrays(v, gen.degrees, gen.indices)
    assert [t for t, _, _ in m.list_fmt(1)][3:13] == list(range(10))
    s = cx.rate_sweep(m)
    yield m, s
    s.close()


@pytest.mark.parametrize("q", [1, 7, 8, 9, 15, 16, 17, 25, 30])
def test_every_type_at_its_boundary_widths(cx, typed, q):
    m, s = typed
    assert [s.bits(1, c) for c in range(3, 13)] == QMAX
    # the double has every width and is quantised in every clone: the encoder refuses it lossless
    assert check_width(cx, m, s, q) == 3 + sum(1 for b in QMAX if b >= q)
    for c, b in enumerate(QMAX, 3):
        if q > b:
            refused(nat.E_ARG, s.hist, 1, c, q)


def test_a_double_has_no_row_0_and_a_constant_integer_no_widths(cx, typed):
    m, s = typed
    d, ci = 4, 13
    assert s.bits(1, d) == 30
    e = refused(nat.E_UNSUPPORTED, s.hist, 1, d, 0)
    assert "lossless double" in e.msg
    refused(nat.E_UNSUPPORTED, s.bytes, 1, d, 0)
    assert s.bits(1, ci) == 0 and "constant integer component" in s.reason(1, ci)
    refused(nat.E_UNSUPPORTED, s.hist, 1, ci, 3)
    # row 0 of everything else, with the double quantised so that the encoder takes the mesh
    q = m.clone()
    cx.requant(q, [(1, d, 10)])
    sq = cx.rate_sweep(q)
    assert sq.bits(1, d) == 0 and sq.planes(1, d, 0) == 2 and sq.planes(1, ci, 0) == 4
    check_row0(cx, q, sq)
    sq.close()


# ---- 4. block edges: coded-vertex counts just below, at and above a block, and several blocks
EDGES = {255: lambda: mg.torus(15, 17), 256: lambda: mg.torus(16, 16), 257: lambda: mg.hub_discs([128]), 384: lambda: mg.torus(24, 16), 1480: lambda: mg.torus(40, 37)}


@pytest.mark.parametrize("coded", sorted(EDGES))
def test_block_edges(cx, coded):
    m = hc.Mesh.from_ply(EDGES[coded]().to_ply())
    s = cx.rate_sweep(m)
    assert s.coded == coded == m.nv and (coded - 1) // BLOCK + 1 == {255: 1, 256: 1, 257: 2, 384: 2, 1480: 6}[coded]
    for q in (1, 8, 9, 17, 30):
        assert check_width(cx, m, s, q) == 3
    check_row0(cx, m, s)
    s.close()


# ---- 5. invariants
def test_determinism_residency_and_what_the_build_leaves(cx):
    ply = mg.with_nonmanifold(mg.torus(24, 16, normals=True)).to_ply()
    m = hc.Mesh.from_ply(ply)
    before = {p: cx.write_hry(hc.Mesh.from_ply(ply), profile=PROFILES[p]) for p in PROFILES}
    assert not cx.resident(m)
    s0 = cx.rate_sweep(m)                        # a fresh mesh: bounds as requant computes them (the mesh goes up for them), walk
    assert cx.resident(m) and m.list_min(1) is not None
    s1 = cx.rate_sweep(m)                        # the resident mesh, its twins repaired by the first walk
    assert cx.resident(m) and s1.stat()["uploaded_bytes"] == 0
    copy = m.clone()                             # bounds known, not resident: it goes up and becomes the resident mesh
    s2 = cx.rate_sweep(copy)
    assert cx.resident(copy) and not cx.resident(m) and s2.stat()["uploaded_bytes"] >= copy.list_count(1) * copy.list_stride(1) + 8 * copy.ne
    fresh = hc.Mesh.from_ply(ply)
    s3 = cx.rate_sweep(fresh)
    assert cx.resident(fresh) and not cx.resident(copy)
    t0 = tables(s0, m)
    assert len(t0) == 6 * 31
    for s in (s1, s2, s3):
        t = tables(s, m)
        assert len(t) == len(t0) and all(np.array_equal(a, b) for a, b in zip(t, t0))
        assert s.coded == s0.coded
    for p in PROFILES:
        assert cx.write_hry(m, profile=PROFILES[p]) == before[p]      # an encode afterwards gives the bytes it gave before
    st = s0.stat()
    assert st["device_ms"] > 0 and st["walk_ms"] > 0
    # bytes() is the entropy of hist(); choose() is rate_pick over the summed rows
    for c in range(6):
        for q in (0, 1, 8, 9, 17, 30):
            got, want = s0.bytes(1, c, q), rref.planes_bytes(s0.hist(1, c, q))
            assert abs(got - want) <= REL * want, (c, q, got, want)
            for h in s0.hist(1, c, q):
                assert abs(hc.rate_hist_bytes(h) - rref.hist_bytes(h)) <= REL * rref.hist_bytes(h)
    rows = {c: [s0.bytes(1, c, q) for q in range(1, 31)] for c in range(6)}
    every = [sum(rows[c][q] for c in range(6)) for q in range(30)]
    for budget in (0.0, every[0], every[0] - 1e-6, (every[9] + every[10]) / 2, every[29], 1e12):
        bits, est = s0.choose(1, -1, budget)
        assert bits == hc.rate_pick(every, budget) == rref.pick(every, budget) and est == (every[bits - 1] if bits else 0.0)
        bits, est = s0.choose(1, 2, budget / 6)
        assert bits == rref.pick(rows[2], budget / 6) and est == (rows[2][bits - 1] if bits else 0.0)
    assert s0.choose(1, -1, every[11])[0] >= 12 and every[0] < every[11] < every[23]
    for s in (s0, s1, s2, s3):
        s.close()
    s0.close()   # (closing twice is harmless)


def test_the_handle_outlives_the_context():
    c = hc.Codec(0)
    m = hc.Mesh.from_ply(mg.torus(12, 10).to_ply())
    s = c.rate_sweep(m)
    want = s.hist(1, 0, 12).copy()
    c.close()
    assert np.array_equal(s.hist(1, 0, 12), want) and s.coded == m.nv and s.bytes(1, 0, 12) > 0
    s.close()


# ---- 6. refusals; each leaves the context usable
def test_refusals(cx):
    m = hc.Mesh.from_ply(mg.torus(12, 10).to_ply())

    def usable():
        s = cx.rate_sweep(m)
        assert s.bits(1, 0) == 30 and int(s.hist(1, 0, 12).sum()) == 2 * m.nv
        return s

    s = usable()
    for l, c in ((5, 0), (-1, 0), (1, 3), (1, -1)):
        refused(nat.E_ARG, s.bits, l, c)
        refused(nat.E_ARG, s.hist, l, c, 4)
        refused(nat.E_ARG, s.bytes, l, c, 4)
    for q in (31, -3):
        refused(nat.E_ARG, s.hist, 1, 0, q)
        refused(nat.E_ARG, s.bytes, 1, 0, q)
        refused(nat.E_ARG, s.planes, 1, 0, q)
    L = nat.load()
    out = (C.c_uint32 * 256)()
    for q, plane in ((8, 1), (8, -1), (16, 2), (30, 4), (0, 4)):
        assert L.hry_rate_sweep_hist(s.h, 1, 0, q, plane, out) == nat.E_ARG
    assert L.hry_rate_sweep_hist(s.h, 1, 0, 30, 3, out) == 0 and sum(out) == m.nv
    for budget in (-1.0, float("nan")):
        refused(nat.E_ARG, s.choose, 1, 0, budget)
    refused(nat.E_ARG, s.choose, 7, 0, 1.0)
    refused(nat.E_ARG, s.choose, 1, 3, 1.0)
    # list 0, the faces: not swept, and the reason is stored
    fm = hc.Mesh.from_ply(mg.with_face_props(mg.torus(12, 10)).to_ply())
    fs = cx.rate_sweep(fm)
    assert fs.bits(0, 0) == 0 and "only list 1" in fs.reason(0, 0) and fs.bits(1, 0) == 30
    refused(nat.E_UNSUPPORTED, fs.hist, 0, 0, 0)
    refused(nat.E_UNSUPPORTED, fs.choose, 0, -1, 1e9)
    fs.close()
    s.close()
    # general bindings
    scene = hc.Mesh.from_obj(b"v 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nf 1 2 3\nf 2 4 3\n")
    e = refused(nat.E_UNSUPPORTED, cx.rate_sweep, scene)
    assert "general bindings" in e.msg
    usable().close()
    # a partial mesh, null arguments: *out stays NULL
    multi = hc.Mesh.from_ply(mg.multi_component(4, 6, 7).to_ply())
    shard = hc.ShardPlan(multi, 2).extract(multi, 0)
    part = cx.read_hry(cx.write_hry(shard, profile=hc.PROFILE_CHUNKED), partial=True)
    assert part.partial
    refused(nat.E_ARG, cx.rate_sweep, part)
    h = C.c_void_p(1)
    assert L.hry_rate_sweep_build(cx.h, None, C.byref(h)) == nat.E_ARG and not h.value
    h = C.c_void_p(1)
    assert L.hry_rate_sweep_build(cx.h, part.h, C.byref(h)) == nat.E_ARG and not h.value and b"partial" in L.hry_last_error()
    usable().close()


def test_a_mesh_without_faces_is_an_all_zero_table(cx):
    rng = np.random.default_rng(3)
    v = np.zeros(50, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")]))
    for n in v.dtype.names:
        v[n] = rng.normal(0, 1, 50)
    m = hc.Mesh.from_arrays(v, *NO_FACES)
    s = cx.rate_sweep(m)
    assert s.coded == 0 and [s.bits(1, c) for c in range(3)] == [30, 30, 30]
    for c in range(3):
        for q in (0, 1, 8, 16, 17, 30):
            assert not s.hist(1, c, q).any() and s.bytes(1, c, q) == 0.0
    assert s.choose(1, -1, 0.0) == (30, 0.0)
    s.close()


# ---- 7. the command line
def budget_lines(text):
    comps, out = [], None
    for ln in text.splitlines():
        w = ln.split()
        if ln.startswith("Budget: list"):
            assert w[1:8:2] == ["list", "attr", "bits", "estimated"] and w[9] == "bytes", ln
            comps.append((int(w[2]), int(w[4]), int(w[6]), float(w[8])))
        elif ln.startswith("Budget: output"):
            assert w[3] == "of" and w[5:7] == ["bytes", "after"] and w[8] == "encodes", ln
            out = (int(w[2]), int(w[4]), int(w[7]))
    return comps, out


@pytest.mark.parametrize("profile", sorted(PROFILES))
def test_cli_max_bytes(cx, tmp_path, profile):
    src = tmp_path / "in.ply"
    src.write_bytes(mg.torus(24, 16, sigma=1e-3).to_ply())

    def run(out, *opts):
        return subprocess.run([cli.HARRY, str(src), str(tmp_path / out), "--profile", profile, *opts], capture_output=True, text=True, timeout=300)

    r = run("q12.hry", "-l1", "-q12")
    assert r.returncode == 0, r.stderr
    s12 = len((tmp_path / "q12.hry").read_bytes())
    r = run("fit.hry", "-l1", "--max-bytes", str(s12))
    assert r.returncode == 0, r.stderr
    comps, out = budget_lines(r.stdout)
    print(r.stdout)
    assert [c[:3] for c in comps] == [(1, 0, 12), (1, 1, 12), (1, 2, 12)] and all(c[3] > 0 for c in comps)
    assert out[:2] == (s12, s12) and out[2] >= 2                                    # 12 bits fit, 13 were tried and do not
    assert (tmp_path / "fit.hry").read_bytes() == (tmp_path / "q12.hry").read_bytes()
    # a byte less: a narrower width, whose next one does not fit
    r = run("less.hry", "-l1", f"--max-bytes={s12 - 1}")
    assert r.returncode == 0, r.stderr
    comps, out = budget_lines(r.stdout)
    b = comps[0][2]
    less = len((tmp_path / "less.hry").read_bytes())
    assert 1 <= b < 12 and {c[2] for c in comps} == {b} and less <= s12 - 1 and out[:2] == (less, s12 - 1)
    r = run("next.hry", "-l1", f"-q{b + 1}")
    assert r.returncode == 0 and len((tmp_path / "next.hry").read_bytes()) > s12 - 1
    r = run("same.hry", "-l1", f"-q{b}")
    assert (tmp_path / "same.hry").read_bytes() == (tmp_path / "less.hry").read_bytes()
    # one component, next to a -q for the others
    r = run("one.hry", "-l1", "-a0", "-q10", "-a1", "-q10", "-a2", "--max-bytes", str(s12))
    assert r.returncode == 0, r.stderr
    comps, out = budget_lines(r.stdout)
    assert len(comps) == 1 and comps[0][:2] == (1, 2) and comps[0][2] > 12 and out[0] <= s12
    # below the size at 1 bit: the run fails and names that size
    r1 = run("q1.hry", "-l1", "-q1")
    s1 = len((tmp_path / "q1.hry").read_bytes())
    bad = run("bad.hry", "-l1", "--max-bytes", str(s1 - 1))
    assert bad.returncode != 0 and f"{s1} bytes at 1 bit" in bad.stderr and not (tmp_path / "bad.hry").exists()
    ok = run("least.hry", "-l1", "--max-bytes", str(s1))
    assert ok.returncode == 0 and budget_lines(ok.stdout)[0][0][2] == 1
    # argument errors
    for opts in (("-l1", "-q12", "--max-bytes", "1000"), ("-l1", "-a0", "--max-error", "0.1", "-a0", "--max-bytes", "1000"), ("--max-bytes", "1000"),
                 ("-l1", "--max-bytes", "-5"), ("-l1", "--max-bytes", "much"), ("-l1", "--max-bytes", "1000", "--gpus", "2"),
                 ("-l1", "--max-bytes", "1000", "--max-bytes", "2000")):
        bad = run("bad.hry", *opts)
        assert bad.returncode != 0 and "Error:" in bad.stderr and not (tmp_path / "bad.hry").exists(), opts
    ply = run("out.ply", "-l1", "--max-bytes", "1000")
    assert ply.returncode != 0 and ".hry" in ply.stderr
    help_ = subprocess.run([cli.HARRY, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--max-bytes" in help_
