"""The quantisation sweep on the GPU (include/harry_amd.h: hry_quant_sweep_build; kernels: harry_amd/csrc/device/sweep.hip) through
Codec.quant_sweep.  Every table entry is checked against the loop the sweep replaces: Codec.requant of a clone to that width --
k_requant, pinned to the reference's goldens -- and Codec.distortion of the source against it (pinned by tests/test_gpu_distortion.py).
Every field is equal, except sum_sq and sum_sq_dist: both sides add the same individually rounded terms in their own fixed order,
each within rows * 2^-53 of the exact sum, so they differ by at most rows * 2^-52 relative (tests/distortion_ref.py: sum_tolerance
-- derived, not measured).  The choice is followed through requant, encode, decode and distortion in both profiles."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import cli
from harry_amd import codec as hc
from harry_amd import meshgen as mg
from tests import distortion_ref as dref
from tests import quant_sweep_ref as qref
from tests.test_order_cpu import MESHES

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
NO = nat.NO_ELEMENT
PROFILES = {"compat": hc.PROFILE_COMPAT, "chunked": hc.PROFILE_CHUNKED}
EXACT = ("max_abs", "a_min", "a_max", "compared", "skipped", "nonfinite", "changed", "argmax")
BLOCK_ROWS = 1024   # a block's run of rows (kDistBlockRows)
NO_FACES = (np.zeros(0, np.uint8), np.zeros(0, np.uint32))


@pytest.fixture(scope="module")
def cx():
    c = hc.Codec(0)
    yield c
    c.close()


def close_sum(got: float, want: float, rows: int) -> bool:
    return abs(got - want) <= dref.sum_tolerance(max(rows, 1)) * want


def same_nan(a: float, b: float) -> bool:
    return a == b or (math.isnan(a) and math.isnan(b))


def check_width(cx, m: hc.Mesh, s: hc.QuantSweep, l: int, q: int, pos_list=None):
    """the table at q bits against the loop: every swept component of list l that has the width goes to q on a clone"""
    comps = [c for c in range(len(m.list_fmt(l))) if s.bits(l, c) >= q]
    if not comps:
        return 0
    clone = m.clone()
    cx.requant(clone, [(l, c, q) for c in comps])
    d = cx.distortion(m, clone)
    rows = m.list_count(l)
    for c in comps:
        got, want = s.component(l, c, q), d.component(l, c)
        print(f"list {l} comp {c} q{q}: got {got}\n                    want {want}")
        for k in EXACT:
            assert same_nan(got[k], want[k]), (l, c, q, k, got[k], want[k])
        assert close_sum(got["sum_sq"], want["sum_sq"], rows), (l, c, q, got["sum_sq"], want["sum_sq"])
        assert got["skipped"] == 0 and got["rms"] == (math.sqrt(got["sum_sq"] / got["compared"]) if got["compared"] else 0.0)
    if pos_list == l:
        got, want = s.position(q), d.position()
        print(f"position q{q}: got {got}\n            want {want}")
        for k in ("list", "max_dist", "compared", "argmax"):
            assert got[k] == want[k], (q, k, got[k], want[k])
        assert close_sum(got["sum_sq_dist"], want["sum_sq_dist"], rows)
    d.close()
    return len(comps)


def snapshot(s: hc.QuantSweep, m: hc.Mesh, l: int = 1) -> tuple:
    comps = tuple(tuple(sorted(r.items())) for c in range(len(m.list_fmt(l))) for r in s.table(l, c))
    return comps, tuple(tuple(sorted(s.position(q).items())) for q in range(1, 31))


def refused(code, fn, *args, **kw):
    with pytest.raises(hc.HryError) as e:
        fn(*args, **kw)
    assert e.value.code == code, e.value
    return e.value


# ---- 1. one float column at every width: a lone row, around a wavefront, around a block of lanes, around a block's run of rows,
# and several blocks for the fold
ROWS = [1, 63, 64, 65, 255, 256, 257, BLOCK_ROWS - 1, BLOCK_ROWS, BLOCK_ROWS + 1, 3 * BLOCK_ROWS + 1]


@pytest.mark.parametrize("rows", ROWS)
def test_one_float_column_at_every_width(cx, rows):
    rng = np.random.default_rng(rows)
    v = np.zeros(rows, np.dtype([("p", "<f4")]))
    v["p"] = rng.normal(0.0, 10.0, rows).astype(np.float32)
    m = hc.Mesh.from_arrays(v, *NO_FACES)
    s = cx.quant_sweep(m)
    assert s.bits(1, 0) == 30 and len(s.table(1, 0)) == 30
    for q in range(1, 31):
        assert check_width(cx, m, s, 1, q) == 1
        assert s.position(q)["list"] == -1           # one column: no positions
    t = s.table(1, 0)
    if rows > 1:
        assert t[0]["max_abs"] > t[11]["max_abs"] > t[23]["max_abs"] and t[11]["changed"] > 0
        assert (t[5]["a_min"], t[5]["a_max"], t[5]["compared"]) == (float(v["p"].min()), float(v["p"].max()), rows)
    assert s.stat()["device_ms"] > 0
    s.close()
    s.close()   # (closing twice is harmless)


# ---- 2. a component of each of the ten types at every width it has; 8 | 9 and 16 | 17: where the storage type changes
TYPES = [("f", "<f4"), ("d", "<f8"), ("ul", "<u8"), ("l", "<i8"), ("ui", "<u4"), ("i", "<i4"), ("us", "<u2"), ("s", "<i2"), ("uc", "u1"), ("c", "i1")]
RANGES = {"ul": (0, 10 ** 6), "l": (-10 ** 6, 10 ** 6), "ui": (0, 50000), "i": (-1000, 1000), "us": (0, 1000), "s": (-300, 300), "uc": (0, 200), "c": (-50, 50)}
WIDTH_IDS = {8: "q8_last_u8_top_of_char", 9: "q9_first_u16", 16: "q16_last_u16_top_of_short", 17: "q17_first_u32", 30: "q30_top"}


@pytest.fixture(scope="module")
def typed(cx):
    rows = 300
    rng = np.random.default_rng(11)
    v = np.zeros(rows, np.dtype(TYPES))
    v["f"] = rng.normal(0.0, 3.0, rows)
    v["d"] = rng.normal(0.0, 100.0, rows)
    for n, (lo, hi) in RANGES.items():
        v[n] = rng.integers(lo, hi + 1, rows)
    m = hc.Mesh.from_arrays(v, *NO_FACES)
    assert [t for t, _, _ in m.list_fmt(1)] == list(range(10))
    s = cx.quant_sweep(m)
    yield m, s
    s.close()


@pytest.mark.parametrize("q", range(1, 31), ids=[WIDTH_IDS.get(q, f"q{q}") for q in range(1, 31)])
def test_every_type_at_every_width(cx, typed, q):
    m, s = typed
    qmax = [s.bits(1, c) for c in range(10)]
    assert qmax == [30, 30, 30, 30, 30, 30, 16, 16, 8, 8]
    assert check_width(cx, m, s, 1, q) == sum(1 for b in qmax if b >= q)
    for c, b in enumerate(qmax):
        if q > b:
            refused(nat.E_ARG, s.component, 1, c, q)


# ---- 3. thirty-two components: positions that share an extent, a constant float (an extent of 0: whatever k_requant makes of
# it), NaN, a refused and a quantised component
def special_mesh(cx):
    rows = 321
    rng = np.random.default_rng(7)
    names = ["x", "y", "z", "cf", "nan", "ci", "done"] + [f"p{k}" for k in range(7, 32)]
    kinds = ["<f4"] * 5 + ["<i4", "<f4"] + [("<f4", "<i2", "u1", "<u4", "<f8")[k % 5] for k in range(7, 32)]
    v = np.zeros(rows, np.dtype(list(zip(names, kinds))))
    v["x"], v["y"], v["z"] = rng.uniform(-100, 100, rows), rng.uniform(0, 1, rows), rng.uniform(-5, 3, rows)   # one extent (x's) for the three
    v["z"][rows - 1] = np.float32(math.nan)   # a position without its z: the row is compared in x and y, not as a position
    v["cf"] = 2.5
    v["nan"] = rng.normal(0, 1, rows)
    v["nan"][[0, 64, rows - 1]] = np.float32(math.nan)
    v["ci"] = -17
    v["done"] = rng.normal(0, 4, rows)
    for n, k in zip(names[7:], kinds[7:]):
        v[n] = rng.normal(0, 50, rows) if "f" in k else rng.integers(0, 120, rows)
    m = hc.Mesh.from_arrays(v, *NO_FACES)
    assert len(m.list_fmt(1)) == 32
    cx.requant(m, [(1, names.index("done"), 10)])
    return m, names, v


def test_special_components_of_a_32_component_list(cx):
    m, names, v = special_mesh(cx)
    ci, done, cf, nan = (names.index(n) for n in ("ci", "done", "cf", "nan"))
    s = cx.quant_sweep(m)
    assert s.bits(1, ci) == 0 and "constant integer component" in s.reason(1, ci)
    assert s.bits(1, done) == 0 and s.reason(1, done) == "already quantised"
    assert s.bits(1, 0) == 30 and s.reason(1, 0) == ""
    e = refused(nat.E_UNSUPPORTED, s.choose, [(1, ci, "max_abs", 1.0)])
    assert "constant integer component" in e.msg and "list 1 attr 5" in e.msg
    assert "already quantised" in refused(nat.E_UNSUPPORTED, s.choose, [(1, done, "max_abs", 1.0)]).msg
    refused(nat.E_UNSUPPORTED, s.component, 1, ci, 4)
    for q in range(1, 31):
        assert check_width(cx, m, s, 1, q, pos_list=1) >= 3
    # the extent is shared: at the same width y, with a two-hundredth of x's range, is quantised as coarsely as x -- its own
    # extent would cost it 1 / 255 / 2 = 0.002
    x8, y8 = s.component(1, 0, 8), s.component(1, 1, 8)
    assert x8["max_abs"] > 0.3 and y8["max_abs"] > 0.1
    # the last row has no finite z: it is no position at any width, though its x and y are compared (check_width pins compared
    # and argmax of every width to the loop's)
    z8 = s.component(1, 2, 8)
    assert (x8["compared"], y8["compared"], z8["compared"], z8["nonfinite"]) == (321, 321, 320, 1)
    for q in (1, 2, 8, 17, 30):
        assert s.position(q)["compared"] == 320 and s.position(q)["argmax"] != 320
    assert s.position(8)["max_dist"] >= max(x8["max_abs"], y8["max_abs"]) or x8["argmax"] == 320 or y8["argmax"] == 320
    n12 = s.component(1, nan, 12)       # the NaN rows are never compared (what the bounds make of a NaN is k_requant's business)
    assert n12["nonfinite"] >= 3 and n12["compared"] + n12["nonfinite"] == 321 and n12["argmax"] not in (0, 64, 320)
    got = s.choose([(1, -1, "max_abs", 0.5)])        # comp -1: every swept component, the two others left out
    assert [c for _, c, _ in got] == [c for c in range(32) if c not in (ci, done)]
    assert s.component(1, cf, 30)["compared"] == 321
    s.close()


# ---- 4. determinism and residency
def list_bytes(m: hc.Mesh) -> int:
    return sum(m.list_count(l) * m.list_stride(l) for l in range(m.nlists) if len(m.list_fmt(l)))


def test_determinism_and_residency(cx):
    ply = mg.torus(40, 37, normals=True).to_ply()
    m = hc.Mesh.from_ply(ply)
    s0 = cx.quant_sweep(m)                       # bounds are computed where they are unset, as requant computes them
    assert m.list_min(1) is not None
    snap = snapshot(s0, m)
    copy = m.clone()                             # bounds known, not resident: its records go up, nothing else changes
    s1 = cx.quant_sweep(copy)
    assert s1.stat()["uploaded_bytes"] == list_bytes(copy) > 0 and not cx.resident(copy)
    cx.upload(m)
    assert cx.resident(m)
    s2 = cx.quant_sweep(copy)                    # beside a resident mesh: that one stays
    assert s2.stat()["uploaded_bytes"] == list_bytes(copy) and cx.resident(m)
    s3 = cx.quant_sweep(m)                       # the resident mesh: read in place
    assert s3.stat()["uploaded_bytes"] == 0 and cx.resident(m)
    for s in (s1, s2, s3):
        assert snapshot(s, m) == snap            # the same bits, sum_sq included
    assert snap[0][0] != snap[0][1] and s0.component(1, 0, 12)["changed"] > 0
    data = cx.write_hry(m)                       # the resident mesh is still what an encode finds
    assert data == cx.write_hry(copy.clone())
    # a decode, the sweep of another mesh, a render: the decode's buffers are still there
    dec = cx.read_hry(data)
    s4 = cx.quant_sweep(copy)
    assert snapshot(s4, m) == snap
    got = cx.render(dec)
    assert cx.render_stat()["uploaded_bytes"] == 0 and got["list1"].shape == (dec.nv, 6)
    for s in (s0, s1, s2, s3, s4):
        s.close()


# ---- 5. the choice, end to end
def roundtrip(cx, m, choice, profile):
    enc = m.clone()
    cx.requant(enc, choice)
    data, order = cx.write_hry(enc, profile=PROFILES[profile], return_order=True)
    dec = cx.read_hry(data)
    d = cx.distortion(m, dec, order)
    order.close()
    return d


def group_extent(m, comps) -> float:
    """the extent requant shares over an interpretation group: the largest max - min, evaluated in float"""
    return float(max(np.float32(m.component(1, c).max()) - np.float32(m.component(1, c).min()) for c in comps))


@pytest.mark.parametrize("profile", sorted(PROFILES))
def test_choice_end_to_end(cx, profile):
    m = hc.Mesh.from_ply(mg.torus(24, 16, normals=True).to_ply())
    s = cx.quant_sweep(m)
    # MAX_ABS on one component, the tolerance between the entries of 10 and 11 bits
    t = s.table(1, 0)
    tol = (t[9]["max_abs"] + t[10]["max_abs"]) / 2
    assert t[10]["max_abs"] < tol < t[9]["max_abs"]
    choice = s.choose([(1, 0, "max_abs", tol)])
    assert len(choice) == 1 and choice[0][:2] == (1, 0)
    b = choice[0][2]
    assert b == qref.pick(t, qref.MAX_ABS, 0.0, tol) and 1 <= b <= 11
    assert t[b - 1]["max_abs"] <= tol and (b == 1 or t[b - 2]["max_abs"] > tol)
    d = roundtrip(cx, m, choice, profile)
    got = d.component(1, 0)
    assert (got["max_abs"], got["changed"]) == (t[b - 1]["max_abs"], t[b - 1]["changed"]) and got["max_abs"] <= tol
    assert d.component(1, 1)["changed"] == 0      # (the others stay lossless)
    d.close()
    # MAX_REL on every component of the list: a thousandth of each group's extent
    rel = 1e-3
    choice = s.choose([(1, -1, nat.TOL_MAX_REL, rel)])
    assert [(l, c) for l, c, _ in choice] == [(1, c) for c in range(6)]
    d = roundtrip(cx, m, choice, profile)
    for (_, c, b), group in zip(choice, [(0, 1, 2)] * 3 + [(3, 4, 5)] * 3):
        t, bound = s.table(1, c), rel * group_extent(m, group)
        assert b == qref.pick(t, qref.MAX_REL, group_extent(m, group), rel) and b >= 1
        assert t[b - 1]["max_abs"] <= bound and (b == 1 or t[b - 2]["max_abs"] > bound)
        got = d.component(1, c)
        assert (got["max_abs"], got["changed"]) == (t[b - 1]["max_abs"], t[b - 1]["changed"])
    d.close()
    # POS_DIST: one width for the three position components
    p = [s.position(q) for q in range(1, 31)]
    tol = (p[8]["max_dist"] + p[9]["max_dist"]) / 2
    choice = s.choose([(1, -1, "pos_dist", tol)])
    b = choice[0][2]
    assert choice == [(1, 0, b), (1, 1, b), (1, 2, b)] and 1 <= b <= 10
    assert p[b - 1]["max_dist"] <= tol and (b == 1 or p[b - 2]["max_dist"] > tol)
    d = roundtrip(cx, m, choice, profile)
    got = d.position()
    assert (got["max_dist"], got["compared"], got["list"]) == (p[b - 1]["max_dist"], p[b - 1]["compared"], 1) and got["max_dist"] <= tol
    d.close()
    # a tolerance on a component next to the positions' one: the smallest width that meets both
    both = s.choose([(1, -1, "pos_dist", tol), (1, 0, "max_abs", 0.0)])
    assert both[0] == (1, 0, 0) and both[1:] == [(1, 1, b), (1, 2, b)]     # nothing meets 0: x stays lossless
    s.close()


# ---- 6. refusals; each leaves the context usable
def test_refusals(cx):
    m = hc.Mesh.from_ply(MESHES["torus"]().to_ply())

    def usable():
        s = cx.quant_sweep(m)
        assert s.bits(1, 0) == 30 and s.component(1, 0, 12)["compared"] == m.nv
        return s

    s = usable()
    for bad in ([(1, 0, "max_abs", -1.0)], [(1, 0, "rms", math.nan)], [(1, 0, 7, 1.0)], [(1, 0, -1, 1.0)], [(9, 0, "max_abs", 1.0)], [(-1, 0, "max_abs", 1.0)],
                [(1, 3, "max_abs", 1.0)], [(1, -2, "max_abs", 1.0)], [(1, 0, "pos_dist", 1.0)], [(0, -1, "pos_dist", 1.0)]):
        refused(nat.E_ARG, s.choose, bad)
    refused(nat.E_ARG, s.choose, [(1, 0, "no such metric", 1.0)])
    for l, c in ((5, 0), (-1, 0), (1, 3), (1, -1)):
        refused(nat.E_ARG, s.bits, l, c)
        refused(nat.E_ARG, s.component, l, c, 4)
    for q in (0, 31, -3):
        refused(nat.E_ARG, s.component, 1, 0, q)
        refused(nat.E_ARG, s.position, q)
    assert s.choose([]) == [] and s.choose([(1, 0, "max_abs", 0.0)]) == [(1, 0, 0)]      # no width meets it: lossless
    L = nat.load()
    n, out = C.c_size_t(), (nat.Quant * 2)()
    tol = (nat.Tolerance * 1)(nat.Tolerance(1, -1, nat.TOL_MAX_ABS, 0, 1.0))
    assert L.hry_quant_choose(s.h, tol, 1, out, 2, C.byref(n)) == nat.E_ARG and n.value == 3   # room for two of three
    s.close()
    # a double cannot stay lossless
    dm = hc.Mesh.from_ply(mg.doubles(mg.torus(12, 10)).to_ply())
    sd = cx.quant_sweep(dm)
    assert sd.bits(1, 0) == 30
    e = refused(nat.E_UNSUPPORTED, sd.choose, [(1, 1, "max_abs", 0.0)])
    assert "list 1 attr 1" in e.msg
    assert sd.choose([(1, 1, "max_abs", 1.0)])[0][2] >= 1
    sd.close()
    # (Of section 2's refusals "a list without its records" has no case: no constructor, reader, clone or decode of the public
    # interface returns a whole mesh whose list holds fewer bytes than count * stride -- only a partial mesh does, and that is
    # refused before its lists are looked at.  tests/test_gpu_distortion.py is silent on it for the same reason.)
    # a partial mesh, null arguments: *out stays NULL
    multi = hc.Mesh.from_ply(MESHES["multi"]().to_ply())
    shard = hc.ShardPlan(multi, 2).extract(multi, 0)
    part = cx.read_hry(cx.write_hry(shard, profile=hc.PROFILE_CHUNKED), partial=True)
    assert part.partial
    refused(nat.E_ARG, cx.quant_sweep, part)
    usable().close()
    h = C.c_void_p(1)
    assert L.hry_quant_sweep_build(cx.h, None, C.byref(h)) == nat.E_ARG and not h.value
    h = C.c_void_p(1)
    assert L.hry_quant_sweep_build(cx.h, part.h, C.byref(h)) == nat.E_ARG and not h.value and b"partial" in L.hry_last_error()
    usable().close()
    # a mesh that is quantised already: nothing is swept, and naming a component says why
    q = m.clone()
    cx.requant(q, [(1, -1, 12)])
    sq = cx.quant_sweep(q)
    assert [sq.bits(1, c) for c in range(3)] == [0, 0, 0] and sq.position(5)["list"] == -1 and sq.choose([(1, -1, "max_abs", 1.0)]) == []
    refused(nat.E_UNSUPPORTED, sq.choose, [(1, -1, "pos_dist", 1.0)])
    sq.close()
    usable().close()


# ---- 7. the restatement over Codec.requant: the table is what the header says it is
def test_table_equals_the_restatement(cx):
    m = hc.Mesh.from_ply(mg.torus(12, 10).to_ply())
    s = cx.quant_sweep(m)
    x = dref.values(m, 1)

    def values_at(comps, bits):
        return qref.codec_values(cx, m, 1, comps, bits)

    want = qref.table(values_at, x, 2, 30)
    for q, w in enumerate(want, 1):
        got = s.component(1, 2, q)
        for k in EXACT:
            assert got[k] == w[k], (q, k, got[k], w[k])
        assert close_sum(got["sum_sq"], w["sum_sq"], len(x))
    for q, w in enumerate(qref.position_table(values_at, x, 0, 30), 1):
        got = s.position(q)
        assert (got["max_dist"], got["compared"], got["argmax"]) == (w["max_dist"], w["compared"], w["argmax"]) and close_sum(got["sum_sq_dist"], w["sum_sq_dist"], len(x))
    s.close()


# ---- 8. the command line
def chosen_lines(text):
    out = []
    for ln in text.splitlines():
        if ln.startswith("Chosen:"):
            w = ln.split()
            assert w[1:8:2] == ["list", "attr", "bits", "max"], ln
            out.append((int(w[2]), int(w[4]), int(w[6]), float(w[8])))
    return out


def test_cli_max_error(cx, tmp_path):
    gen = mg.torus(24, 16, normals=True)
    src = tmp_path / "in.ply"
    src.write_bytes(gen.to_ply())
    m = hc.Mesh.from_ply(src.read_bytes())
    s = cx.quant_sweep(m)
    tol = (s.component(1, 0, 10)["max_abs"] + s.component(1, 0, 11)["max_abs"]) / 2

    def run(out, *opts):
        return subprocess.run([cli.HARRY, str(src), str(tmp_path / out), *opts], capture_output=True, text=True, timeout=300)

    r = run("tol.hry", "-l1", "--max-error", repr(tol), "--report")
    assert r.returncode == 0, r.stderr
    chosen = chosen_lines(r.stdout)
    want = s.choose([(1, -1, "max_abs", tol)])
    assert [c[:3] for c in chosen] == want and len(chosen) == 6
    for l, c, b, mx in chosen:
        ref = s.component(l, c, b)["max_abs"]
        assert abs(mx - ref) <= 1e-8 * ref and mx <= tol * (1 + 1e-8)
    report = {int(w[4]): (int(w[6]), float(w[8])) for w in (ln.split() for ln in r.stdout.splitlines() if ln.startswith("Distortion:"))}
    assert {c: (b, mx) for _, c, b, mx in chosen} == report            # --report's bits and max are the chosen ones
    explicit = [o for _, c, b in want for o in (f"-a{c}", f"-q{b}")]
    r1 = run("explicit.hry", "-l1", *explicit)
    assert r1.returncode == 0 and "Chosen:" not in r1.stdout
    assert (tmp_path / "tol.hry").read_bytes() == (tmp_path / "explicit.hry").read_bytes()
    # relative, bound to -a, next to a -q for another component
    r2 = run("mixed.hry", "-l1", "-a0", "--max-error-rel=0.001", "-a3", "-q10")
    assert r2.returncode == 0, r2.stderr
    (l, c, b, _), = chosen_lines(r2.stdout)
    assert (l, c, b) == s.choose([(1, 0, "max_rel", 0.001)])[0]
    r3 = run("mixed_explicit.hry", "-l1", "-a0", f"-q{b}", "-a3", "-q10")
    assert r3.returncode == 0 and (tmp_path / "mixed.hry").read_bytes() == (tmp_path / "mixed_explicit.hry").read_bytes()
    # without the options: as before
    r4 = run("plain.hry")
    assert r4.returncode == 0 and "Chosen:" not in r4.stdout and "Quantization" not in r4.stdout
    assert (tmp_path / "plain.hry").read_bytes() == cx.write_hry(hc.Mesh.from_ply(src.read_bytes()))
    # the same component by -q and by a tolerance, a tolerance without a list, a negative one: argument errors
    for opts in (("-l1", "-a0", "-q12", "-a0", "--max-error", "0.1"), ("-l1", "-q12", "-a2", "--max-error-rel", "0.1"), ("--max-error", "0.1"),
                 ("-l1", "--max-error", "-1"), ("-l1", "--max-error", "much")):
        bad = run("bad.hry", *opts)
        assert bad.returncode != 0 and "Error:" in bad.stderr and not (tmp_path / "bad.hry").exists(), opts
    assert "Invalid option" in run("bad.hry", "-l1", "-a0", "-q12", "-a0", "--max-error", "0.1").stderr
    help_ = subprocess.run([cli.HARRY, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--max-error " in help_ and "--max-error-rel" in help_
    s.close()


def test_cli_max_error_with_clear_on_a_quantised_input(cx, tmp_path):
    """-c with a tolerance on a .hry whose components are quantised already: the mesh is cleared, swept, and the widths are applied to
    the cleared values -- what is applied is what was swept, so --report's max is M and M is within the tolerance (a direct
    14 -> q rescale of the stored integers truncates and would cost up to a whole step)"""
    first = hc.Mesh.from_ply(mg.torus(24, 16, normals=True).to_ply())
    cx.requant(first, [(1, -1, 14)])
    src = tmp_path / "q14.hry"
    src.write_bytes(cx.write_hry(first))

    def run(out, *opts):
        return subprocess.run([cli.HARRY, str(src), str(tmp_path / out), *opts], capture_output=True, text=True, timeout=300)

    def cleared():
        m = cx.read_hry(src.read_bytes())
        assert [q for _, q, _ in m.list_fmt(1)] == [14] * 6
        cx.requant(m, [], clear=True)
        return m

    m = cleared()
    s = cx.quant_sweep(m)
    assert s.bits(1, 0) == 30
    tol = (s.component(1, 0, 8)["max_abs"] + s.component(1, 0, 9)["max_abs"]) / 2
    r = run("tol.hry", "-c", "-l1", "--max-error", repr(tol), "--report")
    assert r.returncode == 0, r.stderr
    chosen = chosen_lines(r.stdout)
    want = s.choose([(1, -1, "max_abs", tol)])
    assert [c[:3] for c in chosen] == want and len(chosen) == 6 and all(1 <= b < 14 for _, _, b in want)
    for l, c, b, mx in chosen:
        ref = s.component(l, c, b)["max_abs"]
        assert abs(mx - ref) <= 1e-8 * ref and 0 < mx <= tol * (1 + 1e-8), (c, b, mx, ref, tol)
    report = {int(w[4]): (int(w[6]), float(w[8])) for w in (ln.split() for ln in r.stdout.splitlines() if ln.startswith("Distortion:"))}
    assert {c: (b, mx) for _, c, b, mx in chosen} == report            # --report: the quantised input against the result
    applied = cleared()
    cx.requant(applied, want)
    assert (tmp_path / "tol.hry").read_bytes() == cx.write_hry(applied)
    # an explicit -q beside the tolerance is applied to the cleared values too
    r2 = run("mixed.hry", "-c", "-l1", "-a0", "--max-error", repr(tol), "-a3", "-q8")
    assert r2.returncode == 0, r2.stderr
    (l, c, b, _), = chosen_lines(r2.stdout)
    assert (l, c, b) == want[0]
    applied = cleared()
    cx.requant(applied, [(1, 0, b), (1, 3, 8)])
    assert (tmp_path / "mixed.hry").read_bytes() == cx.write_hry(applied)
    # without -c the components are quantised already: no tolerance can be put on them
    r3 = run("kept.hry", "-l1", "--max-error", repr(tol))
    assert r3.returncode != 0 and "already quantised" in r3.stderr and not (tmp_path / "kept.hry").exists()
    s.close()
