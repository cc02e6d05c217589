"""The faces' normal deviation on the GPU (include/harry_amd.h: hry_normal_error; kernels: harry_amd/csrc/device/normal_sweep.hip)
through Codec.quant_sweep(normals=True) and Codec.distortion_ex(normals=True), against the numpy restatement of
tests/normal_error_ref.py over positions that code not under test produced (Codec.requant, pinned to the reference's goldens).
max_chord, argmax and the five counters are equal: every operation is a correctly rounded double operation on both sides, in one
order.  sum_sq_chord: both sides add the same individually rounded terms in their own fixed order, so they differ by at most
faces * 2^-52 relative (tests/distortion_ref.py: sum_tolerance -- derived, not measured)."""
import math

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import codec as hc
from tests import distortion_ref as dref
from tests import normal_error_ref as nref
from tests import quant_sweep_ref as qref
from tests.test_gpu_quant_sweep import snapshot as table_snapshot
from tests.test_normal_sweep_cpu import ANGLES_DEG, oracle_table, tri_widths

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
PROFILES = {"compat": hc.PROFILE_COMPAT, "chunked": hc.PROFILE_CHUNKED}
QMAX = {"tri": 30, "mixed": 30, "ushort": 16, "int": 30, "double": 30, "bad": 30, "bad_inf": 30}
LOOP_BITS = (1, 2, 7, 8, 9, 16, 17, 24, 30)


@pytest.fixture(scope="module")
def cx():
    c = hc.Codec(0)
    yield c
    c.close()


def codec_mesh(name: str) -> hc.Mesh:
    g = nref.mesh(name)
    return hc.Mesh.from_arrays(g.verts, g.degrees, g.indices)


def close_sum(got: float, want: float, faces: int) -> bool:
    return abs(got - want) <= dref.sum_tolerance(max(faces, 1)) * want


def same_record(got: dict, want: dict, faces: int, what):
    print(f"{what}: got  { {k: got[k] for k in nref.FIELDS} }\n{' ' * len(str(what))}  want { {k: want[k] for k in nref.FIELDS} }")
    for k in nref.EXACT:
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert close_sum(got["sum_sq_chord"], want["sum_sq_chord"], faces), (what, got["sum_sq_chord"], want["sum_sq_chord"])
    assert sum(got[k] for k in ("compared", "skipped", "nonfinite", "degenerate", "collapsed")) == faces


def refused(code, fn, *args, **kw):
    with pytest.raises(hc.HryError) as e:
        fn(*args, **kw)
    assert e.value.code == code, e.value
    return e.value


# ---- 1. the sweep against the restatement: every mesh, every width
@pytest.mark.parametrize("name", sorted(QMAX))
def test_sweep_equals_the_reference(cx, name):
    g, m = nref.mesh(name), codec_mesh(name)
    s = cx.quant_sweep(m, normals=True)
    qmax = QMAX[name]
    assert [s.bits(1, c) for c in range(3)] == [qmax] * 3 and s.position(qmax)["list"] == 1
    x = dref.values(m, 1)
    want = nref.table(lambda comps, bits: qref.codec_values(cx, m, 1, comps, bits), x, 0, qmax, g.degrees, g.indices)
    for q in range(1, qmax + 1):
        got = s.normals(q)
        assert got["list"] == 1
        same_record(got, want[q - 1], g.nf, (name, q))
        if got["compared"]:
            assert got["max_angle_deg"] == math.degrees(hc.chord_angle(got["max_chord"]))
            assert got["rms_angle_deg"] == math.degrees(hc.chord_angle(math.sqrt(got["sum_sq_chord"] / got["compared"])))
    refused(nat.E_ARG, s.normals, 0)
    refused(nat.E_ARG, s.normals, qmax + 1)
    s.close()


# ---- 2. the sweep against the loop it replaces
@pytest.mark.parametrize("name", ["tri", "mixed", "ushort"])
def test_sweep_equals_the_loop(cx, name):
    g, m = nref.mesh(name), codec_mesh(name)
    s = cx.quant_sweep(m, normals=True)
    for q in sorted({min(b, QMAX[name]) for b in LOOP_BITS}):
        clone = m.clone()
        cx.requant(clone, [(1, c, q) for c in range(3)])
        d = cx.distortion_ex(m, clone, normals=True)
        got, want = s.normals(q), d.normals()
        assert want["list"] == 1 and d.rows("normal_error") == 0   # (no per-face buffer without rows=True)
        same_record(got, want, g.nf, (name, q))
        d.close()
    s.close()


# ---- 3. the distortion build through the numbering map of an encode
def cleared_values(cx, m: hc.Mesh) -> np.ndarray:
    c = m.clone()
    cx.requant(c, [], clear=True)
    return dref.values(c, 1)


@pytest.mark.parametrize("profile", sorted(PROFILES))
def test_distortion_through_an_order(cx, profile):
    g, src = nref.mesh("mixed"), codec_mesh("mixed")
    enc = src.clone()
    cx.requant(enc, [(1, c, 12) for c in range(3)])
    data, order = cx.write_hry(enc, profile=PROFILES[profile], return_order=True)
    dec = cx.read_hry(data)
    d = cx.distortion_ex(src, dec, order, rows=True, normals=True)
    vmap = order.numpy("vertex")
    want = nref.compare(dref.values(src, 1)[:, :3], cleared_values(cx, dec)[:, :3], g.degrees, g.indices, vmap)
    got = d.normals()
    assert got["list"] == 1
    same_record(got, want, g.nf, ("mixed", profile))
    assert got["compared"] == g.nf and 0.0 < got["max_chord"] < 0.1   # (12 bits: every face keeps a normal, tilted a little)
    faces = d.numpy("normal_error")
    assert faces.dtype == np.float32 and faces.shape == (g.nf,) and np.array_equal(faces, want["faces"])
    assert float(faces[got["argmax"]]) == float(np.float32(got["max_chord"])) and torch.equal(d.tensor("normal_error").cpu(), torch.from_numpy(faces))
    # the same build without the flag: what it returned before
    plain = cx.distortion(src, dec, order, rows=True)
    for c in range(3):
        assert plain.component(1, c) == d.component(1, c)
    assert plain.position() == d.position() and np.array_equal(plain.numpy("error1"), d.numpy("error1"))
    assert plain.rows("normal_error") == 0 and plain.normals()["list"] == -1 and "HRY_DISTORTION_NORMALS" in plain.normals()["reason"]
    for h in (d, plain, order):
        h.close()


def test_distortion_classes_and_refusals(cx):
    """nonfinite and degenerate faces after the fact; a mesh without faces gives list -1 and fails nothing"""
    g, src = nref.mesh("bad_inf"), codec_mesh("bad_inf")
    other = codec_mesh("tri")
    d = cx.distortion_ex(src, other, rows=True, normals=True)
    x, y = dref.values(src, 1)[:, :3], dref.values(other, 1)[:, :3]
    want = nref.compare(x, y, g.degrees, g.indices)
    got = d.normals()
    same_record(got, want, g.nf, "bad_inf against tri")
    assert got["nonfinite"] == 12 and got["degenerate"] >= 2 and np.array_equal(d.numpy("normal_error"), want["faces"])
    d.close()
    cloud = hc.Mesh.from_arrays(g.verts, np.zeros(0, np.uint8), np.zeros(0, np.uint32))
    d = cx.distortion_ex(cloud, cloud.clone(), rows=True, normals=True)
    assert d.normals()["list"] == -1 and "no faces" in d.normals()["reason"] and d.rows("normal_error") == 0
    assert d.position()["compared"] == g.nv - 2 and d.rows("error1") == g.nv   # (the rest of the build is what it was)
    d.close()
    h = hc.C.c_void_p()
    assert nat.load().hry_distortion_build(cx.h, src.h, other.h, None, 8, hc.C.byref(h)) == nat.E_ARG and not h.value   # an unknown bit


# ---- 4. residency and determinism
def normals_snapshot(s: hc.QuantSweep, qmax: int = 30) -> tuple:
    return tuple(tuple(sorted(s.normals(q).items())) for q in range(1, qmax + 1))


def list_bytes(m: hc.Mesh) -> int:
    return sum(m.list_count(l) * m.list_stride(l) for l in range(m.nlists) if len(m.list_fmt(l)))


def test_determinism_and_residency(cx):
    m = codec_mesh("tri")
    s0 = cx.quant_sweep(m, normals=True)          # bounds are computed where they are unset: m goes up for them
    snap, tab = normals_snapshot(s0), table_snapshot(s0, m)
    copy = m.clone()                              # bounds known, not resident: records and corners go up (triangles: no face offsets)
    s1 = cx.quant_sweep(copy, normals=True)
    assert s1.stat()["uploaded_bytes"] == list_bytes(copy) + 4 * copy.ne and not cx.resident(copy)
    mixed = codec_mesh("mixed")
    cx.quant_sweep(mixed).close()                 # (its bounds)
    mixed = mixed.clone()
    sm = cx.quant_sweep(mixed, normals=True)      # mixed degrees: the face offsets go up too
    assert sm.stat()["uploaded_bytes"] == list_bytes(mixed) + 4 * mixed.ne + 4 * (mixed.nf + 1)
    cx.upload(m)
    assert cx.resident(m)
    s2 = cx.quant_sweep(copy, normals=True)       # beside a resident mesh: that one stays
    assert cx.resident(m) and s2.stat()["uploaded_bytes"] == s1.stat()["uploaded_bytes"]
    s3 = cx.quant_sweep(m, normals=True)          # the resident mesh: records, corners read in place
    assert s3.stat()["uploaded_bytes"] == 0 and cx.resident(m)
    s4 = cx.quant_sweep(m, normals=True)          # ... twice: the same bits
    for s in (s1, s2, s3, s4):
        assert normals_snapshot(s) == snap and table_snapshot(s, m) == tab
    # the distortion build: a's corners in place when a is resident, uploaded otherwise; the same record
    clone = m.clone()
    cx.requant(clone, [(1, c, 9) for c in range(3)])
    cx.upload(m)
    d_res = cx.distortion_ex(m, clone, normals=True)
    d_up = cx.distortion_ex(m.clone(), clone, normals=True)
    assert d_up.stat()["uploaded_bytes"] - d_res.stat()["uploaded_bytes"] == list_bytes(m) + 4 * m.ne
    assert d_res.normals() == d_up.normals()      # bit for bit, sum_sq_chord included
    same_record(s3.normals(9), d_res.normals(), m.nf, "resident, 9 bits")
    # a decode, the sweep of another mesh with its bounds known, a render: the decode's buffers are still there
    data = cx.write_hry(m)
    dec = cx.read_hry(data)
    s5 = cx.quant_sweep(copy, normals=True)
    assert normals_snapshot(s5) == snap
    got = cx.render(dec)
    assert cx.render_stat()["uploaded_bytes"] == 0 and got["list1"].shape == (dec.nv, 3)
    for h in (s0, s1, s2, s3, s4, s5, sm, d_res, d_up):
        h.close()


# ---- 5. flags 0 is what it was
def test_without_the_flag_the_sweep_is_untouched(cx):
    m = codec_mesh("tri")
    plain, with_normals = cx.quant_sweep(m), cx.quant_sweep(m, normals=True)
    assert table_snapshot(plain, m) == table_snapshot(with_normals, m)
    e = refused(nat.E_UNSUPPORTED, plain.normals, 8)
    assert "not swept" in str(e)
    e = refused(nat.E_UNSUPPORTED, plain.choose, [(1, -1, "normal_chord", 0.1)])
    assert "not swept" in str(e)
    h = hc.C.c_void_p()
    assert nat.load().hry_quant_sweep_build_ex(cx.h, m.h, 2, hc.C.byref(h)) == nat.E_ARG and not h.value   # an unknown bit
    # positions that are not all swept: list -1 with the reason, and the metric is refused with it
    q = m.clone()
    cx.requant(q, [(1, 0, 10)])
    part = cx.quant_sweep(q, normals=True)
    rec = part.normals(8)
    assert rec["list"] == -1 and rec["compared"] == 0 and "not all swept" in rec["reason"]
    assert "not all swept" in str(refused(nat.E_UNSUPPORTED, part.choose, [(1, -1, "normal_chord", 0.1)]))
    for s in (plain, with_normals, part):
        s.close()


# ---- 6. widths from an angle
def test_choose_from_an_angle(cx):
    want = tri_widths(oracle_table("tri", 30))   # what the CPU test derived from the oracle
    m = codec_mesh("tri")
    s = cx.quant_sweep(m, normals=True)
    for deg, bits in zip(ANGLES_DEG, want):
        chord = hc.angle_chord(math.radians(deg))
        got = s.choose([(1, -1, "normal_chord", chord)])
        assert got == [(1, 0, bits), (1, 1, bits), (1, 2, bits)], (deg, got, bits)
        rec = s.normals(bits)
        assert rec["max_chord"] <= chord and rec["collapsed"] == 0 and rec["max_angle_deg"] <= deg * (1 + 1e-12)
    # collapsed faces bar a width whatever the chord: 2 is the largest chord there is
    first_whole = next(q for q in range(1, 31) if s.normals(q)["collapsed"] == 0)
    assert first_whole > 1 and s.choose([(1, -1, "normal_chord", 2.0)])[0][2] == first_whole
    # with another tolerance on the same components: every tolerance met at that width
    tight = s.position(20)["max_dist"]
    assert s.choose([(1, -1, "normal_chord", hc.angle_chord(math.radians(10.0))), (1, -1, "pos_dist", tight)])[0][2] == max(want[0], s.choose([(1, -1, "pos_dist", tight)])[0][2])
    assert s.choose([(1, -1, "normal_chord", 0.0)]) == [(1, 0, 0), (1, 1, 0), (1, 2, 0)]   # no width meets it: lossless
    refused(nat.E_ARG, s.choose, [(1, 0, "normal_chord", 0.1)])     # comp must be -1
    refused(nat.E_ARG, s.choose, [(0, -1, "normal_chord", 0.1)])    # not the position list
    refused(nat.E_ARG, s.choose, [(1, -1, "normal_chord", -0.1)])
    assert nat.load().hry_quant_pick((nat.CompError * 1)(), 1, nat.TOL_NORMAL_CHORD, 1.0, 0.1) == nat.E_ARG   # not a component's metric
    s.close()
    d = codec_mesh("double")
    sd = cx.quant_sweep(d, normals=True)
    assert "cannot stay lossless" in str(refused(nat.E_UNSUPPORTED, sd.choose, [(1, -1, "normal_chord", 0.0)]))
    sd.close()


# ---- 7. general bindings: the row of a vertex through k_rows_of
def obj_parts(m: hc.Mesh, pl: int):
    return np.diff(m.face_offsets().astype(np.int64)).astype(np.uint8), m.org(), nref.vertex_rows(m, pl)


def test_sweep_with_general_bindings(cx):
    m = hc.Mesh.from_obj(nref.obj_scene(), "")
    s = cx.quant_sweep(m, normals=True)
    pl = s.position(1)["list"]
    assert pl >= 0 and m.list_target(pl) == 1 and [s.bits(pl, c) for c in range(3)] == [30] * 3
    deg, idx, rows = obj_parts(m, pl)
    assert (rows != nref.NO).all() and len(set(deg.tolist())) > 1
    x = dref.values(m, pl)
    want = nref.table(lambda comps, bits: qref.codec_values(cx, m, pl, comps, bits), x, 0, 30, deg, idx, rows=rows)
    for q in range(1, 31):
        got = s.normals(q)
        assert got["list"] == pl
        same_record(got, want[q - 1], m.nf, ("obj", q))
    assert want[0]["collapsed"] > 0 and want[15]["compared"] == m.nf
    s.close()


@pytest.mark.parametrize("profile", sorted(PROFILES))
def test_distortion_through_an_order_with_general_bindings(cx, profile):
    src = hc.Mesh.from_obj(nref.obj_scene(), "")
    probe = cx.quant_sweep(src)
    pl = probe.position(1)["list"]
    probe.close()
    deg, idx, rows = obj_parts(src, pl)
    enc = src.clone()
    cx.requant(enc, [(pl, c, 12) for c in range(3)])
    data, order = cx.write_hry(enc, profile=PROFILES[profile], return_order=True)
    dec = cx.read_hry(data)
    d = cx.distortion_ex(src, dec, order, rows=True, normals=True)
    assert nat.load().hry_distortion_position_component(d.h) == 0
    c = dec.clone()
    cx.requant(c, [], clear=True)
    want = nref.compare(dref.values(src, pl)[:, :3], dref.values(c, pl)[:, :3], deg, idx, order.numpy(f"list{pl}"), rows)
    got = d.normals()
    assert got["list"] == pl
    same_record(got, want, src.nf, ("obj", profile))
    assert got["compared"] == src.nf and got["max_chord"] > 0.0
    assert np.array_equal(d.numpy("normal_error"), want["faces"])
    for h in (d, order):
        h.close()


def test_a_vertex_region_that_does_not_bind_the_position_list(cx):
    """every third vertex in a region with its own list: no normals, with the reason, and nothing else fails"""
    m = hc.Mesh.from_obj(nref.obj_scene("some"), "")
    assert m.nregions(1) == 2
    s = cx.quant_sweep(m, normals=True)
    pl = s.position(1)["list"]
    rec = s.normals(8)
    assert pl >= 0 and rec["list"] == -1 and rec["reason"] == "normals: a vertex region that does not bind the position list"
    assert "does not bind the position list" in str(refused(nat.E_UNSUPPORTED, s.choose, [(pl, -1, "normal_chord", 0.1)]))
    plain = cx.quant_sweep(m)
    assert table_snapshot(plain, m, pl) == table_snapshot(s, m, pl)
    q = m.clone()
    cx.requant(q, [(pl, c, 10) for c in range(3)])
    d, d0 = cx.distortion_ex(m, q, rows=True, normals=True), cx.distortion(m, q, rows=True)
    assert d.normals()["list"] == -1 and d.normals()["reason"] == rec["reason"] and d.rows("normal_error") == 0
    assert d.position() == d0.position() and d.position()["max_dist"] > 0
    for h in (s, plain, d, d0):
        h.close()


# ---- 8. the command line
def test_cli_max_normal_angle_and_report(cx, tmp_path):
    import subprocess

    from harry_amd import cli
    from harry_amd import meshgen as mg
    g = nref.mesh("tri")
    src = tmp_path / "in.ply"
    src.write_bytes(g.to_ply())
    bits = tri_widths(oracle_table("tri", 30))[1]   # one degree

    def run(out, *opts, inp=src):
        return subprocess.run([cli.HARRY, str(inp), str(tmp_path / out), *opts], capture_output=True, text=True, timeout=300)

    r = run("angle.hry", "-l1", "--max-normal-angle", "1", "--report")
    assert r.returncode == 0, r.stderr
    chosen = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("Chosen:")]
    assert [w[1:8:2] + [w[9]] for w in chosen] == [["list", "attr", "bits", "max-angle", "deg"]] * 3
    assert [(int(w[2]), int(w[4]), int(w[6])) for w in chosen] == [(1, 0, bits), (1, 1, bits), (1, 2, bits)]
    m = hc.Mesh.from_ply(src.read_bytes())
    want = nref.compare(dref.values(m, 1)[:, :3], qref.codec_values(cx, m, 1, [0, 1, 2], bits)[:, :3], g.degrees, g.indices)
    max_deg = math.degrees(hc.chord_angle(want["max_chord"]))
    rms_deg = math.degrees(hc.chord_angle(math.sqrt(want["sum_sq_chord"] / want["compared"])))
    assert all(abs(float(w[8]) - max_deg) <= 1e-8 * max_deg for w in chosen) and max_deg <= 1.0
    line, = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("Normals:")]
    assert (line[1], line[3], line[5], line[6], line[8], line[9], line[11]) == ("faces", "max-angle", "deg", "rms", "deg", "collapsed", "degenerate")
    assert (int(line[2]), int(line[10]), int(line[12])) == (g.nf, want["collapsed"], want["degenerate"]) == (3200, 0, 0)
    assert abs(float(line[4]) - max_deg) <= 1e-8 * max_deg and abs(float(line[7]) - rms_deg) <= 1e-8 * rms_deg
    text = r.stdout.splitlines()
    assert text.index(" ".join(line)) == max(i for i, ln in enumerate(text) if ln.startswith("Distortion:")) + 1   # after the Distortion: lines
    explicit = [o for c in range(3) for o in (f"-a{c}", f"-q{bits}")]
    r1 = run("explicit.hry", "-l1", *explicit)
    assert r1.returncode == 0 and "Chosen:" not in r1.stdout and "Normals:" not in r1.stdout
    assert (tmp_path / "angle.hry").read_bytes() == (tmp_path / "explicit.hry").read_bytes()
    # the refusals: several contexts, -q on the same components (all of the list; one of them), an -a, no list, no angle, no faces
    cloud = tmp_path / "cloud.ply"
    cloud.write_bytes(mg.Mesh(g.verts, np.zeros(0, np.uint8), np.zeros(0, np.uint32)).to_ply())
    for opts, inp in ((("--gpus", "2", "-l1", "--max-normal-angle", "1"), src), (("-l1", "-q12", "--max-normal-angle", "1"), src),
                      (("-l1", "-a0", "-q12", "--max-normal-angle", "1"), src), (("-l1", "-a0", "--max-normal-angle", "1"), src),
                      (("--max-normal-angle", "1"), src), (("-l1", "--max-normal-angle", "181"), src), (("-l1", "--max-normal-angle", "-1"), src),
                      (("-l0", "--max-normal-angle", "1"), src), (("-l1", "--max-normal-angle", "1"), cloud)):
        bad = run("bad.hry", *opts, inp=inp)
        assert bad.returncode != 0 and not (tmp_path / "bad.hry").exists(), (opts, bad.stdout, bad.stderr)
    assert "no faces" in run("bad.hry", "-l1", "--max-normal-angle", "1", inp=cloud).stderr
    # beside a -q on another component of the list, and beside --max-error on the positions: every tolerance met
    r2 = run("beside.hry", "-l1", "--max-normal-angle", "10", "--max-error", "1e-5")
    assert r2.returncode == 0, r2.stderr
    s = cx.quant_sweep(m, normals=True)
    both = s.choose([(1, -1, "normal_chord", hc.angle_chord(math.radians(10.0)))] + [(1, c, "max_abs", 1e-5) for c in range(3)])
    assert [(int(w[2]), int(w[4]), int(w[6])) for w in (ln.split() for ln in r2.stdout.splitlines() if ln.startswith("Chosen:"))] == both
    s.close()
    help_ = subprocess.run([cli.HARRY, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--max-normal-angle" in help_
