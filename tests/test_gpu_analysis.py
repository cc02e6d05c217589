"""The twin matcher and the component analysis of twins.hip on the meshes designed for their seams (tests/analysis_meshes.py): the twins
that come down from an upload against the host's matcher (and, on the small meshes, the dictionary restatement of the reference's
rule), the path the matching took, and the device's tables (hry_analysis_tables) against the numpy restatement
(tests/analysis_ref.py), the host's tables and a second run on the same resident mesh -- array by array, no tolerance: all of it is
integer work.  tests/test_analysis_cpu.py asserts the same conditions with the host's twins and compares the host's tables."""
import time

import numpy as np
import pytest

from harry_amd import codec as hc
from oracle import oracle_py as op
from tests import analysis_meshes as am
from tests import analysis_ref as ar

pytestmark = pytest.mark.gpu

NAMES = ("ncomp", "comp") + ar.PER_RANK


@pytest.fixture(scope="module")
def cx():
    c = hc.Codec(0)
    yield c
    c.close()


def same_tables(a, b, what):
    for name in NAMES:
        assert np.array_equal(a[name], b[name]), f"{what}: {name}"


def check_tables(cx, a, nv, what="device"):
    """the device's tables of the resident mesh `a` against the restatement, the host's tables and a second run -> (tables, restatement)"""
    foff, org, twin = a.face_offsets().astype(np.int64), a.org().astype(np.int64), a.twin().astype(np.int64)
    D = cx.analysis_tables(a, where="device")
    R = ar.analysis(foff, org, twin, nv, D["spans"])
    ar.compare(D, R, what)
    H = cx.analysis_tables(a, where="host")
    assert np.array_equal(D["spans"], H["spans"])
    same_tables(D, H, "device against host")
    same_tables(cx.analysis_tables(a, where="device"), D, "second run against the first")   # (atomics in every kernel)
    return D, R


def check_device(cx, m, small=False):
    """upload, twins, twin path, tables -> (offsets, corners, twins, device tables, restatement, the resident mesh)"""
    a = am.to_hc(m)
    cx.upload(a)   # the twins are matched on the device (and what it leaves, on the host)
    foff, org, twin = a.face_offsets().astype(np.int64), a.org().astype(np.int64), a.twin().astype(np.int64)
    assert np.array_equal(twin, am.to_hc(m).twin()), "the twins differ from the host's matcher"
    if small:
        assert np.array_equal(twin, ar.match_twins(foff, org)), "the twins differ from the dictionary restatement"
    D, R = check_tables(cx, a, len(m[0]))
    assert int(D["twin_over"][0]) == am.vertices_over(foff, org, len(m[0])), "k_twin_match reported another count"
    return foff, org, twin, D, R, a


def check_encode(cx, monkeypatch, m):
    """the end the tables serve: the walk on several threads from the device's tables gives the container the oracle writes"""
    monkeypatch.setenv("HRY_DEVICE_ANALYSIS_MIN_FACES", "1")
    monkeypatch.setenv("HRY_PARALLEL_MIN_FACES", "1")
    ply = am.to_ply(m)
    got = cx.write_hry(hc.Mesh.from_ply(ply), profile=hc.PROFILE_CHUNKED)
    assert got == op.Mesh.from_ply(ply).encode_chunked(hc.container_info(got)["chunk_syms"]).data


# ---- the twin matcher
@pytest.mark.parametrize("entries,reported", [(47, 0), (48, 0), (49, 1)])
def test_segment_length(cx, entries, reported):
    m = am.segment_fan(entries)
    foff, org, twin, D, R, _ = check_device(cx, m, small=True)
    seg = am.segment_lengths(foff, org, len(m[0]))
    assert seg[1] == entries == seg.max()
    assert int(D["twin_over"][0]) == reported and am.twin_path(reported) == ("patched" if reported else "device")


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_over_list(cx, n):
    m = am.fans(n)
    foff, org, twin, D, R, _ = check_device(cx, m)
    assert am.vertices_over(foff, org, len(m[0])) == n == int(D["twin_over"][0])
    assert am.twin_path(int(D["twin_over"][0])) == ("host" if n > am.TWIN_OVER_MAX else "patched")
    assert int(D["ncomp"][0]) == n


def test_direction_sequences(cx, monkeypatch):
    m, cases = am.direction_mesh(self_twin=True)
    foff, org, twin, D, R, _ = check_device(cx, m, small=True)
    seqs = {tuple(s) for s in am.direction_sequences(foff, org).values()}
    assert len(cases) == 126 and seqs >= set(cases) | {(None,), (None, None)}
    assert int(D["twin_over"][0]) == 0   # all on the device, the edges that are their own reverse included
    assert np.array_equal(twin, op.Mesh.from_ply(am.to_ply(m)).twin()), "the oracle's twins differ"
    check_encode(cx, monkeypatch, am.direction_mesh()[0])   # (without the faces that repeat a vertex: an encode refuses those, below)


@pytest.mark.parametrize("profile", [hc.PROFILE_COMPAT, hc.PROFILE_CHUNKED])
def test_an_encode_that_would_send_a_vertex_twice_is_refused(cx, profile):
    """a component whose start face repeats a vertex: the walk refuses it before anything sized by the mesh's vertices is written
    (tests/test_analysis_cpu.py), and the context encodes the next mesh as ever"""
    for tris in ([(0, 0, 1), (2, 2, 3), (2, 2, 4)], [(0, 1, 2), (3, 3, 4)]):
        with pytest.raises(hc.HryError) as e:
            cx.write_hry(am.to_hc(am.tri_mesh(tris)), profile=profile)
        assert e.value.code == hc.nat.E_UNSUPPORTED
    ply = am.to_ply(am.tri_mesh([(0, 1, 2), (2, 1, 3)]))
    o = op.Mesh.from_ply(ply)
    got = cx.write_hry(hc.Mesh.from_ply(ply), profile=profile)
    assert got == (o.encode().data if profile == hc.PROFILE_COMPAT else o.encode_chunked(hc.container_info(got)["chunk_syms"]).data)


def test_books(cx):
    m, spines = am.books()
    foff, org, twin, D, R, _ = check_device(cx, m, small=True)
    seg = am.segment_lengths(foff, org, len(m[0]))
    assert [int(seg[s]) for s in spines] == [48, 49] and int(D["twin_over"][0]) == 1
    for s, p in zip(spines, (48, 49)):
        assert am.runs_of(foff, org, s).tolist() == [p]
    assert np.array_equal(twin, op.Mesh.from_ply(am.to_ply(m)).twin())


# ---- the labelling
@pytest.mark.parametrize("reverse", [False, True], ids=["ascending", "reversed"])
@pytest.mark.parametrize("ntri", [16383, 16384, 16385, 32769])
def test_single_strips(cx, ntri, reverse):
    m = am.strip(ntri, reverse)
    foff, org, twin, D, R, _ = check_device(cx, m)
    assert am.leaving(am.face_pairs(foff, twin)) == (ntri - 1) // am.HOOK_FACES
    assert int(D["ncomp"][0]) == 1 and int(D["n_faces"][0]) == ntri and int(D["twin_over"][0]) == 0


def test_alternating_strips(cx):
    n = am.HOOK_FACES + 100
    m = am.alternating_strips(n)
    foff, org, twin, D, R, _ = check_device(cx, m)
    pairs = am.face_pairs(foff, twin)
    tiles = -(-2 * n // am.HOOK_FACES)
    assert tiles == 3 and int(D["ncomp"][0]) == 2
    assert am.labels_per_group(R["comp"], am.HOOK_FACES) == (2, 2)
    out = pairs[pairs[:, 0] // am.HOOK_FACES != pairs[:, 1] // am.HOOK_FACES]
    for t in range(1, tiles):   # every tile boundary joins both components
        assert set(R["comp"][out[out[:, 0] // am.HOOK_FACES == t][:, 0]].tolist()) == {0, 1}


def test_shuffled_tori(cx):
    m = am.shuffled_tori()
    foff, org, twin, D, R, _ = check_device(cx, m)
    pairs = am.face_pairs(foff, twin)
    assert len(m[1]) == 40_000 and int(D["ncomp"][0]) == 2
    assert 2 * am.leaving(pairs) > len(pairs)


def test_repaired_twins(cx, monkeypatch):
    """the resident mesh after an encode that repaired twins: the twins as the encode left them (those of a walk without a device),
    different from the matching between faces of different tiles, two-sided again (tests/test_analysis_cpu.py says why)"""
    monkeypatch.setenv("HRY_DEVICE_ANALYSIS_MIN_FACES", "1")
    monkeypatch.setenv("HRY_PARALLEL_MIN_FACES", "1")
    m = am.repairing()
    a = am.to_hc(m)
    cx.upload(a)
    before = a.twin().copy()
    cx.write_hry(a, profile=hc.PROFILE_CHUNKED)
    walked = am.to_hc(m)
    walked.host_walk(plain=True)
    foff, twin = a.face_offsets().astype(np.int64), a.twin().astype(np.int64)
    assert np.array_equal(twin, walked.twin()) and not np.array_equal(twin, before)
    assert len(m[1]) > am.HOOK_FACES and am.repaired_leaving(foff, before, twin) >= 1 and am.one_sided(twin) == 0
    check_tables(cx, a, len(m[0]))


# ---- the per-component sums
@pytest.mark.parametrize("nf,spare", [(3000, False), (255, False), (256, False), (257, False), (65, False), (3000, True)])
def test_confetti(cx, monkeypatch, nf, spare):
    m = am.confetti(nf, spare)
    foff, org, twin, D, R, _ = check_device(cx, m, small=True)
    assert int(D["ncomp"][0]) == nf and int(D["twin_over"][0]) == 0
    if nf >= am.STATS_BLOCK:
        assert am.labels_per_group(D["comp"], am.STATS_BLOCK) == (am.STATS_BLOCK, am.STATS_BLOCK)
    if spare:   # the neutral word in every wavefront of k_cc_vertex_stats
        assert (R["vfirst"][:len(R["vfirst"]) // am.WAVE * am.WAVE].reshape(-1, am.WAVE) == ar.NONE).any(axis=1).all()
    if nf == 3000 and not spare:
        assert nf > 2 * am.SCAN_BLOCK
        check_encode(cx, monkeypatch, m)


def test_interleaved_strips(cx, monkeypatch):
    m = am.interleaved_strips()
    foff, org, twin, D, R, _ = check_device(cx, m, small=True)
    assert int(D["ncomp"][0]) == 64 and len(m[1]) % am.STATS_BLOCK == 0
    assert am.labels_per_group(R["rank_of_face"], am.WAVE) == (64, 64)
    assert (R["vfirst"] != ar.NONE).all() and am.labels_per_group(R["vfirst"], am.WAVE) == (64, 64)
    rows = np.diff(foff).reshape(-1, am.WAVE)
    assert set(rows.reshape(-1).tolist()) == {3, 4, 9}
    assert ((rows == rows.max(axis=1, keepdims=True)).sum(axis=1) < am.WAVE // 2).all()   # the round count is not most lanes' degree
    check_encode(cx, monkeypatch, m)


def test_face0_component(cx):
    m = am.face0_last()
    foff, org, twin, D, R, _ = check_device(cx, m, small=True)
    assert int(ar.positions(D["spans"], [0])[0]) == len(m[1]) - 1    # face 0 is the last of the sequence ...
    assert int(D["n_faces"][0]) == 1 and int(D["seed"][0]) == 0       # ... a component of its own, and coded first
    assert int(D["by_rank"][0]) == int(D["comp"][0]) == 0 and int(D["ncomp"][0]) == 4


# ---- the ties
def test_chain(cx, monkeypatch):
    m = am.chain()
    foff, org, twin, D, R, _ = check_device(cx, m, small=True)
    assert int(D["ncomp"][0]) == 5000 and am.vertex_sets(foff, org) == 1
    assert (D["group"] == 0).all()
    check_encode(cx, monkeypatch, m)


def test_hub_and_pairs(cx):
    m = am.hub_and_pairs()
    foff, org, twin, D, R, _ = check_device(cx, m, small=True)
    assert int(D["ncomp"][0]) == 600 and am.vertex_sets(foff, org) == 1 + 150
    assert int(D["twin_over"][0]) == 1
    sizes = np.sort(np.bincount(D["group"])[np.unique(D["group"])])
    assert sizes.tolist() == [2] * 150 + [300]


def test_overflow(cx):
    """more pairs than one sub-list of the tie list holds: k_cc_vertex_ties unites the rest on the spot.  The heaviest case: its
    steps are timed and printed (pytest -s)"""
    t = [time.perf_counter()]
    m = am.overflow()
    t.append(time.perf_counter())
    a = am.to_hc(m)
    cx.upload(a)
    t.append(time.perf_counter())
    foff, org, twin = a.face_offsets().astype(np.int64), a.org().astype(np.int64), a.twin().astype(np.int64)
    D = cx.analysis_tables(a, where="device")
    t.append(time.perf_counter())
    D2 = cx.analysis_tables(a, where="device")
    t.append(time.perf_counter())
    R = ar.analysis(foff, org, twin, len(m[0]), D["spans"])
    t.append(time.perf_counter())
    H = cx.analysis_tables(a, where="host")
    t.append(time.perf_counter())
    assert np.array_equal(twin, am.to_hc(m).twin()), "the twins differ from the host's matcher"
    t.append(time.perf_counter())
    print("\noverflow: " + ", ".join(f"{k} {1e3 * (y - x):.0f} ms" for k, x, y in zip(
        ("generator", "upload", "device tables", "second run", "restatement", "host tables", "host matcher"), t, t[1:])))
    ar.compare(D, R, "device")
    same_tables(D, H, "device against host")
    same_tables(D2, D, "second run against the first")
    assert int(R["ncomp"][0]) == len(m[1])                             # no two octagons share an edge
    hits = am.tie_hits(R["hit"], foff)
    assert hits.max() > am.TIE_SUB and hits.min() >= 1                 # a sub-list is full: pairs go to it and to the fallback
    assert int(D["twin_over"][0]) == am.vertices_over(foff, org, len(m[0])) == 4 * am.OVERFLOW_POOL < am.TWIN_OVER_MAX
    assert (D["group"] == 0).all()
