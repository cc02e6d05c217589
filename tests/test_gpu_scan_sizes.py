"""The block boundaries of the device scans (harry_amd/csrc/device/scan.hip over wave.hpp), each through a user whose result is
pinned by a host computation: the three-launch scan through the twin matcher, the one-block scan through the ingest's face
offsets, the three-launch scan with its total in a word of its own through the events of an OBJ scene."""
import numpy as np
import pytest

from harry_amd import codec as hc
from harry_amd import meshgen as mg
from harry_amd import objgen as og
from oracle import oracle_py as op   # checker only
from tests.test_gpu_obj import same_decoded

pytestmark = pytest.mark.gpu

try:   # (torch takes the device before the first Codec, as in test_gpu_ingest.py; only the face offsets need it)
    import torch
except ImportError:
    torch = None
XYZ = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")])


@pytest.fixture(scope="module")
def cx():
    c = hc.Codec(0)
    yield c
    c.close()


# ---- 1. launch_excl_scan over nv counters (launch_twins)
def pairs_mesh(nv: int) -> mg.Mesh:
    """nv vertices, nearly all named by no face, and one pair of triangles on the vertices w .. w + 3 of every window that fits: at
    0, at 1021 (across the first block edge of the scan), in the middle of the large sizes (across block edge 512) and at nv - 4.
    The pair shares the edge of its two HIGHEST vertices, (w + 2, w + 3): the twin matcher keeps a half-edge in the segment of its
    smaller endpoint, so the two that match lie in the segment of w + 2 = [start[w + 2], start[w + 3]) -- of 1023 and 1024 for the
    window at 1021, of nv - 2 and nv - 1 for the last one: prefixes from both sides of a block edge, and the last block's."""
    starts = sorted({w for w in (0, 1021, 512 * 1024 - 3 if nv > 2 ** 19 else 0, nv - 4) if w + 4 <= nv})
    tris = []
    for w in starts:
        tris += [(w + 2, w + 3, w), (w + 3, w + 2, w + 1)]
    v = np.zeros(nv, XYZ)
    v["x"] = np.arange(nv, dtype=np.float32) / nv
    v["y"] = np.arange(nv) % 7
    v["z"] = np.arange(nv) % 3
    return mg.Mesh(v, np.full(len(tris), 3, np.uint8), np.array(tris, np.uint32).reshape(-1))


@pytest.mark.parametrize("nv", [1024, 1025, 2 ** 20, 2 ** 20 + 1])
def test_twins_at_the_scan_block_edges(cx, nv):
    """1024: one full block, the total from its last thread; 1025: two blocks, the block sums are used; 2^20: 1024 block sums, one
    pass of k_scan_top; 2^20 + 1: 1025 block sums, a second pass with a carry"""
    m = pairs_mesh(nv)
    a, b = (hc.Mesh.from_arrays(m.verts, m.degrees, m.indices) for _ in range(2))
    want = b.twin().copy()   # no context: the host's matcher
    assert (want != np.arange(len(want))).sum() == m.nf   # every pair has found its shared edge, nothing else matches
    cx.upload(a)
    assert np.array_equal(a.twin(), want)
    if nv <= 1025:
        assert np.array_equal(want, op.Mesh.from_ply(m.to_ply()).twin())


# ---- 2. launch_scan_counts over the wave sums of the degrees (launch_ingest_offsets)
@pytest.mark.parametrize("nf", [64, 65, 65536, 65537])
def test_face_offsets_at_the_one_block_scan_edges(cx, nf):
    """1, 2, 1024 and 1025 wave sums: a thread of k_scan_counts owns one entry, then two with the trailing threads empty.  Face f
    is on the vertices f .. f + degree - 1: valences stay small, no hub goes to the host"""
    if torch is None:
        pytest.skip("torch is not installed")
    DEV = torch.device("cuda", 0)
    rng = np.random.default_rng(41)
    deg = rng.integers(3, 7, nf).astype(np.uint8)
    idx = np.concatenate([np.arange(f, f + d) for f, d in enumerate(deg.tolist())]).astype(np.int64)
    v = np.zeros(nf + 8, XYZ)
    for k in "xyz":
        v[k] = rng.random(nf + 8, dtype=np.float32)
    xyz = torch.from_numpy(np.stack([v[k] for k in "xyz"], axis=1)).to(DEV)
    a = cx.mesh_from_tensors(torch.from_numpy(idx).to(DEV), [("x y z", xyz)], degrees=torch.from_numpy(deg).to(DEV))
    assert np.array_equal(a.face_offsets(), np.concatenate([[0], np.cumsum(deg, dtype=np.int64)]))
    b = hc.Mesh.from_arrays(v, deg, idx.astype(np.uint32))
    assert (a.nv, a.nf, a.ne) == (b.nv, b.nf, b.ne)
    for get in ("org", "twin", "face_offsets"):
        assert np.array_equal(getattr(a, get)(), getattr(b, get)()), get
    assert a.list_fmt(1) == b.list_fmt(1) and np.array_equal(a.list_data(1), b.list_data(1))


# ---- 3. launch_excl_scan with a separate total (events.hip)
def flat_scene(ntri: int) -> og.Scene:
    """general bindings, a normal per face named by its three corners: one corner list with 3 ntri references"""
    m = mg.torus(16, 32)
    assert m.nf == 1024 and (m.degrees == 3).all()
    if ntri == 1025:   # ... and a triangle of its own
        t = np.zeros(3, m.verts.dtype)
        t["x"], t["y"], t["z"] = [3.0, 4.0, 3.0], [0.0, 0.0, 1.0], [0.5, 0.25, 0.125]
        m = mg.concat([m, mg.Mesh(t, np.full(1, 3, np.uint8), np.arange(3, dtype=np.uint32))])
    assert m.nf == ntri
    return og.scene(m, normals="flat")


@pytest.mark.parametrize("ntri", [1024, 1025])
def test_events_at_the_scan_block_edges(cx, ntri):
    """the corner list's counters are scanned over the 1024 / 1025 coded faces, its 3072 / 3075 references three times, every
    total in a word of `counts`: the chunked container is the oracle's, and decodes like the reference stream"""
    sc = flat_scene(ntri)
    m, o = hc.Mesh.from_obj(sc.obj, ""), op.Mesh.from_obj(sc.obj, "")
    assert m.nf == ntri
    got = cx.write_hry(m, profile=hc.PROFILE_CHUNKED)
    info = hc.container_info(got)
    assert info["minor"] == 2
    assert got == o.clone().encode_chunked(info["chunk_syms"]).data
    same_decoded(cx.read_hry(got), op.Mesh.from_hry(o.clone().encode().data))
