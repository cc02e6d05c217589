"""The first-occurrence numbering (harry_amd/csrc/device/dedup.hip) where its probe table collides: the designed inputs of
tests/dedup_cases.py -- every key's home at the end of the table, so one cluster as long as the case has keys, wrapping from the last
slot to slot 0 -- through the public entries of all five key policies, against the restatements the neighbouring files use.  Every
case is built twice and every buffer of the two builds has the same bytes (the numbering may not depend on the order the atomics
complete in), and every case asserts its census again from the buffers the build returned, the item count that fixes the table's
size included: a case cannot pass on another table than the one it was designed for.  (That the restated hashes are the source's:
tests/test_dedup_cpu.py.)"""
import numpy as np
import pytest

from harry_amd import codec as hc
from tests import dedup_cases as dc
from tests import dedup_ref as dr
from tests import ingest_ref as ir
from tests import render_ref as rr
from tests.test_gpu_creases import check as check_creases
from tests.test_gpu_edges import check as check_edges
from tests.test_gpu_render import check_render
from tests.test_gpu_shells import check as check_shells
from tests.util import same_bytes, xyz_mesh

pytestmark = pytest.mark.gpu

try:   # (torch takes the device before the first Codec, as in test_gpu_ingest.py; only the weld needs it)
    import torch
except ImportError:
    torch = None


@pytest.fixture(scope="module")
def cx():
    c = hc.Codec(0)
    yield c
    c.close()


def same_census(seen, designed):
    """the census from a build's buffers is the designed one, the occupied slots included"""
    assert sorted(seen) == sorted(designed)
    for k in designed:
        assert np.array_equal(seen[k], designed[k]), (k, seen[k], designed[k])


# ---- weld (WeldKey): Codec.mesh_from_tensors(weld=True)
def weld_build(cx, cols, face):
    if torch is None:
        pytest.skip("no torch")
    t = torch.from_numpy(np.ascontiguousarray(np.stack(cols, axis=1))).to(torch.device("cuda", 0))
    names = "x y z a3 a4 a5 a6 a7 a8".split()[:len(cols)]   # (names the layout keeps in this order: the key is the record as laid out)
    mesh, remap = cx.mesh_from_tensors(torch.from_numpy(np.asarray([face], np.int32)).to(t.device), [(" ".join(names), t)], weld=True, return_remap=True)
    return {"remap": remap.cpu().numpy().view(np.uint32), "records": mesh.list_data(1).copy(), "org": mesh.org().copy(), "nv": np.array([mesh.nv])}


WELD_CASES = {
    "one_home_3": lambda: dc.weld_one_home(3),
    "one_home_32": lambda: dc.weld_one_home(32),          # 64 slots at load 1/2 ...
    "one_home_33": lambda: dc.weld_one_home(33),          # ... and 128 at load 1/4, one row later
    "one_home_2048": lambda: dc.weld_one_home(2048),      # 4096 slots at load 1/2: the last row passes 2047 foreign rows
    "last_slots_dups": lambda: dc.weld_last_slots_dups(),
    "stride36_one_home": lambda: dc.weld_stride36_one_home(),
}


@pytest.mark.parametrize("name", sorted(WELD_CASES))
def test_weld(cx, name):
    cols, census = WELD_CASES[name]()
    rec = ir.packed_records(cols)
    want_remap, first = ir.weld(rec)
    face = first[:3].tolist()                              # three rows that stay three vertices
    got = weld_build(cx, cols, face)
    assert got["nv"][0] == len(first) == census["keys"] and len(got["remap"]) == census["items"]
    assert np.array_equal(got["remap"], want_remap)
    assert np.array_equal(got["records"], rec[first]) and np.array_equal(got["org"], want_remap[face])
    same_bytes(weld_build(cx, cols, face), got)
    seen = dc.census_of(dr.weld_hash(got["records"]), len(got["remap"]))   # the first rows, in the order the weld numbered them
    same_census(seen, census)
    assert seen["wraps"] and seen["longest_run"] == seen["keys"] == seen["homes_in_last"]


# ---- edges (EdgeKey): Codec.edges_numpy
def test_edges_fan(cx):
    pos, tris, census = dc.edge_fan_one_cluster()
    mesh = xyz_mesh(pos, tris)
    got, want = check_edges(cx, mesh, "edge_fan_one_cluster")
    same_bytes(cx.edges_numpy(mesh, geometry=True), got)
    rn = cx.render_numpy(mesh)
    assert got["edge_sides"].size == 3 * len(tris) == census["items"] and len(got["edges"]) == census["keys"]
    seen = dc.edges_census(rn["indices"], rn["vertex_source"])
    same_census(seen, census)
    # ... and from the edge rows themselves, which the build numbered: the same keys in the same order
    rows = rn["vertex_source"][got["edges"]]
    assert np.array_equal(dc.census_of(dr.edge_hash(rows[:, 0], rows[:, 1]), got["edge_sides"].size)["occupied"], census["occupied"])
    spokes = rows[:, 0] == 0
    assert spokes.sum() == len(tris) >= 1024 and (np.diff(got["edge_offsets"].astype(np.int64))[spokes] == 2).all()
    assert seen["spokes_in_last"] >= 1024 and seen["wraps"] and seen["longest_run"] >= seen["spokes_in_last"] and seen["slots"] == 8192


# ---- unweld (UnweldKey): Codec.render_numpy of an OBJ scene
def test_unweld(cx):
    obj, pairs, census = dc.unweld_one_home()
    mesh = hc.Mesh.from_obj(obj, "")
    got = check_render(cx, mesh)
    same_bytes(cx.render_numpy(mesh), got)
    keys = rr.corner_keys(mesh)                            # org, then the corner lists in list order: what the unweld's view derives
    assert len(keys) == mesh.ne == census["items"] == 2048 and len(got["corner_source"]) == census["keys"] == 1024
    distinct = keys[got["corner_source"]]                  # the keys the build numbered, in its order
    same_census(dc.census_of(dr.unweld_hash(distinct), mesh.ne), census)
    assert np.array_equal(distinct[:, 0], got["vertex_source"]) and np.array_equal(distinct, pairs[:1024].astype(np.uint32))
    assert census["wraps"] and census["longest_run"] == 1024 and census["slots"] == 4096
    ids, _ = dr.first_occurrence(keys)
    assert np.bincount(ids).tolist() == [2] * 1024         # every output vertex is shared by two corners


# ---- shells (ShellVertexKey): Codec.shells_numpy
@pytest.mark.parametrize("shells", [1, 2])
def test_shells_strips(cx, shells):
    pos, tris, census = dc.shell_vertex_one_home(shells)
    mesh = xyz_mesh(pos, tris)
    got, want = check_shells(cx, mesh, f"shell_vertex_one_home({shells})")
    same_bytes(cx.shells_numpy(mesh, geometry=True), got)
    rn = cx.render_numpy(mesh)
    T = len(tris)
    assert len(got["shell_first"]) == shells and np.array_equal(got["tri_shell"], np.repeat(np.arange(shells), T // shells))
    assert got["shell_counts"][:, 2].tolist() == [T // shells + 2] * shells and got["shell_counts"][:, 7].tolist() == [1] * shells
    seen = dc.shells_census(dc.shell_keys(rn["indices"], rn["vertex_source"], got["tri_shell"]))
    same_census(seen, census)
    assert seen["items"] == 3 * T == rn["indices"].size and seen["corners_in_last"] >= 1024 and seen["wraps"] and seen["longest_run"] == seen["keys"]


# ---- creases (CreaseKey): Codec.creases_numpy
def test_creases_soup(cx):
    pos, tris, census = dc.crease_soup_one_home()
    mesh = xyz_mesh(pos, tris)
    case = ("area", dc.CREASE_COS_LIMIT)
    want, got = check_creases(cx, mesh, "crease_soup_one_home", cases=[case])[case]
    same_bytes(cx.creases_numpy(mesh, cos_limit=dc.CREASE_COS_LIMIT, weights="area"), got)
    rn = cx.render_numpy(mesh)
    n = 3 * len(tris)
    assert np.array_equal(got["slot_group"].reshape(-1), np.arange(n))           # every slot a group of its own: the roots are the slots
    assert np.array_equal(got["indices"].reshape(-1), np.arange(n)) and np.array_equal(got["render_vertex"], rn["indices"].reshape(-1))
    seen = dc.creases_census(dc.crease_keys(rn["indices"], got["slot_group"]))
    same_census(seen, census)
    assert seen["items"] == n == rn["indices"].size and seen["wraps"] and seen["longest_run"] == seen["keys"] == n
