"""Textured meshes from device buffers (include/harry_amd.h: hry_mesh_from_device_corners), the parts that need no GPU: the
declarations and exports, refusals of null arguments, and the tests' restatement (tests/ingest_corners_ref.py) on hand-made cases."""
import ctypes as C
import os
import re

import numpy as np

from harry_amd import _native as nat
from tests import ingest_corners_ref as icr
from tests import util


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(util.ROOT, "include", "harry_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bhry_mesh_from_device_corners\s*\(", code)
    assert re.search(r"typedef struct hry_dev_rows\s*\{", code) and re.search(r"\}\s*hry_dev_rows\s*;", code)
    assert re.search(r"#define HRY_ABI_VERSION 6\b", code)
    assert hasattr(nat.load(), "hry_mesh_from_device_corners")
    assert C.sizeof(nat.DevRows) == 24


def test_null_arguments():
    L = nat.load()
    col = (nat.DevColumn * 3)(*[nat.DevColumn(None, 12, None, 0)] * 3)
    pos = nat.DevRows(col, 3, 0, None)
    ctx = None   # (no context without a device; tests/test_gpu_ingest_corners.py repeats the null pos with a real one)
    out = C.c_void_p(1)
    assert L.hry_mesh_from_device_corners(None, C.byref(pos), None, None, 0, None, 4, 0, None, 0, None, C.byref(out)) == nat.E_ARG
    assert not out.value
    assert L.hry_mesh_from_device_corners(ctx, C.byref(pos), None, None, 0, None, 4, 0, None, 0, None, None) == nat.E_ARG
    out = C.c_void_p(1)
    assert L.hry_mesh_from_device_corners(ctx, None, None, None, 0, None, 4, 0, None, 0, None, C.byref(out)) == nat.E_ARG
    assert not out.value


def test_regions_by_first_occurrence():
    assert icr.regions_by_first_occurrence([7, 7, 3, 7, 9, 3]).tolist() == [0, 0, 1, 0, 2, 1]
    assert icr.regions_by_first_occurrence(np.array([65535, 0, 65535], np.uint16)).tolist() == [0, 1, 0]
    assert icr.regions_by_first_occurrence(np.array([-1, 2, -1], np.int16).view(np.uint16)).tolist() == [0, 1, 0]
    assert icr.regions_by_first_occurrence([]).size == 0


def test_slot_compaction():
    ti, ni = np.array([4, 5, 6]), np.array([1, 0, 2])
    assert icr.corner_attr(3, ti, ni).tolist() == [[4, 1], [5, 0], [6, 2]]
    assert icr.corner_attr(3, ti, None).tolist() == [[4, 0], [5, 0], [6, 0]]
    assert icr.corner_attr(3, None, ni).tolist() == [[1, 0], [0, 0], [2, 0]]   # normals alone sit in slot 0
    assert icr.corner_attr(3).tolist() == [[0, 0]] * 3
    assert icr.corner_attr(3, None, ni, None, np.array([2, 2, 0])).tolist() == [[2, 0], [2, 0], [0, 0]]
    assert icr.vtx_attr(3).tolist() == [[0], [1], [2]]


def test_weld_of_a_list_with_signed_zeros_and_nan_payloads():
    u = np.array([0x00000000, 0x80000000, 0x7FC00000, 0x7FC00001, 0x7FC00000, 0x00000000], np.uint32).view(np.float32)
    rows = np.stack([u, np.ones(6, np.float32)], axis=1)
    remap, welded = icr.weld_rows(rows)
    assert remap.tolist() == [0, 1, 2, 3, 2, 0]
    assert welded.view(np.uint32)[:, 0].tolist() == [0x00000000, 0x80000000, 0x7FC00000, 0x7FC00001]
    e = icr.expected(np.zeros((2, 3), np.float32), [0, 1, 0], uv=rows, uv_idx=[5, 4, 1], weld=True)
    assert e["org"].tolist() == [0, 0, 0] and len(e["lists"][0]) == 1
    assert e["corner_attr"].tolist() == [[0, 0], [2, 0], [1, 0]]
