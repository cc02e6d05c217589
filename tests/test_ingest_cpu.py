"""Meshes from device buffers (include/harry_amd.h: hry_mesh_from_device), the parts that need no GPU: the declarations and exports,
refusals of null arguments, and the tests' restatement of the weld (tests/ingest_ref.py) on hand-made cases."""
import ctypes as C
import os
import re

import numpy as np

from harry_amd import _native as nat
from tests import ingest_ref as ir
from tests import util


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(util.ROOT, "include", "harry_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("hry_mesh_from_device", "hry_mesh_resident"):
        assert re.search(r"\b" + name + r"\s*\(", code), name
    assert re.search(r"typedef struct hry_dev_column\s*\{", code) and re.search(r"\}\s*hry_dev_column\s*;", code)
    assert re.search(r"#define HRY_INGEST_WELD 1\b", code)
    L = nat.load()
    assert hasattr(L, "hry_mesh_from_device") and hasattr(L, "hry_mesh_resident")
    assert C.sizeof(nat.DevColumn) == 32


def test_null_arguments():
    L = nat.load()
    out = C.c_void_p(1)
    col = (nat.DevColumn * 1)(nat.DevColumn(None, 4, b"x", 0))
    # null context
    assert L.hry_mesh_from_device(None, 1, col, 1, 0, None, None, 4, 0, None, 0, 0, None, C.byref(out)) == nat.E_ARG
    assert not out.value
    # null out
    assert L.hry_mesh_from_device(None, 1, col, 1, 0, None, None, 4, 0, None, 0, 0, None, None) == nat.E_ARG
    # null columns with components announced
    out = C.c_void_p(1)
    assert L.hry_mesh_from_device(None, 1, None, 3, 0, None, None, 4, 0, None, 0, 0, None, C.byref(out)) == nat.E_ARG
    assert not out.value
    assert L.hry_mesh_from_device(None, 1, col, 1, 1, None, None, 4, 3, None, 2, 0, None, C.byref(out)) == nat.E_ARG
    assert L.hry_mesh_resident(None, None) == 0


def _f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def test_weld_restatement_hand_cases():
    # -0.0 and +0.0 stay apart; equal bits merge
    x = np.array([0.0, -0.0, 0.0, -0.0], np.float32)
    remap, first = ir.weld(ir.packed_records([x]))
    assert remap.tolist() == [0, 1, 0, 1] and first.tolist() == [0, 1]
    # two NaN payloads stay apart, identical NaN bit patterns merge
    n = _f32([0x7FC00000, 0x7FC00001, 0x7FC00000, 0xFFC00000])
    remap, first = ir.weld(ir.packed_records([n, np.zeros(4, np.float32)]))
    assert remap.tolist() == [0, 1, 0, 2] and first.tolist() == [0, 1, 3]
    # all rows equal: one vertex
    a = np.full(7, 1.5, np.float32)
    remap, first = ir.weld(ir.packed_records([a, a, np.full(7, 3, np.uint8)]))
    assert remap.tolist() == [0] * 7 and first.tolist() == [0]
    # no rows equal: the identity
    b = np.arange(9, dtype=np.float32)
    remap, first = ir.weld(ir.packed_records([b, b[::-1].copy()]))
    assert remap.tolist() == list(range(9)) and first.tolist() == list(range(9))
    # numbering follows first occurrence, not value order
    c = np.array([5, 3, 5, 1, 3, 1, 9], np.int32)
    remap, first = ir.weld(ir.packed_records([c]))
    assert remap.tolist() == [0, 1, 0, 2, 1, 2, 3] and first.tolist() == [0, 1, 3, 6]
    # records mixing widths: a difference in the last byte of the record matters
    u = np.array([7, 7, 7], np.uint8)
    f = np.array([2.0, 2.0, 2.0], np.float32)
    g = np.array([1, 1, 2], np.uint16)
    remap, _ = ir.weld(ir.packed_records([f, g, u]))
    assert remap.tolist() == [0, 0, 1]
    assert ir.weld(np.zeros((0, 4), np.uint8))[0].size == 0
