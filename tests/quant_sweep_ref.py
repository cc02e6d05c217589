"""Restatement in numpy of the quantisation sweep's table and choice rule (include/harry_amd.h: hry_quant_sweep_build,
hry_quant_choose, hry_quant_pick).  The table of a component is, per width, the record tests/distortion_ref.compare gives for the
source's values x against y = the values after a requant of a clone to that width and a requant(clear=True) -- and y comes from
code that is not under test: the oracle's requant on the CPU (oracle_values), Codec.requant -- k_requant, pinned to the
reference's goldens -- on the GPU (codec_values).  pick: the smallest width whose record meets the metric at that width."""
from __future__ import annotations

import math

import numpy as np

from tests import distortion_ref as dref

MAX_ABS, MAX_REL, RMS, POS_DIST = 0, 1, 2, 3


def meets(rec: dict, metric: int, extent: float, value: float) -> bool:
    if metric == MAX_ABS:
        return rec["max_abs"] <= value
    if metric == MAX_REL:
        return rec["max_abs"] <= value * extent
    if metric == RMS:
        return rec["compared"] != 0 and math.sqrt(rec["sum_sq"] / rec["compared"]) <= value
    raise ValueError(metric)


def pick(table: list, metric: int, extent: float, value: float) -> int:
    """table[bits - 1]: the record at `bits`.  The smallest bits whose record meets (metric, value); 0: none does.  The table need
    not be monotone: nothing is said about wider widths"""
    assert value >= 0
    for bits, rec in enumerate(table, 1):
        if meets(rec, metric, extent, value):
            return bits
    return 0


def oracle_values(src, l: int, comps, bits: int) -> np.ndarray:
    """src: an oracle mesh (oracle_py.Mesh).  Its list l as doubles [rows, ncomp] after components `comps` went to `bits` and back"""
    q = src.clone()
    q.requant([(l, c, bits) for c in comps])
    q.requant([], clear=True)
    return dref.values(q, l)


def codec_values(cx, src, l: int, comps, bits: int) -> np.ndarray:
    """the same through Codec.requant (src: a codec Mesh)"""
    q = src.clone()
    cx.requant(q, [(l, c, bits) for c in comps])
    cx.requant(q, [], clear=True)
    return dref.values(q, l)


def table(values_at, x: np.ndarray, c: int, qmax: int) -> list:
    """values_at(comps, bits) -> [rows, ncomp] as above; x: the source's values [rows, ncomp].  The records of component c at
    1 .. qmax bits (skipped is 0: the identity pairs every row)"""
    return [dref.compare(x[:, [c]], values_at([c], q)[:, [c]])["comp"][0] for q in range(1, qmax + 1)]


def position_table(values_at, x: np.ndarray, pos: int, qmax: int) -> list:
    """the positions' records (hry_pos_error without `list`) with components pos .. pos + 2 all at 1 .. qmax bits"""
    cols = [pos, pos + 1, pos + 2]
    return [dref.compare(x[:, cols], values_at(cols, q)[:, cols], pos=0)["pos"] for q in range(1, qmax + 1)]
