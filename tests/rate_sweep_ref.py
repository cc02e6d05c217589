"""Restatement in numpy of the host half of the rate sweep (include/harry_amd.h: hry_rate_hist_bytes, hry_rate_pick): the zeroth-order
entropy of a histogram in bytes and the largest width whose bytes fit a budget.  Shared by the rate sweep's tests."""
import math

import numpy as np


def hist_bytes(hist) -> float:
    """(sum over the symbols with a count, ascending, of count * log2(n / count)) / 8, in double; 0 for an empty histogram"""
    h = np.asarray(hist, np.uint64)
    n = int(h.sum())
    if n == 0:
        return 0.0
    bits = 0.0
    for k in h[h > 0]:
        bits += float(k) * math.log2(float(n) / float(k))
    return bits / 8.0


def planes_bytes(hists) -> float:
    """a component's planes, in plane order"""
    total = 0.0
    for h in hists:
        total += hist_bytes(h)
    return total


def pick(bytes_by_bits, budget: float) -> int:
    """the LARGEST bits in 1 .. len(table) with table[bits - 1] <= budget; 0: none"""
    for q in range(len(bytes_by_bits), 0, -1):
        if bytes_by_bits[q - 1] <= budget:
            return q
    return 0


def planes_at(bits: int) -> int:
    """byte planes of a component quantised to `bits`: its storage type is u8 up to 8 bits, u16 up to 16, u32 above"""
    return 1 if bits <= 8 else 2 if bits <= 16 else 4
