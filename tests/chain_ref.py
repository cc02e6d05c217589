"""What a mesh demands of the decoder's reconstruction chain, from the CPU oracle alone (numpy only).

Input: the oracle's vertex trace of a reference-format decode (oracle_py.Mesh.vertex_trace(): per vertex in decode numbering the
candidate count, the first eight candidate triples (a, b, o) in the reference's fan order, per component the prediction used), the
decoded values of one component in their storage type, its quantisation bits q (0: lossless) and every component's first vertex.

classify_vertices() says per vertex what it is; classify_tiles() says per 64-aligned tile of a chain run by a team of W wavefronts
what the tile is.  The rules restate the comments of make_chain_rec_ids and unpredict3_segment (harry_amd/csrc/device/
unpredict.hip) as facts about the input -- which source is the predecessor, how far back the others lie, whether the parallelogram
leaves [0, top], which form the residual code has (prediction.h:46-64) -- not the kernels' arithmetic: nothing here evaluates a map,
a scan or an interval.

    chained vertex   one or two candidates, and source a or b of one of them is v - 1 (the first such slot in row order), v not
                     the first vertex of its component; every other vertex is a constant of its run
    gap              v + 1 - (the most recent source other than the chained one + 1); 65535 without one (and never more)
    far              a source more than kRing3Near = 16 320 vertices back, or of an earlier component (ring_edge: one of the vertex's
                     own component 16 321 .. 16 384 back -- still inside the ring of 16 384, far by the margin of one tile)
    head (team W)    more than two candidates, or a source other than the predecessor that is not final when the tile is
                     prepared: gap <= lane + 64 (W - 1)
    row head         a head with more than two candidates or a far source
    prepared tile    at most kMaxHeads = 8 heads and at most 8 row heads; else "late" when at most kMaxHeadsLate = 12 vertices have
                     more than two candidates or their latest other source inside the tile itself; else "dense"
    run              the vertices between two heads of a tile (late tile: between two such inner vertices)
    leaves the form  a chained vertex whose chained candidate's a + b - o lies outside [0, top], or whose residual code is far
                     or raw: the speculated map does not describe it, the verified path repairs it (one per run: one more scan;
                     a second one: the run is finished vertex by vertex)
    long stretch     17 or more chained two-candidate vertices in a row inside a run: the composed map's k passes 16
"""
import numpy as np

RING3 = 16384
RING3_NEAR = RING3 - 64
MAX_HEADS, MAX_HEADS_LATE = 8, 12
POS_NONE = 7
NEAR, FAR, RAW = 0, 1, 2
COUNT_CLASSES = ("cand0", "cand1", "cand2", "cand3_8", "cand9p")


def ordered_u32(bits):
    """float bits -> the order-preserving unsigned the residual is folded in (transform.h:19-23; the sign mask that
    prediction.h:33-44 applies to 4-byte floats is zero)"""
    u = np.asarray(bits, np.uint32)
    return u ^ ((np.uint32(0) - (u >> np.uint32(31))) >> np.uint32(1))


def code_class(value, pred, top):
    """prediction.h:46-64, from the decoder's side: RAW when the prediction is 0 (the code is the value), FAR when the code's
    upper bits pass min(pred - 1, top - pred), NEAR otherwise.  value, pred: unsigned integers as int64; the code is the one
    prediction.h:81-99 writes for them."""
    value, pred = np.asarray(value, np.int64), np.asarray(pred, np.int64)
    max_pos = top - pred
    bm_enc = np.minimum(pred, max_pos)
    dlt = np.abs(value - pred)
    code = np.where(dlt > bm_enc, dlt + bm_enc, np.where(value < pred, 2 * dlt - 1, 2 * dlt))
    far = (code >> 1) > np.minimum(pred - 1, max_pos)
    return np.where(pred == 0, RAW, np.where(far, FAR, NEAR)).astype(np.uint8)


def classify_vertices(trace, values, q, comp_first, comp, rings=(4096, 8192, RING3_NEAR)):
    """values: component `comp` of the decoded vertex list in its storage type (uint8 / uint16 / uint32 / float32), decode numbering"""
    count = trace["count"].astype(np.int64)
    tri = trace["triples"].astype(np.int64)
    n = len(count)
    v = np.arange(n, dtype=np.int64)
    comp_first = np.asarray(comp_first, np.int64)
    seg = np.searchsorted(comp_first, v, side="right") - 1
    seg_begin = comp_first[seg]
    is_float = values.dtype.kind == "f"
    bits = values.dtype.itemsize * 8
    top = (1 << q) - 1 if q else (1 << bits) - 1

    out = {"n": n, "seg": seg, "seg_begin": seg_begin, "count": count, "top": top}
    out["cand0"], out["cand1"], out["cand2"] = count == 0, count == 1, count == 2
    out["cand3_8"], out["cand9p"] = (count >= 3) & (count <= 8), count > 8
    nc = np.minimum(count, 3)
    out["nc"] = nc

    # ---- the chained source and the gap (at most two candidates: the compact row)
    row = tri[:, :2].reshape(n, 6)
    j = np.arange(6)
    in_row = (j[None, :] < 3 * count[:, None]) & (count[:, None] <= 2)
    is_pred = in_row & (row + 1 == v[:, None]) & (j[None, :] % 3 != 2) & (v > seg_begin)[:, None]
    pos = np.where(is_pred.any(axis=1), is_pred.argmax(axis=1), POS_NONE)
    other = in_row & (j[None, :] != pos[:, None])
    need = np.where(other, row + 1, 0).max(axis=1)
    gap = np.minimum(np.where(need > 0, v + 1 - need, 65535), 65535)
    out["pos"], out["gap"] = pos, gap
    out["chained"] = pos != POS_NONE
    out["constant"] = ~out["chained"]

    # ---- every source the vertex reads (up to eight candidates)
    k = np.arange(8)
    have = np.broadcast_to((k[None, :] < np.minimum(count, 8)[:, None])[:, :, None], tri.shape)
    back = v[:, None, None] - tri
    out["recent"] = np.where(have, tri, -1).reshape(n, -1).max(axis=1)   # -1: no source
    earlier = have & (tri < seg_begin[:, None, None])
    out["cross"] = earlier.any(axis=(1, 2))
    out["cross_many"] = out["cross"] & (count >= 3)
    for r in rings:
        out[f"older{r}"] = (have & ~earlier & (back > r)).any(axis=(1, 2))
    out["far"] = (have & ((back > RING3_NEAR) | earlier)).any(axis=(1, 2))
    out["ring_edge"] = (have & ~earlier & (back > RING3_NEAR) & (back <= RING3)).any(axis=(1, 2))   # far by the margin of one tile only

    pred_bits = trace["pred"][:, comp]
    if is_float:
        val = values.astype(np.float32)
        a, b, o = val[tri[:, :, 0]], val[tri[:, :, 1]], val[tri[:, :, 2]]
        with np.errstate(all="ignore"):
            pv = (a + (b - o)).astype(np.float32)       # prediction.h:139-147
            avg = ((pv[:, 0].astype(np.float64) + pv[:, 1].astype(np.float64)) / 2.0).astype(np.float32)
            d0, d1 = np.abs(avg - pv[:, 0]).astype(np.float32), np.abs(avg - pv[:, 1]).astype(np.float32)
        out["float_tie"] = (count == 2) & (pv[:, 0] != pv[:, 1]) & (d0 == d1)
        out["clamp0"] = out["clamptop"] = out["chain_clamp"] = np.zeros(n, bool)
        vu = ordered_u32(values.view(np.uint32)).astype(np.int64)
        pu = ordered_u32(pred_bits.astype(np.uint32)).astype(np.int64)
        out["code"] = code_class(vu, pu, (1 << 32) - 1)
    else:
        val = values.astype(np.int64)
        s = val[tri[:, :, 0]] + val[tri[:, :, 1]] - val[tri[:, :, 2]]   # prediction.h:121-138 before it saturates
        hk = have[:, :, 0]
        out["clamp0"] = (hk & (s < 0)).any(axis=1)
        out["clamptop"] = (hk & (s > top)).any(axis=1)
        kp = np.where(out["chained"], pos // 3, 0)
        sc = s[v, kp]
        out["chain_clamp"] = out["chained"] & ((sc < 0) | (sc > top))
        out["code"] = code_class(val, pred_bits.astype(np.int64), top)
        out["float_tie"] = np.zeros(n, bool)
    out["near"], out["far_code"], out["raw"] = out["code"] == NEAR, out["code"] == FAR, out["code"] == RAW
    out["leaves"] = out["chained"] & (out["chain_clamp"] | (out["code"] != NEAR))
    return out


VERTEX_CLASSES = COUNT_CLASSES + ("chained", "constant", "cross", "cross_many", "older4096", "older8192", f"older{RING3_NEAR}", "ring_edge",
                                  "clamp0", "clamptop", "near", "far_code", "raw", "float_tie", "leaves")


def vertex_census(vc):
    cen = {name: int(vc[name].sum()) for name in VERTEX_CLASSES}
    g = vc["gap"][vc["chained"] | ((vc["count"] >= 1) & (vc["count"] <= 2))]
    for name, lo, hi in (("gap1_63", 1, 63), ("gap64_767", 64, 767), ("gap768p", 768, 65534), ("gap_none", 65535, 65535)):
        cen[name] = int(((g >= lo) & (g <= hi)).sum())
    return cen


def classify_tiles(vc, W):
    """per (component, 64-aligned tile) of a k_unpredict3 chain run by W wavefronts: dict of arrays over the tiles"""
    n = vc["n"]
    v = np.arange(n, dtype=np.int64)
    lane = v & 63
    nc, gap = vc["nc"], vc["gap"]
    settled = gap > lane + 64 * (W - 1)
    head = (nc == 3) | ((nc != 0) & ~settled)
    rowhead = head & ((nc == 3) | vc["far"])
    lo = np.maximum(vc["seg_begin"] - (v & ~np.int64(63)), 0)
    inner = (nc == 3) | ((nc != 0) & (gap <= lane - lo))
    key = vc["seg"] * (n // 64 + 2) + (v >> 6)
    first = np.ones(n, bool)
    first[1:] = key[1:] != key[:-1]
    tile = np.cumsum(first) - 1
    nt = int(tile[-1]) + 1 if n else 0
    cnt = lambda m: np.bincount(tile, weights=m, minlength=nt).astype(np.int64)
    nheads, nrow, ninner = cnt(head), cnt(rowhead), cnt(inner)
    prepared = (nheads <= MAX_HEADS) & (nrow <= 8)
    late = ~prepared & (ninner <= MAX_HEADS_LATE)
    dense = ~prepared & ~late
    # runs: between the heads of a prepared tile, between the inner vertices of a late one (a dense tile cuts its runs as it goes)
    cut = np.where(prepared[tile], head, np.where(late[tile], inner, True))
    prev_cut = np.zeros(n, bool)
    prev_cut[1:] = cut[:-1]
    run = np.cumsum(first | cut | prev_cut) - 1
    nr = int(run[-1]) + 1 if n else 0
    in_run = ~cut
    leaving = np.bincount(run, weights=in_run & vc["leaves"], minlength=nr)
    run_tile = np.zeros(nr, np.int64)
    run_tile[run] = tile
    one, more = np.zeros(nt, bool), np.zeros(nt, bool)
    one[run_tile[leaving == 1]] = True
    more[run_tile[leaving >= 2]] = True
    # the longest stretch of chained two-candidate vertices inside a run
    f = in_run & vc["chained"] & (vc["count"] == 2)
    brk = ~f | first | prev_cut
    stretch = np.cumsum(brk) - 1
    length = np.bincount(stretch, weights=f, minlength=int(stretch[-1]) + 1 if n else 0)
    longest = np.zeros(nt, np.int64)
    np.maximum.at(longest, tile, length[stretch].astype(np.int64))
    return {"nheads": nheads, "nrow": nrow, "ninner": ninner, "prepared": prepared, "late": late, "dense": dense,
            "heads0": nheads == 0, "heads1": nheads == 1, "heads2_8": (nheads >= 2) & (nheads <= 8),
            "heads9_12": (nheads >= 9) & (nheads <= 12), "heads13p": nheads > 12, "rowheads9p": nrow > 8,
            "run_leaves0": ~one & ~more & ~dense, "run_leaves1": one, "run_leaves2p": more, "stretch17p": longest >= 17, "longest": longest}


TILE_CLASSES = ("heads0", "heads1", "heads2_8", "heads9_12", "heads13p", "rowheads9p", "late", "dense",
                "run_leaves0", "run_leaves1", "run_leaves2p", "stretch17p")


def tile_census(vc, W):
    tc = classify_tiles(vc, W)
    return {name: int(tc[name].sum()) for name in TILE_CLASSES}
