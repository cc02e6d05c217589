"""Numbering maps of an encode (hry_order_take, Codec.write_hry(..., return_order=True)) on configs[1]: the bench's 1 002 528-triangle
torus, float32 xyz, -l1 -q14, resident in HBM.  Prints ONE JSON line per run (--runs, default 2) with medians over --repeats (10):
  encode_ms / encode_order_ms   the chunked encode without and with HRY_FLAG_ORDER, alternating in one process (wall clock around
                                write_hry, the maps taken and freed inside the timed call); flag_ms: the difference of the medians;
                                same_container: the flag changes no byte.  encode_ms is bench.py's encode of the same workload: compare
                                it with bench.py's line on the parent commit
  rows3 / rows256               Order.to_decoded of a [nv, 3] and a [nv, 256] float32 tensor (HIP events on the codec's stream around
                                hry_order_apply; wall_ms: the Python call with its two synchronisations) against torch's own
                                index_select with Order.tensor("vertex_inv") (events on torch's stream); gbs: bytes read + written
                                (2 x nv x row bytes + the map) per second of the event time, hbm_fraction: of 8 TB/s (MI355X peak)
Warm-up runs first.  Nothing is gated on these numbers."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from harry_amd import codec as hc  # noqa: E402
from harry_amd import meshgen as mg  # noqa: E402

QUANT = [(1, -1, 14)]
HBM_PEAK_GBS = 8000.0


def events_ms(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record(stream)
    out = fn()
    b.record(stream)
    b.synchronize()
    return out, a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def one_run(cx, mesh, args, dev):
    plain, flagged, same = [], [], True
    for i in range(args.warmup + args.repeats):
        t0 = time.perf_counter()
        a = cx.write_hry(mesh, profile=hc.PROFILE_CHUNKED, as_buffer=True)
        t1 = time.perf_counter()
        b, order = cx.write_hry(mesh, profile=hc.PROFILE_CHUNKED, as_buffer=True, return_order=True)
        order.close()
        t2 = time.perf_counter()
        same = same and a == b
        if i >= args.warmup:
            plain.append((t1 - t0) * 1e3)
            flagged.append((t2 - t1) * 1e3)
    out = {"encode_ms": statistics.median(plain), "encode_order_ms": statistics.median(flagged), "same_container": same,
           "encode_ms_min": min(plain), "encode_order_ms_min": min(flagged)}
    out["flag_ms"] = out["encode_order_ms"] - out["encode_ms"]

    _, order = cx.write_hry(mesh, profile=hc.PROFILE_CHUNKED, return_order=True)
    inv = order.tensor("vertex_inv").clamp(min=0)   # (this mesh has no filler rows; an index torch may not see is none either way)
    ours = torch.cuda.ExternalStream(cx.stream(), device=dev)
    theirs = torch.cuda.current_stream(dev)
    nv = mesh.nv
    for width in (3, 256):
        t = torch.rand(nv, width, dtype=torch.float32, device=dev)
        dst = torch.empty_like(t)
        ev, wall, sel = [], [], []
        for i in range(args.warmup + args.repeats):
            got, e, w = events_ms(ours, lambda: order.to_decoded(t, "vertex", out=dst))
            want, s, _ = events_ms(theirs, lambda: t.index_select(0, inv))
            if i >= args.warmup:
                ev.append(e); wall.append(w); sel.append(s)
        moved = 2 * nv * width * 4 + nv * 4
        e = statistics.median(ev)
        out[f"rows{width}"] = {"apply_ms": e, "apply_ms_min": min(ev), "wall_ms": statistics.median(wall), "index_select_ms": statistics.median(sel),
                               "gbs": moved / e / 1e6, "hbm_fraction": moved / e / 1e6 / HBM_PEAK_GBS, "equal": bool(torch.equal(got, want))}
        del t, dst
    order.close()
    out.update({"nv": nv, "nf": mesh.nf, "repeats": args.repeats})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--runs", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    gen = mg.cfg2_torus_1m()
    cx = hc.Codec(0)
    try:
        mesh = hc.Mesh.from_arrays(gen.verts, gen.degrees, gen.indices)
        cx.requant(mesh, QUANT)
        cx.upload(mesh)
        for run in range(args.runs):
            print(json.dumps({"configs1_order": dict(one_run(cx, mesh, args, dev), run=run)}), flush=True)
    finally:
        cx.close()


if __name__ == "__main__":
    main()
