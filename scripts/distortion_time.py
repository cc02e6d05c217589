"""Per-component error of a decode (hry_distortion_build, Codec.distortion) on configs[1]: the bench's 1 002 528-triangle torus, float32
xyz, -l1 -q14, chunked profile.  The decode is resident (what read_hry left in HBM), the maps are the encode's handle, the source goes
up from the host.  Prints ONE JSON line per run (--runs, default 2) with medians over --repeats (20) after --warmup (5):
  build / build_rows   Codec.distortion(src, dec, order) without and with rows=True: device_ms = the two kernels (HIP events inside the
                       build, hry_distortion_stat), call_ms = HIP events on the codec's stream around the whole call (with the source's
                       upload and the results' way down), wall_ms = the Python call; bytes = what the kernels read and write (the
                       records of both sides, the map, the per-row buffer), gbs and hbm_fraction (of 8 TB/s, MI355X peak) from device_ms
  torch                the same statistics from torch on the same device tensors: index_select through the map, dequantisation by
                       arithmetic on tensors, then abs().max(), argmax and square().sum() per component (events on torch's stream);
                       agrees: its maxima and arg-maxima are the build's
Nothing is gated on these numbers."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from harry_amd import codec as hc  # noqa: E402
from harry_amd import meshgen as mg  # noqa: E402

BITS = 14
QUANT = [(1, -1, BITS)]
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


def one_run(cx, src, dec, order, args, dev):
    ours = torch.cuda.ExternalStream(cx.stream(), device=dev)
    theirs = torch.cuda.current_stream(dev)
    nv, out = src.nv, {}
    for key, rows in (("build", False), ("build_rows", True)):
        dev_ms, call, wall, up = [], [], [], 0
        for i in range(args.warmup + args.repeats):
            d, c, w = events_ms(ours, lambda: cx.distortion(src, dec, order, rows=rows))
            st = d.stat()
            if i >= args.warmup:
                dev_ms.append(st["device_ms"]); call.append(c); wall.append(w)
            up = st["uploaded_bytes"]
            if not rows:
                built = [d.component(1, c) for c in range(3)]
            d.close()
        moved = nv * 12 * 2 + nv * 4 + (nv * 4 if rows else 0)
        e = statistics.median(dev_ms)
        out[key] = {"device_ms": e, "device_ms_min": min(dev_ms), "call_ms": statistics.median(call), "wall_ms": statistics.median(wall),
                    "uploaded_bytes": up, "bytes": moved, "gbs": moved / e / 1e6, "hbm_fraction": moved / e / 1e6 / HBM_PEAK_GBS}

    # the same on torch, from tensors that are on the device already
    x = torch.from_numpy(np.stack([src.component(1, c) for c in range(3)], axis=1)).to(dev)                      # float32 [nv, 3]
    q = torch.from_numpy(np.stack([dec.component(1, c).astype(np.int32) for c in range(3)], axis=1)).to(dev)     # the quantised integers
    lo = np.frombuffer(dec.list_min(1).tobytes(), np.float32)
    hi = np.frombuffer(dec.list_max(1).tobytes(), np.float32)
    mn = torch.from_numpy(lo.copy()).to(dev)
    scale = torch.tensor(float((hi - lo).max()), dtype=torch.float32, device=dev)   # one extent over the interpretation group
    steps = torch.tensor(float(2 ** BITS - 1), dtype=torch.float32, device=dev)
    vmap = order.tensor("vertex")

    def baseline():
        y = q.index_select(0, vmap).to(torch.float32) / steps * scale + mn
        res = []
        for c in range(3):
            e = y[:, c].to(torch.float64) - x[:, c].to(torch.float64)
            mag = e.abs()
            res.append((mag.max(), mag.argmax(), e.square().sum()))
        return res
    ms = []
    for i in range(args.warmup + args.repeats):
        res, t, _ = events_ms(theirs, baseline)
        if i >= args.warmup:
            ms.append(t)
    # (torch's argmax may name any row of an equal maximum: the build's is the lowest)
    agrees = all(float(r[0]) == b["max_abs"] and int(r[1]) >= b["argmax"] for r, b in zip(res, built))
    out["torch"] = {"ms": statistics.median(ms), "ms_min": min(ms), "agrees": agrees}
    out.update({"nv": nv, "nf": src.nf, "repeats": args.repeats})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--runs", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    gen = mg.cfg2_torus_1m()
    cx = hc.Codec(0)
    try:
        src = hc.Mesh.from_arrays(gen.verts, gen.degrees, gen.indices)
        enc = src.clone()
        cx.requant(enc, QUANT)
        data, order = cx.write_hry(enc, profile=hc.PROFILE_CHUNKED, return_order=True)
        dec = cx.read_hry(data)   # (nothing else touches the context from here on: the decode stays resident)
        for run in range(args.runs):
            print(json.dumps({"configs1_distortion": dict(one_run(cx, src, dec, order, args, dev), run=run)}), flush=True)
        order.close()
    finally:
        cx.close()


if __name__ == "__main__":
    main()
