"""The rate sweep (hry_rate_sweep_build, Codec.rate_sweep) on configs[1]: the bench's 1 002 528-triangle torus, float32 xyz, against the
loop it replaces, in the same process.  Prints ONE JSON line (one per run with --runs N):
  sweep   Codec.rate_sweep(src) of the resident mesh, medians over --repeats (10) after --warmup (3): device_ms = the kernel (HIP
          events inside the build, hry_rate_sweep_stat), walk_ms = the host's walk, wall_ms = the Python call
  loop    per width 1 .. 30: a clone, Codec.requant of the clone's list 1 to that width, Codec.write_hry (chunked) and the size;
          wall_ms of the thirty together, medians over --loop-repeats (2)
  table   per width: the estimate (the three components' bytes()) next to the real payload bytes (hry_timing.payload_bytes) and file
          sizes of the chunked and the compat profile; agrees: every histogram equals np.bincount of the encoder's "vplanes" stage
Nothing is gated on these numbers."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from harry_amd import codec as hc  # noqa: E402
from harry_amd import meshgen as mg  # noqa: E402


def loop(cx, src):
    t0 = time.perf_counter()
    sizes = []
    for q in range(1, 31):
        clone = src.clone()
        cx.requant(clone, [(1, -1, q)])
        sizes.append(len(cx.write_hry(clone, profile=hc.PROFILE_CHUNKED)))
    return sizes, (time.perf_counter() - t0) * 1e3


def real_sizes(cx, src, s, ncomp):
    """per width: file and payload bytes in both profiles, and whether the sweep's histograms are the encoder's planes"""
    rows, agrees = [], True
    for q in range(1, 31):
        clone = src.clone()
        cx.requant(clone, [(1, -1, q)])
        row = {"bits": q, "estimate": sum(s.bytes(1, c, q) for c in range(ncomp))}
        for name, profile in (("chunked", hc.PROFILE_CHUNKED), ("compat", hc.PROFILE_COMPAT)):
            data = cx.write_hry(clone, profile=profile, keep_stages=name == "compat")
            row[name + "_file"], row[name + "_payload"] = len(data), cx.timing()["payload_bytes"]
        per = 1 if q <= 8 else 2 if q <= 16 else 4
        planes = cx.stage("vplanes").reshape(ncomp * per, -1)
        for c in range(ncomp):
            want = np.stack([np.bincount(planes[c * per + b], minlength=256) for b in range(per)])
            agrees = agrees and np.array_equal(s.hist(1, c, q), want)
        rows.append(row)
    return rows, bool(agrees)


def one_run(cx, src, args):
    ncomp = len(src.list_fmt(1))
    cx.upload(src)
    dev_ms, walk_ms, wall = [], [], []
    for i in range(args.warmup + args.repeats):
        t0 = time.perf_counter()
        s = cx.rate_sweep(src)
        w = (time.perf_counter() - t0) * 1e3
        st = s.stat()
        if i >= args.warmup:
            dev_ms.append(st["device_ms"]); walk_ms.append(st["walk_ms"]); wall.append(w)
        if i + 1 < args.warmup + args.repeats:
            s.close()
    assert cx.resident(src) and st["uploaded_bytes"] == 0
    out = {"sweep": {"device_ms": statistics.median(dev_ms), "device_ms_min": min(dev_ms), "walk_ms": statistics.median(walk_ms), "wall_ms": statistics.median(wall),
                     "coded": s.coded, "rows": sum(s.bits(1, c) + 1 for c in range(ncomp))}}
    if args.sweep_only:
        s.close()
        return out
    walls = []
    for _ in range(args.loop_repeats):
        _, w = loop(cx, src)
        walls.append(w)
    out["loop"] = {"wall_ms": statistics.median(walls), "wall_ms_min": min(walls)}
    out["table"], out["agrees"] = real_sizes(cx, src, s, ncomp)
    s.close()
    out.update({"nv": src.nv, "nf": src.nf, "ncomp": ncomp, "repeats": args.repeats, "loop_over_sweep_wall": out["loop"]["wall_ms"] / out["sweep"]["wall_ms"]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--loop-repeats", type=int, default=2)
    ap.add_argument("--runs", type=int, default=1)
    ap.add_argument("--sweep-only", action="store_true", help="the sweep's times alone (launch-shape comparisons)")
    args = ap.parse_args()
    gen = mg.cfg2_torus_1m()
    cx = hc.Codec(0)
    try:
        src = hc.Mesh.from_arrays(gen.verts, gen.degrees, gen.indices)
        cx.bounds(src)
        for run in range(args.runs):
            print(json.dumps({"configs1_rate_sweep": dict(one_run(cx, src, args), run=run)}), flush=True)
    finally:
        cx.close()


if __name__ == "__main__":
    main()
