"""The quantisation sweep (hry_quant_sweep_build, Codec.quant_sweep) on configs[1]: the bench's 1 002 528-triangle torus, float32 xyz,
against the loop it replaces, in the same process.  Prints ONE JSON line (one per run with --runs N):
  sweep   Codec.quant_sweep(src) of the resident mesh, medians over --repeats (20) after --warmup (5): device_ms = the two kernels (HIP
          events inside the build, hry_quant_sweep_stat), wall_ms = the Python call; widths = (component, width) records of list 1
          and the positions' records
  loop    per width 1 .. 30: a clone, Codec.requant of the clone's list 1 to that width (one pass over the records and the copy down)
          and Codec.distortion(src, clone), its records read back; wall_ms of the thirty together, medians over --loop-repeats (3);
          agrees: every exact field of every record is the sweep's
Nothing is gated on these numbers."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from harry_amd import codec as hc  # noqa: E402
from harry_amd import meshgen as mg  # noqa: E402

EXACT = ("max_abs", "a_min", "a_max", "compared", "skipped", "nonfinite", "changed", "argmax")


def loop(cx, src, ncomp):
    t0 = time.perf_counter()
    table, pos = [], []
    for q in range(1, 31):
        clone = src.clone()
        cx.requant(clone, [(1, -1, q)])
        d = cx.distortion(src, clone)
        table.append([d.component(1, c) for c in range(ncomp)])
        pos.append(d.position())
        d.close()
    return table, pos, (time.perf_counter() - t0) * 1e3


def one_run(cx, src, args):
    ncomp = len(src.list_fmt(1))
    cx.upload(src)
    dev_ms, wall = [], []
    for i in range(args.warmup + args.repeats):
        t0 = time.perf_counter()
        s = cx.quant_sweep(src)
        w = (time.perf_counter() - t0) * 1e3
        st = s.stat()
        if i >= args.warmup:
            dev_ms.append(st["device_ms"]); wall.append(w)
        if i + 1 < args.warmup + args.repeats:
            s.close()
    assert cx.resident(src) and st["uploaded_bytes"] == 0
    widths = sum(s.bits(1, c) for c in range(ncomp)) + 30
    out = {"sweep": {"device_ms": statistics.median(dev_ms), "device_ms_min": min(dev_ms), "wall_ms": statistics.median(wall), "widths": widths}}
    walls, agrees = [], True
    for _ in range(args.loop_repeats):
        table, pos, w = loop(cx, src, ncomp)
        walls.append(w)
        for q in range(1, 31):
            for c in range(ncomp):
                got = s.component(1, c, q)
                agrees = agrees and all(got[k] == table[q - 1][c][k] for k in EXACT)
            agrees = agrees and all(s.position(q)[k] == pos[q - 1][k] for k in ("max_dist", "compared", "argmax", "list"))
    s.close()
    out["loop"] = {"wall_ms": statistics.median(walls), "wall_ms_min": min(walls), "agrees": agrees}
    out.update({"nv": src.nv, "nf": src.nf, "ncomp": ncomp, "repeats": args.repeats, "loop_over_sweep_wall": out["loop"]["wall_ms"] / out["sweep"]["wall_ms"]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--loop-repeats", type=int, default=3)
    ap.add_argument("--runs", type=int, default=1)
    args = ap.parse_args()
    gen = mg.cfg2_torus_1m()
    cx = hc.Codec(0)
    try:
        src = hc.Mesh.from_arrays(gen.verts, gen.degrees, gen.indices)
        cx.bounds(src)
        for run in range(args.runs):
            print(json.dumps({"configs1_quant_sweep": dict(one_run(cx, src, args), run=run)}), flush=True)
    finally:
        cx.close()


if __name__ == "__main__":
    main()
