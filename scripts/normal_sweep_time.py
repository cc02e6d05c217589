"""The normal deviation at every width (hry_quant_sweep_build_ex with HRY_SWEEP_NORMALS, Codec.quant_sweep(normals=True)) on
configs[1]: the bench's 1 002 528-triangle torus, float32 xyz, against the loop it replaces, in the same process.  Prints ONE JSON
line (one per run with --runs N):
  sweep   Codec.quant_sweep(src, normals=True) of the resident mesh, medians over --repeats (20) after --warmup (5): device_ms = all
          kernels of the build (HIP events inside it, hry_quant_sweep_stat), plain_device_ms = the same build without the flag, so
          normals_device_ms = their difference is k_normal_sweep and its fold; wall_ms = the Python call
  loop    per width 1 .. 30: a clone, Codec.requant of the three position components to that width, Codec.requant(clear), a render
          build with face normals, and in torch the chord against the source's face normals, its maximum and the sum of its squares;
          wall_ms of the thirty together, medians over --loop-repeats (3).  The render build's face normals are floats made from float
          positions, so the loop's numbers are not the table's bits: agrees says every max_chord is within 1e-5 of the sweep's on the
          faces both compare
Nothing is gated on these numbers."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402  (before the library, as in scripts/distortion_time.py: the loop's reductions run in torch)

from harry_amd import codec as hc  # noqa: E402
from harry_amd import meshgen as mg  # noqa: E402


def loop(cx, src, n_src):
    t0 = time.perf_counter()
    out = []
    for q in range(1, 31):
        clone = src.clone()
        cx.requant(clone, [(1, c, q) for c in range(3)])
        cx.requant(clone, [], clear=True)
        n = cx.render(clone, face_normals=True)["face_normals"]
        ok = (n_src.abs().sum(1) > 0) & (n.abs().sum(1) > 0)
        d = (n.double() - n_src.double())[ok]
        c2 = (d * d).sum(1)
        out.append((float(c2.max().sqrt()) if len(c2) else 0.0, float(c2.sum()), int(ok.sum())))
    return out, (time.perf_counter() - t0) * 1e3


def one_run(cx, src, args):
    cx.upload(src)
    times = {True: ([], []), False: ([], [])}
    s = None
    for normals in (False, True):
        for i in range(args.warmup + args.repeats):
            if s is not None:
                s.close()
            t0 = time.perf_counter()
            s = cx.quant_sweep(src, normals=normals)
            w = (time.perf_counter() - t0) * 1e3
            st = s.stat()
            if i >= args.warmup:
                times[normals][0].append(st["device_ms"]); times[normals][1].append(w)
    assert cx.resident(src) and st["uploaded_bytes"] == 0 and s.normals(30)["list"] == 1
    med = statistics.median
    out = {"sweep": {"device_ms": med(times[True][0]), "device_ms_min": min(times[True][0]), "plain_device_ms": med(times[False][0]),
                     "normals_device_ms": med(times[True][0]) - med(times[False][0]), "wall_ms": med(times[True][1]), "plain_wall_ms": med(times[False][1])}}
    n_src = cx.render(src, face_normals=True)["face_normals"]
    walls, agrees = [], True
    for _ in range(args.loop_repeats):
        table, w = loop(cx, src, n_src)
        walls.append(w)
        for q in range(1, 31):
            r = s.normals(q)
            agrees = agrees and (r["compared"] != table[q - 1][2] or abs(r["max_chord"] - table[q - 1][0]) <= 1e-5)
    out["table"] = {q: {k: s.normals(q)[k] for k in ("max_angle_deg", "rms_angle_deg", "collapsed")} for q in (4, 8, 12, 16, 20, 24)}
    s.close()
    out.update({"nv": src.nv, "nf": src.nf, "repeats": args.repeats})
    if walls:   # (--loop-repeats 0: the sweep alone)
        out["loop"] = {"wall_ms": med(walls), "wall_ms_min": min(walls), "agrees": agrees}
        out["loop_over_sweep_wall"] = out["loop"]["wall_ms"] / out["sweep"]["wall_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--loop-repeats", type=int, default=3)
    ap.add_argument("--runs", type=int, default=1)
    args = ap.parse_args()
    gen = mg.cfg2_torus_1m()
    torch.cuda.synchronize()
    cx = hc.Codec(0)
    try:
        src = hc.Mesh.from_arrays(gen.verts, gen.degrees, gen.indices)
        cx.bounds(src)
        for run in range(args.runs):
            print(json.dumps({"configs1_normal_sweep": dict(one_run(cx, src, args), run=run)}), flush=True)
    finally:
        cx.close()


if __name__ == "__main__":
    main()
