"""Meshes from device buffers (hry_mesh_from_device, Codec.mesh_from_tensors) against the host constructor: configs[1] (the bench's
1 002 528-triangle torus, float32 xyz) as cuda tensors.  Prints ONE JSON line with, per form of the mesh, medians over the repeats:
  indexed  positions [nv, 3] + int32 triangles [T, 3]:
           ingest_ms (HIP events on the codec's stream around the call) and its wall time, against Mesh.from_arrays + Codec.upload from
           numpy arrays already on the host (host_ms; to_numpy_ms: what bringing the tensors down first costs on top)
  soup     the same triangles as three rows each (3 007 584 rows), welded on the device (weld=True): ingest_ms against the host
           constructor + upload of the unwelded soup (the host path has no weld)
and the chunked encode (-l1 -q14) after either path (encode_ms; the soup: after the ingest only), with the check that both paths give
the same container.  Warm-up runs
first.  Nothing is gated on these numbers.

--obj: a textured scene instead (hry_mesh_from_device_corners, Codec.corner_mesh_from_tensors): og.scene(mg.torus(200, 200, seed=2),
normals="smooth", tex="atlas", charts=7) -- 40 000 vertices, 80 000 triangles, a texture and a normal index per corner -- built from
tensors that hold the reader's own arrays, unwelded (same_container: the chunked container equals the reader's mesh's) and welded
(every list on its own; records: what is left of every list), against Mesh.from_obj of the text + Codec.upload on the host (host_ms; obj_bytes: the size of the text)."""
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
from harry_amd import objgen as og  # noqa: E402

QUANT = [(1, -1, 14)]


def timed(cx, fn):
    """(result, event ms on the codec's stream, wall ms) of fn(); the call synchronises itself"""
    st = torch.cuda.ExternalStream(cx.stream(), device=torch.device("cuda", cx.device))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record(st)
    out = fn()
    b.record(st)
    b.synchronize()
    return out, a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def encode_ms(cx, mesh):
    cx.requant(mesh, QUANT)
    t0 = time.perf_counter()
    data = cx.write_hry(mesh, profile=hc.PROFILE_CHUNKED)
    return data, (time.perf_counter() - t0) * 1e3


def measure(cx, to_device, to_host, warmup, repeats, encode_host=True):
    """to_device(): mesh from the tensors; to_host(): mesh from numpy (timed with its upload); encode_host: also encode that one"""
    rows = []
    for i in range(warmup + repeats):
        dmesh, ev, wall = timed(cx, to_device)
        d_data, d_enc = encode_ms(cx, dmesh)
        t0 = time.perf_counter()
        hmesh = to_host()
        cx.upload(hmesh)
        host_ms = (time.perf_counter() - t0) * 1e3
        h_data, h_enc = encode_ms(cx, hmesh) if encode_host else (None, 0.0)
        if i >= warmup:
            rows.append({"ingest_ms": ev, "ingest_wall_ms": wall, "host_ms": host_ms, "encode_ms_after_ingest": d_enc,
                         "encode_ms_after_host": h_enc, "same_container": d_data == h_data, "nv": dmesh.nv, "nf": dmesh.nf})
    out = {k: statistics.median(r[k] for r in rows) for k in ("ingest_ms", "ingest_wall_ms", "host_ms", "encode_ms_after_ingest", "encode_ms_after_host")}
    out["ingest_ms_min"] = min(r["ingest_ms"] for r in rows)
    out.update({k: rows[-1][k] for k in ("nv", "nf")})
    out["same_container"] = all(r["same_container"] for r in rows) if encode_host else None
    return out


def obj_mode(args, dev):
    sc = og.scene(mg.torus(200, 200, seed=2), normals="smooth", tex="atlas", charts=7)
    ref = hc.Mesh.from_obj(sc.obj, "")
    cattr = ref.bindings(2)
    rows = [torch.from_numpy(ref.list_data(l).view(np.float32).copy()).to(dev) for l in range(3)]
    idx = [torch.from_numpy(a.astype(np.int32).reshape(-1, 3)).to(dev) for a in (ref.org(), cattr[:, 0], cattr[:, 1])]
    torch.cuda.synchronize()
    cx = hc.Codec(0)

    def device(weld):
        return cx.corner_mesh_from_tensors(rows[0], idx[0], uv=rows[1], uv_idx=idx[1], normals=rows[2], normal_idx=idx[2], weld=weld)
    try:
        want = cx.write_hry(ref, profile=hc.PROFILE_CHUNKED)
        out = {"nv": ref.nv, "nf": ref.nf, "obj_bytes": len(sc.obj), "repeats": args.repeats}
        for name, weld in (("unwelded", False), ("welded", True)):
            ev, wall = [], []
            for i in range(args.warmup + args.repeats):
                mesh, e, w = timed(cx, lambda: device(weld))
                if i >= args.warmup:
                    ev.append(e); wall.append(w)
            out[name] = {"ingest_ms": statistics.median(ev), "ingest_wall_ms": statistics.median(wall), "ingest_ms_min": min(ev),
                         "records": [mesh.list_count(l) for l in range(3)]}
            if not weld:   # (the weld merges what the six-digit text made equal: another mesh, checked by its decode only)
                out[name]["same_container"] = cx.write_hry(mesh, profile=hc.PROFILE_CHUNKED) == want
            else:
                back = cx.read_hry(cx.write_hry(mesh, profile=hc.PROFILE_CHUNKED))
                out[name]["decodes"] = (back.nv, back.nf, back.ne) == (mesh.nv, mesh.nf, mesh.ne)
        host = []
        for i in range(args.warmup + args.repeats):
            t0 = time.perf_counter()
            cx.upload(hc.Mesh.from_obj(sc.obj, ""))
            if i >= args.warmup:
                host.append((time.perf_counter() - t0) * 1e3)
        out["host_ms"] = statistics.median(host)
    finally:
        cx.close()
    print(json.dumps({"obj_scene_torus200": out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--obj", action="store_true", help="the textured scene through hry_mesh_from_device_corners instead")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.obj:
        return obj_mode(args, dev)
    m = mg.cfg2_torus_1m()
    pos_np = np.ascontiguousarray(np.stack([m.verts[k] for k in "xyz"], axis=1))
    tri_np = m.indices.reshape(-1, 3)
    pos, tri = torch.from_numpy(pos_np).to(dev), torch.from_numpy(tri_np.astype(np.int32)).to(dev)
    soup_pos = pos[tri.reshape(-1).long()].contiguous()
    soup_idx = torch.arange(soup_pos.shape[0], dtype=torch.int32, device=dev).reshape(-1, 3)
    torch.cuda.synchronize()
    cx = hc.Codec(0)
    try:
        t0 = time.perf_counter()
        _ = (pos.cpu().numpy(), tri.cpu().numpy())
        to_numpy_ms = (time.perf_counter() - t0) * 1e3
        indexed = measure(cx, lambda: cx.mesh_from_tensors(tri, [("x y z", pos)]),
                          lambda: hc.Mesh.from_arrays(m.verts, m.degrees, m.indices), args.warmup, args.repeats)
        indexed["to_numpy_ms"] = to_numpy_ms
        soup_np = pos_np[tri_np.reshape(-1)]
        soup_verts = np.zeros(len(soup_np), m.verts.dtype)
        for j, k in enumerate("xyz"):
            soup_verts[k] = soup_np[:, j]
        soup_deg, soup_flat = np.full(m.nf, 3, np.uint8), np.arange(3 * m.nf, dtype=np.uint32)
        soup = measure(cx, lambda: cx.mesh_from_tensors(soup_idx, [("x y z", soup_pos)], weld=True),
                       lambda: hc.Mesh.from_arrays(soup_verts, soup_deg, soup_flat), args.warmup, args.repeats, encode_host=False)
        del soup["encode_ms_after_host"]   # (the host path has no weld: its soup is a million one-triangle components, not this mesh)
        soup["rows"] = int(soup_pos.shape[0])
    finally:
        cx.close()
    print(json.dumps({"configs1_indexed": indexed, "configs1_soup_weld": soup}))


if __name__ == "__main__":
    main()
