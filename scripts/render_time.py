"""Render-ready buffers (hry_render_build) after a decode: configs[1] (1 002 528 triangles, -l1 -q14, chunked container) and the
bench's 80 000-triangle OBJ scene.  Prints ONE JSON line: per workload the decode's wall time, the render kernels' device_ms (HIP
events), the wall time of hry_render_build plus the copies of every buffer (device to device, into preallocated device memory) and
the bytes the build uploaded.  Each measurement follows a fresh decode (residency holds for the mesh the decode just returned);
warm-up runs first, then medians over the repeats.

--normals: configs[1] only, through Codec.render: the render kernels' device_ms without normals, with area-weighted vertex normals,
with face normals too and with angle weights (hry_render_build_ex), beside a plain torch restatement on the same tensors (float32
fan cross products, index_add_, normalise; torch.cuda events) and the largest component difference between the two results."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from harry_amd import _native as nat  # noqa: E402
from harry_amd import codec as hc  # noqa: E402
from harry_amd import meshgen as mg  # noqa: E402
from harry_amd import objgen as og  # noqa: E402

NAMES = ("indices", "tri_face", "vertex_source", "corner_source", "face_region") + tuple(f"list{l}" for l in range(16))


def one(cx, data, dst):
    L = nat.load()
    t0 = time.perf_counter()
    mesh = cx.read_hry(data)
    t1 = time.perf_counter()
    r = C.c_void_p()
    nat.check(L.hry_render_build(cx.h, mesh.h, C.byref(r)))
    try:
        for name in NAMES:
            rows, width, typ = C.c_uint64(), C.c_int(), C.c_int()
            nat.check(L.hry_render_get(r, name.encode(), None, C.byref(rows), C.byref(width), C.byref(typ)))
            if rows.value:
                nat.check(L.hry_render_copy(cx.h, r, name.encode(), dst, 1))
        t2 = time.perf_counter()
        d, up = C.c_double(), C.c_uint64()
        nat.check(L.hry_render_stat(r, C.byref(d), C.byref(up)))
        return {"decode_ms": (t1 - t0) * 1e3, "render_wall_ms": (t2 - t1) * 1e3, "device_ms": d.value, "uploaded_bytes": up.value,
                "nverts": L.hry_render_nverts(r), "ntris": L.hry_render_ntris(r)}
    finally:
        L.hry_render_free(r)


def measure(cx, data, warmup, repeats, dst):
    for _ in range(warmup):
        one(cx, data, dst)
    runs = [one(cx, data, dst) for _ in range(repeats)]
    out = {k: statistics.median(r[k] for r in runs) for k in ("decode_ms", "render_wall_ms", "device_ms")}
    out["device_ms_min"] = min(r["device_ms"] for r in runs)
    out.update({k: runs[-1][k] for k in ("uploaded_bytes", "nverts", "ntris")})
    return out


def normals_report(warmup, repeats):
    import torch
    torch.cuda.init()   # torch holds the device before the codec starts
    cx = hc.Codec(0)
    try:
        m = hc.Mesh.from_ply(mg.torus(708, 708, seed=2, sigma=1e-4).to_ply())
        cx.requant(m, [(1, -1, 14)])
        cfg1 = cx.write_hry(m, profile=hc.PROFILE_CHUNKED)
        res, got = {}, None
        for key, kw in (("plain", {}), ("area", {"normals": "area"}), ("area_and_faces", {"normals": "area", "face_normals": True}),
                        ("angle", {"normals": "angle"})):
            ms = []
            for i in range(warmup + repeats):
                out = cx.render(cx.read_hry(cfg1), **kw)   # (a fresh decode each time: resident)
                assert cx.render_stat()["uploaded_bytes"] == 0
                if i >= warmup:
                    ms.append(cx.render_stat()["device_ms"])
                if key == "area":
                    got = out
            res["device_ms_" + key] = statistics.median(ms)
        res["ntris"] = cx.render_stat()["ntris"]

        P, idx = got["list1"][:, :3].contiguous(), got["indices"].long()

        def restated():
            p0 = P[idx[:, 0]]
            n = torch.cross(P[idx[:, 1]] - p0, P[idx[:, 2]] - p0, dim=1)
            s = torch.zeros_like(P)
            for k in range(3):
                s.index_add_(0, idx[:, k], n)
            return torch.nn.functional.normalize(s, dim=1)

        ms = []
        for i in range(warmup + repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ref = restated()
            b.record()
            b.synchronize()
            if i >= warmup:
                ms.append(a.elapsed_time(b))
        res["torch_index_add_ms"] = statistics.median(ms)
        res["largest_difference"] = float((ref - got["normals"]).abs().max())
        return res
    finally:
        cx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--normals", action="store_true", help="configs[1]: device_ms with and without normals, against a torch index_add_ pass")
    args = ap.parse_args()
    if args.normals:
        print(json.dumps({"configs1_normals": normals_report(args.warmup, args.repeats)}))
        return
    cx = hc.Codec(0)
    m = hc.Mesh.from_ply(mg.torus(708, 708, seed=2, sigma=1e-4).to_ply())
    cx.requant(m, [(1, -1, 14)])
    cfg1 = cx.write_hry(m, profile=hc.PROFILE_CHUNKED)
    sc = og.scene(mg.torus(200, 200, seed=2), normals="smooth", tex="atlas", charts=7)
    scene = cx.write_hry(hc.Mesh.from_obj(sc.obj, ""), profile=hc.PROFILE_CHUNKED)
    dst = C.c_void_p()
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipMalloc(C.byref(dst), C.c_size_t(64 << 20)) == 0   # the largest buffer of either workload fits
    try:
        res = {"configs1": measure(cx, cfg1, args.warmup, args.repeats, dst), "obj_scene_80k": measure(cx, scene, args.warmup, args.repeats, dst)}
    finally:
        hip.hipFree(dst)
        cx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
