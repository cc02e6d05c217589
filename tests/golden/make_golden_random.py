#!/usr/bin/env python3
"""Record the UNMODIFIED reference binary's answers on the seeded random inputs of tests/util.py (random_ply_case,
random_scene_cases) into tests/golden/random.json: size + sha256 of every input and of the .hry the reference writes from it.
The tests compare the CPU oracle with these answers, so they run where the reference binary is not built.

Run in the build container only (needs oracle/_ref/harry_ref, built by `make -C oracle ref`):

    python tests/golden/make_golden_random.py
"""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import util  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "harry_ref")
PLY_SEEDS = 4


def sha(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


def encode(src: str, flags) -> bytes:
    out = os.path.join(os.path.dirname(src), "out.hry")
    r = subprocess.run([REF, src, out] + flags, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"reference failed: {src} {flags}: {r.stderr[-400:]}")
    with open(out, "rb") as f:
        data = f.read()
    os.remove(out)
    return data


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -C oracle ref")
    rec = {"note": "reference .hry of the seeded inputs of tests/util.py: random_ply_case(seed), random_scene_cases()",
           "ply": {}, "scenes": []}
    with tempfile.TemporaryDirectory() as tmp:
        for seed in range(PLY_SEEDS):
            ply, variants = util.random_ply_case(seed)
            src = os.path.join(tmp, "in.ply")
            with open(src, "wb") as f:
                f.write(ply)
            entry = {"ply_sha256": sha(ply), "variants": []}
            for flags in variants:
                data = encode(src, flags)
                entry["variants"].append({"flags": flags, "hry_bytes": len(data), "hry_sha256": sha(data)})
            rec["ply"][str(seed)] = entry
    with tempfile.TemporaryDirectory() as tmp:
        for name, src_bytes, flags in util.random_scene_cases():
            src = os.path.join(tmp, name)
            with open(src, "wb") as f:
                f.write(src_bytes)
            data = encode(src, flags)
            rec["scenes"].append({"src": name, "src_sha256": sha(src_bytes), "flags": flags, "hry_bytes": len(data), "hry_sha256": sha(data)})
    with open(os.path.join(HERE, "random.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("random.json:", len(rec["ply"]), "PLY inputs,", len(rec["scenes"]), "scenes")


if __name__ == "__main__":
    main()
