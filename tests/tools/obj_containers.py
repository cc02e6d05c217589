"""Every small OBJ fixture (tests/golden/obj/manifest.json, table "small"), in every variant, into the chunked container at
chunk_syms 0 and 256: one line "name tag chunk chunk_syms sha256" per container.  Which branch of general_planes_encode names the
records is this process' (HRY_HOST_EVENTS is read once); tests/test_gpu_obj.py runs it with the host's loop and compares.
    HRY_HOST_EVENTS=1 python tests/tools/obj_containers.py"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from harry_amd import codec as hc
from tests import util

OBJ = os.path.join(ROOT, "tests", "golden", "obj")
with open(os.path.join(OBJ, "manifest.json")) as f:
    small = json.load(f)["small"]
cx = hc.Codec(0)
for name in sorted(small):
    with open(os.path.join(OBJ, name + ".obj"), "rb") as f:
        obj = f.read()
    for tag in sorted(small[name]["variants"]):
        quant, clear = util.flags_to_quant(small[name]["variants"][tag]["flags"])
        for chunk in (0, 256):
            m = hc.Mesh.from_obj(obj, OBJ)
            if quant or clear:
                cx.requant(m, quant, clear)
            got = cx.write_hry(m, profile=hc.PROFILE_CHUNKED, chunk_syms=chunk)
            print(name, tag, chunk, hc.container_info(got)["chunk_syms"], hashlib.sha256(got).hexdigest())
cx.close()
