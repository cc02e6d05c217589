"""tests/tools/plane_cases.py inside the GPU suite: designed symbol planes (tests/planes_ref.py: one symbol, 255 only, a symbol of
prior 1, a sorted ramp, 64 distinct symbols a batch, runs of 62 - 66, streams that end on and beside a 16-symbol store, priors 254 /
255 / 256, totals of 65535, 65536 and 132 096) through the chunked container's coders, exact against the oracle, with the kernels
that ran read back from the stages "enc_plan" and "dec_plan".  A decoder form is a process: HRY_DECODE_LANES and HRY_DECODE_COUNTS32
are read once.  Each process runs every case under both encoder forms.  tests/test_planes_cpu.py pins the lever without a GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = {
    "waves": {"HRY_DECODE_LANES": "0"},                                  # k_chunk_decode for every stream
    "lanes": {"HRY_DECODE_LANES": "1"},                                  # k_chunk_decode_lanes<uint16_t> wherever the totals allow
    "lanes32": {"HRY_DECODE_LANES": "1", "HRY_DECODE_COUNTS32": "1"},    # k_chunk_decode_lanes<uint32_t>
}


@pytest.mark.gpu
@pytest.mark.timeout(330)
@pytest.mark.parametrize("form", list(FORMS))
def test_designed_planes_through_every_coder(form):
    env = {k: v for k, v in os.environ.items() if not k.startswith("HRY_") or k == "HRY_LIB"}   # no other switch decides which kernel runs
    env.update(FORMS[form])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "plane_cases.py")], capture_output=True, text=True, env=env, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("all equal"), (r.stdout + r.stderr)[-3000:]
