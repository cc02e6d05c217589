"""tests/tools/chain_cases.py inside the GPU suite: designed meshes (hubs of 3 .. 14 candidates whose sources belong to an earlier
component, polygons of degree above 4, a ribbon that reads more than 4 096 / 8 192 / 16 320 vertices back, more than 1 024 chains
at once, tiles of every head count, noise that makes runs leave the speculated form once and twice at q 1, 2, 8, 9, 16, clamps at
both ends at q 17 and 24, float ties) through the decoder's candidate table and reconstruction chains, exact against the oracle:
streams, decodes (one launch; pipelined in slices of 64, 4 096 and 16 448 vertices), the stages "ncand" / "cand" / "cand_over"
against the oracle's vertex trace, and the kernels that ran read back from the stage "chain_plan".  A team size is a process:
HRY_CHAIN_WAVES is read once.  What each mesh demands is pinned without a GPU by tests/test_chain_cpu.py."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEAMS = {"unset": None, "1": "1", "4": "4", "8": "8", "12": "12"}


@pytest.mark.gpu
@pytest.mark.timeout(150)
@pytest.mark.parametrize("waves", list(TEAMS))
def test_designed_meshes_through_the_candidate_table_and_every_chain(waves):
    env = {k: v for k, v in os.environ.items() if not k.startswith("HRY_") or k == "HRY_LIB"}   # no other switch decides which kernel runs
    if TEAMS[waves]:
        env["HRY_CHAIN_WAVES"] = TEAMS[waves]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "chain_cases.py")], capture_output=True, text=True, env=env, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("all equal"), (r.stdout + r.stderr)[-3000:]
