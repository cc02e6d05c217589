"""The library's environment switches: every name it reads is in INTEGRATION.md's table and every name there is read, and
every read goes through the helpers of harry_amd/csrc/host/env.hpp (one parse rule)."""
import glob
import os
import re

from tests import util

CSRC = os.path.join(util.ROOT, "harry_amd", "csrc")
HELPERS = os.path.join(CSRC, "host", "env.hpp")


def sources():
    return sorted(p for ext in ("cpp", "hpp", "hip") for p in glob.glob(os.path.join(CSRC, "**", "*." + ext), recursive=True))


def read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def switches_read():
    names = set()
    for p in sources():
        names |= set(re.findall(r'\benv_(?:on|uint)\(\s*"(HRY_[A-Z0-9_]+)"', read(p)))
    return names


def switches_documented():
    text = read(os.path.join(util.ROOT, "INTEGRATION.md"))
    rows = text[text.index("| variable | default | effect |"):].splitlines()[2:]
    names = set()
    for row in rows:
        if not row.startswith("|"):
            break
        names |= set(re.findall(r"`(HRY_[A-Z0-9_]+)`", row.split("|")[1]))
    return names


def test_switches_read_match_the_table_and_the_helpers():
    got, documented = switches_read(), switches_documented()
    assert got, "no env_on / env_uint call found under harry_amd/csrc"
    assert got - documented == set(), "read by the library but missing from INTEGRATION.md's table"
    assert documented - got == set(), "in INTEGRATION.md's table but read nowhere"
    bare = [f"{os.path.relpath(p, CSRC)}:{n}" for p in sources() if p != HELPERS
            for n, line in enumerate(read(p).splitlines(), 1) if 'getenv("HRY_' in line]
    assert bare == [], "switches read around the helpers of host/env.hpp"
