"""Threads started beside the caller: every one is owned by a SideThreads (harry_amd/csrc/host/side_threads.hpp), which joins them
on every way out and keeps the first exception.  No std::thread object is left outside that header and the persistent pool, and
the header's contract holds under gcc's ThreadSanitizer and under AddressSanitizer / UBSan."""
import glob
import os
import re
import shutil
import subprocess

import pytest

from tests import util

CSRC = os.path.join(util.ROOT, "harry_amd", "csrc")
OWNERS = {os.path.join(CSRC, "host", "side_threads.hpp"), os.path.join(CSRC, "host", "thread_pool.cpp")}
CHECK = os.path.join(util.ROOT, "tests", "native", "side_threads_check.cpp")


def sources():
    return sorted(p for ext in ("cpp", "hpp", "hip") for p in glob.glob(os.path.join(CSRC, "**", "*." + ext), recursive=True))


def test_threads_have_one_owner():
    pattern = re.compile(r"std::thread\b(?!::)")
    found = []
    for p in sources():
        if p in OWNERS:
            continue
        with open(p, encoding="utf-8") as f:
            found += [f"{os.path.relpath(p, CSRC)}:{n}" for n, line in enumerate(f.read().splitlines(), 1) if pattern.search(line)]
    assert found == [], "std::thread outside host/side_threads.hpp and host/thread_pool.cpp"


def _usable(flags, tmp_path):
    probe = subprocess.run(["g++", *flags, "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){return 0;}", capture_output=True, text=True)
    return probe.returncode == 0 and subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0


@pytest.mark.timeout(300)
@pytest.mark.parametrize("sanitize", ["thread", "address,undefined"])
def test_side_threads_contract_under_sanitizers(sanitize, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    flags = ["-O1", "-g1", "-std=c++17", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-pthread"]
    if not _usable(flags, tmp_path):
        pytest.skip(f"-fsanitize={sanitize} is not usable here")
    exe = str(tmp_path / "side_threads_check")
    r = subprocess.run(["g++", *flags, CHECK, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1:detect_stack_use_after_return=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.strip() == "ok"
