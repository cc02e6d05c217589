"""grow_keeping (harry_amd/csrc/device/grow_keeping.hpp): the working buffer of a build in two stretches grows between them and keeps
what the first stretch left -- hry_intersections_build does this where there are more pairs than the hierarchy's build left room
for.  No entry point tells whether a context's buffer grew, so the helper itself is held here against a stand-in for the runtime
whose blocks have their real sizes, under AddressSanitizer / UBSan: what is copied, how much, in which order the blocks come and
go, and that a failed allocation leaves the buffer as it was."""
import os
import shutil
import subprocess

import pytest

from tests import util

NATIVE = os.path.join(util.ROOT, "tests", "native")


@pytest.mark.timeout(300)
def test_grow_keeping_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    flags = ["-O1", "-g1", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    probe = subprocess.run(["g++", *flags, "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("-fsanitize=address,undefined is not usable here")
    exe = str(tmp_path / "grow_keeping_check")
    r = subprocess.run(["g++", *flags, "-I", os.path.join(NATIVE, "fake_hip_sized"), os.path.join(NATIVE, "grow_keeping_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:detect_stack_use_after_return=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.strip() == "ok"
