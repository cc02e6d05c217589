"""What the HIP runtime hands out -- streams, events, device and pinned memory, registered host ranges -- is owned by the types
of harry_amd/csrc/device/hip_handles.hpp.  No other source creates or destroys one, and the header's contract (created on first
use, destroyed once, a failed creation leaves the owner empty; a result's block exactly as large as asked, freed on its own device;
one allocation carved into aligned pieces that never share an address) holds against a counting stand-in for the runtime under
AddressSanitizer / UBSan: the paths a device error would take, which no test provokes on a device."""
import glob
import os
import re
import shutil
import subprocess

import pytest

from tests import util

CSRC = os.path.join(util.ROOT, "harry_amd", "csrc")
OWNERS = os.path.join(CSRC, "device", "hip_handles.hpp")
NATIVE = os.path.join(util.ROOT, "tests", "native")
CHECK = os.path.join(NATIVE, "hip_handles_check.cpp")

HANDLES = re.compile(r"hipStreamCreate|hipStreamDestroy|hipEventCreate|hipEventDestroy|hipHostMalloc|hipHostFree|hipHostRegister|hipHostUnregister")
DEVICE_MEMORY = re.compile(r"\bhipMalloc\(|\bhipFree\(")


def sources():
    return sorted(p for ext in ("cpp", "hpp", "hip") for p in glob.glob(os.path.join(CSRC, "**", "*." + ext), recursive=True))


def _found(pattern, allowed):
    found = []
    for p in sources():
        if p in allowed:
            continue
        with open(p, encoding="utf-8") as f:
            found += [f"{os.path.relpath(p, CSRC)}:{n}" for n, line in enumerate(f.read().splitlines(), 1) if pattern.search(line)]
    return found


def test_handles_have_one_owner():
    assert os.path.isfile(OWNERS) and len(sources()) > 30
    assert _found(HANDLES, {OWNERS}) == [], "streams, events, pinned memory and registrations are made and dropped in device/hip_handles.hpp only"
    assert _found(DEVICE_MEMORY, {OWNERS}) == [], "hipMalloc / hipFree outside DevBuf and DeviceBlock (device/hip_handles.hpp)"


@pytest.mark.timeout(300)
def test_hip_handles_contract_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    flags = ["-O1", "-g1", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    probe = subprocess.run(["g++", *flags, "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("-fsanitize=address,undefined is not usable here")
    exe = str(tmp_path / "hip_handles_check")
    r = subprocess.run(["g++", *flags, "-I", os.path.join(NATIVE, "fake_hip"), CHECK, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:detect_stack_use_after_return=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.strip() == "ok"
