"""csrc/replay.h on the CPU (tests/native/replay_host.cpp): the true-modulus chip index, the tap
colons and their element rule, the sine / cosine kernels, the chip range the kernel's code table is
sized by, and whole rows (lengths around the middle element, both record types, negative, zero and
IF carriers, taps at +-1023, post, chip_off) against a naive long-double sum, called by a stand-alone
program on heap arrays of exactly the stated sizes. Built plainly and once more under
AddressSanitizer and UBSan; host C++ only, no GPU."""
import os
import shutil
import subprocess

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"


def test_replay_arithmetic_on_the_host(tmp_path):
    cxx = shutil.which("g++") or HIPCC
    src = os.path.join(ROOT, "tests", "native", "replay_host.cpp")
    for name, flags in (("replay_host", ["-O2"]),
                        ("replay_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = tmp_path / name
        subprocess.run([cxx, *flags, "-std=c++17", "-ffp-contract=off", "-o", str(exe), src], check=True,
                       capture_output=True)
        r = subprocess.run([str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "cases 1435, mismatches 0" in r.stdout, r.stdout
