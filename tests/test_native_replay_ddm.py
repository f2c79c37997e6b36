"""csrc/replay_ddm.h on the CPU (tests/native/replay_ddm_host.cpp): the row time, the rotation, the
sign rule, a cell's update, the order of the peak rule, and whole windows (rows around the kernel's
row tile, one tap and many, with and without the sign wipe) against naive long-double sums and a
plain scan for the peaks, called by a stand-alone program on heap arrays of exactly the stated
sizes. Built plainly and once more under AddressSanitizer and UBSan; host C++ only, no GPU."""
import os
import shutil
import subprocess

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"


def test_ddm_arithmetic_on_the_host(tmp_path):
    cxx = shutil.which("g++") or HIPCC
    src = os.path.join(ROOT, "tests", "native", "replay_ddm_host.cpp")
    for name, flags in (("replay_ddm_host", ["-O2"]),
                        ("replay_ddm_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = tmp_path / name
        subprocess.run([cxx, *flags, "-std=c++17", "-ffp-contract=off", "-o", str(exe), src], check=True,
                       capture_output=True)
        r = subprocess.run([str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "cases 517, mismatches 0" in r.stdout, r.stdout
