"""csrc/acf.h on the CPU (tests/native/acf_host.cpp): the magnitude, the first-index arg-max and
the window sums that gnss_acf_features' host path and kernels share, called by a stand-alone
program on a hand-made record whose arrays end where the last window ends. Built plainly and
once more under AddressSanitizer and UBSan; host C++ only, no GPU."""
import os
import shutil
import subprocess

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"


def test_acf_arithmetic_on_the_host(tmp_path):
    cxx = shutil.which("g++") or HIPCC
    src = os.path.join(ROOT, "tests", "native", "acf_host.cpp")
    for name, flags in (("acf_host", ["-O2"]),
                        ("acf_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = tmp_path / name
        subprocess.run([cxx, *flags, "-std=c++17", "-ffp-contract=off", "-o", str(exe), src], check=True,
                       capture_output=True)
        r = subprocess.run([str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "cases 25, mismatches 0" in r.stdout, r.stdout
