"""csrc/knn.h on the CPU (tests/native/knn_host.cpp): the order with +inf and NaN, the scan's
admission test, the sorted k-list, the packed votes, the column statistics, the device plan's split
shares and whole queries against a full sort of the training rows, called by a stand-alone program
on heap arrays of exactly the stated sizes. Built plainly and once more under AddressSanitizer and
UBSan; host C++ only, no GPU."""
import os
import shutil
import subprocess

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"


def test_knn_arithmetic_on_the_host(tmp_path):
    cxx = shutil.which("g++") or HIPCC
    src = os.path.join(ROOT, "tests", "native", "knn_host.cpp")
    for name, flags in (("knn_host", ["-O2"]),
                        ("knn_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = tmp_path / name
        subprocess.run([cxx, *flags, "-std=c++17", "-ffp-contract=off", "-o", str(exe), src], check=True,
                       capture_output=True)
        r = subprocess.run([str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "cases 813, mismatches 0" in r.stdout, r.stdout
