"""csrc/acf_fit_multi.h on the CPU (tests/native/acf_fit_multi_host.cpp): the joint fit, the
searches, the orders and the selection that gnss_acf_fit_multi's host path and kernel share, called
by a stand-alone program on heap arrays of exactly n_taps, 2 * n_taps and 4 * n_taps elements
(n_taps 1, 2, 25, 71 and 256; the default search, the plain greedy order with max_paths 4, one
candidate, a candidate grid outside the taps, a NaN in the vector) and checked against plain
run-time loops of its own, and a search dealt over four workers against the sequential one. Built
plainly and once more under AddressSanitizer and UBSan; host C++ only, no GPU."""
import os
import shutil
import subprocess

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"


def test_acf_fit_multi_arithmetic_on_the_host(tmp_path):
    cxx = shutil.which("g++") or HIPCC
    src = os.path.join(ROOT, "tests", "native", "acf_fit_multi_host.cpp")
    for name, flags in (("acf_fit_multi_host", ["-O2"]),
                        ("acf_fit_multi_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = tmp_path / name
        subprocess.run([cxx, *flags, "-std=c++17", "-ffp-contract=off", "-o", str(exe), src], check=True,
                       capture_output=True)
        r = subprocess.run([str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "cases 62, mismatches 0" in r.stdout, r.stdout
