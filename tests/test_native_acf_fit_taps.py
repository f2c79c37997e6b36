"""csrc/acf_fit_taps.h on the CPU (tests/native/acf_fit_taps_host.cpp): the coherent sums, the
one-path and two-path grids and the selection that gnss_acf_fit_taps' host path and kernel share,
called by a stand-alone program on heap arrays of exactly n_taps and 2 * n_taps elements (n_taps
1, 25 and 256, the prompt at both ends) and checked against plain loops of its own. Built plainly
and once more under AddressSanitizer and UBSan; host C++ only, no GPU."""
import os
import shutil
import subprocess

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"


def test_acf_fit_taps_arithmetic_on_the_host(tmp_path):
    cxx = shutil.which("g++") or HIPCC
    src = os.path.join(ROOT, "tests", "native", "acf_fit_taps_host.cpp")
    for name, flags in (("acf_fit_taps_host", ["-O2"]),
                        ("acf_fit_taps_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = tmp_path / name
        subprocess.run([cxx, *flags, "-std=c++17", "-ffp-contract=off", "-o", str(exe), src], check=True,
                       capture_output=True)
        r = subprocess.run([str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "cases 55, mismatches 0" in r.stdout, r.stdout
