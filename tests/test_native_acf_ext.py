"""csrc/acf_ext.h on the CPU (tests/native/acf_ext_host.cpp): the local-maximum count, the history,
the DFT bin, the (mag, k) order and the window's outputs that gnss_acf_features_ext's host path
and kernels share, called by a stand-alone program on hand-made values whose arrays end where the
last window ends and where the table ends. Built plainly and once more under AddressSanitizer and
UBSan; host C++ only, no GPU."""
import os
import shutil
import subprocess

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"


def test_acf_ext_arithmetic_on_the_host(tmp_path):
    cxx = shutil.which("g++") or HIPCC
    src = os.path.join(ROOT, "tests", "native", "acf_ext_host.cpp")
    for name, flags in (("acf_ext_host", ["-O2"]),
                        ("acf_ext_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = tmp_path / name
        subprocess.run([cxx, *flags, "-std=c++17", "-ffp-contract=off", "-o", str(exe), src], check=True,
                       capture_output=True)
        r = subprocess.run([str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "cases 28, mismatches 0" in r.stdout, r.stdout
