"""csrc/synth_scene.h on the CPU (tests/native/scene_host.cpp): the per-sample arithmetic and the
host loop that gnss_synth_scene_host and the scene kernel share, called by a stand-alone program
on hand-made paths, into heap buffers of exactly 2 * nsamples bytes, whole and in chunks, with ray
edges on the first and the last sample. Built plainly and once more under AddressSanitizer and
UBSan; host C++ only, no GPU."""
import os
import shutil
import subprocess

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"


def test_scene_arithmetic_on_the_host(tmp_path):
    cxx = shutil.which("g++") or HIPCC
    src = os.path.join(ROOT, "tests", "native", "scene_host.cpp")
    for name, flags in (("scene_host", ["-O2"]),
                        ("scene_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = tmp_path / name
        subprocess.run([cxx, *flags, "-std=c++17", "-ffp-contract=off", "-o", str(exe), src], check=True,
                       capture_output=True)
        r = subprocess.run([str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "cases 20, mismatches 0" in r.stdout, r.stdout
