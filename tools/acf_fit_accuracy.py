"""The two-path ACF fit on the CPU chain, without a GPU (DESIGN §3.9's accuracy table):
gnss_synth_scene_host -> the oracle's trackingCT_multiCorr-GIVEN loop -> gnss_acf_fit on the host
records. The scene is DESIGN §3.3's: PRN 3 alone at 55 dB-Hz, 600 rows (five windows, the first
is pull-in), without a ray, with a ray half a chip late at half the amplitude in phase, and with
the same ray opposed. Prints per window the fit and its errors against the scene and against the
DLL bias that theory predicts (+1/6 chip in phase, -0.2 chip opposed).

    python tools/acf_fit_accuracy.py [--cn0 55] [--ms 600]
"""
import argparse
import importlib
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sdr = importlib.import_module("assignment-for-aae6102_gnss-sdr_amd")
import pyoracle as po  # noqa: E402

CASES = (("none", None, 0.0), ("in_phase", 0.0, 1.0 / 6.0), ("opposed", 0.5, -0.2))


def records(phase, cn0, ms):
    sc = sdr.synth.scene_of(sdr.synth.scenario([3], [3683], [990.0], [cn0], skip_ms=2))
    if phase is not None:
        sdr.synth.add_ray(sc, 3, 0.5, 0.5, phase_cycles=phase)
    data = sdr.synth.generate_scene_host(sc, 0, (2 + 1 + ms + 4) * 58000)
    file, signal, acq, track, _, _ = sdr.initParameters()
    file.skip, file.data = 2, data
    A = SimpleNamespace(sv=np.array([3]), SNR=np.array([20.0]), Doppler=np.zeros(1), codedelay=np.array([3683]),
                        fineFreq=np.array([4580990.0]))
    return po.trackingCT_multiCorr(file, signal, track, A, datalength=ms, raw=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cn0", type=float, default=55.0)
    ap.add_argument("--ms", type=int, default=600)
    args = ap.parse_args()
    print(f"# PRN 3, {args.cn0} dB-Hz, {args.ms} rows; orient +1 (trackingCT_multiCorr); default grid")
    print("# case      win paths    bias      p1      p0       e   ratio    dphi  res1/res2   bias-pred")
    for name, phase, pred in CASES:
        buf = records(phase, args.cn0, args.ms)
        f = sdr.acf_fit(buf, [3], orient=sdr.abi.ACF_ORIENT["trackingCT_multiCorr"])
        for m in range(int(f.windows[0])):
            print(f"{name:10s} {m:3d} {f.paths[0][m]:5d} {f.bias[0][m]:7.3f} {f.p1[0][m]:7.3f} {f.p0[0][m]:7.3f} "
                  f"{f.e[0][m]:7.3f} {f.ratio[0][m]:7.3f} {f.dphi_cycles[0][m]:7.3f} "
                  f"{f.res1[0][m] / f.res2[0][m]:10.2f} {f.bias[0][m] - pred:+10.4f}")


if __name__ == "__main__":
    main()
