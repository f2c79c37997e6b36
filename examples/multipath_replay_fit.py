"""A reflected ray outside the 25-tap window, estimated: multipath_replay.py's scene (the Opensky
scenario, PRN 16) with the ray 1.7 chips late at half the amplitude. The GIVEN loop tracks 600 ms at
its 25 taps (-0.6:0.05:0.6 chip), where the ray touches no tap; the recorded rows are then
correlated again at -2.5:0.05:1.0 and the two-path fit runs on those sums where they lie in HBM
(replay_fit: gnss_replay_correlate with GNSS_OUT_DEVICE, then gnss_acf_fit_taps). Printed per
100-ms window: the 25-tap fit (acf_fit on the loop's records) and the wide fit side by side.

    python examples/multipath_replay_fit.py [--host]

--host runs the replay and the fit on the CPU (the loop itself still needs the GPU).
"""
import argparse
import importlib
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sdr = importlib.import_module("assignment-for-aae6102_gnss-sdr_amd")

PRN, SKIP, ROWS, DELAY, GAIN = 16, 5, 601, 1.7, 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true", help="replay and fit on the host path")
    args = ap.parse_args()

    file, signal, acq, track, _, _ = sdr.initParameters()
    S = sdr.synth
    cfg = S.opensky(skip_ms=SKIP)
    i = S.OPENSKY_SV.index(PRN)
    A = SimpleNamespace(sv=np.array([PRN]), SNR=np.array([20.0]), Doppler=np.zeros(1),
                        codedelay=np.array([S.codedelays(cfg, SKIP)[i]]), fineFreq=np.array([float(S.OPENSKY_FINEFREQ[i])]))
    wide = sdr.colon(-2.5, 0.05, 1.0)
    ctx = sdr.Context(0)
    dev = sdr.DeviceRecord(ctx, 2 * (SKIP + ROWS + 6) * signal.Sample)
    file.skip = SKIP
    scene = S.scene_of(cfg)
    S.add_ray(scene, PRN, DELAY, GAIN)
    S.generate_scene_device(ctx, scene, dev)
    file.dev, file.data = dev, None
    buf = sdr.trackingCT_multiCorr(file, signal, track, A, datalength=ROWS, ctx=ctx, raw=True)
    rows = sdr.replay_rows(buf, A, file, signal, loop="given")
    if args.host:
        file.dev, file.data = None, dev.download()
    fw = sdr.replay_fit(file, signal, rows, wide, ctx=None if args.host else ctx)
    f25 = sdr.acf_fit(buf, [PRN])
    dev.free()
    ctx.close()

    print(f"PRN {PRN}, a ray {DELAY} chips late at {GAIN} of the amplitude; {ROWS} rows, {len(wide)} taps replayed"
          + (" on the host" if args.host else f", kernels {fw.kernel_ms[0]:.3f} ms (replay) + {fw.kernel_ms[1]:.3f} ms (fit)"))
    print("window | 25 taps: paths   bias      e  ratio  res1/res2 | -2.5:0.05:1.0: paths   bias      e  ratio  res1/res2")
    for m in range(int(fw.windows[0])):
        def cols(f):
            return (f"{f.paths[0][m]:5d} {f.bias[0][m]:6.2f} {f.e[0][m]:6.2f} {f.ratio[0][m]:6.3f} "
                    f"{f.res1[0][m] / f.res2[0][m]:10.1f}")
        print(f"{m:6d} | {'':8s} {cols(f25)} | {'':14s} {cols(fw)}")


if __name__ == "__main__":
    main()
