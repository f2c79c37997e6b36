"""Two reflected rays, estimated together: PRN 3 alone at 55 dB-Hz with a ray 0.6 chip late at half
the amplitude, opposed, and a second one 1.4 chips late at 0.4 of it, in quadrature. The GIVEN loop
tracks 600 ms at its 25 taps; rows 99-599 are then correlated again at -2.5:0.05:1.0 and fitted on
those sums where they lie in HBM, once by the two-path fit (replay_fit: gnss_acf_fit_taps, which
folds the second ray into its one reflected path) and once by the multi-ray fit (replay_fit_multi:
gnss_acf_fit_multi). Printed per 100-ms window: both fits side by side.

    python examples/multipath_replay_multi.py [--host]

--host runs the replay and the fits on the CPU (the loop itself still needs the GPU).
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

PRN, SKIP, ROWS = 3, 2, 600
RAYS = ((0.6, 0.5, 0.5), (1.4, 0.4, 0.25))  # (chips late, amplitude ratio, phase in cycles)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true", help="replay and fit on the host path")
    args = ap.parse_args()

    file, signal, acq, track, _, _ = sdr.initParameters()
    S = sdr.synth
    scene = S.scene_of(S.scenario([PRN], [3683], [990.0], [55.0], skip_ms=SKIP))
    for late, ratio, cyc in RAYS:
        S.add_ray(scene, PRN, late, ratio, phase_cycles=cyc)
    A = SimpleNamespace(sv=np.array([PRN]), SNR=np.array([20.0]), Doppler=np.zeros(1), codedelay=np.array([3683]),
                        fineFreq=np.array([4580990.0]))
    wide = sdr.colon(-2.5, 0.05, 1.0)
    ctx = sdr.Context(0)
    dev = sdr.DeviceRecord(ctx, 2 * (SKIP + 1 + ROWS + 4) * signal.Sample)
    file.skip = SKIP
    S.generate_scene_device(ctx, scene, dev)
    file.dev, file.data = dev, None
    buf = sdr.trackingCT_multiCorr(file, signal, track, A, datalength=ROWS, ctx=ctx, raw=True)
    rows = sdr.replay_rows(buf, A, file, signal, loop="given", rows=range(99, ROWS))
    if args.host:
        file.dev, file.data = None, dev.download()
    c = None if args.host else ctx
    two = sdr.replay_fit(file, signal, rows, wide, ctx=c)
    multi = sdr.replay_fit_multi(file, signal, rows, wide, ctx=c)
    dev.free()
    ctx.close()

    print(f"PRN {PRN}; rays " + ", ".join(f"{d} chips late at {g} ({p} cycle)" for d, g, p in RAYS)
          + f"; rows 99-{ROWS - 1}, {len(wide)} taps replayed"
          + (" on the host" if args.host else f"; kernels {multi.kernel_ms[0]:.3f} ms (replay), {two.kernel_ms[1]:.3f} ms "
             f"(two-path fit), {multi.kernel_ms[1]:.3f} ms (multi-ray fit)"))
    print("window | two-path: paths   bias      e  ratio | multi: paths searches   bias |  ray 1: e  ratio   dphi |"
          "  ray 2: e  ratio   dphi | res2/res3")
    for m in range(int(multi.windows[0])):
        e, r, ph, res = multi.e[0][:, m], multi.ratio[0][:, m], multi.dphi_cycles[0][:, m], multi.res[0][:, m]
        print(f"{m:6d} | {'':9s} {two.paths[0][m]:5d} {two.bias[0][m]:6.2f} {two.e[0][m]:6.2f} {two.ratio[0][m]:6.3f} | "
              f"{'':6s} {multi.paths[0][m]:5d} {multi.searches[0][m]:8d} {multi.bias[0][m]:6.2f} | "
              f"{e[1]:9.2f} {r[1]:6.3f} {ph[1]:6.3f} | {e[2]:9.2f} {r[2]:6.3f} {ph[2]:6.3f} | {res[2] / res[3]:9.1f}")


if __name__ == "__main__":
    main()
