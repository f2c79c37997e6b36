"""The multi-ray ACF fit on the CPU chain, without a GPU (DESIGN §3.14's accuracy table):
gnss_synth_scene_host -> the oracle's trackingCT_multiCorr-GIVEN loop -> gnss_replay_correlate on
the host at -2.5:0.05:1.0 -> gnss_acf_fit_multi on the host sums at its defaults. The scene is
PRN 3 alone at 55 dB-Hz; the loop runs ROWS rows and the rows from 99 on are replayed in windows of
100 (the first 99 rows are pull-in). Four cases: two rays (0.6 chip, 0.5, opposed; 1.4 chips, 0.4,
quadrature), two other rays (0.45, 0.5, quadrature; 1.7, 0.4, in phase), one ray (1.7, 0.5, in
phase) and none. Prints per window the fit, its errors against the scene and gnss_acf_fit_taps'
two-path fit of the same sums.

    python tools/acf_fit_multi_accuracy.py [--cn0 55] [--ms 600]
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

# name: the rays as (chips late, amplitude ratio, phase in cycles)
CASES = (("two_rays_a", ((0.6, 0.5, 0.5), (1.4, 0.4, 0.25))), ("two_rays_b", ((0.45, 0.5, 0.25), (1.7, 0.4, 0.0))),
         ("one_ray", ((1.7, 0.5, 0.0),)), ("none", ()))


def sums_of(rays, cn0, ms):
    sc = sdr.synth.scene_of(sdr.synth.scenario([3], [3683], [990.0], [cn0], skip_ms=2))
    for late, ratio, cyc in rays:
        sdr.synth.add_ray(sc, 3, late, ratio, phase_cycles=cyc)
    file, signal, acq, track, _, _ = sdr.initParameters()
    file.skip, file.data = 2, sdr.synth.generate_scene_host(sc, 0, (2 + 1 + ms + 4) * 58000)
    A = SimpleNamespace(sv=np.array([3]), SNR=np.array([20.0]), Doppler=np.zeros(1), codedelay=np.array([3683]),
                        fineFreq=np.array([4580990.0]))
    buf = po.trackingCT_multiCorr(file, signal, track, A, datalength=ms, raw=True)
    t = sdr.replay_rows(buf, A, file, signal, loop="given", rows=range(99, ms))
    taps = sdr.colon(-2.5, 0.05, 1.0)
    return sdr.replay_correlate(file, signal, t, taps)[0], t.n_rows, taps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cn0", type=float, default=55.0)
    ap.add_argument("--ms", type=int, default=600)
    args = ap.parse_args()
    print(f"# PRN 3, {args.cn0} dB-Hz, {args.ms} rows, rows 99.. replayed on -2.5:0.05:1.0; the default search")
    print("# case        win paths searches    bias | ray:      e   e-err   ratio  r-err    dphi | ... | "
          "res0/1  res1/2  res2/3 | two-path: paths      e   ratio")
    for name, rays in CASES:
        sums, n_rows, taps = sums_of(rays, args.cn0, args.ms)
        f = sdr.acf_fit_multi(sums, n_rows, taps, numOverLap=100)
        two = sdr.acf_fit_taps(sums, n_rows, taps, numOverLap=100)
        for m in range(int(f.windows[0])):
            cols = []
            for k in range(1, 3):
                late, ratio = rays[k - 1][:2] if k <= len(rays) else (np.nan, np.nan)
                e, r, ph = f.e[0][k, m], f.ratio[0][k, m], f.dphi_cycles[0][k, m]
                cols.append(f"{e:6.2f} {e - late:+7.3f} {r:7.4f} {r - ratio:+6.3f} {ph:7.4f}")
            res = f.res[0][:, m]
            with np.errstate(invalid="ignore", divide="ignore"):
                drops = res[:3] / res[1:4]
            print(f"{name:12s} {m:3d} {f.paths[0][m]:5d} {f.searches[0][m]:8d} {f.bias[0][m]:7.2f} | "
                  + " | ".join(cols) + " | " + " ".join(f"{d:7.1f}" for d in drops)
                  + f" | {two.paths[0][m]:5d} {two.e[0][m]:6.2f} {two.ratio[0][m]:7.3f}")


if __name__ == "__main__":
    main()
