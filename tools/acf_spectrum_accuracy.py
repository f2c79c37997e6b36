"""The fading-spectrum features F6-F8 on the CPU chain, without a GPU (DESIGN §3.8.1's accuracy
table): gnss_synth_scene_host -> the oracle's trackingCT_multiCorr-GIVEN loop ->
gnss_acf_features_ext on the host records. The scene is DESIGN §3.3's: PRN 3 alone at 55 dB-Hz,
1640 rows, without a ray and with a ray half a chip late at half the amplitude whose carrier turns
at fade_hz against the direct one's. numOverLap = 40 gives fs = 25 Hz and 40 windows; fft_hist =
25 with fft_fill = 1 gives a full one-second history from window 24 on. Prints per window F6-F8
and, over the full-history windows, the numbers the end-to-end test's bounds rest on: the largest
|fftFreq - fade_hz| against fs / (2 fft_hist), and the smallest fftMag with the ray against the
largest without it.

    python tools/acf_spectrum_accuracy.py [--cn0 55] [--ms 1640] [--fade 3]
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

PAR = dict(numOverLap=40, fft_hist=25, fft_fill=1)


def records(fade, cn0, ms):
    sc = sdr.synth.scene_of(sdr.synth.scenario([3], [3683], [990.0], [cn0], skip_ms=2))
    if fade is not None:
        sdr.synth.add_ray(sc, 3, 0.5, 0.5, fade_hz=fade)
    data = sdr.synth.generate_scene_host(sc, 0, (2 + 1 + ms + 4) * 58000)
    file, signal, acq, track, _, _ = sdr.initParameters()
    file.skip, file.data = 2, data
    A = SimpleNamespace(sv=np.array([3]), SNR=np.array([20.0]), Doppler=np.zeros(1), codedelay=np.array([3683]),
                        fineFreq=np.array([4580990.0]))
    return po.trackingCT_multiCorr(file, signal, track, A, datalength=ms, raw=True)


def summary(ray, none, fade, par=PAR):
    """The bounds' numbers over the full-history windows of the two runs (acf_features results)"""
    first = par["fft_hist"] - 1
    fs = 1000.0 / par["numOverLap"]
    ferr = float(np.max(np.abs(ray.fftFreq[0][first:] - fade)))
    lo, hi = float(np.min(ray.fftMag[0][first:])), float(np.max(none.fftMag[0][first:]))
    return dict(freq_err_max=ferr, freq_bound=fs / (2 * par["fft_hist"]), mag_ray_min=lo, mag_none_max=hi,
                factor=lo / hi, threshold=float(np.sqrt(lo * hi)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cn0", type=float, default=55.0)
    ap.add_argument("--ms", type=int, default=1640)
    ap.add_argument("--fade", type=float, default=3.0)
    args = ap.parse_args()
    print(f"# PRN 3, {args.cn0} dB-Hz, {args.ms} rows, ray 0.5 chip late at 0.5, fade {args.fade} Hz; {PAR}")
    print("# case  win    meanMax  numMLC  fftFreq     fftMag")
    res = {}
    for name, fade in (("none", None), ("ray", args.fade)):
        f = sdr.acf_features(records(fade, args.cn0, args.ms), [3], [45.0], extended=True, **PAR)
        res[name] = f
        for m in range(int(f.windows[0])):
            print(f"{name:6s} {m:4d} {f.meanMax[0][m]:10.1f} {f.numMLC[0][m]:7.3f} {f.fftFreq[0][m]:8.4f} "
                  f"{f.fftMag[0][m]:10.3f}")
    s = summary(res["ray"], res["none"], args.fade)
    print(f"# full-history windows {PAR['fft_hist'] - 1}..: max |fftFreq - {args.fade}| = {s['freq_err_max']:.4f} Hz "
          f"(bound {s['freq_bound']:.3f})")
    print(f"# fftMag: min with the ray {s['mag_ray_min']:.3f}, max without {s['mag_none_max']:.3f}, "
          f"factor {s['factor']:.2f}, geometric middle {s['threshold']:.3f}")


if __name__ == "__main__":
    main()
