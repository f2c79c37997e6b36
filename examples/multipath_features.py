"""The flow the ACF features were written for, on a synthetic multipath / NLOS scene: a record
with reflected rays generated straight into HBM (synth.scene_of / add_ray / set_nlos,
generate_scene_device), the 25-tap loop of trackingCT_multiCorr-GIVEN.m, ACF/CalculateFeatures.m,
and the scene's own label for every 100-ms window beside the features (0 line of sight, 1 line of
sight with a ray, 2 no direct signal).

    python examples/multipath_features.py [--ms 1000] [--cn0 50] [--extended [--overlap 40 --hist 25]]

--extended adds the features the script keeps behind comment marks: F6 numMLC, F7 fftFreq and F8
fftMag, the largest line of the spectrum of the channel's last --hist meanMax values (taken from
the windows that exist, fft_fill = 1: a one-second example has far fewer than the script's 300).
With --ms 1640 PRN 22's 2-Hz fade shows in F7 once its history is full.

The scene: four satellites of the Opensky scenario. PRN 3 stays clean; PRN 16 has a ray half a
chip late at half the amplitude, in phase, from 300 ms on; PRN 22 has the same ray slowly fading
(2 Hz) all the time; PRN 26 has no direct signal, only a ray 0.4 chip late.
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

SVS = [3, 16, 22, 26]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ms", type=int, default=1000, help="1-ms steps to track")
    ap.add_argument("--cn0", type=float, default=50.0, help="C/N0 of every satellite, dB-Hz")
    ap.add_argument("--extended", action="store_true", help="print F6-F8 (numMLC, fftFreq, fftMag) as well")
    ap.add_argument("--overlap", type=int, default=None, help="rows per window (the script: 100; --extended: 40)")
    ap.add_argument("--hist", type=int, default=25, help="--extended: windows in the spectrum's history")
    args = ap.parse_args()
    nov = args.overlap or (40 if args.extended else 100)

    file, signal, acq, track, _, _ = sdr.initParameters()
    file.skip = 2
    S = sdr.synth
    at = [S.OPENSKY_SV.index(p) for p in SVS]
    cd = [S.OPENSKY_CODEDELAY[i] for i in at]
    ff = [float(S.OPENSKY_FINEFREQ[i]) for i in at]
    scene = S.scene_of(S.scenario(SVS, cd, [f - signal.IF for f in ff], [args.cn0] * len(SVS), skip_ms=file.skip))
    S.add_ray(scene, 16, 0.5, 0.5, t_on_ms=file.skip + 300)
    S.add_ray(scene, 22, 0.5, 0.5, fade_hz=2.0)
    S.set_nlos(scene, 26)
    S.add_ray(scene, 26, 0.4, 0.7)

    ctx = sdr.Context(0)
    n_ms = file.skip + 1 + args.ms + 4
    dev = sdr.DeviceRecord(ctx, 2 * n_ms * signal.Sample)
    S.generate_scene_device(ctx, scene, dev)
    file.dev = dev
    Acquired = SimpleNamespace(sv=np.array(SVS), SNR=np.full(len(SVS), 20.0), Doppler=np.zeros(len(SVS)),
                               codedelay=np.array(cd), fineFreq=np.array(ff))
    tck, _ = sdr.trackingCT_multiCorr(file, signal, track, Acquired, datalength=args.ms, ctx=ctx)
    dev.free()

    ele = [45.0] * len(SVS)
    ext = dict(extended=True, fft_hist=args.hist, fft_fill=1) if args.extended else {}
    # (the script's all-zero first row left out)
    table = sdr.CalculateFeatures(tck, SVS, ele, numOverLap=nov, **ext)[1:]
    labels = np.concatenate(sdr.scene_labels(scene, tck, SVS, numOverLap=nov))
    print(" prn   ele    meanMax      F1       F2       F3       F4       F5"
          + ("     F6  F7 (Hz)       F8" if args.extended else "") + "  label")
    for row, lab in zip(table, labels):
        more = f" {row[8]:6.3f} {row[9]:8.4f} {row[10]:8.2f}" if args.extended else ""
        print(f"{int(row[0]):4d} {row[1]:5.1f} {row[2]:10.1f} {row[3]:7.4f} {row[4]:8.4f} {row[5]:8.5f} "
              f"{row[6]:8.4f} {row[7]:8.5f}{more}  {int(lab)}")
    ctx.close()


if __name__ == "__main__":
    main()
