"""The two-path fit of the 25-tap ACF beside the ACF features, on the synthetic multipath / NLOS
scene of multipath_features.py: per 100-ms window the scene's label, F2 (the mean arg-max tap's
delay, which follows the composite peak), and the fit: how many paths, the prompt's bias against
the direct path, the ray's excess delay and relative amplitude, with the scene's true delay and
gain beside them.

    python examples/multipath_fit.py [--ms 1000] [--cn0 50]

The scene: four satellites of the Opensky scenario. PRN 3 stays clean; PRN 16 has a ray half a
chip late at half the amplitude, in phase, from 300 ms on; PRN 22 has the same ray slowly fading
(2 Hz) all the time; PRN 26 has no direct signal, only a ray 0.4 chip late (the fit then sees
one path: what it reports as bias is where that ray sits, not an error of a direct path).
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
    args = ap.parse_args()

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
    truth = {16: (0.5, 0.5), 22: (0.5, 0.5), 26: (0.4, 0.7)}  # the rays' delay (chips) and gain

    ctx = sdr.Context(0)
    n_ms = file.skip + 1 + args.ms + 4
    dev = sdr.DeviceRecord(ctx, 2 * n_ms * signal.Sample)
    S.generate_scene_device(ctx, scene, dev)
    file.dev = dev
    Acquired = SimpleNamespace(sv=np.array(SVS), SNR=np.full(len(SVS), 20.0), Doppler=np.zeros(len(SVS)),
                               codedelay=np.array(cd), fineFreq=np.array(ff))
    tck, _ = sdr.trackingCT_multiCorr(file, signal, track, Acquired, datalength=args.ms, ctx=ctx)
    dev.free()

    feat = sdr.acf_features(tck, SVS, [45.0] * len(SVS))
    fit = sdr.acf_fit(tck, SVS)  # (the loop tagged its records with the orientation)
    labels = sdr.scene_labels(scene, tck, SVS)
    print(" prn win label       F2  paths     bias   bias_m        e    ratio     dphi | true delay  gain")
    for c, p in enumerate(SVS):
        delay, gain = truth.get(p, (float("nan"), float("nan")))
        for m in range(int(fit.windows[c])):
            ray = labels[c][m] != 0
            print(f"{p:4d} {m:3d} {int(labels[c][m]):5d} {feat.F2[c][m]:8.4f} {fit.paths[c][m]:6d} {fit.bias[c][m]:8.3f} "
                  f"{fit.bias_m[c][m]:8.1f} {fit.e[c][m]:8.3f} {fit.ratio[c][m]:8.3f} {fit.dphi_cycles[c][m]:8.3f} | "
                  f"{delay if ray else float('nan'):10.2f} {gain if ray else float('nan'):5.2f}")
    ctx.close()


if __name__ == "__main__":
    main()
