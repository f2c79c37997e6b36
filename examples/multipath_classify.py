"""What data_labeled is for: a classifier that says, per 100-ms window, line of sight (0),
multipath (1) or no direct signal (2). A few labelled training scenes through the 25-tap loop of
trackingCT_multiCorr-GIVEN.m, their features (ACF/CalculateFeatures.m's F1-F5), the two-path fit's
bias and amplitude ratio, and the scenes' own labels make the training table; a k-nearest-
neighbour model on standardised columns is trained from it (resident in HBM), a held-out scene
with another noise seed and other ray parameters is classified, and the confusion matrix printed.

    python examples/multipath_classify.py [--ms 1000] [--cn0 50] [--k 5]

Every scene: PRN 3 clean; PRN 16 with a ray in phase from 300 ms on; PRN 22 with a slowly fading
ray all the time; PRN 26 without a direct signal, only a ray. The training scenes differ in their
noise seed and in the rays' delay and gain; the held-out scene lies between them.
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
# (noise seed, the ray's delay in chips and gain for PRN 16 / 22, the same for PRN 26)
TRAIN = [(6102, 0.50, 0.50, 0.40, 0.70), (6201, 0.40, 0.60, 0.30, 0.60), (6302, 0.60, 0.45, 0.50, 0.80)]
HELD_OUT = (7203, 0.45, 0.55, 0.35, 0.65)


def windows_of(ctx, args, seed, delay, gain, nlos_delay, nlos_gain):
    """One scene -> (table [windows][7], labels [windows])"""
    file, signal, acq, track, _, _ = sdr.initParameters()
    file.skip = 2
    S = sdr.synth
    at = [S.OPENSKY_SV.index(p) for p in SVS]
    cd = [S.OPENSKY_CODEDELAY[i] for i in at]
    ff = [float(S.OPENSKY_FINEFREQ[i]) for i in at]
    scene = S.scene_of(S.scenario(SVS, cd, [f - signal.IF for f in ff], [args.cn0] * len(SVS), skip_ms=file.skip,
                                  seed=seed))
    S.add_ray(scene, 16, delay, gain, t_on_ms=file.skip + 300)
    S.add_ray(scene, 22, delay, gain, fade_hz=2.0)
    S.set_nlos(scene, 26)
    S.add_ray(scene, 26, nlos_delay, nlos_gain)
    dev = sdr.DeviceRecord(ctx, 2 * (file.skip + 1 + args.ms + 4) * signal.Sample)
    S.generate_scene_device(ctx, scene, dev)
    file.dev = dev
    Acquired = SimpleNamespace(sv=np.array(SVS), SNR=np.full(len(SVS), 20.0), Doppler=np.zeros(len(SVS)),
                               codedelay=np.array(cd), fineFreq=np.array(ff))
    tck, _ = sdr.trackingCT_multiCorr(file, signal, track, Acquired, datalength=args.ms, ctx=ctx)
    dev.free()
    X = sdr.feature_table(sdr.acf_features(tck, SVS, [45.0] * len(SVS)), sdr.acf_fit(tck, SVS))
    return X, np.concatenate(sdr.scene_labels(scene, tck, SVS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ms", type=int, default=1000, help="1-ms steps to track per scene")
    ap.add_argument("--cn0", type=float, default=50.0, help="C/N0 of every satellite, dB-Hz")
    ap.add_argument("--k", type=int, default=5, help="neighbours that vote")
    args = ap.parse_args()

    ctx = sdr.Context(0)
    sets = [windows_of(ctx, args, *s) for s in TRAIN]
    X, y = np.vstack([s[0] for s in sets]), np.concatenate([s[1] for s in sets])
    model = sdr.knn_train(X, y, ctx=ctx)  # standardised, uploaded once
    print(f"training table: {model.M} windows x {model.D} columns (F1 F2 F3 F4 F5 bias ratio), {model.dropped} dropped; "
          f"per class {np.bincount(model.label, minlength=3).tolist()}")
    Xh, yh = windows_of(ctx, args, *HELD_OUT)
    r = sdr.knn_classify(model, Xh, k=args.k, want_neighbours=True)
    model.free()
    print(" win truth label  votes      nearest d2")
    for m, (t, p, v, d) in enumerate(zip(yh, r.label, r.votes, r.nn_d2[:, 0])):
        print(f"{m:4d} {int(t):5d} {int(p):5d}  {v.tolist()}  {d:10.4f}")
    print("confusion (rows: truth 0 1 2; columns: predicted 0 1 2, then no label)")
    print(sdr.confusion(yh, r.label))
    ctx.close()


if __name__ == "__main__":
    main()
