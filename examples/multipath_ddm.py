"""A reflected ray with a Doppler offset, found in the delay-Doppler map of replayed tracking rows:
the Opensky scenario with PRN 16's ray 0.9 chip late at 0.8 of the amplitude, its carrier 20 Hz above
the direct one. The GIVEN loop tracks 260 ms at its 25 taps; rows 150-249 are correlated again at
-1.5:0.05:1.5 chip (gnss_replay_correlate) and those sums, still in HBM, are summed coherently per
(tap, Doppler offset) at -50:10:50 Hz with one rotation per row (gnss_replay_ddm). Over the 100-ms
window the ray turns two whole cycles: it is absent from the zero-offset row of the map, which is all
replay_coherent and the two-path fit see, and stands at (-0.9 chip, +20 Hz). Printed: the direct and
the secondary peak, and the map's magnitude over the direct peak's around both.

    python examples/multipath_ddm.py [--host]

--host runs the replay and the map on the CPU (the loop itself still needs the GPU).
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

PRN, SKIP, ROWS, WINDOW = 16, 5, 260, range(150, 250)
DELAY, GAIN, FADE_HZ = 0.9, 0.8, 20.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true", help="replay and map on the host path")
    args = ap.parse_args()

    file, signal, acq, track, _, _ = sdr.initParameters()
    S = sdr.synth
    cfg = S.opensky(skip_ms=SKIP)
    i = S.OPENSKY_SV.index(PRN)
    A = SimpleNamespace(sv=np.array([PRN]), SNR=np.array([20.0]), Doppler=np.zeros(1),
                        codedelay=np.array([S.codedelays(cfg, SKIP)[i]]), fineFreq=np.array([float(S.OPENSKY_FINEFREQ[i])]))
    wide = sdr.colon(-1.5, 0.05, 1.5)
    hz = np.arange(-50.0, 51.0, 10.0)
    ctx = sdr.Context(0)
    dev = sdr.DeviceRecord(ctx, 2 * (SKIP + ROWS + 6) * signal.Sample)
    file.skip = SKIP
    scene = S.scene_of(cfg)
    S.add_ray(scene, PRN, DELAY, GAIN, phase_cycles=0.25, fade_hz=FADE_HZ)
    S.generate_scene_device(ctx, scene, dev)
    file.dev, file.data = dev, None
    buf = sdr.trackingCT_multiCorr(file, signal, track, A, datalength=ROWS, ctx=ctx, raw=True)
    rows = sdr.replay_rows(buf, A, file, signal, loop="given", rows=WINDOW)
    if args.host:
        file.dev, file.data = None, dev.download()
    use = None if args.host else ctx
    sums, replay_ms = sdr.replay_correlate(file, signal, rows, wide, ctx=use, device_out=not args.host)
    ddm = sdr.replay_ddm(sums, rows, hz, u=wide, prompt=None, rows_per_window=len(WINDOW), signal=signal, file=file,
                         ctx=use, excl_chips=0.3, excl_hz=10.0)
    dev.free()
    ctx.close()

    print(f"{len(WINDOW)} rows x {len(wide)} taps x {len(hz)} bins"
          + (" on the host" if args.host else f": replay kernel {replay_ms:.3f} ms, map kernels {ddm.kernel_ms:.3f} ms"))
    z = np.hypot(ddm.map[0][0, 0], ddm.map[0][0, 1])  # [bins][taps]
    top = np.sqrt(ddm.peak_pow[0][0])
    print(f"direct peak:    {ddm.peak_chips[0][0]:+.2f} chip, {ddm.peak_hz[0][0]:+.0f} Hz")
    print(f"secondary peak: {ddm.sec_chips[0][0]:+.2f} chip, {ddm.sec_hz[0][0]:+.0f} Hz at "
          f"{np.sqrt(ddm.sec_pow[0][0]) / top:.3f} of the direct one (a ray {DELAY} chip late at gain {GAIN}, "
          f"{FADE_HZ:+.0f} Hz, stands at tap {-DELAY:+.2f})")
    cols = [int(np.argmin(np.abs(wide - t))) for t in (-1.2, -0.9, -0.6, -0.3, 0.0, 0.3)]
    print("    Hz | " + " ".join(f"{wide[k]:+6.2f}" for k in cols))
    for m, f in enumerate(hz):
        print(f"{f:+6.0f} | " + " ".join(f"{z[m, k] / top:6.3f}" for k in cols))


if __name__ == "__main__":
    main()
