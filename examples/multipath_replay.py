"""A reflected ray outside the 25-tap window, found by replaying recorded tracking rows on a wider
tap grid: the Opensky scenario with PRN 16's ray 0.9 chip late at half the amplitude, in quadrature.
The GIVEN loop tracks 260 ms at its 25 taps (-0.6:0.05:0.6 chip); rows 150-249 are then correlated
again at -1.5:0.05:1.5 (gnss_replay_correlate: no loop is closed, every row starts from the NCO state
the loop recorded) and summed with the prompt's sign. Printed per tap: the clean scene's and the ray
scene's correlation magnitude over the prompt's, with the 25-tap record's own value where it has one.
A tap delays the replica, so the late ray stands at the negative taps.

    python examples/multipath_replay.py [--host]

--host runs the replay on the CPU (the loop itself still needs the GPU).
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


def profile(taps_out, prompt_i):
    z = sdr.replay_coherent(taps_out, prompt_i, len(WINDOW))[0, :, :, 0]
    return np.hypot(z[0], z[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true", help="replay on the host path")
    args = ap.parse_args()

    file, signal, acq, track, _, _ = sdr.initParameters()
    S = sdr.synth
    cfg = S.opensky(skip_ms=SKIP)
    i = S.OPENSKY_SV.index(PRN)
    A = SimpleNamespace(sv=np.array([PRN]), SNR=np.array([20.0]), Doppler=np.zeros(1),
                        codedelay=np.array([S.codedelays(cfg, SKIP)[i]]), fineFreq=np.array([float(S.OPENSKY_FINEFREQ[i])]))
    wide = sdr.colon(-1.5, 0.05, 1.5)
    ctx = sdr.Context(0)
    dev = sdr.DeviceRecord(ctx, 2 * (SKIP + ROWS + 6) * signal.Sample)
    file.skip = SKIP
    m25, m61 = {}, {}
    for ray in (False, True):
        scene = S.scene_of(cfg)
        if ray:
            S.add_ray(scene, PRN, 0.9, 0.5, phase_cycles=0.25)
        S.generate_scene_device(ctx, scene, dev)
        file.dev, file.data = dev, None
        buf = sdr.trackingCT_multiCorr(file, signal, track, A, datalength=ROWS, ctx=ctx, raw=True)
        rows = sdr.replay_rows(buf, A, file, signal, loop="given", rows=WINDOW)
        if args.host:
            file.dev, file.data = None, dev.download()
        out, ms = sdr.replay_correlate(file, signal, rows, wide, ctx=None if args.host else ctx)
        prompt = buf.rec[:, sdr.abi.FIELDS.index("P_i"), WINDOW.start: WINDOW.stop]
        m61[ray] = profile(out, prompt)
        m25[ray] = profile(buf.taps[:, :, :, WINDOW.start: WINDOW.stop], prompt)
        print(f"{'ray' if ray else 'clean'} scene: {len(WINDOW)} rows x {len(wide)} taps replayed"
              + (f", kernel {ms:.3f} ms" if not args.host else " on the host"))
    dev.free()
    ctx.close()

    own = {round(float(t), 2): k for k, t in enumerate(rows.taps)}
    p61 = int(np.argmin(np.abs(wide)))
    print("   tap | 25-tap record: clean    ray | replay: clean    ray")
    for k, t in enumerate(wide):
        j = own.get(round(float(t), 2))
        rec = (f"{m25[False][j] / m25[False][12]:7.3f} {m25[True][j] / m25[True][12]:6.3f}" if j is not None
               else "      -      -")
        print(f"{t:6.2f} | {rec:>28s} | {m61[False][k] / m61[False][p61]:13.3f} {m61[True][k] / m61[True][p61]:6.3f}")


if __name__ == "__main__":
    main()
