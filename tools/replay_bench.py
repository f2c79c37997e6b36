"""Timing driver for gnss_replay_correlate: 8 Opensky channels x 1 000 rows of the GIVEN loop
(trackingCT_multiCorr-GIVEN.m), replayed (a) at the loop's own 25 taps and (b) at -1.5:0.05:1.5
(61 taps), the record resident in HBM. In one process, after 3 warm-ups of each, 10 alternating
rounds of (a), (b) and (c) the closed 25-tap loop over the same rows
(gnss_tracking_ct_multicorr; gnss_last_timing().track_ms, the whole call on a resident record); the
medians. Then three closed loops in profiling mode for track_kernel_ms (the sum of the step
kernels, which that mode launches one by one). Once:
the host path (no context, up to 16 threads) over the same rows at the 25 taps, under a host clock.
kernel_ms is gnss_replay_out.kernel_ms (hipEvents around the kernel). The operations are counted
from the shapes and csrc/replay.h: per sample the carrier wipe (~60 fp64 VALU operations), per
tap-sample the colon element, ceil, its conversion, two signed adds (5) and the two sign selects
(2). Shares: of the fp64 VALU peak without contraction (one operation per instruction: half the
78.6 TFLOP/s FMA peak) and of the 8 TB/s HBM peak for the bytes the call needs once (the rows'
samples, the table, the sums). Prints one JSON line. Args: [ROUNDS] [--no-host] [OUTFILE]."""
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (PyTorch's runtime first)

pkg = importlib.import_module("assignment-for-aae6102_gnss-sdr_amd")
from types import SimpleNamespace  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
ROUNDS = int(args[0]) if args and args[0].isdigit() else 10
OUT = next((a for a in args if not a.isdigit()), None)
HOST = "--no-host" not in sys.argv[1:]
WARM, ROWS, SKIP = 3, 1000, 5
OPS_SAMPLE, OPS_TAP = 60, 7
VALU_PEAK = 78.6e12 / 2  # fp64 operations per second without FMA contraction
HBM_PEAK = 8.0e12

sdr, synth = pkg.sdr, pkg.synth
ctx = pkg.Context(0)
cfg = synth.opensky(skip_ms=SKIP)
file, signal, _, track, _, _ = pkg.initParameters()
rec = pkg.DeviceRecord(ctx, 2 * (SKIP + ROWS + 8) * 58000)
synth.generate_device(ctx, cfg, rec)
file.skip, file.dev = SKIP, rec
n_sv = len(synth.OPENSKY_SV)
A = SimpleNamespace(sv=np.array(synth.OPENSKY_SV), SNR=np.full(n_sv, 20.0), Doppler=np.zeros(n_sv),
                    codedelay=np.array(synth.codedelays(cfg, SKIP)), fineFreq=np.array(synth.OPENSKY_FINEFREQ, dtype=float))


def closed_loop():
    buf = sdr.trackingCT_multiCorr(file, signal, track, A, datalength=ROWS, ctx=ctx, raw=True)
    t = ctx.timing()
    return buf, t["track_kernel_ms"], t["track_ms"]


buf, _, _ = closed_loop()
rows = sdr.replay_rows(buf, A, file, signal, loop="given")
taps = {"taps25": rows.taps, "taps61": sdr.colon(-1.5, 0.05, 1.5)}
samples = int(rows.numSample.sum())
ms = {k: [] for k in taps}
loop_wall = []
for r in range(WARM + ROUNDS):
    for k, tp in taps.items():
        out, kms = sdr.replay_correlate(file, signal, rows, tp, ctx=ctx)
        if r >= WARM:
            ms[k].append(kms)
        if k == "taps25" and r == 0:
            scale = float(np.sqrt(np.mean(buf.rec[:, 0, :ROWS] ** 2 + buf.rec[:, 1, :ROWS] ** 2)))
            err25 = float(np.max(np.abs(out - buf.taps[:, :, :, :ROWS])) / scale)
    _, lk, lw = closed_loop()
    if r >= WARM:
        loop_wall.append(lw)

res = {"workload": f"{len(A.sv)} channels x {ROWS} GIVEN rows", "samples": samples, "rounds": ROUNDS,
       "replay25_vs_records": err25}
for k, tp in taps.items():
    nt, med = len(tp), statistics.median(ms[k])
    ops = samples * (OPS_SAMPLE * ((nt + 31) // 32) + OPS_TAP * nt)
    nbytes = 2 * samples + rows.numSample.size * 48 + 16 * nt * rows.numSample.size
    res[k] = {"n_taps": nt, "kernel_ms": med, "kernel_ms_min": min(ms[k]), "kernel_ms_max": max(ms[k]),
              "tap_samples_per_s": samples * nt / (med * 1e-3), "fp64_ops": ops,
              "share_fp64_valu_uncontracted": ops / (med * 1e-3) / VALU_PEAK,
              "share_hbm": nbytes / (med * 1e-3) / HBM_PEAK}
# the loop's kernels alone are summed in profiling mode only (one bracketed launch per step): a pass of its own
ctx.set_profiling(True)
prof = [closed_loop()[1] for _ in range(3)]
ctx.set_profiling(False)
res["closed_loop_25"] = {"track_ms": statistics.median(loop_wall), "track_kernel_ms_profiling": statistics.median(prof)}
if HOST:
    dev25, _ = sdr.replay_correlate(file, signal, rows, taps["taps25"], ctx=ctx)
    file.dev, file.data = None, rec.download()
    t0 = time.perf_counter()
    h, _ = sdr.replay_correlate(file, signal, rows, taps["taps25"])
    res["host_path_25"] = {"wall_ms": (time.perf_counter() - t0) * 1e3, "threads": min(16, os.cpu_count() or 1),
                           "vs_device": float(np.max(np.abs(h - dev25)) / scale)}
rec.free()
ctx.close()
line = json.dumps(res)
print(line)
if OUT:
    open(OUT, "w").write(line + "\n")
