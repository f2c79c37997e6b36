"""Tracking-only driver for profiling: cfg3-shape (8 channels) with a short 1-ms
phase so the 10-ms correlator kernel dominates. Args: N1 N10 [ntaps] [nch]."""
import importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("assignment-for-aae6102_gnss-sdr_amd")
N1 = int(sys.argv[1]) if len(sys.argv) > 1 else 100
N10 = int(sys.argv[2]) if len(sys.argv) > 2 else 4000
ntaps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
nch = int(sys.argv[4]) if len(sys.argv) > 4 else 8
ctx = pkg.Context(0)
file, signal, acq, track, _, _ = pkg.initParameters()
skip = 0
cfg = pkg.synth.opensky(skip_ms=skip) if nch <= 8 else pkg.synth.all_prn(nch, skip_ms=skip)
dev = pkg.DeviceRecord(ctx, (skip + N1 + 19 + N10 + 3) * 58000 * 2)
pkg.synth.generate_device(ctx, cfg, dev)
file.skip, file.dev = skip, dev
from types import SimpleNamespace
S = 58000
cds = pkg.synth.codedelays(cfg, skip)
A = SimpleNamespace(sv=np.array([cfg.sv[i].prn for i in range(nch)]), SNR=np.zeros(nch), Doppler=np.zeros(nch),
                    codedelay=np.array(cds[:nch]), fineFreq=np.array([4.58e6 + cfg.sv[i].doppler_hz for i in range(nch)]))
track.msToProcessCT_1ms, track.msToProcessCT_10ms = N1, N10
taps = None if ntaps == 3 else np.array([-0.5, -0.4, -0.3, -0.2, -0.1, 0.0, 0.1, 0.2, 0.3, 0.4, 0.5])
if os.environ.get("TRK_SUB"):  # lane span 8 * v samples (GNSS_OPT_FORCE_SUB; A/B of the lane geometry)
    ctx.set_option(pkg.abi.OPT_FORCE_SUB, int(os.environ["TRK_SUB"]))
if os.environ.get("TRK_SLOT"):  # GNSS_OPT_SLOT_PATH: 1 = the <= 3-tap prefixes through the LDS slots, 2 = registers
    ctx.set_option(pkg.abi.OPT_SLOT_PATH, int(os.environ["TRK_SLOT"]))
if os.environ.get("TRK_SPACING"):  # E/P/L at +- this many chips (track.CorrelatorSpacing and the taps)
    track.CorrelatorSpacing = float(os.environ["TRK_SPACING"])
    taps = np.array([-track.CorrelatorSpacing, 0.0, track.CorrelatorSpacing])
if os.environ.get("TRK_PROFILE"):
    ctx.set_profiling(True)  # per-launch hipEvents: track10_kernel_ms = the 10-ms launch(es)
for it in range(int(os.environ.get('TRK_ITERS', '2'))):
    t = time.perf_counter()
    buf = pkg.trackingCT(file, signal, track, A, ctx=ctx, taps=taps, raw=True)
    tm = ctx.timing()
    print("track wall", round(time.perf_counter() - t, 4), "track10_kernel_ms", round(tm["track10_kernel_ms"], 3),
          "track_kernel_ms", round(tm["track_kernel_ms"], 3), "launches", tm["track_launches"], flush=True)
if os.environ.get("TRK_HASH"):  # a digest of every record / tap value of the last call (A/B bit-identity)
    import hashlib
    h = hashlib.sha256(np.ascontiguousarray(buf.rec).tobytes())
    if getattr(buf, "taps", None) is not None:
        h.update(np.ascontiguousarray(buf.taps).tobytes())
    print("records sha256", h.hexdigest()[:16], flush=True)
