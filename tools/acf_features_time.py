"""Timing driver for gnss_acf_features on device-resident records of the config-5 size (32
channels x 91 000 rows x 25 taps: 1.16 GB of tap sums and 0.42 GB of loop records in HBM, seeded,
generated on the device). In one process, after a warm-up call:
  1. the device call, ITERS times: a host clock around the call, which ends in a synchronise of
     the context's stream (so the kernels, the features' download and the host's F1 are inside);
  2. gnss_dev_download of the same taps + rec arrays into pinned host memory, ITERS times: the
     least any route that runs the script on the host must pay before it computes anything;
  3. the host path on the downloaded arrays, once, and the two results compared bit for bit.
With --trace the process makes the warm-up call and two more and nothing else: run it under
`rocprofv3 --kernel-trace --stats -- python tools/acf_features_time.py --trace` for the kernels'
durations, from which the row pass's bytes / time follow (the bytes are printed here).
Args: [--trace] [ITERS] [OUTFILE]."""
import ctypes as C
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import torch  # noqa: E402  (PyTorch's runtime first)

pkg = importlib.import_module("assignment-for-aae6102_gnss-sdr_amd")
import srcdigest  # noqa: E402

args = [a for a in sys.argv[1:] if a != "--trace"]
TRACE = "--trace" in sys.argv[1:]
ITERS = int(args[0]) if args else 7
OUT = args[1] if len(args) > 1 else None
N, L, TAPS = 32, 91000, pkg.abi.MC_TAPS
abi = pkg.abi
ctx = pkg.Context(0)
lib = ctx.lib
dev = torch.device("cuda:0")
torch.manual_seed(20240611)
# a correlation triangle about the prompt tap on a random carrier phase, plus noise
tri = 4000.0 * torch.clamp(1 - (torch.arange(TAPS, device=dev, dtype=torch.float64) - 12).abs() * 0.05, min=0)
phase = torch.rand((N, 1, L), device=dev, dtype=torch.float64) * 6.283185307179586
taps = torch.randn((N, 2, TAPS, L), device=dev, dtype=torch.float64) * 1500.0
taps[:, 0] += tri[None, :, None] * torch.cos(phase)
taps[:, 1] += tri[None, :, None] * torch.sin(phase)
rec = torch.randn((N, abi.NFIELDS, L), device=dev, dtype=torch.float64)
del phase
torch.cuda.synchronize()
lens = torch.full((N,), L, dtype=torch.int64).numpy()

cfg = abi.GnssAcfCfg()
cfg.n, cfg.ind_start, cfg.numOverLap = N, abi.ACF_DEFAULTS["ind_start"], abi.ACF_DEFAULTS["numOverLap"]
cfg.corrSpacing, cfg.maxDelay = abi.ACF_DEFAULTS["corrSpacing"], abi.ACF_DEFAULTS["maxDelay"]
cfg.a[:] = list(abi.ACF_DEFAULTS["a"])
cfg.prn[:N], cfg.ele[:N] = list(range(1, N + 1)), [5.0 + 2.5 * i for i in range(N)]
CAP = (L - 1) // 100


def track_out(rec_ptr, taps_ptr, flags):
    o = abi.GnssTrackOut()
    o.max_len = L
    o.rec = C.cast(C.c_void_p(rec_ptr), C.POINTER(C.c_double))
    o.taps = C.cast(C.c_void_p(taps_ptr), C.POINTER(C.c_double))
    o.len = lens.ctypes.data_as(C.POINTER(C.c_int64))
    o.flags = flags
    return o


class Out:
    def __init__(self):
        import numpy as np
        self.windows = np.zeros(N, dtype=np.int64)
        self.arr = {f: np.zeros((N, CAP)) for f in abi.ACF_FIELDS}
        o = abi.GnssAcfOut()
        o.cap = CAP
        o.windows = self.windows.ctypes.data_as(C.POINTER(C.c_int64))
        for f in abi.ACF_FIELDS:
            setattr(o, f, self.arr[f].ctypes.data_as(C.POINTER(C.c_double)))
        self.c = o


def call(h, records, out):
    t = time.perf_counter()
    st = lib.gnss_acf_features(h, C.byref(cfg), C.byref(records), TAPS, C.byref(out.c))
    dt = time.perf_counter() - t
    if st != abi.OK:
        raise abi.GnssError(st, (lib.gnss_last_error(h) or b"").decode() if h else "")
    return dt * 1e3


d_rec = track_out(rec.data_ptr(), taps.data_ptr(), abi.OUT_DEVICE)
d_out = Out()
call(ctx.h, d_rec, d_out)  # warm-up: code objects, the context's scratch and pinned staging
if TRACE:
    call(ctx.h, d_rec, d_out), call(ctx.h, d_rec, d_out)
    ctx.close()
    sys.exit(0)

t_call = [call(ctx.h, d_rec, d_out) for _ in range(ITERS)]
h_taps = torch.empty(taps.shape, dtype=torch.float64, pin_memory=True)
h_rec = torch.empty(rec.shape, dtype=torch.float64, pin_memory=True)


def download():
    t = time.perf_counter()
    for dst, src in ((h_taps, taps), (h_rec, rec)):
        ctx.check(lib.gnss_dev_download(ctx.h, C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()),
                                        C.c_uint64(src.numel() * 8)))
    return (time.perf_counter() - t) * 1e3


download()
t_down = [download() for _ in range(ITERS)]
h_out = Out()
t_host = call(None, track_out(h_rec.data_ptr(), h_taps.data_ptr(), 0), h_out)
same = bool((d_out.windows == h_out.windows).all()) and all(
    d_out.arr[f].tobytes() == h_out.arr[f].tobytes() for f in abi.ACF_FIELDS)

tap_bytes = N * 2 * TAPS * L * 8
row_out = N * L * (8 + 1)
med = statistics.median
lines = [f"src_digest {srcdigest.src_digest()} commit {srcdigest.head_commit()}",
         f"{N} channels x {L} rows x {TAPS} taps, device-resident, seeded; {int(d_out.windows.sum())} windows; "
         f"{ITERS} timed calls after one warm-up",
         f"taps {tap_bytes / 1e9:.4f} GB, rec {N * abi.NFIELDS * L * 8 / 1e9:.4f} GB; the row pass reads the taps once "
         f"and writes {row_out / 1e6:.1f} MB (prompt magnitude + index per row): {(tap_bytes + row_out) / 1e9:.4f} GB",
         f"(1) device call (host clock, ends in a stream synchronise), ms: median {med(t_call):.3f} min "
         f"{min(t_call):.3f} max {max(t_call):.3f}",
         f"(3) gnss_dev_download of taps + rec into pinned memory, ms: median {med(t_down):.3f} min "
         f"{min(t_down):.3f} max {max(t_down):.3f}",
         f"    host path on the downloaded arrays, one call, ms: {t_host:.1f}",
         f"device features == host features bit for bit: {same}",
         f"acceptance (1) < (3): {med(t_call) < med(t_down)}"]
text = "\n".join(lines) + "\n"
print(text)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write(text)
ctx.close()
sys.exit(0 if same else 1)
