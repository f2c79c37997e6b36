"""Timing driver for gnss_acf_fit on device-resident records of the config-5 size (32 channels x
91 000 rows x 25 taps: 1.16 GB of tap sums in HBM, seeded, generated on the device; 29 088 windows
of 81 + 7 776 hypotheses at the default grid). In one process, after a warm-up of each:
  ROUNDS alternating rounds of (a) the device call and (b) the host path (up to 16 threads) on a
  pinned host copy of the same taps, each under a host clock (the device call ends in a
  synchronise of the context's stream, so the kernel and the rows' download are inside); the
  medians; the two results compared bit for bit.
With --trace the process makes the warm-up device call and two more and nothing else: run it under
`rocprofv3 --kernel-trace --stats -- python tools/acf_fit_time.py --trace` for the kernel's
duration. The operations and bytes the definition needs are counted here from the shapes.
Args: [--trace] [ROUNDS] [OUTFILE]."""
import ctypes as C
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (PyTorch's runtime first)

pkg = importlib.import_module("assignment-for-aae6102_gnss-sdr_amd")
import srcdigest  # noqa: E402

args = [a for a in sys.argv[1:] if a != "--trace"]
TRACE = "--trace" in sys.argv[1:]
ROUNDS = int(args[0]) if args else 3
OUT = args[1] if len(args) > 1 else None
N, L, TAPS = 32, 91000, pkg.abi.MC_TAPS
abi = pkg.abi
ctx = pkg.Context(0)
lib = ctx.lib
dev = torch.device("cuda:0")
torch.manual_seed(20240611)
# a correlation triangle about the prompt tap and half of it half a chip later, on a random
# carrier phase per row, plus noise
j = torch.arange(TAPS, device=dev, dtype=torch.float64)
tri = 4000.0 * (torch.clamp(1 - (j - 12).abs() * 0.05, min=0) + 0.5 * torch.clamp(1 - (j - 22).abs() * 0.05, min=0))
phase = torch.rand((N, 1, L), device=dev, dtype=torch.float64) * 6.283185307179586
taps = torch.randn((N, 2, TAPS, L), device=dev, dtype=torch.float64) * 1500.0
taps[:, 0] += tri[None, :, None] * torch.cos(phase)
taps[:, 1] += tri[None, :, None] * torch.sin(phase)
del phase
torch.cuda.synchronize()
lens = np.full(N, L, dtype=np.int64)
D = abi.ACF_FIT_DEFAULTS
CAP = (L - D["ind_start"]) // D["numOverLap"]

cfg = abi.GnssAcfFitCfg()
cfg.n, cfg.orient = N, -1
for k, v in D.items():
    setattr(cfg, k, v)


def track_out(taps_ptr, flags):
    o = abi.GnssTrackOut()
    o.max_len = L
    o.taps = C.cast(C.c_void_p(taps_ptr), C.POINTER(C.c_double))
    o.len = lens.ctypes.data_as(C.POINTER(C.c_int64))
    o.flags = flags
    return o


class Out:
    def __init__(self):
        self.windows = np.zeros(N, dtype=np.int64)
        self.paths = np.zeros((N, CAP), dtype=np.int32)
        self.arr = {f: np.zeros((N, CAP)) for f in abi.ACF_FIT_FIELDS}
        o = abi.GnssAcfFitOut()
        o.cap = CAP
        o.windows = self.windows.ctypes.data_as(C.POINTER(C.c_int64))
        o.paths = self.paths.ctypes.data_as(C.POINTER(C.c_int32))
        for f in abi.ACF_FIT_FIELDS:
            setattr(o, f, self.arr[f].ctypes.data_as(C.POINTER(C.c_double)))
        self.c = o


def call(h, records, out):
    t = time.perf_counter()
    st = lib.gnss_acf_fit(h, C.byref(cfg), C.byref(records), TAPS, C.byref(out.c))
    dt = time.perf_counter() - t
    if st != abi.OK:
        raise abi.GnssError(st, (lib.gnss_last_error(h) or b"").decode() if h else "")
    return dt * 1e3


d_rec = track_out(taps.data_ptr(), abi.OUT_DEVICE)
d_out = Out()
call(ctx.h, d_rec, d_out)  # warm-up: the code object, the context's scratch and pinned staging
if TRACE:
    call(ctx.h, d_rec, d_out), call(ctx.h, d_rec, d_out)
    ctx.close()
    sys.exit(0)

h_taps = torch.empty(taps.shape, dtype=torch.float64, pin_memory=True)
ctx.check(lib.gnss_dev_download(ctx.h, C.c_void_p(h_taps.data_ptr()), C.c_void_p(taps.data_ptr()),
                                C.c_uint64(taps.numel() * 8)))
h_rec = track_out(h_taps.data_ptr(), 0)
h_out = Out()
t_dev, t_host = [], []
for _ in range(ROUNDS):
    t_dev.append(call(ctx.h, d_rec, d_out))
    t_host.append(call(None, h_rec, h_out))
same = bool((d_out.windows == h_out.windows).all()) and d_out.paths.tobytes() == h_out.paths.tobytes() and all(
    d_out.arr[f].tobytes() == h_out.arr[f].tobytes() for f in abi.ACF_FIT_FIELDS)

# what the definition needs, from the shapes: fp64 adds, subtracts and multiplies (a compare, a
# select and |x| not counted; a division as one)
W = int(d_out.windows.sum())
P, E = D["p_count"], D["e_count"]
two = TAPS * (4 + 7 + 7) + 3 + 4 * 4 + 6 + 2 + TAPS * (4 + 8 + 3 + 1)  # sums, det, A0/A1, the ratio test, residual
one = TAPS * (2 + 3 + 3) + 2 + TAPS * (2 + 4 + 3 + 1)
flop = W * (P * E * two + P * one + 2 * 50 * D["numOverLap"])
tap_bytes = W * D["numOverLap"] * 2 * TAPS * 8
med = statistics.median
lines = [f"src_digest {srcdigest.src_digest()} commit {srcdigest.head_commit()}",
         f"{N} channels x {L} rows x {TAPS} taps, device-resident, seeded; {W} windows of {P} + {P * E} hypotheses; "
         f"{ROUNDS} alternating rounds after one warm-up of each",
         f"per two-path hypothesis {two} fp64 operations, per one-path hypothesis {one}: {flop / 1e9:.1f} GFLOP in all; "
         f"the windows' tap sums {tap_bytes / 1e9:.4f} GB, read once",
         f"(a) device call (host clock, ends in a stream synchronise), ms: median {med(t_dev):.3f} min "
         f"{min(t_dev):.3f} max {max(t_dev):.3f}",
         f"(b) host path on a pinned host copy of the taps, ms: median {med(t_host):.1f} min {min(t_host):.1f} "
         f"max {max(t_host):.1f}",
         f"paths: {int((d_out.paths == 2).sum())} windows two-path, {int((d_out.paths == 1).sum())} one-path",
         f"device outputs == host outputs bit for bit: {same}"]
text = "\n".join(lines) + "\n"
print(text)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write(text)
ctx.close()
sys.exit(0 if same else 1)
