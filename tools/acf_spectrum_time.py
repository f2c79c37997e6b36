"""Timing driver for gnss_acf_features_ext on device-resident records of the config-5 size (32
channels x 91 000 rows x 25 taps, seeded, generated on the device as tools/acf_features_time.py
does; the prompt tap's amplitude swings at 3 Hz so that the spectra have a line). In one process,
after a warm-up call of each:
  1. the device call of gnss_acf_features (F1-F5 alone) and of gnss_acf_features_ext, ITERS times
     each, alternating: a host clock around the call, which ends in a synchronise of the context's
     stream (the kernels, the downloads and the host's stores inside);
  2. the host path of gnss_acf_features_ext on a pinned host copy of the same arrays, once, and the
     two results compared bit for bit.
With --trace the process makes the warm-up call and two more of gnss_acf_features_ext and nothing
else: run it under `rocprofv3 --kernel-trace --stats -- python tools/acf_spectrum_time.py --trace`
for the durations of acf_spectrum_kernel and of the counting row pass.
Args: [--trace] [ITERS] [OUTFILE]."""
import ctypes as C
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import torch  # noqa: E402  (PyTorch's runtime first)

pkg = importlib.import_module("assignment-for-aae6102_gnss-sdr_amd")
import srcdigest  # noqa: E402

args = [a for a in sys.argv[1:] if a != "--trace"]
TRACE = "--trace" in sys.argv[1:]
ITERS = int(args[0]) if args else 5
OUT = args[1] if len(args) > 1 else None
N, L, TAPS = 32, 91000, pkg.abi.MC_TAPS
abi = pkg.abi
ctx = pkg.Context(0)
lib = ctx.lib
dev = torch.device("cuda:0")
torch.manual_seed(20240611)
tri = 4000.0 * torch.clamp(1 - (torch.arange(TAPS, device=dev, dtype=torch.float64) - 12).abs() * 0.05, min=0)
swing = 1 + 0.3 * torch.cos(6.283185307179586 * 3.0 * 1e-3 * torch.arange(L, device=dev, dtype=torch.float64))
phase = torch.rand((N, 1, L), device=dev, dtype=torch.float64) * 6.283185307179586
taps = torch.randn((N, 2, TAPS, L), device=dev, dtype=torch.float64) * 1500.0
taps[:, 0] += tri[None, :, None] * swing[None, None, :] * torch.cos(phase)
taps[:, 1] += tri[None, :, None] * swing[None, None, :] * torch.sin(phase)
rec = torch.randn((N, abi.NFIELDS, L), device=dev, dtype=torch.float64)
del phase
torch.cuda.synchronize()
lens = torch.full((N,), L, dtype=torch.int64).numpy()

cfg = abi.GnssAcfCfg()
cfg.n, cfg.ind_start, cfg.numOverLap = N, abi.ACF_DEFAULTS["ind_start"], abi.ACF_DEFAULTS["numOverLap"]
cfg.corrSpacing, cfg.maxDelay = abi.ACF_DEFAULTS["corrSpacing"], abi.ACF_DEFAULTS["maxDelay"]
cfg.a[:] = list(abi.ACF_DEFAULTS["a"])
cfg.prn[:N], cfg.ele[:N] = list(range(1, N + 1)), [5.0 + 2.5 * i for i in range(N)]
xcfg = abi.GnssAcfExtCfg()
xcfg.fft_hist, xcfg.fft_n, xcfg.fft_fill = (abi.ACF_EXT_DEFAULTS[k] for k in ("fft_hist", "fft_n", "fft_fill"))
xcfg.fs = 1000.0 / cfg.numOverLap
CAP = (L - 1) // 100
FIELDS = list(abi.ACF_FIELDS) + list(abi.ACF_EXT_FIELDS)


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
        self.windows = np.zeros(N, dtype=np.int64)
        self.arr = {f: np.zeros((N, CAP)) for f in FIELDS}
        self.c, self.x = abi.GnssAcfOut(), abi.GnssAcfExtOut()
        self.c.cap = CAP
        self.c.windows = self.windows.ctypes.data_as(C.POINTER(C.c_int64))
        for f in FIELDS:
            setattr(self.x if f in abi.ACF_EXT_FIELDS else self.c, f, self.arr[f].ctypes.data_as(C.POINTER(C.c_double)))


def call(h, records, out, ext=True):
    t = time.perf_counter()
    if ext:
        st = lib.gnss_acf_features_ext(h, C.byref(cfg), C.byref(xcfg), C.byref(records), TAPS, C.byref(out.c),
                                       C.byref(out.x))
    else:
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

p_out = Out()
call(ctx.h, d_rec, p_out, ext=False)
t_plain, t_ext = [], []
for _ in range(ITERS):
    t_plain.append(call(ctx.h, d_rec, p_out, ext=False))
    t_ext.append(call(ctx.h, d_rec, d_out))
h_taps = torch.empty(taps.shape, dtype=torch.float64, pin_memory=True)
h_rec = torch.empty(rec.shape, dtype=torch.float64, pin_memory=True)
for dst, src in ((h_taps, taps), (h_rec, rec)):
    ctx.check(lib.gnss_dev_download(ctx.h, C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()),
                                    C.c_uint64(src.numel() * 8)))
h_out = Out()
t_host = call(None, track_out(h_rec.data_ptr(), h_taps.data_ptr(), 0), h_out)
same = bool((d_out.windows == h_out.windows).all()) and all(
    d_out.arr[f].tobytes() == h_out.arr[f].tobytes() for f in FIELDS)
same_plain = all(d_out.arr[f].tobytes() == p_out.arr[f].tobytes() for f in abi.ACF_FIELDS)

W = int(d_out.windows.sum())
bins, H = xcfg.fft_n // 2 + 1, xcfg.fft_hist
flop = W * bins * (4 * H + 3)  # two multiplies and two adds per (bin, sample); the squares and their sum
med = statistics.median
full = d_out.arr["fftFreq"][:, H - 1:]
lines = [f"src_digest {srcdigest.src_digest()} commit {srcdigest.head_commit()}",
         f"{N} channels x {L} rows x {TAPS} taps, device-resident, seeded; {W} windows; fft_hist {H}, fft_n "
         f"{xcfg.fft_n} ({bins} bins), fft_fill {xcfg.fft_fill}; {ITERS} timed calls of each after one warm-up",
         f"spectrum: {flop / 1e9:.2f} GFLOP (4 per bin and sample, counted from the shapes); the counting row pass "
         f"writes {N * L / 1e6:.2f} MB more",
         f"(1) gnss_acf_features device call, ms:     median {med(t_plain):.3f} min {min(t_plain):.3f} max {max(t_plain):.3f}",
         f"(2) gnss_acf_features_ext device call, ms: median {med(t_ext):.3f} min {min(t_ext):.3f} max {max(t_ext):.3f}",
         f"(3) gnss_acf_features_ext host path on a pinned host copy, one call, ms: {t_host:.1f}",
         f"device outputs == host outputs bit for bit (9 fields): {same}; out == gnss_acf_features' out: {same_plain}",
         f"fftFreq over the full-history windows: min {full.min():.4f} max {full.max():.4f} Hz (the swing is at 3 Hz)"]
text = "\n".join(lines) + "\n"
print(text)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write(text)
ctx.close()
sys.exit(0 if same and same_plain else 1)
