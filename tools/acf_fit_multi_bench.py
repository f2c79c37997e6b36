"""Timing driver for gnss_acf_fit_multi on device-resident seeded sums of config 5's shape (32
channels x 91 000 rows x 61 taps at -1.5:0.05:1.5, generated on the device; 29 088 windows of 100
rows; a direct path and rays 0.5 and 1.1 chips late). In one process, after a warm-up of each,
ROUNDS alternating rounds of
  (a) gnss_acf_fit_multi at its defaults (281 candidates, max_paths 3, sweeps 4);
  (b) the same with max_paths = 2;
  (c) gnss_acf_fit_taps on the same sums at its default grid of 81 x 196 hypotheses: the yardstick;
for each the kernel (hipEvents around it: gnss_last_timing's track_kernel_ms) and the whole call
under a host clock (it ends in a stream synchronise: the kernel and the rows' download). Then once
the host path (no context, up to 16 threads) on one channel at (a)'s parameters under a host clock,
compared with the device's rows bit for bit. The medians; the solve count of (a) and (b) from the
`searches` output, per order, and the fp64 operations that follow from the shapes (flops()); one
JSON line.
Args: [ROUNDS] [--channels N] [--no-host] [OUTFILE]."""
import ctypes as C
import importlib
import json
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

argv = sys.argv[1:]
N = int(argv[argv.index("--channels") + 1]) if "--channels" in argv else 32
pos = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--channels")]
ROUNDS = int(pos[0]) if pos and pos[0].isdigit() else 5
OUT = next((a for a in pos if not a.isdigit()), None)
HOST = "--no-host" not in argv
L = 91000
abi, sdr = pkg.abi, pkg.sdr
ctx = pkg.Context(0)
lib = ctx.lib
dev = torch.device("cuda:0")
torch.manual_seed(20240611)
P = abi.ACF_MULTI_MAX_PATHS


def seeded(u):
    """a correlation triangle about u = 0, half of it 0.5 chip later, opposed, and 0.4 of it 1.1
    chips later in quadrature, on a random carrier phase per row, plus noise: [N][2][len(u)][L] on
    the device"""
    uu = torch.tensor(u, device=dev, dtype=torch.float64)
    tri = lambda x: torch.clamp(1 - x.abs(), min=0)
    re = 4000.0 * (tri(uu) - 0.5 * tri(uu + 0.5))
    im = 4000.0 * 0.4 * tri(uu + 1.1)
    phase = torch.rand((N, 1, L), device=dev, dtype=torch.float64) * 6.283185307179586
    taps = torch.randn((N, 2, len(u), L), device=dev, dtype=torch.float64) * 1500.0
    c, s = torch.cos(phase), torch.sin(phase)
    taps[:, 0] += re[None, :, None] * c - im[None, :, None] * s
    taps[:, 1] += re[None, :, None] * s + im[None, :, None] * c
    torch.cuda.synchronize()
    return taps


lens = np.full(N, L, dtype=np.int64)
DM, DT = abi.ACF_FIT_MULTI_DEFAULTS, abi.ACF_FIT_TAPS_DEFAULTS
CAP = (L - 1) // 100


class MultiOut:
    def __init__(self, n=N):
        self.windows = np.zeros(n, dtype=np.int64)
        self.ints = {f: np.zeros((n, CAP), dtype=np.int32) for f in ("paths", "searches")}
        self.arr = {"bias": np.zeros((n, CAP)), "energy": np.zeros((n, CAP)), "res": np.zeros((n, P + 1, CAP))}
        self.arr.update({f: np.zeros((n, P, CAP)) for f in ("q", "A_re", "A_im")})
        o = abi.GnssAcfFitMultiOut()
        o.cap = CAP
        o.windows = self.windows.ctypes.data_as(C.POINTER(C.c_int64))
        for f, a in self.ints.items():
            setattr(o, f, a.ctypes.data_as(C.POINTER(C.c_int32)))
        for f, a in self.arr.items():
            setattr(o, f, a.ctypes.data_as(C.POINTER(C.c_double)))
        self.c = o

    def same(self, other, n=N):
        return bool((self.windows[:n] == other.windows[:n]).all()) and \
            all(a[:n].tobytes() == other.ints[f][:n].tobytes() for f, a in self.ints.items()) and \
            all(a[:n].tobytes() == other.arr[f][:n].tobytes() for f, a in self.arr.items())


class TapsOut:
    def __init__(self, n=N):
        self.windows = np.zeros(n, dtype=np.int64)
        self.paths = np.zeros((n, CAP), dtype=np.int32)
        self.arr = {f: np.zeros((n, CAP)) for f in abi.ACF_FIT_FIELDS}
        o = abi.GnssAcfFitOut()
        o.cap = CAP
        o.windows = self.windows.ctypes.data_as(C.POINTER(C.c_int64))
        o.paths = self.paths.ctypes.data_as(C.POINTER(C.c_int32))
        for f in abi.ACF_FIT_FIELDS:
            setattr(o, f, self.arr[f].ctypes.data_as(C.POINTER(C.c_double)))
        self.c = o


def source(ptr):
    src = abi.GnssAcfFitTapsIn()
    src.taps, src.max_rows, src.n_rows = ptr, L, lens.ctypes.data
    return src


def timed(fn, h, cfg, src, out):
    t = time.perf_counter()
    st = fn(h, C.byref(cfg), C.byref(src), C.byref(out.c))
    dt = (time.perf_counter() - t) * 1e3
    if st != abi.OK:
        raise abi.GnssError(st, (lib.gnss_last_error(h) or b"").decode() if h else "")
    return dt, (ctx.timing()["track_kernel_ms"] if h else 0.0)


def multi_call(h, ptr, u, prompt, par, out, n=N, flags=abi.OUT_DEVICE):
    """gnss_acf_fit_multi -> (call ms under the host clock, kernel ms)"""
    cfg = abi.GnssAcfFitMultiCfg()
    cfg.n, cfg.n_taps, cfg.prompt, cfg.flags, cfg.u = n, len(u), prompt, flags, u.ctypes.data
    for k, v in par.items():
        setattr(cfg, k, v)
    return timed(lib.gnss_acf_fit_multi, h, cfg, source(ptr), out)


def taps_call(h, ptr, u, prompt, grid, out):
    """gnss_acf_fit_taps -> (call ms under the host clock, kernel ms)"""
    cfg = abi.GnssAcfFitTapsCfg()
    cfg.n, cfg.n_taps, cfg.prompt, cfg.flags, cfg.u = N, len(u), prompt, abi.OUT_DEVICE, u.ctypes.data
    for k, v in grid.items():
        setattr(cfg, k, v)
    return timed(lib.gnss_acf_fit_taps, h, cfg, source(ptr), out)


def flops(n_taps, by_order):
    """fp64 operations of the searches, from the shapes: a candidate tried among m slots costs per
    tap R (3), m + 2 products and sums (2 (m + 2)) and, for the residual, R again (3), 4 m for the
    subtractions and 4 for |d|^2 and the sum: 6 m + 14; every search tries q_count candidates (the
    few too close to another slot are skipped, the elimination's 2 m^3 / 3 per candidate is left
    out: below 1 %). by_order[m - 1]: the searches of order m over all windows. The orders run the
    same whatever max_paths is, so order 1 has 2 per window (the append and one round that cannot
    move), order 2 what (b)'s `searches` has beyond them and order 3 what (a)'s has beyond (b)'s."""
    return sum(float(s) * DM["q_count"] * n_taps * (6.0 * m + 14.0) for m, s in enumerate(by_order, start=1))


med = statistics.median
u61 = np.ascontiguousarray(sdr.colon(-1.5, 0.05, 1.5))
res = {"commit": srcdigest.head_commit(), "src_digest": srcdigest.src_digest(), "channels": N, "rows": L, "taps": 61,
       "windows": N * CAP, "rounds": ROUNDS}
t61 = seeded(u61)
par3, par2 = dict(DM), dict(DM, max_paths=2)
outs = {"multi_default": MultiOut(), "multi_max_paths_2": MultiOut(), "taps_81x196": TapsOut()}
calls = {"multi_default": lambda: multi_call(ctx.h, t61.data_ptr(), u61, 30, par3, outs["multi_default"]),
         "multi_max_paths_2": lambda: multi_call(ctx.h, t61.data_ptr(), u61, 30, par2, outs["multi_max_paths_2"]),
         "taps_81x196": lambda: taps_call(ctx.h, t61.data_ptr(), u61, 30, DT, outs["taps_81x196"])}
for f in calls.values():
    f()  # warm-up
times = {k: ([], []) for k in calls}
for _ in range(ROUNDS):
    for k, f in calls.items():
        c, kern = f()
        times[k][0].append(c), times[k][1].append(kern)
for k, (c, kern) in times.items():
    res[k] = {"kernel_ms": med(kern), "kernel_ms_min": min(kern), "kernel_ms_max": max(kern), "call_ms": med(c)}
s3, s2 = (outs[k].ints["searches"].astype(np.int64) for k in ("multi_default", "multi_max_paths_2"))
s1 = np.minimum(s2, 2)
orders = {"multi_default": [s1.sum(), (s2 - s1).sum(), (s3 - s2).sum()], "multi_max_paths_2": [s1.sum(), (s2 - s1).sum()]}
for k, by_order in orders.items():
    o = outs[k]
    fl = flops(61, by_order)
    res[k].update(searches_mean=float(o.ints["searches"].mean()), searches_by_order=[int(x) for x in by_order],
                  solves=float(o.ints["searches"].sum()) * DM["q_count"],
                  paths_hist=np.bincount(o.ints["paths"].ravel(), minlength=P + 1).tolist(), fp64_ops=fl,
                  fp64_gops_per_s=fl / (res[k]["kernel_ms"] * 1e-3) / 1e9)
res["taps_81x196"]["two_path_windows"] = int((outs["taps_81x196"].paths == 2).sum())
if HOST:
    one = t61[0].cpu().numpy()  # channel 0: [2][61][L]
    h_out = MultiOut(1)
    ms, _ = multi_call(None, one.ctypes.data, u61, 30, par3, h_out, n=1, flags=0)
    res["host_path_one_channel"] = {"wall_ms": ms, "threads": min(16, os.cpu_count() or 1), "windows": CAP,
                                    "equals_device": h_out.same(outs["multi_default"], 1)}
ctx.close()
line = json.dumps(res)
print(line)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, "w").write(line + "\n")
sys.exit(0 if res.get("host_path_one_channel", {}).get("equals_device", True) else 1)
