"""Timing driver for gnss_acf_fit_taps on device-resident seeded sums of config 5's shape (32
channels x 91 000 rows, generated on the device; 29 088 windows of 100 rows). In one process, after
a warm-up of each, ROUNDS alternating rounds of
  (a) gnss_acf_fit_taps at the 25-tap grid (u[j] = (j - 12) * 0.05, prompt 12) with gnss_acf_fit's
      default grid of 81 x 96 hypotheses: the kernel (hipEvents around it: gnss_last_timing's
      track_kernel_ms) and the whole call under a host clock (it ends in a stream synchronise: the
      kernel and the rows' download);
  (b) gnss_acf_fit on the same sums at the same grid, the whole call under the host clock (that
      call reports no kernel time of its own; its kernel holds z in registers where (a) reads LDS);
      the two results compared bit for bit;
  (c) gnss_acf_fit_taps at 61 taps (-1.5:0.05:1.5) with its own default grid of 81 x 196
      hypotheses on 32 x 91 000 x 61 sums: the kernel and the call;
then once the host path (no context, up to 16 threads) on one channel of (c)'s sums under a host
clock, compared with the device's rows bit for bit. The medians; one JSON line.
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


def seeded(u):
    """a correlation triangle about u = 0 and half of it half a chip later, on a random carrier
    phase per row, plus noise: [N][2][len(u)][L] on the device"""
    uu = torch.tensor(u, device=dev, dtype=torch.float64)
    tri = 4000.0 * (torch.clamp(1 - uu.abs(), min=0) + 0.5 * torch.clamp(1 - (uu + 0.5).abs(), min=0))
    phase = torch.rand((N, 1, L), device=dev, dtype=torch.float64) * 6.283185307179586
    taps = torch.randn((N, 2, len(u), L), device=dev, dtype=torch.float64) * 1500.0
    taps[:, 0] += tri[None, :, None] * torch.cos(phase)
    taps[:, 1] += tri[None, :, None] * torch.sin(phase)
    torch.cuda.synchronize()
    return taps


lens = np.full(N, L, dtype=np.int64)
D25, DT = abi.ACF_FIT_DEFAULTS, abi.ACF_FIT_TAPS_DEFAULTS
CAP = (L - 1) // 100


class Out:
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

    def same(self, other, n=N):
        return bool((self.windows[:n] == other.windows[:n]).all()) and \
            self.paths[:n].tobytes() == other.paths[:n].tobytes() and \
            all(self.arr[f][:n].tobytes() == other.arr[f][:n].tobytes() for f in abi.ACF_FIT_FIELDS)


def taps_call(h, ptr, u, prompt, grid, out, n=N, flags=abi.OUT_DEVICE):
    """gnss_acf_fit_taps -> (call ms under the host clock, kernel ms)"""
    cfg = abi.GnssAcfFitTapsCfg()
    cfg.n, cfg.n_taps, cfg.prompt, cfg.flags, cfg.u = n, len(u), prompt, flags, u.ctypes.data
    for k in ("ind_start", "numOverLap", "p_min", "p_step", "p_count", "e_min", "e_step", "e_count", "ratio_max", "gain_min"):
        setattr(cfg, k, grid[k])
    src = abi.GnssAcfFitTapsIn()
    src.taps, src.max_rows, src.n_rows = ptr, L, lens.ctypes.data
    t = time.perf_counter()
    st = lib.gnss_acf_fit_taps(h, C.byref(cfg), C.byref(src), C.byref(out.c))
    dt = (time.perf_counter() - t) * 1e3
    if st != abi.OK:
        raise abi.GnssError(st, (lib.gnss_last_error(h) or b"").decode() if h else "")
    return dt, (ctx.timing()["track_kernel_ms"] if h else 0.0)


def fixed_call(ptr, out):
    """gnss_acf_fit (orient +1, its default grid) -> call ms under the host clock"""
    cfg = abi.GnssAcfFitCfg()
    cfg.n, cfg.orient = N, 1
    for k, v in D25.items():
        setattr(cfg, k, v)
    rec = abi.GnssTrackOut()
    rec.max_len = L
    rec.taps = C.cast(C.c_void_p(ptr), C.POINTER(C.c_double))
    rec.len = lens.ctypes.data_as(C.POINTER(C.c_int64))
    rec.flags = abi.OUT_DEVICE
    t = time.perf_counter()
    st = lib.gnss_acf_fit(ctx.h, C.byref(cfg), C.byref(rec), abi.MC_TAPS, C.byref(out.c))
    dt = (time.perf_counter() - t) * 1e3
    if st != abi.OK:
        raise abi.GnssError(st, (lib.gnss_last_error(ctx.h) or b"").decode())
    return dt


med = statistics.median
u25 = (np.arange(25) - 12.0) * 0.05
u61 = np.ascontiguousarray(sdr.colon(-1.5, 0.05, 1.5))
grid25 = dict(DT, e_count=D25["e_count"])
res = {"commit": srcdigest.head_commit(), "src_digest": srcdigest.src_digest(), "channels": N, "rows": L,
       "windows": N * CAP, "rounds": ROUNDS}

t25 = seeded(u25)
a_out, b_out = Out(), Out()
taps_call(ctx.h, t25.data_ptr(), u25, 12, grid25, a_out), fixed_call(t25.data_ptr(), b_out)  # warm-up
a_call, a_kern, b_call = [], [], []
for _ in range(ROUNDS):
    c, k = taps_call(ctx.h, t25.data_ptr(), u25, 12, grid25, a_out)
    a_call.append(c), a_kern.append(k)
    b_call.append(fixed_call(t25.data_ptr(), b_out))
res["taps25_grid_81x96"] = {"kernel_ms": med(a_kern), "kernel_ms_min": min(a_kern), "kernel_ms_max": max(a_kern),
                            "call_ms": med(a_call)}
res["gnss_acf_fit_81x96"] = {"call_ms": med(b_call), "call_ms_min": min(b_call), "call_ms_max": max(b_call)}
res["taps25_equals_gnss_acf_fit"] = a_out.same(b_out)
del t25
torch.cuda.empty_cache()

t61 = seeded(u61)
c_out = Out()
taps_call(ctx.h, t61.data_ptr(), u61, 30, DT, c_out)  # warm-up
c_call, c_kern = [], []
for _ in range(ROUNDS):
    c, k = taps_call(ctx.h, t61.data_ptr(), u61, 30, DT, c_out)
    c_call.append(c), c_kern.append(k)
res["taps61_grid_81x196"] = {"kernel_ms": med(c_kern), "kernel_ms_min": min(c_kern), "kernel_ms_max": max(c_kern),
                             "call_ms": med(c_call), "two_path_windows": int((c_out.paths == 2).sum())}
if HOST:
    one = t61[0].cpu().numpy()  # channel 0: [2][61][L]
    h_out = Out(1)
    ms, _ = taps_call(None, one.ctypes.data, u61, 30, DT, h_out, n=1, flags=0)
    res["host_path_61_one_channel"] = {"wall_ms": ms, "threads": min(16, os.cpu_count() or 1), "windows": CAP,
                                       "equals_device": h_out.same(c_out, 1)}
ctx.close()
line = json.dumps(res)
print(line)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, "w").write(line + "\n")
sys.exit(0 if res["taps25_equals_gnss_acf_fit"] and res.get("host_path_61_one_channel", {}).get("equals_device", True) else 1)
