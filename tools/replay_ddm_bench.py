"""Timing driver for gnss_replay_ddm on device-resident seeded sums of config 5's shape (32 channels
x 91 000 rows x 61 taps, generated on the device; 2 912 windows of 1 000 rows, 101 Doppler bins
-50:1:50 Hz): 1.4e11 fp64 operations counted from the shapes (8 per row, tap and bin). In one
process, after WARMUP calls, ROUNDS calls with the map left on the device (GNSS_DDM_MAP_DEVICE: only
the peaks come back): the kernels (hipEvents around both: kernel_ms) and the whole call under a host
clock; then once with the map downloaded, compared with the device's copy bit for bit; then once
the host path (no context, up to 16 threads) on one channel's sums under a host clock, compared with
the device's rows bit for bit. The medians; one JSON line.
Args: [ROUNDS] [--channels N] [--warmup W] [--no-host] [OUTFILE]."""
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


def opt(name, default):
    return int(argv[argv.index(name) + 1]) if name in argv else default


N, WARMUP = opt("--channels", 32), opt("--warmup", 3)
pos = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] not in ("--channels", "--warmup"))]
ROUNDS = int(pos[0]) if pos and pos[0].isdigit() else 10
OUT = next((a for a in pos if not a.isdigit()), None)
HOST = "--no-host" not in argv
L, R, FS = 91000, 1000, 58e6
CAP = L // R
abi, sdr = pkg.abi, pkg.sdr
ctx = pkg.Context(0)
lib = ctx.lib
dev = torch.device("cuda:0")
torch.manual_seed(20240612)

u = np.ascontiguousarray(sdr.colon(-1.5, 0.05, 1.5))
hz = np.arange(-50.0, 51.0, 1.0)
NT, ND = len(u), len(hz)
OPS = 8.0 * N * CAP * R * NT * ND

# a triangle about u = 0 with the data bit's sign per row and half of it 0.9 chip later turning at
# 20 Hz, plus noise: [N][2][NT][L] on the device
uu = torch.tensor(u, device=dev, dtype=torch.float64)
bit = torch.where(torch.rand((N, 1, L), device=dev) < 0.5, -1.0, 1.0).double()
ms = torch.arange(L, device=dev, dtype=torch.float64)[None, None, :] * 1e-3
taps = torch.randn((N, 2, NT, L), device=dev, dtype=torch.float64) * 1500.0
tri, ray = 4000.0 * torch.clamp(1 - uu.abs(), min=0), 2000.0 * torch.clamp(1 - (uu + 0.9).abs(), min=0)
taps[:, 0] += bit * (tri[None, :, None] + ray[None, :, None] * torch.cos(2 * np.pi * 20.0 * ms))
taps[:, 1] += bit * (ray[None, :, None] * torch.sin(2 * np.pi * 20.0 * ms))
torch.cuda.synchronize()
n_rows = np.full(N, L, dtype=np.int64)
num = np.full((N, L), 58000, dtype=np.int64)
posb = np.ascontiguousarray(np.broadcast_to(2 * 58000 * np.arange(L, dtype=np.int64), (N, L)))


class Out:
    def __init__(self, n, map_ptr):
        self.n_win = np.zeros(n, dtype=np.int64)
        self.arr = {f: np.zeros((n, CAP), dtype=np.float64 if f.endswith("pow") else np.int32)
                    for f in ("peak_bin", "peak_tap", "peak_pow", "sec_bin", "sec_tap", "sec_pow")}
        o = abi.GnssReplayDdmOut()
        o.cap, o.map, o.n_win = CAP, map_ptr, self.n_win.ctypes.data
        for f, a in self.arr.items():
            setattr(o, f, a.ctypes.data)
        self.c = o

    def same(self, other, n):
        return all(self.arr[f][:n].tobytes() == other.arr[f][:n].tobytes() for f in self.arr)


def call(h, ptr, out, n, flags):
    """gnss_replay_ddm -> (call ms under the host clock, kernel ms)"""
    cfg = abi.GnssReplayDdmCfg()
    cfg.n, cfg.n_taps, cfg.prompt, cfg.rows_per_window, cfg.n_dopp, cfg.flags = n, NT, NT // 2, R, ND, flags
    cfg.dopp_hz, cfg.u, cfg.excl_chips, cfg.excl_hz, cfg.Fs, cfg.bytes_per_sample = hz.ctypes.data, u.ctypes.data, 0.3, 10.0, FS, 2
    src = abi.GnssReplayDdmIn()
    src.taps, src.max_rows = ptr, L
    src.n_rows, src.pos_bytes, src.numSample = n_rows.ctypes.data, posb.ctypes.data, num.ctypes.data
    t = time.perf_counter()
    st = lib.gnss_replay_ddm(h, C.byref(cfg), C.byref(src), C.byref(out.c))
    dt = (time.perf_counter() - t) * 1e3
    if st != abi.OK:
        raise abi.GnssError(st, (lib.gnss_last_error(h) or b"").decode() if h else "")
    return dt, float(out.c.kernel_ms)


med = statistics.median
res = {"commit": srcdigest.head_commit(), "src_digest": srcdigest.src_digest(), "channels": N, "rows": L, "taps": NT,
       "bins": ND, "rows_per_window": R, "windows": N * CAP, "rounds": ROUNDS, "warmup": WARMUP, "fp64_ops": OPS}
dmap = torch.zeros((N, CAP, 2, ND, NT), dtype=torch.float64, device=dev)
torch.cuda.synchronize()
both = abi.OUT_DEVICE | abi.DDM_MAP_DEVICE
a_out = Out(N, dmap.data_ptr())
for _ in range(WARMUP):
    call(ctx.h, taps.data_ptr(), a_out, N, both)
calls, kerns = [], []
for _ in range(ROUNDS):
    c, k = call(ctx.h, taps.data_ptr(), a_out, N, both)
    calls.append(c), kerns.append(k)
res["map_on_device"] = {"kernel_ms": med(kerns), "kernel_ms_min": min(kerns), "kernel_ms_max": max(kerns),
                        "call_ms": med(calls), "fp64_tflops": OPS / (med(kerns) * 1e-3) / 1e12}
hmap = np.zeros((N, CAP, 2, ND, NT))
b_out = Out(N, hmap.ctypes.data)
c, k = call(ctx.h, taps.data_ptr(), b_out, N, abi.OUT_DEVICE)
res["map_downloaded"] = {"call_ms": c, "kernel_ms": k, "map_bytes": hmap.nbytes,
                         "equals_device_copy": bool(hmap.tobytes() == dmap.cpu().numpy().tobytes()) and b_out.same(a_out, N)}
res["peaks_channel0_window0"] = {f: float(a_out.arr[f][0, 0]) for f in a_out.arr}
ok = res["map_downloaded"]["equals_device_copy"]
if HOST:
    one = np.ascontiguousarray(taps[:1].cpu().numpy())
    m1 = np.zeros((1, CAP, 2, ND, NT))
    h_out = Out(1, m1.ctypes.data)
    ms_host, _ = call(None, one.ctypes.data, h_out, 1, 0)
    same = bool(m1.tobytes() == hmap[:1].tobytes()) and h_out.same(b_out, 1)
    res["host_path_one_channel"] = {"wall_ms": ms_host, "threads": min(16, os.cpu_count() or 1), "windows": CAP,
                                    "equals_device": same}
    ok = ok and same
ctx.close()
line = json.dumps(res)
print(line)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, "w").write(line + "\n")
sys.exit(0 if ok else 1)
