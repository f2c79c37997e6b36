"""What the tests of the two-path fit on any tap grid share (test_acf_fit_taps_kat.py on the CPU,
test_gpu_acf_fit_taps.py on the GPU): seeded sums of any n_taps in gnss_replay_out.taps' layout,
the call through the C-ABI with host or uploaded sums, gnss_acf_fit_taps_window on one vector,
model vectors and the bit-for-bit comparisons."""
import ctypes as C
from types import SimpleNamespace as NS

import numpy as np

import acf_fit_taps_twin as T
from acf_common import same_bits

SMALL = dict(p_min=-0.1, p_step=0.1, p_count=3, e_min=0.3, e_step=0.2, e_count=2)  # 3 x 2 hypotheses
WIDE = np.round(np.arange(-50, 21) * 0.05, 2)  # -2.5:0.05:1.0, 71 taps, the prompt at index 50


def grid_u(n_taps, prompt, spacing=0.05):
    """the uniform grid with u = 0 at `prompt`"""
    return (np.arange(n_taps) - float(prompt)) * spacing


def sums(n_taps, prompt, n_rows, max_rows, u=None, seed=11):
    """Seeded sums [n][2][n_taps][max_rows]: per row a triangle about u = 0 and half of it 0.4 chip
    later on a random carrier phase, the data bit's sign on the whole row, plus noise; junk past
    n_rows that nothing may read into a result."""
    n_rows = np.asarray(n_rows, dtype=np.int64)
    n = len(n_rows)
    u = grid_u(n_taps, prompt) if u is None else np.asarray(u, dtype=np.float64)
    rng = np.random.default_rng(seed)
    shape = 4000.0 * (T.tri(u) + 0.5 * T.tri(u + 0.4))
    if not shape[prompt]:
        shape[prompt] = 4000.0  # (a grid with no tap near 0: the signs still follow the bits)
    ph = rng.uniform(-0.3, 0.3, (n, 1, max_rows))
    bit = rng.choice([-1.0, 1.0], (n, 1, max_rows))
    taps = rng.normal(0, 300.0, (n, 2, n_taps, max_rows))
    taps[:, 0] += bit * shape[None, :, None] * np.cos(ph)
    taps[:, 1] += bit * shape[None, :, None] * np.sin(ph)
    for c in range(n):
        taps[c, :, :, n_rows[c]:] = 1e30
    return NS(taps=np.ascontiguousarray(taps), n_rows=n_rows, max_rows=int(max_rows), n=n, n_taps=int(n_taps),
              prompt=int(prompt), u=np.ascontiguousarray(u))


def c_cfg(pkg, n, u, prompt, flags=0, n_taps=None, **params):
    """-> (cfg, what must stay alive)"""
    par = dict(T.DEFAULTS, **params)
    cfg = pkg.abi.GnssAcfFitTapsCfg()
    uu = None if u is None else np.ascontiguousarray(u, dtype=np.float64)
    cfg.n, cfg.prompt, cfg.flags = n, prompt, flags
    cfg.n_taps = (0 if uu is None else len(uu)) if n_taps is None else n_taps
    cfg.u = None if uu is None else uu.ctypes.data
    for k, v in par.items():
        setattr(cfg, k, v)
    return cfg, uu


class OutBuffers:
    """Caller-allocated gnss_acf_fit_out: `cap` windows per channel, filled with values no fit
    writes so that an unwritten element shows."""

    def __init__(self, pkg, n, cap, n_taps, want=True):
        self.n, self.cap = n, cap
        shape = (max(n, 1), max(cap, 1))
        self.windows = np.full(max(n, 1), -1, dtype=np.int64)
        self.paths = np.full(shape, -9, dtype=np.int32)
        self.arr = {f: np.full(shape, -7.0) for f in T.FIELDS}
        o = pkg.abi.GnssAcfFitOut()
        o.cap = cap
        o.windows = self.windows.ctypes.data_as(C.POINTER(C.c_int64))
        o.paths = self.paths.ctypes.data_as(C.POINTER(C.c_int32))
        for f in T.FIELDS:
            setattr(o, f, self.arr[f].ctypes.data_as(C.POINTER(C.c_double)))
        self.zI = self.zQ = None
        if want:
            zs = (shape[0], max(n_taps, 1), shape[1])
            self.zI, self.zQ = np.full(zs, -7.0), np.full(zs, -7.0)
            o.zI = self.zI.ctypes.data_as(C.POINTER(C.c_double))
            o.zQ = self.zQ.ctypes.data_as(C.POINTER(C.c_double))
        self.c = o

    def untouched(self):
        return (self.windows == -1).all() and (self.paths == -9).all() and all(
            (a == -7.0).all() for a in self.arr.values()) and (self.zI is None or ((self.zI == -7.0).all() and
                                                                                  (self.zQ == -7.0).all()))


def cap_of(s, **params):
    par = dict(T.DEFAULTS, **params)
    return max([max(int(l) - par["ind_start"], 0) // par["numOverLap"] for l in s.n_rows] + [1])


def lib_run(pkg, s, *, ctx=None, dev=None, want=True, cap=None, n=None, u="own", prompt=None, n_taps=None,
            flags=None, taps="own", n_rows="own", max_rows=None, **params):
    """gnss_acf_fit_taps on the sums s (dev: the device pointer of an uploaded copy) ->
    (status, OutBuffers); the keywords replace single arguments for the refusal tests."""
    lib = pkg.abi.load()
    n = s.n if n is None else n
    cfg, keep = c_cfg(pkg, n, s.u if isinstance(u, str) else u, s.prompt if prompt is None else prompt,
                      (pkg.abi.OUT_DEVICE if dev is not None else 0) if flags is None else flags, n_taps, **params)
    src = pkg.abi.GnssAcfFitTapsIn()
    nr = s.n_rows if isinstance(n_rows, str) else n_rows
    src.taps = (s.taps.ctypes.data if dev is None else dev) if isinstance(taps, str) else taps
    src.max_rows = s.max_rows if max_rows is None else max_rows
    src.n_rows = None if nr is None else nr.ctypes.data
    win = {k: v for k, v in params.items() if k in ("ind_start", "numOverLap")}
    out = OutBuffers(pkg, max(n, 0), cap_of(s, **win) if cap is None else cap, s.n_taps, want)
    st = lib.gnss_acf_fit_taps(ctx.h if ctx is not None else None, C.byref(cfg), C.byref(src), C.byref(out.c))
    return st, out


def fit_window(pkg, zI, zQ, u, prompt=0, **params):
    """gnss_acf_fit_taps_window on one coherent vector -> (status, dict of paths and the fields)."""
    zI, zQ = np.ascontiguousarray(zI, dtype=np.float64), np.ascontiguousarray(zQ, dtype=np.float64)
    out = OutBuffers(pkg, 1, 1, len(zI))
    cfg, keep = c_cfg(pkg, 1, u, prompt, **params)
    st = pkg.abi.load().gnss_acf_fit_taps_window(C.byref(cfg), zI.ctypes.data_as(C.POINTER(C.c_double)),
                                                 zQ.ctypes.data_as(C.POINTER(C.c_double)), C.byref(out.c))
    got = {f: float(out.arr[f][0, 0]) for f in T.FIELDS}
    got["paths"] = int(out.paths[0, 0])
    if st == pkg.abi.OK:
        assert out.windows[0] == 1 and same_bits(out.zI[0, :, 0], zI) and same_bits(out.zQ[0, :, 0], zQ)
    return st, got


def model(u, p, e, A0, A1):
    """z[j] = A0 R(u[j] - p) + A1 R(u[j] - (p - e)) -> zI, zQ"""
    u = np.asarray(u, dtype=np.float64)
    z = A0 * T.tri(u - p) + A1 * T.tri(u - (p - e))
    return np.real(z).copy(), np.imag(z).copy()


def assert_equals_twin(out, chans):
    """Every output of the written windows bit for bit; the elements past them untouched."""
    for c, ch in enumerate(chans):
        W = ch["windows"]
        assert out.windows[c] == W, (c, out.windows[c], W)
        assert np.array_equal(out.paths[c, :W], ch["paths"]), (c, out.paths[c, :W], ch["paths"])
        assert np.all(out.paths[c, W:] == -9), c
        for f in T.FIELDS:
            assert same_bits(out.arr[f][c, :W], ch[f]), (c, f, out.arr[f][c, :W][:3], ch[f][:3])
            assert np.all(out.arr[f][c, W:] == -7.0), (c, f)
        if out.zI is not None:
            assert same_bits(out.zI[c, :, :W], ch["zI"]) and same_bits(out.zQ[c, :, :W], ch["zQ"]), c
            assert np.all(out.zI[c, :, W:] == -7.0) and np.all(out.zQ[c, :, W:] == -7.0), c


def assert_same_outputs(a, b):
    """Two OutBuffers (host path, device path) bit for bit in every element, written or not."""
    assert np.array_equal(a.windows, b.windows)
    assert np.array_equal(a.paths, b.paths)
    for f in T.FIELDS:
        assert same_bits(a.arr[f], b.arr[f]), f
    if a.zI is not None and b.zI is not None:
        assert same_bits(a.zI, b.zI) and same_bits(a.zQ, b.zQ)
