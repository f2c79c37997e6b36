"""What the tests of the two-path ACF fit share (test_acf_fit_kat.py on the CPU,
test_gpu_acf_fit.py on the GPU): the call through the C-ABI with host or uploaded records (the
seeded records are acf_common's), gnss_acf_fit_window on one vector, model vectors, and the
bit-for-bit comparisons."""
import ctypes as C

import numpy as np

import acf_fit_twin as T
from acf_common import c_track_out, same_bits

SMALL = dict(p_min=-0.1, p_step=0.1, p_count=3, e_min=0.3, e_step=0.2, e_count=2)  # the 3 x 2 grid


def c_cfg(pkg, n, orient=1, **params):
    par = dict(T.DEFAULTS, **params)
    cfg = pkg.abi.GnssAcfFitCfg()
    cfg.n, cfg.orient = n, orient
    for k, v in par.items():
        setattr(cfg, k, v)
    return cfg


class OutBuffers:
    """Caller-allocated gnss_acf_fit_out: `cap` windows per channel, filled with values no fit
    writes so that an unwritten element shows."""

    def __init__(self, pkg, n, cap, want=True):
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
            self.zI, self.zQ = np.full((shape[0], 25, shape[1]), -7.0), np.full((shape[0], 25, shape[1]), -7.0)
            o.zI = self.zI.ctypes.data_as(C.POINTER(C.c_double))
            o.zQ = self.zQ.ctypes.data_as(C.POINTER(C.c_double))
        self.c = o


def cap_of(r, **params):
    par = dict(T.DEFAULTS, **params)
    return max([max(int(l) - par["ind_start"], 0) // par["numOverLap"] for l in r.lens] + [1])


def lib_run(pkg, r, *, ctx=None, dev=None, want=True, cap=None, n_taps=25, n=None, orient=1, **params):
    """gnss_acf_fit -> (status, OutBuffers)."""
    lib = pkg.abi.load()
    n = r.n if n is None else n
    cfg = c_cfg(pkg, n, orient, **params)
    rec = c_track_out(pkg, r, dev)
    win = {k: v for k, v in params.items() if k in ("ind_start", "numOverLap")}
    out = OutBuffers(pkg, max(n, 0), cap_of(r, **win) if cap is None else cap, want)
    st = lib.gnss_acf_fit(ctx.h if ctx is not None else None, C.byref(cfg), C.byref(rec), n_taps, C.byref(out.c))
    return st, out


def fit_window(pkg, zI, zQ, orient=1, **params):
    """gnss_acf_fit_window on one coherent vector -> (status, dict of paths and the fields)."""
    zI, zQ = np.ascontiguousarray(zI, dtype=np.float64), np.ascontiguousarray(zQ, dtype=np.float64)
    out = OutBuffers(pkg, 1, 1)
    cfg = c_cfg(pkg, 1, orient, **params)
    st = pkg.abi.load().gnss_acf_fit_window(C.byref(cfg), zI.ctypes.data_as(C.POINTER(C.c_double)),
                                            zQ.ctypes.data_as(C.POINTER(C.c_double)), C.byref(out.c))
    got = {f: float(out.arr[f][0, 0]) for f in T.FIELDS}
    got["paths"] = int(out.paths[0, 0])
    if st == pkg.abi.OK:
        assert out.windows[0] == 1 and same_bits(out.zI[0, :, 0], zI) and same_bits(out.zQ[0, :, 0], zQ)
    return st, got


def model(p, e, A0, A1, orient=1, corrSpacing=0.05):
    """z[j] = A0 R(u[j] - p) + A1 R(u[j] - (p - e)) -> zI, zQ"""
    u = (orient * (np.arange(25) - 12.0)) * corrSpacing
    z = A0 * T.R(u - p) + A1 * T.R(u - (p - e))
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
