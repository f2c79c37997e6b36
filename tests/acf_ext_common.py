"""What the F6-F8 tests share (test_acf_ext_kat.py on the CPU, test_gpu_acf_ext.py on the GPU): the
call of gnss_acf_features_ext through the C-ABI with host or uploaded records (acf_common's seeded
records and buffers), the twiddle table, and the bit-for-bit comparisons."""
import ctypes as C

import numpy as np

import acf_common as K
import acf_ext_twin as X
import acf_twin as T


def twiddle(pkg, N):
    c, s = np.zeros(N), np.zeros(N)
    st = pkg.abi.load().gnss_acf_twiddle(N, c.ctypes.data_as(C.POINTER(C.c_double)),
                                         s.ctypes.data_as(C.POINTER(C.c_double)))
    assert st == pkg.abi.OK
    return c, s


def split(params):
    """(gnss_acf_cfg's parameters, gnss_acf_ext_cfg's with fs by the default rule of :172)"""
    base = {k: v for k, v in params.items() if k in T.DEFAULTS}
    ext = dict(X.DEFAULTS, **{k: v for k, v in params.items() if k in X.DEFAULTS or k == "fs"})
    if "fs" not in ext:
        ext["fs"] = 1000.0 / dict(T.DEFAULTS, **base)["numOverLap"]
    return base, ext


class ExtBuffers:
    def __init__(self, pkg, n, cap, null=None):
        self.arr = {f: np.full((max(n, 1), max(cap, 1)), np.nan) for f in X.FIELDS}
        self.c = pkg.abi.GnssAcfExtOut()
        for f in X.FIELDS:
            if f != null:
                setattr(self.c, f, self.arr[f].ctypes.data_as(C.POINTER(C.c_double)))


def ext_run(pkg, r, *, ctx=None, dev=None, want=False, dev_ind=None, dev_corr=None, cap=None, n_taps=25, n=None,
            null=None, **params):
    """gnss_acf_features_ext -> (status, acf_common.OutBuffers, ExtBuffers)"""
    lib = pkg.abi.load()
    n = r.n if n is None else n
    base, ext = split(params)
    cfg = K.c_cfg(pkg, n, **base)
    xcfg = pkg.abi.GnssAcfExtCfg()
    xcfg.fft_hist, xcfg.fft_n, xcfg.fft_fill, xcfg.fs = ext["fft_hist"], ext["fft_n"], ext["fft_fill"], ext["fs"]
    rec = K.c_track_out(pkg, r, dev)
    cap = K.cap_of(r, **base) if cap is None else cap
    out = K.OutBuffers(pkg, max(n, 0), cap, r.max_len, want, dev_ind, dev_corr)
    xout = ExtBuffers(pkg, max(n, 0), cap, null)
    st = lib.gnss_acf_features_ext(ctx.h if ctx is not None else None, C.byref(cfg), C.byref(xcfg), C.byref(rec),
                                   n_taps, C.byref(out.c), C.byref(xout.c))
    return st, out, xout


def twin(pkg, r, **params):
    """The twin's F6-F8 per channel, from the base twin's corr and meanMax and the library's table"""
    base, ext = split(params)
    _, chans = K.twin(r, **base)
    par = dict(T.DEFAULTS, **base)
    c, s = twiddle(pkg, ext["fft_n"])
    return [X.channel(ch["corr"], ch["meanMax"], c, s, ind_start=par["ind_start"], numOverLap=par["numOverLap"],
                      fs=ext["fs"], fft_hist=ext["fft_hist"], fft_fill=ext["fft_fill"]) for ch in chans]


def assert_ext_equals_twin(out, xout, chans):
    for c, ch in enumerate(chans):
        W = int(out.windows[c])
        assert W == len(ch["numMLC"]), (c, W)
        for f in X.FIELDS:
            assert K.same_bits(xout.arr[f][c, :W], ch[f]), (c, f, xout.arr[f][c, :W][:4], ch[f][:4])


def assert_same_ext(out, a, b):
    for c in range(out.n):
        W = int(out.windows[c])
        for f in X.FIELDS:
            assert K.same_bits(a.arr[f][c, :W], b.arr[f][c, :W]), (c, f)


def assert_same_base(a, b, ind=True):
    """Two acf_common.OutBuffers: the features and, where both hold them, maxCorrInd and corr"""
    K.assert_same_outputs(a, b)
    if ind and a.ind is not None and b.ind is not None:
        assert np.array_equal(a.ind, b.ind) and K.same_bits(a.corr, b.corr)
