"""What the ACF feature tests share (test_acf_kat.py on the CPU, test_gpu_acf.py on the GPU):
seeded records in gnss_track_out layout with the hand-made rows, the call through the C-ABI with
host or uploaded records, and the bit-for-bit comparisons against the twin."""
import ctypes as C
from types import SimpleNamespace as NS

import numpy as np

import acf_twin as T

PRN = [14, 22, 26]
ELE = [8.36, 54.23, 24.23]
# (len per channel, max_len): every len the window rule treats differently, max_len odd and larger
SHAPES = {"short": ([99, 100, 101], 103), "long": ([1000, 1001, 257], 1003)}


def lsb(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    """fp64 arrays equal bit for bit (so -0 differs from +0); a NaN equals a NaN in the same
    place whatever its sign and payload, which MATLAB does not tell apart either."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(lsb(a)[ok], lsb(b)[ok])


def ulps(a, b):
    """|a - b| in units of the last place, for finite same-sign values; NaN pairs count as 0"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    d = np.abs(lsb(a) - lsb(b))
    return np.where(both_nan, 0, d)


def hand_rows(taps, c, row):
    """The hand-made rows of channel c from `row` on; returns {row: expected index}. Integer I/Q
    with (3,4), (5,0) and (4,3) all of magnitude exactly 5."""
    want = {}

    def put(r, cols, fill=(1.0, 1.0)):
        taps[c, 0, :, r], taps[c, 1, :, r] = fill
        for col, iq in cols.items():
            taps[c, 0, col - 1, r], taps[c, 1, col - 1, r] = iq

    put(row, {1: (3, 4), 13: (5, 0), 25: (4, 3)})  # a three-way tie: the first index wins
    want[row] = 1
    put(row + 1, {13: (5, 0), 25: (4, 3)})
    want[row + 1] = 13
    put(row + 2, {7: (4, 3), 8: (3, 4)})  # neighbours
    want[row + 2] = 7
    put(row + 3, {24: (-3, 4), 25: (0, -5)})
    want[row + 3] = 24
    put(row + 4, {1: (9, 0)})  # a peak at column 1
    want[row + 4] = 1
    put(row + 5, {25: (0, 9)})  # and at column 25
    want[row + 5] = 25
    put(row + 6, {5: (np.nan, 50.0), 9: (6, 0)})  # a NaN tap counts as missing
    want[row + 6] = 9
    put(row + 7, {1: (np.nan, 1.0), 2: (1.0, np.nan), 20: (2, 0)})
    want[row + 7] = 20
    put(row + 8, {}, fill=(np.nan, np.nan))  # an all-NaN row gives index 1
    want[row + 8] = 1
    return want


def records(shape="long", seed=7, lens=None, max_len=None, hand=True):
    """Seeded records of 3 channels: a correlation triangle about the prompt tap plus noise, so the
    peak wanders over the middle columns; a code discriminator; junk past len that nothing may
    read into a result."""
    lens0, ml0 = SHAPES[shape]
    lens = np.array(lens0 if lens is None else lens, dtype=np.int64)
    ml = int(ml0 if max_len is None else max_len)
    n = len(lens)
    rng = np.random.default_rng(seed)
    tri = 4000.0 * np.clip(1 - np.abs(np.arange(25) - 12) * 0.05, 0, None)
    taps = rng.normal(0, 1500.0, (n, 2, 25, ml))
    taps[:, 0] += tri[None, :, None] * np.cos(rng.uniform(0, 6.28, (n, 1, ml)))
    taps[:, 1] += tri[None, :, None] * np.sin(rng.uniform(0, 6.28, (n, 1, ml)))
    rec = rng.normal(0, 1.0, (n, 18, ml))
    want = {}
    if hand:
        for c in range(n):
            if lens[c] >= 40:
                want[c] = hand_rows(taps, c, 20 + c)
    for c in range(n):  # past len: values that would show in any result that read them
        taps[c, :, :, lens[c]:] = 1e30
        rec[c, :, lens[c]:] = -1e30
    return NS(taps=np.ascontiguousarray(taps), rec=np.ascontiguousarray(rec), lens=lens, max_len=ml, n=n, want=want)


def twin(r, prn=None, ele=None, **params):
    n = r.n
    return T.features(r.taps, r.rec[:, 7], r.lens, (prn or PRN)[:n], (ele or ELE)[:n], **params)


def c_track_out(pkg, r, dev=None):
    """gnss_track_out over the host arrays, or over device copies (dev = (rec_ptr, taps_ptr))."""
    o = pkg.abi.GnssTrackOut()
    o.max_len = r.max_len
    o.len = r.lens.ctypes.data_as(C.POINTER(C.c_int64))
    if dev is None:
        o.rec = r.rec.ctypes.data_as(C.POINTER(C.c_double))
        o.taps = r.taps.ctypes.data_as(C.POINTER(C.c_double))
    else:
        o.rec = C.cast(C.c_void_p(dev[0]), C.POINTER(C.c_double))
        o.taps = C.cast(C.c_void_p(dev[1]), C.POINTER(C.c_double))
        o.flags = pkg.abi.OUT_DEVICE
    return o


def c_cfg(pkg, n, prn=None, ele=None, **params):
    par = dict(T.DEFAULTS, **params)
    cfg = pkg.abi.GnssAcfCfg()
    cfg.n, cfg.ind_start, cfg.numOverLap = n, par["ind_start"], par["numOverLap"]
    cfg.corrSpacing, cfg.maxDelay = par["corrSpacing"], par["maxDelay"]
    cfg.a[:] = list(par["a"])
    m = min(max(n, 0), pkg.abi.VT_MAX_CH, len(prn or PRN))
    cfg.prn[:m], cfg.ele[:m] = (prn or PRN)[:m], (ele or ELE)[:m]
    return cfg


class OutBuffers:
    """Caller-allocated gnss_acf_out: `cap` windows per channel; the optional arrays as host
    arrays (want) or as given device pointers (dev_ind / dev_corr)."""

    def __init__(self, pkg, n, cap, max_len, want=False, dev_ind=None, dev_corr=None):
        self.n, self.cap = n, cap
        self.windows = np.full(max(n, 1), -1, dtype=np.int64)
        self.arr = {f: np.full((max(n, 1), max(cap, 1)), np.nan) for f in T.FIELDS}
        o = pkg.abi.GnssAcfOut()
        o.cap = cap
        o.windows = self.windows.ctypes.data_as(C.POINTER(C.c_int64))
        for f in T.FIELDS:
            setattr(o, f, self.arr[f].ctypes.data_as(C.POINTER(C.c_double)))
        self.ind = self.corr = None
        if want:
            self.ind = np.zeros((n, max_len), dtype=np.uint8)
            self.corr = np.full((n, 25, max_len), -7.0)
            o.maxCorrInd, o.corr = self.ind.ctypes.data, self.corr.ctypes.data
        if dev_ind is not None:
            o.maxCorrInd = dev_ind
        if dev_corr is not None:
            o.corr = dev_corr
        self.c = o


def cap_of(r, **params):
    par = dict(T.DEFAULTS, **params)
    return max([max(int(l) - par["ind_start"], 0) // par["numOverLap"] for l in r.lens] + [1])


def lib_run(pkg, r, *, ctx=None, dev=None, want=False, dev_ind=None, dev_corr=None, cap=None, n_taps=25,
            n=None, **params):
    """gnss_acf_features -> (status, OutBuffers)."""
    lib = pkg.abi.load()
    n = r.n if n is None else n
    cfg = c_cfg(pkg, n, **params)
    rec = c_track_out(pkg, r, dev)
    out = OutBuffers(pkg, max(n, 0), cap_of(r, **params) if cap is None else cap, r.max_len, want, dev_ind, dev_corr)
    st = lib.gnss_acf_features(ctx.h if ctx is not None else None, C.byref(cfg), C.byref(rec), n_taps, C.byref(out.c))
    return st, out


def assert_equals_twin(r, out, chans, ind=None, corr=None):
    """Every field bit for bit (F1 within 2 ulp: pow), the optional arrays over the rows below len."""
    for c, ch in enumerate(chans):
        W = ch["windows"]
        assert out.windows[c] == W, (c, out.windows[c], W)
        for f in T.FIELDS:
            got = out.arr[f][c, :W]
            if f == "F1":
                assert np.all(ulps(got, ch[f]) <= 2), (c, f)
            else:
                assert same_bits(got, ch[f]), (c, f, got[:3], ch[f][:3])
        L = int(r.lens[c])
        if ind is not None:
            assert np.array_equal(ind[c, :L], ch["maxCorrInd"]), c
            assert not np.any(ind[c, L:]), c  # rows past len are left alone
        if corr is not None:
            assert same_bits(corr[c, :, :L], ch["corr"]), c
            assert np.all(corr[c, :, L:] == -7.0), c


def assert_same_outputs(a, b):
    """Two OutBuffers (host path, device path) bit for bit, the written windows only."""
    assert np.array_equal(a.windows, b.windows)
    for c in range(a.n):
        W = int(a.windows[c])
        for f in T.FIELDS:
            assert same_bits(a.arr[f][c, :W], b.arr[f][c, :W]), (c, f)
