"""CalculateFeatures.m's F6-F8 through the C-ABI on host records (gnss_acf_features_ext with ctx =
NULL; csrc/acf_ext.cpp and csrc/acf.cpp over csrc/acf_ext.h): no GPU. The host path equals the
numpy twin (acf_ext_twin.py) bit for bit over the window rule's lengths, both start rows, three
window widths, histories shorter than, equal to and longer than the windows on hand, spectrum
lengths that are a power of two, not one, and equal to the history, both fill modes and the
hand-made NaN rows; `out` equals gnss_acf_features' on the same call; the known answers; the
twiddle table; every GNSS_EARG case; the mirror's 11-column data_labeled."""
import ctypes as C
from types import SimpleNamespace as NS

import numpy as np
import pytest

import acf_common as K
import acf_ext_common as E
import acf_twin as T

SHAPES = {"short": {}, "long": {}, "k1004": dict(lens=[1004, 258, 101], max_len=1004)}

# windows per channel in the comments
CASES = [
    ("short", dict()),  # 0 / 0 / 1
    ("short", dict(ind_start=7, numOverLap=64, fft_fill=1)),  # 1 / 1 / 1
    ("short", dict(numOverLap=2, fft_hist=3, fft_n=3)),  # 49 / 49 / 50, N = H
    ("short", dict(numOverLap=2, ind_start=7, fft_hist=2, fft_n=2, fft_fill=1)),  # the narrowest: 2 bins
    ("short", dict(numOverLap=2, fft_n=1000)),  # fewer windows than fft_hist = 300
    ("long", dict(fft_hist=10, fft_n=1000, fft_fill=1)),  # 9 / 10 / 2: fewer than and equal to fft_hist
    ("long", dict(fft_hist=10, fft_n=10)),
    ("long", dict(ind_start=7, numOverLap=64, fft_hist=3)),  # 15 / 15 / 3
    ("long", dict(fft_hist=2, fft_fill=1)),
    ("k1004", dict(numOverLap=2)),  # 501 / 128 / 50: more windows than fft_hist = 300
    ("k1004", dict(numOverLap=2, ind_start=7, fft_n=300, fft_fill=1)),  # 498 / 125 / 47, N = H = 300
]


def records(shape):
    return K.records("short" if shape == "short" else "long", **SHAPES[shape])


@pytest.mark.parametrize("shape,par", CASES, ids=[f"{s}-{i}" for i, (s, _) in enumerate(CASES)])
def test_host_path_equals_twin(pkg, shape, par):
    r = records(shape)
    st, out, ext = E.ext_run(pkg, r, want=True, **par)
    assert st == pkg.abi.OK
    E.assert_ext_equals_twin(out, ext, E.twin(pkg, r, **par))
    # out: gnss_acf_features' on the same call, bit for bit, maxCorrInd and corr included
    base, _ = E.split(par)
    st, plain = K.lib_run(pkg, r, want=True, **base)
    assert st == pkg.abi.OK
    E.assert_same_base(plain, out)
    st, bare, ext2 = E.ext_run(pkg, r, **par)  # the optional outputs NULL: the same features
    assert st == pkg.abi.OK
    E.assert_same_base(plain, bare)
    E.assert_same_ext(out, ext, ext2)


def test_nan_rows_reach_the_history_and_leave_it(pkg):
    """Channel 0's all-NaN row (row 28) makes its window's meanMax NaN: while that window is in the
    history every bin is NaN, so I = 1 (fftFreq 0) and fftMag NaN; with fft_hist = 3 it leaves after
    three windows."""
    r = K.records("short")
    st, out, ext = E.ext_run(pkg, r, numOverLap=2, fft_hist=3, fft_n=8)
    assert st == pkg.abi.OK
    bad = np.flatnonzero(np.isnan(out.arr["meanMax"][0, :49]))
    assert len(bad) and bad[-1] + 3 < 49
    for m in range(49):
        dirty = np.any((bad <= m) & (bad > m - 3))
        assert np.isnan(ext.arr["fftMag"][0, m]) == dirty, m
        if dirty:
            assert ext.arr["fftFreq"][0, m] == 0.0
    assert np.all(np.isfinite(ext.arr["numMLC"][0, :49]))


def prompt_series(v, numOverLap=2):
    """One channel whose window m has the prompt magnitude v[m] in every row and nothing else"""
    L = numOverLap * len(v) + 1
    r = K.records("long", lens=[L], max_len=L, hand=False)
    r.taps[:] = 0.0
    r.taps[0, 0, 12, : L - 1] = np.repeat(v, numOverLap)
    return r


def test_constant_history(pkg):
    """A constant meanMax: y = 0, every bin 0, so I = 1, fftFreq = 0 and fftMag = 0 -- from window
    fft_hist on with the script's zero fill, in every window with fft_fill = 1 (H = 1 in the first)"""
    r = prompt_series(np.full(12, 37.5))
    for fill in (0, 1):
        st, out, ext = E.ext_run(pkg, r, numOverLap=2, fft_hist=5, fft_n=16, fft_fill=fill, fs=10.0)
        assert st == pkg.abi.OK and out.windows[0] == 12 and np.all(out.arr["meanMax"][0, :12] == 37.5)
        first = 0 if fill else 4
        assert np.all(ext.arr["fftFreq"][0, first:12] == 0.0) and np.all(ext.arr["fftMag"][0, first:12] == 0.0)
        if not fill:  # the step from the zero fill is what the first windows show
            assert np.all(ext.arr["fftMag"][0, :4] > 0)
        assert np.all(ext.arr["numMLC"][0, :12] == 1.0)


@pytest.mark.parametrize("k0", [1, 5, 31])
def test_a_cosine_comes_back_at_its_bin(pkg, k0):
    """H = N = 64 and no padding: the history B + A*c[(k0*i) mod N] from gnss_acf_twiddle's table
    (a magnitude cannot be negative; the mean takes B away) has its line at bin k0, fftFreq =
    (k0*fs)/N exactly, fftMag within 1e-12*A of A."""
    N, A, B, fs = 64, 1000.0, 3000.0, 25.0
    c, _ = E.twiddle(pkg, N)
    v = B + A * c[(k0 * np.arange(N)) % N]
    st, out, ext = E.ext_run(pkg, prompt_series(v), numOverLap=2, fft_hist=N, fft_n=N, fs=fs)
    assert st == pkg.abi.OK and out.windows[0] == N
    assert np.array_equal(out.arr["meanMax"][0, :N], v)
    assert ext.arr["fftFreq"][0, N - 1] == (k0 * fs) / N
    assert abs(ext.arr["fftMag"][0, N - 1] - A) <= 1e-12 * A


def test_hand_made_rows_count_interior_peaks(pkg):
    base = np.ones(25)

    def row(cols):
        v = base.copy()
        for col, x in cols.items():
            v[col - 1] = x
        return v

    nan = float("nan")
    rows = [
        (row({13: 9}), 1),  # a single peak
        (row({5: 4, 20: 7}), 2),  # two interior peaks
        (np.arange(25, 0, -1.0), 0),  # a peak on column 1
        (np.arange(1.0, 26.0), 0),  # a peak on column 25
        (row({1: 9, 25: 9, 13: 5}), 1),  # both edges above an interior peak
        (base, 0),  # a plateau over the whole row
        (row({12: 6, 13: 6}), 0),  # a plateau of two equal values
        (row({2: 3, 24: 3}), 2),  # the first and the last column that can count
        (row({13: 9, 12: nan}), 0),  # a NaN neighbour compares false
        (row({13: 9, 3: nan}), 1),  # a NaN elsewhere
        (np.full(25, nan), 0),
        (np.where(np.arange(25) % 2 == 1, 2.0, 1.0), 12),  # every second column: columns 2, 4, ..., 24
    ]
    L = 2 * len(rows) + 2 + 1
    r = K.records("long", lens=[L], max_len=L, hand=False)
    r.taps[:] = 0.0
    for m, (v, _) in enumerate(rows):
        r.taps[0, 0, :, 2 * m] = v  # as I ...
        r.taps[0, 1, :, 2 * m + 1] = -v  # ... and as Q
    r.taps[0, 0, :, 2 * len(rows)] = rows[1][0]  # a window of two different rows: 2 and 1 peaks
    r.taps[0, 0, :, 2 * len(rows) + 1] = rows[0][0]
    st, out, ext = E.ext_run(pkg, r, numOverLap=2, fft_hist=2, fft_n=2)
    assert st == pkg.abi.OK and out.windows[0] == len(rows) + 1
    assert list(ext.arr["numMLC"][0, : len(rows)]) == [float(n) for _, n in rows]
    assert ext.arr["numMLC"][0, len(rows)] == 1.5


@pytest.mark.parametrize("N", [2, 3, 300, 1000, 1024, 2048])
def test_twiddle_table(pkg, N):
    c, s = E.twiddle(pkg, N)
    t = np.arange(N)
    assert np.max(np.abs(c - np.cos(2 * np.pi * t / N))) <= 2.3e-16
    assert np.max(np.abs(s - np.sin(2 * np.pi * t / N))) <= 2.3e-16
    assert c[0] == 1.0 and s[0] == 0.0


def test_every_earg_case(pkg):
    abi = pkg.abi
    lib = abi.load()
    r = K.records("long")
    ok = lambda **kw: E.ext_run(pkg, r, **kw)[0]
    assert ok() == abi.OK
    # the added bounds
    assert ok(fft_hist=1, fft_n=16) == abi.EARG and ok(fft_hist=0, fft_n=16) == abi.EARG
    assert ok(fft_hist=513) == abi.EARG and ok(fft_hist=513, fft_n=2048) == abi.EARG
    assert ok(fft_hist=2, fft_n=2) == abi.OK and ok(fft_hist=512, fft_n=512) == abi.OK
    assert ok(fft_n=299) == abi.EARG and ok(fft_n=2049) == abi.EARG and ok(fft_hist=2, fft_n=1) == abi.EARG
    assert ok(fft_n=2048) == abi.OK and ok(fft_hist=512, fft_n=2048) == abi.OK
    assert ok(fft_fill=2) == abi.EARG and ok(fft_fill=-1) == abi.EARG and ok(fft_fill=1) == abi.OK
    for fs in (0.0, -10.0, float("nan"), float("inf"), -float("inf")):
        assert ok(fs=fs) == abi.EARG, fs
    for f in E.X.FIELDS:
        assert ok(null=f) == abi.EARG, f
    # everything gnss_acf_features checks
    assert ok(n_taps=24) == abi.EARG and ok(n_taps=26) == abi.EARG and ok(n_taps=0) == abi.EARG
    assert ok(numOverLap=1) == abi.EARG and ok(numOverLap=4097, cap=4) == abi.EARG and ok(numOverLap=0, cap=4, fs=1.0) == abi.EARG
    assert ok(numOverLap=4096) == abi.OK
    assert ok(ind_start=0) == abi.EARG and ok(ind_start=-3) == abi.EARG
    assert ok(corrSpacing=0.0) == abi.EARG and ok(corrSpacing=float("nan")) == abi.EARG
    assert ok(cap=9) == abi.EARG and ok(cap=10) == abi.OK
    assert ok(n=0) == abi.EARG and ok(n=abi.VT_MAX_CH + 1) == abi.EARG
    long = K.records("long")
    long.lens[2] = long.max_len + 1
    assert E.ext_run(pkg, long, cap=16)[0] == abi.EARG
    long.lens[2] = -1
    assert E.ext_run(pkg, long, cap=16)[0] == abi.EARG
    assert lib.gnss_acf_features_ext(None, None, None, None, 25, None, None) == abi.EARG
    # the table's
    one = np.zeros(4)
    p = one.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.gnss_acf_twiddle(1, p, p) == abi.EARG and lib.gnss_acf_twiddle(2049, p, p) == abi.EARG
    assert lib.gnss_acf_twiddle(4, None, p) == abi.EARG and lib.gnss_acf_twiddle(4, p, None) == abi.EARG


def test_mirror_data_labeled(pkg):
    """CalculateFeatures(extended=True): (1 + sum of windows) x 11 with the zero first row (:32,
    :165), F6-F8 after F5; without `extended` the 8 columns as before, and acf_features without the
    three lists."""
    r = K.records("long")
    prn, ele = [22, 3, 14], [54.23, 8.36, 24.23]
    par = dict(numOverLap=64, ind_start=7, fft_hist=5, fft_n=100, fft_fill=1)
    ct = {p: NS(taps_i=r.taps[c, 0, :, : r.lens[c]], taps_q=r.taps[c, 1, :, : r.lens[c]],
                DLLdiscri=r.rec[c, 7, : r.lens[c]]) for c, p in enumerate(prn)}
    want8, _ = K.twin(r, prn, ele, numOverLap=64, ind_start=7)
    chans = E.twin(pkg, r, **par)
    got = pkg.CalculateFeatures(ct, prn, ele, extended=True, **par)
    assert got.shape == (1 + 15 + 15 + 3, 11) and not np.any(got[0])
    for j, f in enumerate(pkg.abi.ACF_EXT_FIELDS):
        assert K.same_bits(got[1:, 8 + j], np.concatenate([ch[f] for ch in chans])), f
    old = pkg.CalculateFeatures(ct, prn, ele, numOverLap=64, ind_start=7)
    assert old.shape == (34, 8) and K.same_bits(old, got[:, :8])
    for col in (0, 1, 2, 4, 5, 6, 7):
        assert K.same_bits(old[:, col], want8[:, col]), col
    assert np.all(K.ulps(old[:, 3], want8[:, 3]) <= 2)
    # the per-channel form; fs by default 1000 / (numOverLap * pdi) (:172)
    f = pkg.acf_features(ct, prn, ele, extended=True, **par)
    assert tuple(pkg.abi.ACF_EXT_FIELDS) == ("numMLC", "fftFreq", "fftMag")
    assert pkg.abi.ACF_EXT_DEFAULTS == dict(fft_hist=300, fft_n=1024, fft_fill=0)
    for c, ch in enumerate(chans):
        assert K.same_bits(f.numMLC[c], ch["numMLC"]) and K.same_bits(f.fftFreq[c], ch["fftFreq"])
    k = [np.round(x * 100 / (1000.0 / 64)) for x in f.fftFreq]  # the bins
    slow = pkg.acf_features(ct, prn, ele, extended=True, pdi=10, **par)
    given = pkg.acf_features(ct, prn, ele, extended=True, fs=2.5, **par)
    for c in range(3):
        assert np.array_equal(slow.fftFreq[c], (k[c] * (1000.0 / 640)) / 100)
        assert np.array_equal(given.fftFreq[c], (k[c] * 2.5) / 100)
        assert K.same_bits(slow.fftMag[c], f.fftMag[c])
    plain = pkg.acf_features(ct, prn, ele, numOverLap=64, ind_start=7)
    assert not hasattr(plain, "numMLC") and K.same_bits(np.concatenate(plain.F2), np.concatenate(f.F2))
    with pytest.raises(TypeError):
        pkg.acf_features(ct, prn, ele, fft_hist=5)  # an extended parameter without extended=True
    with pytest.raises(TypeError):
        pkg.acf_features(ct, prn, ele, extended=True, fft_len=5)
    with pytest.raises(pkg.abi.GnssError) as e:
        pkg.acf_features(ct, prn, ele, extended=True, fft_hist=1)
    assert e.value.status == pkg.abi.EARG
