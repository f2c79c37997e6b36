"""ACF/CalculateFeatures.m through the C-ABI on host records (gnss_acf_features with ctx = NULL;
csrc/acf.cpp over csrc/acf.h): no GPU. The host path equals the numpy twin (acf_twin.py) bit for
bit on every field -- F1 within 2 ulp, its pow being the C library's on one side and Python's on
the other -- on seeded records with hand-made tie / edge / NaN rows, over the window rule's
lengths, both start rows and three window widths; the script's known answers; every GNSS_EARG
case; and the mirror's data_labeled."""
from types import SimpleNamespace as NS

import numpy as np
import pytest

import acf_common as K
import acf_twin as T


@pytest.mark.parametrize("numOverLap", [100, 2, 64])
@pytest.mark.parametrize("ind_start", [1, 7])
@pytest.mark.parametrize("shape", ["short", "long"])
def test_host_path_equals_twin(pkg, shape, ind_start, numOverLap):
    r = K.records(shape)
    par = dict(ind_start=ind_start, numOverLap=numOverLap)
    st, out = K.lib_run(pkg, r, want=True, **par)
    assert st == pkg.abi.OK
    _, chans = K.twin(r, **par)
    K.assert_equals_twin(r, out, chans, out.ind, out.corr)
    st, bare = K.lib_run(pkg, r, **par)  # the optional outputs NULL: the same features
    assert st == pkg.abi.OK
    K.assert_same_outputs(out, bare)


def test_hand_made_rows_pick_the_first_index(pkg):
    r = K.records("long")
    st, out = K.lib_run(pkg, r, want=True)
    assert st == pkg.abi.OK and set(r.want) == {0, 1, 2}
    for c, rows in r.want.items():
        for row, idx in rows.items():
            assert out.ind[c, row] == idx, (c, row)
    # the exact ties are exact: 5 from (3,4), (5,0) and (4,3)
    row = min(r.want[0])
    assert out.corr[0, 0, row] == out.corr[0, 12, row] == out.corr[0, 24, row] == 5.0
    assert np.all(np.isnan(out.corr[0, :, row + 8]))
    assert np.isnan(out.arr["meanMax"][0, 0])  # the all-NaN row's prompt is in channel 0's first window


def test_window_count_quirk(pkg):
    """:234: floor((L - ind_start) / numOverLap), so a multiple of numOverLap loses its last window."""
    for L, W in ((1000, 9), (1001, 10), (100, 0), (101, 1), (1, 0), (0, 0)):
        r = K.records("long", lens=[L, L, L], hand=False)
        st, out = K.lib_run(pkg, r)
        assert st == pkg.abi.OK and list(out.windows) == [W] * 3, (L, out.windows)
    r = K.records("long", lens=[100, 100, 100], hand=False)
    one = {5: NS(taps_i=r.taps[0, 0, :, :100], taps_q=r.taps[0, 1, :, :100], DLLdiscri=r.rec[0, 7, :100])}
    rows = pkg.CalculateFeatures(one, [5], [30.0])  # no window: the zero row alone
    assert rows.shape == (1, 8) and not np.any(rows)


def constant_peak(col, L=301, max_len=303):
    r = K.records("long", lens=[L, L, L], max_len=max_len, hand=False)
    r.taps[:, :, :, :L] = 1.0
    r.taps[:, 0, col - 1, :L] = 100.0
    return r


def test_tmp_delay_running_mean_then_zero_filled_row(pkg):
    """:238 for a constant index k: window 1's mean(maxCorrInd(m,:)) is the running mean, so every
    tmpDelay is 0; a later window's row is zero filled, so tmpDelay(n) = (k - n*k/N) * corrSpacing,
    tmpDelay(1) = (k - k/100) * 0.05."""
    k = 15
    r = constant_peak(k)
    st, out = K.lib_run(pkg, r)
    assert st == pkg.abi.OK and list(out.windows) == [3, 3, 3]
    assert out.arr["varDelay"][0, 0] == 0.0
    s = 0.0
    for n in range(1, 101):
        t = (k - (n * k) / 100) * 0.05
        s = s + t * t if n > 1 else t * t
    assert out.arr["varDelay"][0, 1] == s / 100 and out.arr["varDelay"][0, 2] == s / 100
    # numOverLap = 2 isolates tmpDelay(1) of window 2: tmpDelay(2) = (k - 2k/2) * 0.05 = 0
    st, out = K.lib_run(pkg, r, numOverLap=2)
    assert st == pkg.abi.OK
    t1 = (k - k / 2) * 0.05
    assert out.arr["varDelay"][0, 0] == 0.0 and out.arr["varDelay"][0, 1] == (t1 * t1) / 2
    st, out = K.lib_run(pkg, r, numOverLap=100, ind_start=7)
    t1 = (k - k / 100) * 0.05
    assert st == pkg.abi.OK and out.arr["varDelay"][0, 1] > t1 * t1 / 100 > 0


def test_prompt_peak_is_not_zero_delay(pkg):
    """cenDelay = 0.6 / 0.05 + 1 = 12.999999999999998 in fp64 (:176): a peak that sits on the prompt
    tap in every row contributes (13 - cenDelay) * 0.05 = 8.881784197001253e-17 chip per row, not 0.
    F2 is exactly minus that where the window's sum is exact (numOverLap = 2: (t + t) / 2 = t); the
    default window's left-to-right sum of 100 such terms rounds 17 times on the way, and F2 is
    -8.881784197001236e-17, the value of the loop below."""
    r = constant_peak(13)
    st, out = K.lib_run(pkg, r, numOverLap=2)
    assert st == pkg.abi.OK and out.windows[0] == 150
    assert np.all(out.arr["F2"][:, :150] == -8.881784197001253e-17)
    st, out = K.lib_run(pkg, r)
    assert st == pkg.abi.OK
    t = (13 - (0.6 / 0.05 + 1)) * 0.05
    s = t
    for _ in range(99):
        s = s + t
    assert t == 8.881784197001253e-17 and -(s / 100 + 0.0) * 1 == -8.881784197001236e-17
    assert np.all(out.arr["F2"][:, :3] == -8.881784197001236e-17)
    v = s = float(np.sqrt(100.0 * 100.0 + 1.0))
    for _ in range(99):
        s = s + v
    assert np.all(out.arr["meanMax"][:, :3] == s / 100)
    assert np.all(out.arr["varDelay"][:, 0] == 0.0)


def test_every_earg_case(pkg):
    abi = pkg.abi
    r = K.records("long")
    ok = lambda **kw: K.lib_run(pkg, r, **kw)[0]
    assert ok() == abi.OK
    assert ok(n_taps=24) == abi.EARG and ok(n_taps=26) == abi.EARG and ok(n_taps=0) == abi.EARG
    assert ok(numOverLap=1) == abi.EARG and ok(numOverLap=4097, cap=4) == abi.EARG and ok(numOverLap=0, cap=4) == abi.EARG
    assert ok(numOverLap=4096) == abi.OK and ok(numOverLap=2) == abi.OK
    assert ok(ind_start=0) == abi.EARG and ok(ind_start=-3) == abi.EARG
    assert ok(corrSpacing=0.0) == abi.EARG and ok(corrSpacing=-0.05) == abi.EARG
    assert ok(corrSpacing=float("nan")) == abi.EARG
    assert ok(cap=9) == abi.EARG and ok(cap=10) == abi.OK  # channel 1 (L = 1001) has 10 windows
    assert ok(n=0) == abi.EARG and ok(n=abi.VT_MAX_CH + 1) == abi.EARG
    long = K.records("long")
    long.lens[2] = long.max_len + 1
    assert K.lib_run(pkg, long, cap=16)[0] == abi.EARG
    long.lens[2] = -1
    assert K.lib_run(pkg, long, cap=16)[0] == abi.EARG
    lib = abi.load()
    assert lib.gnss_acf_features(None, None, None, 25, None) == abi.EARG


def test_mirror_data_labeled(pkg):
    """CalculateFeatures: (1 + sum of windows) x 8, the zero first row (:165), the channels in
    prnList's order whatever the PRNs' order, from the scalar loops' structs (taps_i / taps_q,
    25 x steps, DLLdiscri or codeError) and from the vector loop's (tap_i / tap_q, steps x 25)."""
    r = K.records("long")
    prn, ele = [22, 3, 14], [54.23, 8.36, 24.23]
    want, chans = K.twin(r, prn, ele)
    ct = {p: NS(taps_i=r.taps[c, 0, :, : r.lens[c]], taps_q=r.taps[c, 1, :, : r.lens[c]],
                **{("DLLdiscri" if c else "codeError"): r.rec[c, 7, : r.lens[c]]}) for c, p in enumerate(prn)}
    vt = {p: NS(tap_i=r.taps[c, 0, :, : r.lens[c]].T, tap_q=r.taps[c, 1, :, : r.lens[c]].T,
                codeError=r.rec[c, 7, : r.lens[c]]) for c, p in enumerate(prn)}
    track = pkg.initParameters()[3]
    buf = pkg.TrackOutBuffers(3, track, 25, ctPOS=r.max_len)  # the loops' raw buffers: channel c is prnList[c]
    buf.rec[:], buf.taps[:], buf.len[:] = r.rec, r.taps, r.lens
    for src in (ct, vt, pkg.StructArray(ct), buf):
        got = pkg.CalculateFeatures(src, prn, ele)
        assert got.shape == want.shape == (1 + 9 + 10 + 2, 8)
        assert not np.any(got[0])
        assert list(got[1:, 0]) == [22.0] * 9 + [3.0] * 10 + [14.0] * 2
        assert list(got[1:, 1]) == [54.23] * 9 + [8.36] * 10 + [24.23] * 2
        for col in (2, 4, 5, 6, 7):
            assert K.same_bits(got[:, col], want[:, col]), col
        assert np.all(K.ulps(got[:, 3], want[:, 3]) <= 2)
    # the per-channel form, with the script's other parameters
    f = pkg.acf_features(ct, prn, ele, numOverLap=64, ind_start=7, want_index=True, want_corr=True)
    _, chans = K.twin(r, prn, ele, numOverLap=64, ind_start=7)
    assert list(f.windows) == [c["windows"] for c in chans]
    for c, ch in enumerate(chans):
        assert K.same_bits(f.F2[c], ch["F2"]) and K.same_bits(f.varCodeDisc[c], ch["varCodeDisc"])
        assert np.array_equal(f.maxCorrInd[c, : r.lens[c]], ch["maxCorrInd"])
        assert K.same_bits(f.corr[c, :, : r.lens[c]], ch["corr"])
    with pytest.raises(TypeError):
        pkg.acf_features(ct, prn, ele, numOverlap=64)
    with pytest.raises(pkg.abi.GnssError) as e:
        pkg.acf_features(ct, prn, ele, numOverLap=1)
    assert e.value.status == pkg.abi.EARG
