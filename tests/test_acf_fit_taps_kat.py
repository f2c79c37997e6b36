"""The two-path fit on any tap grid through the C-ABI on host sums (gnss_acf_fit_taps with
ctx = NULL and gnss_acf_fit_taps_window; csrc/acf_fit_taps.cpp over csrc/acf_fit_taps.h): no GPU.
The host path equals the numpy twin (acf_fit_taps_twin.py) bit for bit in every output over the tap
counts, prompt positions, window widths and start rows, on a non-uniform and an unsorted grid and
on hand-made non-finite rows; at 25 taps it equals gnss_acf_fit and gnss_acf_fit_window bit for bit;
noise-free model vectors on -2.5:0.05:1.0 come back exactly; every GNSS_EARG case and the Python
wrapper's errors."""
import os

import numpy as np
import pytest

import acf_common as K
import acf_fit_common as F25
import acf_fit_taps_common as F
import acf_fit_taps_twin as T

MID = dict(p_min=-0.2, p_step=0.1, p_count=5, e_min=0.1, e_step=0.3, e_count=7)  # 5 x 7 hypotheses

# (n_taps, prompt, numOverLap, ind_start): every tap count with the prompt at 0, in the middle and
# at n_taps - 1, every window width and both start rows
CASES = [(1, 0, 2, 1), (2, 0, 64, 7), (2, 1, 100, 1), (25, 0, 100, 7), (25, 12, 2, 1), (25, 24, 64, 1),
         (31, 15, 100, 1), (31, 30, 2, 7), (33, 0, 64, 1), (33, 16, 100, 7), (61, 30, 100, 1), (61, 60, 64, 7),
         (61, 0, 2, 1), (256, 0, 100, 1), (256, 128, 64, 7), (256, 255, 100, 1)]


@pytest.mark.parametrize("n_taps,prompt,numOverLap,ind_start", CASES)
def test_host_path_equals_twin(pkg, n_taps, prompt, numOverLap, ind_start):
    """A long channel beside a short one and one of 0 rows; zI / zQ wanted and NULL."""
    n_rows = [230, 101, 0] if numOverLap > 2 else [37, 12, 0]
    s = F.sums(n_taps, prompt, n_rows, max(n_rows) + 3)
    par = dict(ind_start=ind_start, numOverLap=numOverLap, **MID)
    st, out = F.lib_run(pkg, s, **par)
    assert st == pkg.abi.OK
    chans = T.fit(s.taps, s.n_rows, s.u, s.prompt, **par)
    assert chans[0]["windows"] > chans[1]["windows"] >= 0 and chans[2]["windows"] == 0
    F.assert_equals_twin(out, chans)
    st, bare = F.lib_run(pkg, s, want=False, **par)
    assert st == pkg.abi.OK
    F.assert_same_outputs(out, bare)
    if n_taps >= 25:
        assert any(np.any(ch["paths"] > 0) for ch in chans)


def test_default_grid_equals_twin(pkg):
    """The 81 x 196 grid on 61 taps at -1.5:0.05:1.5, two windows."""
    s = F.sums(61, 30, [201], 203)
    st, out = F.lib_run(pkg, s)
    assert st == pkg.abi.OK and out.windows[0] == 2
    F.assert_equals_twin(out, T.fit(s.taps, s.n_rows, s.u, s.prompt))
    assert np.all(out.paths[0, :2] == 2), out.paths  # (the seeded sums hold a ray 0.4 chip late)
    assert np.all(np.abs(out.arr["e"][0, :2] - 0.4) <= 0.05)


def test_non_uniform_and_unsorted_grids(pkg):
    rng = np.random.default_rng(3)
    u = np.sort(np.concatenate([[0.0], rng.uniform(-1.6, 0.8, 32)]))  # non-uniform, ascending
    for order in (np.arange(33), rng.permutation(33)):                 # ... and in any order
        uu = u[order]
        prompt = int(np.flatnonzero(uu == 0)[0])
        s = F.sums(33, prompt, [205, 64], 207, u=uu)
        st, out = F.lib_run(pkg, s, numOverLap=64, **MID)
        assert st == pkg.abi.OK
        chans = T.fit(s.taps, s.n_rows, s.u, s.prompt, numOverLap=64, **MID)
        F.assert_equals_twin(out, chans)
        assert np.all(chans[0]["paths"] > 0)


def test_non_finite_rows_give_no_fit(pkg):
    """Hand-made rows: a NaN tap, a NaN in the prompt's I (sign -1, the sum NaN), +inf and -inf in
    one series (their signed sum NaN or infinite) and a lone +inf: paths = 0 and every output NaN
    in those windows, the windows between them fitted."""
    s = F.sums(31, 15, [701], 703)
    t = s.taps[0]
    t[1, 3, 5] = np.nan            # window 0: a NaN in tap 3's Q
    t[0, 15, 210] = np.nan         # window 2: the prompt's I
    t[0, 7, 401], t[0, 7, 402] = np.inf, -np.inf  # window 4
    t[1, 30, 650] = np.inf         # window 6
    st, out = F.lib_run(pkg, s, **MID)
    assert st == pkg.abi.OK and out.windows[0] == 7
    chans = T.fit(s.taps, s.n_rows, s.u, s.prompt, **MID)
    F.assert_equals_twin(out, chans)
    assert list(out.paths[0, :7] == 0) == [True, False, True, False, True, False, True]
    for f in T.FIELDS:
        assert np.all(np.isnan(out.arr[f][0, [0, 2, 4, 6]])), f
    assert np.isnan(out.zQ[0, 3, 0]) and np.isnan(out.zI[0, 15, 2]) and not np.isfinite(out.zI[0, 7, 4])
    assert out.zQ[0, 30, 6] in (np.inf, -np.inf)


def test_thread_count_does_not_change_the_bits(pkg):
    s = F.sums(61, 30, [1001, 340], 1003)
    st, many = F.lib_run(pkg, s, **MID)
    cpus = os.sched_getaffinity(0)
    try:  # one host thread: the library sizes its pool by the CPUs it may run on
        os.sched_setaffinity(0, {min(cpus)})
        st1, single = F.lib_run(pkg, s, **MID)
    finally:
        os.sched_setaffinity(0, cpus)
    assert st == st1 == pkg.abi.OK and many.windows[0] == 10
    F.assert_same_outputs(many, single)


@pytest.mark.parametrize("orient", [1, -1])
@pytest.mark.parametrize("shape,numOverLap", [("long", 100), ("short", 2), ("short", 64)])
def test_at_25_taps_equals_gnss_acf_fit(pkg, orient, shape, numOverLap):
    """acf_common's seeded records, hand-made rows included, through gnss_acf_fit and, with
    u[j] = (orient*(j-12))*corrSpacing and prompt 12, through gnss_acf_fit_taps: every output and
    zI / zQ bit for bit, at gnss_acf_fit's default grid."""
    r = K.records(shape, hand=True)
    par = dict(numOverLap=numOverLap, e_count=96)
    st, ref = F25.lib_run(pkg, r, orient=orient, **par)
    assert st == pkg.abi.OK
    u = (orient * (np.arange(25) - 12.0)) * 0.05
    s = F.NS(taps=r.taps, n_rows=r.lens, max_rows=r.max_len, n=r.n, n_taps=25, prompt=12, u=u)
    st, out = F.lib_run(pkg, s, **par)
    assert st == pkg.abi.OK
    F.assert_same_outputs(ref, out)
    assert np.any(ref.paths == 0)  # (the hand-made rows' windows)
    if numOverLap != 64:           # (64 rows from row 0 or 64: every window of 99..101 rows holds one)
        assert np.any(ref.paths > 0)


@pytest.mark.parametrize("orient", [1, -1])
def test_window_equals_gnss_acf_fit_window(pkg, orient):
    u = (orient * (np.arange(25) - 12.0)) * 0.05
    A0 = 3000.0 * np.exp(2j * np.pi * 0.07)
    rng = np.random.default_rng(2)
    for p, e, ph, noise in ((0.16, 0.5, 0.25, 0.0), (0.0, 0.3, 0.1234, 0.01), (-0.23, 0.95, 0.5, 0.01), (0.1, 0.5, 0.0, 0.0)):
        zI, zQ = F25.model(p, e, A0, 0.5 * A0 * np.exp(2j * np.pi * ph), orient)
        zI, zQ = zI + rng.normal(0, noise * abs(A0), 25), zQ + rng.normal(0, noise * abs(A0), 25)
        st, ref = F25.fit_window(pkg, zI, zQ, orient)
        st2, got = F.fit_window(pkg, zI, zQ, u, 12, e_count=96)
        assert st == st2 == pkg.abi.OK and got["paths"] == ref["paths"] > 0
        assert all(K.same_bits(got[f], ref[f]) for f in T.FIELDS), (got, ref)
    zI[4] = np.nan
    st, ref = F25.fit_window(pkg, zI, zQ, orient)
    st2, got = F.fit_window(pkg, zI, zQ, u, 12, e_count=96)
    assert st == st2 == pkg.abi.OK and got["paths"] == ref["paths"] == 0 and all(np.isnan(got[f]) for f in T.FIELDS)


def grid_point(ip, ie):
    d = T.DEFAULTS
    return d["p_min"] + ip * d["p_step"], d["e_min"] + ie * d["e_step"]


# A0 a power of two: A0 * R is exact, so the one-path fit of a lone path has res1 = 0 exactly
A0 = 4096.0 + 0j


@pytest.mark.parametrize("ip", [40, 47])       # p = 0 and 0.07
@pytest.mark.parametrize("ie", [85, 165, 195])  # e = 0.9, 1.7 and 2.0
def test_noise_free_model_on_the_wide_grid(pkg, ip, ie):
    """A1 = 0.5 A0 exp(j phi) on -2.5:0.05:1.0: exactly the grid's p and e, the ratio within 1e-9
    of 0.5, paths = 2, and the twin's bits."""
    u = pkg.colon(-2.5, 0.05, 1.0)
    assert len(u) == 71 and u[50] == 0
    p, e = grid_point(ip, ie)
    assert abs(p - (0.0, 0.07)[ip == 47]) < 1e-12 and abs(e - {85: 0.9, 165: 1.7, 195: 2.0}[ie]) < 1e-12
    for phi in (0.0, 0.9):
        zI, zQ = F.model(u, p, e, A0, 0.5 * A0 * np.exp(1j * phi))
        st, got = F.fit_window(pkg, zI, zQ, u, 50)
        assert st == pkg.abi.OK and got["paths"] == 2, got
        assert got["p0"] == p and got["e"] == e and got["bias"] == p, (got["p0"], got["e"])
        ratio = np.hypot(got["A1_re"], got["A1_im"]) / np.hypot(got["A0_re"], got["A0_im"])
        assert abs(ratio - 0.5) <= 1e-9, ratio
        tw = T.fit_vector(zI, zQ, u, **{k: T.DEFAULTS[k] for k in T.GRID})
        assert tw["paths"] == 2 and all(K.same_bits(got[f], tw[f]) for f in T.FIELDS)


@pytest.mark.parametrize("ip", [40, 47])
def test_the_25_inner_taps_do_not_see_a_ray_at_1_7_chips(pkg, ip):
    """The e = 1.7 vector cut to the taps at -0.6..0.6: the reflected triangle (-2.7..-0.7 + p)
    touches none of them, the one-path fit is exact (res1 = 0), so paths = 1."""
    u = pkg.colon(-2.5, 0.05, 1.0)
    p, e = grid_point(ip, 165)
    zI, zQ = F.model(u, p, e, A0, 0.5 * A0 * np.exp(0.9j))
    inner = slice(50 - 12, 50 + 13)
    assert len(u[inner]) == 25 and abs(u[inner][0] + 0.6) < 1e-12
    st, got = F.fit_window(pkg, zI[inner], zQ[inner], u[inner], 12)
    assert st == pkg.abi.OK and got["paths"] == 1 and got["p1"] == p == got["bias"], got
    st, wide = F.fit_window(pkg, zI, zQ, u, 50)
    assert wide["paths"] == 2 and wide["e"] == e


def refusals(abi):
    """(name, keywords of F.lib_run that make the call one to refuse)"""
    nan, inf = float("nan"), float("inf")
    bad_u = F.grid_u(31, 15)
    bad_u[30] = inf
    nan_u = F.grid_u(31, 15)
    nan_u[0] = nan
    return [("n = 0", dict(n=0)), ("n = 33", dict(n=33)), ("n_taps = 0", dict(n_taps=0)),
            ("n_taps = 257", dict(n_taps=257)), ("prompt = -1", dict(prompt=-1)), ("prompt = n_taps", dict(prompt=31)),
            ("u null", dict(u=None, n_taps=31)), ("u inf", dict(u=bad_u)), ("u NaN", dict(u=nan_u)),
            ("numOverLap = 1", dict(numOverLap=1)), ("numOverLap = 4097", dict(numOverLap=4097)),
            ("ind_start = 0", dict(ind_start=0)), ("p_step = 0", dict(p_step=0.0)), ("e_step < 0", dict(e_step=-0.01)),
            ("p_step NaN", dict(p_step=nan)), ("e_step inf", dict(e_step=inf)), ("p_min inf", dict(p_min=inf)),
            ("e_min NaN", dict(e_min=nan)), ("p_count = 0", dict(p_count=0)), ("e_count = 0", dict(e_count=0)),
            ("65537 hypotheses", dict(p_count=257, e_count=256)), ("ratio_max < 0", dict(ratio_max=-1.0)),
            ("gain_min NaN", dict(gain_min=nan)), ("taps null", dict(taps=None)), ("n_rows null", dict(n_rows=None)),
            ("max_rows = 0", dict(max_rows=0)), ("n_rows above max_rows", dict(n_rows=np.array([206, 100], dtype=np.int64))),
            ("n_rows < 0", dict(n_rows=np.array([205, -1], dtype=np.int64))), ("cap too small", dict(cap=1)),
            ("an unknown flag", dict(flags=2)), ("a device pointer without a context", dict(flags=abi.OUT_DEVICE))]


def test_refusals(pkg):
    s = F.sums(31, 15, [205, 100], 205)
    st, good = F.lib_run(pkg, s, **MID)
    assert st == pkg.abi.OK and list(good.windows) == [2, 0]
    for name, kw in refusals(pkg.abi):
        st, out = F.lib_run(pkg, s, **dict(MID, **kw))
        assert st == pkg.abi.EARG, (name, st)
        assert out.untouched(), name
    lib = pkg.abi.load()
    cfg, keep = F.c_cfg(pkg, 2, s.u, s.prompt, **MID)
    src = pkg.abi.GnssAcfFitTapsIn()
    src.taps, src.max_rows, src.n_rows = s.taps.ctypes.data, s.max_rows, s.n_rows.ctypes.data
    ok = F.OutBuffers(pkg, 2, 2, 31)
    assert lib.gnss_acf_fit_taps(None, None, F.C.byref(src), F.C.byref(ok.c)) == pkg.abi.EARG
    assert lib.gnss_acf_fit_taps(None, F.C.byref(cfg), None, F.C.byref(ok.c)) == pkg.abi.EARG
    assert lib.gnss_acf_fit_taps(None, F.C.byref(cfg), F.C.byref(src), None) == pkg.abi.EARG
    ok.c.res2 = None  # a null output array
    assert lib.gnss_acf_fit_taps(None, F.C.byref(cfg), F.C.byref(src), F.C.byref(ok.c)) == pkg.abi.EARG
    assert ok.untouched()
    # the window call: a null vector, a bad grid, cap = 0
    z = np.zeros(31)
    assert F.fit_window(pkg, z, z, s.u, 15, **MID)[0] == pkg.abi.OK
    assert F.fit_window(pkg, z, z, s.u, 31, **MID)[0] == pkg.abi.EARG
    assert F.fit_window(pkg, z, z, s.u, 15, **dict(MID, p_count=0))[0] == pkg.abi.EARG
    zp = z.ctypes.data_as(F.C.POINTER(F.C.c_double))
    one = F.OutBuffers(pkg, 1, 1, 31)
    assert lib.gnss_acf_fit_taps_window(F.C.byref(cfg), None, zp, F.C.byref(one.c)) == pkg.abi.EARG
    one.c.cap = 0
    assert lib.gnss_acf_fit_taps_window(F.C.byref(cfg), zp, zp, F.C.byref(one.c)) == pkg.abi.EARG
    assert one.untouched()
    st, again = F.lib_run(pkg, s, **MID)  # and a good call after them
    assert st == pkg.abi.OK
    F.assert_same_outputs(good, again)


def test_python_wrapper(pkg):
    s = F.sums(61, 30, [301, 150], 303)
    res = pkg.acf_fit_taps(s.taps, s.n_rows, s.u, want_acf=True, **MID)  # the prompt: the one tap with u == 0
    assert res.prompt == 30 and list(res.windows) == [3, 1] and res.kernel_ms == 0.0
    chans = T.fit(s.taps, s.n_rows, s.u, 30, **MID)
    for c, ch in enumerate(chans):
        assert np.array_equal(res.paths[c], ch["paths"])
        for f in T.FIELDS:
            assert K.same_bits(getattr(res, f)[c], ch[f]), (c, f)
        assert K.same_bits(res.zI[c], ch["zI"]) and K.same_bits(res.zQ[c], ch["zQ"])
        a0, a1 = ch["A0_re"] + 1j * ch["A0_im"], ch["A1_re"] + 1j * ch["A1_im"]
        assert K.same_bits(res.ratio[c], np.abs(a1) / np.abs(a0))
        assert K.same_bits(res.bias_m[c], ch["bias"] * 299792458.0 / 1.023e6)
        assert res.dphi_cycles[c].shape == ch["bias"].shape
    assert pkg.abi.ACF_FIT_TAPS_DEFAULTS == T.DEFAULTS
    with pytest.raises(ValueError):
        pkg.acf_fit_taps(s.taps, s.n_rows, s.u + 0.01)  # no tap with u == 0
    two = s.u.copy()
    two[3] = 0.0
    with pytest.raises(ValueError):
        pkg.acf_fit_taps(s.taps, s.n_rows, two)  # two of them
    assert pkg.acf_fit_taps(s.taps, s.n_rows, two, 30, **MID).prompt == 30
    with pytest.raises(TypeError):
        pkg.acf_fit_taps(s.taps, s.n_rows, s.u, corrSpacing=0.05)  # (the taps' coordinates are u)
    with pytest.raises(TypeError):
        pkg.acf_fit_taps(s.taps, s.n_rows, s.u, e_cnt=3)
    with pytest.raises(ValueError):
        pkg.acf_fit_taps(s.taps, s.n_rows, s.u[:60])
    with pytest.raises(pkg.abi.GnssError):
        pkg.acf_fit_taps(s.taps, s.n_rows, s.u, numOverLap=1)
