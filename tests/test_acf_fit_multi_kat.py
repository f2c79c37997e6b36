"""The multi-ray fit through the C-ABI on host sums (gnss_acf_fit_multi with ctx = NULL and
gnss_acf_fit_multi_window; csrc/acf_fit_multi.cpp over csrc/acf_fit_multi.h): no GPU. The host path
equals the numpy twin (acf_fit_multi_twin.py) bit for bit in every output, `searches` included,
over acf_fit_multi_common's case list and on hand-made inputs (non-finite rows, an all-zero vector,
duplicated taps, a candidate grid outside the taps); with max_paths = 1 it ties to
gnss_acf_fit_taps' one-path fit bit for bit; noise-free on-grid model vectors of one, two and three
paths come back exactly; the CPU chain scene -> GIVEN loop -> replay -> fit resolves two rays and
the direct path in every window; every GNSS_EARG case and the Python wrapper's errors."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import acf_common as K
import acf_fit_multi_common as M
import acf_fit_multi_twin as T
import acf_fit_taps_common as F2

MID = dict(q_min=-1.6, q_step=0.02, q_count=100, max_paths=3, sweeps=2, sep_min=5)


@pytest.mark.parametrize("name", list(M.CASES))
def test_host_path_equals_twin(pkg, name):
    """zI / zQ wanted and NULL."""
    s, par, windows = M.case(name)
    st, out = M.lib_run(pkg, s, **par)
    assert st == pkg.abi.OK and list(out.windows[: s.n]) == windows
    M.assert_equals_twin(out, T.fit(s.taps, s.n_rows, s.u, s.prompt, **par))
    st, bare = M.lib_run(pkg, s, want=False, **par)
    assert st == pkg.abi.OK
    M.assert_same_outputs(out, bare)
    assert np.all(out.paths[0, : windows[0]] > 0)


def test_non_finite_rows_give_no_fit(pkg):
    """A NaN tap, a NaN in the prompt's I, +inf and -inf in one series and a lone +inf: paths = 0,
    searches = 0 and every floating output NaN in those windows, the windows between them fitted."""
    s = M.sums(31, 20, [701], 703)
    t = s.taps[0]
    t[1, 3, 5] = np.nan
    t[0, 20, 210] = np.nan
    t[0, 7, 401], t[0, 7, 402] = np.inf, -np.inf
    t[1, 30, 650] = np.inf
    st, out = M.lib_run(pkg, s, **MID)
    assert st == pkg.abi.OK and out.windows[0] == 7
    M.assert_equals_twin(out, T.fit(s.taps, s.n_rows, s.u, s.prompt, **MID))
    bad = [0, 2, 4, 6]
    assert list(out.paths[0, :7] == 0) == [True, False, True, False, True, False, True]
    assert np.all(out.searches[0, bad] == 0) and np.all(out.searches[0, [1, 3, 5]] > 0)
    for f in T.FIELDS:
        assert np.all(np.isnan(out.arr[f][0, ..., bad])), f
    assert np.isnan(out.zQ[0, 3, 0]) and np.isnan(out.zI[0, 20, 2]) and not np.isfinite(out.zI[0, 7, 4])


def test_an_all_zero_vector_ties_go_to_the_lowest_index(pkg):
    """z = 0: every usable candidate fits with res = 0, so each search takes the lowest index it
    may: 0, then sep_min, then 2 sep_min behind the slots before it."""
    u = M.grid_u(61, 40)
    z = np.zeros(61)
    par = dict(q_min=-1.0, q_step=0.01, q_count=101, max_paths=3, sweeps=4, sep_min=5, gain_min=16.0)
    st, got = M.fit_window(pkg, z, z, u, 40, **par)
    assert st == pkg.abi.OK and M.same_vector(got, T.fit_vector(z, z, u, **par))
    assert got["paths"] == 1 and got["q"][0] == -1.0 and got["energy"] == 0 and got["searches"] == 2 + 3 + 4
    assert np.all(got["res"][:4] == 0) and np.isnan(got["res"][4])
    s = M.sums(61, 40, [130], 131)
    s.taps[:, :, :, :130] = 0.0
    st, out = M.lib_run(pkg, s, numOverLap=64, **par)
    assert st == pkg.abi.OK and list(out.windows) == [2]
    M.assert_equals_twin(out, T.fit(s.taps, s.n_rows, s.u, s.prompt, numOverLap=64, **par))
    assert np.all(out.arr["q"][0, 0, :2] == -1.0) and np.all(out.paths[0, :2] == 1)


def test_duplicated_and_unsorted_taps(pkg):
    rng = np.random.default_rng(4)
    u = np.concatenate([[0.0], rng.uniform(-1.9, 0.8, 24)])
    u = np.concatenate([u, u[5:13]])[rng.permutation(33)]  # eight taps twice, in any order
    prompt = int(np.flatnonzero(u == 0)[0])
    s = M.sums(33, prompt, [205, 64], 207, u=u)
    st, out = M.lib_run(pkg, s, numOverLap=64, **MID)
    assert st == pkg.abi.OK
    chans = T.fit(s.taps, s.n_rows, s.u, s.prompt, numOverLap=64, **MID)
    M.assert_equals_twin(out, chans)
    assert np.all(chans[0]["paths"] > 0)


def test_a_candidate_grid_outside_the_taps_forms_no_order(pkg):
    """Every candidate's triangle misses every tap: order 1 is not formed, paths = 0 after one
    search, q / A / bias NaN, res[0] and energy given."""
    s = M.sums(25, 12, [131], 131)
    par = dict(numOverLap=65, q_min=1.7, q_step=0.01, q_count=50)
    st, out = M.lib_run(pkg, s, **par)
    assert st == pkg.abi.OK and list(out.windows) == [2]
    M.assert_equals_twin(out, T.fit(s.taps, s.n_rows, s.u, s.prompt, **par))
    assert np.all(out.paths[0, :2] == 0) and np.all(out.searches[0, :2] == 1)
    assert np.all(np.isnan(out.arr["q"][0, :, :2])) and np.all(np.isnan(out.arr["bias"][0, :2]))
    assert np.all(out.arr["energy"][0, :2] > 0) and K.same_bits(out.arr["res"][0, 0, :2], out.arr["energy"][0, :2])
    assert np.all(np.isnan(out.arr["res"][0, 1:, :2]))


def test_one_path_ties_to_gnss_acf_fit_taps(pkg):
    """max_paths = 1 on the q grid that is gnss_acf_fit_taps' p grid: q[0], A[0], res[1], energy,
    zI, zQ equal its p1, A1p_re / A1p_im, res1, energy, zI, zQ bit for bit."""
    s = M.sums(61, 40, [301, 150], 303)
    s.taps[0, 0, 7, 150] = np.nan  # (a window without a fit in both)
    st, two = F2.lib_run(pkg, s, p_min=-0.40, p_step=0.01, p_count=81, e_min=0.3, e_step=0.5, e_count=2)
    st2, out = M.lib_run(pkg, s, q_min=-0.40, q_step=0.01, q_count=81, max_paths=1)
    assert st == st2 == pkg.abi.OK and list(out.windows) == list(two.windows) == [3, 1]
    for c, W in enumerate([3, 1]):
        assert K.same_bits(out.arr["q"][c, 0, :W], two.arr["p1"][c, :W])
        assert K.same_bits(out.arr["A_re"][c, 0, :W], two.arr["A1p_re"][c, :W])
        assert K.same_bits(out.arr["A_im"][c, 0, :W], two.arr["A1p_im"][c, :W])
        assert K.same_bits(out.arr["res"][c, 1, :W], two.arr["res1"][c, :W])
        assert K.same_bits(out.arr["energy"][c, :W], two.arr["energy"][c, :W])
        assert K.same_bits(out.zI[c, :, :W], two.zI[c, :, :W]) and K.same_bits(out.zQ[c, :, :W], two.zQ[c, :, :W])
    assert list(out.paths[0, :3]) == [1, 0, 1] and list(two.paths[0, :3] > 0) == [True, False, True]


def test_window_call_equals_the_windowed_call(pkg):
    s, par, windows = M.case("61taps-long-short")
    st, out = M.lib_run(pkg, s, **par)
    assert st == pkg.abi.OK
    search = {k: v for k, v in par.items() if k in T.SEARCH}
    for c, m in ((0, 0), (0, 9), (1, 0)):
        st, got = M.fit_window(pkg, out.zI[c, :, m], out.zQ[c, :, m], s.u, s.prompt, **search)
        assert st == pkg.abi.OK
        assert got["paths"] == out.paths[c, m] and got["searches"] == out.searches[c, m]
        for f in T.FIELDS:
            assert K.same_bits(got[f], out.arr[f][c, ..., m]), (c, m, f)


def q_at(i):
    return T.DEFAULTS["q_min"] + float(i) * T.DEFAULTS["q_step"]


IN_PHASE, OPPOSED, QUADRATURE = 1.0 + 0j, -1.0 + 0j, 1j
# Noise-free model vectors on -2.5:0.05:1.0: the paths' candidate indices of the default grid
# (q = -2.40 + 0.01 i; index 240 is q = 0) with the amplitude against the first path's 4096. The
# separations are 0.15 chip and more; in phase, opposed and in quadrature. Each was checked with the
# twin alone before it was listed.
MODELS = [
    [(240, IN_PHASE)],
    [(247, IN_PHASE)],
    [(100, QUADRATURE)],
    [(240, IN_PHASE), (180, 0.5 * OPPOSED)],
    [(240, IN_PHASE), (225, 0.5 * IN_PHASE)],
    [(247, IN_PHASE), (107, 0.5 * QUADRATURE)],
    [(240, IN_PHASE), (70, 0.5 * IN_PHASE)],
    [(240, IN_PHASE), (180, 0.5 * OPPOSED), (100, 0.4 * QUADRATURE)],
    [(240, IN_PHASE), (225, 0.5 * IN_PHASE), (195, 0.4 * OPPOSED)],
    [(243, IN_PHASE), (198, 0.5 * QUADRATURE), (73, 0.4 * IN_PHASE)],
    [(240, IN_PHASE), (200, 0.6 * OPPOSED), (160, 0.3 * IN_PHASE)],
]


@pytest.mark.parametrize("k", range(len(MODELS)))
def test_noise_free_model_vectors_come_back_exactly(pkg, k):
    """max_paths = the paths of the model (a further order of an exact fit would divide rounding
    residues): paths, every position exactly, the amplitudes within 1e-9 relative, the twin's bits."""
    paths = [(q_at(i), 4096.0 * a) for i, a in MODELS[k]]
    zI, zQ = M.model(M.WIDE, paths)
    search = dict({k2: T.DEFAULTS[k2] for k2 in T.SEARCH}, max_paths=len(paths))
    st, got = M.fit_window(pkg, zI, zQ, M.WIDE, 50, **search)
    tw = T.fit_vector(zI, zQ, M.WIDE, **search)
    assert st == pkg.abi.OK and M.same_vector(got, tw), (got, tw)
    assert got["paths"] == len(paths), got
    want = sorted(paths, key=lambda p: -p[0])
    for j, (q, A) in enumerate(want):
        assert got["q"][j] == q, (j, got["q"], q)
        assert abs(got["A_re"][j] + 1j * got["A_im"][j] - A) <= 1e-9 * 4096.0, (j, got["A_re"][j], got["A_im"][j], A)
    assert got["bias"] == want[0][0] and np.all(np.isnan(got["q"][len(paths):]))


def test_thread_count_does_not_change_the_bits(pkg):
    s = M.sums(61, 40, [1001, 340], 1003)
    st, many = M.lib_run(pkg, s)
    cpus = os.sched_getaffinity(0)
    try:  # one host thread: the library sizes its pool by the CPUs it may run on
        os.sched_setaffinity(0, {min(cpus)})
        st1, single = M.lib_run(pkg, s)
    finally:
        os.sched_setaffinity(0, cpus)
    assert st == st1 == pkg.abi.OK and many.windows[0] == 10
    M.assert_same_outputs(many, single)


# ---- the CPU chain -------------------------------------------------------------------------------
CHAIN_RAYS = ((0.6, 0.5, 0.5), (1.4, 0.4, 0.25))  # (chips late, amplitude ratio, phase in cycles)


def test_cpu_chain_resolves_two_rays(pkg, po):
    """PRN 3 alone at 55 dB-Hz with rays 0.6 chip late (half the amplitude, opposed) and 1.4 chips
    late (0.4, in quadrature): gnss_synth_scene_host -> the oracle's GIVEN loop for 600 rows -> rows
    99-599 replayed on the host at -2.5:0.05:1.0 -> the default fit on five windows of 100 rows. In
    every window paths = 3, |e[k] - truth| <= 0.05 (one tap spacing, the bound of the existing
    end-to-end tests) and |ratio[k] - truth| <= 0.1. Measured here: e 0.59..0.62 and 1.39..1.40,
    ratios 0.490..0.503 and 0.399..0.408, res2/res3 215..407. gnss_acf_fit_taps on the same sums
    reports at most two paths. bias is printed, not asserted: the scene gives no truth for it."""
    sc = pkg.synth.scene_of(pkg.synth.scenario([3], [3683], [990.0], [55.0], skip_ms=2))
    for late, ratio, cyc in CHAIN_RAYS:
        pkg.synth.add_ray(sc, 3, late, ratio, phase_cycles=cyc)
    file, signal, _, track, _, _ = pkg.initParameters()
    file.skip, file.data = 2, pkg.synth.generate_scene_host(sc, 0, (2 + 1 + 600 + 4) * 58000)
    A = SimpleNamespace(sv=np.array([3]), SNR=np.array([20.0]), Doppler=np.zeros(1), codedelay=np.array([3683]),
                        fineFreq=np.array([4580990.0]))
    buf = po.trackingCT_multiCorr(file, signal, track, A, datalength=600, raw=True)
    assert buf.status == 0
    t = pkg.replay_rows(buf, A, file, signal, loop="given", rows=range(99, 600))
    taps = pkg.colon(-2.5, 0.05, 1.0)
    sums, _ = pkg.replay_correlate(file, signal, t, taps)
    f = pkg.acf_fit_multi(sums, t.n_rows, taps, numOverLap=100)
    two = pkg.acf_fit_taps(sums, t.n_rows, taps, numOverLap=100)
    print("multi fit paths", f.paths[0], "searches", f.searches[0], "bias", f.bias[0])
    print("          e", np.round(f.e[0][1:3], 3).tolist(), "ratio", np.round(f.ratio[0][1:3], 4).tolist())
    print("          dphi", np.round(f.dphi_cycles[0][1:3], 4).tolist(), "res(m-1)/res(m)",
          np.round(f.res[0][:3] / f.res[0][1:4], 1).tolist())
    print("two-path fit paths", two.paths[0], "e", two.e[0], "ratio", np.round(two.ratio[0], 3), "bias", two.bias[0])
    assert f.windows[0] == 5 and f.prompt == 50
    assert np.all(f.paths[0] == 3)
    for k, (late, ratio, _) in enumerate(CHAIN_RAYS, start=1):
        assert np.all(np.abs(f.e[0][k] - late) <= 0.05), (k, f.e[0][k])
        assert np.all(np.abs(f.ratio[0][k] - ratio) <= 0.1), (k, f.ratio[0][k])
    assert np.all(two.paths[0] <= 2)
    tw = T.fit(sums, t.n_rows, taps, 50, numOverLap=100)[0]
    assert np.array_equal(f.paths[0], tw["paths"]) and np.array_equal(f.searches[0], tw["searches"])
    for name in T.FIELDS:
        assert K.same_bits(getattr(f, name)[0], tw[name]), name


# ---- refusals and the wrapper --------------------------------------------------------------------
def refusals(abi):
    """(name, keywords of M.lib_run that make the call one to refuse)"""
    nan, inf = float("nan"), float("inf")
    bad_u = M.grid_u(31, 20)
    bad_u[30] = inf
    nan_u = M.grid_u(31, 20)
    nan_u[0] = nan
    return [("n = 0", dict(n=0)), ("n = 33", dict(n=33)), ("n_taps = 0", dict(n_taps=0)),
            ("n_taps = 257", dict(n_taps=257)), ("prompt = -1", dict(prompt=-1)), ("prompt = n_taps", dict(prompt=31)),
            ("u null", dict(u=None, n_taps=31)), ("u inf", dict(u=bad_u)), ("u NaN", dict(u=nan_u)),
            ("numOverLap = 1", dict(numOverLap=1)), ("numOverLap = 4097", dict(numOverLap=4097)),
            ("ind_start = 0", dict(ind_start=0)), ("q_step = 0", dict(q_step=0.0)), ("q_step < 0", dict(q_step=-0.01)),
            ("q_step NaN", dict(q_step=nan)), ("q_step inf", dict(q_step=inf)), ("q_min inf", dict(q_min=inf)),
            ("q_min NaN", dict(q_min=nan)), ("q_count = 0", dict(q_count=0)), ("q_count = 4097", dict(q_count=4097)),
            ("max_paths = 0", dict(max_paths=0)), ("max_paths = 5", dict(max_paths=5)), ("sweeps = -1", dict(sweeps=-1)),
            ("sweeps = 17", dict(sweeps=17)), ("sep_min = 0", dict(sep_min=0)), ("sep_min > q_count", dict(sep_min=101)),
            ("gain_min < 0", dict(gain_min=-1.0)), ("gain_min NaN", dict(gain_min=nan)), ("taps null", dict(taps=None)),
            ("n_rows null", dict(n_rows=None)), ("max_rows = 0", dict(max_rows=0)),
            ("n_rows above max_rows", dict(n_rows=np.array([206, 100], dtype=np.int64))),
            ("n_rows < 0", dict(n_rows=np.array([205, -1], dtype=np.int64))), ("cap too small", dict(cap=1)),
            ("an unknown flag", dict(flags=2)), ("a device pointer without a context", dict(flags=abi.OUT_DEVICE))]


def test_refusals(pkg):
    s = M.sums(31, 20, [205, 100], 205)
    st, good = M.lib_run(pkg, s, **MID)
    assert st == pkg.abi.OK and list(good.windows) == [2, 0]
    for name, kw in refusals(pkg.abi):
        st, out = M.lib_run(pkg, s, **dict(MID, **kw))
        assert st == pkg.abi.EARG, (name, st)
        assert out.untouched(), name
    lib = pkg.abi.load()
    cfg, keep = M.c_cfg(pkg, 2, s.u, s.prompt, **MID)
    src = pkg.abi.GnssAcfFitTapsIn()
    src.taps, src.max_rows, src.n_rows = s.taps.ctypes.data, s.max_rows, s.n_rows.ctypes.data
    ok = M.OutBuffers(pkg, 2, 2, 31)
    assert lib.gnss_acf_fit_multi(None, None, M.C.byref(src), M.C.byref(ok.c)) == pkg.abi.EARG
    assert lib.gnss_acf_fit_multi(None, M.C.byref(cfg), None, M.C.byref(ok.c)) == pkg.abi.EARG
    assert lib.gnss_acf_fit_multi(None, M.C.byref(cfg), M.C.byref(src), None) == pkg.abi.EARG
    ok.c.res = None  # a null output array
    assert lib.gnss_acf_fit_multi(None, M.C.byref(cfg), M.C.byref(src), M.C.byref(ok.c)) == pkg.abi.EARG
    assert ok.untouched()
    # the window call: a null vector, a bad search, cap = 0
    z = np.zeros(31)
    assert M.fit_window(pkg, z, z, s.u, 20, **MID)[0] == pkg.abi.OK
    assert M.fit_window(pkg, z, z, s.u, 31, **MID)[0] == pkg.abi.EARG
    assert M.fit_window(pkg, z, z, s.u, 20, **dict(MID, max_paths=5))[0] == pkg.abi.EARG
    zp = z.ctypes.data_as(M.C.POINTER(M.C.c_double))
    one = M.OutBuffers(pkg, 1, 1, 31)
    assert lib.gnss_acf_fit_multi_window(M.C.byref(cfg), None, zp, M.C.byref(one.c)) == pkg.abi.EARG
    one.c.cap = 0
    assert lib.gnss_acf_fit_multi_window(M.C.byref(cfg), zp, zp, M.C.byref(one.c)) == pkg.abi.EARG
    assert one.untouched()
    st, again = M.lib_run(pkg, s, **MID)  # and a good call after them
    assert st == pkg.abi.OK
    M.assert_same_outputs(good, again)


def test_python_wrapper(pkg):
    s = M.sums(61, 40, [301, 150], 303)
    res = pkg.acf_fit_multi(s.taps, s.n_rows, s.u, want_acf=True, **MID)  # the prompt: the one tap with u == 0
    assert res.prompt == 40 and list(res.windows) == [3, 1] and res.kernel_ms == 0.0
    chans = T.fit(s.taps, s.n_rows, s.u, 40, **MID)
    for c, ch in enumerate(chans):
        assert np.array_equal(res.paths[c], ch["paths"]) and np.array_equal(res.searches[c], ch["searches"])
        for f in T.FIELDS + ["zI", "zQ"]:
            assert K.same_bits(getattr(res, f)[c], ch[f]), (c, f)
        a = ch["A_re"] + 1j * ch["A_im"]
        with np.errstate(invalid="ignore"):
            assert K.same_bits(res.ratio[c], np.abs(a) / np.abs(a[0]))
            assert K.same_bits(res.e[c], ch["q"][0] - ch["q"])
        assert K.same_bits(res.bias_m[c], ch["bias"] * 299792458.0 / 1.023e6)
        assert res.dphi_cycles[c].shape == ch["q"].shape and np.all(np.abs(res.dphi_cycles[c][0]) < 1e-12)
    assert pkg.abi.ACF_FIT_MULTI_DEFAULTS == T.DEFAULTS and pkg.abi.ACF_MULTI_MAX_PATHS == T.MAX_PATHS
    with pytest.raises(ValueError):
        pkg.acf_fit_multi(s.taps, s.n_rows, s.u + 0.01)  # no tap with u == 0
    with pytest.raises(TypeError):
        pkg.acf_fit_multi(s.taps, s.n_rows, s.u, e_count=3)  # (gnss_acf_fit_taps' grid)
    with pytest.raises(ValueError):
        pkg.acf_fit_multi(s.taps, s.n_rows, s.u[:60])
    with pytest.raises(pkg.abi.GnssError):
        pkg.acf_fit_multi(s.taps, s.n_rows, s.u, max_paths=5)
