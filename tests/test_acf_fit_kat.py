"""The two-path fit of the 25-tap ACF through the C-ABI on host records (gnss_acf_fit with
ctx = NULL and gnss_acf_fit_window; csrc/acf_fit.cpp over csrc/acf_fit_taps.h at 25 taps): no GPU.
The host path equals the numpy twin (acf_fit_twin.py) bit for bit in every output on seeded records over the
window rule's lengths, both start rows, three window widths and two grids; the window counts are
gnss_acf_features'; model vectors on grid points come back exactly; the selection, ratio_max, the
sign wipe, ties and degenerate inputs, every GNSS_EARG case, and the Python wrapper."""
from types import SimpleNamespace as NS

import numpy as np
import pytest

import acf_common as K
import acf_fit_common as F
import acf_fit_twin as T


@pytest.mark.parametrize("grid", ["default", "small"])
@pytest.mark.parametrize("numOverLap", [100, 2, 64])
@pytest.mark.parametrize("ind_start", [1, 7])
def test_host_path_equals_twin(pkg, ind_start, numOverLap, grid):
    """3 channels of 99 / 100 / 101 rows; channel 1's and 2's hand-made rows hold NaN taps, so some
    windows are paths = 0 (with numOverLap = 100 every window of them)."""
    r = K.records("short", hand=numOverLap != 100)
    par = dict(ind_start=ind_start, numOverLap=numOverLap, **(F.SMALL if grid == "small" else {}))
    for orient in ((1, -1) if grid == "small" else (1,)):
        st, out = F.lib_run(pkg, r, orient=orient, **par)
        assert st == pkg.abi.OK
        chans = T.fit(r.taps, r.lens, orient, **par)
        F.assert_equals_twin(out, chans)
        st, feat = K.lib_run(pkg, r, ind_start=ind_start, numOverLap=numOverLap)  # gnss_acf_features' windows
        assert st == pkg.abi.OK and np.array_equal(out.windows, feat.windows)
        st, bare = F.lib_run(pkg, r, orient=orient, want=False, **par)  # zI / zQ NULL: the same rows
        assert st == pkg.abi.OK
        F.assert_same_outputs(out, bare)
    if numOverLap == 2:
        assert any(np.any(ch["paths"] == 0) for ch in chans) and any(np.any(ch["paths"] > 0) for ch in chans)


def test_window_count_quirk(pkg):
    for L, W in ((1000, 9), (1001, 10), (100, 0), (101, 1), (1, 0), (0, 0)):
        r = K.records("long", lens=[L, L, L], hand=False)
        st, out = F.lib_run(pkg, r, **F.SMALL)
        assert st == pkg.abi.OK and list(out.windows) == [W] * 3, (L, out.windows)


PHASES = [0.0, 0.5, 0.25, 0.1234]


@pytest.mark.parametrize("orient", [1, -1])
@pytest.mark.parametrize("phase", PHASES)
def test_exact_model_on_grid_points(pkg, phase, orient):
    """z built from the model on grid points (p 0.16, e 0.50, A1 = 0.5 A0 turned by `phase` cycles):
    exactly that ip and ie, the amplitudes within 1e-12 relative, res2 <= 1e-24 energy, paths = 2."""
    d = T.DEFAULTS
    ip, ie = 56, 45
    p, e = d["p_min"] + ip * d["p_step"], d["e_min"] + ie * d["e_step"]
    assert abs(p - 0.16) < 1e-12 and abs(e - 0.50) < 1e-12
    A0 = 3000.0 * np.exp(2j * np.pi * 0.07)
    A1 = 0.5 * A0 * np.exp(2j * np.pi * phase)
    zI, zQ = F.model(p, e, A0, A1, orient)
    st, got = F.fit_window(pkg, zI, zQ, orient)
    assert st == pkg.abi.OK
    assert got["p0"] == p and got["e"] == e, (got["p0"], got["e"])  # the grid values themselves: ip and ie
    for k, v in (("A0_re", A0.real), ("A0_im", A0.imag), ("A1_re", A1.real), ("A1_im", A1.imag)):
        assert abs(got[k] - v) <= 1e-12 * abs(A0), (k, got[k], v)
    assert got["res2"] <= 1e-24 * got["energy"], (got["res2"], got["energy"])
    assert got["paths"] == 2 and got["bias"] == p
    tw = T.fit_vector(zI, zQ, orient, **{k: d[k] for k in T.GRID})
    assert tw["paths"] == 2 and all(K.same_bits(got[f], tw[f]) for f in T.FIELDS)


def test_one_path_with_noise_selects_one_path(pkg):
    """A one-path vector plus 1 % seeded complex noise per tap: paths = 1, bias within a grid step."""
    rng = np.random.default_rng(11)
    for p in (0.0, 0.16, -0.23):
        A = 3000.0 * np.exp(2j * np.pi * 0.31)
        zI, zQ = F.model(p, 0.5, A, 0.0)
        zI = zI + rng.normal(0, 0.01 * abs(A), 25)
        zQ = zQ + rng.normal(0, 0.01 * abs(A), 25)
        st, got = F.fit_window(pkg, zI, zQ)
        assert st == pkg.abi.OK and got["paths"] == 1, got
        assert abs(got["bias"] - p) <= 0.01 + 1e-12 and got["bias"] == got["p1"], (p, got["bias"])
        print("p", p, "res1/res2", got["res1"] / got["res2"])


def test_ratio_max(pkg):
    """The stronger path second: never |A1| > |A0| at the default ratio_max = 1; with 10 it is."""
    A0 = 1000.0 + 0j
    for phase in PHASES:
        A1 = 2.0 * A0 * np.exp(2j * np.pi * phase)
        zI, zQ = F.model(0.16, 0.5, A0, A1)
        st, got = F.fit_window(pkg, zI, zQ)
        assert st == pkg.abi.OK
        if not np.isnan(got["res2"]):
            assert np.hypot(got["A1_re"], got["A1_im"]) <= np.hypot(got["A0_re"], got["A0_im"]), got
        st, got = F.fit_window(pkg, zI, zQ, ratio_max=10.0)
        assert st == pkg.abi.OK and got["paths"] == 2
        assert np.hypot(got["A1_re"], got["A1_im"]) > 1.9 * np.hypot(got["A0_re"], got["A0_im"]), got
        assert abs(got["p0"] - 0.16) < 1e-9 and abs(got["e"] - 0.5) < 1e-9


def test_sign_wipe(pkg):
    """Flipping the sign of all 50 sums of arbitrary rows leaves every output bit unchanged."""
    r = K.records("long", lens=[300, 301, 257], hand=False)
    st, a = F.lib_run(pkg, r, **F.SMALL)
    rng = np.random.default_rng(5)
    flip = rng.random((r.n, r.max_len)) < 0.5
    assert flip.any() and not flip.all()
    r.taps[:] = np.where(flip[:, None, None, :], -r.taps, r.taps)
    st2, b = F.lib_run(pkg, r, **F.SMALL)
    assert st == st2 == pkg.abi.OK and a.windows[1] == 3
    F.assert_same_outputs(a, b)


def test_ties_and_degenerate_inputs(pkg):
    d = T.DEFAULTS
    z0 = np.zeros(25)
    st, got = F.fit_window(pkg, z0, z0)  # all zero: every residual 0, the first hypothesis of each grid
    assert st == pkg.abi.OK and got["paths"] == 1 and got["p1"] == d["p_min"] and got["bias"] == d["p_min"]
    assert got["res1"] == 0.0 and got["res2"] == 0.0 and got["p0"] == d["p_min"] and got["e"] == d["e_min"]
    assert got["energy"] == 0.0
    # a grid whose every two-path hypothesis is skipped (the second path beyond the taps): one path
    zI, zQ = F.model(0.0, 0.5, 1000.0, 0.0)
    st, got = F.fit_window(pkg, zI, zQ, e_min=3.0, e_count=4)
    assert st == pkg.abi.OK and got["paths"] == 1 and got["p1"] == 0.0 and np.isnan(got["res2"]) and np.isnan(got["e"])
    assert got["res1"] <= 1e-24 * got["energy"]
    # a NaN tap: no fit, NaN outputs, for that window only
    r = K.records("long", lens=[301, 301, 301], hand=False)
    r.taps[1, 1, 3, 150] = np.nan
    st, out = F.lib_run(pkg, r, **F.SMALL)
    assert st == pkg.abi.OK and list(out.windows) == [3, 3, 3]
    assert out.paths[1, 1] == 0 and all(np.isnan(out.arr[f][1, 1]) for f in T.FIELDS)
    assert np.isnan(out.zQ[1, 3, 1]) and np.sum(np.isnan(out.zQ)) == 1
    rest = np.ones((3, 3), dtype=bool)
    rest[1, 1] = False
    assert np.all(out.paths[rest] > 0) and all(np.all(np.isfinite(out.arr[f][rest])) for f in ("bias", "res1", "energy"))
    inf = z0.copy()
    inf[7] = np.inf
    st, got = F.fit_window(pkg, inf, z0)
    assert st == pkg.abi.OK and got["paths"] == 0 and np.isnan(got["energy"])


def test_every_earg_case(pkg):
    abi = pkg.abi
    r = K.records("long")
    ok = lambda **kw: F.lib_run(pkg, r, **dict(F.SMALL, **kw))[0]
    nan = float("nan")
    bad = [dict(n_taps=24), dict(n_taps=26), dict(n_taps=0), dict(numOverLap=1), dict(numOverLap=4097, cap=4),
           dict(numOverLap=0, cap=4), dict(ind_start=0), dict(ind_start=-3), dict(orient=0), dict(orient=2),
           dict(corrSpacing=0.0), dict(corrSpacing=-0.05), dict(corrSpacing=nan), dict(p_step=0.0), dict(p_step=nan),
           dict(e_step=-0.01), dict(e_step=nan), dict(p_min=nan), dict(e_min=float("inf")), dict(p_count=0),
           dict(e_count=0), dict(p_count=-1), dict(p_count=257, e_count=256), dict(p_count=65536, e_count=65536),
           dict(ratio_max=-1.0), dict(ratio_max=nan), dict(gain_min=nan), dict(cap=9), dict(n=0),
           dict(n=abi.VT_MAX_CH + 1)]
    assert ok() == abi.OK
    for kw in bad:
        assert ok(**kw) == abi.EARG, kw
        assert ok() == abi.OK  # the next call still works
    assert ok(numOverLap=4096) == abi.OK and ok(cap=10) == abi.OK and ok(orient=-1) == abi.OK
    assert ok(p_count=256, e_count=256, numOverLap=1000) == abi.OK  # 65 536 hypotheses: the cap itself
    long = K.records("long")
    long.lens[2] = long.max_len + 1
    assert F.lib_run(pkg, long, cap=16, **F.SMALL)[0] == abi.EARG
    long.lens[2] = -1
    assert F.lib_run(pkg, long, cap=16, **F.SMALL)[0] == abi.EARG
    lib = abi.load()
    assert lib.gnss_acf_fit(None, None, None, 25, None) == abi.EARG
    assert lib.gnss_acf_fit_window(None, None, None, None) == abi.EARG
    z = np.zeros(25)
    assert F.fit_window(pkg, z, z, orient=0)[0] == abi.EARG and F.fit_window(pkg, z, z, p_count=0)[0] == abi.EARG
    assert F.fit_window(pkg, z, z)[0] == abi.OK


def test_python_wrapper(pkg):
    """sdr.acf_fit from the per-PRN structs of the scalar loops (taps_i / taps_q) and of the vector
    loop (tap_i / tap_q), a StructArray and raw buffers; the derived ratio, dphi_cycles and bias_m;
    the orientation tag."""
    r = K.records("long", hand=False)
    prn = [22, 3, 14]
    ct = {p: NS(taps_i=r.taps[c, 0, :, : r.lens[c]], taps_q=r.taps[c, 1, :, : r.lens[c]],
                DLLdiscri=r.rec[c, 7, : r.lens[c]]) for c, p in enumerate(prn)}
    vt = {p: NS(tap_i=r.taps[c, 0, :, : r.lens[c]].T, tap_q=r.taps[c, 1, :, : r.lens[c]].T,
                codeError=r.rec[c, 7, : r.lens[c]]) for c, p in enumerate(prn)}
    track = pkg.initParameters()[3]
    buf = pkg.TrackOutBuffers(3, track, 25, ctPOS=r.max_len)
    buf.rec[:], buf.taps[:], buf.len[:] = r.rec, r.taps, r.lens
    chans = T.fit(r.taps, r.lens, -1, **F.SMALL)
    for src in (ct, vt, pkg.StructArray(ct), buf):
        f = pkg.acf_fit(src, prn, orient=-1, want_acf=True, **F.SMALL)
        assert list(f.windows) == [9, 10, 2] and f.orient == -1
        for c, ch in enumerate(chans):
            assert np.array_equal(f.paths[c], ch["paths"])
            for k in T.FIELDS + ["zI", "zQ"]:
                assert K.same_bits(getattr(f, k)[c], ch[k]), (c, k)
            a0, a1 = ch["A0_re"] + 1j * ch["A0_im"], ch["A1_re"] + 1j * ch["A1_im"]
            assert np.allclose(f.ratio[c], np.abs(a1) / np.abs(a0), rtol=1e-14, equal_nan=True)
            turn = f.dphi_cycles[c] - np.angle(a1 / a0) / (2 * np.pi)
            assert np.all(np.abs((turn + 0.5) % 1.0 - 0.5) <= 1e-12)  # (equal up to a whole cycle at +-0.5)
            assert np.allclose(f.bias_m[c], ch["bias"] * 299792458.0 / 1.023e6, rtol=1e-15)
    with pytest.raises(ValueError):
        pkg.acf_fit(ct, prn)  # untagged records and no orient
    tagged = pkg.StructArray(ct)
    tagged.acf_orient = -1
    assert K.same_bits(pkg.acf_fit(tagged, prn, **F.SMALL).bias[1], chans[1]["bias"])
    assert pkg.abi.ACF_ORIENT == dict(trackingCT_multiCorr=1, trackingCT_POS_updated_multicorrelator=-1,
                                      trackingVT_POS_updated_multicorrelator=-1)
    with pytest.raises(TypeError):
        pkg.acf_fit(ct, prn, orient=1, numOverlap=64)
    with pytest.raises(pkg.abi.GnssError) as e:
        pkg.acf_fit(ct, prn, orient=3)
    assert e.value.status == pkg.abi.EARG
