"""GPU tests of CalculateFeatures.m's F6-F8 on device-resident 25-tap records
(gnss_acf_features_ext with GNSS_OUT_DEVICE; the counting form of csrc/acf.hip's row pass and
csrc/acf_ext.hip): the device path equals the host path in every output bit -- the three new
features, the six of gnss_acf_features, maxCorrInd and corr -- on every shape of
test_acf_ext_kat.py, on bin counts that are no multiple of the block (513, 501 and 2), a long
channel beside a short one, the widest window, both row-pass forms (odd and even max_len), corr
wanted and not; two runs give the same bits; the refusals leave the context usable; end to end on
DESIGN §3.3's scene with a ray fading at 3 Hz through trackingCT_multiCorr."""
import importlib.util
import os

import numpy as np
import pytest

import acf_common as K
import acf_ext_common as E
from conftest import ROOT, acquired_of, params
from test_acf_ext_kat import CASES, records
from test_gpu_acf import Dev

pytestmark = pytest.mark.gpu


def device_equals_host(pkg, ctx, r, **par):
    st, host, hext = E.ext_run(pkg, r, want=True, **par)
    assert st == pkg.abi.OK
    d = Dev(ctx, r)
    try:
        st, dev, dext = E.ext_run(pkg, r, ctx=ctx, dev=(d.rec, d.taps), dev_ind=d.ind, dev_corr=d.corr, **par)
        assert st == pkg.abi.OK, ctx.lib.gnss_last_error(ctx.h)
        K.assert_same_outputs(host, dev)
        E.assert_same_ext(host, hext, dext)
        ind, corr = d.outputs()
        assert np.array_equal(ind, host.ind)
        assert K.same_bits(corr, host.corr)
        st, bare, bext = E.ext_run(pkg, r, ctx=ctx, dev=(d.rec, d.taps), **par)  # maxCorrInd and corr not wanted
        assert st == pkg.abi.OK
        K.assert_same_outputs(host, bare)
        E.assert_same_ext(host, hext, bext)
    finally:
        d.free()
    return host, hext


@pytest.mark.parametrize("shape,par", CASES, ids=[f"{s}-{i}" for i, (s, _) in enumerate(CASES)])
def test_device_path_equals_host(pkg, ctx, shape, par):
    """The CPU shapes (odd max_len: one row per lane; k1004: even, two rows per lane)"""
    device_equals_host(pkg, ctx, records(shape), **par)


@pytest.mark.parametrize("fft_hist,fft_n,bins", [(300, 1024, 513), (300, 1000, 501), (2, 2, 2)])
@pytest.mark.parametrize("max_len", [514, 515])
def test_bin_counts_off_the_block(pkg, ctx, max_len, fft_hist, fft_n, bins):
    """513 bins (two turns of the lanes and one bin), 501 and 2; lens 513 / 512 / 511 in a series
    of 514 (two rows per lane, windows ending at the last row and before it) and of 515 (one row)."""
    assert fft_n // 2 + 1 == bins
    r = K.records("long", lens=[513, 512, 511], max_len=max_len)
    for par in (dict(numOverLap=64), dict(numOverLap=2, ind_start=2, fft_fill=1)):
        host, _ = device_equals_host(pkg, ctx, r, fft_hist=fft_hist, fft_n=fft_n, **par)
        assert list(host.windows) == ([8, 7, 7] if "ind_start" not in par else [255, 255, 254])


def test_long_channel_beside_a_short_one(pkg, ctx):
    """20 001 rows beside 101: 200 windows against 1, on both row forms"""
    for max_len in (20002, 20003):
        r = K.records("long", lens=[20001, 101], max_len=max_len)
        host, hext = device_equals_host(pkg, ctx, r, fft_hist=50, fft_n=128)
        assert list(host.windows) == [200, 1]
    E.assert_ext_equals_twin(host, hext, E.twin(pkg, r, fft_hist=50, fft_n=128))


def test_widest_window(pkg, ctx):
    """numOverLap = 4096 on 8 200 rows: 16 turns of the lanes over a window's count bytes"""
    r = K.records("long", lens=[8200], max_len=8201, hand=False)
    host, hext = device_equals_host(pkg, ctx, r, numOverLap=4096, fft_hist=2, fft_n=64, fs=1.0)
    assert list(host.windows) == [2]
    E.assert_ext_equals_twin(host, hext, E.twin(pkg, r, numOverLap=4096, fft_hist=2, fft_n=64, fs=1.0))


def test_two_runs_are_bit_identical(pkg, ctx):
    r = K.records("long", max_len=1004)
    d = Dev(ctx, r, want=False)
    try:
        st1, a, ax = E.ext_run(pkg, r, ctx=ctx, dev=(d.rec, d.taps), fft_hist=8)
        st2, b, bx = E.ext_run(pkg, r, ctx=ctx, dev=(d.rec, d.taps), fft_hist=8)
        assert st1 == st2 == pkg.abi.OK and list(a.windows) == [9, 10, 2]
        K.assert_same_outputs(a, b)
        E.assert_same_ext(a, ax, bx)
    finally:
        d.free()


def test_refusals_leave_the_context_usable(pkg, ctx):
    abi = pkg.abi
    r = K.records("long", max_len=1004)
    _, host, hext = E.ext_run(pkg, r, fft_hist=8)
    d = Dev(ctx, r, want=False)
    try:
        run = lambda c=ctx, **kw: E.ext_run(pkg, r, ctx=c, dev=(d.rec, d.taps), **dict(dict(fft_hist=8), **kw))

        def fine():
            st, out, ext = run()
            assert st == abi.OK
            K.assert_same_outputs(host, out)
            E.assert_same_ext(host, hext, ext)

        fine()
        for bad in (dict(fft_hist=1), dict(fft_hist=513, fft_n=2048), dict(fft_n=7), dict(fft_n=2049),
                    dict(fft_fill=2), dict(fs=0.0), dict(fs=float("nan")), dict(fs=float("inf")), dict(null="fftMag"),
                    dict(n_taps=24), dict(numOverLap=1), dict(numOverLap=4097, cap=4), dict(ind_start=0),
                    dict(corrSpacing=0.0), dict(cap=9), dict(n=0), dict(n=abi.VT_MAX_CH + 1)):
            assert run(**bad)[0] == abi.EARG, bad
            assert ctx.lib.gnss_last_error(ctx.h)
            fine()
        keep = r.lens[2]
        r.lens[2] = r.max_len + 1  # the kernels would index past the series: refused before any launch
        assert run(cap=16)[0] == abi.EARG
        r.lens[2] = keep
        fine()
        assert E.ext_run(pkg, r, dev=(d.rec, d.taps))[0] == abi.EARG  # device records without a context
        m = pkg.Context(devices=[0, 0])  # no gathering across members
        try:
            assert run(m)[0] == abi.EARG
        finally:
            m.close()
        fine()
    finally:
        d.free()


def test_python_mirror_on_resident_records(pkg, ctx, opensky_short):
    """gnss_tracking_ct_mc with GNSS_OUT_DEVICE, then sdr.acf_features(extended=True) on the buffers
    as they lie in HBM: equal to the same call on the downloaded records in all nine lists, and the
    11-column data_labeled's first eight columns equal to the 8-column one."""
    from test_gpu_pos import OPENSKY
    skip, cfg, data = opensky_short
    file, signal, acq, track = params(pkg, skip, data)
    track.msPosCT, track.pdi = 400, 1
    A = acquired_of(OPENSKY["svs"], OPENSKY["cd"], OPENSKY["ff"])
    buf = pkg.trackingCT_POS_updated_multicorrelator(file, signal, track, A, ctx=ctx, raw=True, device_records=True)
    assert buf.c.flags == pkg.abi.OUT_DEVICE and list(buf.len) == [400] * 8
    ele = [8.36, 54.23, 24.23, 47.1, 6.39, 31.54, 45.0, 64.42]
    par = dict(numOverLap=40, fft_hist=5, fft_n=64, fft_fill=1)
    f = pkg.acf_features(buf, OPENSKY["svs"], ele, ctx=ctx, extended=True, **par)
    h = pkg.acf_features(buf.host(), OPENSKY["svs"], ele, extended=True, **par)
    assert list(f.windows) == [9] * 8
    for k in list(pkg.abi.ACF_FIELDS) + list(pkg.abi.ACF_EXT_FIELDS):
        for c in range(8):
            assert K.same_bits(getattr(f, k)[c], getattr(h, k)[c]), (k, c)
    for c in range(8):  # (H = 1 in a channel's first window: y = 0)
        assert np.all(f.numMLC[c] > 0) and f.fftMag[c][0] == 0.0 and np.all(f.fftMag[c][1:] > 0)
    wide = pkg.CalculateFeatures(buf, OPENSKY["svs"], ele, ctx=ctx, extended=True, **par)
    old = pkg.CalculateFeatures(buf, OPENSKY["svs"], ele, ctx=ctx, numOverLap=40)
    assert wide.shape == (73, 11) and old.shape == (73, 8) and not np.any(wide[0])
    assert K.same_bits(wide[:, :8], old)
    assert K.same_bits(wide[1:, 10], np.concatenate(f.fftMag))


# ---- end to end --------------------------------------------------------------------------------
FADE = 3.0
PAR = dict(numOverLap=40, fft_hist=25, fft_fill=1)  # fs = 25 Hz, a full history from window 24 on
# DESIGN §3.8.1, from the CPU chain (tools/acf_spectrum_accuracy.py), over the full-history windows:
# the smallest fftMag with the ray and the largest without it; the threshold is their geometric
# middle
MAG_RAY_MIN, MAG_NONE_MAX = 414.647, 15.600  # a factor of 26.6
MAG_THRESHOLD = float(np.sqrt(MAG_RAY_MIN * MAG_NONE_MAX))  # 80.43


def accuracy_tool():
    spec = importlib.util.spec_from_file_location("acf_spectrum_accuracy",
                                                  os.path.join(ROOT, "tools", "acf_spectrum_accuracy.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def given(pkg, ctx):
    """§3.3's scene -- PRN 3 at 55 dB-Hz -- without a ray and with one 0.5 chip late at half the
    amplitude fading at 3 Hz, each through generate_scene_device and gnss_tracking_ct_multicorr
    (1640 rows, 40 windows) and the extended features on its records."""
    out = {}
    for name, fade in (("none", None), ("ray", FADE)):
        sc = pkg.synth.scene_of(pkg.synth.scenario([3], [3683], [990.0], [55.0], skip_ms=2))
        if fade is not None:
            pkg.synth.add_ray(sc, 3, 0.5, 0.5, fade_hz=fade)
        dev = pkg.DeviceRecord(ctx, 2 * (2 + 1 + 1640 + 4) * 58000)
        try:
            pkg.synth.generate_scene_device(ctx, sc, dev)
            file, signal, acq, track = params(pkg, 2, None)
            file.dev = dev
            tck, _ = pkg.trackingCT_multiCorr(file, signal, track, acquired_of([3], [3683], [4580990.0]),
                                              datalength=1640, ctx=ctx)
        finally:
            dev.free()
        out[name] = pkg.acf_features(tck, [3], [45.0], extended=True, **PAR)
        assert out[name].windows[0] == 40
    s = accuracy_tool().summary(out["ray"], out["none"], FADE, PAR)
    print("fftFreq with the ray", np.round(out["ray"].fftFreq[0][24:], 4))
    print("fftMag with the ray", np.round(out["ray"].fftMag[0][24:], 3))
    print("fftMag without", np.round(out["none"].fftMag[0][24:], 3))
    print({k: round(v, 4) for k, v in s.items()})
    return out


def test_fade_frequency(given):
    """In the full-history windows |fftFreq - 3| <= fs / (2 fft_hist) = 0.5 Hz, half the width of a
    25-sample main lobe."""
    f = given["ray"].fftFreq[0][24:]
    assert len(f) == 16 and np.all(np.abs(f - FADE) <= 25.0 / (2 * 25))


def test_fade_magnitude_tells_the_ray(given):
    """Every full-history fftMag with the ray lies above the threshold, every one without below"""
    assert np.all(given["ray"].fftMag[0][24:] > MAG_THRESHOLD)
    assert np.all(given["none"].fftMag[0][24:] < MAG_THRESHOLD)
