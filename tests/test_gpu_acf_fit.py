"""GPU tests of the two-path fit of the 25-tap ACF on device-resident records (gnss_acf_fit with
GNSS_OUT_DEVICE, csrc/acf_fit.hip): the kernel's outputs equal the host path's bit for bit -- every
field, zI and zQ -- over the window rule's lengths, both start rows, the window widths, grids of 1,
6, 255, 257 and 7 776 hypotheses, a long channel beside a short one and numOverLap = 4096; two
runs give the same bits; end to end on DESIGN §3.3's scene through the GIVEN loop (host records)
and through the 10-ms multicorrelator loop (resident records), which pin the two orientations;
the refusals, each leaving the context usable."""
import numpy as np
import pytest

import acf_common as K
import acf_fit_common as F
import acf_fit_twin as T
from conftest import acquired_of, params
from test_gpu_acf import Dev

pytestmark = pytest.mark.gpu

# hypothesis counts 1, 6, 255 (one short of a block's lanes), 257 (one lane's second turn) and the
# default 81 x 96 = 7 776 (30 turns and a remainder of 96)
GRIDS = {
    "1": dict(p_min=0.0, p_step=0.1, p_count=1, e_min=0.5, e_step=0.1, e_count=1),
    "6": F.SMALL,
    "255": dict(p_min=-0.35, p_step=0.05, p_count=15, e_min=0.1, e_step=0.05, e_count=17),
    "257": dict(p_min=0.05, p_step=0.1, p_count=1, e_min=0.05, e_step=0.003, e_count=257),
    "7776": {},
}


def device_equals_host(pkg, ctx, r, orient=1, **par):
    st, host = F.lib_run(pkg, r, orient=orient, **par)
    assert st == pkg.abi.OK
    d = Dev(ctx, r, want=False)
    try:
        st, dev = F.lib_run(pkg, r, ctx=ctx, dev=(d.rec, d.taps), orient=orient, **par)
        assert st == pkg.abi.OK, ctx.lib.gnss_last_error(ctx.h)
        F.assert_same_outputs(host, dev)
        st, bare = F.lib_run(pkg, r, ctx=ctx, dev=(d.rec, d.taps), orient=orient, want=False, **par)  # zI / zQ NULL
        assert st == pkg.abi.OK
        F.assert_same_outputs(host, bare)
    finally:
        d.free()
    return host


@pytest.mark.parametrize("grid", ["6", "7776"])
@pytest.mark.parametrize("numOverLap", [100, 2, 64])
@pytest.mark.parametrize("ind_start", [1, 7])
def test_device_path_equals_host(pkg, ctx, ind_start, numOverLap, grid):
    """99 / 100 / 101 rows (one window or none at numOverLap = 100 and 64); with numOverLap = 2 some
    windows hold the hand-made NaN rows (paths = 0)."""
    r = K.records("short", hand=numOverLap == 2)
    host = device_equals_host(pkg, ctx, r, orient=-1 if grid == "6" else 1, ind_start=ind_start,
                              numOverLap=numOverLap, **GRIDS[grid])
    assert list(host.windows) == [(L - ind_start) // numOverLap for L in (99, 100, 101)]
    if numOverLap == 2:
        assert np.any(host.paths == 0) and np.any(host.paths > 0)


@pytest.mark.parametrize("grid", list(GRIDS))
def test_every_hypothesis_count(pkg, ctx, grid):
    """lens 513 / 512 / 511 in a series of 514 (windows that end at the last row, one row before it
    and two before it), at every grid; the twin agrees with both on the small grids."""
    r = K.records("long", lens=[513, 512, 511], max_len=514, hand=False)
    par = dict(GRIDS[grid], numOverLap=64 if grid == "7776" else 2, ind_start=1 if grid == "7776" else 2)
    host = device_equals_host(pkg, ctx, r, **par)
    assert list(host.windows) == ([8, 7, 7] if grid == "7776" else [255, 255, 254])
    if grid in ("1", "6"):
        F.assert_equals_twin(host, T.fit(r.taps, r.lens, 1, **par))


def test_long_channel_beside_a_short_one(pkg, ctx):
    r = K.records("long", lens=[20001, 101], max_len=20003, hand=False)
    host = device_equals_host(pkg, ctx, r)
    assert list(host.windows) == [200, 1]
    host = device_equals_host(pkg, ctx, r, ind_start=7, **GRIDS["255"])
    assert list(host.windows) == [199, 0]


def test_widest_window(pkg, ctx):
    """numOverLap = 4096 on one channel of 8 200 rows: 65 tiles of rows per window, two windows."""
    r = K.records("long", lens=[8200], max_len=8201, hand=False)
    host = device_equals_host(pkg, ctx, r, numOverLap=4096, **GRIDS["255"])
    assert list(host.windows) == [2] and np.all(host.paths[0, :2] > 0)
    F.assert_equals_twin(host, T.fit(r.taps, r.lens, 1, numOverLap=4096, **GRIDS["255"]))


def test_two_runs_are_bit_identical(pkg, ctx):
    r = K.records("long", hand=False)
    d = Dev(ctx, r, want=False)
    try:
        st1, a = F.lib_run(pkg, r, ctx=ctx, dev=(d.rec, d.taps))
        st2, b = F.lib_run(pkg, r, ctx=ctx, dev=(d.rec, d.taps))
        assert st1 == st2 == pkg.abi.OK and list(a.windows) == [9, 10, 2]
        F.assert_same_outputs(a, b)
    finally:
        d.free()


# ---- end to end --------------------------------------------------------------------------------
def scene(pkg, phase):
    """DESIGN §3.3's scene: PRN 3 alone at 55 dB-Hz, a ray half a chip late at half the amplitude"""
    sc = pkg.synth.scene_of(pkg.synth.scenario([3], [3683], [990.0], [55.0], skip_ms=2))
    if phase is not None:
        pkg.synth.add_ray(sc, 3, 0.5, 0.5, phase_cycles=phase)
    return sc


@pytest.fixture(scope="module")
def given(pkg, ctx):
    """The scene without a ray, with the ray in phase and with it opposed, each through
    gnss_tracking_ct_multicorr (600 rows, five windows) and the fit on its records."""
    out = {}
    for name, phase in (("none", None), ("in_phase", 0.0), ("opposed", 0.5)):
        dev = pkg.DeviceRecord(ctx, 2 * (2 + 1 + 600 + 4) * 58000)
        try:
            pkg.synth.generate_scene_device(ctx, scene(pkg, phase), dev)
            file, signal, acq, track = params(pkg, 2, None)
            file.dev = dev
            tck, _ = pkg.trackingCT_multiCorr(file, signal, track, acquired_of([3], [3683], [4580990.0]),
                                              datalength=600, ctx=ctx)
        finally:
            dev.free()
        assert tck.acf_orient == 1
        out[name] = pkg.acf_fit(tck, [3])
    return out


def after_pull_in(f):
    assert f.windows[0] == 5
    keys = ("paths", "bias", "e", "ratio", "dphi_cycles", "res1", "res2")
    w = {k: np.asarray(getattr(f, k)[0][1:]) for k in keys}
    print({k: np.round(v, 4) for k, v in w.items()}, "res1/res2", np.round(w["res1"] / w["res2"], 2))
    return w


def test_given_loop_in_phase_ray(given):
    """The windows after pull-in (the ones DESIGN §3.3 reads F2 from): the ray's excess delay to one
    tap spacing, its relative amplitude, and the DLL's bias of 1/6 chip."""
    w = after_pull_in(given["in_phase"])
    assert np.all(w["paths"] == 2)
    assert np.all(np.abs(w["e"] - 0.5) <= 0.05)
    assert np.all(np.abs(w["ratio"] - 0.5) <= 0.1)
    assert np.all(np.abs(w["bias"] - 1.0 / 6.0) <= 0.03)


def test_given_loop_opposed_ray(given):
    w = after_pull_in(given["opposed"])
    assert np.all(w["paths"] == 2)
    assert np.all(np.abs(w["bias"] + 0.2) <= 0.03)
    assert np.all(np.abs(np.abs(w["dphi_cycles"]) - 0.5) <= 0.05)


def test_given_loop_without_a_ray(given):
    w = after_pull_in(given["none"])
    assert np.all(w["paths"] == 1)
    assert np.all(np.abs(w["bias"]) <= 0.02)


def test_ten_ms_loop_on_resident_records(pkg, ctx):
    """The in-phase scene through gnss_tracking_ct_mc at pdi = 10 into DeviceTrackOutBuffers, the fit
    on the records as they lie in HBM with that loop's orientation (-1: Spacing = 0.6:-0.05:-0.6):
    e within 0.05 of 0.5 in the window after pull-in; the resident fit equals the host fit on the
    downloaded records bit for bit. With the other orientation the ray would sit on the early side,
    where no e > 0 reaches it."""
    ms = 1210
    dev = pkg.DeviceRecord(ctx, 2 * (2 + 1 + ms + 14) * 58000)
    try:
        pkg.synth.generate_scene_device(ctx, scene(pkg, 0.0), dev)
        file, signal, acq, track = params(pkg, 2, None)
        file.dev = dev
        track.msPosCT, track.pdi = ms, 10
        buf = pkg.trackingCT_POS_updated_multicorrelator(file, signal, track, acquired_of([3], [3683], [4580990.0]),
                                                         ctx=ctx, raw=True, device_records=True)
    finally:
        dev.free()
    assert buf.c.flags == pkg.abi.OUT_DEVICE and list(buf.len) == [121] and buf.acf_orient == -1
    f = pkg.acf_fit(buf, [3], ctx=ctx, numOverLap=40, want_acf=True)
    h = pkg.acf_fit(buf.host(), [3], numOverLap=40, want_acf=True)
    assert f.windows[0] == 3 and f.orient == -1
    for k in T.FIELDS + ["zI", "zQ"]:
        assert K.same_bits(getattr(f, k)[0], getattr(h, k)[0]), k
    print("paths", f.paths[0], "bias", f.bias[0], "e", f.e[0], "ratio", f.ratio[0], "res1/res2", f.res1[0] / f.res2[0])
    assert np.all(f.paths[0][1:] == 2)
    assert np.all(np.abs(f.e[0][1:] - 0.5) <= 0.05)
    wrong = pkg.acf_fit(buf, [3], ctx=ctx, numOverLap=40, orient=1)
    assert not np.any((wrong.paths[0][1:] == 2) & (np.abs(wrong.e[0][1:] - 0.5) <= 0.05))


def test_refusals_leave_the_context_usable(pkg, ctx):
    abi = pkg.abi
    r = K.records("long", max_len=1004)
    _, host = F.lib_run(pkg, r, **F.SMALL)
    d = Dev(ctx, r, want=False)
    try:
        run = lambda c=ctx, **kw: F.lib_run(pkg, r, ctx=c, dev=(d.rec, d.taps), **dict(F.SMALL, **kw))

        def fine():
            st, out = run()
            assert st == abi.OK
            F.assert_same_outputs(host, out)

        fine()
        for bad in (dict(n_taps=24), dict(numOverLap=1), dict(numOverLap=4097, cap=4), dict(ind_start=0),
                    dict(orient=0), dict(corrSpacing=0.0), dict(p_step=0.0), dict(e_step=float("nan")),
                    dict(p_count=0), dict(p_count=257, e_count=256), dict(ratio_max=-1.0), dict(cap=9), dict(n=0),
                    dict(n=abi.VT_MAX_CH + 1)):
            assert run(**bad)[0] == abi.EARG, bad
            assert ctx.lib.gnss_last_error(ctx.h)
            fine()
        keep = r.lens[2]
        r.lens[2] = r.max_len + 1  # the kernel would index past the series: refused before any launch
        assert run(cap=16)[0] == abi.EARG
        r.lens[2] = keep
        fine()
        assert F.lib_run(pkg, r, dev=(d.rec, d.taps), **F.SMALL)[0] == abi.EARG  # device records without a context
        m = pkg.Context(devices=[0, 0])  # no gathering across members
        try:
            assert run(m)[0] == abi.EARG
        finally:
            m.close()
        fine()
    finally:
        d.free()
