"""GPU tests of the two-path fit on any tap grid over device-resident sums (gnss_acf_fit_taps with
GNSS_OUT_DEVICE, csrc/acf_fit_taps.hip): the kernel's outputs equal the host path's bit for bit --
every field, zI and zQ -- over tap counts of one series group, a group boundary and one either
side of it, and the maximum; grids of 1, 6, 255, 257 and 15 876 hypotheses; window widths around
the row tile of 64, 2 and 4096; both start rows; lens 513 / 512 / 511 in a series of 514; a long
channel beside a short one. Two runs give the same bits; at 25 taps the
kernel equals gnss_acf_fit's kernel on the same uploaded sums; the chain replay -> fit stays
resident with the host chain's bits; end to end a ray 1.7 chips late, outside every 25-tap record,
is estimated on -2.5:0.05:1.0; the refusals, each leaving the context usable."""
import ctypes as C

import numpy as np
import pytest

import acf_common as K
import acf_fit_common as F25
import acf_fit_taps_common as F
import acf_fit_taps_twin as T
from conftest import acquired_of, params
from test_gpu_acf import Dev

pytestmark = pytest.mark.gpu

# hypothesis counts 1, 6, 255 (one short of a block's lanes), 257 (one lane's second turn) and the
# default 81 x 196 = 15 876
GRIDS = {
    "1": dict(p_min=0.0, p_step=0.1, p_count=1, e_min=0.5, e_step=0.1, e_count=1),
    "6": F.SMALL,
    "255": dict(p_min=-0.35, p_step=0.05, p_count=15, e_min=0.1, e_step=0.05, e_count=17),
    "257": dict(p_min=0.05, p_step=0.1, p_count=1, e_min=0.05, e_step=0.003, e_count=257),
    "15876": {},
}


class Up:
    """A device copy of an array (gnss_dev_alloc / gnss_dev_upload)."""

    def __init__(self, ctx, a):
        self.ctx, self.p = ctx, C.c_void_p()
        ctx.check(ctx.lib.gnss_dev_alloc(ctx.h, C.c_uint64(a.nbytes), C.byref(self.p)))
        ctx.check(ctx.lib.gnss_dev_upload(ctx.h, self.p, a.ctypes.data_as(C.c_void_p), C.c_uint64(a.nbytes)))
        self.ptr = self.p.value

    def free(self):
        self.ctx.lib.gnss_dev_free(self.ctx.h, self.p)


def device_equals_host(pkg, ctx, s, **par):
    st, host = F.lib_run(pkg, s, **par)
    assert st == pkg.abi.OK
    d = Up(ctx, s.taps)
    try:
        st, dev = F.lib_run(pkg, s, ctx=ctx, dev=d.ptr, **par)
        assert st == pkg.abi.OK, ctx.lib.gnss_last_error(ctx.h)
        F.assert_same_outputs(host, dev)
        st, bare = F.lib_run(pkg, s, ctx=ctx, dev=d.ptr, want=False, **par)  # zI / zQ NULL
        assert st == pkg.abi.OK
        F.assert_same_outputs(host, bare)
    finally:
        d.free()
    return host


EDGE = ([513, 512, 511], 514)  # test_gpu_acf_fit.py's lens: the last windows end close to the series' end
# name: (n_taps, prompt, (n_rows, max_rows), numOverLap, ind_start, grid, windows, twin too)
CASES = {
    "1tap": (1, 0, EDGE, 2, 1, "1", [256, 255, 255], True),
    "25taps": (25, 12, EDGE, 63, 7, "6", [8, 8, 8], True),
    "33taps-long-short": (33, 32, ([20001, 101], 20003), 100, 1, "257", [200, 1], False),
    "64taps": (64, 0, ([300, 131], 301), 64, 1, "255", [4, 2], False),
    "65taps": (65, 40, ([300, 131], 301), 65, 7, "15876", [4, 1], False),
    "61taps": (61, 30, EDGE, 100, 1, "15876", [5, 5, 5], False),
    "256taps-widest-window": (256, 200, ([8200], 8201), 4096, 1, "255", [2], True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_device_path_equals_host(pkg, ctx, name):
    n_taps, prompt, (n_rows, max_rows), numOverLap, ind_start, grid, windows, twin = CASES[name]
    s = F.sums(n_taps, prompt, n_rows, max_rows, u=F.grid_u(n_taps, prompt, 0.0125 if n_taps == 256 else 0.05))
    par = dict(GRIDS[grid], numOverLap=numOverLap, ind_start=ind_start)
    host = device_equals_host(pkg, ctx, s, **par)
    assert list(host.windows) == windows
    if n_taps > 1:
        assert np.all(host.paths[0, : windows[0]] > 0)
    if twin:
        F.assert_equals_twin(host, T.fit(s.taps, s.n_rows, s.u, s.prompt, **par))


def test_non_finite_sums_and_an_unsorted_grid(pkg, ctx):
    rng = np.random.default_rng(8)
    u = np.concatenate([[0.0], rng.uniform(-1.6, 0.8, 32)])[rng.permutation(33)]
    s = F.sums(33, int(np.flatnonzero(u == 0)[0]), [400, 0, 131], 401, u=u)
    s.taps[0, 1, 32, 70] = np.nan
    s.taps[0, 0, s.prompt, 140] = np.nan
    s.taps[2, 0, 0, 3] = np.inf
    host = device_equals_host(pkg, ctx, s, numOverLap=65, **GRIDS["255"])
    assert list(host.windows) == [6, 0, 2]
    assert list(host.paths[0, :6] == 0) == [False, True, True, False, False, False]
    assert list(host.paths[2, :2] == 0) == [True, False]
    F.assert_equals_twin(host, T.fit(s.taps, s.n_rows, s.u, s.prompt, numOverLap=65, **GRIDS["255"]))


def test_two_runs_are_bit_identical(pkg, ctx):
    s = F.sums(61, 30, [1000, 1001, 257], 1003)
    d = Up(ctx, s.taps)
    try:
        st1, a = F.lib_run(pkg, s, ctx=ctx, dev=d.ptr)
        st2, b = F.lib_run(pkg, s, ctx=ctx, dev=d.ptr)
        assert st1 == st2 == pkg.abi.OK and list(a.windows) == [9, 10, 2]
        F.assert_same_outputs(a, b)
    finally:
        d.free()


@pytest.mark.parametrize("orient", [1, -1])
def test_at_25_taps_equals_gnss_acf_fit_on_the_device(pkg, ctx, orient):
    """acf_common's records uploaded once, through both kernels at gnss_acf_fit's default grid."""
    r = K.records("long", hand=True)
    u = (orient * (np.arange(25) - 12.0)) * 0.05
    s = F.NS(taps=r.taps, n_rows=r.lens, max_rows=r.max_len, n=r.n, n_taps=25, prompt=12, u=u)
    d = Dev(ctx, r, want=False)
    try:
        st, ref = F25.lib_run(pkg, r, ctx=ctx, dev=(d.rec, d.taps), orient=orient)
        st2, out = F.lib_run(pkg, s, ctx=ctx, dev=d.taps, e_count=96)
    finally:
        d.free()
    assert st == st2 == pkg.abi.OK and list(ref.windows) == [9, 10, 2]
    F.assert_same_outputs(ref, out)
    assert np.any(ref.paths == 0) and np.any(ref.paths > 0)


A2 = dict(svs=[3, 16], cd=[3684, 26051], ff=[4580975.0, 4579675.0])  # test_gpu_replay.py's scene


def test_the_chain_stays_resident(pkg, ctx, opensky_short):
    """2 channels x 200 rows of the GIVEN loop replayed at -1.5:0.05:1.5 into HBM and fitted there
    (the tensor of replay_correlate(device_out=True), then replay_fit): the bits of the chain
    with the replay's sums returned to the host and fitted by the host path."""
    skip, cfg, data = opensky_short
    file, signal, acq, track = params(pkg, skip, data)
    A = acquired_of(A2["svs"], A2["cd"], A2["ff"])
    buf = pkg.trackingCT_multiCorr(file, signal, track, A, datalength=200, ctx=ctx, raw=True)
    t = pkg.replay_rows(buf, A, file, signal, loop="given")
    taps = pkg.colon(-1.5, 0.05, 1.5)
    assert list(t.n_rows) == [200, 200] and len(taps) == 61
    par = dict(numOverLap=64, ind_start=7, want_acf=True)
    on_dev, ms = pkg.replay_correlate(file, signal, t, taps, ctx=ctx, device_out=True)
    assert on_dev.is_cuda
    dev = pkg.acf_fit_taps(on_dev, t.n_rows, taps, ctx=ctx, **par)
    sums, _ = pkg.replay_correlate(file, signal, t, taps, ctx=ctx)  # the kernel's sums downloaded by the call
    assert K.same_bits(sums, on_dev.cpu().numpy())
    host = pkg.acf_fit_taps(sums, t.n_rows, taps, **par)
    both = pkg.replay_fit(file, signal, t, taps, ctx=ctx, **par)
    assert list(dev.windows) == [3, 3] and dev.kernel_ms > 0 and host.kernel_ms == 0
    assert both.kernel_ms[0] > 0 and both.kernel_ms[1] > 0
    for c in range(2):
        assert np.array_equal(dev.paths[c], host.paths[c]) and np.array_equal(both.paths[c], host.paths[c])
        assert np.all(host.paths[c] > 0)
        for k in T.FIELDS + ["zI", "zQ", "ratio", "dphi_cycles", "bias_m"]:
            assert K.same_bits(getattr(dev, k)[c], getattr(host, k)[c]), (c, k)
            assert K.same_bits(getattr(both, k)[c], getattr(host, k)[c]), (c, k)


# ---- end to end --------------------------------------------------------------------------------
E2E_E, E2E_RATIO = 1.7, 0.5


def test_end_to_end_ray_1_7_chips_late(pkg, ctx):
    """test_gpu_acf_fit.py's scene (PRN 3 alone at 55 dB-Hz) with the ray 1.7 chips late at half the
    amplitude, in phase; gnss_tracking_ct_multicorr for 600 rows; rows 99-599 replayed on
    -2.5:0.05:1.0 and fitted in HBM (501 rows: the window rule, floor((L - ind_start) / numOverLap),
    gives five windows of 100 rows only from 501 on), every one of the five asserted: the library
    equals the twin on the same replayed sums bit for bit, paths = 2, |e - 1.7| <= 0.05,
    |ratio - 0.5| <= 0.1, |bias| <= 0.03 (the bounds test_gpu_acf_fit.py sets for the 0.5-chip ray).
    The 25-tap fit of the same loop's records sees one path in windows 1..4: the ray touches none
    of its taps."""
    sc = pkg.synth.scene_of(pkg.synth.scenario([3], [3683], [990.0], [55.0], skip_ms=2))
    pkg.synth.add_ray(sc, 3, E2E_E, E2E_RATIO, phase_cycles=0.0)
    A = acquired_of([3], [3683], [4580990.0])
    taps = pkg.colon(-2.5, 0.05, 1.0)
    rec = pkg.DeviceRecord(ctx, 2 * (2 + 1 + 600 + 4) * 58000)
    try:
        pkg.synth.generate_scene_device(ctx, sc, rec)
        file, signal, acq, track = params(pkg, 2, None)
        file.dev = rec
        buf = pkg.trackingCT_multiCorr(file, signal, track, A, datalength=600, ctx=ctx, raw=True)
        t = pkg.replay_rows(buf, A, file, signal, loop="given", rows=range(99, 600))
        f = pkg.replay_fit(file, signal, t, taps, ctx=ctx, numOverLap=100, want_acf=True)
        sums, _ = pkg.replay_correlate(file, signal, t, taps, ctx=ctx)  # the same rows' sums on the host
    finally:
        rec.free()
    assert list(t.n_rows) == [501] and f.windows[0] == 5 and f.prompt == 50
    tw = T.fit(sums, t.n_rows, taps, 50, numOverLap=100)[0]
    a0, a1 = tw["A0_re"] + 1j * tw["A0_im"], tw["A1_re"] + 1j * tw["A1_im"]
    print("wide fit  paths", f.paths[0], "e", f.e[0], "ratio", np.round(f.ratio[0], 4), "bias", f.bias[0],
          "res1/res2", np.round(f.res1[0] / f.res2[0], 1), "kernel_ms", f.kernel_ms)
    print("twin      paths", tw["paths"], "e", tw["e"], "ratio", np.round(np.abs(a1) / np.abs(a0), 4), "bias", tw["bias"])
    f25 = pkg.acf_fit(buf, [3])  # (the raw records carry the GIVEN loop's orientation)
    print("25-tap fit paths", f25.paths[0], "bias", f25.bias[0], "e", f25.e[0], "res1/res2",
          np.round(f25.res1[0] / f25.res2[0], 2))
    assert np.array_equal(f.paths[0], tw["paths"])
    for k in T.FIELDS + ["zI", "zQ"]:
        assert K.same_bits(getattr(f, k)[0], tw[k]), k
    assert np.all(f.paths[0] == 2)
    assert np.all(np.abs(f.e[0] - E2E_E) <= 0.05)
    assert np.all(np.abs(f.ratio[0] - E2E_RATIO) <= 0.1)
    assert np.all(np.abs(f.bias[0]) <= 0.03)
    assert f25.windows[0] == 5 and np.all(f25.paths[0][1:] == 1)


def test_refusals_leave_the_context_usable(pkg, ctx):
    abi = pkg.abi
    s = F.sums(33, 16, [400, 131], 401)
    _, host = F.lib_run(pkg, s, **F.SMALL)
    d = Up(ctx, s.taps)
    try:
        run = lambda c=ctx, **kw: F.lib_run(pkg, s, ctx=c, dev=d.ptr, **dict(F.SMALL, **kw))

        def fine():
            st, out = run()
            assert st == abi.OK
            F.assert_same_outputs(host, out)

        fine()
        nan_u = s.u.copy()
        nan_u[32] = np.nan
        for bad in (dict(n=0), dict(n=abi.VT_MAX_CH + 1), dict(n_taps=0), dict(n_taps=257), dict(prompt=-1),
                    dict(prompt=33), dict(u=nan_u), dict(u=None, n_taps=33), dict(numOverLap=1),
                    dict(numOverLap=4097, cap=4), dict(ind_start=0), dict(p_step=0.0), dict(e_step=float("nan")),
                    dict(p_min=float("inf")), dict(p_count=0), dict(p_count=257, e_count=256), dict(ratio_max=-1.0),
                    dict(gain_min=float("nan")), dict(cap=2), dict(flags=abi.OUT_DEVICE | 2), dict(taps=None),
                    dict(n_rows=None), dict(max_rows=0),
                    dict(n_rows=np.array([400, 402], dtype=np.int64), cap=8),  # n_rows[c] = max_rows + 1
                    dict(taps=s.taps.ctypes.data),                             # a host pointer as device sums
                    dict(max_rows=402)):                                       # more than the allocation holds
            st, out = run(**bad)
            assert st == abi.EARG, bad
            assert out.untouched(), bad
            assert ctx.lib.gnss_last_error(ctx.h)
            fine()
        assert F.lib_run(pkg, s, dev=d.ptr, **F.SMALL)[0] == abi.EARG  # device sums without a context
        m = pkg.Context(devices=[0, 0])  # a context of gnss_ctx_create_multi
        try:
            st, out = run(m)
            assert st == abi.EARG and out.untouched()
        finally:
            m.close()
        fine()
        import torch
        with pytest.raises(ValueError):
            pkg.acf_fit_taps(torch.zeros((1, 2, 3, 8), dtype=torch.float64, device="cuda:0"), [8], [-0.5, 0.0, 0.5])
        with pytest.raises(ValueError):
            pkg.acf_fit_taps(torch.zeros((1, 2, 3, 8), dtype=torch.float32, device="cuda:0"), [8], [-0.5, 0.0, 0.5],
                             ctx=ctx)
        fine()
    finally:
        d.free()
