"""GPU tests of the multi-ray fit over device-resident sums (gnss_acf_fit_multi with
GNSS_OUT_DEVICE, csrc/acf_fit_multi.hip): the kernel's outputs equal the host path's bit for bit --
every field, `searches`, zI and zQ, given and NULL -- over acf_fit_multi_common's case list (tap
counts of one series group, one more, and the maximum; candidate counts 1, 255, 257, 281 and 4096;
max_paths 1..4; sweeps 0, 1, 4; window widths 2, 64, 65, 100 and 4096; lens 513 / 512 / 511 in a
series of 514; a long channel beside a short one) and on non-finite sums. Two runs give the same
bits; the chain replay -> fit stays resident with the host chain's bits; end to end two rays and the
direct path are resolved in every window; the refusals, each leaving the context usable."""
import ctypes as C

import numpy as np
import pytest

import acf_common as K
import acf_fit_multi_common as M
import acf_fit_multi_twin as T
from conftest import acquired_of, params

pytestmark = pytest.mark.gpu

SMALL = dict(q_min=-1.6, q_step=0.02, q_count=100, max_paths=3, sweeps=2, sep_min=5)


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
    st, host = M.lib_run(pkg, s, **par)
    assert st == pkg.abi.OK
    d = Up(ctx, s.taps)
    try:
        st, dev = M.lib_run(pkg, s, ctx=ctx, dev=d.ptr, **par)
        assert st == pkg.abi.OK, ctx.lib.gnss_last_error(ctx.h)
        M.assert_same_outputs(host, dev)
        st, bare = M.lib_run(pkg, s, ctx=ctx, dev=d.ptr, want=False, **par)  # zI / zQ NULL
        assert st == pkg.abi.OK
        M.assert_same_outputs(host, bare)
        st, again = M.lib_run(pkg, s, ctx=ctx, dev=d.ptr, **par)             # a second run: the same bits
        assert st == pkg.abi.OK
        M.assert_same_outputs(dev, again)
    finally:
        d.free()
    return host


@pytest.mark.parametrize("name", list(M.CASES))
def test_device_path_equals_host(pkg, ctx, name):
    s, par, windows = M.case(name)
    host = device_equals_host(pkg, ctx, s, **par)
    assert list(host.windows[: s.n]) == windows
    assert np.all(host.paths[0, : windows[0]] > 0)


def test_non_finite_sums_and_an_unsorted_grid(pkg, ctx):
    rng = np.random.default_rng(8)
    u = np.concatenate([[0.0], rng.uniform(-1.9, 0.8, 32)])[rng.permutation(33)]
    s = M.sums(33, int(np.flatnonzero(u == 0)[0]), [400, 0, 131], 401, u=u)
    s.taps[0, 1, 32, 70] = np.nan
    s.taps[0, 0, s.prompt, 140] = np.nan
    s.taps[2, 0, 0, 3] = np.inf
    host = device_equals_host(pkg, ctx, s, numOverLap=65, **SMALL)
    assert list(host.windows) == [6, 0, 2]
    assert list(host.paths[0, :6] == 0) == [False, True, True, False, False, False]
    assert list(host.paths[2, :2] == 0) == [True, False]
    M.assert_equals_twin(host, T.fit(s.taps, s.n_rows, s.u, s.prompt, numOverLap=65, **SMALL))


def test_a_candidate_grid_outside_the_taps(pkg, ctx):
    s = M.sums(25, 12, [131], 131)
    host = device_equals_host(pkg, ctx, s, numOverLap=65, q_min=1.7, q_step=0.01, q_count=50)
    assert np.all(host.paths[0, :2] == 0) and np.all(host.searches[0, :2] == 1)


A2 = dict(svs=[3, 16], cd=[3684, 26051], ff=[4580975.0, 4579675.0])  # test_gpu_replay.py's scene
NAMES = T.FIELDS + ["zI", "zQ", "ratio", "dphi_cycles", "e", "bias_m"]


def test_the_chain_stays_resident(pkg, ctx, opensky_short):
    """2 channels x 200 rows of the GIVEN loop replayed at -1.5:0.05:1.5 into HBM and fitted there
    (the tensor of replay_correlate(device_out=True), then replay_fit_multi): the bits of the chain
    with the replay's sums returned to the host and fitted by the host path."""
    skip, cfg, data = opensky_short
    file, signal, acq, track = params(pkg, skip, data)
    A = acquired_of(A2["svs"], A2["cd"], A2["ff"])
    buf = pkg.trackingCT_multiCorr(file, signal, track, A, datalength=200, ctx=ctx, raw=True)
    t = pkg.replay_rows(buf, A, file, signal, loop="given")
    taps = pkg.colon(-1.5, 0.05, 1.5)
    assert list(t.n_rows) == [200, 200] and len(taps) == 61
    par = dict(numOverLap=64, ind_start=7, want_acf=True, q_min=-1.4, q_count=181)
    on_dev, ms = pkg.replay_correlate(file, signal, t, taps, ctx=ctx, device_out=True)
    assert on_dev.is_cuda
    dev = pkg.acf_fit_multi(on_dev, t.n_rows, taps, ctx=ctx, **par)
    sums, _ = pkg.replay_correlate(file, signal, t, taps, ctx=ctx)  # the kernel's sums downloaded by the call
    assert K.same_bits(sums, on_dev.cpu().numpy())
    host = pkg.acf_fit_multi(sums, t.n_rows, taps, **par)
    both = pkg.replay_fit_multi(file, signal, t, taps, ctx=ctx, **par)
    assert list(dev.windows) == [3, 3] and dev.kernel_ms > 0 and host.kernel_ms == 0
    assert both.kernel_ms[0] > 0 and both.kernel_ms[1] > 0
    for c in range(2):
        for got in (dev, both):
            assert np.array_equal(got.paths[c], host.paths[c]) and np.array_equal(got.searches[c], host.searches[c])
            for k in NAMES:
                assert K.same_bits(getattr(got, k)[c], getattr(host, k)[c]), (c, k)
        assert np.all(host.paths[c] > 0)


# ---- end to end --------------------------------------------------------------------------------
E2E_RAYS = ((0.6, 0.5, 0.5), (1.4, 0.4, 0.25))  # (chips late, amplitude ratio, phase in cycles)


def test_end_to_end_two_rays(pkg, ctx):
    """test_acf_fit_multi_kat.py's chain on the device: PRN 3 alone at 55 dB-Hz with rays 0.6 chip
    late (half the amplitude, opposed) and 1.4 chips late (0.4, in quadrature);
    gnss_tracking_ct_multicorr for 600 rows; rows 99-599 replayed on -2.5:0.05:1.0 and fitted in
    HBM, five windows of 100 rows, every one asserted: the library equals the twin on the same
    replayed sums bit for bit, paths = 3, |e[k] - truth| <= 0.05, |ratio[k] - truth| <= 0.1. bias
    is printed, not asserted: the scene gives no truth for it."""
    sc = pkg.synth.scene_of(pkg.synth.scenario([3], [3683], [990.0], [55.0], skip_ms=2))
    for late, ratio, cyc in E2E_RAYS:
        pkg.synth.add_ray(sc, 3, late, ratio, phase_cycles=cyc)
    A = acquired_of([3], [3683], [4580990.0])
    taps = pkg.colon(-2.5, 0.05, 1.0)
    rec = pkg.DeviceRecord(ctx, 2 * (2 + 1 + 600 + 4) * 58000)
    try:
        pkg.synth.generate_scene_device(ctx, sc, rec)
        file, signal, acq, track = params(pkg, 2, None)
        file.dev = rec
        buf = pkg.trackingCT_multiCorr(file, signal, track, A, datalength=600, ctx=ctx, raw=True)
        t = pkg.replay_rows(buf, A, file, signal, loop="given", rows=range(99, 600))
        f = pkg.replay_fit_multi(file, signal, t, taps, ctx=ctx, numOverLap=100, want_acf=True)
        sums, _ = pkg.replay_correlate(file, signal, t, taps, ctx=ctx)  # the same rows' sums on the host
    finally:
        rec.free()
    assert list(t.n_rows) == [501] and f.windows[0] == 5 and f.prompt == 50
    tw = T.fit(sums, t.n_rows, taps, 50, numOverLap=100)[0]
    print("multi fit paths", f.paths[0], "searches", f.searches[0], "bias", f.bias[0], "kernel_ms", f.kernel_ms)
    print("          e", np.round(f.e[0][1:3], 3).tolist(), "ratio", np.round(f.ratio[0][1:3], 4).tolist())
    print("          res(m-1)/res(m)", np.round(f.res[0][:3] / f.res[0][1:4], 1).tolist())
    print("twin      paths", tw["paths"], "q", tw["q"][:3].tolist())
    assert np.array_equal(f.paths[0], tw["paths"]) and np.array_equal(f.searches[0], tw["searches"])
    for k in T.FIELDS + ["zI", "zQ"]:
        assert K.same_bits(getattr(f, k)[0], tw[k]), k
    assert np.all(f.paths[0] == 3)
    for k, (late, ratio, _) in enumerate(E2E_RAYS, start=1):
        assert np.all(np.abs(f.e[0][k] - late) <= 0.05), (k, f.e[0][k])
        assert np.all(np.abs(f.ratio[0][k] - ratio) <= 0.1), (k, f.ratio[0][k])


def test_refusals_leave_the_context_usable(pkg, ctx):
    abi = pkg.abi
    s = M.sums(33, 20, [400, 131], 401)
    _, host = M.lib_run(pkg, s, **SMALL)
    d = Up(ctx, s.taps)
    try:
        run = lambda c=ctx, **kw: M.lib_run(pkg, s, ctx=c, dev=d.ptr, **dict(SMALL, **kw))

        def fine():
            st, out = run()
            assert st == abi.OK
            M.assert_same_outputs(host, out)

        fine()
        nan_u = s.u.copy()
        nan_u[32] = np.nan
        for bad in (dict(n=0), dict(n=abi.VT_MAX_CH + 1), dict(n_taps=0), dict(n_taps=257), dict(prompt=-1),
                    dict(prompt=33), dict(u=nan_u), dict(u=None, n_taps=33), dict(numOverLap=1),
                    dict(numOverLap=4097, cap=4), dict(ind_start=0), dict(q_step=0.0), dict(q_step=float("nan")),
                    dict(q_min=float("inf")), dict(q_count=0), dict(q_count=4097), dict(max_paths=0), dict(max_paths=5),
                    dict(sweeps=-1), dict(sweeps=17), dict(sep_min=0), dict(sep_min=101), dict(gain_min=-1.0),
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
        assert M.lib_run(pkg, s, dev=d.ptr, **SMALL)[0] == abi.EARG  # device sums without a context
        m = pkg.Context(devices=[0, 0])  # a context of gnss_ctx_create_multi
        try:
            st, out = run(m)
            assert st == abi.EARG and out.untouched()
        finally:
            m.close()
        fine()
        import torch
        with pytest.raises(ValueError):
            pkg.acf_fit_multi(torch.zeros((1, 2, 3, 8), dtype=torch.float64, device="cuda:0"), [8], [-0.5, 0.0, 0.5])
        with pytest.raises(ValueError):
            pkg.acf_fit_multi(torch.zeros((1, 2, 3, 8), dtype=torch.float32, device="cuda:0"), [8], [-0.5, 0.0, 0.5],
                              ctx=ctx)
        fine()
    finally:
        d.free()
