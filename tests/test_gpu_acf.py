"""GPU tests of ACF/CalculateFeatures.m on device-resident 25-tap records (gnss_acf_features with
GNSS_OUT_DEVICE, csrc/acf.hip): the kernels' outputs equal the host path's bit for bit -- the
features, maxCorrInd and corr -- on every case of test_acf_kat.py (odd max_len: one row per lane)
and on even max_len (two rows per lane, a tail lane whose second row lies past len), with the
optional outputs NULL and non-NULL; a channel of 100 001 rows beside one of 101; end to end on the
resident buffers of gnss_tracking_ct_mc; the refusals, each leaving the context usable."""
import ctypes as C

import numpy as np
import pytest

import acf_common as K
import acf_twin as T
from conftest import acquired_of, params

pytestmark = pytest.mark.gpu


class Dev:
    """Device copies of a record set's rec and taps, and device arrays for the optional outputs."""

    def __init__(self, ctx, r, want=True):
        self.ctx, self.r, self.ptrs = ctx, r, []
        self.rec, self.taps = self.upload(r.rec), self.upload(r.taps)
        self.ind = self.corr = None
        if want:  # filled like the host's, so rows past len compare as untouched
            self.ind = self.upload(np.zeros((r.n, r.max_len), dtype=np.uint8))
            self.corr = self.upload(np.full((r.n, 25, r.max_len), -7.0))

    def upload(self, a):
        p = C.c_void_p()
        self.ctx.check(self.ctx.lib.gnss_dev_alloc(self.ctx.h, C.c_uint64(a.nbytes), C.byref(p)))
        self.ptrs.append(p)
        self.ctx.check(self.ctx.lib.gnss_dev_upload(self.ctx.h, p, a.ctypes.data_as(C.c_void_p), C.c_uint64(a.nbytes)))
        return p.value

    def download(self, ptr, shape, dtype):
        a = np.empty(shape, dtype=dtype)
        self.ctx.check(self.ctx.lib.gnss_dev_download(self.ctx.h, a.ctypes.data_as(C.c_void_p), C.c_void_p(ptr),
                                                      C.c_uint64(a.nbytes)))
        return a

    def outputs(self):
        r = self.r
        return (self.download(self.ind, (r.n, r.max_len), np.uint8),
                self.download(self.corr, (r.n, 25, r.max_len), np.float64))

    def free(self):
        for p in self.ptrs:
            self.ctx.lib.gnss_dev_free(self.ctx.h, p)
        self.ptrs = []


def device_equals_host(pkg, ctx, r, **par):
    st, host = K.lib_run(pkg, r, want=True, **par)
    assert st == pkg.abi.OK
    d = Dev(ctx, r)
    try:
        st, dev = K.lib_run(pkg, r, ctx=ctx, dev=(d.rec, d.taps), dev_ind=d.ind, dev_corr=d.corr, **par)
        assert st == pkg.abi.OK, ctx.lib.gnss_last_error(ctx.h)
        K.assert_same_outputs(host, dev)
        ind, corr = d.outputs()
        assert np.array_equal(ind, host.ind)
        assert K.same_bits(corr, host.corr)
        st, bare = K.lib_run(pkg, r, ctx=ctx, dev=(d.rec, d.taps), **par)  # the optional outputs NULL
        assert st == pkg.abi.OK
        K.assert_same_outputs(host, bare)
    finally:
        d.free()
    return host


@pytest.mark.parametrize("numOverLap", [100, 2, 64])
@pytest.mark.parametrize("ind_start", [1, 7])
@pytest.mark.parametrize("shape", ["short", "long"])
def test_device_path_equals_host(pkg, ctx, shape, ind_start, numOverLap):
    r = K.records(shape)
    host = device_equals_host(pkg, ctx, r, ind_start=ind_start, numOverLap=numOverLap)
    _, chans = K.twin(r, ind_start=ind_start, numOverLap=numOverLap)
    K.assert_equals_twin(r, host, chans, host.ind, host.corr)


@pytest.mark.parametrize("lens,max_len", [([1000, 1001, 257], 1004), ([99, 100, 101], 102), ([513, 512, 511], 514)])
def test_two_rows_per_lane(pkg, ctx, lens, max_len):
    """Even max_len: 16-B loads, two rows per lane; an odd len ends in a lane whose second row is
    loaded (it lies inside the series) and never stored; 512 rows fill one block exactly."""
    r = K.records("long", lens=lens, max_len=max_len)
    for par in (dict(), dict(ind_start=7, numOverLap=64), dict(ind_start=2, numOverLap=2)):
        device_equals_host(pkg, ctx, r, **par)


def test_long_channel_beside_a_short_one(pkg, ctx):
    """100 001 rows beside 101: 1000 windows against 1, the windows cross the row pass's blocks
    and the window kernel's waves; on both row forms (even and odd max_len)."""
    for max_len in (100002, 100003):
        r = K.records("long", lens=[100001, 101], max_len=max_len)
        host = device_equals_host(pkg, ctx, r)
        assert list(host.windows) == [1000, 1]
    _, chans = K.twin(r)
    K.assert_equals_twin(r, host, chans, host.ind, host.corr)


def test_end_to_end_on_resident_records(pkg, ctx, opensky_short):
    """gnss_tracking_ct_mc with GNSS_OUT_DEVICE, then the features on the buffers as they lie in
    HBM: equal to the twin on the downloaded records, and to the mirror's data_labeled."""
    from test_gpu_pos import OPENSKY
    skip, cfg, data = opensky_short
    file, signal, acq, track = params(pkg, skip, data)
    track.msPosCT, track.pdi = 400, 1
    A = acquired_of(OPENSKY["svs"], OPENSKY["cd"], OPENSKY["ff"])
    buf = pkg.trackingCT_POS_updated_multicorrelator(file, signal, track, A, ctx=ctx, raw=True, device_records=True)
    assert buf.c.flags == pkg.abi.OUT_DEVICE and list(buf.len) == [400] * 8
    ele = [8.36, 54.23, 24.23, 47.1, 6.39, 31.54, 45.0, 64.42]
    f = pkg.acf_features(buf, OPENSKY["svs"], ele, ctx=ctx, want_index=True, want_corr=True)
    h = buf.host()
    want, chans = T.features(h.taps, h.rec[:, pkg.abi.FIELDS_POS.index("codeError")], h.len, OPENSKY["svs"], ele)
    assert list(f.windows) == [3] * 8 and want.shape == (25, 8)
    for c, ch in enumerate(chans):
        for k in T.FIELDS:
            if k == "F1":
                assert np.all(K.ulps(getattr(f, k)[c], ch[k]) <= 2)
            else:
                assert K.same_bits(getattr(f, k)[c], ch[k]), (c, k)
        assert np.array_equal(f.maxCorrInd[c].cpu().numpy(), ch["maxCorrInd"])
        assert K.same_bits(f.corr[c].cpu().numpy(), ch["corr"])
        assert np.all(ch["meanMax"] > 0)
    got = pkg.CalculateFeatures(buf, OPENSKY["svs"], ele, ctx=ctx)
    assert got.shape == want.shape and not np.any(got[0])
    for col in (0, 1, 2, 4, 5, 6, 7):
        assert K.same_bits(got[:, col], want[:, col]), col
    # the same from the host records and from the per-PRN structs
    tck, _ = pkg.trackingCT_POS_updated_multicorrelator(file, signal, track, A, ctx=ctx)
    for src in (h, tck):
        again = pkg.CalculateFeatures(src, OPENSKY["svs"], ele)
        assert K.same_bits(again, got)


def test_refusals_leave_the_context_usable(pkg, ctx):
    abi = pkg.abi
    r = K.records("long", max_len=1004)
    _, host = K.lib_run(pkg, r)
    d = Dev(ctx, r, want=False)
    try:
        run = lambda c=ctx, **kw: K.lib_run(pkg, r, ctx=c, dev=(d.rec, d.taps), **kw)

        def fine():
            st, out = run()
            assert st == abi.OK
            K.assert_same_outputs(host, out)

        fine()
        for bad in (dict(n_taps=24), dict(numOverLap=1), dict(numOverLap=4097, cap=4), dict(ind_start=0),
                    dict(corrSpacing=0.0), dict(cap=9), dict(n=0), dict(n=abi.VT_MAX_CH + 1)):
            assert run(**bad)[0] == abi.EARG, bad
            assert ctx.lib.gnss_last_error(ctx.h)
            fine()
        keep = r.lens[2]
        r.lens[2] = r.max_len + 1  # the kernels would index past the series: refused before any launch
        assert run(cap=16)[0] == abi.EARG
        r.lens[2] = keep
        fine()
        assert K.lib_run(pkg, r, dev=(d.rec, d.taps))[0] == abi.EARG  # device records without a context
        m = pkg.Context(devices=[0, 0])  # no gathering across members
        try:
            assert run(m)[0] == abi.EARG
        finally:
            m.close()
        fine()
    finally:
        d.free()
