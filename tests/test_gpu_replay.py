"""The replay correlator on the GPU (gnss_replay_correlate with a context: csrc/replay.hip) against
the oracle's correlate_step, the numpy twin, the host path and the records of the GPU's own loops.
Tolerance: differences below 1e-8 of the scale. Bits: a row's do not depend on the other
rows or channels, on host or device output, on segmentation, on where the record lies, or on the run.
The shapes are the smallest at which the kernel can go wrong: numSample around its 256 lanes, the
odd-length row's middle element, every byte alignment, tap counts around its tile of 32."""
import numpy as np
import pytest

import replay_common as rc
from conftest import acquired_of, params

pytestmark = pytest.mark.gpu

TILE = 32  # csrc/replay.h kReplayTile


def dev(pkg, ctx, dt, t, taps, chip_off=0, post=None, data=None, **kw):
    file, signal = rc.file_signal(pkg, dt, data)
    out, ms = pkg.replay_correlate(file, signal, t, taps, chip_off, post, ctx=ctx, **kw)
    assert ms > 0.0
    return out


def host(pkg, dt, t, taps, chip_off=0, post=None, data=None):
    file, signal = rc.file_signal(pkg, dt, data)
    return pkg.replay_correlate(file, signal, t, taps, chip_off, post)[0]


@pytest.mark.parametrize("name", ["edges-1tap-type2", "edges-25-type2", "align-25-type2", "edges-1tap-type1",
                                  "edges-25-type1", "align-25-type1", "wide-61", "many-256", f"tile-{TILE - 1}",
                                  f"tile-{TILE}", f"tile-{TILE + 1}"])
def test_device_against_the_oracle(pkg, po, ctx, name):
    dt, t, taps = rc.oracle_cases(po)[name]
    err = rc.rel_err(dev(pkg, ctx, dt, t, taps), rc.oracle_ref(po, name), t)
    print(name, "device vs oracle", err)
    assert err < rc.TOL


@pytest.mark.parametrize("name", ["far-off0", "far-off1", "far-off1-post", "far-off0-post-real"])
def test_device_against_the_twin(pkg, po, ctx, name):
    dt, t, taps, off, post = rc.twin_cases()[name]
    err = rc.rel_err(dev(pkg, ctx, dt, t, taps, off, post), rc.twin_ref(po, name), t)
    print(name, "device vs twin", err)
    assert err < rc.TOL


def test_rows_spanning_more_chips_than_the_code_table(pkg, po, ctx):
    """A row of over 16384 chips takes the kernel's modulus form: the same sums (the oracle's)."""
    t = rc.table([16], [[(64, 58001, 0.25, 20e6, 4.58e6, 0.5), (70, 257, -0.3, 1.023e6, 0.0, 0.0)]])
    taps = np.array([-0.5, 0.0, 0.5])
    ref = rc.oracle_table(po, 2, t, taps)
    assert rc.rel_err(dev(pkg, ctx, 2, t, taps), ref, t) < rc.TOL
    assert rc.rel_err(host(pkg, 2, t, taps), ref, t) < rc.TOL


def mixed_rows(n_rows_per_chan, n=2049):
    prn = [3, 16, 22, 26, 31, 32, 4, 27][: len(n_rows_per_chan)]
    return rc.table(prn, [[(64 + 2 * ((7 * i + c) % 4000), n + (i % 3), *rc.state(i + c)) for i in range(k)]
                          for c, k in enumerate(n_rows_per_chan)])


def test_channels_with_0_1_2_and_300_rows(pkg, po, ctx):
    t = mixed_rows([0, 1, 2, 300], n=700)
    taps = rc.taps_25(po)
    got = dev(pkg, ctx, 2, t, taps)
    assert rc.rel_err(got, host(pkg, 2, t, taps), t) < rc.TOL
    assert np.all(got[0] == 0) and np.all(got[1, :, :, 1:] == 0) and np.all(got[2, :, :, 2:] == 0)


def test_8_channels_of_64_rows(pkg, po, ctx):
    t = mixed_rows([64] * 8, n=1500)
    taps = rc.taps_25(po)
    assert rc.rel_err(dev(pkg, ctx, 2, t, taps), host(pkg, 2, t, taps), t) < rc.TOL


def test_a_10_ms_row_beside_1_ms_rows(pkg, po, ctx):
    t = rc.table([16], [[(64, 58001, *rc.state(0)), (100, 580003, *rc.state(1)), (4000, 57999, *rc.state(2))]])
    taps = rc.taps_25(po)
    assert rc.rel_err(dev(pkg, ctx, 2, t, taps), host(pkg, 2, t, taps), t) < rc.TOL


# ---- the records of the GPU's own loops ------------------------------------------------------------
A2 = dict(svs=[3, 16], cd=[3684, 26051], ff=[4580975.0, 4579675.0])


def prompt_rms(buf, n):
    return float(np.sqrt(np.mean(buf.rec[:, 0, :n] ** 2 + buf.rec[:, 1, :n] ** 2)))


@pytest.fixture(scope="module")
def given(pkg, ctx, opensky_short):
    """600 rows of gnss_tracking_ct_multicorr on two channels, and their replay table."""
    skip, cfg, data = opensky_short
    file, signal, acq, track = params(pkg, skip, data)
    A = acquired_of(A2["svs"], A2["cd"], A2["ff"])
    buf = pkg.trackingCT_multiCorr(file, signal, track, A, datalength=600, ctx=ctx, raw=True)
    return file, signal, A, buf, pkg.replay_rows(buf, A, file, signal, loop="given")


def test_given_records_replayed_with_their_own_taps(pkg, ctx, given):
    file, signal, A, buf, t = given
    out, ms = pkg.replay_correlate(file, signal, t, t.taps, t.chip_off, t.post, ctx=ctx)
    err = np.max(np.abs(out - buf.taps[:, :, :, :600])) / prompt_rms(buf, 600)
    print("device replay of the GIVEN records", err, "kernel_ms", ms)
    assert err < rc.TOL


@pytest.mark.parametrize("pdi,n", [(1, 120), (10, 12)])
def test_mc_records_replayed_with_their_own_taps(pkg, ctx, opensky_short, pdi, n):
    skip, cfg, data = opensky_short
    file, signal, acq, track = params(pkg, skip, data)
    A = acquired_of(A2["svs"], A2["cd"], A2["ff"])
    track.msPosCT, track.pdi = 120, pdi
    buf = pkg.trackingCT_POS_updated_multicorrelator(file, signal, track, A, ctx=ctx, raw=True)
    t = pkg.replay_rows(buf, A, file, signal, loop="mc")
    assert list(t.n_rows) == [n, n]
    out, _ = pkg.replay_correlate(file, signal, t, t.taps, t.chip_off, t.post, ctx=ctx)
    err = np.max(np.abs(out - buf.taps[:, :, :, :n])) / prompt_rms(buf, n)
    print("device replay of the mc records, pdi", pdi, err)
    assert err < rc.TOL


def test_pos_records_replayed_with_post(pkg, ctx, opensky_short):
    skip, cfg, data = opensky_short
    file, signal, acq, track = params(pkg, skip, data)
    A = acquired_of(A2["svs"], A2["cd"], A2["ff"])
    track.msToProcessCT_1ms, track.ctPOS = 20, 26
    buf = pkg.trackingCT_POS(file, signal, track, A, [0, 0], ctx=ctx, raw=True)
    t = pkg.replay_rows(buf, A, file, signal, loop="pos")
    assert t.numSample[0, 19] < 60000 < t.numSample[0, 20]
    out, _ = pkg.replay_correlate(file, signal, t, t.taps, t.chip_off, t.post, ctx=ctx)
    F, scale = pkg.abi.FIELDS, prompt_rms(buf, 26)
    for k, name in enumerate("EPL"):
        for iq, s in enumerate("iq"):
            err = np.max(np.abs(out[:, iq, k, :26] - buf.rec[:, F.index(f"{name}_{s}"), :26])) / scale
            assert err < rc.TOL, (name, s, err)


@pytest.fixture(scope="module")
def wide(pkg, po, ctx, given):
    """Rows 0-99 of both channels at -1.5:0.05:1.5 on the device (host output)."""
    file, signal, A, buf, _ = given
    t = pkg.replay_rows(buf, A, file, signal, loop="given", rows=range(100))
    taps = rc.taps_61(po)
    out, _ = pkg.replay_correlate(file, signal, t, taps, ctx=ctx)
    return t, taps, out


def test_device_equals_host_path_within_tolerance(pkg, given, wide):
    file, signal, A, buf, _ = given
    t, taps, out = wide
    ref, _ = pkg.replay_correlate(file, signal, t, taps)
    err = np.max(np.abs(out - ref)) / prompt_rms(buf, 100)
    print("device vs host path, 61 taps", err)
    assert err < rc.TOL


def test_device_output_second_run_and_row_subset_give_the_same_bits(pkg, ctx, given, wide):
    file, signal, A, buf, _ = given
    t, taps, out = wide
    again, _ = pkg.replay_correlate(file, signal, t, taps, ctx=ctx)
    assert rc.same_bits(again, out)
    on_dev, _ = pkg.replay_correlate(file, signal, t, taps, ctx=ctx, device_out=True)
    assert rc.same_bits(on_dev.cpu().numpy(), out)
    sub = pkg.replay_rows(buf, A, file, signal, loop="given", rows=[3, 50, 97])
    part, _ = pkg.replay_correlate(file, signal, sub, taps, ctx=ctx)
    assert rc.same_bits(part[:, :, :, :3], out[:, :, :, [3, 50, 97]])
    one = rc.subset(t, [1], lambda c: range(100))
    alone, _ = pkg.replay_correlate(file, signal, one, taps, ctx=ctx)
    assert rc.same_bits(alone[0], out[1])


def test_a_small_window_segments_the_rows_with_the_same_bits(pkg, ctx, given, wide):
    file, signal, A, buf, _ = given
    t, taps, out = wide
    ctx.set_window(4 << 20)  # 100 rows of two channels span 11.6 MB
    try:
        seg, _ = pkg.replay_correlate(file, signal, t, taps, ctx=ctx)
        assert ctx.timing()["track_segments"] >= 3
        ctx.set_window(1 << 16)  # below one row
        with pytest.raises(pkg.abi.GnssError) as e:
            pkg.replay_correlate(file, signal, t, taps, ctx=ctx)
        assert e.value.status == pkg.abi.EARG
    finally:
        ctx.set_window(0)
    assert rc.same_bits(seg, out)


def test_a_device_resident_record_gives_the_same_bits(pkg, po, ctx):
    sc, A = rc.e2e_scene(pkg, ray=True)
    n = 40 * 58000
    rec = pkg.DeviceRecord(ctx, 2 * n)
    try:
        pkg.synth.generate_scene_device(ctx, sc, rec)
        data = rec.download()
        file, signal, acq, track = params(pkg, 5, None)
        file.dev = rec
        buf = pkg.trackingCT_multiCorr(file, signal, track, A, datalength=30, ctx=ctx, raw=True)
        t = pkg.replay_rows(buf, A, file, signal, loop="given")
        taps = rc.taps_61(po)
        resident, _ = pkg.replay_correlate(file, signal, t, taps, ctx=ctx)
        file.dev, file.data = None, data
        staged, _ = pkg.replay_correlate(file, signal, t, taps, ctx=ctx)
    finally:
        rec.free()
    assert rc.same_bits(resident, staged)


def test_refusals_leave_the_context_usable(pkg, po, ctx):
    t = rc.edge_rows(2, [255, 256, 257])
    taps = np.array([-0.5, 0.0, 0.5])
    good = dev(pkg, ctx, 2, t, taps)
    for name, status, mutate in rc.refusals(pkg.abi):
        st, untouched = rc.refusal_call(pkg, pkg.abi, ctx, mutate)
        assert st == status and untouched, (name, st)
        if name == "colon count":
            msg = pkg.abi.load().gnss_last_error(ctx.h).decode()
            assert "channel 0 row 1 tap 0" in msg, msg
        assert rc.same_bits(dev(pkg, ctx, 2, t, taps), good), name
    # GNSS_OUT_DEVICE with host memory, and a multi-device context
    import ctypes as C
    file, signal = rc.file_signal(pkg, 2)
    f, _k = pkg.sdr.to_c_file(file)
    s = pkg.sdr.to_c_signal(signal)
    cfg, r, out = pkg.abi.GnssReplayCfg(), pkg.abi.GnssReplayRows(), pkg.abi.GnssReplayOut()
    cfg.n_taps, cfg.tap_offsets, cfg.flags = 3, taps.ctypes.data, pkg.abi.OUT_DEVICE
    r.n_chan, r.max_rows = 1, t.max_rows
    for name in ("prn", "n_rows", "pos_bytes", "numSample", "remChip", "codeFreq", "carrFreq", "remPhase"):
        setattr(r, name, getattr(t, name).ctypes.data)
    res = np.zeros((1, 2, 3, t.max_rows))
    out.taps = res.ctypes.data
    lib = pkg.abi.load()
    assert lib.gnss_replay_correlate(ctx.h, C.byref(f), C.byref(s), C.byref(cfg), C.byref(r), C.byref(out)) == pkg.abi.EARG
    multi = pkg.Context(devices=[0, 0])
    try:
        cfg.flags = 0
        assert lib.gnss_replay_correlate(multi.h, C.byref(f), C.byref(s), C.byref(cfg), C.byref(r),
                                         C.byref(out)) == pkg.abi.EARG
    finally:
        multi.close()
    assert np.all(res == 0)
    assert rc.same_bits(dev(pkg, ctx, 2, t, taps), good)


def test_end_to_end_ray_beyond_the_25_taps_on_the_device(pkg, po, ctx):
    """The end-to-end conditions of tests/test_replay_kat.py with the GPU's GIVEN loop and the kernel."""
    taps = rc.taps_61(po)
    n = 271 * 58000
    rec = pkg.DeviceRecord(ctx, 2 * n)
    m = {}
    try:
        for ray in (False, True):
            sc, A = rc.e2e_scene(pkg, ray)
            pkg.synth.generate_scene_device(ctx, sc, rec)
            file, signal, acq, track = params(pkg, 5, None)
            file.dev = rec
            buf = pkg.trackingCT_multiCorr(file, signal, track, A, datalength=260, ctx=ctx, raw=True)
            t = pkg.replay_rows(buf, A, file, signal, loop="given", rows=rc.E2E_ROWS)
            out, _ = pkg.replay_correlate(file, signal, t, taps, ctx=ctx)
            m[ray] = rc.e2e_profile(pkg, out, buf.rec[:, pkg.abi.FIELDS.index("P_i"), 150:250], taps)
    finally:
        rec.free()
    rc.e2e_check(taps, m[False], m[True])
