"""GPU parity off the 58 MHz / 4.58 MHz grid: the tracking kernels, the acquisition through
rocFFT and the vector-tracking correlator at the sampling rates of tests/rate_matrix.py (26,
16.3676, 12.5, 10 and 8.5 MHz; zero IF with a negative and a zero-crossing carrier), against
the CPU oracle, which tests/test_oracle_rates.py pins on the same records.

Every comparison is an existing one, with its bounds unchanged: test_gpu_tracking.compare
(integer fields bit-exact, P/E/L within 1e-8 of the series RMS, NCO state at rtol 1e-7 / atol
1e-9, C/N0 within 1e-6 dB), test_gpu_acquisition.compare, test_gpu_vt._check (1e-9), and for a
single correlation step 1e-12 of the RMS (test_correlate_step_random_states).

With GNSS_RATE_REPORT=<file> in the environment the figures measured on the way (worst errors
per rate and variant, and the lane geometry of the engine's rule) are written to that file
(profiles/rate_matrix_parity.txt is such a run); they are a record, not thresholds."""
import importlib
import os
from types import SimpleNamespace

import numpy as np
import pytest

import rate_matrix as rm
from test_gpu_acquisition import compare as compare_acq
from test_gpu_acquisition import precision  # noqa: F401  (the fp64 / fp32 fixture)
from test_gpu_tracking import compare as compare_trk
from test_gpu_vt import _check as check_vt

pytestmark = pytest.mark.gpu

RATE_IDS = list(rm.RATES)
NOT_EDGE = [r for r in RATE_IDS if r != "edge_8m5"]
REPORT = {}  # (section, rate, variant) -> text


@pytest.fixture(scope="module", autouse=True)
def rate_report():
    yield
    path = os.environ.get("GNSS_RATE_REPORT")
    if not path or not REPORT:
        return
    with open(path, "w") as f:
        f.write("Rate-matrix parity, GPU vs CPU oracle (tests/test_gpu_rates.py): measured values, not thresholds.\n"
                "Bounds asserted: step sums 1e-12 of the RMS; P/E/L 1e-8 of the series RMS; 11-tap array 1e-10;\n"
                "SNR 1e-6 dB (fp64) / 1e-3 dB (fp32); VT sums 1e-9 of |P|.\n"
                "Lane geometry = the engine's rule (track_geom.h sub_ok / sub_for / bpc_for) as restated in\n"
                "tests/rate_matrix.py: lane span in samples / blocks per channel, 1-ms and 10-ms steps.\n\n")
        for rate, (Fs, IF) in rm.RATES.items():
            g1, g10 = rm.lane_geometry(Fs, 1), rm.lane_geometry(Fs, 10)
            f.write(f"{rate}: Fs {Fs:.10g} IF {IF:.10g} Sample {rm.sample_of(Fs)}; own choice: 1 ms {8 * g1[0]} "
                    f"samples / {g1[1]} blocks, 10 ms {8 * g10[0]} samples / {g10[1]} blocks; "
                    f"8*fc/Fs = {8 * rm.FC / Fs:.4f}\n")
        f.write("\n")
        for key in sorted(REPORT):
            f.write(f"{key[0]:<10} {key[1]:<10} {key[2]:<22} {REPORT[key]}\n")


def _sdr():
    return importlib.import_module("assignment-for-aae6102_gnss-sdr_amd.sdr")


def _pel_error(g, r):
    """Worst P/E/L error over the channels, relative to each channel's prompt RMS (compare's)."""
    worst = 0.0
    for c in range(len(r.len)):
        n = int(r.len[c])
        scale = np.sqrt(np.mean(r.rec[c, 0, :n] ** 2 + r.rec[c, 1, :n] ** 2))
        worst = max(worst, float(np.max(np.abs(g.rec[c, :6, :n] - r.rec[c, :6, :n])) / scale))
    return worst


def _track(pkg, ctx, rate, ntaps=3, prec=1, dtyp=2):
    taps = rm.taps11() if ntaps == 11 else None
    g = pkg.trackingCT(rm.file_of(rate, prec, dtyp), rm.signal_of(rate), rm.track_params(), rm.acquired_for(rate),
                       ctx=ctx, taps=taps, raw=True)
    return g, ctx.timing()["track_launches"]


def _geom(rate, forced=0):
    Fs = rm.RATES[rate][0]
    g1, g10 = rm.lane_geometry(Fs, 1, forced), rm.lane_geometry(Fs, 10, forced)
    return f"lanes {8 * g1[0]}/{8 * g10[0]} blocks {g1[1]}/{g10[1]}"


# ---- a. one correlation step ----------------------------------------------------------------
STEP_VARIANTS = [(rate, "default") for rate in RATE_IDS] + \
                [(rate, str(v)) for rate in RATE_IDS for v in rm.step_subs(rm.RATES[rate][0])]


@pytest.mark.parametrize("rate,sub", STEP_VARIANTS, ids=[f"{r}-sub{s}" for r, s in STEP_VARIANTS])
def test_correlate_step_rates(pkg, po, ctx, opts, rate, sub):
    """gnss_correlate_step over the rate's case list (both pdi, 3 and 11 taps, early / late
    samples on exact chip boundaries, negative and zero carriers and phases, f/Fs up to 0.42)
    with the default lane span and with every GNSS_OPT_FORCE_SUB the rate admits."""
    if sub != "default":
        opts(pkg.abi.OPT_FORCE_SUB, int(sub))
    sdr = _sdr()
    file, signal = rm.file_of(rate), rm.signal_of(rate)
    worst, bad = 0.0, []
    for case, r in zip(rm.step_cases(rate), rm.oracle_steps(rate)):
        g, ns = sdr.correlate_step(file, signal, case.prn, case.pdi, case.remChip, case.codeFreq, case.carrierFreq,
                                   case.remPhase, case.pos_bytes, rm.case_taps(case), ctx=ctx)
        err = float(np.max(np.abs(g - r)) / np.sqrt(np.mean(r ** 2)))
        worst = max(worst, err)
        if ns != case.n or not err < 1e-12:
            bad.append((vars(case), ns, err))
    REPORT[("a.step", rate, f"sub {sub}")] = f"worst sum error / RMS {worst:.3e} over {len(rm.step_cases(rate))} cases"
    print(rate, sub, "worst step error / RMS", worst)
    assert not bad, (len(bad), bad[:3])


# ---- b. closed-loop trackingCT ----------------------------------------------------------------
@pytest.mark.parametrize("rate", RATE_IDS)
def test_tracking_persistent_and_step(pkg, ctx, opts, rate):
    """3 channels, 700 x 1 ms + 60 ms at 10 ms: the persistent loop (at most 4 launches) against
    the oracle, and one launch per step bit-identical to it. At 8.5 MHz (inside sub_ok's 1.1
    margin, the kernel's d * M = 0.963) the rate is admitted, so it must run like the others:
    no GNSS_EINDEX from inside a run."""
    r = rm.oracle_tracking(rate)
    assert r.status == 0
    p, launches = _track(pkg, ctx, rate)
    err = _pel_error(p, r)
    REPORT[("b.track", rate, "persistent")] = f"worst P/E/L error / RMS {err:.3e}; {launches} launches; {_geom(rate)}"
    print(rate, "persistent: worst P/E/L", err, "launches", launches)
    assert launches <= 4
    compare_trk(pkg, p, r)
    opts(pkg.abi.OPT_NO_PERSIST, 1)
    q, launches_q = _track(pkg, ctx, rate)
    REPORT[("b.track", rate, "step")] = (f"worst P/E/L error / RMS {_pel_error(q, r):.3e}; {launches_q} launches; "
                                         f"{_geom(rate)}")
    assert launches_q > 100
    for c in range(3):
        assert np.array_equal(p.rec[c], q.rec[c]), c
        assert p.len[c] == q.len[c] and p.countinx[c] == q.countinx[c]
    assert np.array_equal(p.CN0, q.CN0)


SUB_VARIANTS = [(rate, v) for rate in NOT_EDGE for v in rm.tracking_subs(rm.RATES[rate][0])]


@pytest.mark.parametrize("persist", [True, False], ids=["persistent", "step"])
@pytest.mark.parametrize("rate,sub", SUB_VARIANTS, ids=[f"{r}-sub{v}" for r, v in SUB_VARIANTS])
def test_tracking_every_admitted_sub(pkg, ctx, opts, rate, sub, persist):
    """Every lane span the rate admits (8 * SUB * 1.1 * fc / Fs < 1), through both paths."""
    opts(pkg.abi.OPT_FORCE_SUB, sub)
    if not persist:
        opts(pkg.abi.OPT_NO_PERSIST, 1)
    r = rm.oracle_tracking(rate)
    g, launches = _track(pkg, ctx, rate)
    err = _pel_error(g, r)
    REPORT[("b.track", rate, f"sub {sub} {'persistent' if persist else 'step'}")] = \
        f"worst P/E/L error / RMS {err:.3e}; {launches} launches; {_geom(rate, sub)}"
    print(rate, sub, persist, "worst P/E/L", err, "launches", launches)
    compare_trk(pkg, g, r)


@pytest.mark.parametrize("rate", NOT_EDGE)
def test_tracking_11_taps(pkg, ctx, rate):
    """The ACF taps -0.5:0.1:0.5 (at the low rates up to ten tap boundaries fall into one
    8-sample lane), records as compare and the tap array within 1e-10 of its RMS."""
    r = rm.oracle_tracking(rate, 11)
    assert r.status == 0
    g, launches = _track(pkg, ctx, rate, 11)
    err = _pel_error(g, r)
    terr = 0.0
    for c in range(3):
        n = int(r.len[c])
        scale = np.sqrt(np.mean(r.taps[c, :, :, :n] ** 2))
        terr = max(terr, float(np.max(np.abs(g.taps[c, :, :, :n] - r.taps[c, :, :, :n])) / scale))
    REPORT[("b.track", rate, "11 taps")] = (f"worst P/E/L error / RMS {err:.3e}; tap array {terr:.3e}; "
                                            f"{launches} launches; {_geom(rate)}")
    print(rate, "11 taps: worst P/E/L", err, "taps", terr, "launches", launches)
    compare_trk(pkg, g, r)
    assert terr < 1e-10
    for c in range(3):
        n = int(r.len[c])
        assert np.array_equal(g.rec[c, 0, :n], g.taps[c, 0, 5, :n])
        assert np.array_equal(g.rec[c, 2, :n], g.taps[c, 0, 0, :n])
        assert np.array_equal(g.rec[c, 5, :n], g.taps[c, 1, 10, :n])


# ---- c. formats off the grid ------------------------------------------------------------------
@pytest.mark.parametrize("prec,dtyp", [(2, 2), (1, 1)], ids=["int16-iq", "int8-real"])
def test_tracking_formats_16m(pkg, ctx, prec, dtyp):
    """int16 I/Q (per-read mean removal from the group prefix sums) and int8 real at
    16.3676 MHz, where Fs * ms is no integer, as test_gpu_formats.test_tracking_formats."""
    rate = "l1_16m"
    r = rm.oracle_tracking(rate, 3, prec, dtyp)
    assert r.status == 0
    g, launches = _track(pkg, ctx, rate, 3, prec, dtyp)
    err = _pel_error(g, r)
    REPORT[("c.format", rate, f"prec {prec} type {dtyp}")] = f"worst P/E/L error / RMS {err:.3e}; {launches} launches"
    print(rate, prec, dtyp, "worst P/E/L", err)
    compare_trk(pkg, g, r)
    F = pkg.abi.FIELDS
    pos = g.rec[0, F.index("absoluteSample"), :rm.N1]
    ns = g.rec[0, F.index("numSample"), :rm.N1]
    assert np.array_equal(np.diff(pos), ns[1:] * prec * dtyp)


# ---- d. acquisition through rocFFT, unforced --------------------------------------------------
@pytest.mark.parametrize("rate", rm.ACQ_RATES)
def test_acquisition_rocfft_unforced(pkg, ctx, precision, rate):  # noqa: F811
    """Sample = 16368 / 12500 / 10000 are not the two sizes of the own FFT, so the engine takes
    rocFFT by itself (16368 = 2^4 * 3 * 11 * 31; the fine transform is L * Sample * datalen
    points). +-3 kHz / 500 Hz, datalen 10, L 10, PRNs 5, 9 (absent), 13, 20."""
    r, rd = rm.oracle_acquisition(rate)
    g, gd = pkg.acquisition(rm.file_of(rate), rm.signal_of(rate), rm.acq_params(), ctx=ctx, prn_list=rm.ACQ_PRNS,
                            diag=True)
    dsnr = float(np.max(np.abs(gd.SNR - rd.SNR))) if len(gd.SNR) == len(rd.SNR) else float("nan")
    acq_mask = np.isin(gd.prn, g.sv)
    margin = (gd.peak - gd.peak2) / gd.peak
    gate = np.abs(gd.SNR - 12.0)
    REPORT[("d.acq", rate, precision)] = (f"worst |SNR difference| {dsnr:.3e} dB; min peak margin "
                                          f"{float(margin[acq_mask].min()) if acq_mask.any() else float('nan'):.4f}; "
                                          f"min |SNR - 12| {float(gate.min()):.3f} dB")
    print(rate, precision, "SNR diff", dsnr, "margins", margin, "gate", gate)
    compare_acq(g, gd, r, rd, precision)
    assert list(g.sv) == rm.PRNS
    assert margin[acq_mask].min() > 1e-4
    assert gate.min() > 0.01


# ---- e. the floor -----------------------------------------------------------------------------
def test_rate_below_the_floor_is_an_argument_error(pkg, ctx):
    """Fs = 8 MHz (8 * fc / Fs = 1.023: an 8-sample lane would hold more than one chip
    boundary): trackingCT and correlate_step refuse it on the host with GNSS_EARG and a text
    naming the sampling-rate floor -- not GNSS_EINDEX from a kernel, which the header keeps for
    indices MATLAB would reject -- and the context stays usable: a 26 MHz call passes after."""
    sdr = _sdr()
    Fs, IF = rm.FLOOR
    S = rm.sample_of(Fs)
    data = np.zeros(2 * S * 60, dtype=np.int8)
    file = SimpleNamespace(skip=0, dataType=2, dataPrecision=1, data=data, fileRoute=None, dev=None)
    signal = rm.signal_of(rm.FLOOR)
    track = pkg.initParameters()[3]
    track.msToProcessCT_1ms, track.msToProcessCT_10ms = 30, 0
    A = SimpleNamespace(sv=np.array([5]), SNR=np.array([20.0]), Doppler=np.zeros(1), codedelay=np.array([100]),
                        fineFreq=np.array([IF]))
    with pytest.raises(pkg.abi.GnssError) as e:
        pkg.trackingCT(file, signal, track, A, ctx=ctx)
    assert e.value.status == pkg.abi.EARG
    assert "sampling-rate floor" in str(e.value), str(e.value)
    with pytest.raises(pkg.abi.GnssError) as e:
        sdr.correlate_step(file, signal, 5, 1, 0.0, rm.FC, IF, 0.0, 0, np.array([-0.5, 0.0, 0.5]), ctx=ctx)
    assert e.value.status == pkg.abi.EARG
    assert "sampling-rate floor" in str(e.value), str(e.value)
    # a code frequency of the caller's that no 8-sample lane can take, at an admitted rate
    with pytest.raises(pkg.abi.GnssError) as e:
        sdr.correlate_step(rm.file_of("edge_8m5"), rm.signal_of("edge_8m5"), 5, 1, 0.0, 8.5e6 / 8, 2.0e6, 0.0, 0,
                           np.array([-0.5, 0.0, 0.5]), ctx=ctx)
    assert e.value.status == pkg.abi.EARG
    # the context is still usable
    case, r = rm.step_cases("urban26")[0], rm.oracle_steps("urban26")[0]
    g, ns = sdr.correlate_step(rm.file_of("urban26"), rm.signal_of("urban26"), case.prn, case.pdi, case.remChip,
                               case.codeFreq, case.carrierFreq, case.remPhase, case.pos_bytes, rm.case_taps(case),
                               ctx=ctx)
    assert ns == case.n and np.max(np.abs(g - r)) / np.sqrt(np.mean(r ** 2)) < 1e-12


# ---- f. vector tracking at 26 MHz, zero IF ----------------------------------------------------
def test_vt_run_urban26(pkg, po, ctx):
    """gnss_tracking_vt_run, 3 channels x 200 steps in one launch at Fs = 26 MHz, IF = 0 (the
    negative carrFreq of PRNs 5 and 20 through vt.hip's own phase reduction), the code
    frequency cycling over 1.023e6 + {0, 20, -20, 3.25, -7.5} Hz, against or_vt_step."""
    rate = "urban26"
    Fs, IF = rm.RATES[rate]
    S = rm.sample_of(Fs)
    _, cds = rm.scene(rate)
    file, signal = rm.file_of(rate), rm.signal_of(rate)
    track = rm.track_params()
    ffs = [IF + d for d in rm.DOPPLERS]
    chans = [pkg.vt_channel(p, (S - cd + 1 + rm.SKIP * S) * 2, 0.0, 0.0, rm.FC, f, f)
             for p, cd, f in zip(rm.PRNS, cds, ffs)]
    st = [po.vt_state(c.file_ptr, 0.0, 0.0, rm.FC, c.carrFreq, c.carrFreqBasis) for c in chans]
    nsteps = 200
    cyc = rm.FC + np.array([0.0, 20.0, -20.0, 3.25, -7.5])
    series = np.ascontiguousarray(np.tile(cyc[np.arange(nsteps) % 5][:, None], (1, 3)))
    out = pkg.trackingVT_run(file, signal, track, chans, series, ctx=ctx)
    assert ctx.timing()["track_launches"] == 1
    assert (out["status"] == 0).all()
    iq = rm.record(rate)
    worst = [0.0]
    neg = 0
    for k in range(nsteps):
        for i, prn in enumerate(rm.PRNS):
            status, rec = po.vt_step(st[i], series[k, i], prn, iq=iq, Fs=Fs)
            assert status == 0
            R = dict(zip(po.VT_REC, rec))
            neg += prn == 5 and R["carrFreq"] < 0
            check_vt({f: out[f][k, i] for f in out}, R, k, prn, worst)
    REPORT[("f.vt", rate, "run 200 steps")] = f"worst sum error / |P| {worst[0]:.3e}"
    print(rate, "VT worst sum error / |P|", worst[0])
    assert neg == nsteps  # PRN 5 (-2310 Hz) stays on the negative side throughout
    assert worst[0] < 1e-9
