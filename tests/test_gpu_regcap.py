"""The <= 3-tap correlators' register capture against the LDS-slot path it replaces
(GNSS_OPT_SLOT_PATH 1 forces the slots, 2 the registers): every record field and every sum bit
for bit, and the existing comparisons against the CPU oracle with their bounds unchanged
(test_gpu_tracking.compare, test_gpu_pos.compare_pos; a single step within 1e-12 of the RMS
as test_gpu_rates.test_correlate_step_rates).

The engine's choice is checked through gnss_ctx_lane_path against gnss_lane_boundaries, the
host predicate (tests/test_lane_boundaries.py pins that one on the CPU): registers where a
lane holds at most 2 distinct boundary samples, one of them the rounding allowance, i.e. one
boundary set. With two or three real boundaries in a lane (+-0.25 and +-0.1 chip, the low
rates) the engine keeps the slots; forcing the registers there makes nearly every wave take
the rolled second pass of the capture, in the persistent loop and in the step kernel, which
is how these tests cover it."""
import importlib

import numpy as np
import pytest

import rate_matrix as rm
from conftest import acquired_of, params
from test_gpu_pos import compare_pos
from test_gpu_tracking import compare as compare_trk

pytestmark = pytest.mark.gpu

N1, N10 = 60, 200
SVS, CDS, FFS = [16, 26], [26051, 57908], [4579675.0, 4581800.0]
EPL = [-0.5, 0.0, 0.5]
FS = 58e6


def _sdr():
    return importlib.import_module("assignment-for-aae6102_gnss-sdr_amd.sdr")


def predicted(pkg, taps, samples, cps, post=None):
    import ctypes as C
    n = len(taps)
    a = (C.c_double * n)(*taps)
    p = (C.c_double * n)(*post) if post is not None else None
    return pkg.abi.load().gnss_lane_boundaries(a, p, n, samples, cps)


def same_bits(p, q):
    assert np.array_equal(p.len, q.len) and np.array_equal(p.countinx, q.countinx)
    assert p.rec.tobytes() == q.rec.tobytes()
    assert p.CN0.tobytes() == q.CN0.tobytes()


@pytest.fixture(scope="module")
def reference(pkg, po, opensky_short):
    """reference(half): the oracle's trackingCT of the two channels with E/L at -+half chip
    (N1 + N10 ms), computed once per spacing for the whole module."""
    done = {}

    def get(half=0.5):
        if half not in done:
            file, signal, track, A = tracking_inputs(pkg, opensky_short, half)
            r = po.trackingCT(file, signal, track, A, taps=taps_of(half), raw=True)
            for a in (r.rec, r.len, r.countinx, r.CN0):
                a.setflags(write=False)
            done[half] = r
        return done[half]

    return get


def taps_of(half):
    return None if half == 0.5 else np.array([-half, 0.0, half])


def tracking_inputs(pkg, opensky_short, half=0.5):
    skip, cfg, data = opensky_short
    file, signal, acq, track = params(pkg, skip, data)
    track.msToProcessCT_1ms, track.msToProcessCT_10ms = N1, N10
    track.CorrelatorSpacing = half
    return file, signal, track, acquired_of(SVS, CDS, FFS)


# ---- a. standard E/P/L, every lane span, both paths ---------------------------------------------
@pytest.mark.parametrize("persist", [True, False], ids=["persistent", "step"])
@pytest.mark.parametrize("sub", [1, 2, 3, 4])
def test_epl_register_equals_slot(pkg, ctx, opensky_short, reference, opts, sub, persist):
    file, signal, track, A = tracking_inputs(pkg, opensky_short)
    opts(pkg.abi.OPT_FORCE_SUB, sub)
    if not persist:
        opts(pkg.abi.OPT_NO_PERSIST, 1)
    g = pkg.trackingCT(file, signal, track, A, ctx=ctx, raw=True)
    # 24-sample lanes cannot hold the E/L boundary and the prompt's (28.3 samples on); 32 can
    want = predicted(pkg, EPL, 8 * sub, 1.1 * rm.FC / FS) <= 2
    assert want == (sub <= 3)
    assert ctx.lane_path() == int(want)
    opts(pkg.abi.OPT_SLOT_PATH, 1)
    s = pkg.trackingCT(file, signal, track, A, ctx=ctx, raw=True)
    assert ctx.lane_path() == 0
    same_bits(g, s)
    r = reference()
    assert r.status == 0
    compare_trk(pkg, g, r)


# ---- b. tap sets with two and three boundaries in a lane, closed loop -------------------------
BOUNDARIES = {0.25: [2, 3, 3], 0.1: [3, 4, 4]}  # gnss_lane_boundaries at 8-, 16-, 24-sample lanes, 58 MHz


@pytest.mark.parametrize("persist", [True, False], ids=["persistent", "step"])
@pytest.mark.parametrize("sub", [1, 2, 3])
@pytest.mark.parametrize("half", [0.25, 0.1], ids=["quarter", "tenth"])
def test_custom_taps_tracking(pkg, ctx, opensky_short, reference, opts, half, sub, persist):
    """trackingCT with E/L at -+0.25 and -+0.1 chip: the engine's own choice, the forced slots
    and the forced registers (where the lanes' second and third boundaries go through the rolled
    second pass) give the same bits in every record field, and pass compare against the oracle."""
    file, signal, track, A = tracking_inputs(pkg, opensky_short, half)
    taps = taps_of(half)
    opts(pkg.abi.OPT_FORCE_SUB, sub)
    if not persist:
        opts(pkg.abi.OPT_NO_PERSIST, 1)
    want = BOUNDARIES[half][sub - 1]
    assert predicted(pkg, list(taps), 8 * sub, 1.1 * rm.FC / FS) == want
    g = pkg.trackingCT(file, signal, track, A, ctx=ctx, taps=taps, raw=True)
    assert ctx.lane_path() == int(want <= 2)
    launches = ctx.timing()["track_launches"]
    if not persist:
        assert launches > 60
    elif sub >= 2:  # (8-sample lanes: the 10-ms step has more blocks than the loop keeps resident)
        assert launches <= 4
    opts(pkg.abi.OPT_SLOT_PATH, 1)
    s = pkg.trackingCT(file, signal, track, A, ctx=ctx, taps=taps, raw=True)
    assert ctx.lane_path() == 0
    opts(pkg.abi.OPT_SLOT_PATH, 2)
    q = pkg.trackingCT(file, signal, track, A, ctx=ctx, taps=taps, raw=True)
    assert ctx.lane_path() == 1
    same_bits(g, s)
    same_bits(q, s)
    r = reference(half)
    assert r.status == 0
    compare_trk(pkg, q, r)


# ---- b'. the same tap sets with two and three boundaries in a lane: single steps, random states ----------
@pytest.mark.parametrize("sub", [1, 2, 3])
@pytest.mark.parametrize("half", [0.25, 0.1], ids=["quarter", "tenth"])
def test_custom_taps_steps(pkg, po, ctx, opensky_short, opts, half, sub):
    skip, cfg, data = opensky_short
    file, signal, acq, track = params(pkg, skip, data)
    taps = np.array([-half, 0.0, half])
    sdr = _sdr()
    opts(pkg.abi.OPT_FORCE_SUB, sub)
    rng = np.random.default_rng(int(half * 100) * 10 + sub)
    ca = {prn: po.generate_ca(prn) for prn in SVS}
    expect = BOUNDARIES[half][sub - 1]
    for k in range(6):
        pdi = (1, 10)[k % 2]
        prn = SVS[k % 2]
        remChip = float(rng.uniform(-0.5, 0.5)) if k else 0.0
        codeFreq = rm.FC + float(rng.uniform(-4.0, 4.0))
        carrier = FFS[k % 2] + float(rng.uniform(-50.0, 50.0))
        phase = float(rng.uniform(-2 * np.pi, 2 * np.pi))
        n = rm.num_sample(pdi, remChip, codeFreq, FS)
        pos = 2 * int(rng.integers(0, len(data) // 2 - n - 8))
        assert predicted(pkg, list(taps), 8 * sub, codeFreq / FS) == expect
        opts(pkg.abi.OPT_SLOT_PATH, 0)
        g, ns = sdr.correlate_step(file, signal, prn, pdi, remChip, codeFreq, carrier, phase, pos, taps, ctx=ctx)
        assert ctx.lane_path() == int(expect <= 2)
        opts(pkg.abi.OPT_SLOT_PATH, 1)
        s, ns_s = sdr.correlate_step(file, signal, prn, pdi, remChip, codeFreq, carrier, phase, pos, taps, ctx=ctx)
        assert ctx.lane_path() == 0
        opts(pkg.abi.OPT_SLOT_PATH, 2)
        q, ns_q = sdr.correlate_step(file, signal, prn, pdi, remChip, codeFreq, carrier, phase, pos, taps, ctx=ctx)
        assert ctx.lane_path() == 1
        assert ns == ns_s == ns_q == n
        assert g.tobytes() == s.tobytes() == q.tobytes(), (k, g, s, q)
        r = po.correlate_step(data[pos: pos + 2 * n], n, remChip, codeFreq, FS, carrier, phase, ca[prn], pdi, taps)
        err = float(np.max(np.abs(g - r)) / np.sqrt(np.mean(r ** 2)))
        print(half, sub, k, "step error / RMS", err)
        assert err < 1e-12, (k, err)


# ---- c. low sampling rates: a chip is 8.3 / 12.2 samples --------------------------------------
@pytest.mark.parametrize("persist", [True, False], ids=["persistent", "step"])
@pytest.mark.parametrize("rate", ["edge_8m5", "zero_12m5"])
def test_low_rates(pkg, ctx, opts, rate, persist):
    if not persist:
        opts(pkg.abi.OPT_NO_PERSIST, 1)
    args = (rm.file_of(rate), rm.signal_of(rate), rm.track_params(), rm.acquired_for(rate))
    g = pkg.trackingCT(*args, ctx=ctx, raw=True)
    Fs = rm.RATES[rate][0]
    want = all(predicted(pkg, EPL, 8 * rm.lane_geometry(Fs, pdi)[0], 1.1 * rm.FC / Fs) <= 2 for pdi in (1, 10))
    assert not want  # (E/L and the prompt's boundary both fit the lane: the slots stay)
    assert ctx.lane_path() == int(want)
    opts(pkg.abi.OPT_SLOT_PATH, 2)  # the registers all the same: the second boundary by the rolled pass
    q = pkg.trackingCT(*args, ctx=ctx, raw=True)
    assert ctx.lane_path() == 1
    same_bits(g, q)
    r = rm.oracle_tracking(rate)
    assert r.status == 0
    compare_trk(pkg, g, r)


@pytest.mark.parametrize("rate", ["edge_8m5", "zero_12m5"])
def test_low_rate_steps_through_the_registers(pkg, po, ctx, opts, rate):
    """At these rates the engine keeps the slots for E/P/L, so the register form is also run
    where the engine itself admits it: the late tap twice, so all three boundaries are one set (E and L are
    a whole chip apart), 8-sample lanes."""
    sdr = _sdr()
    Fs = rm.RATES[rate][0]
    taps = np.array([-0.5, 0.5, 0.5])
    file, signal = rm.file_of(rate), rm.signal_of(rate)
    for case in rm.step_cases(rate)[:40:5]:
        assert predicted(pkg, list(taps), 8, case.codeFreq / Fs) == 2
        opts(pkg.abi.OPT_SLOT_PATH, 0)
        g, ns = sdr.correlate_step(file, signal, case.prn, case.pdi, case.remChip, case.codeFreq, case.carrierFreq,
                                   case.remPhase, case.pos_bytes, taps, ctx=ctx)
        assert ctx.lane_path() == 1
        opts(pkg.abi.OPT_SLOT_PATH, 1)
        s, _ = sdr.correlate_step(file, signal, case.prn, case.pdi, case.remChip, case.codeFreq, case.carrierFreq,
                                  case.remPhase, case.pos_bytes, taps, ctx=ctx)
        assert g.tobytes() == s.tobytes()
        iq = rm.record(rate)[case.pos_bytes: case.pos_bytes + 2 * case.n]
        r = po.correlate_step(iq, case.n, case.remChip, case.codeFreq, Fs, case.carrierFreq, case.remPhase,
                              po.generate_ca(case.prn), case.pdi, taps)
        assert ns == case.n and np.max(np.abs(g - r)) / np.sqrt(np.mean(r ** 2)) < 1e-12


# ---- d. the POS loop's prompt offset (+0.05 chip) ---------------------------------------------
@pytest.mark.parametrize("persist", [True, False], ids=["persistent", "step"])
def test_pos_prompt_offset(pkg, po, ctx, opensky_short, opts, persist):
    if not persist:
        opts(pkg.abi.OPT_NO_PERSIST, 1)
    skip, cfg, data = opensky_short
    file, signal, acq, track = params(pkg, skip, data)
    track.msToProcessCT_1ms, track.ctPOS = N1, N1 + N10 // 10
    A = acquired_of(SVS, CDS, FFS)
    cx = [7, -1]
    g = pkg.trackingCT_POS(file, signal, track, A, cx, ctx=ctx, raw=True)
    assert ctx.lane_path() == 1
    opts(pkg.abi.OPT_SLOT_PATH, 1)
    s = pkg.trackingCT_POS(file, signal, track, A, cx, ctx=ctx, raw=True)
    assert ctx.lane_path() == 0
    same_bits(g, s)
    r = po.trackingCT_POS(file, signal, track, A, cx, raw=True)
    assert r.status == 0
    compare_pos(pkg, g, r)


# ---- e. int16 I/Q records (the per-step kernels' FMT 1 forms) -----------------------------------
def test_int16_register_equals_slot(pkg, ctx, opts):
    """16.3676 MHz, int16 I/Q with the per-read mean removed: 8-sample lanes hold one boundary
    set (E/L to the prompt is 8 samples), so the engine takes the registers by itself."""
    rate = "l1_16m"
    args = (rm.file_of(rate, 2, 2), rm.signal_of(rate), rm.track_params(), rm.acquired_for(rate))
    g = pkg.trackingCT(*args, ctx=ctx, raw=True)
    assert ctx.lane_path() == 1
    opts(pkg.abi.OPT_SLOT_PATH, 1)
    s = pkg.trackingCT(*args, ctx=ctx, raw=True)
    assert ctx.lane_path() == 0
    same_bits(g, s)
    r = rm.oracle_tracking(rate, 3, 2, 2)
    assert r.status == 0
    compare_trk(pkg, g, r)


def test_slot_path_option_values(pkg, ctx):
    assert ctx.lib.gnss_ctx_set_option(ctx.h, pkg.abi.OPT_SLOT_PATH, 3) == pkg.abi.EARG
    assert ctx.lib.gnss_ctx_set_option(ctx.h, pkg.abi.OPT_SLOT_PATH, -1) == pkg.abi.EARG
    assert ctx.lib.gnss_ctx_set_option(ctx.h, pkg.abi.OPT_SLOT_PATH, 0) == 0
