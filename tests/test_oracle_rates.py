"""The reference side of the sampling-rate matrix (tests/rate_matrix.py), on the CPU: the C
oracle against the independent numpy twin for single correlation steps at every rate, and the
oracle's closed-loop trackingCT per rate with the preconditions the GPU tests (test_gpu_rates)
rely on: at IF = 0 the carrier of PRN 5 is negative throughout with remPhase in (-2*pi, 0], and
at 12.5 MHz PRN 20's carrier takes both signs, so a GPU run that matches these records has run
the negative side of the kernels' phase reduction and a sign change inside a run."""
import numpy as np
import pytest

import numpy_twin as tw
import rate_matrix as rm


@pytest.mark.parametrize("rate", list(rm.RATES))
def test_correlate_step_twin_per_rate(po, rate):
    """trackingCT.m:96-118 for one step: oracle vs twin within 1e-12 of the RMS (this suite's
    bound for the pair, test_oracle_numpy_twin). 10-ms steps of the twin (a Python fsum over
    Sample * 10 products per tap) are checked on a fixed random 30 % of the cases to bound the
    time; the 1-ms cases all run."""
    Fs = rm.RATES[rate][0]
    worst = 0.0
    cases = rm.step_cases(rate)
    keep10 = np.random.default_rng(5).random(len(cases)) < 0.3
    for k, (case, got) in enumerate(zip(cases, rm.oracle_steps(rate))):
        if case.pdi == 10 and not keep10[k]:
            continue
        iq = rm.record(rate)[case.pos_bytes: case.pos_bytes + 2 * case.n]
        ref = tw.correlate_step(iq, case.n, case.remChip, case.codeFreq, Fs, case.carrierFreq, case.remPhase,
                                po.generate_ca(case.prn), rm.case_taps(case))
        err = np.max(np.abs(got - ref)) / np.sqrt(np.mean(ref ** 2))
        worst = max(worst, err)
        assert err < 1e-12, (case, err)
    print(rate, "oracle vs twin, worst / RMS", worst)


def test_step_cases_cover_the_named_points():
    """The case list holds what the matrix promises: both pdi, both tap sets, a carrier of
    exactly 0 at the IF = 0 rates, f/Fs = 0.42 at 10 MHz, negative phases, and early / late
    samples on exact chip boundaries (remChip = 0 and -0.5 * fc / Fs at the nominal code rate)."""
    for rate, (Fs, IF) in rm.RATES.items():
        cs = rm.step_cases(rate)
        assert {c.pdi for c in cs} == {1, 10} and {c.ntaps for c in cs} == {3, 11}
        assert any(c.remPhase < 0 for c in cs) and any(c.remPhase == 0 for c in cs)
        assert {c.remChip for c in cs} == {0.0, 0.009, -0.009, -0.5 * rm.FC / Fs}
        assert (0.0 in {c.carrierFreq for c in cs}) == (IF == 0.0)
        assert all(c.pos_bytes % 2 == 0 and c.pos_bytes + 2 * c.n <= len(rm.record(rate)) for c in cs)
    # a numSample tie: 26000.5 rounds away from zero (MATLAB's round), not to even
    assert rm.num_sample(1, -0.5 * rm.FC / 26e6, rm.FC, 26e6) == 26001
    assert rm.F_EXTRA / 10e6 > 0.42 and any(c.carrierFreq == rm.F_EXTRA for c in rm.step_cases("low_10m"))


@pytest.mark.parametrize("rate", list(rm.RATES))
def test_oracle_tracking_per_rate(pkg, rate):
    """700 x 1 ms + 60 ms at 10 ms, three channels: the oracle tracks every one (status 0, the
    full series length), and the carrier takes the signs the GPU tests need."""
    r = rm.oracle_tracking(rate)
    assert r.status == 0
    assert np.array_equal(r.len, rm.N1 + r.countinx + rm.N10)
    assert np.all((r.countinx >= 0) & (r.countinx <= 18))
    F = pkg.abi.FIELDS
    A = rm.acquired_for(rate)
    assert list(A.sv) == rm.PRNS
    if rate in rm.ZERO_IF:
        n = int(r.len[0])
        cf = r.rec[0, F.index("carrierFreq"), :n]
        ph = r.rec[0, F.index("remPhase"), :n]
        assert np.all(cf < 0), (cf.min(), cf.max())
        assert np.all(ph <= 0) and np.all(ph > -2 * np.pi) and np.any(ph < 0)
    if rate == "zero_12m5":
        n = int(r.len[2])
        cf = r.rec[2, F.index("carrierFreq"), :n]
        assert cf.min() < 0 < cf.max(), (cf.min(), cf.max())


@pytest.mark.parametrize("rate", rm.ACQ_RATES)
def test_oracle_acquisition_per_rate(rate):
    """datalen 10: exactly the three present PRNs, every SNR clear of the 12 dB gate and every
    acquired peak clear of the off-window value (the margins test_gpu_rates asserts on the GPU)."""
    A, d = rm.oracle_acquisition(rate)
    assert list(A.sv) == rm.PRNS
    assert list(d.prn) == rm.ACQ_PRNS
    assert np.abs(d.SNR - 12.0).min() > 0.01
    m = np.isin(d.prn, A.sv)
    assert ((d.peak - d.peak2) / d.peak)[m].min() > 1e-4


@pytest.mark.parametrize("prec,dtyp", [(2, 2), (1, 1)], ids=["int16-iq", "int8-real"])
def test_oracle_tracking_formats_16m(prec, dtyp):
    r = rm.oracle_tracking("l1_16m", 3, prec, dtyp)
    assert r.status == 0
    assert np.array_equal(r.len, rm.N1 + r.countinx + rm.N10)


def test_lane_geometry_of_the_matrix():
    """What the rates were chosen for, from the engine's rule (8 * SUB * 1.1 * fc / Fs < 1)."""
    assert rm.tracking_subs(58e6) == [1, 2, 3, 4] and rm.lane_geometry(58e6, 10) == (3, 96)
    assert rm.lane_geometry(58e6, 1) == (1, 29)
    assert rm.tracking_subs(26e6) == [1, 2] and rm.step_subs(26e6) == [1, 2, 3]
    assert rm.tracking_subs(10e6) == [1] and rm.lane_geometry(10e6, 1) == (1, 5)
    assert rm.tracking_subs(8.5e6) == [] and rm.lane_geometry(8.5e6, 10)[0] == 1
    assert 8 * 1.01 * rm.FC / 8.5e6 < 1 < 8 * 1.01 * rm.FC / rm.FLOOR[0]
