"""GPU tests of the positioning pass on device-resident records (gnss_ct_pos_solve with
GNSS_OUT_DEVICE, csrc/ctpos.hip): the measurement table extracted by the kernels equals the
host's bit for bit -- on the reference's recorded run and on every schedule-stress case -- and
with it the whole solution; the host mirror's trackingCT_POS_updated end to end on a synthetic
record, its hand-over to the vector-tracking loop, and the kernels' bound check."""
from types import SimpleNamespace as NS

import numpy as np
import pytest

import ctpos_common as K
import ctpos_twin as T
from conftest import acquired_of, params
from test_ctpos_kat import fitted_within

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    return T.fixture()


@pytest.mark.parametrize("name", ["fixture", "early", "window", "period4", "period5", "mc_pdi1", "mc_pdi10", "four",
                                  "big", "zero"])
def test_device_extraction_equals_host(po, pkg, ctx, z, name):
    """The records uploaded as device records: Index, index, codePhaseMeas, carrFreq(Index) and
    rows equal the host extraction's, and so does every field of the solution."""
    case = K.cases(z)[name]
    h = K.lib_run(po, pkg, z, case)
    d = K.lib_run(po, pkg, z, case, records=K.device_records(pkg, z, case), ctx=ctx)
    K.assert_same_solution(h, d)
    rows = len(d.localTime)
    if name == "fixture":
        assert rows == 660 and np.array_equal(d.codePhaseMeas, z["sol_codePhaseMeas"])
    if name == "big":  # the prefix-max crosses waves and the block's 1024-wide chunks
        assert rows == 1320 and np.all(np.diff(d.Index) == 1)
    if name == "zero":
        assert rows == 0
    if name in ("period4", "period5"):
        assert np.all(np.diff(d.Index) == 1)


def test_device_errors_follow_the_host(po, pkg, ctx, z):
    abi = pkg.abi
    full = K.cases(z)["fixture"]
    case = dict(full, start=int(z["rec_absoluteSample"][:, 0].min()))  # index = 0: MATLAB raises
    with pytest.raises(abi.GnssError) as e:
        K.lib_run(po, pkg, z, case, records=K.device_records(pkg, z, case), ctx=ctx)
    assert e.value.status == abi.EINDEX
    case = dict(full, sel=[0, 1, 2])
    with pytest.raises(abi.GnssError) as e:
        K.lib_run(po, pkg, z, case, records=K.device_records(pkg, z, case), ctx=ctx)
    assert e.value.status == abi.EARG
    with pytest.raises(abi.GnssError) as e:  # 1e30-m pseudoranges: the capped olspos
        K.lib_run(po, pkg, z, full, records=K.device_records(pkg, z, full), ctx=ctx, cSpeed=1e31)
    assert e.value.status == abi.ENOCONV
    small = dict(full, hi=1800)  # the next call on the context succeeds
    assert len(K.lib_run(po, pkg, z, small, records=K.device_records(pkg, z, small), ctx=ctx).localTime) == 60


def test_len_below_the_last_index_gives_an_empty_tail(po, pkg, ctx, z):
    """len shortened through the public argument: the pass runs over min(len) steps, so the epochs
    whose step lies beyond it are simply not reached (part 1's rule), on the device as on the host;
    no record index leaves the series, no fault, and the context stays usable."""
    full = K.cases(z)["fixture"]
    whole = K.lib_run(po, pkg, z, full)
    for cut in (1700, 1681, 1680, 1, 0):
        dev, host = K.device_records(pkg, z, full), K.host_records(pkg, z, full)
        dev.len[2] = host.len[2] = cut  # one channel's len: the minimum counts
        d = K.lib_run(po, pkg, z, full, records=dev, ctx=ctx)
        h = K.lib_run(po, pkg, z, full, records=host)
        K.assert_same_solution(h, d)
        want = int(np.sum(whole.Index <= cut))
        assert len(d.localTime) == want
        assert np.array_equal(d.usrPos, whole.usrPos[:want])
    d = K.lib_run(po, pkg, z, full, records=K.device_records(pkg, z, full), ctx=ctx)
    K.assert_same_solution(whole, d)


# ---- end to end on the synthetic 3-s Opensky record -------------------------------------------
SVS = [3, 16, 22, 26, 31]  # the fixture's PRNs: its ephemerides serve
CD = [3684, 26051, 2611, 57908, 39064]
FF = [4580975.0, 4579675.0, 4581525.0, 4581800.0, 4581025.0]
CX = [12, 12, 3, 13, 5]
NAV1 = [13, 4, 14, 6, 10]
MS1_E2E, CTPOS = 240, 300
TOW0 = 390114.0


def e2e_inputs(pkg, po, z, opensky_short):
    skip, cfg, data = opensky_short
    file, signal, acq, track = params(pkg, skip, data)
    _, _, _, _, solu, cmn = pkg.initParameters()
    file.skiptimeVT = 100
    track.msToProcessCT_1ms, track.ctPOS, track.pdi = MS1_E2E, CTPOS, 1
    A = acquired_of(SVS, CD, FF)
    eph = {p: NS(sfb=[1], TOW=[TOW0], updateflag=1,
                 **{f: [z["eph"][i, j]] for j, f in enumerate(pkg.abi.EPH_SV_FIELDS)}) for i, p in enumerate(SVS)}
    nav1 = np.zeros(32)
    nav1[np.array(SVS) - 1] = NAV1
    # TckResult_Eph(prn).absoluteSample on the scalar loop's own grid (one code period per entry)
    S = signal.Sample
    eph_rec = {p: NS(absoluteSample=(skip * S + S - cd + 1 + S * np.arange(1, 61)) * 2.0) for p, cd in zip(SVS, CD)}
    return file, signal, track, cmn, solu, A, eph, NS(nav1=nav1), eph_rec


def twin_args(po, pkg, z, tck, signal, solu, TOW1, start):
    g = lambda f: np.stack([np.asarray(getattr(tck(p), f), dtype=np.float64) for p in SVS])
    return dict(absoluteSample=g("absoluteSample"), remChip=g("remChip"), codeFreq=g("codeFreq"),
                carrFreq=g("carrFreq"), countinx=np.array(CX), nav1=np.array(NAV1), sfb1=np.ones(5, dtype=np.int64),
                TOW1=np.asarray(TOW1, dtype=np.float64), eph=z["eph"], sampleStartMea=start, Fs=signal.Fs,
                IF=signal.IF, codelength=signal.codelength, dataType=2, navSolPeriod=solu.navSolPeriod,
                ms1=MS1_E2E, cnslxyz=K.cnslxyz(po, pkg), ALPHA=pkg.sdr.ALPHA, BETA=pkg.sdr.BETA, doy=171,
                cSpeed=299792458.0)


def twin_on(po, pkg, z, tck, signal, solu, TOW1, start):
    """The twin on given records; raises past 10 olspos iterations at any epoch."""
    return T.solve(po, max_iter=10, **twin_args(po, pkg, z, tck, signal, solu, TOW1, start))


def consistent_tow(po, pkg, z, tt0):
    """Each PRN's TOW so that the first epoch's transmit times put the receiver at cnslxyz: the
    transmit time t with (Trx - t) * c = the range from the satellite at t, its clock and group
    delay applied as the loop applies them (:483-486), for one reception time Trx."""
    c, usr = 299792458.0, K.cnslxyz(po, pkg)
    Trx = TOW0 + 0.075
    tow = []
    for s in range(5):
        t = Trx - 0.07
        for _ in range(6):
            pos, _, clkm, _, grp = po.svposvel(z["eph"][s], t)
            rho = np.linalg.norm(po.geo("erotcorr", pos, c * (Trx - t)) - usr)
            t = Trx - (rho - clkm + grp * c) / c
        tow.append(TOW0 + (t - tt0[s]))
    return tow


def test_end_to_end_and_hand_over(po, pkg, ctx, z, opensky_short):
    file, signal, track, cmn, solu, A, eph, sbf, eph_rec = e2e_inputs(pkg, po, z, opensky_short)
    start = int(max(eph_rec[p].absoluteSample[n1 + 20 - 1] for p, n1 in zip(SVS, NAV1))) + 1
    # on the CPU oracle's records, before anything touches the GPU: the inputs behave
    r = po.trackingCT_POS(file, signal, track, A, CX, raw=True)
    assert r.status == 0
    otck = pkg.sdr.build_tck_result(A, r, None, pkg.abi.FIELDS_POS)
    tt0 = T.first_transmit_time(**twin_args(po, pkg, z, otck, signal, solu, [TOW0] * 5, start))
    tow = consistent_tow(po, pkg, z, tt0)
    for p, w in zip(SVS, tow):
        eph[p].TOW = [w]
    t0 = twin_on(po, pkg, z, otck, signal, solu, tow, start)
    assert t0.rows > 30 and t0.iters.max() <= 10
    assert np.linalg.norm(t0.usrPosENU[0]) < 100  # the first fix sits at cnslxyz
    assert np.sum(t0.Index <= MS1_E2E + min(CX)) > 10  # epochs on both sides of the switch

    cns = K.cnslxyz(po, pkg)
    run = lambda dev: pkg.trackingCT_POS_updated(file, signal, track, cmn, A, eph_rec, cns, eph, sbf, solu,
                                                 countinx=CX, ctx=ctx, device_records=dev)
    tck_h, nav_h = run(False)
    tck_d, nav_d = run(True)
    assert tck_h.prns() == tck_d.prns() == sorted(SVS)
    for p in SVS:
        for f in pkg.abi.FIELDS_POS:
            assert np.array_equal(getattr(tck_h(p), f), getattr(tck_d(p), f)), (p, f)
        assert len(tck_h(p).carrFreq) == CTPOS
    K.assert_same_solution(nav_h, nav_d)
    # both equal the twin run on the downloaded records
    t = twin_on(po, pkg, z, tck_h, signal, solu, tow, start)
    assert np.array_equal(nav_d.Index, t.Index) and np.array_equal(nav_d.index, t.index)
    for f in T.EXACT_FIELDS:
        assert np.array_equal(getattr(nav_d, f), getattr(t, f)), f
    fitted_within(nav_d, t)
    # the struct is navSolCT_10ms_Opensky.mat's
    for f, _ in pkg.abi.NAVSOL_CT_FIELDS:
        assert getattr(nav_d, f).shape[1:] == z["sol_" + f].shape[1:], f

    # hand-over: this navSolutionsCT starts the vector-tracking loop (until now only the
    # reference's recorded file could)
    track.msToProcessVT = 40
    vt, nsol = pkg.trackingVT_POS_updated(file, signal, track, cmn, solu, A, cns, eph, sbf, None, tck_d, nav_d,
                                          ctx=ctx, nsteps=40)
    assert vt.prns() == sorted(SVS) and vt(16).codeFreq.shape == (40,)
    assert nsol.usrPos.shape == (40, 3) and np.all(np.isfinite(nsol.usrPos))
