"""Shared set-up of the positioning pass (gnss_ct_pos_solve) for the CPU known-answer tests
(test_ctpos_kat.py) and the GPU tests (test_gpu_ctpos.py): the reference's recorded run
(tests/golden/ref_navSolCT_10ms_Opensky.npz, tests/golden/extract_navsol_fixture.py) and the
schedule-stress cases cut from its records, each runnable through the numpy twin
(ctpos_twin.solve) and through the library (sdr.ct_positioning)."""
from types import SimpleNamespace as NS

import numpy as np

import ctpos_twin as T

MS1 = 1000  # track.msToProcessCT_1ms of the recorded run
SERIES = ("absoluteSample", "remChip", "codeFreq", "carrFreq")


def cnslxyz(po, pkg):
    return po.geo("llh2xyz", pkg.initParameters()[4].iniPos)  # SDR_main.m:66


def after_step(z, step, sel=None):
    """sampleStartMea just past every channel's record of 1-based `step` (:156-160)."""
    a = z["rec_absoluteSample"] if sel is None else z["rec_absoluteSample"][sel]
    return int(a[:, step - 1].max()) + 1


def series(z, case, f):
    """Series f of the case's channels: steps [lo, hi), every dec-th row where the case decimates."""
    a = z["rec_" + f][case["sel"], case["lo"]:case["hi"]]
    d = case.get("dec", 1)
    return a[:, d - 1::d]


def cases(z):
    """name -> dict(sel, lo, hi, start, period, mode, pdi): channels, the record slice [lo, hi)
    (0-based steps), sampleStartMea, solu.navSolPeriod, the mode and track.pdi."""
    full = dict(sel=list(range(5)), lo=0, hi=3000, start=int(z["sampleStartMea"]), period=20, mode="pos_updated",
                pdi=1)
    c = {"fixture": full}
    # the epochs start 300 steps before the first channel's 1 -> 10 ms switch (1000 + countinx):
    # the refresh is every 10th epoch, then every epoch
    c["early"] = dict(full, hi=1100, start=after_step(z, 700))
    # ... and 10 steps earlier the last epoch, at step 1011, falls where the last channel
    # (countinx 5) runs 10-ms steps and others (12, 13) still 1-ms ones: pdi = 10 multiplies their
    # negative (index - ms1 - countinx), their transmitTime jumps by 9 ms per step short of the
    # switch, and the fit lands 30000 km up (the reference's, had its epochs started that early);
    # the records end there, because the next epoch's tropo lookup raises at that latitude
    c["window"] = dict(full, hi=1011, start=after_step(z, 690))
    # navSolPeriod shorter than the 10-ms steps: one epoch per step, the solution lags
    c["period4"] = dict(full, hi=1800, period=4)
    c["period5"] = dict(full, hi=1800, period=5)
    # the 25-tap sibling's transmitTime and fixed cadence on 1-ms rows, and on 10-ms rows
    c["mc_pdi1"] = dict(full, hi=1000, start=after_step(z, 100), mode="multicorr", pdi=1)
    # (10-ms rows built from every 10th 1-ms row, so that every channel's row k ends within the same
    # millisecond; the sibling's transmitTime counts `index` in ms whatever pdi is (:481-483), and
    # the epochs sit 5 ms into a row, away from the rows' staggered ends, where `index` would differ
    # between channels and the pseudoranges by 9 ms of light time)
    c["mc_pdi10"] = dict(full, hi=1000, dec=10, start=after_step(z, 100) + 5 * 58000 * 2, mode="multicorr", pdi=10)
    c["four"] = dict(full, sel=[0, 1, 2, 3], hi=1800)
    # more rows than the schedule kernel's block is wide (1-ms period on 10-ms rows: 1320 epochs)
    c["big"] = dict(full, period=1)
    c["zero"] = dict(full, start=int(z["rec_absoluteSample"].max()) + 5)
    return c


def twin_run(po, pkg, z, case, **over):
    sel = case["sel"]
    kw = T.fixture_args(z)
    for f in SERIES:
        kw[f] = series(z, case, f)
    for f in ("countinx", "nav1", "sfb1", "TOW1", "eph"):
        kw[f] = z[f][sel]
    kw.update(sampleStartMea=case["start"], navSolPeriod=case["period"], mode=case["mode"], pdi=case["pdi"],
              cnslxyz=cnslxyz(po, pkg), ALPHA=pkg.sdr.ALPHA, BETA=pkg.sdr.BETA)
    kw.update(over)
    return T.solve(po, **kw)


def lib_inputs(pkg, z, case):
    """The fixture as the host mirror's arguments -> (TckResultCT, file, signal, track, cmn,
    Acquired, eph, sbf, solu, countinx)."""
    file, signal, _, track, solu, cmn = pkg.initParameters()
    sel = case["sel"]
    prns = [int(z["prns"][i]) for i in sel]
    tck = {p: NS(**{f: series(z, case, f)[q] for f in SERIES}) for q, p in enumerate(prns)}
    eph = {p: NS(sfb=[z["sfb1"][i]], TOW=[z["TOW1"][i]], updateflag=1,
                 **{f: [z["eph"][i, j]] for j, f in enumerate(pkg.abi.EPH_SV_FIELDS)}) for i, p in zip(sel, prns)}
    nav1 = np.zeros(32)
    nav1[np.array(prns) - 1] = z["nav1"][sel]
    solu.navSolPeriod = case["period"]
    track.msToProcessCT_1ms, track.pdi = MS1, case["pdi"]
    return tck, file, signal, track, cmn, NS(sv=np.array(prns)), eph, NS(nav1=nav1), solu, z["countinx"][sel]


def lib_run(po, pkg, z, case, records=None, ctx=None, **over):
    tck, file, signal, track, cmn, A, eph, sbf, solu, cx = lib_inputs(pkg, z, case)
    cmn.cSpeed = over.pop("cSpeed", cmn.cSpeed)
    return pkg.ct_positioning(tck if records is None else records, file, signal, track, cmn, A, cnslxyz(po, pkg), eph,
                              sbf, solu, countinx=cx, sampleStartMea=case["start"], mode=case["mode"], ctx=ctx, **over)


def host_records(pkg, z, case):
    """The case's records as raw host records (TrackOutBuffers)."""
    _, _, _, track, _, _ = pkg.initParameters()
    L = series(z, case, "remChip").shape[1]
    buf = pkg.TrackOutBuffers(len(case["sel"]), track, 0, ctPOS=L)
    for f in SERIES:
        buf.rec[:, pkg.abi.FIELDS_POS.index(f)] = series(z, case, f)
    buf.len[:] = L
    return buf


def device_records(pkg, z, case, device="cuda:0"):
    """The case's records uploaded as GNSS_OUT_DEVICE records (DeviceTrackOutBuffers)."""
    import torch
    _, _, _, track, _, _ = pkg.initParameters()
    sel, L = case["sel"], series(z, case, "remChip").shape[1]
    buf = pkg.DeviceTrackOutBuffers(len(sel), track, 0, device=device, ctPOS=L)
    host = np.zeros((len(sel), pkg.abi.NFIELDS, L))
    for f in SERIES:
        host[:, pkg.abi.FIELDS_POS.index(f)] = series(z, case, f)
    buf.rec.copy_(torch.from_numpy(host))
    torch.cuda.synchronize()
    buf.len[:] = L
    return buf


def assert_same_solution(a, b):
    """Two navSolutionsCT equal bit for bit, the measurement table and Index included."""
    for f in ("Index", "index", "carrFreqMeas", "iters") + tuple(T.EXACT_FIELDS) + tuple(T.FIT_FIELDS):
        x, y = getattr(a, f), getattr(b, f)
        assert x.shape == y.shape and np.array_equal(x, y), f
