"""numpy restatement of the positioning half of trackingCT_POS_updated.m (:147-171, :420-565)
and of its 25-tap sibling (trackingCT_POS_updated_multicorrelator.m:446-590), with olspos.m,
hmat.m and LS_SA_code_Vel.m, vectorised where MATLAB is. Independent of the library: the orbit
and geo helpers are the CPU oracle's (pyoracle.svposvel / pyoracle.geo), MATLAB's `\\` is
numpy.linalg.lstsq and inv() numpy.linalg.inv. The tests hold the library against this twin and
the twin against the reference's recorded navSolCT_10ms_Opensky.mat (tests/golden/
ref_navSolCT_10ms_Opensky.npz)."""
import os
from types import SimpleNamespace

import numpy as np

from conftest import GOLDEN

PATH = os.path.join(GOLDEN, "ref_navSolCT_10ms_Opensky.npz")
LAMBDA = 0.190293672798365  # :514
FIT_FIELDS = ["usrPos", "clkBias", "usrVel", "clkDrift", "DOP", "satEA", "satAZ", "usrPosENU", "usrPosLLH",
              "usrVelENU"]
EXACT_FIELDS = ["codePhaseMeas", "timeTransmit", "rawPseudorange", "localTime"]


class IndexZero(IndexError):
    """`index` = 0 (:447): MATLAB raises on TckResultCT(prn).remChip(0)."""


class NoConvergence(RuntimeError):
    """olspos.m's while loop has no iteration cap; the twin stops at `max_iter`."""


def fixture():
    with np.load(PATH) as f:
        return {k: f[k] for k in f.files}


def fixture_args(z, po=None):
    """The fixture as solve()'s keyword arguments (initParameters.m's Opensky values)."""
    return dict(absoluteSample=z["rec_absoluteSample"], remChip=z["rec_remChip"], codeFreq=z["rec_codeFreq"],
                carrFreq=z["rec_carrFreq"], countinx=z["countinx"], nav1=z["nav1"], sfb1=z["sfb1"], TOW1=z["TOW1"],
                eph=z["eph"], sampleStartMea=int(z["sampleStartMea"]), Fs=58e6, IF=4.58e6, codelength=1023.0,
                dataType=2, navSolPeriod=20, ms1=1000, doy=171, cSpeed=299792458.0)


def schedule(absoluteSample, sampleStartMea, measSampleStep, length=None):
    """:423-447: per epoch the tracking step `Index` at which it fires (at most one per step) and
    every channel's `index` -> (Index[k], index[k][s], curr[k]). IndexZero where index = 0."""
    A = np.asarray(absoluteSample, dtype=np.float64)
    L = A.shape[1] if length is None else int(length)
    Index, index, curr = [], [], []
    last = 0
    while True:
        c = float(sampleStartMea) + float(measSampleStep) * len(Index)
        first = np.array([np.searchsorted(a[:L], c, side="right") + 1 for a in A])  # 1-based
        step = max(int(first.max()), last + 1)
        if step > L:
            break
        if first.min() < 2:
            raise IndexZero(len(Index))
        Index.append(step)
        index.append(first - 1)
        curr.append(c)
        last = step
    return np.array(Index, dtype=np.int64), np.array(index, dtype=np.int64).reshape(len(Index), A.shape[0]), curr


def olspos(po, prvec, svxyzr, initpos, tol=1e-3, max_iter=50):
    """olspos.m:30-61 -> (estusr[4], dop[4], iterations)."""
    est = np.array(list(initpos) + [0.0] * (4 - len(initpos)), dtype=np.float64)
    beta = np.full(4, 1e9)
    it = 0
    while np.linalg.norm(beta) > tol:  # (a NaN beta ends the loop, as in MATLAB)
        if it >= max_iter:
            raise NoConvergence(it)
        d = est[:3] - svxyzr                     # hmat.m:18
        r = np.sqrt(np.sum(d * d, axis=1))
        y = prvec - r - est[3]
        H = np.column_stack([d / r[:, None], np.ones(len(r))])
        beta = np.linalg.lstsq(H, y, rcond=None)[0]
        est = est + beta
        it += 1
    Q = np.linalg.inv(H.T @ H)
    dop = np.array([np.sqrt(np.trace(Q)), np.sqrt(Q[0, 0] + Q[1, 1] + Q[2, 2]), np.sqrt(Q[0, 0] + Q[1, 1]),
                    np.sqrt(Q[2, 2])])
    return est, dop, it


def ls_vel(XR, XS, VS, dop_R, dtSV):
    """LS_SA_code_Vel.m:61-95 -> (VR[3], dtRV)."""
    dist = np.sqrt(np.sum((XS - XR) ** 2, axis=1))
    A = np.column_stack([(XR[0] - XS[:, 0]) / dist, (XR[1] - XS[:, 1]) / dist, (XR[2] - XS[:, 2]) / dist,
                         np.ones(len(dist))])
    b = np.sum(A[:, :3] * VS, axis=1) - dtSV
    y0 = dop_R * LAMBDA
    x = np.linalg.inv(A.T @ A) @ A.T @ (y0 - b)
    return x[:3], x[3]


def code_phase(A, remChip, codeFreq, index, curr, Fs, dataType):
    """codePhaseMeas of every channel at measurement sample `curr` (:450-453)."""
    s, i0 = np.arange(A.shape[0]), index - 1
    return remChip[s, i0] + (codeFreq[s, i0] / Fs) * ((curr - A[s, i0]) / dataType)


def transmit_time(cpm, index, step, countinx, nav1, sfb1, TOW1, codelength, ms1, mode):
    """transmitTime of every channel (:455-457; the 25-tap sibling's :481-483)."""
    if mode == "pos_updated":
        lp = 1 if step <= ms1 + countinx[-1] else 10  # the loop variable as the last channel left it
        return cpm / codelength / 1000 + ((index - ms1 - countinx) * lp + (ms1 + countinx) -
                                          (nav1 + sfb1 * 20)) / 1000 + TOW1
    return cpm / codelength / 1000 + (index - (nav1 + sfb1 * 20)) / 1000 + TOW1


def first_transmit_time(*, absoluteSample, remChip, codeFreq, countinx, nav1, sfb1, TOW1, sampleStartMea, Fs,
                        codelength, dataType, navSolPeriod, ms1, mode="pos_updated", **unused):
    """The first epoch's transmitTime alone (no fit): what a test needs to place its TOW."""
    A = np.asarray(absoluteSample, dtype=np.float64)
    Index, index, curr = schedule(A, sampleStartMea, float(np.fix(Fs * navSolPeriod / 1000) * dataType))
    cpm = code_phase(A, remChip, codeFreq, index[0], curr[0], Fs, dataType)
    return transmit_time(cpm, index[0], Index[0], np.asarray(countinx, dtype=np.int64), nav1, sfb1, TOW1, codelength,
                         ms1, mode)


def solve(po, *, absoluteSample, remChip, codeFreq, carrFreq, countinx, nav1, sfb1, TOW1, eph, sampleStartMea, Fs,
          IF, codelength, dataType, navSolPeriod, ms1, cnslxyz, ALPHA, BETA, doy, cSpeed, mode="pos_updated",
          pdi=1, ms=1e-3, length=None, force_corrUpt=None, max_iter=50):
    """The whole pass -> SimpleNamespace of the navSolutionsCT fields (:509-551) as rows, plus
    Index (the tracking step of each row) and iters (olspos iterations per row).
    force_corrUpt: the az / el / iono / tropo refresh held at that many epochs throughout (the
    cadence test's counter-example; None: the reference's)."""
    A = np.asarray(absoluteSample, dtype=np.float64)
    n = A.shape[0]
    countinx = np.asarray(countinx, dtype=np.int64)
    measSampleStep = float(np.fix(Fs * navSolPeriod / 1000) * dataType)  # :164
    Index, index, curr = schedule(A, sampleStartMea, measSampleStep, length)
    names = ["rawPseudorange", "usrPos", "usrVel", "usrPosENU", "usrPosLLH", "clkBias", "usrVelENU", "clkDrift",
             "DOP", "satEA", "satAZ", "timeTransmit", "codePhaseMeas", "localTime", "iters"]
    rows = {k: [] for k in names}
    if n < 4 and len(Index):
        raise ValueError("insufficient number of satellites")  # hmat.m:10
    localTime = np.inf
    est = np.asarray(cnslxyz, dtype=np.float64)[:3]
    if mode == "pos_updated":
        corrUpt = 0.01 / (1 * ms)  # :47,128-130
    else:
        corrUpt = 0.01 / (pdi * ms)
    counter = np.full(n, (corrUpt if force_corrUpt is None else force_corrUpt) - 1)
    el, az, iono, trop = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    for k, step in enumerate(Index):
        cpm = code_phase(A, remChip, codeFreq, index[k], curr[k], Fs, dataType)
        if mode == "pos_updated" and step > ms1 + countinx.min() and force_corrUpt is None:
            corrUpt = 0.01 / (10 * ms)  # :301-302 ran this step
            counter = np.full(n, corrUpt - 1)
        tt = transmit_time(cpm, index[k], step, countinx, nav1, sfb1, TOW1, codelength, ms1, mode)
        cu = corrUpt if force_corrUpt is None else force_corrUpt
        if localTime == np.inf:
            localTime = tt.max() + 75 / 1000  # :462-465
        pr = (localTime - tt) * cSpeed
        prvec, svr, svv, clkv = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
        for s in range(n):  # :472-505
            pos, vel, clkm, clkv[s], grp = po.svposvel(eph[s], tt[s])
            svv[s] = vel
            prvec[s] = pr[s] + clkm - grp * cSpeed
            svr[s] = po.geo("erotcorr", pos, prvec[s])
            counter[s] += 1
            if counter[s] == cu:
                enu = po.geo("xyz2enu", svr[s], est[:3])
                az[s] = np.arctan2(enu[0], enu[1]) * 180 / np.pi
                el[s] = np.arctan(enu[2] / np.linalg.norm(enu[:2])) * 180 / np.pi
                llh = po.geo("xyz2llh", est[:3])
                if not np.isfinite(llh[0]):  # Get_UNB3_Model.m indexes its table with NaN: MATLAB raises
                    raise IndexError("trop_UNB3 at a NaN latitude")
                iono[s] = po.geo("ionocorr", tt[s], svr[s], est[:3], ALPHA, BETA)
                trop[s] = abs(po.geo("trop_UNB3", doy, llh[0] * 180 / np.pi, llh[2], el[s]))
                counter[s] = 0
            prvec[s] = prvec[s] - iono[s] - trop[s]
        est, dop, it = olspos(po, prvec, svr, est, max_iter=max_iter)  # :512
        VR, dtRV = ls_vel(est[:3], svr, svv, carrFreq[np.arange(n), step - 1] - IF, clkv)  # :513-514
        llh = po.geo("xyz2llh", est[:3])
        Lb, lb = llh[0], llh[1]
        Cen = np.array([[-np.sin(lb), np.cos(lb), 0],
                        [-np.sin(Lb) * np.cos(lb), -np.sin(Lb) * np.sin(lb), np.cos(Lb)],
                        [-np.cos(Lb) * np.cos(lb), -np.cos(Lb) * np.sin(lb), -np.sin(Lb)]])
        localTime = localTime - est[3] / cSpeed  # :550
        vals = dict(rawPseudorange=pr, usrPos=est[:3].copy(), usrVel=VR, usrPosENU=po.geo("xyz2enu", est[:3], cnslxyz),
                    usrPosLLH=np.array([llh[0] * 180 / np.pi, llh[1] * 180 / np.pi, llh[2]]), clkBias=est[3],
                    usrVelENU=Cen @ VR, clkDrift=dtRV, DOP=dop, satEA=el.copy(), satAZ=az.copy(), timeTransmit=tt,
                    codePhaseMeas=cpm, localTime=localTime, iters=it)
        for f, v in vals.items():
            rows[f].append(v)
        localTime = localTime + measSampleStep / Fs  # :554
    width = dict(rawPseudorange=n, usrPos=3, usrVel=3, usrPosENU=3, usrPosLLH=3, usrVelENU=3, DOP=4, satEA=n,
                 satAZ=n, timeTransmit=n, codePhaseMeas=n)
    out = SimpleNamespace(**{f: np.array(v, dtype=np.float64).reshape((len(Index), width[f]) if f in width
                                                                      else (len(Index),))
                             for f, v in rows.items()})
    out.Index = Index
    out.index = index
    out.rows = len(Index)
    return out
