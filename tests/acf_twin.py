"""A numpy restatement of ACF/CalculateFeatures.m:165-296 (the definition in
include/gnss_mi355x.h), independent of csrc/acf.h: vectorised over rows and windows as the script
could be, every sum explicitly left to right (np.add.accumulate, never np.sum, whose pairwise
blocks round differently), the script's all-zero first row of data_labeled included. The
reference ships no output of the script, so this restatement is what the library is held to."""
import numpy as np

DEFAULTS = dict(ind_start=1, numOverLap=100, corrSpacing=0.05, maxDelay=0.6,
                a=(4092.9779845217, 340.423503277404, -2.99026922880033, 0.0251763660254827))
FIELDS = ["meanMax", "F1", "F2", "varDelay", "meanCodeDisc", "varCodeDisc"]


def lsum(x):
    """sum over the last axis, left to right, starting from the first element"""
    return np.add.accumulate(x, axis=-1)[..., -1]


def expected_corr(a, ele):
    return a[0] + a[1] * ele ** 1 + a[2] * ele ** 2 + a[3] * ele ** 3  # :188


def channel(tap_i, tap_q, disc, ele, *, ind_start, numOverLap, corrSpacing, maxDelay, a):
    """One PRN: tap_i / tap_q [25][L] in storage order, disc [L]. -> dict of the per-window
    arrays, maxCorrInd [L] (1-based) and corr [25][L]."""
    N = int(numOverLap)
    L = tap_i.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        corr = np.sqrt(tap_i * tap_i + tap_q * tap_q)  # :197-225
    # [~, ind] = max(row): the first index of the largest, NaN as missing, 1 when all are NaN
    ind = np.argmax(np.where(np.isnan(corr), -np.inf, corr), axis=0) + 1
    cen = maxDelay / corrSpacing + 1  # :176
    W = max((L - ind_start) // N, 0) if L > ind_start else 0  # :234
    r0 = ind_start - 1
    rows = slice(r0, r0 + W * N)
    iw = ind[rows].reshape(W, N)
    pw = corr[12][rows].reshape(W, N)  # maxCorr(n) = corr(r, 13) (:237)
    dw = np.asarray(disc, dtype=np.float64)[rows].reshape(W, N)
    out = {"windows": W, "maxCorrInd": ind.astype(np.uint8), "corr": corr}
    if W == 0:
        out.update({f: np.zeros(0) for f in FIELDS})
        return out
    S = np.cumsum(iw.astype(np.int64), axis=1)  # exact
    den = np.full((W, N), float(N))
    den[0] = np.arange(1, N + 1)  # the first window's row grows with n (:238; cleared per PRN, :294)
    fw = iw.astype(np.float64)
    tmp = (fw - S.astype(np.float64) / den) * corrSpacing
    with np.errstate(invalid="ignore", over="ignore"):
        meanMax = lsum(pw) / N  # :260
        meanDelay = lsum((fw - cen) * corrSpacing) / N  # :270
        varDelay = lsum(tmp * tmp) / N  # :271
        meanCD = lsum(dw) / N  # :273
        e = dw - meanCD[:, None]
        varCD = lsum(e * e) / (N - 1)  # :274
        out.update(meanMax=meanMax, F1=meanMax / expected_corr(a, float(ele)), F2=-(meanDelay + 0.00) * 1,
                   varDelay=varDelay, meanCodeDisc=meanCD, varCodeDisc=varCD)
    return out


def features(taps, disc, lens, prnList, eleList, **params):
    """taps [n][2][25][max_len], disc [n][max_len], lens [n] -> (data_labeled, per-channel dicts)."""
    par = dict(DEFAULTS, **params)
    data = [np.zeros((1, 8))]  # :165
    chans = []
    for c, (p, el) in enumerate(zip(prnList, eleList)):
        L = int(lens[c])
        ch = channel(taps[c, 0, :, :L], taps[c, 1, :, :L], disc[c, :L], el, **par)
        chans.append(ch)
        W = ch["windows"]
        data.append(np.column_stack([np.full(W, float(p)), np.full(W, float(el))] + [ch[f] for f in FIELDS]).reshape(W, 8))
    return np.vstack(data), chans
