"""A numpy restatement of CalculateFeatures.m's F6-F8 (:229-231, :243-268; the definition in
include/gnss_mi355x.h), independent of csrc/acf_ext.h: the local-maximum count vectorised over
rows, the spectrum as a (bins x history) product whose sums run explicitly left to right
(np.add.accumulate, never np.sum or a matrix product, whose blocks round differently). The twiddle
table is an input: numpy's cos need not equal the C library's to the bit."""
import numpy as np

DEFAULTS = dict(fft_hist=300, fft_n=1024, fft_fill=0)
FIELDS = ("numMLC", "fftFreq", "fftMag")


def lsum(x):
    return np.add.accumulate(x, axis=-1)[..., -1]


def row_counts(corr):
    """corr [25][L] -> cnt [L]: the columns 2..24 (1-based) above both neighbours (:247-251); a
    comparison with NaN is false"""
    with np.errstate(invalid="ignore"):
        mid = corr[1:-1]
        return np.sum((mid > corr[:-2]) & (mid > corr[2:]), axis=0).astype(np.int64)


def spectrum(x, c, s, fs):
    """The history x (oldest first) -> (fftFreq, fftMag) (:263-268) over the bins 0 .. N/2"""
    N, H = len(c), len(x)
    with np.errstate(invalid="ignore", over="ignore"):
        y = x - lsum(x) / H
        k = np.arange(N // 2 + 1)
        t = (k[:, None] * np.arange(H)[None, :]) % N
        re, im = lsum(y[None, :] * c[t]), lsum(y[None, :] * s[t])
        mag = np.sqrt(re * re + im * im)
    if np.all(np.isnan(mag)):
        I, M = 1, np.nan
    else:
        I = int(np.argmax(np.where(np.isnan(mag), -np.inf, mag))) + 1  # the first index of the largest
        M = mag[I - 1]
    return ((I - 1) * fs) / N, M / (N / 2)


def channel(corr, meanMax, c, s, *, ind_start, numOverLap, fs, fft_hist, fft_fill):
    """One PRN: corr [25][L] and the windows' meanMax -> dict of the three per-window arrays"""
    W, N = len(meanMax), int(numOverLap)
    cnt = row_counts(corr)
    out = {f: np.zeros(W) for f in FIELDS}
    hist = np.zeros(fft_hist)  # :231, :293
    for m in range(W):
        r0 = ind_start - 1 + m * N
        out["numMLC"][m] = int(np.sum(cnt[r0:r0 + N])) / N  # :256
        hist = np.concatenate([hist[1:], meanMax[m:m + 1]])  # :262
        x = hist[-min(m + 1, fft_hist):] if fft_fill else hist
        out["fftFreq"][m], out["fftMag"][m] = spectrum(x, c, s, fs)
    return out
