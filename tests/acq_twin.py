"""A plain numpy restatement of acquisition.m:41-68: the whole PRN x bin x code-phase correlation
surface and the detector that reads it (test infrastructure; numpy only, no oracle code).

`surface` is written once and evaluated three ways, so a test can tell what a correct evaluation's
rounding looks like without asking the code under test:
  fft=np.fft, dtype=complex128   the fp64 reference;
  fft=<another FFT>              a second fp64 evaluation with a different transform (the tests
                                 pass the C oracle's mixed-radix FFT);
  dtype=complex64                the same arithmetic in fp32 (numpy's FFT keeps the type).
"""
import math

import numpy as np

from numpy_twin import ca_code

FC = 1.023e6  # codeFreqBasis


def surface(samples, S, datalen, nbins, IF, freqMin, freqStep, Fs, prns, dtype=np.complex128, fft=np.fft, fc=FC):
    """corr[p, b, tau] of acquisition.m:41-61 on `samples` (complex, >= S * datalen of them, as
    numpy_twin.read_samples forms them):
      carrier_b = exp(1i * (2 pi (IF + f_b) * n) / Fs), n = 1..S                            (:41-44)
      scode     = [CA CA](ceil(n * (fc / Fs)))                                              (:50-51)
      corr[p, b] = sum over ms of |ifft(fft(scode) .* conj(fft(x_ms .* carrier_b)))|^2      (:53-61)
    the ms summed in order. The carrier is evaluated in fp64, its angle rounded step by step as
    written above (it reaches 2.9e4 rad at IF = 4.58 MHz, where one ulp is 3.6e-12 rad: an angle
    reduced in cycles first gives a surface 1e-11 of the RMS away), and rounded to `dtype`; every
    product, transform, square and sum after that is in `dtype`'s precision."""
    dtype = np.dtype(dtype)
    real = np.float32 if dtype == np.complex64 else np.float64
    n = np.arange(1, S + 1, dtype=float)
    x = np.asarray(samples)[: S * datalen].astype(dtype)
    # conj(fft(x_ms .* carrier_b)) does not depend on the PRN: once per (ms, bin)
    Xc = np.empty((datalen, nbins, S), dtype=dtype)
    for b in range(nbins):
        w = 2.0 * np.pi * (IF + (freqMin + freqStep * b))
        carrier = np.exp(1j * ((w * n) / Fs)).astype(dtype)
        for ms in range(datalen):
            X = fft.fft(x[ms * S:(ms + 1) * S] * carrier)
            assert X.dtype == dtype, X.dtype
            Xc[ms, b] = np.conj(X)
    idx = np.ceil(n * (fc / Fs)).astype(np.int64) - 1
    corr = np.zeros((len(prns), nbins, S), dtype=real)
    for p, prn in enumerate(prns):
        ca = ca_code(prn)
        scode = np.concatenate([ca, ca])[idx].astype(dtype)
        C = fft.fft(scode)
        assert C.dtype == dtype, C.dtype
        for ms in range(datalen):
            for b in range(nbins):
                y = fft.ifft(C * Xc[ms, b])
                assert y.dtype == dtype, y.dtype
                corr[p, b] += np.abs(y) ** 2
    return corr


def detect(corr_2d, cshift):
    """acquisition.m:62-68 on one PRN's surface [nbins, S]: (fbin, codePhase, SNR, peak, peak2),
    indices 1-based. peak is the global maximum; fbin the first bin and codePhase the first
    column holding it, each found on its own ([~, fbin] = max(max(corr')), [peak, codePhase] =
    max(max(corr))); the SNR is peak^2 over the mean square of corr(fbin, [1:cp-cshift,
    cp+cshift:end]) and peak2 the maximum over that range. The mean's sum is exact (fsum)."""
    c = np.asarray(corr_2d, dtype=float)
    S = c.shape[1]
    peak = c.max()
    hit = c == peak
    fbin = int(np.argmax(hit.any(axis=1))) + 1
    cp = int(np.argmax(hit.any(axis=0))) + 1
    row = c[fbin - 1]
    off = np.concatenate([row[: max(0, cp - cshift)], row[min(S, cp + cshift - 1):]])
    ss = np.float64(math.fsum(off * off))
    with np.errstate(divide="ignore", invalid="ignore"):
        snr = 10.0 * np.log10((peak * peak) / (ss / np.float64(len(off))))
    peak2 = float(off.max()) if len(off) else 0.0
    return fbin, cp, float(snr), float(peak), peak2
