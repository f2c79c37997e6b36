"""The cases shared by tests/test_acq_twin_kat.py (CPU: the numpy twin against the C oracle) and
tests/test_gpu_acq_surface.py (GPU: every cell of the correlation surface against the twin).
Every input is fixed here; a reference is computed once per case and shared."""
import math
from types import SimpleNamespace

import numpy as np

import acq_twin
import numpy_twin

RATES = {26000: dict(Fs=26e6, IF=0.0), 58000: dict(Fs=58e6, IF=4.58e6)}
SKIP_MS, RECORD_MS = 1, 13
FMT = {"int8-iq": (1, 2), "int16-iq": (2, 2), "int8-real": (1, 1)}


def case(S, kind, datalen, freqNum, freqMin, freqStep, prns, fmt="int8-iq"):
    return SimpleNamespace(S=S, kind=kind, datalen=datalen, freqNum=freqNum, freqMin=freqMin, freqStep=freqStep,
                           prns=list(prns), fmt=fmt, **RATES[S])


# The smallest shapes the own correlator admits (S = 13 x 2000 and 29 x 2000): datalen 1 / 2 / 3
# (a single ms, a pair, an odd count whose spare transform must not be summed), freqNum 3 / 9 (not
# a multiple of the detector's 8-bin load group), PRN lists of 1 / 2 / 5 with present and absent
# SVs mixed (Urban holds 1 3 7 11 18 22, Opensky 3 4 16 22 26 27 31 32).
SURFACE_CASES = {
    "urban-1ms-3bin-1prn": case(26000, "urban", 1, 3, 700, 500, [1]),
    "urban-2ms-9bin-2prn": case(26000, "urban", 2, 9, -2000, 500, [7, 2]),
    "urban-3ms-9bin-5prn": case(26000, "urban", 3, 9, -2000, 500, [1, 2, 7, 5, 11]),
    "opensky-2ms-3bin-2prn": case(58000, "opensky", 2, 3, 500, 500, [3, 5]),
    "opensky-3ms-9bin-5prn": case(58000, "opensky", 3, 9, -2000, 500, [3, 1, 16, 2, 26]),
    "urban-int16-iq": case(26000, "urban", 2, 9, -2000, 500, [7, 2], "int16-iq"),
    "urban-int8-real": case(26000, "urban", 2, 9, -2000, 500, [7, 2], "int8-real"),
    "opensky-int16-iq": case(58000, "opensky", 2, 3, 500, 500, [3, 5], "int16-iq"),
    "opensky-int8-real": case(58000, "opensky", 2, 3, 500, 500, [3, 5], "int8-real"),
}

# Detector windows at the row ends: the code delays (samples) of one strong SV each, so the
# peaks sit at columns delay + 1, around column cshift = ceil(Fs / fc) and its mirror at the
# row's end (an empty left range, an empty right range and both one-off neighbours).
EDGE_PRNS = {26000: [1, 2, 3, 5, 6, 7, 8, 9, 10], 58000: [1, 2, 3, 5, 6, 7, 8]}
EDGE_DELAYS = {26000: [0, 1, 25, 26, 27, 25973, 25974, 25975, 25999],
               58000: [0, 56, 57, 58, 57942, 57943, 57999]}
EDGE_CASES = {S: case(S, "edges", 2, 3, -250, 250, EDGE_PRNS[S]) for S in (26000, 58000)}

_iq8 = {}
_ref = {}


def record_iq8(pkg, po, kind, S):
    """The int8 I/Q bytes of a 13-ms record (skip 1 ms): synth.urban / synth.opensky, or the
    edge scenario (seed 77, 52 dB-Hz, Doppler 0)."""
    key = (kind, S)
    if key not in _iq8:
        if kind == "urban":
            cfg = pkg.synth.urban(skip_ms=SKIP_MS)
        elif kind == "opensky":
            cfg = pkg.synth.opensky(skip_ms=SKIP_MS)
        elif kind == "edges":
            n = len(EDGE_PRNS[S])
            cfg = pkg.synth.scenario(EDGE_PRNS[S], EDGE_DELAYS[S], [0.0] * n, [52.0] * n, skip_ms=SKIP_MS, seed=77,
                                     **RATES[S])
        elif kind == "zeros":
            _iq8[key] = np.zeros(2 * RECORD_MS * S, dtype=np.int8)
            return _iq8[key]
        else:
            raise KeyError(kind)
        assert math.ceil(cfg.Fs * 1e-3) == S and cfg.IF == RATES[S]["IF"]
        _iq8[key] = po.synth_if(cfg, 0, RECORD_MS * S)
    return _iq8[key]


def structs(pkg, po, c):
    """(file, signal, acq) of a case, as sdr.acquisition / pyoracle.acquisition take them."""
    prec, dtyp = FMT[c.fmt]
    rec = pkg.synth.convert_record(record_iq8(pkg, po, c.kind, c.S), prec, dtyp)
    file = SimpleNamespace(skip=SKIP_MS, dataType=dtyp, dataPrecision=prec, data=rec, fileRoute=None, dev=None)
    signal = SimpleNamespace(IF=c.IF, Fs=c.Fs, codeFreqBasis=acq_twin.FC, ms=1e-3, Sample=c.S, codelength=1023.0)
    acq = SimpleNamespace(freqNum=c.freqNum, freqMin=c.freqMin, freqStep=c.freqStep, datalen=c.datalen, L=10)
    return file, signal, acq


def cshift_of(c):
    return math.ceil(c.Fs / acq_twin.FC)


def samples_of(pkg, po, c):
    """The block's samples as the reference forms them: one fread of datalen ms at skip ms
    (an int16 record's means are taken over that read, acquisition.m:28-37)."""
    prec, dtyp = FMT[c.fmt]
    file, _, _ = structs(pkg, po, c)
    buf = np.asarray(file.data).view(np.int8)[SKIP_MS * c.S * prec * dtyp:]
    return numpy_twin.read_samples(buf, prec, dtyp, c.S * c.datalen)


def oracle_fft(po):
    """The C oracle's FFT with numpy.fft's two names: the second fp64 transform."""
    return SimpleNamespace(fft=lambda x: po.fft(x), ifft=lambda x: po.fft(x, inverse=True))


def twin_surface(pkg, po, c, which="fp64"):
    """The twin's surface of a case: "fp64" (numpy's FFT), "fp64b" (the oracle's FFT) or "fp32"
    (complex64). Computed once; the arrays are read-only."""
    key = (id(c), which)
    if key not in _ref:
        kw = {"fp64": {}, "fp64b": dict(fft=oracle_fft(po)), "fp32": dict(dtype=np.complex64)}[which]
        s = acq_twin.surface(samples_of(pkg, po, c), c.S, c.datalen, c.freqNum, c.IF, c.freqMin, c.freqStep, c.Fs,
                             c.prns, **kw)
        s.setflags(write=False)
        _ref[key] = s
    return _ref[key]


def cell_distance(a, ref):
    """Per PRN: max over the cells of |a - ref| / rms(ref[p])."""
    a, ref = np.asarray(a, dtype=float), np.asarray(ref, dtype=float)
    rms = np.sqrt(np.mean(ref * ref, axis=(1, 2)))
    return np.max(np.abs(a - ref), axis=(1, 2)) / rms


def detect_all(surf, cshift):
    """acq_twin.detect per PRN, as arrays named like the library's diag."""
    rows = [acq_twin.detect(s, cshift) for s in surf]
    f = lambda i, t: np.array([r[i] for r in rows], dtype=t)
    return SimpleNamespace(fbin=f(0, np.int64), codePhase=f(1, np.int64), SNR=f(2, float), peak=f(3, float),
                           peak2=f(4, float))
