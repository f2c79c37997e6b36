"""The sampling-rate matrix shared by test_oracle_rates (CPU) and test_gpu_rates (GPU): one
scene (PRNs 5 / 13 / 20) synthesised at five (Fs, IF) points off the 58 MHz / 4.58 MHz grid every
other tracking test runs on, the oracle's results on it (cached per rate, tap count and record
format: they do not depend on the lane span or on the persistent / per-step choice), and the
single-step case list. A plain helper module, no fixtures.

What each rate brings (track_geom.h's lane geometry, track.hip's carrier table and step sizing):
  urban26    BASELINE config 4's signal: IF = 0, so the carrier is the Doppler alone (negative
             for PRNs 5 and 20); 32-sample lanes refused, 16-sample lanes in the 10-ms phase
  l1_16m     Fs*ms = 16367.6 is no integer (Sample = ceil = 16368), f/Fs = 0.25, and the
             acquisition runs rocFFT at a length with the prime factors 11 and 31
  zero_12m5  Sample = 12500 is no multiple of 8; PRN 20's carrier crosses zero inside the run
  low_10m    only 8-sample lanes are left, at 0.90 chip per lane with the 1.1 margin
  edge_8m5   inside the 1.1 margin (8 * 1.1 * fc / Fs = 1.06) while the kernel's own
             d * M = 0.963 stays below 1
"""
import functools
import math
from types import SimpleNamespace

import numpy as np

import pyoracle as po

pkg = po.PKG

FC = 1.023e6
RATES = {"urban26": (26e6, 0.0), "l1_16m": (16.3676e6, 4.1304e6), "zero_12m5": (12.5e6, 0.0),
         "low_10m": (10e6, 2.5e6), "edge_8m5": (8.5e6, 2.0e6)}
ZERO_IF = [r for r, (_, IF) in RATES.items() if IF == 0.0]
ACQ_RATES = ["l1_16m", "zero_12m5", "low_10m"]  # acquisition off the two own-FFT sizes (rocFFT)
FLOOR = (8e6, 2.0e6)  # below the host's floor: 8 * fc / Fs = 1.023

PRNS, DOPPLERS, CN0S = [5, 13, 20], [-2310.0, 1475.0, -35.0], [46.0, 44.0, 45.0]
ABSENT_PRN = 9
SKIP, N1, N10 = 3, 700, 60
F_EXTRA = 4.2e6 + 3000  # at low_10m: f/Fs = 0.42, the rotation table reaches 82 rad


@functools.lru_cache(maxsize=None)
def taps11():
    """-0.5:0.1:0.5 as MATLAB's colon forms it (E = tap 0, P = tap 5, L = tap 10)."""
    return po.colon(-0.5, 0.1, 0.5)


def sample_of(Fs):
    return math.ceil(Fs * 1e-3)


def signal_of(rate):
    Fs, IF = RATES[rate] if isinstance(rate, str) else rate
    return SimpleNamespace(IF=IF, Fs=Fs, codeFreqBasis=FC, ms=1e-3, Sample=sample_of(Fs), codelength=1023.0)


@functools.lru_cache(maxsize=None)
def scene(rate):
    """(synth config, the three code delays in samples) of a rate."""
    Fs, IF = RATES[rate]
    S = sample_of(Fs)
    cds = [int(x) for x in np.random.default_rng(int(Fs) % 1000).integers(0, S, 3)]
    cfg = pkg.synth.scenario(PRNS, cds, DOPPLERS, CN0S, Fs=Fs, IF=IF, skip_ms=SKIP, seed=77)
    return cfg, cds


@functools.lru_cache(maxsize=None)
def record(rate, prec=1, dtyp=2):
    """The record's byte image (read-only): int8 I/Q, or synth.convert_record's other formats."""
    if (prec, dtyp) != (1, 2):
        data = pkg.synth.convert_record(record(rate), prec, dtyp)
    else:
        cfg, _ = scene(rate)
        data = po.synth_if(cfg, 0, (SKIP + N1 + 19 + N10 + 6) * sample_of(RATES[rate][0]))
    data.setflags(write=False)
    return data


def file_of(rate, prec=1, dtyp=2):
    return SimpleNamespace(skip=SKIP, dataType=dtyp, dataPrecision=prec, data=record(rate, prec, dtyp),
                           fileRoute=None, dev=None)


def track_params():
    track = pkg.initParameters()[3]
    track.msToProcessCT_1ms, track.msToProcessCT_10ms = N1, N10
    return track


def acq_params():
    """+-3 kHz / 500 Hz (13 bins), datalen 10, L 10 (at datalen 4 the absent PRN 9 reads 12.05 dB
    at 26 MHz: on the 12 dB gate)."""
    return SimpleNamespace(freqNum=13, freqMin=-3000, freqStep=500, datalen=10, L=10)


ACQ_PRNS = [5, ABSENT_PRN, 13, 20]


@functools.lru_cache(maxsize=None)
def oracle_acquisition(rate):
    return po.acquisition(file_of(rate), signal_of(rate), acq_params(), prn_list=ACQ_PRNS, diag=True)


def acquired_for(rate):
    """trackingCT's Acquired: the oracle's acquisition where the matrix runs one, else the
    scene's own code delays and IF + Doppler."""
    if rate in ACQ_RATES:
        return oracle_acquisition(rate)[0]
    _, cds = scene(rate)
    IF = RATES[rate][1]
    return SimpleNamespace(sv=np.array(PRNS), SNR=np.full(3, 20.0), Doppler=np.zeros(3),
                           codedelay=np.array(cds), fineFreq=np.array([IF + d for d in DOPPLERS]))


@functools.lru_cache(maxsize=None)
def oracle_tracking(rate, ntaps=3, prec=1, dtyp=2):
    """The oracle's trackingCT (raw buffers, .status) of the rate's three channels."""
    taps = taps11() if ntaps == 11 else None
    r = po.trackingCT(file_of(rate, prec, dtyp), signal_of(rate), track_params(), acquired_for(rate),
                      taps=taps, raw=True)
    for a in (r.rec, r.taps, r.len, r.countinx, r.CN0):
        if a is not None:
            a.setflags(write=False)
    return r


def num_sample(pdi, remChip, codeFreq, Fs):
    """trackingCT.m:80: round((codelength*pdi - remChip) / (codeFreq/Fs)), MATLAB's round (halves
    away from zero, as C's round; numpy's rounds them to even). remChip = -0.5 * fc / Fs at the
    nominal code rate makes the quotient Sample*pdi + 0.5 where Fs*ms is an integer: a tie."""
    q = (1023.0 * pdi - remChip) / (codeFreq / Fs)
    return math.floor(q) + (1 if q - math.floor(q) >= 0.5 else 0)


@functools.lru_cache(maxsize=None)
def step_cases(rate):
    """Single correlation steps: pdi x taps x (remChip, codeFreq) x carrier x phase, each at a
    random even byte offset of the rate's record. The first and last (remChip, codeFreq) put
    early / late samples on exact chip boundaries. Carriers: each channel's IF + Doppler,
    exactly 0.0 at IF = 0, and f/Fs = 0.42 at low_10m."""
    Fs, IF = RATES[rate]
    rng = np.random.default_rng(1000 + list(RATES).index(rate))
    carriers = [(prn, IF + d) for prn, d in zip(PRNS, DOPPLERS)]
    if IF == 0.0:
        carriers.append((20, 0.0))
    if rate == "low_10m":
        carriers.append((5, F_EXTRA))
    states = [(0.0, FC), (0.009, FC + 3.1), (-0.009, FC - 2.7), (-0.5 * FC / Fs, FC)]
    nrec = len(record(rate)) // 2
    cases = []
    for pdi in (1, 10):
        for ntaps in (3, 11):
            for rc, cf in states:
                for prn, f in carriers:
                    for ph in (0.0, float(rng.uniform(-2 * np.pi, 2 * np.pi))):
                        n = num_sample(pdi, rc, cf, Fs)
                        pos = 2 * int(rng.integers(0, nrec - n - 8))
                        cases.append(SimpleNamespace(prn=prn, pdi=pdi, ntaps=ntaps, remChip=rc, codeFreq=cf,
                                                     carrierFreq=f, remPhase=ph, pos_bytes=pos, n=n))
    return tuple(cases)


def case_taps(case):
    return taps11() if case.ntaps == 11 else np.array([-0.5, 0.0, 0.5])


def oracle_step(rate, case):
    iq = record(rate)[case.pos_bytes: case.pos_bytes + 2 * case.n]
    return po.correlate_step(iq, case.n, case.remChip, case.codeFreq, RATES[rate][0], case.carrierFreq,
                             case.remPhase, po.generate_ca(case.prn), case.pdi, case_taps(case))


@functools.lru_cache(maxsize=None)
def oracle_steps(rate):
    return tuple(oracle_step(rate, c) for c in step_cases(rate))


# ---- the engine's lane geometry (csrc/track_geom.h: sub_ok / sub_for / bpc_for), restated ------
def sub_ok(Fs, sub):
    """A lane of 8*sub samples holds at most one chip boundary per tap, with the 1.1 margin."""
    return 8.0 * sub * 1.1 * FC / Fs < 1.0


def tracking_subs(Fs):
    """The GNSS_OPT_FORCE_SUB values trackingCT admits at a rate (others leave its own choice)."""
    return [v for v in (1, 2, 3, 4) if sub_ok(Fs, v)]


def step_subs(Fs, codeFreq=FC + 3.1):
    """The GNSS_OPT_FORCE_SUB values gnss_correlate_step admits: 8 * v * codeFreq / Fs < 1."""
    return [v for v in (1, 2, 3, 4) if 8.0 * v * codeFreq / Fs < 1.0]


def lane_geometry(Fs, pdi, forced=0):
    """(sub, blocks per channel) of an int8 3- or 11-tap step of pdi ms."""
    sub = 3 if pdi >= 10 else 1
    while sub > 1 and not sub_ok(Fs, sub):
        sub -= 1
    if forced and sub_ok(Fs, forced):
        sub = forced
    groups = (sample_of(Fs) * pdi * 1.01 + 64) / 8.0 + 2
    return sub, math.ceil(groups / (256.0 * sub))
