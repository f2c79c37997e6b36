"""The replay correlator restated in numpy (the definition is in include/gnss_mi355x.h): one row,
any taps, chip_off, post, negative chip numbers. Calls no product code; the C/A chips (+-1) are
handed in. The carrier is numpy's sin / cos of the reference's Wave(k), the sums are taken in
extended precision: a known answer to ~1e-13 of the sums' scale, not a bit pattern."""
import math

import numpy as np

EPS = 2.220446049250313e-16
TWO_PI = 2.0 * 3.14159265358979323846


def colon_ends(a, d, b):
    """MATLAB colon a:d:b for d > 0 (MathWorks' colonop): (intervals, last element)."""
    tol = 2.0 * EPS * max(abs(a), abs(b))
    if a == math.floor(a) and d == 1:
        n = math.floor(b) - a
    elif a == math.floor(a) and d == math.floor(d):
        q = math.floor(a / d)
        n = math.floor((b - (a - q * d)) / d) - q
    else:
        x = (b - a) / d
        n = math.floor(x + 0.5) if x >= 0 else -math.floor(-x + 0.5)  # (C's round: halves away from zero)
        if a + n * d - b > tol:
            n = n - 1
    c = a + n * d
    if c - b > -tol:
        c = b
    return int(n), c


def colon_elements(a, d, c, nn):
    """Elements 0..nn of the colon with ends a, c: the lower half counts up from a, the upper half
    down from c, the middle element of an even interval count is their mean."""
    k = np.arange(nn + 1, dtype=np.float64)
    t = np.where(k <= nn // 2, a + k * d, c - (nn - k) * d)
    if nn % 2 == 0:
        t[nn // 2] = (a + c) / 2
    return t


def samples(record, pos_bytes, n, dataType):
    """(xr, xi) of n samples from byte pos_bytes of an int8 record."""
    r = np.asarray(record, dtype=np.int8)
    if dataType == 2:
        x = r[pos_bytes: pos_bytes + 2 * n].astype(np.float64)
        return x[0::2], x[1::2]
    return r[pos_bytes: pos_bytes + n].astype(np.float64), np.zeros(n)


def replay_row(record, dataType, pos_bytes, n, remChip, codeFreq, Fs, carrFreq, remPhase, ca, taps, chip_off=0,
               post=None):
    """(I[n_taps], Q[n_taps]) of one row; ValueError if a tap's colon has not n elements."""
    xr, xi = samples(record, pos_bytes, n, dataType)
    k = np.arange(n, dtype=np.float64)
    W = TWO_PI * (carrFreq * (k / Fs)) + remPhase
    sn, cs = np.sin(W), np.cos(W)
    tI = (xr * sn + xi * cs).astype(np.longdouble)
    tQ = (xr * cs - xi * sn).astype(np.longdouble)
    d = codeFreq / Fs
    ca = np.asarray(ca, dtype=np.float64)
    I, Q = np.zeros(len(taps)), np.zeros(len(taps))
    for s, tap in enumerate(taps):
        a = (0 + tap) + remChip
        nn, c = colon_ends(a, d, ((n - 1) * d + tap) + remChip)
        if nn != n - 1:
            raise ValueError(f"tap {s}: {nn + 1} elements, not {n}")
        t = colon_elements(a, d, c, nn)
        if post is not None:
            t = t + post[s]
        chip = np.ceil(t).astype(np.int64) + chip_off
        code = ca[np.mod(chip + 1022, 1023)].astype(np.longdouble)  # (numpy's mod is the true modulus)
        I[s] = float(np.sum(code * tI))
        Q[s] = float(np.sum(code * tQ))
    return I, Q


def replay_table(record, dataType, Fs, rows, ca_of, taps, chip_off=0, post=None):
    """A whole table (the arrays of gnss_replay_rows as a namespace) -> [n_chan, 2, n_taps, max_rows]."""
    nch = len(rows.prn)
    out = np.zeros((nch, 2, len(taps), rows.max_rows))
    for c in range(nch):
        ca = ca_of(int(rows.prn[c]))
        for i in range(int(rows.n_rows[c])):
            out[c, 0, :, i], out[c, 1, :, i] = replay_row(
                record, dataType, int(rows.pos_bytes[c, i]), int(rows.numSample[c, i]), float(rows.remChip[c, i]),
                float(rows.codeFreq[c, i]), Fs, float(rows.carrFreq[c, i]), float(rows.remPhase[c, i]), ca, taps,
                chip_off, post)
    return out
