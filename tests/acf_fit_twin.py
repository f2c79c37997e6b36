"""A numpy restatement of the two-path fit of the 25-tap ACF (the definition in
include/gnss_mi355x.h), independent of csrc/acf_fit.h: vectorised over the hypotheses of a grid,
every sum explicitly left to right from its first term (np.add.accumulate, never np.sum, whose
pairwise blocks round differently). The reference has no such estimator, so this restatement is
what the library is held to, bit for bit."""
import numpy as np

DEFAULTS = dict(ind_start=1, numOverLap=100, corrSpacing=0.05, p_min=-0.40, p_step=0.01, p_count=81,
                e_min=0.05, e_step=0.01, e_count=96, ratio_max=1.0, gain_min=16.0)
FIELDS = ["bias", "p1", "A1p_re", "A1p_im", "res1", "p0", "e", "A0_re", "A0_im", "A1_re", "A1_im", "res2", "energy"]
GRID = ("corrSpacing", "p_min", "p_step", "p_count", "e_min", "e_step", "e_count", "ratio_max", "gain_min")


def lsum(x):
    """sum over the last axis, left to right, starting from the first element"""
    return np.add.accumulate(x, axis=-1)[..., -1]


def R(x):
    t = 1.0 - np.abs(x)
    return np.where(t > 0, t, 0.0)


def first_smallest(res, ok):
    """index of the smallest res among the hypotheses that were not skipped, the lowest index on a
    tie; a NaN never wins; None if nothing is left"""
    idx = np.flatnonzero(ok & ~np.isnan(res))
    return int(idx[np.argmin(res[idx])]) if len(idx) else None


def coherent(tap_i, tap_q, row, N):
    """tap_i / tap_q [25][L] -> zI, zQ [25] of the window of N rows from `row`"""
    I, Q = tap_i[:, row: row + N], tap_q[:, row: row + N]
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.where(I[12] >= 0, 1.0, -1.0)  # a NaN compares false: -1
        return lsum(s * I), lsum(s * Q)


def fit_vector(zI, zQ, orient, *, corrSpacing, p_min, p_step, p_count, e_min, e_step, e_count, ratio_max, gain_min):
    """One coherent vector -> dict of paths and FIELDS."""
    zI, zQ = np.asarray(zI, dtype=np.float64), np.asarray(zQ, dtype=np.float64)
    out = {f: np.nan for f in FIELDS}
    out["paths"] = 0
    if not (np.all(np.isfinite(zI)) and np.all(np.isfinite(zQ))):
        return out
    u = (float(orient) * (np.arange(25) - 12.0)) * corrSpacing
    p = p_min + np.arange(p_count, dtype=np.float64) * p_step
    e = e_min + np.arange(e_count, dtype=np.float64) * e_step
    with np.errstate(all="ignore"):
        # one path
        r = R(u[None, :] - p[:, None])
        a = lsum(r * r)
        A_re, A_im = lsum(r * zI) / a, lsum(r * zQ) / a
        dI, dQ = zI - A_re[:, None] * r, zQ - A_im[:, None] * r
        res = lsum(dI * dI + dQ * dQ)
        i1 = first_smallest(res, a != 0)
        if i1 is None:
            return out
        out.update(paths=1, p1=p[i1], A1p_re=A_re[i1], A1p_im=A_im[i1], res1=res[i1],
                   energy=lsum(zI * zI + zQ * zQ))
        # two paths, h = ip * e_count + ie
        ph, eh = np.repeat(p, e_count), np.tile(e, p_count)
        qh = ph - eh
        r0, r1 = R(u[None, :] - ph[:, None]), R(u[None, :] - qh[:, None])
        a, b, c = lsum(r0 * r0), lsum(r1 * r1), lsum(r0 * r1)
        h0I, h0Q, h1I, h1Q = lsum(r0 * zI), lsum(r0 * zQ), lsum(r1 * zI), lsum(r1 * zQ)
        det = a * b - c * c
        ok = (a != 0) & (b != 0) & (det > (1e-9 * a) * b)
        A0_re, A0_im = (b * h0I - c * h1I) / det, (b * h0Q - c * h1Q) / det
        A1_re, A1_im = (a * h1I - c * h0I) / det, (a * h1Q - c * h0Q) / det
        m0, m1 = A0_re * A0_re + A0_im * A0_im, A1_re * A1_re + A1_im * A1_im
        ok &= ~(m1 > (ratio_max * ratio_max) * m0)
        dI = (zI - A0_re[:, None] * r0) - A1_re[:, None] * r1
        dQ = (zQ - A0_im[:, None] * r0) - A1_im[:, None] * r1
        res2 = lsum(dI * dI + dQ * dQ)
        i2 = first_smallest(res2, ok)
        if i2 is not None:
            out.update(p0=ph[i2], e=eh[i2], A0_re=A0_re[i2], A0_im=A0_im[i2], A1_re=A1_re[i2], A1_im=A1_im[i2],
                       res2=res2[i2])
            if out["res1"] > gain_min * out["res2"]:
                out["paths"] = 2
    out["bias"] = out["p0"] if out["paths"] == 2 else out["p1"]
    return out


def fit(taps, lens, orient, **params):
    """taps [n][2][25][max_len], lens [n] -> per channel a dict of windows, paths [W], FIELDS [W]
    and zI, zQ [25][W]."""
    par = dict(DEFAULTS, **params)
    N, start = int(par["numOverLap"]), int(par["ind_start"])
    grid = {k: par[k] for k in GRID}
    chans = []
    for c, L in enumerate(int(l) for l in lens):
        W = (L - start) // N if L > start else 0
        ch = {f: np.zeros(W) for f in FIELDS}
        ch.update(windows=W, paths=np.zeros(W, dtype=np.int32), zI=np.zeros((25, W)), zQ=np.zeros((25, W)))
        for m in range(W):
            zI, zQ = coherent(taps[c, 0, :, :L], taps[c, 1, :, :L], start - 1 + m * N, N)
            ch["zI"][:, m], ch["zQ"][:, m] = zI, zQ
            for k, v in fit_vector(zI, zQ, orient, **grid).items():
                ch[k][m] = v
        chans.append(ch)
    return chans
