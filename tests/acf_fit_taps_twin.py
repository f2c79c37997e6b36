"""A numpy restatement of the two-path fit on any tap grid (gnss_acf_fit_taps: the definition of
gnss_acf_fit in include/gnss_mi355x.h with n_taps, prompt and u[j] given by the caller),
independent of csrc/ and of the 25-tap twin: vectorised over the hypotheses of a grid, every sum
explicitly left to right from its first term (np.add.accumulate, never np.sum, whose pairwise
blocks round differently). This restatement is what the library is held to, bit for bit."""
import numpy as np

DEFAULTS = dict(ind_start=1, numOverLap=100, p_min=-0.40, p_step=0.01, p_count=81, e_min=0.05, e_step=0.01,
                e_count=196, ratio_max=1.0, gain_min=16.0)
FIELDS = ["bias", "p1", "A1p_re", "A1p_im", "res1", "p0", "e", "A0_re", "A0_im", "A1_re", "A1_im", "res2", "energy"]
GRID = ("p_min", "p_step", "p_count", "e_min", "e_step", "e_count", "ratio_max", "gain_min")


def left_sum(x):
    """the last axis summed left to right from its first element"""
    return np.add.accumulate(x, axis=-1)[..., -1]


def tri(x):
    """R(x) = max(0, 1 - |x|)"""
    t = 1.0 - np.abs(x)
    return np.where(t > 0, t, 0.0)


def lowest(res, alive):
    """the index of the smallest res among the hypotheses that survived, the lowest index on a
    tie; a NaN res never wins; None when nothing is left"""
    idx = np.flatnonzero(alive & (res <= np.inf))  # (the comparison is false for a NaN)
    return int(idx[np.argmin(res[idx])]) if len(idx) else None  # (argmin: the first of equal minima)


def coherent_sums(I, Q, prompt, row, N):
    """I / Q [n_taps][L] -> zI, zQ [n_taps] of the N rows from `row`, each row signed by the
    prompt tap's I of that row (>= 0: +1, otherwise and for a NaN -1)"""
    wI, wQ = I[:, row: row + N], Q[:, row: row + N]
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.where(wI[prompt] >= 0, 1.0, -1.0)
        return left_sum(s * wI), left_sum(s * wQ)


def fit_vector(zI, zQ, u, *, p_min, p_step, p_count, e_min, e_step, e_count, ratio_max, gain_min, chunk=4096):
    """One coherent vector at the coordinates u -> dict of paths and FIELDS."""
    zI, zQ, u = (np.asarray(a, dtype=np.float64) for a in (zI, zQ, u))
    out = dict.fromkeys(FIELDS, np.nan)
    out["paths"] = 0
    if not (np.isfinite(zI).all() and np.isfinite(zQ).all()):
        return out
    p = p_min + np.arange(p_count, dtype=np.float64) * p_step
    e = e_min + np.arange(e_count, dtype=np.float64) * e_step
    with np.errstate(all="ignore"):
        # the one-path grid
        r = tri(u[None, :] - p[:, None])
        a = left_sum(r * r)
        Are, Aim = left_sum(r * zI) / a, left_sum(r * zQ) / a
        dI, dQ = zI - Are[:, None] * r, zQ - Aim[:, None] * r
        res1 = left_sum(dI * dI + dQ * dQ)
        i1 = lowest(res1, a != 0)
        if i1 is None:
            return out
        out.update(paths=1, p1=p[i1], A1p_re=Are[i1], A1p_im=Aim[i1], res1=res1[i1],
                   energy=left_sum(zI * zI + zQ * zQ))
        # the two-path grid, h = ip * e_count + ie, in chunks of hypotheses (the memory of a wide grid)
        H = p_count * e_count
        cols = {k: np.empty(H) for k in ("A0_re", "A0_im", "A1_re", "A1_im", "res2")}
        alive = np.empty(H, dtype=bool)
        for lo in range(0, H, chunk):
            h = np.arange(lo, min(lo + chunk, H))
            ph, eh = p[h // e_count], e[h % e_count]
            qh = ph - eh
            r0, r1 = tri(u[None, :] - ph[:, None]), tri(u[None, :] - qh[:, None])
            a, b, c = left_sum(r0 * r0), left_sum(r1 * r1), left_sum(r0 * r1)
            h0I, h0Q, h1I, h1Q = left_sum(r0 * zI), left_sum(r0 * zQ), left_sum(r1 * zI), left_sum(r1 * zQ)
            det = a * b - c * c
            ok = (a != 0) & (b != 0) & (det > (1e-9 * a) * b)
            A0re, A0im = (b * h0I - c * h1I) / det, (b * h0Q - c * h1Q) / det
            A1re, A1im = (a * h1I - c * h0I) / det, (a * h1Q - c * h0Q) / det
            m0, m1 = A0re * A0re + A0im * A0im, A1re * A1re + A1im * A1im
            ok &= ~(m1 > (ratio_max * ratio_max) * m0)
            dI = (zI - A0re[:, None] * r0) - A1re[:, None] * r1
            dQ = (zQ - A0im[:, None] * r0) - A1im[:, None] * r1
            cols["res2"][h] = left_sum(dI * dI + dQ * dQ)
            cols["A0_re"][h], cols["A0_im"][h], cols["A1_re"][h], cols["A1_im"][h] = A0re, A0im, A1re, A1im
            alive[h] = ok
        i2 = lowest(cols["res2"], alive)
        if i2 is not None:
            out.update(p0=p[i2 // e_count], e=e[i2 % e_count], **{k: v[i2] for k, v in cols.items()})
            if out["res1"] > gain_min * out["res2"]:
                out["paths"] = 2
    out["bias"] = out["p0"] if out["paths"] == 2 else out["p1"]
    return out


def fit(taps, n_rows, u, prompt, **params):
    """taps [n][2][n_taps][max_rows], n_rows [n] -> per channel a dict of windows, paths [W],
    FIELDS [W] and zI, zQ [n_taps][W]."""
    par = dict(DEFAULTS, **params)
    N, start = int(par["numOverLap"]), int(par["ind_start"])
    grid = {k: par[k] for k in GRID}
    nt = len(u)
    chans = []
    for c, L in enumerate(int(x) for x in n_rows):
        W = (L - start) // N if L > start else 0
        ch = {f: np.zeros(W) for f in FIELDS}
        ch.update(windows=W, paths=np.zeros(W, dtype=np.int32), zI=np.zeros((nt, W)), zQ=np.zeros((nt, W)))
        for m in range(W):
            zI, zQ = coherent_sums(taps[c, 0], taps[c, 1], prompt, start - 1 + m * N, N)
            ch["zI"][:, m], ch["zQ"][:, m] = zI, zQ
            for k, v in fit_vector(zI, zQ, u, **grid).items():
                ch[k][m] = v
        chans.append(ch)
    return chans
