"""A numpy restatement of gnss_replay_ddm's definition (include/gnss_mi355x.h): the rows' times, the
rotation by numpy's own sin / cos, the signed sums and the peak rule. Independent of csrc/: no
tiling, no shared code. Tests compare the library against it within the project's tolerance and
apply its peak rule to the library's own map."""
import numpy as np


def row_times(pos_bytes, numSample, i0, R, bps, Fs):
    """t_i of rows i0 .. i0+R-1 of one channel."""
    pos = np.asarray(pos_bytes[i0: i0 + R], dtype=np.int64)
    ns = np.asarray(numSample[i0: i0 + R], dtype=np.int64)
    s = (pos - pos[0]) // bps
    return ((2 * s + ns - 1).astype(np.float64) / 2.0) / Fs


def window_map(I, Q, prompt_i, t, dopp_hz):
    """I, Q [n_taps][R] of one window, prompt_i [R] or None, t [R] -> ZI, ZQ [n_dopp][n_taps]."""
    s = np.ones(I.shape[1]) if prompt_i is None else np.where(prompt_i >= 0, 1.0, -1.0)
    th = np.asarray(dopp_hz, dtype=np.float64)[:, None] * t[None, :]
    ang = 2.0 * np.pi * (th - np.rint(th))
    cs, sn = np.cos(ang), np.sin(ang)  # [n_dopp][R]
    sI, sQ = I * s, Q * s
    return cs @ sI.T + sn @ sQ.T, cs @ sQ.T - sn @ sI.T


def ddm(taps, n_rows, pos_bytes, numSample, dopp_hz, prompt, R, bps, Fs):
    """taps [n][2][n_taps][max_rows] -> per channel an array [n_win][2][n_dopp][n_taps]."""
    out = []
    for c in range(taps.shape[0]):
        nw = int(n_rows[c]) // R
        m = np.zeros((nw, 2, len(dopp_hz), taps.shape[2]))
        for w in range(nw):
            sl = slice(w * R, (w + 1) * R)
            t = row_times(pos_bytes[c], numSample[c], w * R, R, bps, Fs)
            m[w, 0], m[w, 1] = window_map(taps[c, 0, :, sl], taps[c, 1, :, sl],
                                          None if prompt < 0 else taps[c, 0, prompt, sl], t, dopp_hz)
        out.append(m)
    return out


def peaks(zI, zQ, u, dopp_hz, excl_chips, excl_hz):
    """The peak rule on one window's map [n_dopp][n_taps] -> (peak_bin, peak_tap, peak_pow, sec_bin,
    sec_tap, sec_pow); -1 / NaN where there is no candidate."""
    P = zI * zI + zQ * zQ
    nt = P.shape[1]

    def first_max(ok):
        v = np.where(ok & ~np.isnan(P), P, -1.0).reshape(-1)  # (a power is never negative)
        k = int(np.argmax(v))  # (numpy's argmax takes the first of equals)
        return (-1, -1, np.nan) if v[k] < 0 else (k // nt, k % nt, float(v[k]))

    pb, pt, pp = first_max(np.ones(P.shape, dtype=bool))
    if pb < 0:
        return pb, pt, pp, -1, -1, np.nan
    u, hz = np.asarray(u), np.asarray(dopp_hz)
    ok = (np.abs(u - u[pt]) >= excl_chips)[None, :] | (np.abs(hz - hz[pb]) >= excl_hz)[:, None]
    return (pb, pt, pp) + first_max(ok)
