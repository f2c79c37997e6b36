"""A numpy restatement of the multi-ray fit on any tap grid (gnss_acf_fit_multi: the definition in
include/gnss_mi355x.h, the order of the elimination's operations as csrc/acf_fit_multi.h's head
fixes it), independent of csrc/ and of the other twins: vectorised over the candidates of a search,
every sum explicitly left to right from its first term (np.add.accumulate, never np.sum, whose
pairwise blocks round differently). This restatement is what the library is held to, bit for bit,
`searches` included."""
import numpy as np

MAX_PATHS = 4
DEFAULTS = dict(ind_start=1, numOverLap=100, q_min=-2.40, q_step=0.01, q_count=281, max_paths=3, sweeps=4, sep_min=5,
                gain_min=16.0)
SEARCH = ("q_min", "q_step", "q_count", "max_paths", "sweeps", "sep_min", "gain_min")
SCALARS = ["bias", "energy"]          # [W] per channel
VECTORS = ["q", "A_re", "A_im"]       # [4][W]
FIELDS = SCALARS + VECTORS + ["res"]  # res: [5][W]


def left_sum(x):
    """the last axis summed left to right from its first element"""
    return np.add.accumulate(x, axis=-1)[..., -1]


def tri(x):
    """R(x) = max(0, 1 - |x|)"""
    t = 1.0 - np.abs(x)
    return np.where(t > 0, t, 0.0)


def coherent_sums(I, Q, prompt, row, N):
    """I / Q [n_taps][L] -> zI, zQ [n_taps] of the N rows from `row`, each row signed by the
    prompt tap's I of that row (>= 0: +1, otherwise and for a NaN -1)"""
    wI, wQ = I[:, row: row + N], Q[:, row: row + N]
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.where(wI[prompt] >= 0, 1.0, -1.0)
        return left_sum(s * wI), left_sum(s * wQ)


def joint(R, k, zI, zQ):
    """The joint fit of the slots' r vectors R (a list of m arrays [1 or C][n], slot order; slot k
    is the one whose usability counts) -> ok [C], A_re, A_im (lists of m arrays [C]), res [C]."""
    m = len(R)
    G = [[None] * m for _ in range(m)]
    for a in range(m):
        for b in range(a, m):
            G[a][b] = G[b][a] = left_sum(R[a] * R[b])
    hI = [left_sum(R[a] * zI) for a in range(m)]
    hQ = [left_sum(R[a] * zQ) for a in range(m)]
    g0 = [G[a][a] for a in range(m)]
    ok = g0[k] != 0
    for e in range(m):
        d = G[e][e]
        ok = ok & (d > (1e-9 * g0[e]))
        for i in range(e + 1, m):
            f = G[i][e] / d
            for l in range(e + 1, m):
                G[i][l] = G[i][l] - f * G[e][l]
            hI[i] = hI[i] - f * hI[e]
            hQ[i] = hQ[i] - f * hQ[e]
    A_re, A_im = [None] * m, [None] * m
    for e in range(m - 1, -1, -1):
        sI, sQ = hI[e], hQ[e]
        for l in range(e + 1, m):
            sI = sI - G[e][l] * A_re[l]
            sQ = sQ - G[e][l] * A_im[l]
        A_re[e], A_im[e] = sI / G[e][e], sQ / G[e][e]
    dI, dQ = zI, zQ
    for l in range(m):
        dI = dI - np.reshape(A_re[l], (-1, 1)) * R[l]
        dQ = dQ - np.reshape(A_im[l], (-1, 1)) * R[l]
    res = left_sum(dI * dI + dQ * dQ)
    shape = np.broadcast(ok, res).shape
    return np.broadcast_to(ok, shape), A_re, A_im, np.broadcast_to(res, shape)


def fit_vector(zI, zQ, u, *, q_min, q_step, q_count, max_paths, sweeps, sep_min, gain_min):
    """One coherent vector at the coordinates u -> dict of paths, searches, bias, energy, q / A_re /
    A_im [4] and res [5]."""
    zI, zQ, u = (np.asarray(a, dtype=np.float64) for a in (zI, zQ, u))
    nan = np.nan
    out = dict(paths=0, searches=0, bias=nan, energy=nan, q=np.full(MAX_PATHS, nan), A_re=np.full(MAX_PATHS, nan),
               A_im=np.full(MAX_PATHS, nan), res=np.full(MAX_PATHS + 1, nan))
    if not (np.isfinite(zI).all() and np.isfinite(zQ).all()):
        return out
    idx = np.arange(q_count)
    q = q_min + idx.astype(np.float64) * q_step
    cand = tri(u[None, :] - q[:, None])  # [q_count][n]
    pos, kept, res = [], {}, [None] * (MAX_PATHS + 1)
    searches = 0

    def search(m, k):
        """Search(k) among m slots -> (winner or None, its res); the winner placed"""
        R = [cand if l == k else cand[pos[l]][None, :] for l in range(m)]
        ok, _, _, r = joint(R, k, zI, zQ)
        alive = ok.copy()
        for l in range(m):
            if l != k:
                alive &= ~(np.abs(idx - pos[l]) < sep_min)
        live = np.flatnonzero(alive & (r <= np.inf))  # (false for a NaN)
        if not len(live):
            return None, None
        win = int(live[np.argmin(r[live])])  # (argmin: the first, so the lowest index, of equal minima)
        pos[k] = win
        return win, r[win]

    with np.errstate(all="ignore"):
        res[0] = out["energy"] = left_sum(zI * zI + zQ * zQ)
        formed = 0
        for m in range(1, max_paths + 1):
            pos.append(0)
            searches += 1
            win, r_m = search(m, m - 1)
            if win is None:
                pos.pop()
                break
            for _ in range(sweeps):
                moved = False
                for k in range(m):
                    before = pos[k]
                    searches += 1
                    win, r = search(m, k)
                    if win is not None:
                        r_m = r
                        moved = moved or win != before
                if not moved:
                    break
            kept[m], res[m], formed = list(pos), r_m, m
        out["searches"] = searches
        for m in range(formed + 1):
            out["res"][m] = res[m]
        sel = 1 if formed else 0
        for m in range(1, formed + 1):
            if res[m - 1] > gain_min * res[m]:
                sel = m
        out["paths"] = sel
        if sel:
            at = kept[sel]
            _, A_re, A_im, _ = joint([cand[i][None, :] for i in at], 0, zI, zQ)
            for rank, a in enumerate(sorted(range(sel), key=lambda a: -at[a])):
                out["q"][rank], out["A_re"][rank], out["A_im"][rank] = q[at[a]], A_re[a][0], A_im[a][0]
            out["bias"] = out["q"][0]
    return out


def fit(taps, n_rows, u, prompt, **params):
    """taps [n][2][n_taps][max_rows], n_rows [n] -> per channel a dict of windows, paths and
    searches [W], bias and energy [W], q / A_re / A_im [4][W], res [5][W] and zI, zQ [n_taps][W]."""
    par = dict(DEFAULTS, **params)
    N, start = int(par["numOverLap"]), int(par["ind_start"])
    search = {k: par[k] for k in SEARCH}
    nt = len(u)
    chans = []
    for c, L in enumerate(int(x) for x in n_rows):
        W = (L - start) // N if L > start else 0
        ch = dict(windows=W, paths=np.zeros(W, dtype=np.int32), searches=np.zeros(W, dtype=np.int32),
                  bias=np.zeros(W), energy=np.zeros(W), res=np.zeros((MAX_PATHS + 1, W)), zI=np.zeros((nt, W)),
                  zQ=np.zeros((nt, W)))
        ch.update({f: np.zeros((MAX_PATHS, W)) for f in VECTORS})
        for m in range(W):
            zI, zQ = coherent_sums(taps[c, 0], taps[c, 1], prompt, start - 1 + m * N, N)
            ch["zI"][:, m], ch["zQ"][:, m] = zI, zQ
            for k, v in fit_vector(zI, zQ, u, **search).items():
                ch[k][..., m] = v
        chans.append(ch)
    return chans
