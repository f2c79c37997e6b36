"""What the tests of the multi-ray fit share (test_acf_fit_multi_kat.py on the CPU,
test_gpu_acf_fit_multi.py on the GPU): seeded sums with two rays in gnss_replay_out.taps' layout,
the case list, the call through the C-ABI with host or uploaded sums, gnss_acf_fit_multi_window on
one vector, model vectors and the bit-for-bit comparisons."""
import ctypes as C
from types import SimpleNamespace as NS

import numpy as np

import acf_fit_multi_twin as T
from acf_common import same_bits

P = T.MAX_PATHS
WIDE = np.round(np.arange(-50, 21) * 0.05, 2)  # -2.5:0.05:1.0, 71 taps, the prompt at index 50
RAYS = ((0.6, 0.5, 0.5), (1.4, 0.4, 0.25))     # (chips late, amplitude ratio, phase in cycles)


def grid_u(n_taps, prompt, spacing=0.05):
    """the uniform grid with u = 0 at `prompt`"""
    return (np.arange(n_taps) - float(prompt)) * spacing


def sums(n_taps, prompt, n_rows, max_rows, u=None, seed=17):
    """Seeded sums [n][2][n_taps][max_rows]: per row a triangle about u = 0 and RAYS' two behind it,
    all on a random carrier phase, the data bit's sign on the whole row, plus noise; junk past
    n_rows that nothing may read into a result."""
    n_rows = np.asarray(n_rows, dtype=np.int64)
    n = len(n_rows)
    u = grid_u(n_taps, prompt) if u is None else np.asarray(u, dtype=np.float64)
    rng = np.random.default_rng(seed)
    shape = T.tri(u).astype(np.complex128)
    for late, ratio, cyc in RAYS:
        shape += ratio * np.exp(2j * np.pi * cyc) * T.tri(u + late)
    shape *= 4000.0
    if not shape[prompt]:
        shape[prompt] = 4000.0  # (a grid with no tap near 0: the signs still follow the bits)
    ph = rng.uniform(-0.3, 0.3, (n, 1, max_rows))
    bit = rng.choice([-1.0, 1.0], (n, 1, max_rows))
    taps = rng.normal(0, 300.0, (n, 2, n_taps, max_rows))
    z = bit * shape[None, :, None] * np.exp(1j * ph)
    taps[:, 0] += z.real
    taps[:, 1] += z.imag
    for c in range(n):
        taps[c, :, :, n_rows[c]:] = 1e30
    return NS(taps=np.ascontiguousarray(taps), n_rows=n_rows, max_rows=int(max_rows), n=n, n_taps=int(n_taps),
              prompt=int(prompt), u=np.ascontiguousarray(u))


EDGE = ([513, 512, 511], 514)  # the last windows end close to the series' end
# name: (n_taps, prompt, tap spacing, (n_rows, max_rows), numOverLap, ind_start, the search, windows).
# Between them: n_taps 1, 25, 61, 65 (a series group of the kernel's stage 1 and one tap more), 256;
# q_count 1, 255, 257 (a block's lanes less and plus one), 281, 4096; max_paths 1..4; sweeps 0, 1, 4;
# sep_min 1, 5; windows of 2, 64, 65, 100 and 4096 rows; the edge lens; a long channel beside a short one.
CASES = {
    "1tap": (1, 0, 0.05, EDGE, 2, 1, dict(q_min=0.0, q_step=0.1, q_count=1, max_paths=2, sweeps=1, sep_min=1),
             [256, 255, 255]),
    "25taps": (25, 12, 0.05, EDGE, 65, 7, dict(q_min=-0.6, q_step=0.005, q_count=255, max_paths=3), [7, 7, 7]),
    "61taps-long-short": (61, 40, 0.05, ([1001, 101], 1003), 100, 1, {}, [10, 1]),
    "65taps": (65, 44, 0.05, ([300, 131], 301), 64, 7,
               dict(q_min=-2.1, q_step=0.01, q_count=257, max_paths=4, sweeps=1), [4, 1]),
    "61taps-greedy": (61, 40, 0.05, ([37, 12], 40), 2, 1, dict(max_paths=4, sweeps=0, sep_min=1), [18, 5]),
    "25taps-one-path": (25, 12, 0.05, ([200], 201), 64, 1, dict(q_min=-1.4, max_paths=1), [3]),
    "256taps-widest-window": (256, 200, 0.0125, ([8200], 8201), 4096, 1,
                              dict(q_min=-2.4, q_step=0.0007, q_count=4096, max_paths=4, sweeps=1), [2]),
}


def case(name):
    """-> (sums, the parameters of the call, the windows per channel)"""
    n_taps, prompt, spacing, (n_rows, max_rows), numOverLap, ind_start, search, windows = CASES[name]
    s = sums(n_taps, prompt, n_rows, max_rows, u=grid_u(n_taps, prompt, spacing))
    return s, dict(search, numOverLap=numOverLap, ind_start=ind_start), windows


def c_cfg(pkg, n, u, prompt, flags=0, n_taps=None, **params):
    """-> (cfg, what must stay alive)"""
    par = dict(T.DEFAULTS, **params)
    cfg = pkg.abi.GnssAcfFitMultiCfg()
    uu = None if u is None else np.ascontiguousarray(u, dtype=np.float64)
    cfg.n, cfg.prompt, cfg.flags = n, prompt, flags
    cfg.n_taps = (0 if uu is None else len(uu)) if n_taps is None else n_taps
    cfg.u = None if uu is None else uu.ctypes.data
    for k, v in par.items():
        setattr(cfg, k, v)
    return cfg, uu


class OutBuffers:
    """Caller-allocated gnss_acf_fit_multi_out: `cap` windows per channel, filled with values no
    fit writes so that an unwritten element shows."""

    def __init__(self, pkg, n, cap, n_taps, want=True):
        self.n, self.cap = n, cap
        nn, cc = max(n, 1), max(cap, 1)
        self.windows = np.full(nn, -1, dtype=np.int64)
        self.ints = {f: np.full((nn, cc), -9, dtype=np.int32) for f in ("paths", "searches")}
        self.arr = {f: np.full((nn, cc), -7.0) for f in T.SCALARS}
        self.arr.update({f: np.full((nn, P, cc), -7.0) for f in T.VECTORS})
        self.arr["res"] = np.full((nn, P + 1, cc), -7.0)
        o = pkg.abi.GnssAcfFitMultiOut()
        o.cap = cap
        o.windows = self.windows.ctypes.data_as(C.POINTER(C.c_int64))
        for f, a in self.ints.items():
            setattr(o, f, a.ctypes.data_as(C.POINTER(C.c_int32)))
        for f, a in self.arr.items():
            setattr(o, f, a.ctypes.data_as(C.POINTER(C.c_double)))
        self.zI = self.zQ = None
        if want:
            zs = (nn, max(n_taps, 1), cc)
            self.zI, self.zQ = np.full(zs, -7.0), np.full(zs, -7.0)
            o.zI = self.zI.ctypes.data_as(C.POINTER(C.c_double))
            o.zQ = self.zQ.ctypes.data_as(C.POINTER(C.c_double))
        self.c = o

    @property
    def paths(self):
        return self.ints["paths"]

    @property
    def searches(self):
        return self.ints["searches"]

    def untouched(self):
        return (self.windows == -1).all() and all((a == -9).all() for a in self.ints.values()) and all(
            (a == -7.0).all() for a in self.arr.values()) and (self.zI is None or ((self.zI == -7.0).all() and
                                                                                  (self.zQ == -7.0).all()))


def cap_of(s, **params):
    par = dict(T.DEFAULTS, **params)
    return max([max(int(l) - par["ind_start"], 0) // par["numOverLap"] for l in s.n_rows] + [1])


def lib_run(pkg, s, *, ctx=None, dev=None, want=True, cap=None, n=None, u="own", prompt=None, n_taps=None,
            flags=None, taps="own", n_rows="own", max_rows=None, **params):
    """gnss_acf_fit_multi on the sums s (dev: the device pointer of an uploaded copy) ->
    (status, OutBuffers); the keywords replace single arguments for the refusal tests."""
    lib = pkg.abi.load()
    n = s.n if n is None else n
    cfg, keep = c_cfg(pkg, n, s.u if isinstance(u, str) else u, s.prompt if prompt is None else prompt,
                      (pkg.abi.OUT_DEVICE if dev is not None else 0) if flags is None else flags, n_taps, **params)
    src = pkg.abi.GnssAcfFitTapsIn()
    nr = s.n_rows if isinstance(n_rows, str) else n_rows
    src.taps = (s.taps.ctypes.data if dev is None else dev) if isinstance(taps, str) else taps
    src.max_rows = s.max_rows if max_rows is None else max_rows
    src.n_rows = None if nr is None else nr.ctypes.data
    win = {k: v for k, v in params.items() if k in ("ind_start", "numOverLap")}
    out = OutBuffers(pkg, max(n, 0), cap_of(s, **win) if cap is None else cap, s.n_taps, want)
    st = lib.gnss_acf_fit_multi(ctx.h if ctx is not None else None, C.byref(cfg), C.byref(src), C.byref(out.c))
    return st, out


def fit_window(pkg, zI, zQ, u, prompt=0, **params):
    """gnss_acf_fit_multi_window on one coherent vector -> (status, dict as the twin's fit_vector)."""
    zI, zQ = np.ascontiguousarray(zI, dtype=np.float64), np.ascontiguousarray(zQ, dtype=np.float64)
    out = OutBuffers(pkg, 1, 1, len(zI))
    cfg, keep = c_cfg(pkg, 1, u, prompt, **params)
    st = pkg.abi.load().gnss_acf_fit_multi_window(C.byref(cfg), zI.ctypes.data_as(C.POINTER(C.c_double)),
                                                  zQ.ctypes.data_as(C.POINTER(C.c_double)), C.byref(out.c))
    got = {f: out.arr[f][0, ..., 0].copy() for f in T.FIELDS}
    got["paths"], got["searches"] = int(out.paths[0, 0]), int(out.searches[0, 0])
    if st == pkg.abi.OK:
        assert out.windows[0] == 1 and same_bits(out.zI[0, :, 0], zI) and same_bits(out.zQ[0, :, 0], zQ)
    return st, got


def same_vector(got, tw):
    """a fit_window result against the twin's fit_vector, bit for bit"""
    return got["paths"] == tw["paths"] and got["searches"] == tw["searches"] and all(
        same_bits(np.asarray(got[f]), np.asarray(tw[f])) for f in T.FIELDS)


def model(u, paths):
    """z[j] = sum over (q, A) of A R(u[j] - q) -> zI, zQ"""
    u = np.asarray(u, dtype=np.float64)
    z = sum(A * T.tri(u - q) for q, A in paths)
    return np.real(z).copy(), np.imag(z).copy()


def assert_equals_twin(out, chans):
    """Every output of the written windows bit for bit; the elements past them untouched."""
    for c, ch in enumerate(chans):
        W = ch["windows"]
        assert out.windows[c] == W, (c, out.windows[c], W)
        for f, a in out.ints.items():
            assert np.array_equal(a[c, :W], ch[f]), (c, f, a[c, :W], ch[f])
            assert np.all(a[c, W:] == -9), (c, f)
        for f in T.FIELDS:
            assert same_bits(out.arr[f][c, ..., :W], ch[f]), (c, f, out.arr[f][c, ..., :W], ch[f])
            assert np.all(out.arr[f][c, ..., W:] == -7.0), (c, f)
        if out.zI is not None:
            assert same_bits(out.zI[c, :, :W], ch["zI"]) and same_bits(out.zQ[c, :, :W], ch["zQ"]), c
            assert np.all(out.zI[c, :, W:] == -7.0) and np.all(out.zQ[c, :, W:] == -7.0), c


def assert_same_outputs(a, b):
    """Two OutBuffers (host path, device path) bit for bit in every element, written or not."""
    assert np.array_equal(a.windows, b.windows)
    for f in a.ints:
        assert np.array_equal(a.ints[f], b.ints[f]), f
    for f in T.FIELDS:
        assert same_bits(a.arr[f], b.arr[f]), f
    if a.zI is not None and b.zI is not None:
        assert same_bits(a.zI, b.zI) and same_bits(a.zQ, b.zQ)
