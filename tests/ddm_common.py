"""What the delay-Doppler map's CPU and GPU tests share: seeded sums and row tables, the call with
raw structs (refusals) and through sdr.replay_ddm, the twin's reference (computed once per shape),
the refusal table and the end-to-end scene with its four conditions."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np

import ddm_twin as twin
import replay_common as rc

FS = rc.FS
FILE = SimpleNamespace(dataPrecision=1, dataType=2)
SIGNAL = SimpleNamespace(Fs=FS)


def table(n_rows, max_rows, seed=0):
    """A replay table's time columns for channels of n_rows rows: rows of 2047..2051 samples that
    follow each other with gaps of 0..3 samples (I/Q int8: 2 bytes per sample)."""
    rng = np.random.Generator(np.random.PCG64(7100 + seed))
    n = len(n_rows)
    ns = rng.integers(2047, 2052, (n, max_rows)).astype(np.int64)
    gap = rng.integers(0, 4, (n, max_rows)).astype(np.int64)
    pos = 64 + 2 * (np.cumsum(ns + gap, axis=1) - ns - gap)
    return SimpleNamespace(n_rows=np.asarray(n_rows, dtype=np.int64), max_rows=max_rows, pos_bytes=pos, numSample=ns)


@functools.lru_cache(maxsize=None)
def sums(n, nt, max_rows):
    """Random sums [n][2][nt][max_rows] around a scale of 1000."""
    rng = np.random.Generator(np.random.PCG64(7200 + 1000 * n + nt))
    return rng.standard_normal((n, 2, nt, max_rows)) * 1000.0


def bins(nd):
    """nd Doppler offsets from -500 Hz in steps of 7.3 Hz (256 of them: up to 1361.5 Hz), not in order
    at the ends so that no ordering is assumed."""
    hz = -500.0 + 7.3 * np.arange(nd)
    if nd > 2:
        hz[[0, -1]] = hz[[-1, 0]]
    return hz


def shape(R, nt, nd, prompt, n_rows=None):
    """The inputs of one case: channels with 2 windows + a remainder, 1 window and no row at all."""
    n_rows = [2 * R + 1, R, 0] if n_rows is None else n_rows
    mr = max(max(n_rows), 1) + 2
    return SimpleNamespace(R=R, nt=nt, nd=nd, prompt=min(prompt, nt - 1), tab=table(n_rows, mr, seed=R),
                           taps=sums(len(n_rows), nt, mr), hz=bins(nd), u=rc.taps_n(nt))


_REF = {}


def twin_ref(s):
    key = (s.R, s.nt, s.nd, s.prompt, tuple(s.tab.n_rows))
    if key not in _REF:
        _REF[key] = twin.ddm(s.taps, s.tab.n_rows, s.tab.pos_bytes, s.tab.numSample, s.hz, s.prompt, s.R, 2, FS)
    return _REF[key]


def run(pkg, s, taps=None, ctx=None, **kw):
    return pkg.replay_ddm(s.taps if taps is None else taps, s.tab, s.hz, u=s.u, prompt=s.prompt, rows_per_window=s.R,
                          signal=SIGNAL, file=FILE, ctx=ctx, **kw)


def rel_err(got, ref):
    """The largest difference over all channels' windows, relative to the largest reference magnitude."""
    worst = max([float(np.max(np.abs(g - r), initial=0.0)) for g, r in zip(got, ref)])
    top = max([float(np.max(np.abs(r), initial=0.0)) for r in ref])
    return worst / max(top, 1.0)


PEAK_FIELDS = ("peak_bin", "peak_tap", "peak_pow", "sec_bin", "sec_tap", "sec_pow")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_result(a, b, with_map=True):
    """Every output of two runs, bit for bit."""
    ok = list(a.n_win) == list(b.n_win)
    for c in range(len(a.n_win)):
        ok = ok and all(same_bits(getattr(a, f)[c], getattr(b, f)[c]) for f in PEAK_FIELDS)
        if with_map:
            ok = ok and same_bits(a.map[c], b.map[c])
    return ok


def peaks_follow_the_twins_rule(res, excl_chips=0.3, excl_hz=10.0):
    """The twin's peak rule applied to the result's own map gives the result's peaks, exactly."""
    for c in range(len(res.n_win)):
        for w in range(int(res.n_win[c])):
            want = twin.peaks(res.map[c][w, 0], res.map[c][w, 1], res.u, res.dopp_hz, excl_chips, excl_hz)
            got = tuple(getattr(res, f)[c][w] for f in PEAK_FIELDS)
            for g, x in zip(got, want):
                if not (g == x or (np.isnan(g) and np.isnan(x))):
                    return False, (c, w, got, want)
    return True, None


# ---- the raw call, for the refusals ----------------------------------------------------------------
def raw_call(pkg, ctx, mutate=None, taps_ptr=None, flags=0, map_ptr=None):
    """One gnss_replay_ddm call on a small good case after mutate(kw) -> (status, outputs untouched).
    kw: the cfg / in / out structs and the arrays behind them."""
    abi = pkg.abi
    s = shape(4, 5, 3, 2, n_rows=[9, 4])
    n, cap = 2, 2
    kw = dict(cfg=abi.GnssReplayDdmCfg(), src=abi.GnssReplayDdmIn(), out=abi.GnssReplayDdmOut(),
              hz=s.hz.copy(), u=s.u.copy(), n_rows=s.tab.n_rows.copy(), pos=s.tab.pos_bytes.copy(),
              ns=s.tab.numSample.copy(), taps=s.taps)
    cfg, src, out = kw["cfg"], kw["src"], kw["out"]
    cfg.n, cfg.n_taps, cfg.prompt, cfg.rows_per_window, cfg.n_dopp, cfg.flags = n, s.nt, s.prompt, s.R, s.nd, flags
    cfg.excl_chips, cfg.excl_hz, cfg.Fs, cfg.bytes_per_sample = 0.3, 10.0, FS, 2
    cfg.dopp_hz, cfg.u = kw["hz"].ctypes.data, kw["u"].ctypes.data
    src.taps = kw["taps"].ctypes.data if taps_ptr is None else taps_ptr
    src.max_rows = s.tab.max_rows
    src.n_rows, src.pos_bytes, src.numSample = kw["n_rows"].ctypes.data, kw["pos"].ctypes.data, kw["ns"].ctypes.data
    keep = dict(map=np.full((n, cap, 2, s.nd, s.nt), 7.25), n_win=np.full(n, 77, dtype=np.int64))
    for f in PEAK_FIELDS:
        keep[f] = np.full((n, cap), 7.25) if f.endswith("pow") else np.full((n, cap), 77, dtype=np.int32)
    out.cap = cap
    for f, a in keep.items():
        setattr(out, f, a.ctypes.data)
    if map_ptr is not None:
        out.map = map_ptr
    before = {f: a.copy() for f, a in keep.items()}
    args = [C.byref(cfg), C.byref(src), C.byref(out)]
    if mutate is not None:
        mutate(kw, args)
    st = abi.load().gnss_replay_ddm(ctx.h if ctx is not None else None, *args)
    return st, all(same_bits(keep[f], before[f]) for f in keep)


def refusals(abi):
    """(name, status, mutate(kw, args)): one per line of the refusal list, host or device path alike."""
    def cfg(field, value):
        def f(kw, args):
            setattr(kw["cfg"], field, value)
        return f

    def src(field, value):
        def f(kw, args):
            setattr(kw["src"], field, value)
        return f

    def out(field, value):
        def f(kw, args):
            setattr(kw["out"], field, value)
        return f

    def arr(name, index, value):
        def f(kw, args):
            kw[name][index] = value
        return f

    def null_arg(k):
        def f(kw, args):
            args[k] = None
        return f

    E, IO = abi.EARG, abi.EIO
    return [
        ("cfg null", E, null_arg(0)), ("in null", E, null_arg(1)), ("out null", E, null_arg(2)),
        ("taps null", E, src("taps", None)), ("n_rows null", E, src("n_rows", None)),
        ("pos_bytes null", E, src("pos_bytes", None)), ("numSample null", E, src("numSample", None)),
        ("dopp_hz null", E, cfg("dopp_hz", None)), ("u null", E, cfg("u", None)),
        ("peak_bin null", E, out("peak_bin", None)), ("sec_pow null", E, out("sec_pow", None)),
        ("n_win null", E, out("n_win", None)),
        ("n 0", E, cfg("n", 0)), ("n 65", E, cfg("n", 65)),
        ("n_taps 0", E, cfg("n_taps", 0)), ("n_taps 257", E, cfg("n_taps", 257)),
        ("prompt -2", E, cfg("prompt", -2)), ("prompt n_taps", E, cfg("prompt", 5)),
        ("rows_per_window 1", E, cfg("rows_per_window", 1)), ("rows_per_window 4097", E, cfg("rows_per_window", 4097)),
        ("n_dopp 0", E, cfg("n_dopp", 0)), ("n_dopp 257", E, cfg("n_dopp", 257)),
        ("dopp_hz nan", E, arr("hz", 1, np.nan)), ("dopp_hz inf", E, arr("hz", 1, np.inf)),
        ("dopp_hz over 1e5", E, arr("hz", 2, -100000.5)),
        ("u nan", E, arr("u", 0, np.nan)), ("u inf", E, arr("u", 4, -np.inf)),
        ("excl_chips negative", E, cfg("excl_chips", -0.1)), ("excl_hz nan", E, cfg("excl_hz", np.nan)),
        ("Fs 0", E, cfg("Fs", 0.0)), ("Fs inf", E, cfg("Fs", np.inf)),
        ("bytes_per_sample 3", E, cfg("bytes_per_sample", 3)), ("bytes_per_sample 0", E, cfg("bytes_per_sample", 0)),
        ("max_rows 0", E, src("max_rows", 0)),
        ("n_rows negative", E, arr("n_rows", 1, -1)), ("n_rows over max_rows", E, arr("n_rows", 0, 12)),
        ("more windows than cap", E, out("cap", 1)), ("cap negative", E, out("cap", -1)),
        ("numSample 0 in a window", E, arr("ns", (0, 5), 0)),
        ("unknown flag", E, cfg("flags", 4)), ("map flag without the device flag", E, cfg("flags", abi.DDM_MAP_DEVICE)),
        ("device input without a context or of host memory", E, cfg("flags", abi.OUT_DEVICE)),
        ("pos not a multiple of the sample size", IO, arr("pos", (0, 6), 64 + 2 * 100000 + 1)),
        ("pos decreases within a window", IO, arr("pos", (1, 2), 66)),
        ("pos negative", IO, arr("pos", (0, 0), -2)),
    ]


# ---- end to end ------------------------------------------------------------------------------------
E2E_HZ = np.arange(-50.0, 51.0, 10.0)
RAY_HZ = 20.0
# The direct path's own triangle is 1 - |u| at 0 Hz: 0.7 at the edge of an exclusion box of 0.3 chip,
# above any ray of gain 0.5. The secondary-peak condition therefore runs on a third scene whose ray
# has gain 0.8 (0.8 * sinc(0.02) = 0.7995 against 0.7 + the clean scene's 0.03); the box, the rule and
# the other three conditions' scene (gain 0.5) are the issue's.
E2E_GAINS = (None, 0.5, 0.8)


def e2e_scene(pkg, gain):
    """replay_common.e2e_scene's scene; with a gain its ray, 0.9 chip late, with a carrier 20 Hz above
    the direct one."""
    sc, A = rc.e2e_scene(pkg, False)
    if gain is not None:
        pkg.synth.add_ray(sc, 16, 0.9, gain, phase_cycles=0.25, fade_hz=RAY_HZ)
    return sc, A


def e2e_check(taps, res):
    """The end-to-end conditions on the maps of rows 150-249 (one window of 100 rows, over which bins
    10 Hz apart are orthogonal), res[gain] for gain in E2E_GAINS; returns the figures."""
    k = lambda v: int(np.argmin(np.abs(taps - v)))  # noqa: E731
    b = lambda v: int(np.argmin(np.abs(E2E_HZ - v)))  # noqa: E731

    def m_of(r):
        z = np.hypot(r.map[0][0, 0], r.map[0][0, 1])  # [bins][taps]
        return z / z[b(0.0), k(0.0)]

    mc, mr, ms = m_of(res[None]), m_of(res[0.5]), m_of(res[0.8])
    strong = res[0.8]
    fig = dict(ray_at_plus=float(mr[b(RAY_HZ), k(-0.9)]), ray_at_minus=float(mr[b(-RAY_HZ), k(-0.9)]),
               clean_off_zero=float(np.max(mc[E2E_HZ != 0])), sec_gain_05=(float(res[0.5].sec_chips[0][0]), float(res[0.5].sec_hz[0][0])),
               strong_at_plus=float(ms[b(RAY_HZ), k(-0.9)]), strong_flank=float(ms[b(0.0), k(-0.3)]),
               peak=(float(strong.peak_chips[0][0]), float(strong.peak_hz[0][0])),
               sec=(float(strong.sec_chips[0][0]), float(strong.sec_hz[0][0])))
    print("ddm end to end:", fig)
    # the ideal is 0.5 * sinc(0.02) = 0.4997; the static-ray test keeps the same share of its ideal
    assert fig["ray_at_plus"] >= 0.3, fig
    assert fig["ray_at_minus"] <= 0.1, fig
    assert abs(int(strong.sec_tap[0][0]) - k(-0.9)) <= 1 and int(strong.sec_bin[0][0]) == b(RAY_HZ), fig
    assert abs(int(strong.peak_tap[0][0]) - k(0.0)) <= 1 and int(strong.peak_bin[0][0]) == b(0.0), fig
    assert fig["clean_off_zero"] <= 0.1, fig
    return fig
