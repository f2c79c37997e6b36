"""What the replay correlator's CPU and GPU tests share: the hand-made records and row tables, their
oracle / twin references (each computed once per session), the project's tolerance rule for
correlator sums, the refusals and the end-to-end scene."""
import functools
from types import SimpleNamespace

import numpy as np

import replay_twin as twin

FS = 58e6
TOL = 1e-8  # of the scale: the fp64 guard under the 1e-5 north-star
EDGE_N = [1, 2, 255, 256, 257, 2049, 58001, 580003]
CARRIERS = [-1.2e6, 0.0, 4.58e6]
RECORD_BYTES = 2 * 580003 + 4096


@functools.lru_cache(maxsize=None)
def record(dataType):
    """Random int8 bytes, long enough for the longest hand-made read of either record type."""
    rng = np.random.Generator(np.random.PCG64(61020 + dataType))
    return rng.integers(-128, 128, RECORD_BYTES, dtype=np.int8)


def file_signal(pkg, dataType, data=None):
    file, signal, _, _, _, _ = pkg.initParameters()
    file.skip, file.dataType, file.dataPrecision = 0, dataType, 1
    file.data = record(dataType) if data is None else data
    return file, signal


def table(prn, rows):
    """rows: per channel a list of (pos_bytes, numSample, remChip, codeFreq, carrFreq, remPhase)."""
    nch = len(prn)
    mr = max([len(r) for r in rows] + [1])
    t = SimpleNamespace(prn=np.array(prn, dtype=np.int32), n_rows=np.array([len(r) for r in rows], dtype=np.int64),
                        max_rows=mr, pos_bytes=np.zeros((nch, mr), dtype=np.int64),
                        numSample=np.zeros((nch, mr), dtype=np.int64), remChip=np.zeros((nch, mr)),
                        codeFreq=np.zeros((nch, mr)), carrFreq=np.zeros((nch, mr)), remPhase=np.zeros((nch, mr)))
    for c, rr in enumerate(rows):
        for i, (p, n, rc, cf, f, ph) in enumerate(rr):
            t.pos_bytes[c, i], t.numSample[c, i] = p, n
            t.remChip[c, i], t.codeFreq[c, i], t.carrFreq[c, i], t.remPhase[c, i] = rc, cf, f, ph
    return t


def subset(t, chans, rows_of):
    """The table of channels `chans` with, per channel, the rows rows_of(c) of t."""
    return table([int(t.prn[c]) for c in chans],
                 [[(t.pos_bytes[c, i], t.numSample[c, i], t.remChip[c, i], t.codeFreq[c, i], t.carrFreq[c, i],
                    t.remPhase[c, i]) for i in rows_of(c)] for c in chans])


def state(i):
    """The i-th hand-made NCO state: remChip negative and positive, carriers negative, 0 and IF."""
    return ([-0.3, 0.7, 0.0, -0.999, 0.45][i % 5], 1.023e6 + [0.0, 3.7, -5.2][i % 3], CARRIERS[i % 3],
            [0.0, 1.3, -2.9, 6.1][i % 4])


def edge_rows(dataType, ns=EDGE_N):
    """One row per numSample edge, each at another byte alignment."""
    bps = dataType
    rows = []
    for i, n in enumerate(ns):
        rc, cf, f, ph = state(i)
        rows.append((48 + bps * (i + 1) + 16 * i, n, rc, cf, f, ph))
    return table([16], [rows])


def align_rows(dataType):
    """257-sample rows at every pos_bytes residue mod 16 a sample-aligned read can have."""
    rows = []
    for i, r in enumerate(range(0, 16, dataType)):
        rc, cf, f, ph = state(i + 1)
        rows.append((64 + r, 257, rc, cf, f, ph))
    return table([16], [rows])


def taps_25(po):
    return po.colon(-0.6, 0.05, 0.6)


def taps_61(po):
    return po.colon(-1.5, 0.05, 1.5)


def taps_n(n):
    """n taps 0.1 chip apart around 0 (256 of them: +-12.75)."""
    return (np.arange(n) - (n - 1) / 2.0) * 0.1


def oracle_table(po, dataType, t, taps):
    """po.correlate_step (chip_off 0, no post, ceil(t) > -1022) per row in groups of <= 32 taps."""
    rec = record(dataType)
    out = np.zeros((len(t.prn), 2, len(taps), t.max_rows))
    for c in range(len(t.prn)):
        ca = po.generate_ca(int(t.prn[c]))
        for i in range(int(t.n_rows[c])):
            p, n = int(t.pos_bytes[c, i]), int(t.numSample[c, i])
            if dataType == 2:
                iq = rec[p: p + 2 * n]
            else:
                iq = np.zeros(2 * n, dtype=np.int8)
                iq[0::2] = rec[p: p + n]
            for g in range(0, len(taps), 32):
                s = po.correlate_step(iq, n, float(t.remChip[c, i]), float(t.codeFreq[c, i]), FS, float(t.carrFreq[c, i]),
                                      float(t.remPhase[c, i]), ca, 1, taps[g: g + 32])
                out[c, 0, g: g + 32, i], out[c, 1, g: g + 32, i] = s[0::2], s[1::2]
    return out


# the hand-made cases against the oracle: name -> (dataType, table, taps), reference cached
def oracle_cases(po):
    cases = {}
    for dt in (2, 1):
        cases[f"edges-1tap-type{dt}"] = (dt, edge_rows(dt), np.array([0.0]))
        cases[f"edges-25-type{dt}"] = (dt, edge_rows(dt), taps_25(po))
        cases[f"align-25-type{dt}"] = (dt, align_rows(dt), taps_25(po))
    cases["wide-61"] = (2, edge_rows(2, [255, 257, 2049, 58001]), taps_61(po))
    cases["many-256"] = (2, edge_rows(2, [256, 2049]), taps_n(256))
    for n in (31, 32, 33):  # around the kernel's tile of 32 taps
        cases[f"tile-{n}"] = (2, edge_rows(2, [257, 2049]), taps_n(n))
    return cases


_REF = {}


def oracle_ref(po, name):
    if name not in _REF:
        dt, t, taps = oracle_cases(po)[name]
        _REF[name] = oracle_table(po, dt, t, taps)
    return _REF[name]


# against the twin: chip_off 1, post, taps far out (negative chip numbers)
FAR_TAPS = np.array([-1023.0, -600.0, -0.5, 0.0, 0.5, 600.0, 1023.0])
FAR_POST = np.array([0.0, 0.05, 0.0, 0.05, -0.05, 0.0, 0.05])


def twin_cases():
    rows = {dt: edge_rows(dt, [1, 2, 255, 257, 2049]) for dt in (2, 1)}
    return {"far-off0": (2, rows[2], FAR_TAPS, 0, None), "far-off1": (2, rows[2], FAR_TAPS, 1, None),
            "far-off1-post": (2, rows[2], FAR_TAPS, 1, FAR_POST), "far-off0-post-real": (1, rows[1], FAR_TAPS, 0, FAR_POST)}


def twin_ref(po, name):
    if name not in _REF:
        dt, t, taps, off, post = twin_cases()[name]
        _REF[name] = twin.replay_table(record(dt), dt, FS, t, po.generate_ca, taps, off, post)
    return _REF[name]


def rel_err(got, ref, t, scale=None):
    """The largest difference over the table's rows, relative to the scale: for hand-made rows the
    largest reference magnitude in the compared array, floored at 1."""
    worst, top = 0.0, 0.0
    for c in range(len(t.prn)):
        k = int(t.n_rows[c])
        worst = max(worst, float(np.max(np.abs(got[c, :, :, :k] - ref[c, :, :, :k]), initial=0.0)))
        top = max(top, float(np.max(np.abs(ref[c, :, :, :k]), initial=0.0)))
    return worst / (max(top, 1.0) if scale is None else scale)


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


# ---- refusals: name -> (status name, what to break) ------------------------------------------------
def refusals(abi):
    """(name, expected status, mutate(kw)) with kw = dict(t=table, taps=, chip_off=, post=, dataPrecision=)."""
    def setrow(field, value):
        def f(kw):
            getattr(kw["t"], field)[0, 1] = value
        return f

    def setkw(key, value):
        def f(kw):
            kw[key] = value
        return f

    def settab(field, value):
        def f(kw):
            setattr(kw["t"], field, value)
        return f

    big = RECORD_BYTES
    return [
        ("no taps", abi.EARG, setkw("taps", np.zeros(0))),
        ("257 taps", abi.EARG, setkw("taps", taps_n(257))),
        ("chip_off 2", abi.EARG, setkw("chip_off", 2)),
        ("tap nan", abi.EARG, setkw("taps", np.array([0.0, np.nan]))),
        ("tap 1023.5", abi.EARG, setkw("taps", np.array([0.0, 1023.5]))),
        ("post inf", abi.EARG, setkw("post", np.array([0.0, np.inf, 0.0]))),
        ("numSample 0", abi.EARG, setrow("numSample", 0)),
        ("numSample 2^22+1", abi.EARG, setrow("numSample", (1 << 22) + 1)),
        ("remChip nan", abi.EARG, setrow("remChip", np.nan)),
        ("codeFreq 0", abi.EARG, setrow("codeFreq", 0.0)),
        ("prn 52", abi.EARG, settab("prn", np.array([52], dtype=np.int32))),
        ("n_rows over max_rows", abi.EARG, settab("n_rows", np.array([99], dtype=np.int64))),
        ("int16 record", abi.EARG, setkw("dataPrecision", 2)),
        ("pos negative", abi.EIO, setrow("pos_bytes", -2)),
        ("pos odd (I/Q)", abi.EIO, setrow("pos_bytes", 65)),
        ("read past the end", abi.EIO, setrow("pos_bytes", big - 100)),
        ("colon count", abi.EINDEX, "colon"),
    ]


def refusal_call(pkg, abi, ctx, mutate):
    """Runs one refusal on a 3-row table with the E / P / L taps; returns (status, output untouched)."""
    t = edge_rows(2, [255, 256, 257])
    kw = dict(t=t, taps=np.array([-0.5, 0.0, 0.5]), chip_off=0, post=None, dataPrecision=1)
    if mutate == "colon":
        mutate = find_bad_colon
    mutate(kw)
    file, signal = file_signal(pkg, 2)
    file.dataPrecision = kw["dataPrecision"]
    f, _k1 = pkg.sdr.to_c_file(file)
    s = pkg.sdr.to_c_signal(signal)
    import ctypes as C
    taps = np.ascontiguousarray(kw["taps"], dtype=np.float64)
    cfg = abi.GnssReplayCfg()
    cfg.n_taps, cfg.chip_off, cfg.tap_offsets = len(taps), kw["chip_off"], taps.ctypes.data
    if kw["post"] is not None:
        post = np.ascontiguousarray(kw["post"], dtype=np.float64)
        cfg.post = post.ctypes.data
    r = abi.GnssReplayRows()
    r.n_chan, r.max_rows = len(t.prn), t.max_rows
    keep = []
    for name in ("prn", "n_rows", "pos_bytes", "numSample", "remChip", "codeFreq", "carrFreq", "remPhase"):
        a = np.ascontiguousarray(getattr(t, name))
        keep.append(a)
        setattr(r, name, a.ctypes.data)
    res = np.full((1, 2, max(len(taps), 1), t.max_rows), 7.25)
    out = abi.GnssReplayOut()
    out.taps = res.ctypes.data
    st = abi.load().gnss_replay_correlate(ctx.h if ctx is not None else None, C.byref(f), C.byref(s), C.byref(cfg),
                                          C.byref(r), C.byref(out))
    return st, bool(np.all(res == 7.25))


def find_bad_colon(kw):
    """A row whose prompt colon has not numSample elements: a code rate so low that a step is below
    remChip's rounding, so (n-1)*d + remChip lands whole roundings away from n - 1 steps (the twin
    confirms the count)."""
    t = kw["t"]
    n = int(t.numSample[0, 1])
    for cf in (1e-9, 3e-9, 7e-9, 2e-8):
        d = cf / FS
        nn, _ = twin.colon_ends((0 + 0.0) + 0.7, d, ((n - 1) * d + 0.0) + 0.7)
        if nn != n - 1:
            t.remChip[0, 1], t.codeFreq[0, 1] = 0.7, cf
            return
    raise AssertionError("no row with a short colon found")


# ---- the end-to-end scene (host path or device path) -----------------------------------------------
E2E_ROWS = range(150, 250)


def e2e_profile(pkg, taps_out, prompt_i, taps):
    """m(tau): rows summed with the prompt's sign, magnitude per tap over the prompt tap's."""
    z = pkg.sdr.replay_coherent(taps_out, prompt_i, len(E2E_ROWS))[0, :, :, 0]
    ip = int(np.argmin(np.abs(taps)))
    return np.hypot(z[0], z[1]) / np.hypot(z[0, ip], z[1, ip])


def e2e_scene(pkg, ray):
    """synth.opensky(skip_ms=5) as a scene, 271 ms, optionally PRN 16's quadrature ray 0.9 chip late at
    gain 0.5 -> (scene, Acquired of PRN 16)."""
    from conftest import acquired_of
    synth = pkg.synth
    cfg = synth.opensky(skip_ms=5)
    i16 = list(synth.OPENSKY_SV).index(16)
    A = acquired_of([16], [synth.codedelays(cfg, 5)[i16]], [synth.OPENSKY_FINEFREQ[i16]])
    sc = synth.scene_of(cfg)
    if ray:
        synth.add_ray(sc, 16, 0.9, 0.5, phase_cycles=0.25)
    return sc, A


def e2e_check(taps, m_clean, m_ray):
    """The issue's end-to-end conditions; returns the figures."""
    k = lambda v: int(np.argmin(np.abs(taps - v)))  # noqa: E731
    tri = np.maximum(0.0, 1.0 - np.abs(taps))
    fig = dict(clean_dev=float(np.max(np.abs(m_clean - tri))), rise_m09=float(m_ray[k(-0.9)] - m_clean[k(-0.9)]),
               change_p09=float(abs(m_ray[k(0.9)] - m_clean[k(0.9)])), ray_m12=float(m_ray[k(-1.2)]),
               clean_m12=float(m_clean[k(-1.2)]))
    print("replay end to end:", fig)
    # |m - triangle| <= 0.1: the C/A off-peak autocorrelation is at most 65/1023 = 0.064, plus twice the
    # 1.8 % noise of a 35-dB coherent sum
    assert fig["clean_dev"] <= 0.1, fig
    assert fig["rise_m09"] >= 0.25, fig
    assert fig["change_p09"] <= 0.1, fig
    assert fig["ray_m12"] >= 0.25 and fig["clean_m12"] <= 0.1, fig
    return fig
