"""GPU parity of the 25-tap vector-tracking loop (trackingVT_POS_updated_multicorrelator.m;
gnss_tracking_vt_mc_run / gnss_tracking_vt_mc, csrc/vt_mc.hip) against the numpy twin
(tests/vt_mc_twin.py, itself held against the C oracle in tests/test_vt_mc_twin.py) on the shared
synthetic Opensky record. Bounds as tests/test_gpu_vt.py::_check and test_gpu_vtnav.py::_compare:
integer fields exact; each of the 50 sums within 1e-9 of max(|P_i|, |P_q|, 1) (fp64 fixed-order
sums on the GPU against long-double sums); NCO fields rtol / atol 1e-9; C/N0 rtol 1e-9. Shapes
are the smallest that still cross what can go wrong: PRN 22 (the table's pad quirk is visible),
code frequencies that change the read size, block counts with slices shorter than a block,
GNSS_VT_MAX_CH channels, every record format, pdi = 2."""
from types import SimpleNamespace

import numpy as np
import pytest

import vt_mc_twin as T
import vt_nav_common as V
from conftest import params

pytestmark = pytest.mark.gpu

S = 58000
INTS = ("numSample", "absoluteSample", "codedelay", "cn0_row")
NCO = ("remChip", "remCarrPhase", "codeFreq", "carrFreq", "carrNco", "carrError", "codeError")
OFFS = (0.0, 20.0, -20.0, 3.25, -7.5)
_cache = {}


def _scene(pkg):
    return dict(zip(pkg.synth.OPENSKY_SV, zip(pkg.synth.OPENSKY_CODEDELAY, pkg.synth.OPENSKY_FINEFREQ)))


def _chans(pkg, prns, skip, bps=2, remChip=None, shift=None):
    """Channels on the scene's code phases (as test_gpu_vt._chans) and the twin's states."""
    sc = _scene(pkg)
    chans, st = [], []
    for i, p in enumerate(prns):
        cd, ff = sc[p]
        fp = (S - cd + 1 + skip * S + (shift[i] if shift else 0)) * bps
        rc = remChip[i] if remChip else 0.0
        chans.append(pkg.vt_channel(p, fp, rc, 0.0, 1.023e6, ff, ff))
        st.append(T.new_state(fp, rc, 0.0, 1.023e6, ff, ff))
    return chans, st


def _series(nsteps, n):
    return np.array([[1.023e6 + OFFS[(s + 2 * i) % len(OFFS)] for i in range(n)] for s in range(nsteps)])


def _pll(track):
    return (track.PLLBW, track.PLLDamp, track.PLLGain)


def _twin_run(key, buf, st, prns, series, track, **kw):
    """The twin's records [step][channel] (computed once per key, never changed afterwards)."""
    if key not in _cache:
        _cache[key] = [[T.step(buf, st[i], series[s, i], p, pll=_pll(track), **kw) for i, p in enumerate(prns)]
                       for s in range(series.shape[0])]
    return _cache[key]


def _check(out, s, i, R, worst):
    for f in INTS:
        assert out[f][s, i] == R[f], (s, i, f, out[f][s, i], R[f])
    scale = max(abs(R["P_i"]), abs(R["P_q"]), 1.0)
    err = max(np.abs(out["tap_i"][s, i] - R["tap_i"]).max(), np.abs(out["tap_q"][s, i] - R["tap_q"]).max()) / scale
    worst[0] = max(worst[0], err)
    assert err <= 1e-9, (s, i, err)
    for f, j in (("E", T.E), ("P", T.P), ("L", T.L)):  # E / P / L are taps 2 / 12 / 22
        assert out[f + "_i"][s, i] == out["tap_i"][s, i, j] and out[f + "_q"][s, i] == out["tap_q"][s, i, j]
    for f in NCO:
        assert np.isclose(out[f][s, i], R[f], rtol=1e-9, atol=1e-9), (s, i, f, out[f][s, i], R[f])
    if R["cn0_row"]:
        assert np.isclose(out["CN0"][s, i], R["CN0"], rtol=1e-9, atol=0), (s, i)


def _against_twin(out, ref, tag=""):
    worst = [0.0]
    assert (out["status"] == 0).all()
    for s, row in enumerate(ref):
        for i, R in enumerate(row):
            _check(out, s, i, R, worst)
    print(tag, "worst sum error / |P|", worst[0])


def _buf(data):
    return np.ascontiguousarray(data, dtype=np.int8).reshape(-1)


PRNS5 = [3, 22, 26]


def _run5(pkg, ctx, opensky_short):
    skip, cfg, data = opensky_short
    file, signal, acq, track = params(pkg, skip, data)
    chans, st = _chans(pkg, PRNS5, skip)
    series = _series(8, 3)
    out = pkg.trackingVT_mc_run(file, signal, track, chans, series, ctx=ctx)
    return out, st, series, track, chans


def test_steps_against_twin(pkg, ctx, opensky_short):
    """Item 5: PRNs 3, 22, 26, 8 steps with code frequencies 0, +20, -20, +3.25, -7.5 Hz off
    1.023 MHz: the read size takes several values and the colons' step differs from the one
    that sized the read on most steps."""
    out, st, series, track, chans = _run5(pkg, ctx, opensky_short)
    assert ctx.timing()["track_launches"] == 8
    ref = _twin_run("steps", _buf(opensky_short[2]), st, PRNS5, series, track)
    _against_twin(out, ref, "steps")
    assert len(set(int(x) for x in out["numSample"].ravel())) >= 3
    old = np.vstack([np.full((1, 3), 1.023e6), series[:-1]])
    assert np.mean(old != series) > 0.5
    # the channel state after the run is the twin's
    assert [c.file_ptr for c in chans] == [ref[-1][i]["absoluteSample"] for i in range(3)]


def test_cn0_row_and_zk_wrap(pkg, ctx, opensky_short):
    """Item 6: PRN 22 alone (n = 1), 21 steps: one C/N0 row, and Zk wraps to its first slot."""
    skip, cfg, data = opensky_short
    file, signal, acq, track = params(pkg, skip, data)
    chans, st = _chans(pkg, [22], skip)
    series = _series(21, 1)
    out = pkg.trackingVT_mc_run(file, signal, track, chans, series, ctx=ctx)
    ref = _twin_run("cn0", _buf(data), st, [22], series, track)
    _against_twin(out, ref, "cn0")
    assert list(out["cn0_row"][:, 0]) == [0] * 19 + [1, 0]
    assert chans[0].index_int == 1 and chans[0].snrIndex == 2
    assert chans[0].Zk[0] == out["P_i"][20, 0] ** 2 + out["P_q"][20, 0] ** 2


@pytest.mark.parametrize("nb", [1, 7, 1024])
def test_block_counts(pkg, ctx, opensky_short, opts, nb):
    """Item 7: GNSS_OPT_VT_BLOCKS = 1 (one block walks the whole read), 7 (uneven slices) and
    1 024 (57-sample slices, most lanes idle; 2 048 partial rows for the last block)."""
    skip, cfg, data = opensky_short
    file, signal, acq, track = params(pkg, skip, data)
    chans, st = _chans(pkg, [22, 16], skip)
    series = _series(2, 2)
    opts(pkg.abi.OPT_VT_BLOCKS, nb)
    out = pkg.trackingVT_mc_run(file, signal, track, chans, series, ctx=ctx)
    ref = _twin_run("blocks", _buf(data), st, [22, 16], series, track)
    _against_twin(out, ref, f"nb={nb}")


def test_channel_independence_at_max_channels(pkg, ctx, opensky_short, opts):
    """Item 8: GNSS_VT_MAX_CH = 32 channels (the scene's 5 PRNs at different code phases and
    read offsets), one step: every channel's record is bit-equal to that channel run alone at
    the same blocks per channel, and two of them are held against the twin."""
    skip, cfg, data = opensky_short
    file, signal, acq, track = params(pkg, skip, data)
    n = pkg.abi.VT_MAX_CH
    sv = list(pkg.synth.OPENSKY_SV)[:5]
    prns = [sv[i % 5] for i in range(n)]
    rcs = [0.013 * i for i in range(n)]
    shift = [3 * i for i in range(n)]
    opts(pkg.abi.OPT_VT_BLOCKS, 8)
    series = np.array([[1.023e6 + OFFS[i % 5] for i in range(n)]])
    chans, st = _chans(pkg, prns, skip, remChip=rcs, shift=shift)
    out = pkg.trackingVT_mc_run(file, signal, track, chans, series, ctx=ctx)
    assert (out["status"] == 0).all()
    for i in range(n):
        c1, _ = _chans(pkg, [prns[i]], skip, remChip=[rcs[i]], shift=[shift[i]])
        o1 = pkg.trackingVT_mc_run(file, signal, track, c1, series[:, i:i + 1], ctx=ctx)
        for f in o1:
            assert np.array_equal(o1[f][0, 0], out[f][0, i]), (i, f)
    worst = [0.0]
    buf = _buf(data)
    for i in (7, 22):
        _check(out, 0, i, T.step(buf, st[i], series[0, i], prns[i], pll=_pll(track)), worst)
    print("32 channels: worst sum error / |P|", worst[0])


@pytest.mark.parametrize("prec,dtyp", [(1, 1), (2, 2)], ids=["int8-real", "int16-iq"])
def test_formats(pkg, ctx, opensky_short, prec, dtyp):
    """Item 9: int8 real (xi = 0) and int16 I/Q with each read's means removed (the means from
    the read's exact integer sums)."""
    skip, cfg, data = opensky_short
    rec8 = pkg.synth.convert_record(_buf(data)[: 2 * S * (skip + 6)], prec, dtyp)
    file = SimpleNamespace(skip=skip, dataType=dtyp, dataPrecision=prec, data=rec8, fileRoute=None, dev=None)
    _, signal, acq, track, _, _ = pkg.initParameters()
    chans, st = _chans(pkg, [22, 3], skip, bps=prec * dtyp)
    series = _series(3, 2)
    out = pkg.trackingVT_mc_run(file, signal, track, chans, series, ctx=ctx)
    ref = [[T.step(rec8, st[i], series[s, i], p, pll=_pll(track), prec=prec, dtype=dtyp)
            for i, p in enumerate([22, 3])] for s in range(3)]
    _against_twin(out, ref, f"format {prec} {dtyp}")


def test_pdi_2(pkg, ctx, opensky_short):
    """Item 10: pdi = 2: the repmat table (2 050 entries) and reads of ~116 000 samples."""
    skip, cfg, data = opensky_short
    file, signal, acq, track = params(pkg, skip, data)
    chans, st = _chans(pkg, [22, 31], skip)
    series = _series(3, 2)
    out = pkg.trackingVT_mc_run(file, signal, track, chans, series, pdi=2, ctx=ctx)
    ref = [[T.step(_buf(data), st[i], series[s, i], p, pll=_pll(track), pdi=2) for i, p in enumerate([22, 31])]
           for s in range(3)]
    _against_twin(out, ref, "pdi=2")
    assert out["numSample"].min() > 115000


def test_errors_are_decided_on_the_host(pkg, ctx, opensky_short):
    """Item 11: a read past EOF is GNSS_EIO and an initial remChip of -1.5 (table index 0) is
    GNSS_EINDEX, both before any launch: the record carries the status, the call returns it, and
    the next call on the context succeeds."""
    skip, cfg, data = opensky_short
    abi = pkg.abi
    file, signal, acq, track = params(pkg, skip, _buf(data)[: 2 * S * (skip + 3)])
    chans, _ = _chans(pkg, [22], skip)
    with pytest.raises(abi.GnssError) as e:
        pkg.trackingVT_mc_run(file, signal, track, chans, np.full((6, 1), 1.023e6), ctx=ctx)
    assert e.value.status == abi.EIO
    st = e.value.records["status"][:, 0]
    k = int(np.argmax(st != 0))
    assert k >= 1 and (st[:k] == 0).all() and st[k] == abi.EIO and (st[k + 1:] == 0).all()
    assert ctx.timing()["track_launches"] == k  # (the failing step launched nothing)
    chans, _ = _chans(pkg, [22], skip, remChip=[-1.5])
    with pytest.raises(abi.GnssError) as e:
        pkg.trackingVT_mc_run(file, signal, track, chans, np.full((1, 1), 1.023e6), ctx=ctx)
    assert e.value.status == abi.EINDEX and e.value.records["status"][0, 0] == abi.EINDEX
    assert ctx.timing()["track_launches"] == 0
    chans, _ = _chans(pkg, [22], skip)
    out = pkg.trackingVT_mc_run(file, signal, track, chans, np.full((1, 1), 1.023e6), ctx=ctx)
    assert out["status"][0, 0] == 0 and out["numSample"][0, 0] > 0


def _vt_inputs(pkg, z, skip):
    """test_gpu_vtnav._inputs, with TckResultCT as long as the unclamped msStartTckVT (:97): its
    last row holds the reference's state."""
    import test_gpu_vtnav as G
    Acquired, eph, sbf, ct, ns = G._inputs(pkg, z, skip)
    last = int(z["prns"][-1])
    ms = int(sbf.nav1[last - 1] + eph[last].sfb[0] * 20 + V.ROW)
    long = {}
    for p, e in ct.items():
        g = SimpleNamespace()
        for f, a in vars(e).items():
            b = np.zeros(ms)
            b[-1] = a[-1]
            setattr(g, f, b)
        long[p] = g
    return Acquired, eph, sbf, ct, long, ns


def _composed(pkg, po, z, ct, buf, nsteps, sign, track):
    """The loop composed on the CPU: the oracle's EKF (signal.IF times `sign`) predicts each
    step's code frequency and takes the twin's discriminators."""
    from test_vt_mc_twin import oracle_nav_if
    prns = [int(p) for p in z["prns"]]
    onav = oracle_nav_if(pkg, po, z, sign)
    st = [T.new_state(ct[p].absoluteSample[-1], ct[p].remChip[-1], ct[p].remCarrPhase[-1], ct[p].codeFreq[-1],
                      ct[p].carrFreq[-1], ct[p].carrFreq[-1], 0.0, ct[p].carrError[-1]) for p in prns]
    recs, nav = [], []
    for s in range(nsteps):
        row = []
        for i, p in enumerate(prns):
            cf, dpr, vel = onav.predict(i, T.num_sample(st[i]), st[i]["codeFreq"])
            R = T.step(buf, st[i], cf, p, pll=_pll(track))
            R.update(deltaPr=dpr, sv_vel=vel)
            row.append(R)
        x, es = onav.update([R["codeError"] for R in row], [R["codeFreq"] for R in row],
                            [R["carrFreq"] for R in row])
        recs.append(row)
        nav.append(x)
    return recs, np.array(nav)


def test_closed_loop_against_composition(pkg, po, ctx, opensky_short):
    """Item 12: trackingVT_POS_updated_multicorrelator on the fixture's five PRNs, 10 steps,
    against the oracle's EKF with signal.IF negated composed with the twin: read sizes, offsets,
    codedelay and sv_vel exact, sums within 1e-9, codeFreq within 1e-12 relative, usrPos /
    clkBias within 1e-5 m. The same composition with + IF is far outside those bounds."""
    skip, cfg, data = opensky_short
    file, signal, acq, track = params(pkg, skip, data)
    _, _, _, _, solu, cmn = pkg.initParameters()
    z = V.fixture()
    Acquired, eph, sbf, ct_short, ct, ns = _vt_inputs(pkg, z, skip)
    with pytest.raises(IndexError):  # (no msStartTckVT clamp: row 7675 of a 3000-row TckResultCT)
        pkg.trackingVT_POS_updated_multicorrelator(file, signal, track, cmn, solu, Acquired, V.cnslxyz(pkg), eph,
                                                   sbf, None, ct_short, ns, ctx=ctx, nsteps=1)
    nsteps = 10
    tck, nsol, cn0 = pkg.trackingVT_POS_updated_multicorrelator(
        file, signal, track, cmn, solu, Acquired, V.cnslxyz(pkg), eph, sbf, None, ct, ns, ctx=ctx, nsteps=nsteps,
        return_cn0=True)
    assert ctx.timing()["track_launches"] == nsteps and cn0.shape == (0, 5)
    buf = _buf(data)
    recs, onav = _composed(pkg, po, z, ct, buf, nsteps, -1, track)
    worst = 0.0
    for i, p in enumerate(int(x) for x in z["prns"]):
        g = tck(p)
        col = lambda f: np.array([recs[s][i][f] for s in range(nsteps)])
        assert np.array_equal(g.absoluteSample, col("absoluteSample")), p
        assert np.array_equal(g.codedelay, col("codedelay")), p
        assert np.array_equal(g.sv_vel, col("sv_vel")), p
        scale = np.maximum(np.maximum(np.abs(col("P_i")), np.abs(col("P_q"))), 1.0)
        worst = max(worst, float(np.max(np.abs(g.tap_i - col("tap_i")) / scale[:, None])),
                    float(np.max(np.abs(g.tap_q - col("tap_q")) / scale[:, None])))
        assert np.allclose(g.codeFreq, col("codeFreq"), rtol=1e-12, atol=0), p
        assert g.codeFreq[0] == ct[p].codeFreq[-1]
        # the result's fields: the reference's 50 names, (nsteps,) each, E_i == tap 2
        for k, name in enumerate(pkg.abi.MC_TAP_NAMES):
            for q in "iq":
                a = getattr(g, name.format(q))
                assert a.shape == (nsteps,) and np.array_equal(a, getattr(g, "tap_" + q)[:, k]), name
        assert np.array_equal(g.E_i, g.tap_i[:, 2]) and np.array_equal(g.L_q, g.tap_q[:, 22])
        assert np.array_equal(g.E_i_060, g.tap_i[:, 0]) and np.array_equal(g.L_q060, g.tap_q[:, 24])
    print("closed loop: worst sum error / |P|", worst)
    assert worst <= 1e-9
    assert np.allclose(nsol.usrPos, onav[:, :3], rtol=0, atol=1e-5)
    assert np.allclose(nsol.clkBias, onav[:, 6], rtol=0, atol=1e-5)
    assert nsol.usrPos.shape == (nsteps, 3) and nsol.kalman_gain.shape == (8, 10, nsteps)
    # + IF: the state leaves those bounds with the first update (on the CPU, one step; the second
    # step's predicted code frequency is already one whose replica MATLAB cannot index)
    _, onav_p = _composed(pkg, po, z, ct, buf, 1, +1, track)
    assert np.abs(onav_p[0, :3] - onav[0, :3]).max() > 1e-2
    assert abs(onav_p[0, 6] - onav[0, 6]) > 1e-2


def test_bit_identical_from_run_to_run(pkg, ctx, opensky_short):
    """Item 13: the run of test_steps_against_twin twice: every output bit for bit."""
    a = _run5(pkg, ctx, opensky_short)[0]
    b = _run5(pkg, ctx, opensky_short)[0]
    for f in a:
        assert np.array_equal(a[f], b[f]), f
