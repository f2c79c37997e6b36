"""The 25-tap vector-tracking loop (trackingVT_POS_updated_multicorrelator.m) without a GPU:
the numpy twin that the GPU tests take their expected values from (tests/vt_mc_twin.py) held
against the C oracle's correlator, the library's host half (gnss_vt_mc_prepare /
gnss_vt_mc_nco_step) held against the twin, and the sign of signal.IF in the EKF's
prr_measured (+ for trackingVT_POS_updated.m:380, - for the multicorrelator file's :504)."""
import ctypes as C
import os
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest

import vt_mc_twin as T
import vt_nav_common as V
from conftest import ROOT

S = 58000
FS = 58e6


def _scene(pkg):
    return dict(zip(pkg.synth.OPENSKY_SV, zip(pkg.synth.OPENSKY_CODEDELAY, pkg.synth.OPENSKY_FINEFREQ)))


def _state(pkg, prn, skip, remChip=0.0, bps=2):
    cd, ff = _scene(pkg)[prn]
    return T.new_state((S - cd + 1 + skip * S) * bps, remChip, 0.0, 1.023e6, ff, ff)


def _wiped(buf, st, n):
    """InphaseSignal / QuadratureSignal of the read (:285-291)."""
    raw = T.read_samples(buf[st["file_ptr"]:], 1, 2, n)
    Wave = (2 * np.pi * (st["carrFreq"] * (np.arange(0, n + 1) / FS))) + st["remCarrPhase"]
    prod = raw * np.exp(1j * Wave[:n])
    return np.imag(prod), np.real(prod)


def test_twin_taps_against_c_oracle(pkg, po, opensky_short):
    """Item 1. Where c(1022) == c(1023) the table's pad quirk is invisible and the oracle's
    Code(ceil(t)+1) on [c(end) c ... c(1)] is the same replica: the twin's 25 taps equal
    po.correlate_step's within 1e-12 of |P|. For PRN 22 the two chips differ, and the twin must
    differ from the oracle by exactly (c(1022) - c(1023)) * sum over the samples with
    ceil(t) = 0, a difference of more than 1e-3 of |P|: the GPU tests on PRN 22 see the quirk."""
    skip, cfg, data = opensky_short
    buf = np.ascontiguousarray(data, dtype=np.int8).reshape(-1)
    taps = T.spacing()
    for prn in (3, 16, 26, 31, 22):
        st = _state(pkg, prn, skip)
        n, ti, tq, tp, _ = T.correlate(buf, st, 1.023e6, prn)
        ca = po.generate_ca(prn)
        o = po.correlate_step(buf[st["file_ptr"]:], n, 0.0, 1.023e6, FS, st["carrFreq"], 0.0, ca, 1, taps)
        scale = max(abs(ti[T.P]), abs(tq[T.P]))
        di, dq = ti - o[0::2], tq - o[1::2]
        if prn != 22:
            assert int(ca[1021]) == int(ca[1022])
            assert max(np.abs(di).max(), np.abs(dq).max()) <= 1e-12 * scale, prn
            continue
        assert int(ca[1021]) != int(ca[1022])
        I, Q = _wiped(buf, st, n)
        worst = 0.0
        for j, t in enumerate(T.tap_colons(st, 1.023e6, n)):
            m = np.ceil(t) == 0
            k = float(ca[1021]) - float(ca[1022])
            assert abs(di[j] - k * float(np.sum(I[m].astype(np.longdouble)))) <= 1e-12 * scale, j
            assert abs(dq[j] - k * float(np.sum(Q[m].astype(np.longdouble)))) <= 1e-12 * scale, j
            if taps[j] > 0:
                assert not m.any()  # (an early tap never reaches the pad)
            worst = max(worst, abs(di[j]) / scale, abs(dq[j]) / scale)
        print("PRN 22: twin - oracle, worst / |P|", worst)
        assert worst > 1e-3


def _c_chan(pkg, st, prn):
    c = pkg.vt_channel(prn, st["file_ptr"], st["remChip"], st["remCarrPhase"], st["codeFreq"], st["carrFreq"],
                       st["carrFreqBasis"], st["oldCarrNco"], st["oldCarrError"])
    return c


def _prepare(pkg, signal, c, cf, pdi=1):
    a, cc, n = (C.c_double * 25)(), (C.c_double * 25)(), C.c_int64()
    st = pkg.abi.load().gnss_vt_mc_prepare(C.byref(pkg.sdr.to_c_signal(signal)), pdi, C.byref(c), cf, a, cc,
                                           C.byref(n))
    return st, np.array(a[:]), np.array(cc[:]), n.value


def test_host_half_against_twin(pkg):
    """Item 2. gnss_vt_mc_prepare: numSample and every colon's ends exact; gnss_vt_mc_nco_step:
    the scalar end from given sums within 1e-9 (rtol / atol), over 45 steps of a changing code
    frequency, so that two C/N0 rows and the Zk wrap are crossed."""
    abi = pkg.abi
    lib = abi.load()
    _, signal, _, track, _, _ = pkg.initParameters()
    pll = (track.PLLBW, track.PLLDamp, track.PLLGain)
    rng = np.random.default_rng(7)
    st = T.new_state(123456 * 2, 0.3, 1.1, 1.023e6 - 4.0, 4580975.0, 4580975.0)
    c = _c_chan(pkg, st, 22)
    cs, ctr = pkg.sdr.to_c_signal(signal), pkg.sdr.to_c_track(track)[0]
    for k in range(45):
        cf = 1.023e6 + [0.0, 20.0, -20.0, 3.25, -7.5][k % 5]
        n = T.num_sample(st)
        ts = T.tap_colons(st, cf, n)
        rc, a, cc, ng = _prepare(pkg, signal, c, cf)
        assert rc == abi.OK and ng == n
        assert np.array_equal(a, [t[0] for t in ts]) and np.array_equal(cc, [t[-1] for t in ts])
        ti = rng.normal(0, 3e3, 25) + 4e4 * np.exp(-np.abs(np.arange(25) - 12) / 6.0)
        tq = rng.normal(0, 3e3, 25)
        Wave = (2 * np.pi * (st["carrFreq"] * (np.arange(0, n + 1) / FS))) + st["remCarrPhase"]
        R = T.finish(st, cf, n, ti, tq, ts[T.P], Wave, pll=pll)
        o = abi.GnssVtMcOut()
        assert lib.gnss_vt_mc_nco_step(C.byref(cs), C.byref(ctr), 1, C.byref(c), cf, (C.c_double * 25)(*ti),
                                       (C.c_double * 25)(*tq), C.byref(o)) == abi.OK
        for f in ("numSample", "absoluteSample", "codedelay", "cn0_row"):
            assert getattr(o, f) == R[f], (k, f)
        assert o.tap_i[:] == list(ti) and o.tap_q[:] == list(tq)
        assert (o.E_i, o.P_q, o.L_i) == (ti[2], tq[12], ti[22])
        for f in ("remChip", "remCarrPhase", "codeFreq", "carrFreq", "carrNco", "carrError", "codeError"):
            assert np.isclose(getattr(o, f), R[f], rtol=1e-9, atol=1e-9), (k, f)
        if R["cn0_row"]:
            assert np.isclose(o.CN0, R["CN0"], rtol=1e-9, atol=0)
        assert c.file_ptr == st["file_ptr"] and c.snrIndex == st["snrIndex"] and c.index_int == st["index_int"]
    assert st["snrIndex"] == 3


def test_host_half_index_and_argument_errors(pkg):
    """Item 2, the statuses. remChip = -1.5: the latest tap's first element is -2.1, table index
    0 -> GNSS_EINDEX, as the twin's IndexError. Past the table's end: the read is sized so that
    the prompt ends within a sample of 1023 * pdi, so with equal old and new code frequencies no
    remChip reaches index 1023 * pdi + 5 (remChip = +2.5 ends at index 1026 of 1027: OK, and the
    twin agrees); a new code frequency 0.3 % above the one that sized the read does, GNSS_EINDEX
    on both sides."""
    abi = pkg.abi
    _, signal, _, _, _, _ = pkg.initParameters()
    good = T.new_state(0, 0.0, 0.0, 1.023e6, 4.58e6, 4.58e6)
    assert _prepare(pkg, signal, _c_chan(pkg, good, 3), 1.023e6)[0] == abi.OK
    low = T.new_state(0, -1.5, 0.0, 1.023e6, 4.58e6, 4.58e6)
    assert _prepare(pkg, signal, _c_chan(pkg, low, 3), 1.023e6)[0] == abi.EINDEX
    hi = T.new_state(0, 2.5, 0.0, 1.023e6, 4.58e6, 4.58e6)
    n = T.num_sample(hi)
    rc, a, cc, ng = _prepare(pkg, signal, _c_chan(pkg, hi, 3), 1.023e6)
    assert rc == abi.OK and ng == n and np.ceil(cc[0]) + 2 == 1026
    assert _prepare(pkg, signal, _c_chan(pkg, hi, 3), 1.023e6 * 1.003)[0] == abi.EINDEX
    buf = np.zeros(4 * S, dtype=np.int8)
    T.correlate(buf, dict(hi), 1.023e6, 3)
    for st, cf in ((low, 1.023e6), (hi, 1.023e6 * 1.003)):
        with pytest.raises(IndexError):
            T.correlate(buf, dict(st), cf, 3)
    # GNSS_EARG
    c = _c_chan(pkg, good, 3)
    lib = abi.load()
    cs = pkg.sdr.to_c_signal(signal)
    assert lib.gnss_vt_mc_prepare(None, 1, C.byref(c), 1.023e6, None, None, None) == abi.EARG
    assert lib.gnss_vt_mc_prepare(C.byref(cs), 1, None, 1.023e6, None, None, None) == abi.EARG
    assert lib.gnss_vt_mc_prepare(C.byref(cs), 0, C.byref(c), 1.023e6, None, None, None) == abi.EARG
    assert lib.gnss_vt_mc_prepare(C.byref(cs), 1, C.byref(c), 0.0, None, None, None) == abi.EARG
    assert lib.gnss_vt_mc_prepare(C.byref(cs), 1, C.byref(c), 1.023e6, None, None, None) == abi.OK
    for prn, cfo in ((0, 1.023e6), (52, 1.023e6), (3, 0.0)):
        bad = _c_chan(pkg, good, 3)
        bad.prn, bad.codeFreq = prn, cfo
        assert lib.gnss_vt_mc_prepare(C.byref(cs), 1, C.byref(bad), 1.023e6, None, None, None) == abi.EARG
    o = abi.GnssVtMcOut()
    z25 = (C.c_double * 25)()
    _, _, _, track, _, _ = pkg.initParameters()
    ctr = pkg.sdr.to_c_track(track)[0]
    assert lib.gnss_vt_mc_nco_step(C.byref(cs), C.byref(ctr), 1, C.byref(c), 1.023e6, None, z25, C.byref(o)) == abi.EARG
    c.index_int = 20
    assert lib.gnss_vt_mc_nco_step(C.byref(cs), C.byref(ctr), 1, C.byref(c), 1.023e6, z25, z25, C.byref(o)) == abi.EARG


def _replay(pkg, z, onav, update, nsteps):
    """test_vt_nav_kat's replay of the reference's recorded VT run through `update` and the
    oracle's EKF side by side -> the steps at which they are not bit-identical, the last state."""
    abi = pkg.abi
    lib = abi.load()
    nav = V.product_nav(pkg, z)
    n = len(z["prns"])
    last_abs, cf_last = z["ct_absoluteSample"][:, -1].copy(), z["ct_codeFreq"][:, -1].copy()
    mism, x = [], None
    for k in range(nsteps):
        for i in range(n):
            ns = int(z["vt_absoluteSample"][i, k] - last_abs[i]) // 2
            cf, dpr, sv = C.c_double(cf_last[i]), C.c_double(), (C.c_double * 3)()
            assert lib.gnss_vt_nav_predict(C.byref(nav), i, ns, C.byref(cf), C.byref(dpr), sv) == abi.OK
            onav.predict(i, ns, cf_last[i])
            last_abs[i], cf_last[i] = z["vt_absoluteSample"][i, k], z["vt_codeFreq"][i, k]
        args = [(C.c_double * n)(*z[f][:, k]) for f in ("vt_codeError", "vt_codeFreq", "vt_carrFreq")]
        sol = abi.GnssVtNavSol()
        assert update(C.byref(nav), *args, C.byref(sol)) == abi.OK
        x, es = onav.update(z["vt_codeError"][:, k], z["vt_codeFreq"][:, k], z["vt_carrFreq"][:, k])
        if list(x) != sol.usrPos[:] + sol.usrVel[:] + [sol.clkBias, sol.clkDrift] or list(es) != sol.state[:]:
            mism.append(k)
    return mism, x


def oracle_nav_if(pkg, po, z, sign):
    """po.VtNav on the reference's inputs with signal.IF times `sign`."""
    _, signal, _, _, _, cmn = pkg.initParameters()
    sg = SimpleNamespace(**vars(signal))
    sg.IF = sign * signal.IF
    return po.VtNav([int(p) for p in z["prns"]], z["eph"], V.cnslxyz(pkg), pkg.sdr.ALPHA, pkg.sdr.BETA, cmn.doy,
                    cmn.cSpeed, signal.Fc, sg, z["navSolCT_usrPos"][V.ROW - 1], z["navSolCT_usrVel"][V.ROW - 1],
                    z["navSolCT_clkBias"][V.ROW - 1], z["navSolCT_clkDrift"][V.ROW - 1],
                    z["navSolCT_timeTransmit"][0])


def test_plain_update_keeps_plus_if(pkg, po):
    """Item 3. gnss_vt_nav_update through its existing entry point is bit-identical to the
    oracle's update (+ signal.IF), as before the sign became a parameter."""
    z = V.fixture()
    mism, _ = _replay(pkg, z, oracle_nav_if(pkg, po, z, +1), pkg.abi.load().gnss_vt_nav_update, 40)
    assert mism == []


def test_multicorrelator_update_uses_minus_if(pkg, po):
    """Item 4. gnss_vt_mc_nav_update equals the oracle's EKF built from a signal whose IF is
    negated, bit for bit, and is far from the + IF one."""
    z = V.fixture()
    lib = pkg.abi.load()
    mism, xm = _replay(pkg, z, oracle_nav_if(pkg, po, z, -1), lib.gnss_vt_mc_nav_update, 40)
    assert mism == []
    mism_p, xp = _replay(pkg, z, oracle_nav_if(pkg, po, z, +1), lib.gnss_vt_mc_nav_update, 3)
    assert mism_p == [0, 1, 2]


def test_added_struct_layout_matches_header(pkg):
    """The structs added within ABI v13 (abi.ADDED_STRUCTS), checked as test_abi checks the
    older ones: size and every field's offset against the header; they did not move the version (14 since gnss_acquisition_surface)."""
    header = os.path.join(ROOT, "include", "gnss_mi355x.h")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(){"]
    for cname, pyname in pkg.abi.ADDED_STRUCTS.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in getattr(pkg.abi, pyname)._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "p.c")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-o", os.path.join(d, "p"), src], check=True)
        out = subprocess.run([os.path.join(d, "p")], check=True, capture_output=True, text=True).stdout
    got = dict(l.rsplit(" ", 1) for l in out.strip().splitlines())
    for cname, pyname in pkg.abi.ADDED_STRUCTS.items():
        st = getattr(pkg.abi, pyname)
        assert int(got[cname]) == C.sizeof(st), cname
        for fname, _ in st._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(st, fname).offset, (cname, fname)
    assert pkg.abi.load().gnss_abi_version() == 14
    assert pkg.abi.GnssVtMcOut._fields_[: len(pkg.abi.GnssVtOut._fields_)] == pkg.abi.GnssVtOut._fields_
