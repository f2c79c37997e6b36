"""The replay correlator on the CPU (gnss_replay_correlate with no context: the host path): hand-made
rows against the oracle's correlate_step and the numpy twin, the table derivation from the records
of three loops, row independence, the refusals, the struct layouts and the end-to-end ray scene.
Largest differences seen on the host path: 6e-14 of the scale. No GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import replay_common as rc
import replay_twin as twin
from conftest import ROOT, acquired_of


def host(pkg, dt, t, taps, chip_off=0, post=None):
    file, signal = rc.file_signal(pkg, dt)
    out, ms = pkg.replay_correlate(file, signal, t, taps, chip_off, post)
    assert ms == 0.0
    return out


def test_twin_against_the_oracle(po):
    """The twin is a known answer in its own right: it agrees with correlate_step where both apply."""
    dt, t, taps = rc.oracle_cases(po)["tile-33"]
    got = twin.replay_table(rc.record(dt), dt, rc.FS, t, po.generate_ca, taps)
    assert rc.rel_err(got, rc.oracle_ref(po, "tile-33"), t) < rc.TOL


@pytest.mark.parametrize("name", ["edges-1tap-type2", "edges-25-type2", "align-25-type2", "edges-1tap-type1",
                                  "edges-25-type1", "align-25-type1", "wide-61", "many-256", "tile-31", "tile-32",
                                  "tile-33"])
def test_host_path_against_the_oracle(pkg, po, name):
    dt, t, taps = rc.oracle_cases(po)[name]
    err = rc.rel_err(host(pkg, dt, t, taps), rc.oracle_ref(po, name), t)
    print(name, "host vs oracle", err)
    assert err < rc.TOL


@pytest.mark.parametrize("name", ["far-off0", "far-off1", "far-off1-post", "far-off0-post-real"])
def test_host_path_against_the_twin(pkg, po, name):
    dt, t, taps, off, post = rc.twin_cases()[name]
    err = rc.rel_err(host(pkg, dt, t, taps, off, post), rc.twin_ref(po, name), t)
    print(name, "host vs twin", err)
    assert err < rc.TOL


@pytest.fixture(scope="module")
def loops(pkg, po):
    """An Opensky record long enough for 120 1-ms rows, 12 10-ms rows and trackingCT_POS's switch."""
    skip = 5
    cfg = pkg.synth.opensky(skip_ms=skip)
    file, signal, _, track, _, _ = pkg.initParameters()
    file.skip, file.data = skip, po.synth_if(cfg, 0, (skip + 130) * 58000)
    A2 = acquired_of([3, 16], [3684, 26051], [4580975.0, 4579675.0])
    A1 = acquired_of([16], [26051], [4579675.0])
    return file, signal, track, A2, A1


def prompt_rms(buf, n):
    """The RMS of the prompt series (P_i, P_q are fields 0 and 1): the scale when comparing against records."""
    return float(np.sqrt(np.mean(buf.rec[:, 0, :n] ** 2 + buf.rec[:, 1, :n] ** 2)))


def replay_own(pkg, buf, A, file, signal, loop):
    t = pkg.replay_rows(buf, A, file, signal, loop=loop)
    out, _ = pkg.replay_correlate(file, signal, t, t.taps, t.chip_off, t.post)
    return t, out


def test_table_of_the_given_loop(pkg, po, loops):
    file, signal, track, A2, _ = loops
    buf = po.trackingCT_multiCorr(file, signal, track, A2, datalength=120, raw=True)
    assert buf.status == 0
    t, out = replay_own(pkg, buf, A2, file, signal, "given")
    assert list(t.n_rows) == [120, 120] and t.chip_off == 0 and t.post is None
    err = np.max(np.abs(out - buf.taps[:, :, :, :120])) / prompt_rms(buf, 120)
    print("given rows", err)
    assert err < rc.TOL


@pytest.mark.parametrize("pdi,n", [(1, 120), (10, 12)])
def test_table_of_the_mc_loop(pkg, po, loops, pdi, n):
    file, signal, track, _, A1 = loops
    track.msPosCT, track.pdi = 120, pdi
    buf = po.trackingCT_mc(file, signal, track, A1, raw=True)
    assert buf.status == 0
    t, out = replay_own(pkg, buf, A1, file, signal, "mc")
    assert list(t.n_rows) == [n] and t.chip_off == 1
    err = np.max(np.abs(out - buf.taps[:, :, :, :n])) / prompt_rms(buf, n)
    print("mc rows pdi", pdi, err)
    assert err < rc.TOL


def test_table_of_the_pos_loop_across_its_switch(pkg, po, loops):
    file, signal, track, _, A1 = loops
    track.msToProcessCT_1ms, track.ctPOS = 20, 26  # 20 rows of 1 ms, then 6 of 10 ms
    try:
        buf = po.trackingCT_POS(file, signal, track, A1, [0], raw=True)
    finally:
        track.msToProcessCT_1ms = 1000
    assert buf.status == 0
    t, out = replay_own(pkg, buf, A1, file, signal, "pos")
    assert t.numSample[0, 19] < 60000 < t.numSample[0, 20] and list(t.post) == [0.0, 0.05, 0.0]
    F = pkg.abi.FIELDS
    scale = prompt_rms(buf, 26)
    for k, name in enumerate("EPL"):
        for iq, s in enumerate("iq"):
            err = np.max(np.abs(out[0, iq, k, :26] - buf.rec[0, F.index(f"{name}_{s}"), :26])) / scale
            assert err < rc.TOL, (name, s, err)


def test_rows_are_independent(pkg, po):
    t = rc.table([16, 3], [[(64 + 2 * i, 2049 + i, *rc.state(i)) for i in range(6)],
                           [(96 + 2 * i, 1025 + i, *rc.state(i + 2)) for i in range(4)]])
    taps = rc.taps_61(po)
    full = host(pkg, 2, t, taps)
    assert rc.same_bits(full, host(pkg, 2, t, taps))  # a second run
    sub = host(pkg, 2, rc.subset(t, [0, 1], lambda c: [1, 3]), taps)
    assert rc.same_bits(sub[:, :, :, :2], full[:, :, :, [1, 3]])
    one = host(pkg, 2, rc.subset(t, [1], lambda c: range(4)), taps)
    assert rc.same_bits(one[0], full[1, :, :, :4])
    cpus = os.sched_getaffinity(0)
    try:  # one host thread: the library sizes its pool by the CPUs it may run on
        os.sched_setaffinity(0, {min(cpus)})
        single = host(pkg, 2, t, taps)
    finally:
        os.sched_setaffinity(0, cpus)
    assert rc.same_bits(single, full)


def test_rows_beyond_n_rows_and_idle_channels_are_untouched(pkg, po):
    t = rc.table([16, 3, 22], [[(64, 300, *rc.state(0))], [], [(70, 301, *rc.state(1)), (90, 302, *rc.state(2))]])
    out = host(pkg, 2, t, np.array([-0.5, 0.0, 0.5]))
    assert np.all(out[0, :, :, 1:] == 0) and np.all(out[1] == 0) and np.all(out[2] != 0)


def test_refusals(pkg):
    for name, status, mutate in rc.refusals(pkg.abi):
        st, untouched = rc.refusal_call(pkg, pkg.abi, None, mutate)
        assert st == status, (name, st)
        assert untouched, name
    # a device record and a device output need a context
    t = rc.edge_rows(2, [255])
    file, signal = rc.file_signal(pkg, 2)
    with pytest.raises(ValueError):
        pkg.replay_correlate(file, signal, t, [0.0], device_out=True)


def test_struct_layouts_match_the_header(pkg):
    header = os.path.join(ROOT, "include", "gnss_mi355x.h")
    structs = {"gnss_replay_cfg": "GnssReplayCfg", "gnss_replay_rows": "GnssReplayRows", "gnss_replay_out": "GnssReplayOut"}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(){",
             'printf("max_taps %d\\n", GNSS_REPLAY_MAX_TAPS);']
    for cname, pyname in structs.items():
        st = getattr(pkg.abi, pyname)
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in st._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write("\n".join(lines))
        exe = os.path.join(d, "p")
        subprocess.run(["gcc", "-o", exe, c], check=True)
        got = dict(l.rsplit(" ", 1) for l in subprocess.run([exe], check=True, capture_output=True,
                                                            text=True).stdout.strip().splitlines())
    assert int(got["max_taps"]) == pkg.abi.REPLAY_MAX_TAPS == 256
    for cname, pyname in structs.items():
        st = getattr(pkg.abi, pyname)
        assert int(got[cname]) == C.sizeof(st), cname
        for fname, _ in st._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(st, fname).offset, (cname, fname)


def test_replay_coherent_is_the_signed_window_sum(pkg):
    rng = np.random.default_rng(5)
    t = rng.standard_normal((2, 2, 3, 10))
    p = rng.standard_normal((2, 10))
    z = pkg.replay_coherent(t, p, 4)
    assert z.shape == (2, 2, 3, 2)
    want = sum(t[1, 0, 2, 4 + k] * (1 if p[1, 4 + k] >= 0 else -1) for k in range(4))
    assert abs(z[1, 0, 2, 1] - want) < 1e-12


def test_end_to_end_ray_beyond_the_25_taps(pkg, po):
    """A quadrature ray 0.9 chip late is outside the 25-tap window; the replay at -1.5:0.05:1.5 over
    rows 150-249 of the GIVEN loop shows it at the negative taps. Oracle loop, host path:
    clean deviation 0.031, rise at -0.9 0.39, change at +0.9 0.05, m(-1.2) 0.34 against 0.006."""
    file, signal, _, track, _, _ = pkg.initParameters()
    taps = rc.taps_61(po)
    m = {}
    for ray in (False, True):
        sc, A = rc.e2e_scene(pkg, ray)
        file.skip, file.data = 5, pkg.synth.generate_scene_host(sc, 0, 271 * 58000)
        buf = po.trackingCT_multiCorr(file, signal, track, A, datalength=260, raw=True)
        assert buf.status == 0
        t = pkg.replay_rows(buf, A, file, signal, loop="given", rows=rc.E2E_ROWS)
        out, _ = pkg.replay_correlate(file, signal, t, taps)
        m[ray] = rc.e2e_profile(pkg, out, buf.rec[:, pkg.abi.FIELDS.index("P_i"), 150:250], taps)
    rc.e2e_check(taps, m[False], m[True])
