"""The delay-Doppler map on the CPU (gnss_replay_ddm with host sums: the host path): seeded sums
against the numpy twin, the Doppler sign and the row-middle approximation pinned to the replay
correlator itself, the refusals, thread-count and window independence, the struct layouts and the
end-to-end scene with a ray 20 Hz off the direct carrier. Largest figures seen: DESIGN §3.13. No GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import ddm_common as dc
import replay_common as rc
from conftest import ROOT


@pytest.mark.parametrize("prompt", [-1, 12])
@pytest.mark.parametrize("nd", [1, 11, 256])
@pytest.mark.parametrize("nt", [1, 25, 61, 256])
@pytest.mark.parametrize("R", [2, 3, 100])
def test_host_path_against_the_twin(pkg, R, nt, nd, prompt):
    """(prompt 12 on a single tap is tap 0: the one index that tap count has)"""
    s = dc.shape(R, nt, nd, prompt)
    res = dc.run(pkg, s)
    assert res.kernel_ms == 0.0 and list(res.n_win) == [2, 1, 0]
    err = dc.rel_err(res.map, dc.twin_ref(s))
    print(f"R {R} taps {nt} bins {nd} prompt {s.prompt}: host vs twin {err:.3g}")
    assert err < rc.TOL
    ok, where = dc.peaks_follow_the_twins_rule(res)
    assert ok, where


def test_peaks_only_equals_the_peaks_beside_a_map(pkg):
    s = dc.shape(3, 25, 11, 12)
    assert dc.same_result(dc.run(pkg, s, want_map=False), dc.run(pkg, s), with_map=False)
    assert dc.run(pkg, s, want_map=False).map is None


def test_peak_ties_take_the_first_index_and_a_box_over_everything_leaves_no_second(pkg):
    """dopp_hz with one value repeated gives equal bins, two identical tap columns equal taps: the
    peak takes the first of each. A box that covers every cell leaves no secondary peak."""
    s = dc.shape(5, 6, 4, -1, n_rows=[5])
    s.hz = np.full(4, 40.0)
    taps = s.taps.copy()
    taps[:, :, 2] *= 1000.0  # the largest cells, whatever the rotation
    taps[:, :, 4] = taps[:, :, 2]
    res = dc.run(pkg, s, taps=taps, excl_chips=0.05, excl_hz=1.0)
    m = res.map[0][0]
    P = m[0] ** 2 + m[1] ** 2
    assert np.all(P[:, 2] == P[0, 4]) and P[0, 2] == P.max()
    assert (int(res.peak_bin[0][0]), int(res.peak_tap[0][0])) == (0, 2)
    # the next cell in order at least 0.05 chip away holds the same power: (bin 0, tap 4)
    assert (int(res.sec_bin[0][0]), int(res.sec_tap[0][0])) == (0, 4) and res.sec_pow[0][0] == res.peak_pow[0][0]
    none = dc.run(pkg, s, taps=taps, excl_chips=1e9, excl_hz=1e9)
    assert int(none.sec_bin[0][0]) == -1 and int(none.sec_tap[0][0]) == -1 and np.isnan(none.sec_pow[0][0])
    assert (int(none.peak_bin[0][0]), int(none.peak_tap[0][0])) == (0, 2)
    assert dc.peaks_follow_the_twins_rule(res, 0.05, 1.0)[0] and dc.peaks_follow_the_twins_rule(none, 1e9, 1e9)[0]


def test_sign_and_row_middle_against_the_replay(pkg, po):
    """Pinned to the replay, not to the code under test. A cell is the rows' sum with carrFreq + nu in
    place of carrFreq, the rotation held at the row's middle sample: the exact sum is the replay
    itself run with carrFreq + nu and remPhase + 2*pi*nu*s_i/Fs per row. |exp(ia) - 1| <= |a| bounds
    each sample's share: |ddm - exact| <= sum_rows pi*|nu|*(n_i/Fs) * sum_k (|xr_k| + |xi_k|). With
    every nu negated the map must break that bound somewhere: the sign is the replay's.
    Largest left side over its bound seen: DESIGN §3.13."""
    synth = pkg.synth
    R, n = 12, 2049
    fd = 1234.0
    # the generator ties the amplitude to the noise (sqrt(2 * sigma^2 * cn0 / Fs)): a sigma of 0.01 LSB
    # rounds away and 146.7 dB-Hz makes the amplitude 40 LSB
    cfg = synth.scenario([16], [0], [fd], [146.7], skip_ms=0, sigma=0.01)
    data = synth.generate_scene_host(synth.scene_of(cfg), 0, R * n + 64)
    assert int(np.max(np.abs(data))) > 8  # a noise-free record is not an empty one
    crate = synth.FC * (1.0 + fd / synth.FL1)
    rows = []
    for i in range(R):
        phase = cfg.sv[0].code_phase0 + i * n * crate / rc.FS  # chips at the row's first sample
        rows.append((2 * i * n, n, phase % 1023.0, crate, 4.58e6 + fd, 0.3 * i))
    t = rc.table([16], [rows])
    taps = np.array([-0.5, -0.25, 0.0, 0.25, 0.5])
    nus = np.array([310.0, -620.0, 1010.0])
    t_last = ((R - 1) * n + (n - 1) / 2.0) / rc.FS
    for nu in nus:  # the negated map differs only where nu * t is not near a half-integer
        assert abs(nu * t_last - np.rint(nu * t_last)) < 0.45 and abs(nu * t_last) > 0.05
    file, signal = rc.file_signal(pkg, 2, data)
    base, _ = pkg.replay_correlate(file, signal, t, taps)
    assert np.hypot(base[0, 0, 2], base[0, 1, 2]).min() > 1e4  # the prompt holds the SV in every row

    def ddm(hz):
        res = pkg.replay_ddm(base, t, hz, u=taps, prompt=-1, rows_per_window=R, signal=signal, file=file)
        return res.map[0][0]  # [2][bins][taps]

    exact = np.zeros((2, len(nus), len(taps)))
    s_i = t.pos_bytes[0] // 2
    for m, nu in enumerate(nus):
        t2 = rc.subset(t, [0], lambda c: range(R))
        t2.carrFreq[0] = t.carrFreq[0] + nu
        t2.remPhase[0] = t.remPhase[0] + 2 * np.pi * nu * s_i / rc.FS
        out, _ = pkg.replay_correlate(file, signal, t2, taps)
        exact[:, m, :] = out[0].sum(axis=2)
    x = data.astype(np.float64)
    l1 = np.array([np.sum(np.abs(x[2 * i * n: 2 * (i + 1) * n])) for i in range(R)])
    bound = np.array([np.sum(np.pi * abs(nu) * (n / rc.FS) * l1) for nu in nus])[:, None]
    left = np.hypot(*(ddm(nus) - exact))
    print("row-middle: largest |ddm - exact| / bound", float(np.max(left / bound)))
    assert np.all(left <= bound)
    wrong = np.hypot(*(ddm(-nus) - exact))
    print("negated nu: largest |ddm - exact| / bound", float(np.max(wrong / bound)))
    assert np.any(wrong > bound)


def test_refusals(pkg):
    st, untouched = dc.raw_call(pkg, None)
    assert st == pkg.abi.OK and not untouched
    for name, status, mutate in dc.refusals(pkg.abi):
        st, untouched = dc.raw_call(pkg, None, mutate)
        assert st == status, (name, st)
        assert untouched, name
    s = dc.shape(4, 5, 3, 2)
    with pytest.raises(ValueError):
        dc.run(pkg, s, device_out=True)


def test_thread_count_and_window_independence(pkg):
    s = dc.shape(100, 61, 11, 30, n_rows=[700, 250, 100])
    full = dc.run(pkg, s)
    assert list(full.n_win) == [7, 2, 1]
    assert dc.same_result(full, dc.run(pkg, s))  # a second run
    cpus = os.sched_getaffinity(0)
    try:  # one host thread: the library sizes its pool by the CPUs it may run on
        os.sched_setaffinity(0, {min(cpus)})
        single = dc.run(pkg, s)
    finally:
        os.sched_setaffinity(0, cpus)
    assert dc.same_result(single, full)
    # window 4 of channel 0 alone: its rows as a one-channel, one-window table
    sl = slice(400, 500)
    one = dc.shape(100, 61, 11, 30, n_rows=[100])
    one.tab.pos_bytes, one.tab.numSample = s.tab.pos_bytes[:1, sl].copy(), s.tab.numSample[:1, sl].copy()
    one.tab.max_rows = 100
    alone = dc.run(pkg, one, taps=s.taps[:1, :, :, sl])
    assert dc.same_bits(alone.map[0][0], full.map[0][4])
    assert all(dc.same_bits(getattr(alone, f)[0][0], getattr(full, f)[0][4]) for f in dc.PEAK_FIELDS)


def test_struct_layouts_match_the_header(pkg):
    header = os.path.join(ROOT, "include", "gnss_mi355x.h")
    structs = {"gnss_replay_ddm_cfg": "GnssReplayDdmCfg", "gnss_replay_ddm_in": "GnssReplayDdmIn",
               "gnss_replay_ddm_out": "GnssReplayDdmOut"}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(){",
             'printf("max_dopp %d\\n", GNSS_DDM_MAX_DOPP);', 'printf("map_device %d\\n", GNSS_DDM_MAP_DEVICE);']
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
    assert int(got["max_dopp"]) == pkg.abi.DDM_MAX_DOPP == 256 and int(got["map_device"]) == pkg.abi.DDM_MAP_DEVICE
    for cname, pyname in structs.items():
        st = getattr(pkg.abi, pyname)
        assert int(got[cname]) == C.sizeof(st), cname
        for fname, _ in st._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(st, fname).offset, (cname, fname)


def test_end_to_end_ray_with_a_doppler_offset(pkg, po):
    """A ray 0.9 chip late at gain 0.5 whose carrier runs 20 Hz above the direct one turns two whole
    cycles within rows 150-249 and cancels in the zero-offset sum; the map at -1.5:0.05:1.5 chip and
    -50:10:50 Hz shows it at (-0.9 chip, +20 Hz) and not at -20 Hz. The secondary peak is asked of a
    ray of gain 0.8 (ddm_common.E2E_GAINS says why). Oracle loop, host path; the figures are in
    DESIGN §3.13."""
    file, signal, _, track, _, _ = pkg.initParameters()
    taps = rc.taps_61(po)
    res = {}
    for gain in dc.E2E_GAINS:
        sc, A = dc.e2e_scene(pkg, gain)
        file.skip, file.data = 5, pkg.synth.generate_scene_host(sc, 0, 271 * 58000)
        buf = po.trackingCT_multiCorr(file, signal, track, A, datalength=260, raw=True)
        assert buf.status == 0
        t = pkg.replay_rows(buf, A, file, signal, loop="given", rows=rc.E2E_ROWS)
        out, _ = pkg.replay_correlate(file, signal, t, taps)
        res[gain] = pkg.replay_ddm(out, t, dc.E2E_HZ, u=taps, prompt=None, rows_per_window=len(rc.E2E_ROWS),
                                   signal=signal, file=file, excl_chips=0.3, excl_hz=10.0)
    dc.e2e_check(taps, res)
