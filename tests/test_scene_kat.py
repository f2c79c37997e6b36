"""The multipath / NLOS scene generator on the CPU (gnss_synth_scene_host, csrc/synth_scene.h):
a ray-less scene is the oracle's record byte for byte; a scene with an LNAV SV, an NLOS SV, a
negative code phase and rays of every kind equals the numpy twin (tests/scene_twin.py) byte for
byte on a range from 0 and on one past 2^32; chunked generation; the refusals; the structs'
layout; and scene_labels on a hand-made record. No GPU."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import scene_twin as T
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "gnss_mi355x.h")


def test_rayless_scene_equals_oracle(pkg, po):
    cfg = pkg.synth.opensky(skip_ms=2)  # (lnav = 0: the oracle has random bits only)
    n = 3 * 58000 + 7
    got = pkg.synth.generate_scene_host(pkg.synth.scene_of(cfg), 12345, n)
    want = po.synth_if(cfg, 12345, n)
    assert got.dtype == np.int8 and got.shape == (2 * n,)
    assert T.mismatch_report(got, want, sample0=12345) == ""


@pytest.fixture(scope="module")
def kat(pkg):
    return T.kat_scene(pkg)


@pytest.mark.parametrize("sample0,n", T.KAT_RANGES)
def test_host_path_equals_numpy_twin(pkg, po, kat, sample0, n):
    want, pre = T.generate(kat, sample0, n, po.generate_ca, pkg.synth.lnav_bits(3000))
    got = pkg.synth.generate_scene_host(kat, sample0, n)
    assert T.mismatch_report(got, want, pre, sample0) == ""
    # the scene does what it is meant to: a ray switches inside the range, off 64's grid
    edges = [kat.ray[r].t_on - sample0 for r in range(kat.n_ray)] + [kat.ray[r].t_off - sample0 for r in range(kat.n_ray)]
    assert any(0 < e < n and e % 64 for e in edges)


def test_scene_has_the_cases_the_twin_test_names(kat):
    assert kat.n_sv == 3 and kat.sv[0].lnav == 1 and kat.los_gain[1] == 0.0
    assert kat.sv[2].code_phase0 - 1.7 < 0  # th_r < 0 at small n
    delays = sorted(kat.ray[r].delay_chips for r in range(kat.n_ray))
    assert delays[0] == 0.0 and 1.7 in delays and 0.5 in delays
    assert any(kat.ray[r].phase0_cycles == 0.5 and kat.ray[r].fade_hz == 3.0 for r in range(kat.n_ray))


@pytest.mark.parametrize("threads", [1, 3])
def test_chunked_generation_is_the_whole(pkg, kat, threads):
    a, n, cut = 5_300_000_123, 9001, 4097
    whole = pkg.synth.generate_scene_host(kat, a, n, nthreads=threads)
    parts = np.concatenate([pkg.synth.generate_scene_host(kat, a, cut), pkg.synth.generate_scene_host(kat, a + cut, n - cut)])
    assert np.array_equal(whole, parts)


def bad_scenes(pkg):
    """(name, scene) for every argument error of the two entry points."""
    def base():
        sc = pkg.synth.scene_of(pkg.synth.opensky(skip_ms=2))
        pkg.synth.add_ray(sc, 3, 0.5, 0.5)
        return sc

    def edit(f):
        sc = base()
        f(sc)
        return sc

    def field(name, value):
        return lambda sc: setattr(sc.ray[0], name, value)

    nan, inf = float("nan"), float("inf")
    cases = [("n_sv -1", lambda sc: setattr(sc, "n_sv", -1)), ("n_sv 65", lambda sc: setattr(sc, "n_sv", 65)),
             ("n_ray -1", lambda sc: setattr(sc, "n_ray", -1)), ("n_ray 129", lambda sc: setattr(sc, "n_ray", 129)),
             ("prn 0", lambda sc: setattr(sc.sv[1], "prn", 0)), ("prn 52", lambda sc: setattr(sc.sv[1], "prn", 52)),
             ("ray.sv -1", field("sv", -1)), ("ray.sv n_sv", field("sv", 8)),
             ("delay < 0", field("delay_chips", -0.5)), ("delay nan", field("delay_chips", nan)),
             ("delay inf", field("delay_chips", inf)),
             ("gain < 0", field("gain", -1.0)), ("gain nan", field("gain", nan)), ("gain inf", field("gain", inf)),
             ("los_gain < 0", lambda sc: sc.los_gain.__setitem__(2, -1.0)),
             ("los_gain nan", lambda sc: sc.los_gain.__setitem__(2, nan)),
             ("los_gain inf", lambda sc: sc.los_gain.__setitem__(2, inf)),
             ("phase nan", field("phase0_cycles", nan)), ("phase inf", field("phase0_cycles", -inf)),
             ("fade nan", field("fade_hz", nan)), ("fade inf", field("fade_hz", inf)),
             ("t_off < t_on", lambda sc: (setattr(sc.ray[0], "t_on", 100), setattr(sc.ray[0], "t_off", 99)))]
    return [(name, edit(f)) for name, f in cases]


def test_host_refusals(pkg):
    lib = pkg.abi.load()
    out = np.full(2 * 64, 77, dtype=np.int8)
    for name, sc in bad_scenes(pkg):
        st = lib.gnss_synth_scene_host(C.byref(sc), 0, 64, out.ctypes.data_as(C.c_void_p), 1)
        assert st == pkg.abi.EARG, name
        assert np.all(out == 77), name
    ok = pkg.synth.scene_of(pkg.synth.opensky(skip_ms=2))
    pkg.synth.add_ray(ok, 3, 0.5, 0.5).t_off = 0  # (t_off == t_on: an empty ray, not an error)
    assert lib.gnss_synth_scene_host(C.byref(ok), 0, 64, out.ctypes.data_as(C.c_void_p), 1) == pkg.abi.OK
    assert lib.gnss_synth_scene_host(None, 0, 64, out.ctypes.data_as(C.c_void_p), 1) == pkg.abi.EARG


def test_struct_sizes_and_version(pkg, tmp_path):
    structs = {"gnss_synth_ray": pkg.abi.GnssSynthRay, "gnss_synth_scene": pkg.abi.GnssSynthScene}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(){",
             'printf("GNSS_MAX_RAYS %d\\n", GNSS_MAX_RAYS);', 'printf("GNSS_ABI_VERSION %d\\n", GNSS_ABI_VERSION);']
    for cname, st in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in st._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    c = tmp_path / "p.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "p"
    subprocess.run(["gcc", "-o", str(exe), str(c)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = dict(l.rsplit(" ", 1) for l in out.strip().splitlines())
    for cname, st in structs.items():
        assert int(got[cname]) == C.sizeof(st), cname
        for fname, _ in st._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(st, fname).offset, (cname, fname)
    assert int(got["GNSS_MAX_RAYS"]) == pkg.abi.MAX_RAYS == 128
    assert int(got["GNSS_ABI_VERSION"]) == 14 and pkg.abi.load().gnss_abi_version() == 14


def test_add_ray_and_scene_of(pkg):
    cfg = pkg.synth.opensky(skip_ms=2)
    sc = pkg.synth.scene_of(cfg)
    assert sc.n_sv == cfg.n_sv and sc.n_ray == 0 and all(sc.los_gain[i] == 1.0 for i in range(sc.n_sv))
    assert bytes(sc.sv[5]) == bytes(cfg.sv[5])
    r = pkg.synth.add_ray(sc, 16, 0.5, 0.25, phase_cycles=0.5, fade_hz=2.0, t_on_ms=3, t_off_ms=7)
    assert (r.sv, r.t_on, r.t_off, sc.n_ray) == (2, 3 * 58000, 7 * 58000, 1)
    r = pkg.synth.add_ray(sc, 3, 0.1, 0.1)
    assert (r.sv, r.t_on, r.t_off) == (0, 0, 2 ** 64 - 1)
    pkg.synth.set_nlos(sc, 4)
    assert sc.los_gain[1] == 0.0
    with pytest.raises(ValueError):
        pkg.synth.add_ray(sc, 9, 0.1, 0.1)


def test_scene_labels_on_a_hand_made_record(pkg):
    """Rows of 58000 samples from sample 1000 (absoluteSample in bytes, 2 per sample), 351 rows:
    three windows of 100 rows from row 0 with ind_start = 1."""
    S, first, rows = 58000, 1000, 351
    pos = 2 * (first + S * np.arange(1, rows + 1))  # the file position after each row's read
    rec = SimpleNamespace(absoluteSample=pos.astype(np.float64), numSample=np.full(rows, float(S)))
    tck = {3: rec, 4: rec, 16: rec}
    sc = pkg.synth.scene_of(pkg.synth.opensky(skip_ms=2))
    win = lambda m: first + m * 100 * S  # the first sample of window m

    mid = pkg.synth.add_ray(sc, 3, 0.5, 0.5)  # switches on in the middle of window 1
    mid.t_on = win(1) + 50 * S + 17
    pkg.synth.set_nlos(sc, 16)
    lab = pkg.scene_labels(sc, tck, [3, 4, 16])
    assert [list(x) for x in lab] == [[0, 1, 1], [0, 0, 0], [2, 2, 2]]

    mid.t_on = win(1)  # window 0 ends one sample before t_on
    assert list(pkg.scene_labels(sc, tck, [3])[0]) == [0, 1, 1]
    mid.t_on = win(1) - 1  # ... and here its last sample has the ray
    assert list(pkg.scene_labels(sc, tck, [3])[0]) == [1, 1, 1]
    mid.t_on, mid.t_off = 0, win(2)  # switches off with window 1's last sample
    assert list(pkg.scene_labels(sc, tck, [3])[0]) == [1, 1, 0]
    mid.t_off = win(2) + 1
    assert list(pkg.scene_labels(sc, tck, [3])[0]) == [1, 1, 1]
    # other windows: 7 rows each from row 3 (ind_start 4): (351 - 4) // 7 = 49 of them
    mid.t_on, mid.t_off = first + 10 * S, first + 10 * S + 1  # one sample, the first of row 10
    lab = pkg.scene_labels(sc, tck, [3], ind_start=4, numOverLap=7)[0]
    assert len(lab) == 49 and list(np.flatnonzero(lab)) == [1]  # rows 10..16 are window 1
