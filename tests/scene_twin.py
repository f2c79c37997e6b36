"""A numpy twin of the multipath / NLOS scene generator, written from the model in
include/gnss_mi355x.h (gnss_synth_scene), not from the C++: float64 throughout, the model's
operation order, uint64 wrap-around for the counter hash. Also the scene and the ranges that the
CPU and GPU byte-equality tests share."""
import math

import numpy as np

TWO_PI = 2.0 * 3.14159265358979323846
FL1, FC = 1575.42e6, 1.023e6
U = np.uint64


def mix64(z):
    z = z + U(0x9E3779B97F4A7C15)
    z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
    return z ^ (z >> U(31))


def _term(n, nd, th, v, ca, lnav_bits, amp, carr0, frate):
    """amp * D * ca[chip] * (cos, sin)(2 pi ph) for the code phase th of SV v."""
    chip = np.floor(th).astype(np.int64) % 1023  # (numpy's % is already non-negative)
    bitf = np.floor((th + v.bit_phase_chips) / 20460.0)
    if v.lnav:
        D = np.where(lnav_bits[bitf.astype(np.int64) % 3000] != 0, -1.0, 1.0)
    else:
        bh = mix64(U(v.bit_seed) ^ bitf.astype(np.int64).astype(np.uint64))
        D = np.where((bh & U(1)) != 0, 1.0, -1.0)
    ph = carr0 - nd * frate
    ph = ph - np.floor(ph)
    a = amp * D * ca[chip].astype(np.float64)
    return a * np.cos(TWO_PI * ph), a * np.sin(TWO_PI * ph)


def generate(scene, sample0, nsamples, ca_of, lnav_bits):
    """Samples [sample0, sample0 + nsamples) of the scene as int8 I/Q. ca_of(prn): the 1023 +-1
    chips; lnav_bits: the 3000 LNAV bits (0/1)."""
    with np.errstate(over="ignore"):
        n = U(sample0) + np.arange(nsamples, dtype=np.uint64)
        nd = n.astype(np.float64)
        Fs, IF, sigma = scene.Fs, scene.IF, scene.noise_sigma
        re, im = np.zeros(nsamples), np.zeros(nsamples)
        amp, crate, th, ca = [], [], [], []
        for s in range(scene.n_sv):
            v = scene.sv[s]
            amp.append(math.sqrt(2.0 * sigma * sigma * math.pow(10.0, v.cn0_dbhz / 10.0) / Fs))
            crate.append(FC * (1.0 + v.doppler_hz / FL1) / Fs)
            frate = (IF + v.doppler_hz) / Fs
            th.append(v.code_phase0 + nd * crate[s])
            ca.append(np.asarray(ca_of(v.prn)))
            tr, ti = _term(n, nd, th[s], v, ca[s], lnav_bits, amp[s] * scene.los_gain[s], v.carr_phase0, frate)
            re, im = re + tr, im + ti
        for r in range(scene.n_ray):
            y = scene.ray[r]
            v = scene.sv[y.sv]
            on = (n >= U(y.t_on)) & (n < U(y.t_off))
            frate = (IF + v.doppler_hz + y.fade_hz) / Fs
            tr, ti = _term(n, nd, th[y.sv] - y.delay_chips, v, ca[y.sv], lnav_bits, amp[y.sv] * y.gain,
                           v.carr_phase0 + y.phase0_cycles, frate)
            re[on] = re[on] + tr[on]
            im[on] = im[on] + ti[on]
        h1 = mix64(U(scene.seed) ^ (n * U(0xD1B54A32D192ED03)))
        h2 = mix64(h1 ^ U(0x8CB92BA72F3D8DD7))
        u1 = ((h1 >> U(11)).astype(np.float64) + 1.0) * (1.0 / 9007199254740992.0)
        u2 = (h2 >> U(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
        rr = np.sqrt(-2.0 * np.log(u1)) * sigma
        pre_i, pre_q = re + rr * np.cos(TWO_PI * u2), im + rr * np.sin(TWO_PI * u2)
    out = np.empty(2 * nsamples, dtype=np.int8)
    out[0::2] = np.clip(np.rint(pre_i), -128, 127).astype(np.int8)
    out[1::2] = np.clip(np.rint(pre_q), -128, 127).astype(np.int8)
    return out, (pre_i, pre_q)


# ---- the scene of the byte-equality tests -------------------------------------------------
KAT_RANGES = [(0, 58000), (5_300_000_123, 58_007)]


def kat_scene(pkg):
    """Three SVs: PRN 3 with the LNAV message, PRN 16 without its direct signal, PRN 22 with a
    code phase just below 0 at sample 0 (a delayed ray's th_r is negative for the first samples
    and crosses 0 inside the first range). Rays: delay 0; delay 1.7; delay 0.5 half a cycle off
    with a 3 Hz fade; and per range one that switches on and off inside it at offsets that are no
    multiples of 64."""
    S = pkg.synth
    cfg = S.scenario([3, 16, 22], [3683, 26051, 2610], [990.0, -305.0, 1565.0], [47.0, 44.0, 50.0], skip_ms=2)
    cfg.sv[0].lnav = 1
    cfg.sv[2].code_phase0 = -0.3
    sc = S.scene_of(cfg)
    S.set_nlos(sc, 16)
    S.add_ray(sc, 3, 0.0, 0.4)
    S.add_ray(sc, 22, 1.7, 0.6)
    S.add_ray(sc, 16, 0.5, 0.8, phase_cycles=0.5, fade_hz=3.0)
    for a, _ in KAT_RANGES:
        r = S.add_ray(sc, 3, 0.25, 0.7, phase_cycles=0.1)
        r.t_on, r.t_off = a + 1001, a + 40003
    return sc


def mismatch_report(got, want, pre=None, sample0=0):
    """'' if the byte arrays agree, else where they differ (and the twin's value before rint)."""
    bad = np.flatnonzero(got != want)
    if len(bad) == 0:
        return ""
    lines = [f"{len(bad)} of {len(want)} bytes differ"]
    for b in bad[:8]:
        line = f"sample {sample0 + b // 2} {'IQ'[b % 2]}: {got[b]} != {want[b]}"
        if pre is not None:
            line += f" (before rounding {pre[b % 2][b // 2]!r})"
        lines.append(line)
    return "\n".join(lines)
