"""The acquisition's whole correlation surface against a numpy twin, cell by cell.

gnss_acquisition_surface (sdr.acquisition_surface) runs gnss_acquisition's own coarse half and
hands back corr[PRN, bin, code phase]; tests/acq_twin.py restates acquisition.m:41-68 in plain
numpy (pinned to the C oracle by tests/test_acq_twin_kat.py). One call covers every index class
of the P x 2000 four-step correlator, every ms of the non-coherent sum, every ring slot and
every batch tail, and the detector is checked exactly on the surface it read.

(a) every cell, every variant: e = max over cells |gpu - twin64| / rms(twin64[p]) per PRN, for
    the split path (GNSS_OPT_ACQ_PIPE 1 / 2 / 3, the engine's batch and 7 pairs per batch), the
    fused path (ring 2 / 3 / 4), batched rocFFT, the fp32 mode (own and rocFFT) and the int16
    I/Q and int8 real records, at S = 26 000 and 58 000. The bound is computed in the test from
    two references and not from the code under test: 16 x the same statistic between the numpy
    twin and the twin on the oracle's FFT (fp64), or between the complex64 twin and the fp64
    twin (fp32 mode). The fp64 own variants must also be bit-identical to each other.
(b) the detector exactly: the diag of the same call equals acq_twin.detect on the downloaded
    surface: peak / peak2 bit for bit, fbin / codePhase equal, SNR within 2 S 2^-53 10/ln10 dB
    (two orders of summing S non-negative terms).
(c) detector edges and ties: off-peak windows at the row ends (cp - cshift < 1, cp + cshift >
    S and their one-off neighbours), a tie across bins (freqStep = 0), a tie everywhere (an
    all-zero record: peak 0, fbin 1, codePhase 1, NaN SNR, GNSS_ENODATA).
(d) the fine search across its index classes: 11 values of signal.IF put the arg-max of
    X[D q + r], q = j1 + 2000 j2, into 9 of the 130 j2 classes, at q mod 2000 = 0, 2, 999,
    1999, ..., every residue r and both sides of the fftshift seam (K = 2, 5, 8, N - 4, N - 1).

Measured on an MI355X: e per variant group, smallest to largest over the cases' PRNs, in units of
rms(twin64[p]); the bound is 16 x the reference spread, 0.5-2.1e-14 (fp64) and 1.2-12e-6 (fp32).

  group (variants)                    S = 26 000 (IF 0)     S = 58 000 (IF 4.58 MHz)   bound
  split (pipe 1/2/3 x batch 0/7)      5.9e-15 .. 2.1e-14    4.8e-15 .. 1.3e-14         0.8-3.4e-13
  fused (ring 2/3/4)                  5.9e-15 .. 2.1e-14    4.8e-15 .. 1.3e-14         0.8-3.4e-13
  rocFFT                              5.4e-15 .. 1.7e-14    1.1e-14 .. 5.3e-14         0.8-3.4e-13
  int16 I/Q, int8 real (default)      8.9e-15 .. 1.1e-14    5.7e-15 .. 7.3e-15         1.1-3.1e-13
  fp32 own / fp32 rocFFT              1.4e-6 .. 6.8e-6      1.7e-6 .. 4.9e-5           2.0e-5-1.9e-4

What (a) found when it first ran: at IF = 4.58 MHz every fp64 variant was 6.4e-12 .. 6.4e-11 from
the twin, 30-200 x over the bound. The reference rounds the carrier's angle (2 pi (IF + f_b) n) / Fs
in radians, where it reaches 2.9e4 and one ulp is 3.6e-12 rad; the kernels formed it in cycles,
frac(((IF + f_b) / Fs) n), the own correlator with the product fused into the subtraction and the
rocFFT path without, 4.0e-12 from each other. Both fp64 wipe kernels now round the angle as the
reference does (acq_carrier_angle, gnss_internal.h); the figures above are measured with that.
"""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest

import acq_surface_common as K

pytestmark = pytest.mark.gpu

FACTOR = 16  # x the reference spread (the four-step's other summation order, contracted FMAs)


def fmt(a):
    return np.array2string(np.asarray(a), precision=3, max_line_width=400)


def variants(abi, c):
    """(name, group, precision, options) of every launch shape a case runs."""
    if c.fmt != "int8-iq":
        return [("default", "formats", "fp64", {})]
    v = [("default", "split", "fp64", {})]
    for pipe in (1, 2, 3):
        for batch in (0, 7):  # the engine's batch; 7: an odd batch count and a short tail
            v.append((f"pipe{pipe}-batch{batch}", "split", "fp64", {abi.OPT_ACQ_PIPE: pipe, abi.OPT_ACQ_BATCH: batch}))
    for ring in (2, 3, 4):
        v.append((f"fused-ring{ring}", "fused", "fp64", {abi.OPT_ACQ_FUSED: 1, abi.OPT_ACQ_RING: ring}))
    v.append(("rocfft", "rocfft", "fp64", {abi.OPT_ACQ_ROCFFT: 1}))
    v.append(("fp32", "fp32", "fp32", {}))
    v.append(("fp32-batch7", "fp32", "fp32", {abi.OPT_ACQ_BATCH: 7}))
    v.append(("fp32-rocfft", "fp32-rocfft", "fp32", {abi.OPT_ACQ_ROCFFT: 1}))
    return v


def gpu_surface(pkg, po, ctx, c, prec="fp64", options=None):
    """One gnss_acquisition_surface call under `options` and `prec`; both reset afterwards."""
    file, signal, acq = K.structs(pkg, po, c)
    options = options or {}
    try:
        ctx.set_acq_precision(prec == "fp64")
        for k, v in options.items():
            ctx.set_option(k, v)
        return pkg.sdr.acquisition_surface(file, signal, acq, ctx=ctx, prn_list=c.prns)
    finally:
        for k in options:
            ctx.set_option(k, 0)
        ctx.set_acq_precision(True)


@pytest.fixture(scope="module", params=list(K.SURFACE_CASES))
def run(request, pkg, po, ctx):
    """Every variant's (surface, diag) of one case, computed once for the tests below."""
    c = K.SURFACE_CASES[request.param]
    out = {}
    for name, group, prec, options in variants(pkg.abi, c):
        out[name] = (group, prec) + gpu_surface(pkg, po, ctx, c, prec, options)
    return SimpleNamespace(name=request.param, c=c, out=out)


def bounds(pkg, po, c):
    t64 = K.twin_surface(pkg, po, c)
    return {"fp64": FACTOR * K.cell_distance(K.twin_surface(pkg, po, c, "fp64b"), t64),
            "fp32": FACTOR * K.cell_distance(K.twin_surface(pkg, po, c, "fp32"), t64)}


def test_every_cell_within_the_reference_spread(pkg, po, run):
    """(a) Every cell of every variant's surface within 16 x the distance between two correct
    evaluations of the same case (a misplaced cell, a dropped or doubled ms, a wrong twiddle or
    a stale ring slot shows at 1e-7 or at order 1).
    Measured on an MI355X: fp64 e = 4.8e-15 .. 5.3e-14, under 0.22 x the bound; fp32 1.4e-6 ..
    4.9e-5, under 0.45 x the bound (module docstring)."""
    c = run.c
    t64, bound = K.twin_surface(pkg, po, c), bounds(pkg, po, c)
    bad = []
    for name, (group, prec, surf, _) in run.out.items():
        assert surf.shape == t64.shape
        e = K.cell_distance(surf, t64)
        print(f"{run.name} {group} {name}: e {fmt(e)} "
              f"bound {fmt(bound[prec])}")
        if not np.all(e <= bound[prec]):
            bad.append((name, e.tolist(), bound[prec].tolist()))
    assert not bad, bad


def test_fp64_own_variants_bit_identical(run):
    """The split, pipelined, paired and fused fp64 surfaces of one case are the same bits (each
    pair's cells are written by its own row pass; the fused kernel runs the same arithmetic)."""
    own = {n: s for n, (g, p, s, _) in run.out.items() if g in ("split", "fused")}
    if not own:
        assert run.c.fmt != "int8-iq"
        return
    first = own["pipe1-batch0"]
    for name, s in own.items():
        assert np.array_equal(first, s), (name, int(np.sum(first != s)))
    assert len(own) == 10


def check_detector(c, surf, d, what):
    """(b) diag against acq_twin.detect on the surface the detector read."""
    S = c.S
    t = K.detect_all(surf, K.cshift_of(c))
    assert np.array_equal(d.prn, c.prns), what
    assert np.array_equal(d.peak, t.peak), (what, d.peak, t.peak)
    assert np.array_equal(d.peak2, t.peak2), (what, d.peak2, t.peak2)
    assert np.array_equal(d.fbin, t.fbin), (what, d.fbin, t.fbin)
    assert np.array_equal(d.codePhase, t.codePhase), (what, d.codePhase, t.codePhase)
    tol = 2 * S * 2.0 ** -53 * 10 / math.log(10)
    nan = np.isnan(t.SNR)
    assert np.array_equal(np.isnan(d.SNR), nan), what
    if not nan.all():
        err = np.max(np.abs(d.SNR[~nan] - t.SNR[~nan]))
        assert err <= tol, (what, err, tol)


def test_detector_exact_on_its_own_surface(run):
    for name, (_, _, surf, d) in run.out.items():
        check_detector(run.c, surf, d, (run.name, name))


def test_detector_decisions_equal_the_twin(pkg, po, run):
    """fbin and codePhase of every variant are the twin's (and so the oracle's,
    test_acq_twin_kat.py)."""
    c = run.c
    t = K.detect_all(K.twin_surface(pkg, po, c), K.cshift_of(c))
    for name, (_, _, _, d) in run.out.items():
        assert np.array_equal(d.fbin, t.fbin), (name, d.fbin, t.fbin)
        assert np.array_equal(d.codePhase, t.codePhase), (name, d.codePhase, t.codePhase)


# ---- (c) detector edges and ties ----------------------------------------------------------
@pytest.mark.parametrize("S", list(K.EDGE_CASES))
def test_offpeak_window_at_the_row_ends(pkg, po, ctx, S):
    """Peaks at columns 1, 2, cshift, cshift +- 1 and their mirrors at the row's end (asserted
    on the twin first): an empty left range, an empty right range, both one-off neighbours."""
    c = K.EDGE_CASES[S]
    t64 = K.twin_surface(pkg, po, c)
    t = K.detect_all(t64, K.cshift_of(c))
    assert np.array_equal(t.codePhase, np.array(K.EDGE_DELAYS[S]) + 1) and np.all(t.fbin == 2)
    bound = bounds(pkg, po, c)
    for prec in ("fp64", "fp32"):
        surf, d = gpu_surface(pkg, po, ctx, c, prec)
        assert np.array_equal(d.fbin, t.fbin) and np.array_equal(d.codePhase, t.codePhase), (prec, d.codePhase)
        check_detector(c, surf, d, (S, prec))
        e = K.cell_distance(surf, t64)
        print(f"edges-{S} {prec}: e {fmt(e)} bound {fmt(bound[prec])}")
        assert np.all(e <= bound[prec]), (prec, e, bound[prec])
        # the SNR over the short window, against the twin's own
        assert np.max(np.abs(d.SNR - t.SNR)) < (1e-6 if prec == "fp64" else 1e-3)


def test_tie_across_bins(pkg, po, ctx):
    """freqStep = 0: three bins of the same carrier. The three rows of the surface are the same
    bits on every path, and the first-index rule picks bin 1."""
    abi = pkg.abi
    c = K.case(26000, "urban", 2, 3, 250, 0, [1, 2])
    t = K.detect_all(K.twin_surface(pkg, po, c), K.cshift_of(c))
    assert np.all(t.fbin == 1)
    for prec, options in (("fp64", {}), ("fp64", {abi.OPT_ACQ_FUSED: 1}), ("fp64", {abi.OPT_ACQ_PIPE: 3, abi.OPT_ACQ_BATCH: 2}),
                          ("fp64", {abi.OPT_ACQ_ROCFFT: 1}), ("fp32", {}), ("fp32", {abi.OPT_ACQ_ROCFFT: 1})):
        surf, d = gpu_surface(pkg, po, ctx, c, prec, options)
        assert np.array_equal(surf[:, 0], surf[:, 1]) and np.array_equal(surf[:, 0], surf[:, 2]), (prec, options)
        assert np.all(d.fbin == 1), (prec, options, d.fbin)
        assert np.array_equal(d.codePhase, t.codePhase), (prec, options)
        check_detector(c, surf, d, (prec, options))


def raw_acquisition(pkg, ctx, file, signal, acq, prns):
    """gnss_acquisition with its status returned (sdr.acquisition turns ENODATA into a message)."""
    f, k1 = pkg.sdr.to_c_file(file)
    s = pkg.sdr.to_c_signal(signal)
    a, k2 = pkg.sdr.to_c_acq(acq, prns)
    out, dg = pkg.abi.GnssAcquired(), pkg.abi.GnssAcqDiag()
    st = ctx.lib.gnss_acquisition(ctx.h, C.byref(f), C.byref(s), C.byref(a), C.byref(out), C.byref(dg))
    return st, out, dg


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_tie_everywhere(pkg, po, ctx, prec):
    """An all-zero record: every cell ties at 0. peak 0, fbin 1, codePhase 1, NaN SNR (0 / 0),
    nothing acquired, as the oracle gives; the hook itself returns GNSS_OK."""
    c = K.case(26000, "zeros", 2, 3, -250, 250, [1, 9])
    file, signal, acq = K.structs(pkg, po, c)
    r, rd = po.acquisition(file, signal, acq, prn_list=c.prns, diag=True)
    assert len(r.sv) == 0 and np.all(rd.fbin == 1) and np.all(rd.codePhase == 1) and np.all(np.isnan(rd.SNR))
    assert np.all(rd.peak == 0) and np.all(rd.peak2 == 0)
    surf, d = gpu_surface(pkg, po, ctx, c, prec)
    assert not surf.any()
    check_detector(c, surf, d, prec)
    try:
        ctx.set_acq_precision(prec == "fp64")
        st, out, dg = raw_acquisition(pkg, ctx, file, signal, acq, c.prns)
    finally:
        ctx.set_acq_precision(True)
    assert st == pkg.abi.ENODATA and out.n == 0 and dg.n == 2
    d2 = SimpleNamespace(fbin=np.array(dg.fbin[:2]), codePhase=np.array(dg.codePhase[:2]), SNR=np.array(dg.SNR[:2]),
                         peak=np.array(dg.peak[:2]), peak2=np.array(dg.peak2[:2]))
    for got in (d, d2):
        assert np.all(got.fbin == 1) and np.all(got.codePhase == 1) and np.all(np.isnan(got.SNR))
        assert np.all(got.peak == 0) and np.all(got.peak2 == 0)


def test_surface_hook_arguments(pkg, po, ctx):
    """NULL arguments -> GNSS_EARG; the context stays usable."""
    c = K.SURFACE_CASES["urban-1ms-3bin-1prn"]
    file, signal, acq = K.structs(pkg, po, c)
    f, k1 = pkg.sdr.to_c_file(file)
    s = pkg.sdr.to_c_signal(signal)
    a, k2 = pkg.sdr.to_c_acq(acq, c.prns)
    assert ctx.lib.gnss_acquisition_surface(ctx.h, C.byref(f), C.byref(s), C.byref(a), None, None) == pkg.abi.EARG
    surf, d = gpu_surface(pkg, po, ctx, c)
    assert surf.shape == (1, 3, 26000) and list(d.prn) == [1]


# ---- (d) the fine search across its index classes --------------------------------------------
FS26 = 26e6
FINE_IFS = [0.0, 1234567.0, -1234567.0, FS26 / 4, -FS26 / 4, FS26 / 2 - 150, -FS26 / 2 + 150, FS26 / 2 - 25,
            6500850.0, 100000.0, 199950.0]
# The classes the oracle alone reaches over FINE_IFS at datalen 2 (N = 520 000, D = 2): the DFT
# index of the 1-based arg-max K in fftshift order is kk = (K - 1 + N / 2) mod N = D q + r and
# j2 = q div 2000. (Labelled in shifted 1-based order instead, j2' = (K div D) div 2000, the same
# arg-maxes are {0, 32, 58, 64, 65, 71, 97, 129}: N / 2 = D * 65 * 2000 turns one into the other.)
FINE_J2 = {0, 6, 32, 64, 65, 97, 123, 128, 129}
FINE_J2_SHIFTED = {0, 32, 58, 64, 65, 71, 97, 129}
FINE_QMOD = {0, 2, 999, 1999}
FINE_SEAM_K = {2, 5, 8, 519996, 519999}
_fine = {}


def fine_case(pkg, po, S, Fs, IF, datalen, fmt="int8-iq"):
    """PRNs 5 and 9 at delays 1 000 / 20 000 samples, Doppler +120 / -180 Hz, 50 dB-Hz, the
    record generated at the same IF the search is told; and the oracle's result on it."""
    key = (S, IF, datalen, fmt)
    if key not in _fine:
        cfg = pkg.synth.scenario([5, 9], [1000, 20000], [120.0, -180.0], [50.0, 50.0], Fs=Fs, IF=IF, skip_ms=K.SKIP_MS)
        prec, dtyp = K.FMT[fmt]
        rec = pkg.synth.convert_record(po.synth_if(cfg, 0, K.RECORD_MS * S), prec, dtyp)
        file = SimpleNamespace(skip=K.SKIP_MS, dataType=dtyp, dataPrecision=prec, data=rec, fileRoute=None, dev=None)
        signal = SimpleNamespace(IF=IF, Fs=Fs, codeFreqBasis=1.023e6, ms=1e-3, Sample=S, codelength=1023.0)
        acq = SimpleNamespace(freqNum=3, freqMin=-500, freqStep=500, datalen=datalen, L=10)
        r = po.acquisition(file, signal, acq, prn_list=[5, 9])
        assert list(r.sv) == [5, 9] and list(r.codedelay) == [1000, 20000], (key, r.sv, r.codedelay)
        _fine[key] = (file, signal, acq, r)
    return _fine[key]


def fine_classes(r, signal, acq, dtyp=2):
    """(K, j2, q mod 2000, residue) of each fineFreq of an oracle result."""
    N = acq.L * signal.Sample * acq.datalen
    out = []
    for f in r.fineFreq:
        if dtyp == 2:  # fineFreq = -K Fs / N + Fs / 2 (acquisition.m:119), fftshift undone
            k = int(round((signal.Fs / 2 - f) * N / signal.Fs))
            kk = (k - 1 + N // 2) % N
        else:  # fineFreq = K Fs / N (:117)
            k = int(round(f * N / signal.Fs))
            kk = k - 1
        q, res = divmod(kk, acq.datalen)
        out.append((k, q // 2000, q % 2000, res))
    return out


def check_fine(pkg, ctx, file, signal, acq, r):
    g = pkg.acquisition(file, signal, acq, ctx=ctx, prn_list=[5, 9])
    assert np.array_equal(g.sv, r.sv)
    assert np.array_equal(g.codedelay, r.codedelay)
    assert np.array_equal(g.fineFreq, r.fineFreq), (g.fineFreq, r.fineFreq)


def test_fine_sweep_reaches_the_listed_classes(pkg, po):
    """A property of the inputs, asserted on the reference alone (no GPU call)."""
    cls = []
    for IF in FINE_IFS:
        file, signal, acq, r = fine_case(pkg, po, 26000, FS26, IF, 2)
        cls += fine_classes(r, signal, acq)
    assert {c[1] for c in cls} == FINE_J2, sorted({c[1] for c in cls})
    assert {(c[0] // 2) // 2000 for c in cls} == FINE_J2_SHIFTED
    assert {c[3] for c in cls} == {0, 1}
    assert FINE_QMOD <= {c[2] for c in cls}
    assert FINE_SEAM_K <= {c[0] for c in cls}
    assert {(c[1], c[3]) for c in cls} >= {(129, 0), (0, 0), (65, 1), (64, 1), (64, 0), (65, 0)}


@pytest.mark.parametrize("IF", FINE_IFS)
def test_fine_search_index_classes(pkg, po, ctx, IF):
    file, signal, acq, r = fine_case(pkg, po, 26000, FS26, IF, 2)
    check_fine(pkg, ctx, file, signal, acq, r)


@pytest.mark.parametrize("fine", ["own", "rocfft"])
@pytest.mark.parametrize("IF", [0.0, FS26 / 2 - 25, 6500850.0])
def test_fine_search_three_residues(pkg, po, ctx, opts, IF, fine):
    """datalen 3 (N = 780 000): three residues r; also through the rocFFT fine search."""
    if fine == "rocfft":
        opts(pkg.abi.OPT_FINE_ROCFFT, 1)
    file, signal, acq, r = fine_case(pkg, po, 26000, FS26, IF, 3)
    check_fine(pkg, ctx, file, signal, acq, r)


def test_fine_search_three_residues_reached(pkg, po):
    res = set()
    for IF in (0.0, FS26 / 2 - 25, 6500850.0):
        file, signal, acq, r = fine_case(pkg, po, 26000, FS26, IF, 3)
        res |= {c[3] for c in fine_classes(r, signal, acq)}
    assert res == {0, 1, 2}


def test_fine_search_int8_real(pkg, po, ctx):
    """The mirror-pair rule of a real record (fshift 2: the first of |F(i)| = |F(N - i)|)."""
    file, signal, acq, r = fine_case(pkg, po, 26000, FS26, 1234567.0, 2, "int8-real")
    check_fine(pkg, ctx, file, signal, acq, r)


def test_fine_search_58000(pkg, po, ctx):
    """S = 58 000 (P = 29: j2 < 290)."""
    file, signal, acq, r = fine_case(pkg, po, 58000, 58e6, 4.58e6, 2)
    assert fine_classes(r, signal, acq)[0][1] < 290
    check_fine(pkg, ctx, file, signal, acq, r)
