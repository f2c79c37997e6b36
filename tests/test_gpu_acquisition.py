"""GPU parity for acquisition.m (through the C-ABI) against the CPU oracle:
acquired PRN set, Doppler bin, code-phase index and fine frequency bit-exact;
SNR within 1e-6 dB at the default fp64 correlation (the reference's precision) and
within 1e-3 dB in the fp32 fast mode (gnss_ctx_set_acq_precision(ctx, 0)); the
config-2 case also reports the detector's peak margin."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN, params

pytestmark = pytest.mark.gpu


SNR_TOL = {"fp64": 1e-6, "fp32": 1e-3}


@pytest.fixture(params=["fp64", "fp32"])
def precision(request, ctx):
    """The acquisition correlation precision of ctx for one test (fp64 = the default)."""
    ctx.set_acq_precision(request.param == "fp64")
    yield request.param
    ctx.set_acq_precision(True)


def compare(g, gd, r, rd, prec="fp64"):
    assert np.array_equal(gd.prn, rd.prn)
    assert np.array_equal(gd.fbin, rd.fbin), (gd.fbin, rd.fbin)
    assert np.array_equal(gd.codePhase, rd.codePhase)
    assert np.max(np.abs(gd.SNR - rd.SNR)) < SNR_TOL[prec], np.max(np.abs(gd.SNR - rd.SNR))
    # peak and peak2 against the oracle too: the SNR's tolerance as a ratio
    ratio_tol = 10 ** (SNR_TOL[prec] / 10) - 1
    assert np.max(np.abs(gd.peak / rd.peak - 1)) < ratio_tol, np.max(np.abs(gd.peak / rd.peak - 1))
    assert np.max(np.abs(gd.peak2 / rd.peak2 - 1)) < ratio_tol, np.max(np.abs(gd.peak2 / rd.peak2 - 1))
    assert np.array_equal(g.sv, r.sv)
    assert np.array_equal(g.codedelay, r.codedelay)
    assert np.array_equal(g.Doppler, r.Doppler)
    assert np.array_equal(g.fineFreq, r.fineFreq)


def test_config1_prn3_acquisition(pkg, po, ctx, opensky_short, precision):
    """BASELINE config 1: PRN 3, +-5 kHz / 500 Hz (21 bins), 20 x 1 ms, fine FFT L = 10."""
    skip, cfg, data = opensky_short
    file, signal, acq, track = params(pkg, skip, data)
    acq.freqMin, acq.freqNum, acq.freqStep, acq.datalen, acq.L = -5000, 21, 500, 20, 10
    g, gd = pkg.acquisition(file, signal, acq, ctx=ctx, prn_list=[3], diag=True)
    r, rd = po.acquisition(file, signal, acq, prn_list=[3], diag=True)
    compare(g, gd, r, rd, precision)
    assert list(g.sv) == [3]
    # fine frequency on the 5 Hz grid (Fs / (L*S*datalen)), near the true 990 Hz
    assert abs(g.fineFreq[0] - 4.58e6 - 990) <= 5


def test_32prn_acquisition(pkg, po, ctx, opensky_short, precision):
    """BASELINE config 2 grid (32 PRNs, +-7 kHz / 500 Hz); 8 ms non-coherent to bound
    the oracle's CPU time."""
    skip, cfg, data = opensky_short
    file, signal, acq, track = params(pkg, skip, data)
    acq.freqMin, acq.freqNum, acq.freqStep, acq.datalen, acq.L = -7000, 29, 500, 8, 10
    g, gd = pkg.acquisition(file, signal, acq, ctx=ctx, diag=True)
    r, rd = po.acquisition(file, signal, acq, diag=True)
    compare(g, gd, r, rd, precision)
    assert set(pkg.synth.OPENSKY_SV) <= set(g.sv)


def test_no_satellites_acquired(pkg, po, ctx):
    """acquisition.m:84-85: nothing above 12 dB -> empty Acquired."""
    cfg = pkg.synth.scenario([], [], [], [], skip_ms=0)
    data = po.synth_if(cfg, 0, 30 * 58000)
    file, signal, acq, track = params(pkg, 0, data)
    acq.freqMin, acq.freqNum, acq.datalen = -3000, 13, 20
    g = pkg.acquisition(file, signal, acq, ctx=ctx, prn_list=[1, 2, 3, 4])
    assert len(g.sv) == 0 and len(g.fineFreq) == 0


def test_argument_errors_raise(pkg, po, ctx):
    """A PRN outside generateCAcode's shift table (g2s, 51 entries, generateCAcode.m:16-27:
    MATLAB's g2s(PRN) is an index error) -> GNSS_EARG; a record shorter than the datalen ms
    acquisition.m:34 reads -> GNSS_EIO (MATLAB's fread comes back short and
    rawsignal(1+(idx-1)*Sample:idx*Sample) indexes past it, :57). The context stays usable."""
    cfg = pkg.synth.scenario([], [], [], [], skip_ms=0)
    data = po.synth_if(cfg, 0, 30 * 58000)
    file, signal, acq, track = params(pkg, 0, data)
    acq.freqMin, acq.freqNum, acq.datalen = -3000, 13, 20
    for prns in ([0], [52], [3, -1]):
        with pytest.raises(pkg.abi.GnssError) as e:
            pkg.acquisition(file, signal, acq, ctx=ctx, prn_list=prns)
        assert e.value.status == pkg.abi.EARG, prns
    short, *_ = params(pkg, 0, data[: 2 * 58000 * 19])
    with pytest.raises(pkg.abi.GnssError) as e:
        pkg.acquisition(short, signal, acq, ctx=ctx, prn_list=[3])
    assert e.value.status == pkg.abi.EIO
    g = pkg.acquisition(file, signal, acq, ctx=ctx, prn_list=[1, 2])
    assert len(g.sv) == 0


def test_urban_parameters(pkg, po, ctx, precision):
    """BASELINE config 4 shape: IF = 0, Fs = 26 MHz (assumed), +-10 kHz / 250 Hz (81 bins),
    10 ms; PRN subset to bound the oracle's CPU time."""
    skip = 3
    cfg = pkg.synth.urban(skip_ms=skip)
    S = 26000
    data = po.synth_if(cfg, 0, (skip + 14) * S)
    file = SimpleNamespace(skip=skip, dataType=2, dataPrecision=1, data=data, fileRoute=None, dev=None)
    signal = SimpleNamespace(IF=0.0, Fs=26e6, codeFreqBasis=1.023e6, ms=1e-3, Sample=S,
                             codelength=1023.0)
    acq = SimpleNamespace(freqNum=81, freqMin=-10000, freqStep=250, datalen=10, L=10)
    prns = [1, 3, 5, 7]
    g, gd = pkg.acquisition(file, signal, acq, ctx=ctx, prn_list=prns, diag=True)
    r, rd = po.acquisition(file, signal, acq, prn_list=prns, diag=True)
    compare(g, gd, r, rd, precision)
    assert {1, 3, 7} <= set(g.sv)


def test_acquisition_matches_golden_vectors(pkg, po, ctx):
    from test_golden_oracle import golden_record
    z = np.load(os.path.join(GOLDEN, "golden_acq_small.npz"))
    g, data = golden_record(pkg, po)
    file, signal, acq, track = params(pkg, int(g["skip"]), data)
    acq.freqMin, acq.freqNum, acq.datalen = -5000, 21, 4
    A, d = pkg.acquisition(file, signal, acq, ctx=ctx, prn_list=[3, 7, 16], diag=True)
    assert np.array_equal(d.fbin, z["fbin"]) and np.array_equal(d.codePhase, z["codePhase"])
    assert np.max(np.abs(d.SNR - z["SNR"])) < 1e-3
    assert np.array_equal(A.sv, z["sv"]) and np.array_equal(A.codedelay, z["codedelay"])
    assert np.array_equal(A.fineFreq, z["fineFreq"])


def test_config4_bench_record_parity(pkg, po, ctx):
    """The config-4 bench record (Urban scenario, skip 1000 ms): the PRNs the full 32-PRN
    search reports beyond the scenario's six (a noise peak above the 12 dB gate) and two
    absent ones, GPU vs oracle on the same bytes."""
    skip, S = 1000, 26000
    cfg = pkg.synth.urban(skip_ms=skip, Fs=26e6)
    data = po.synth_if(cfg, 0, (skip + 30) * S)
    file = SimpleNamespace(skip=skip, dataType=2, dataPrecision=1, data=data, fileRoute=None, dev=None)
    signal = SimpleNamespace(IF=0.0, Fs=26e6, codeFreqBasis=1.023e6, ms=1e-3, Sample=S,
                             codelength=1023.0)
    acq = SimpleNamespace(freqNum=81, freqMin=-10000, freqStep=250, datalen=10, L=10)
    prns = [2, 22, 25, 30]
    g, gd = pkg.acquisition(file, signal, acq, ctx=ctx, prn_list=prns, diag=True)
    r, rd = po.acquisition(file, signal, acq, prn_list=prns, diag=True)
    compare(g, gd, r, rd)


def test_config2_datalen20_against_oracle(pkg, po, ctx, precision):
    """BASELINE config 2 at its own length (datalen 20, +-7 kHz / 500 Hz, L = 10) against
    the oracle: the 8 present SVs and 4 absent PRNs. Decisions bit-exact, SNR within the
    precision's tolerance, and the decision margins reported and asserted: every acquired
    PRN's peak clears the largest off-window value by > 1e-4 relative (the fp32 surface's
    error is ~1e-6) and every PRN's SNR is > 0.01 dB from the 12 dB gate."""
    skip = 2
    cfg = pkg.synth.opensky(skip_ms=skip)
    data = po.synth_if(cfg, 0, (skip + 20 + 12) * 58000)
    file, signal, acq, track = params(pkg, skip, data)
    acq.freqMin, acq.freqNum, acq.freqStep, acq.datalen, acq.L = -7000, 29, 500, 20, 10
    prns = sorted(pkg.synth.OPENSKY_SV + [1, 2, 5, 6])
    g, gd = pkg.acquisition(file, signal, acq, ctx=ctx, prn_list=prns, diag=True)
    r, rd = po.acquisition(file, signal, acq, prn_list=prns, diag=True, nthreads=16)
    compare(g, gd, r, rd, precision)
    assert list(g.sv) == sorted(pkg.synth.OPENSKY_SV)
    acq_mask = np.isin(gd.prn, g.sv)
    margin = (gd.peak - gd.peak2) / gd.peak
    gate = np.abs(gd.SNR - 12.0)
    print("peak margins", dict(zip(gd.prn[acq_mask].tolist(), np.round(margin[acq_mask], 4).tolist())),
          "min |SNR-12|", float(gate.min()))
    assert margin[acq_mask].min() > 1e-4
    assert gate.min() > 0.01


def test_config4_all_32_prns_against_oracle(pkg, po, ctx):
    """BASELINE config 4 at its benchmarked shape: the bench's own Urban
    record (the HIP generator's bytes, skip 1000 ms), all 32 PRNs, +-10 kHz / 250 Hz (81
    bins), datalen 10, L 10, against the oracle on the same bytes (acquisition.m:47-80 and
    the fine search :83-126). Decisions bit-exact, SNR within 1e-6 dB, and the margins
    reported and asserted as in the config-2 test: every acquired PRN's peak clears the
    largest off-window value by > 1e-4 relative, and every PRN's SNR is > 0.01 dB from the
    12 dB gate (so no decision rests on round-off)."""
    skip, S = 1000, 26000
    cfg = pkg.synth.urban(skip_ms=skip, Fs=26e6)
    dev = pkg.DeviceRecord(ctx, (skip + 30) * S * 2)
    pkg.synth.generate_device(ctx, cfg, dev)
    file = SimpleNamespace(skip=skip, dataType=2, dataPrecision=1, data=None, fileRoute=None, dev=dev)
    signal = SimpleNamespace(IF=0.0, Fs=26e6, codeFreqBasis=1.023e6, ms=1e-3, Sample=S,
                             codelength=1023.0)
    acq = SimpleNamespace(freqNum=81, freqMin=-10000, freqStep=250, datalen=10, L=10)
    g, gd = pkg.acquisition(file, signal, acq, ctx=ctx, diag=True)
    hostf = SimpleNamespace(skip=skip, dataType=2, dataPrecision=1, data=dev.download(), fileRoute=None,
                            dev=None)
    r, rd = po.acquisition(hostf, signal, acq, diag=True, nthreads=16)
    compare(g, gd, r, rd)
    assert len(gd.prn) == 32
    assert set(pkg.synth.URBAN_SV) <= set(g.sv)
    acq_mask = np.isin(gd.prn, g.sv)
    margin = (gd.peak - gd.peak2) / gd.peak
    gate = np.abs(gd.SNR - 12.0)
    print("acquired", list(g.sv), "peak margins",
          dict(zip(gd.prn[acq_mask].tolist(), np.round(margin[acq_mask], 4).tolist())),
          "min |SNR-12|", float(gate.min()))
    assert margin[acq_mask].min() > 1e-4
    assert gate.min() > 0.01


@pytest.mark.parametrize("shape", ["cfg2", "cfg4"])
def test_fused_correlator_equals_split_path(pkg, ctx, opts, shape):
    """The fused fp64 correlator (GNSS_OPT_ACQ_FUSED: one persistent launch, the column/row
    intermediate in each XCD's L2) against the default two-launch path (the intermediate
    through HBM) at the benchmarked shapes, all 32 PRNs: every PRN's SNR,
    peak, second peak, bin and code phase identical bit for bit, for ring depths 2, 3
    and 4 (acquisition.m:47-61; the same arithmetic in the same order)."""
    abi = pkg.abi
    if shape == "cfg2":
        skip, S, Fs, IF = 2, 58000, 58e6, 4.58e6
        cfg = pkg.synth.opensky(skip_ms=skip)
        acq = SimpleNamespace(freqNum=29, freqMin=-7000, freqStep=500, datalen=20, L=10)
    else:
        skip, S, Fs, IF = 1000, 26000, 26e6, 0.0
        cfg = pkg.synth.urban(skip_ms=skip, Fs=Fs)
        acq = SimpleNamespace(freqNum=81, freqMin=-10000, freqStep=250, datalen=10, L=10)
    dev = pkg.DeviceRecord(ctx, (skip + 30) * S * 2)
    pkg.synth.generate_device(ctx, cfg, dev)
    file = SimpleNamespace(skip=skip, dataType=2, dataPrecision=1, data=None, fileRoute=None, dev=dev)
    signal = SimpleNamespace(IF=IF, Fs=Fs, codeFreqBasis=1.023e6, ms=1e-3, Sample=S, codelength=1023.0)
    g0, d0 = pkg.acquisition(file, signal, acq, ctx=ctx, diag=True)
    opts(abi.OPT_ACQ_FUSED, 1)
    for ring in (3, 2, 4):
        opts(abi.OPT_ACQ_RING, ring)
        g1, d1 = pkg.acquisition(file, signal, acq, ctx=ctx, diag=True)
        for f in ("prn", "SNR", "peak", "peak2", "fbin", "codePhase"):
            a, b = np.asarray(getattr(d0, f)), np.asarray(getattr(d1, f))
            assert np.array_equal(a, b), (ring, f, a, b)
        assert np.array_equal(g0.sv, g1.sv) and np.array_equal(g0.fineFreq, g1.fineFreq)
    assert len(d0.prn) == 32


@pytest.mark.parametrize("shape", ["cfg2", "cfg4"])
def test_pipelined_batches_equal_one_stream(pkg, ctx, opts, shape, precision):
    """The split correlator's batches pipelined over two streams (GNSS_OPT_ACQ_PIPE = 2:
    batch b's row pass beside batch b+1's column pass, two intermediates) and in paired
    launches (= 3: batch b+1's column blocks and batch b's row blocks in one grid; fp64, the
    fp32 mode runs 2) against the
    same batches in order on one stream (= 1): every PRN's SNR, peak, second peak, bin and
    code phase identical bit for bit at the benchmarked shapes, with the engine's batch
    size and with 7 pairs per batch (an odd batch count and a short tail batch)
    (acquisition.m:47-61; each pair's corr entries are written by its own row pass)."""
    abi = pkg.abi
    if shape == "cfg2":
        skip, S, Fs, IF = 2, 58000, 58e6, 4.58e6
        cfg = pkg.synth.opensky(skip_ms=skip)
        acq = SimpleNamespace(freqNum=29, freqMin=-7000, freqStep=500, datalen=20, L=10)
    else:
        skip, S, Fs, IF = 1000, 26000, 26e6, 0.0
        cfg = pkg.synth.urban(skip_ms=skip, Fs=Fs)
        acq = SimpleNamespace(freqNum=81, freqMin=-10000, freqStep=250, datalen=10, L=10)
    dev = pkg.DeviceRecord(ctx, (skip + 30) * S * 2)
    pkg.synth.generate_device(ctx, cfg, dev)
    file = SimpleNamespace(skip=skip, dataType=2, dataPrecision=1, data=None, fileRoute=None, dev=dev)
    signal = SimpleNamespace(IF=IF, Fs=Fs, codeFreqBasis=1.023e6, ms=1e-3, Sample=S, codelength=1023.0)
    for batch in (0, 7):
        opts(abi.OPT_ACQ_BATCH, batch)
        res = []
        for pipe in (1, 2, 3):
            opts(abi.OPT_ACQ_PIPE, pipe)
            res.append(pkg.acquisition(file, signal, acq, ctx=ctx, diag=True))
        (g0, d0) = res[0]
        for pipe, (g1, d1) in zip((2, 3), res[1:]):
            for f in ("prn", "SNR", "peak", "peak2", "fbin", "codePhase"):
                a, b = np.asarray(getattr(d0, f)), np.asarray(getattr(d1, f))
                assert np.array_equal(a, b), (batch, pipe, f, a, b)
            assert np.array_equal(g0.sv, g1.sv) and np.array_equal(g0.fineFreq, g1.fineFreq)
        assert len(d0.prn) == 32
