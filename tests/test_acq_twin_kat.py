"""The numpy twin of the acquisition surface (tests/acq_twin.py) pinned to the C oracle, on the
cases tests/test_gpu_acq_surface.py runs on the GPU (no GPU here): the twin's detector applied
to the twin's surface gives the oracle's fbin and codePhase exactly, its peak and peak2 within
1e-13 relative and its SNR within 1e-9 dB (measured: peak ratio 1 +- 1.6e-15, SNR equal to
1e-13 dB). The twin is then the per-cell reference the oracle itself cannot be: the oracle
reports five scalars per PRN, the twin all freqNum x Sample cells."""
import numpy as np
import pytest

import acq_surface_common as K
import acq_twin

CASES = dict(K.SURFACE_CASES)
CASES.update({f"edges-{S}": c for S, c in K.EDGE_CASES.items()})


@pytest.mark.parametrize("name", list(CASES))
def test_twin_matches_oracle(pkg, po, name):
    c = CASES[name]
    file, signal, acq = K.structs(pkg, po, c)
    _, rd = po.acquisition(file, signal, acq, prn_list=c.prns, diag=True)
    for which in ("fp64", "fp64b"):
        d = K.detect_all(K.twin_surface(pkg, po, c, which), K.cshift_of(c))
        assert np.array_equal(rd.prn, c.prns)
        assert np.array_equal(d.fbin, rd.fbin), (which, d.fbin, rd.fbin)
        assert np.array_equal(d.codePhase, rd.codePhase), (which, d.codePhase, rd.codePhase)
        assert np.max(np.abs(d.peak / rd.peak - 1)) < 1e-13, which
        assert np.max(np.abs(d.peak2 / rd.peak2 - 1)) < 1e-13, which
        assert np.max(np.abs(d.SNR - rd.SNR)) < 1e-9, which


@pytest.mark.parametrize("S", list(K.EDGE_CASES))
def test_edge_scenario_peaks_sit_at_the_row_ends(pkg, po, S):
    """The edge record puts every SV's peak at column delay + 1 of bin 2, well above the gate:
    the detector's off-peak window is empty on the left (cp - cshift < 1), empty on the right
    (cp + cshift > S), or one column long on either side."""
    c = K.EDGE_CASES[S]
    cs = K.cshift_of(c)
    d = K.detect_all(K.twin_surface(pkg, po, c), cs)
    assert np.array_equal(d.codePhase, np.array(K.EDGE_DELAYS[S]) + 1)
    assert np.all(d.fbin == 2) and np.all(d.SNR > 30)
    left = np.maximum(0, d.codePhase - cs)
    right = np.maximum(0, S - (d.codePhase + cs) + 1)
    assert {0, 1} <= set(left.tolist()) and {0, 1} <= set(right.tolist())


def test_detect_ties_and_window():
    """detect() on hand-made surfaces: the first bin and the first column holding the maximum
    are found independently; the off-peak range is [1:cp-cshift, cp+cshift:end]."""
    c = np.zeros((3, 10))
    c[2, 1] = c[1, 4] = 5.0  # first bin 2 (row 1), first column 2 (of row 2)
    c[1, 8] = 2.0
    fbin, cp, snr, peak, peak2 = acq_twin.detect(c, 2)
    assert (fbin, cp, peak) == (2, 2, 5.0)
    # row 1 (bin 2), cp 2, cshift 2: columns 4..10 -> 0-based 3..9, holding the 5 and the 2
    assert peak2 == 5.0 and snr == pytest.approx(10 * np.log10(25.0 / ((25.0 + 4.0) / 7)))
    z = acq_twin.detect(np.zeros((3, 10)), 2)
    assert z[:2] == (1, 1) and np.isnan(z[2]) and z[3:] == (0.0, 0.0)


def test_fp32_twin_is_fp32(pkg, po):
    """The complex64 evaluation is carried in fp32 throughout (numpy's FFT keeps the type; the
    twin asserts it) and sits at the fp32 rounding scale from the fp64 one, not at fp64's."""
    c = K.SURFACE_CASES["urban-1ms-3bin-1prn"]
    t32, t64 = K.twin_surface(pkg, po, c, "fp32"), K.twin_surface(pkg, po, c)
    assert t32.dtype == np.float32 and t64.dtype == np.float64
    e = K.cell_distance(t32, t64)
    assert np.all(e > 1e-8) and np.all(e < 1e-4), e
    assert np.all(K.cell_distance(K.twin_surface(pkg, po, c, "fp64b"), t64) < 1e-12)
