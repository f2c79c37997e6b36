"""gnss_lane_boundaries (the host predicate that admits the register-capture correlators)
against a brute force: for a tap set, a code rate d (chips per sample) and a lane of M samples,
every placement of the code phase that puts some tap's boundary on a sample edge of the lane
(and a coarse sweep between), with every tap's boundary nudged to either side of where it
falls (the rounding of the kernel's boundary search), counting the distinct capture samples
0 .. M - 2 the lane then holds. The predicate speaks for every code rate up to the one it is
given (the engine passes cps_max, the loop runs below it), and boundaries less than a sample
apart at that rate part at a lower one, so the brute force takes the most over that rate and
the lower rates at which a pair of boundaries comes just a sample apart. CPU only."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

FC = 1.023e6
TAP_SETS = {
    "epl": ([-0.5, 0.0, 0.5], None),
    "pos": ([-0.5, 0.0, 0.5], [0.0, 0.05, 0.0]),
    "quarter": ([-0.25, 0.0, 0.25], None),
    "tenth": ([-0.1, 0.0, 0.1], None),
    "narrow": ([-0.05, 0.0, 0.05], None),
    "late_twice": ([-0.5, 0.5, 0.5], None),
    "one_set": ([-1.0, 0.0, 1.0], None),
    "pair": ([-0.5, 0.5], None),
    "single": ([0.0], None),
    "four": ([-0.5, -0.25, 0.25, 0.5], None),
}
RATES = [58e6, 26e6, 16.3676e6, 12.5e6, 10e6, 8.5e6]


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.abi.load()


def predicate(lib, taps, post, M, d):
    n = len(taps)
    a = (C.c_double * n)(*taps)
    p = (C.c_double * n)(*post) if post is not None else None
    return lib.gnss_lane_boundaries(a, p, n, M, d)


def brute(taps, post, M, d):
    offs = [t + (post[i] if post is not None else 0.0) for i, t in enumerate(taps)]
    phases = [k / 64.0 for k in range(64)]
    for o in offs:
        for i in range(M):
            phases.append((-o - i * d) % 1.0)  # this tap's boundary exactly at sample edge i
    eps = 1e-7
    best = 0
    for t0 in phases:
        # boundary of tap o: the x >= 0 nearest the lane start where t0 + o + x d is an integer
        xs = [(math.ceil(t0 + o - 1e-12) - (t0 + o)) / d for o in offs]
        for signs in itertools.product((-eps, eps), repeat=len(offs)):
            caps = set()
            for x, e in zip(xs, signs):
                for xx in (x + e, x + e + 1.0 / d):  # (d M < 1: at most this one more in the lane)
                    c = math.floor(xx)
                    if 0 <= c <= M - 2 and xx < M - 1:
                        caps.add(c)
            best = max(best, len(caps))
    return best


def rates_upto(taps, post, d):
    """d and the lower rates at which two boundaries are just over one sample apart."""
    offs = [t + (post[i] if post is not None else 0.0) for i, t in enumerate(taps)]
    out = {d}
    for a in offs:
        for b in offs:
            gap = (a - b) % 1.0
            if 1e-9 < gap < 1.0 - 1e-9 and gap * 0.999 < d:
                out.add(gap * 0.999)
    return sorted(out)


@pytest.mark.parametrize("name", list(TAP_SETS))
def test_predicate_against_brute_force(lib, name):
    taps, post = TAP_SETS[name]
    checked = 0
    for Fs in RATES:
        for margin in (1.0, 1.1):
            d = margin * FC / Fs
            for sub in (1, 2, 3, 4):
                M = 8 * sub
                if d * M >= 1.0:  # (the engine admits no such lane)
                    continue
                got, want = predicate(lib, taps, post, M, d), max(brute(taps, post, M, x) for x in rates_upto(taps, post, d))
                # never below what a lane can hold; above it only by the one sample that the
                # predicate grants for rounding whether or not a set can be parted
                assert want <= got <= want + 1, (name, Fs, margin, M, got, want)
                checked += 1
    assert checked >= 20


def test_known_values(lib):
    d = 1.1 * FC / 58e6
    assert [predicate(lib, [-0.5, 0.0, 0.5], None, 8 * s, d) for s in (1, 2, 3, 4)] == [2, 2, 2, 3]
    assert [predicate(lib, [-0.25, 0.0, 0.25], None, 8 * s, d) for s in (1, 2, 3, 4)] == [2, 3, 3, 4]
    assert [predicate(lib, [-0.1, 0.0, 0.1], None, 8 * s, d) for s in (1, 2, 3, 4)] == [3, 4, 4, 4]
    assert predicate(lib, [-0.5, 0.0, 0.5], [0.0, 0.05, 0.0], 24, d) == 2
    assert predicate(lib, [-0.5, 0.0, 0.5], None, 8, 1.1 * FC / 8.5e6) == 3
    assert predicate(lib, [-0.5, 0.0, 0.5], None, 8, 1.1 * FC / 12.5e6) == 3
    assert predicate(lib, [0.0], None, 24, d) == 2
    assert predicate(lib, [-0.5, 0.5, 0.5], None, 8, 1.1 * FC / 8.5e6) == 2
    assert lib.gnss_lane_boundaries(None, None, 3, 24, d) == -1
    a = (C.c_double * 3)(-0.5, 0.0, 0.5)
    assert lib.gnss_lane_boundaries(a, None, 3, 0, d) == -1
    assert lib.gnss_lane_boundaries(a, None, 3, 24, 0.0) == -1


def test_option_is_additive(pkg):
    assert pkg.abi.OPT_SLOT_PATH == 12
    assert np.all(np.arange(13) == [pkg.abi.OPT_FORCE_SUB, pkg.abi.OPT_NO_PERSIST, pkg.abi.OPT_FORCE_VPB,
                                    pkg.abi.OPT_ACQ_ROCFFT, pkg.abi.OPT_FINE_ROCFFT, pkg.abi.OPT_ACQ_BATCH,
                                    pkg.abi.OPT_ACQ_FUSED, pkg.abi.OPT_ACQ_RING, pkg.abi.OPT_ACQ_PIPE,
                                    pkg.abi.OPT_VT_BLOCKS, pkg.abi.OPT_FORCE_PEER, pkg.abi.OPT_VT_SPAN,
                                    pkg.abi.OPT_SLOT_PATH])
