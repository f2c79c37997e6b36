"""The k-NN classifier through the C-ABI on the host (gnss_knn_standardize, gnss_knn_classify with
ctx = NULL; csrc/knn.cpp over csrc/knn.h): no GPU. Hand-made tables whose mu, inv and every d2 are
exact; exact ties (duplicates, rows mirrored about the query) and a 2-2-1 vote; non-finite
queries; the host path against the numpy twin (knn_twin.py) bit for bit over D, k and M; every
refusal, each followed by a good call; the Python layer."""
from types import SimpleNamespace as NS

import numpy as np
import pytest

import knn_common as K
import knn_twin as T

# columns 0 and 1: mu 0 and 2, sd 2, inv 0.5; column 2 is constant: inv 0
HAND_X = np.array([[-2.0, 0.0, 7.0], [2.0, 0.0, 7.0], [-2.0, 4.0, 7.0], [2.0, 4.0, 7.0]])
HAND_Y = [0, 1, 1, 2]


def test_hand_made_standardisation(pkg):
    st, mu, inv, z = K.standardize(pkg, HAND_X)
    assert st == pkg.abi.OK
    assert list(mu) == [0.0, 2.0, 7.0] and list(inv) == [0.5, 0.5, 0.0]
    assert np.array_equal(z, [[-1, -1, 0], [1, -1, 0], [-1, 1, 0], [1, 1, 0]])
    tmu, tinv, tz = T.standardize(HAND_X)
    assert np.array_equal(K.bits(mu), K.bits(tmu)) and np.array_equal(K.bits(inv), K.bits(tinv))
    assert np.array_equal(K.bits(z), K.bits(tz))


def test_hand_made_neighbours_and_ties(pkg):
    m = K.Model(pkg, HAND_X, HAND_Y)
    # the query is training row 2: itself first at d2 = 0, then rows 0 and 3 tied at 4 (the lower
    # row first), then row 1 at 8; the constant column changes nothing, whatever the query holds there
    for third in (7.0, 123.0, -1e300):
        st, o = K.classify(pkg, m, [[-2.0, 4.0, third]], 4)
        assert st == pkg.abi.OK
        assert list(o.nn_index[0]) == [2, 0, 3, 1] and list(o.nn_d2[0]) == [0.0, 4.0, 4.0, 8.0]
        assert list(o.votes[0]) == [1, 2, 1] and o.label[0] == 1
    # k = 3: one vote each, the nearest neighbour's class
    st, o = K.classify(pkg, m, [[-2.0, 4.0, 7.0], [2.0, 4.0, 7.0]], 3)
    assert list(o.nn_index[0]) == [2, 0, 3] and list(o.votes[0]) == [1, 1, 1] and o.label[0] == 1
    assert list(o.nn_index[1]) == [3, 1, 2] and list(o.votes[1]) == [0, 2, 1] and o.label[1] == 1
    # the centre: all four rows mirrored about the query, d2 = 2 each, in row order
    st, o = K.classify(pkg, m, [[0.0, 2.0, 0.0]], 4)
    assert list(o.nn_index[0]) == [0, 1, 2, 3] and list(o.nn_d2[0]) == [2.0] * 4
    K.assert_equals_twin(o, m, [[0.0, 2.0, 0.0]], 4)


def test_duplicates_keep_the_lower_row(pkg):
    """mu = 3 exactly, so the rows at 1 and at 5 are mirrored about a query at 3: z = -+2 inv."""
    x = np.array([[1.0], [5.0], [1.0], [3.0], [1.0], [5.0], [3.0], [5.0]])
    m = K.Model(pkg, x, [0, 1, 2, 0, 1, 2, 0, 1])
    assert m.mu[0] == 3.0
    q = [[1.0], [5.0], [3.0]]
    st, o = K.classify(pkg, m, q, 8)
    assert st == pkg.abi.OK
    assert list(o.nn_index[0]) == [0, 2, 4, 3, 6, 1, 5, 7] and np.all(o.nn_d2[0][:3] == 0)
    assert list(o.nn_index[1]) == [1, 5, 7, 3, 6, 0, 2, 4] and np.all(o.nn_d2[1][:3] == 0)
    assert list(o.nn_index[2]) == [3, 6, 0, 1, 2, 4, 5, 7]  # six exact ties, in row order
    assert np.all(o.nn_d2[2][:2] == 0) and np.all(o.nn_d2[2][2:] == o.nn_d2[2][2])
    K.assert_equals_twin(o, m, q, 8)


def test_two_two_one_vote_goes_to_the_nearest(pkg):
    """Rows mirrored about the query 0: ranks (3, 4), (2, 5), (1, 6) tie in pairs. At k = 5 the
    neighbours are rows 3, 4, 2, 5, 1 with classes 2, 0, 0, 2, 1: classes 0 and 2 hold two votes
    each and the nearest neighbour is of class 2 (the lowest class number would be 0)."""
    x = np.array([[-4.0], [-3.0], [-2.0], [-1.0], [1.0], [2.0], [3.0], [4.0]])
    m = K.Model(pkg, x, [1, 1, 0, 2, 0, 2, 1, 1])
    assert m.mu[0] == 0.0
    st, o = K.classify(pkg, m, [[0.0]], 5)
    assert st == pkg.abi.OK
    assert list(o.nn_index[0]) == [3, 4, 2, 5, 1] and list(o.votes[0]) == [2, 1, 2] and o.label[0] == 2
    st, o = K.classify(pkg, m, [[0.0]], 3)  # 2-1: the plain majority
    assert list(o.votes[0]) == [2, 0, 1] and o.label[0] == 0


def test_non_finite_queries(pkg):
    m = K.Model(pkg, HAND_X, HAND_Y)
    q = np.array([[-2.0, 4.0, 7.0], [np.nan, 4.0, 7.0], [-2.0, np.inf, 7.0], [-2.0, 4.0, np.nan],
                  [-2.0, 4.0, -np.inf], [2.0, 0.0, 7.0]])  # (rows 3 and 4: in the column with inv = 0)
    for want in (True, False):
        st, o = K.classify(pkg, m, q, 2, want=want)
        assert st == pkg.abi.OK
        assert list(o.label) == [1, -1, -1, -1, -1, 1]
        assert np.all(o.votes[1:5] == 0) and list(o.votes[0]) == [1, 1, 0] and list(o.votes[5]) == [1, 1, 0]
    assert np.all(o.label >= -1)
    st, o = K.classify(pkg, m, q, 2)
    assert np.all(o.nn_index[1:5] == -1) and np.all(np.isnan(o.nn_d2[1:5]))
    assert list(o.nn_index[0]) == [2, 0] and list(o.nn_index[5]) == [1, 0]
    K.assert_equals_twin(o, m, q, 2)


def test_overflowing_finite_query_on_a_constant_column(pkg):
    """q - mu overflows and inf * 0 is NaN: d2 is NaN for every row, which the order puts after
    +inf and breaks by row; stored as the one quiet NaN."""
    m = K.Model(pkg, np.array([[-1e308, 1.0]]), [1], n_class=2)
    st, o = K.classify(pkg, m, [[1e308, 1.0]], 1)
    assert st == pkg.abi.OK and o.label[0] == 1 and list(o.nn_index[0]) == [0]
    assert K.bits(o.nn_d2)[0, 0] == 0x7FF8000000000000
    K.assert_equals_twin(o, m, [[1e308, 1.0]], 1)


@pytest.mark.parametrize("k", [1, 5, 32])
@pytest.mark.parametrize("D", [1, 8, 11, 16])
def test_host_path_equals_twin(pkg, D, k):
    """M = k, k + 1 and 1000; a table of normal deviates and one on a coarse grid (many exact ties);
    among the queries some training rows themselves and one row with a NaN."""
    for M in (k, k + 1, 1000):
        for grid in (None, 0.5):
            x, y = K.table(100 * D + k, M, D, grid=grid)
            if grid and M > 1:
                x[M // 2] = x[0]  # a duplicated row
            st, mu, inv, z = K.standardize(pkg, x)
            assert st == pkg.abi.OK
            tmu, tinv, tz = T.standardize(x)
            assert np.array_equal(K.bits(mu), K.bits(tmu)) and np.array_equal(K.bits(inv), K.bits(tinv))
            assert np.array_equal(K.bits(z), K.bits(tz))
            m = K.Model(pkg, x, y)
            rng = np.random.default_rng(M + D)
            q = rng.integers(-3, 4, size=(24, D)) * 0.5 if grid else rng.normal(0.0, 1.5, size=(24, D))
            q = np.vstack([q, x[: min(M, 3)]])
            q[5, D - 1] = np.nan
            st, o = K.classify(pkg, m, q, k)
            assert st == pkg.abi.OK
            K.assert_equals_twin(o, m, q, k)
            assert o.nn_index[24, 0] == 0 and o.nn_d2[24, 0] == 0.0  # training row 0 finds itself first
            st, bare = K.classify(pkg, m, q, k, want=False)  # nn_index / nn_d2 NULL: the same labels
            assert st == pkg.abi.OK
            K.assert_same(o, bare)


def test_every_refusal(pkg):
    abi = pkg.abi
    x, y = K.table(3, 40, 4)
    m = K.Model(pkg, x, y)
    q = x[:5] + 0.25
    _, good = K.classify(pkg, m, q, 5)

    def fine():
        st, o = K.classify(pkg, m, q, 5)
        assert st == abi.OK
        K.assert_same(good, o)

    fine()
    for kw in (dict(D=0), dict(D=17), dict(D=-1), dict(n_class=0), dict(n_class=9), dict(M=0), dict(M=-5),
               dict(M=(1 << 24) + 1), dict(flags=2), dict(cfg_flags=4), dict(flags=abi.KNN_MODEL_DEVICE),
               dict(Q=-1), dict(null=("q",)), dict(null=("mu",)), dict(null=("inv",)), dict(null=("z",)),
               dict(null=("label",)), dict(null=("label_out",)), dict(null=("votes",))):
        assert K.classify(pkg, m, q, 5, **kw)[0] == abi.EARG, kw
        fine()
    for k in (0, -1, 33, 41):  # 41: above M = 40
        assert K.classify(pkg, m, q, k)[0] == abi.EARG, k
        fine()
    assert K.classify(pkg, m, q, 32)[0] == abi.OK and K.classify(pkg, m, q, 5, host=True)[0] == abi.OK
    for bad in (-1, 3):
        keep = m.label[17]
        m.label[17] = bad
        assert K.classify(pkg, m, q, 5)[0] == abi.EARG, bad
        m.label[17] = keep
        fine()
    st, o = K.classify(pkg, m, q, 5, Q=0)  # Q = 0: fine, nothing written
    assert st == abi.OK and np.all(o.label == -9) and np.all(o.votes == -9) and np.all(o.nn_index == -9)
    lib = abi.load()
    assert lib.gnss_knn_classify(None, None, None, None, 0, None) == abi.EARG
    fine()
    # the standardisation's
    ok = lambda **kw: K.standardize(pkg, x, **kw)[0]
    assert ok() == abi.OK
    for kw in (dict(M=0), dict(M=(1 << 24) + 1), dict(D=0), dict(D=17), dict(null=("x",)), dict(null=("mu",)),
               dict(null=("inv",)), dict(null=("z",))):
        assert ok(**kw) == abi.EARG, kw
        assert ok() == abi.OK
    for v in (np.nan, np.inf, -np.inf):
        bad = x.copy()
        bad[7, 2] = v
        assert K.standardize(pkg, bad)[0] == abi.EARG
    assert K.standardize(pkg, np.full((2, 1), 1.7e308))[0] == abi.EARG  # the column's sum overflows: mu
    assert ok() == abi.OK and lib.gnss_abi_version() == 14


def test_python_layer(pkg):
    """feature_table's columns and their order, knn_train's dropped rows, knn_classify against the
    twin, confusion."""
    w = [3, 2]
    f = NS(prn=[3, 8], windows=np.array(w), **{k: [np.arange(n) + 10.0 * i + c for c, n in enumerate(w)]
                                                for i, k in enumerate(pkg.abi.ACF_FIELDS)})
    X = pkg.feature_table(f)
    assert X.shape == (5, 5)
    for col, name in enumerate(["F1", "F2", "varDelay", "meanCodeDisc", "varCodeDisc"]):
        assert np.array_equal(X[:, col], np.concatenate(getattr(f, name))), name
    for i, k in enumerate(pkg.abi.ACF_EXT_FIELDS):
        setattr(f, k, [np.arange(n) + 100.0 * (i + 1) for n in w])
    fit = NS(prn=[3, 8], windows=np.array(w), bias=[np.full(n, 0.25) for n in w], ratio=[np.full(n, 0.5) for n in w],
             e=[np.full(n, 0.4) for n in w], orient=1)
    X = pkg.feature_table(f, fit)
    assert X.shape == (5, 10) and np.array_equal(X[:, 5], np.concatenate(f.numMLC)) and np.all(X[:, 8] == 0.25)
    assert np.all(X[:, 9] == 0.5)
    X = pkg.feature_table(f, fit, columns=["ratio", "F3", "meanMax", "e"])
    assert X.shape == (5, 4) and np.all(X[:, 0] == 0.5) and np.array_equal(X[:, 1], np.concatenate(f.varDelay))
    assert np.array_equal(X[:, 2], np.concatenate(f.meanMax)) and np.all(X[:, 3] == 0.4)
    for bad in (["F9"], ["bias", "nothing"], ["windows"], ["orient"]):
        with pytest.raises(ValueError):
            pkg.feature_table(f, fit, columns=bad)
    with pytest.raises(ValueError):
        pkg.feature_table(f, None, columns=["bias"])  # no fit given

    x, y = K.table(9, 300, 11)
    x[5, 3], x[200, 0] = np.nan, np.inf
    model = pkg.knn_train(x, y)
    keep = np.all(np.isfinite(x), axis=1)
    assert model.dropped == 2 and model.M == 298 and model.D == 11 and not model.resident
    tmu, tinv, tz = T.standardize(x[keep])
    assert np.array_equal(K.bits(model.z), K.bits(tz)) and np.array_equal(model.label, y[keep])
    q = np.vstack([x[:8], x[keep][:4] + 0.1])
    r = pkg.knn_classify(model, q, k=7, want_neighbours=True)
    label, votes, nn_index, nn_d2 = T.classify(tmu, tinv, tz, y[keep], q, 7, 3)
    assert np.array_equal(r.label, label) and np.array_equal(r.votes, votes) and np.array_equal(r.nn_index, nn_index)
    assert np.array_equal(K.bits(r.nn_d2), K.bits(nn_d2)) and r.label[5] == -1
    bare = pkg.knn_classify(model, q, k=7)
    assert np.array_equal(bare.label, label) and not hasattr(bare, "nn_index")
    model.free()  # nothing resident: a no-op
    with pytest.raises(pkg.abi.GnssError) as e:
        pkg.knn_classify(model, q, k=0)
    assert e.value.status == pkg.abi.EARG
    with pytest.raises(ValueError):
        pkg.knn_classify(model, q[:, :5])
    with pytest.raises(ValueError):
        pkg.knn_train(x, np.full(300, 3))  # a label outside 0..2
    c = pkg.confusion([0, 0, 1, 2, 2, 2], [0, 1, 1, -1, 2, 0])
    assert c.tolist() == [[1, 1, 0, 0], [0, 1, 0, 0], [1, 0, 1, 1]]
