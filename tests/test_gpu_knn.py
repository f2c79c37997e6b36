"""GPU tests of the k-NN classifier (gnss_knn_classify with a context, csrc/knn.hip): the device
outputs -- label, votes, nn_index, nn_d2 -- equal the host path's bit for bit over the query
counts around a block, the training sizes around a tile and around a split's share, D = 1, 11, 16
and k = 1, 5, 32, and once more with the optional arrays NULL; exact ties across a tile boundary and
a split boundary; non-finite queries among finite ones; a resident model; two runs; the refusals,
each leaving the context usable; end to end: DESIGN §3.3's three scenes as the training set, the
training windows themselves and a held-out trio classified."""
import ctypes as C

import numpy as np
import pytest

import knn_common as K
from conftest import acquired_of, params

pytestmark = pytest.mark.gpu

# csrc/knn.h: kKnnLanes queries per block, kKnnTile training rows per LDS tile, and
# knn_split_share(M, Q): for Q <= 32 * LANES and M <= 64 * SHARE a split takes kKnnShareMin rows
LANES, TILE, SHARE = 256, 64, 1024
QS = [1, LANES - 1, LANES, LANES + 1, 2 * LANES + 88]  # the last: three query blocks
MS = ["k", TILE - 1, TILE, TILE + 1, SHARE - 1, SHARE, SHARE + 1, 3 * SHARE + 2 * TILE]  # the last: four splits


def queries(x, Q, D, seed, grid):
    rng = np.random.default_rng(seed)
    q = rng.integers(-3, 4, size=(Q, D)) * grid if grid else rng.normal(0.0, 1.5, size=(Q, D))
    n = min(Q, len(x), 7)
    q[Q - n:] = x[:n]  # some training rows themselves: d2 = 0
    return q


def device_equals_host(pkg, ctx, m, q, k):
    st, host = K.classify(pkg, m, q, k)
    assert st == pkg.abi.OK
    st, dev = K.classify(pkg, m, q, k, ctx=ctx)
    assert st == pkg.abi.OK, ctx.lib.gnss_last_error(ctx.h)
    K.assert_same(host, dev)
    return host


@pytest.mark.parametrize("k", [1, 5, 32])
@pytest.mark.parametrize("D", [1, 11, 16])
def test_device_path_equals_host(pkg, ctx, D, k):
    """Every M of MS at Q = LANES + 1 and every Q of QS at M = SHARE + 1; the tables alternate
    between normal deviates and a coarse grid whose many equal distances the order breaks by row."""
    cases = [(M, LANES + 1) for M in MS] + [(SHARE + 1, Q) for Q in QS]
    for n, (M, Q) in enumerate(cases):
        M = k if M == "k" else M
        grid = 0.5 if n % 2 else None
        x, y = K.table(1000 * D + 10 * k + n, M, D, grid=grid)
        m = K.Model(pkg, x, y)
        q = queries(x, Q, D, n, grid)
        host = device_equals_host(pkg, ctx, m, q, k)
        assert host.nn_index[Q - 1, 0] >= 0 and host.nn_d2[Q - 1, 0] == 0.0, (M, Q)
        if n in (0, 7, 12):
            st, bare = K.classify(pkg, m, q, k, ctx=ctx, want=False)  # nn_index / nn_d2 NULL
            assert st == pkg.abi.OK
            K.assert_same(host, bare)


def test_ties_across_tile_and_split_boundaries(pkg, ctx):
    """One row repeated on both sides of a tile boundary (rows 63 | 64), of the first split's
    boundary (1023 | 1024), of the second's (2047 | 2048) and elsewhere: queried itself, every copy
    is at d2 = 0 and the merged list keeps the lower rows, ascending; a second group of copies one
    grid step away ties at the next distance."""
    D, M = 3, 3 * SHARE + 2 * TILE
    x, y = K.table(77, M, D)
    copies = [10, TILE - 1, TILE, SHARE - 1, SHARE, 2 * SHARE - 1, 2 * SHARE, 3000]
    near = [5, 2 * TILE - 1, 2 * TILE, SHARE + TILE - 1, SHARE + TILE, 3 * SHARE - 1, 3 * SHARE, M - 1]
    x[copies] = [0.25, -0.5, 1.0]
    x[near] = [0.25, -0.5, 1.0 + 2.0 ** -20]
    m = K.Model(pkg, x, y)
    q = np.tile(x[10], (LANES + 1, 1))
    q[1::2] = x[5]
    for k in (1, 5, 8, 12, 32):
        host = device_equals_host(pkg, ctx, m, q, k)
        both = sorted(copies) + sorted(near)
        assert list(host.nn_index[0][: min(k, 16)]) == both[: min(k, 16)], (k, host.nn_index[0])
        other = sorted(near) + sorted(copies)
        assert list(host.nn_index[1][: min(k, 16)]) == other[: min(k, 16)], (k, host.nn_index[1])
        assert np.all(host.nn_d2[0][: min(k, 8)] == 0.0)


def test_non_finite_queries_among_finite_ones(pkg, ctx):
    D, k = 11, 5
    x, y = K.table(5, SHARE + 1, D)
    x[:, 4] = 2.5  # a constant column: inv = 0
    m = K.Model(pkg, x, y)
    assert m.inv[4] == 0.0
    q = queries(x, 2 * LANES + 88, D, 1, None)
    bad = {3: (0, np.nan), 63: (4, np.inf), 64: (4, np.nan), LANES - 1: (10, -np.inf), LANES: (0, np.inf),
           2 * LANES + 87: (7, np.nan)}
    for row, (col, v) in bad.items():
        q[row, col] = v
    host = device_equals_host(pkg, ctx, m, q, k)
    for row in range(len(q)):
        if row in bad:
            assert host.label[row] == -1 and np.all(host.votes[row] == 0) and np.all(host.nn_index[row] == -1)
            assert np.all(K.bits(host.nn_d2[row]) == 0x7FF8000000000000)
        else:
            assert host.label[row] >= 0 and host.votes[row].sum() == k and np.all(np.isfinite(host.nn_d2[row]))
    # a finite query so far out that q - mu overflows on the constant column: NaN distances, in row order
    q[0, 4] = -1.7e308
    m.mu[4] = 1.7e308  # (a model a caller made: the standardisation itself refuses such a column)
    host = device_equals_host(pkg, ctx, m, q[:5], k)
    assert list(host.nn_index[0]) == [0, 1, 2, 3, 4] and np.all(K.bits(host.nn_d2[0]) == 0x7FF8000000000000)


class Resident:
    """z and label of a host model in the context's HBM (gnss_dev_alloc / gnss_dev_upload)."""

    def __init__(self, ctx, m):
        self.ctx, self.ptr = ctx, []
        for a in (m.z, m.label):
            p = C.c_void_p()
            ctx.check(ctx.lib.gnss_dev_alloc(ctx.h, C.c_uint64(a.nbytes), C.byref(p)))
            self.ptr.append(p)
            ctx.check(ctx.lib.gnss_dev_upload(ctx.h, p, a.ctypes.data_as(C.c_void_p), C.c_uint64(a.nbytes)))
        self.dev = (self.ptr[0].value, self.ptr[1].value)

    def free(self):
        for p in self.ptr:
            self.ctx.lib.gnss_dev_free(self.ctx.h, p)


def test_resident_model_and_two_runs(pkg, ctx):
    D, k, M, Q = 11, 15, 2 * SHARE + 5, LANES + 1
    x, y = K.table(21, M, D)
    m = K.Model(pkg, x, y)
    q = queries(x, Q, D, 2, None)
    host = device_equals_host(pkg, ctx, m, q, k)
    r = Resident(ctx, m)
    try:
        for _ in range(2):
            st, dev = K.classify(pkg, m, q, k, ctx=ctx, dev=r.dev)
            assert st == pkg.abi.OK, ctx.lib.gnss_last_error(ctx.h)
            K.assert_same(host, dev)
        st, again = K.classify(pkg, m, q, k, ctx=ctx)
        assert st == pkg.abi.OK
        K.assert_same(dev, again)
        st, on_host = K.classify(pkg, m, q, k, ctx=ctx, host=True)  # GNSS_KNN_HOST with a context
        assert st == pkg.abi.OK
        K.assert_same(host, on_host)
    finally:
        r.free()


def test_python_layer_with_a_resident_model(pkg, ctx):
    x, y = K.table(31, SHARE + 77, 8)
    x[9, 2] = np.nan
    q = queries(x[10:], 300, 8, 3, None)
    plain = pkg.knn_train(x, y)
    want = pkg.knn_classify(plain, q, k=5, want_neighbours=True)
    model = pkg.knn_train(x, y, ctx=ctx)
    try:
        assert model.resident and model.dropped == 1 and model.M == SHARE + 76
        got = pkg.knn_classify(model, q, k=5, want_neighbours=True)
        up = pkg.knn_classify(plain, q, k=5, ctx=ctx, want_neighbours=True)  # uploaded for the call
    finally:
        model.free()
    assert not model.resident
    for r in (got, up):
        assert np.array_equal(r.label, want.label) and np.array_equal(r.votes, want.votes)
        assert np.array_equal(r.nn_index, want.nn_index) and np.array_equal(K.bits(r.nn_d2), K.bits(want.nn_d2))
    assert np.array_equal(pkg.knn_classify(model, q, k=5).label, want.label)  # freed: the host path


def test_refusals_leave_the_context_usable(pkg, ctx):
    abi = pkg.abi
    x, y = K.table(3, SHARE + 40, 4)
    m = K.Model(pkg, x, y)
    q = x[:5] + 0.25
    _, good = K.classify(pkg, m, q, 5)
    r = Resident(ctx, m)
    try:
        def fine():
            for dev in (None, r.dev):
                st, o = K.classify(pkg, m, q, 5, ctx=ctx, dev=dev)
                assert st == abi.OK
                K.assert_same(good, o)

        fine()
        for kw in (dict(D=0), dict(D=17), dict(n_class=0), dict(n_class=9), dict(M=0), dict(M=(1 << 24) + 1),
                   dict(flags=2), dict(cfg_flags=4), dict(Q=-1), dict(null=("q",)), dict(null=("mu",)),
                   dict(null=("z",)), dict(null=("label",)), dict(null=("label_out",)), dict(null=("votes",))):
            assert K.classify(pkg, m, q, 5, ctx=ctx, **kw)[0] == abi.EARG, kw
            assert ctx.lib.gnss_last_error(ctx.h)
            fine()
        for k in (0, 33):
            assert K.classify(pkg, m, q, k, ctx=ctx)[0] == abi.EARG, k
            fine()
        small = K.Model(pkg, x[:7], y[:7])
        assert K.classify(pkg, small, q, 8, ctx=ctx)[0] == abi.EARG  # k above M
        fine()
        keep = m.label[17]
        m.label[17] = 3  # (the host model's label: checked before the upload)
        assert K.classify(pkg, m, q, 5, ctx=ctx)[0] == abi.EARG
        m.label[17] = keep
        fine()
        bad = np.array([3], dtype=np.int32)  # (the resident model's: it comes back for the check)
        ctx.check(ctx.lib.gnss_dev_upload(ctx.h, C.c_void_p(r.dev[1] + 4 * 17), bad.ctypes.data_as(C.c_void_p), 4))
        assert K.classify(pkg, m, q, 5, ctx=ctx, dev=r.dev)[0] == abi.EARG
        ctx.check(ctx.lib.gnss_dev_upload(ctx.h, C.c_void_p(r.dev[1] + 4 * 17),
                                          m.label[17:18].ctypes.data_as(C.c_void_p), 4))
        fine()
        assert K.classify(pkg, m, q, 5, dev=r.dev)[0] == abi.EARG  # a device model without a context
        assert K.classify(pkg, m, q, 5, ctx=ctx, dev=r.dev, host=True)[0] == abi.EARG  # ... on the host path
        assert K.classify(pkg, m, q, 5, ctx=ctx, flags=abi.KNN_MODEL_DEVICE)[0] == abi.EARG  # host arrays as device
        fine()
        multi = pkg.Context(devices=[0, 0])
        try:
            assert K.classify(pkg, m, q, 5, ctx=multi)[0] == abi.EARG
            st, o = K.classify(pkg, m, q, 5, ctx=multi, host=True)  # the host path needs no device
            assert st == abi.OK
            K.assert_same(good, o)
        finally:
            multi.close()
        st, o = K.classify(pkg, m, q, 5, ctx=ctx, Q=0)
        assert st == abi.OK and np.all(o.label == -9) and np.all(o.nn_index == -9)
        fine()
    finally:
        r.free()


# ---- end to end --------------------------------------------------------------------------------
def scene(pkg, kind, seed, delay=None, gain=None):
    """DESIGN §3.3's scenes: PRN 3 alone at 55 dB-Hz; 'clean', 'ray' (a ray `delay` chips late at
    `gain`), 'nlos' (no direct signal, only that ray)"""
    sc = pkg.synth.scene_of(pkg.synth.scenario([3], [3683], [990.0], [55.0], skip_ms=2, seed=seed))
    if kind == "nlos":
        pkg.synth.set_nlos(sc, 3)
    if kind != "clean":
        pkg.synth.add_ray(sc, 3, delay, gain)
    return sc


def windows_of(pkg, ctx, sc):
    """600 rows of gnss_tracking_ct_multicorr (five windows), their features, fit and labels"""
    dev = pkg.DeviceRecord(ctx, 2 * (2 + 1 + 600 + 4) * 58000)
    try:
        pkg.synth.generate_scene_device(ctx, sc, dev)
        file, signal, acq, track = params(pkg, 2, None)
        file.dev = dev
        tck, _ = pkg.trackingCT_multiCorr(file, signal, track, acquired_of([3], [3683], [4580990.0]), datalength=600,
                                          ctx=ctx)
    finally:
        dev.free()
    X = pkg.feature_table(pkg.acf_features(tck, [3], [45.0]), pkg.acf_fit(tck, [3]))
    y = np.concatenate(pkg.scene_labels(sc, tck, [3]))
    assert X.shape == (5, 7) and y.shape == (5,)
    return X, y


@pytest.fixture(scope="module")
def sets(pkg, ctx):
    train = [windows_of(pkg, ctx, scene(pkg, "clean", 6102)), windows_of(pkg, ctx, scene(pkg, "ray", 6102, 0.5, 0.5)),
             windows_of(pkg, ctx, scene(pkg, "nlos", 6102, 0.4, 0.7))]
    held = [windows_of(pkg, ctx, scene(pkg, "clean", 7203)), windows_of(pkg, ctx, scene(pkg, "ray", 7203, 0.45, 0.55)),
            windows_of(pkg, ctx, scene(pkg, "nlos", 7203, 0.35, 0.65))]
    return train, held


def test_training_windows_get_their_own_label(pkg, ctx, sets):
    train, _ = sets
    X, y = np.vstack([t[0] for t in train]), np.concatenate([t[1] for t in train])
    assert list(y) == [0] * 5 + [1] * 5 + [2] * 5
    model = pkg.knn_train(X, y, ctx=ctx)
    try:
        assert model.dropped == 0
        r = pkg.knn_classify(model, X, k=1, want_neighbours=True)
    finally:
        model.free()
    assert np.array_equal(r.label, y) and np.all(r.nn_d2[:, 0] == 0.0)
    assert np.array_equal(r.nn_index[:, 0], np.arange(15))
    h = pkg.knn_classify(model, X, k=1, want_neighbours=True)  # the host path: the same bits
    assert np.array_equal(h.label, r.label) and np.array_equal(K.bits(h.nn_d2), K.bits(r.nn_d2))


def test_held_out_windows_after_pull_in(pkg, ctx, sets):
    """Another noise seed and nearby ray parameters; window 0 (pull-in) left out; k = 5: more than
    half of each class's windows get their class."""
    train, held = sets
    X, y = np.vstack([t[0] for t in train]), np.concatenate([t[1] for t in train])
    Xh, yh = np.vstack([t[0][1:] for t in held]), np.concatenate([t[1][1:] for t in held])
    assert list(yh) == [0] * 4 + [1] * 4 + [2] * 4
    model = pkg.knn_train(X, y, ctx=ctx)
    try:
        r = pkg.knn_classify(model, Xh, k=5, want_neighbours=True)
    finally:
        model.free()
    c = pkg.confusion(yh, r.label)
    print("columns F1 F2 F3 F4 F5 bias ratio; training rows\n", np.round(X, 4), "\nheld-out rows\n", np.round(Xh, 4))
    print("votes\n", r.votes, "\nconfusion (rows: truth 0 1 2; columns: predicted 0 1 2, none)\n", c)
    for cls in range(3):
        assert 2 * c[cls, cls] > c[cls].sum(), (cls, c)
