"""What the tests of the k-NN classifier share (test_knn_kat.py on the CPU, test_gpu_knn.py on the
GPU): the calls through the C-ABI with a host or a resident model, seeded tables, and the
bit-for-bit comparisons."""
import ctypes as C

import numpy as np

import knn_twin as T


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def standardize(pkg, x, M=None, D=None, null=()):
    """gnss_knn_standardize -> (status, mu, inv, z)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    M = x.shape[0] if M is None else M
    D = x.shape[1] if D is None else D
    mu, inv, z = np.full(x.shape[1], -7.0), np.full(x.shape[1], -7.0), np.full(x.shape, -7.0)
    p = dict(x=x.ctypes.data, mu=mu.ctypes.data, inv=inv.ctypes.data, z=z.ctypes.data)
    for name in null:
        p[name] = None
    st = pkg.abi.load().gnss_knn_standardize(p["x"], M, D, p["mu"], p["inv"], p["z"])
    return st, mu, inv, z


class Model:
    """A host model from a raw table (standardised by the library) and its labels."""

    def __init__(self, pkg, x, label, n_class=3):
        st, self.mu, self.inv, self.z = standardize(pkg, x)
        assert st == pkg.abi.OK
        self.label = np.ascontiguousarray(label, dtype=np.int32)
        self.n_class = n_class
        self.M, self.D = self.z.shape


class Out:
    """label, votes, nn_index, nn_d2 filled with values no call writes, so an unwritten element shows."""

    def __init__(self, Q, k, n_class, want=True):
        kk = max(k, 1)
        self.label = np.full(max(Q, 1), -9, dtype=np.int32)
        self.votes = np.full((max(Q, 1), n_class), -9, dtype=np.int32)
        self.nn_index = np.full((max(Q, 1), kk), -9, dtype=np.int32) if want else None
        self.nn_d2 = np.full((max(Q, 1), kk), -7.0) if want else None


def classify(pkg, m, q, k, *, ctx=None, host=False, dev=None, want=True, Q=None, null=(), **over):
    """gnss_knn_classify -> (status, Out). dev: (z, label) device pointers of a resident model.
    over: fields of the C model or of the cfg set to other values (the refusals); null: arrays
    passed as NULL."""
    q = np.ascontiguousarray(q, dtype=np.float64)
    Q = q.shape[0] if Q is None else Q
    cfg = pkg.abi.GnssKnnCfg()
    cfg.k, cfg.flags = k, pkg.abi.KNN_HOST if host else 0
    cm = pkg.abi.GnssKnnModel()
    cm.M, cm.D, cm.n_class = m.M, m.D, m.n_class
    cm.mu, cm.inv, cm.z, cm.label = m.mu.ctypes.data, m.inv.ctypes.data, m.z.ctypes.data, m.label.ctypes.data
    if dev is not None:
        cm.z, cm.label, cm.flags = dev[0], dev[1], pkg.abi.KNN_MODEL_DEVICE
    o = Out(Q, k, m.n_class, want)
    co = pkg.abi.GnssKnnOut()
    co.label, co.votes = o.label.ctypes.data, o.votes.ctypes.data
    if want:
        co.nn_index, co.nn_d2 = o.nn_index.ctypes.data, o.nn_d2.ctypes.data
    for name, v in over.items():
        setattr(cfg if name in ("cfg_flags",) else cm, "flags" if name == "cfg_flags" else name, v)
    qp = q.ctypes.data
    for name in null:
        if name == "q":
            qp = None
        elif name in ("label_out", "votes"):
            setattr(co, "label" if name == "label_out" else name, None)
        else:
            setattr(cm, name, None)
    st = pkg.abi.load().gnss_knn_classify(ctx.h if ctx is not None else None, C.byref(cfg), C.byref(cm), qp, Q,
                                          C.byref(co))
    return st, o


def assert_same(a, b, Q=None):
    """Two Outs bit for bit in every element (the optional arrays where both have them)."""
    assert np.array_equal(a.label, b.label), (a.label[:8], b.label[:8])
    assert np.array_equal(a.votes, b.votes)
    if a.nn_index is not None and b.nn_index is not None:
        assert np.array_equal(a.nn_index, b.nn_index), np.argwhere(a.nn_index != b.nn_index)[:4]
        assert np.array_equal(bits(a.nn_d2), bits(b.nn_d2)), np.argwhere(bits(a.nn_d2) != bits(b.nn_d2))[:4]


def assert_equals_twin(o, m, q, k):
    label, votes, nn_index, nn_d2 = T.classify(m.mu, m.inv, m.z, m.label, q, k, m.n_class)
    assert np.array_equal(o.label, label), (o.label[:8], label[:8])
    assert np.array_equal(o.votes, votes)
    assert np.array_equal(o.nn_index, nn_index), np.argwhere(o.nn_index != nn_index)[:4]
    assert np.array_equal(bits(o.nn_d2), bits(nn_d2))


def table(seed, M, D, n_class=3, grid=None):
    """A seeded training table [M][D] with labels; grid: the values are whole multiples of it (many
    exact ties in d2), else normal deviates."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, size=(M, D)).astype(np.float64) * grid if grid else rng.normal(0.0, 1.0, size=(M, D))
    return x, rng.integers(0, n_class, size=M).astype(np.int32)
