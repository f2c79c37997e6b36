"""A numpy restatement of the k-NN classifier (include/gnss_mi355x.h, csrc/knn.h): the reference of
test_knn_kat.py and test_gpu_knn.py. Every operation is one fp64 numpy operation, rounded on its
own; every sum over the columns or over the rows is a Python loop from its first term (np.sum adds
pairwise); the neighbours are np.lexsort((t, d2))[:k], which puts a NaN d2 after +inf."""
import numpy as np


def standardize(x):
    """x [M][D] -> mu [D], inv [D], z [M][D]"""
    x = np.asarray(x, dtype=np.float64)
    M, D = x.shape
    mu, inv = np.zeros(D), np.zeros(D)
    for j in range(D):
        s = x[0, j]
        for t in range(1, M):
            s = s + x[t, j]
        mu[j] = s / np.float64(M)
        d = x[:, j] - mu[j]
        dd = d * d
        q = dd[0]
        for t in range(1, M):
            q = q + dd[t]
        sd = np.sqrt(q / np.float64(M))
        inv[j] = np.float64(0.0) if sd == 0 else np.float64(1.0) / sd
    z = (x - mu[None, :]) * inv[None, :]
    return mu, inv, z


def classify(mu, inv, z, label, q, k, n_class):
    """q [Q][D] -> label [Q], votes [Q][n_class], nn_index [Q][k], nn_d2 [Q][k]"""
    z, q = np.asarray(z, dtype=np.float64), np.asarray(q, dtype=np.float64)
    M, D = z.shape
    Q = q.shape[0]
    out_label = np.full(Q, -1, dtype=np.int32)
    votes = np.zeros((Q, n_class), dtype=np.int32)
    nn_index = np.full((Q, k), -1, dtype=np.int32)
    nn_d2 = np.full((Q, k), np.nan)
    t = np.arange(M)
    with np.errstate(all="ignore"):
        for i in range(Q):
            if not np.all(np.isfinite(q[i])):
                continue
            zq = (q[i] - mu) * inv
            d = zq[0] - z[:, 0]
            d2 = d * d
            for j in range(1, D):
                d = zq[j] - z[:, j]
                d2 = d2 + d * d
            d2 = np.where(np.isnan(d2), np.nan, d2)  # (the one quiet NaN)
            nn = np.lexsort((t, d2))[:k]
            nn_index[i], nn_d2[i] = nn, d2[nn]
            for c in label[nn]:
                votes[i, c] += 1
            most = votes[i].max()
            out_label[i] = next(c for c in label[nn] if votes[i, c] == most)
    return out_label, votes, nn_index, nn_d2
