// knn.h — the k-nearest-neighbour classifier over standardised feature rows (gnss_knn_standardize,
// gnss_knn_classify; the definition is in include/gnss_mi355x.h). One source for the arithmetic,
// called in loops by the host path (knn.cpp) and by the kernels (knn.hip), compiled without
// contraction and without fast-math on both sides; every sum runs left to right from its first
// term: the two paths give the same bits.
//   - standardisation: mu, sd and inv = 1 / sd per column (0 for a constant column), z = (x - mu) * inv;
//   - a query's distance to training row t: d2 = sum_j (zq[j] - z[t][j])^2, j ascending;
//   - neighbours: the k smallest rows under the total order (d2, t), a NaN d2 after +inf (a finite
//     query far enough out overflows q - mu, and inf * 0 on a constant column is NaN; every NaN
//     d2 is stored as the one quiet NaN, so host and device agree on its bits too);
//   - the vote, a tie going to the class of the nearest neighbour among the tied classes.
// A k-list is kept sorted by insertion; its storage is the caller's (the host's arrays, the
// kernels' LDS columns), reached through a small accessor, so the walk is written once.
// No HIP include and no project include: tests/native/knn_host.cpp calls these functions on the
// CPU under AddressSanitizer and UBSan.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define GNSS_KNN_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define GNSS_KNN_HD inline
#endif

namespace gnss {

constexpr int kKnnMaxD = 16;
constexpr int kKnnMaxK = 32;
constexpr int kKnnMaxClass = 8;
constexpr int64_t kKnnMaxM = (int64_t)1 << 24;
constexpr int kKnnEmpty = 0x7fffffff;  // the training index of an empty k-list slot (its d2 is NaN)

// the device plan (knn.hip; tests/test_gpu_knn.py restates these)
constexpr int kKnnLanes = 256;       // queries per block, one per lane
constexpr int kKnnTile = 64;         // training rows per LDS tile
constexpr int kKnnShareMin = 1024;   // training rows per split at least
constexpr int kKnnMaxSplits = 64;
constexpr size_t kKnnLdsPerCu = 160 * 1024;  // gfx950
constexpr int kKnnMaxBlocksPerCu = 8;        // 32 waves per CU, four per block

GNSS_KNN_HD bool knn_finite(double x)
{
    return x - x == 0;
}

GNSS_KNN_HD double knn_nan()
{
    return __builtin_nan("");
}

// ---- standardisation (host, once per model) ----------------------------------------------------
// column j of x[M][D]: mu and inv; false for a non-finite value, mu, sd or inv
inline bool knn_column_stats(const double* x, int64_t M, int D, int j, double* mu, double* inv)
{
    double s = 0;
    for (int64_t t = 0; t < M; t++) {
        const double v = x[t * D + j];
        if (!knn_finite(v)) return false;
        s = t ? s + v : v;
    }
    const double m = s / (double)M;
    double q = 0;
    for (int64_t t = 0; t < M; t++) {
        const double d = x[t * D + j] - m;
        const double dd = d * d;
        q = t ? q + dd : dd;
    }
    const double sd = std::sqrt(q / (double)M);
    const double r = sd == 0 ? 0.0 : 1.0 / sd;
    *mu = m;
    *inv = r;
    return knn_finite(m) && knn_finite(sd) && knn_finite(r);
}

GNSS_KNN_HD double knn_z(double x, double mu, double inv)
{
    return (x - mu) * inv;
}

// ---- distance ------------------------------------------------------------------------------------
// one more column into d2: acc + (a - b) * (a - b), the first column's term as it is
GNSS_KNN_HD double knn_d2_term(double acc, double a, double b, bool first)
{
    const double d = a - b;
    const double dd = d * d;
    return first ? dd : acc + dd;
}

// a NaN distance as the one quiet NaN
GNSS_KNN_HD double knn_d2_close(double d2)
{
    return d2 == d2 ? d2 : knn_nan();
}

GNSS_KNN_HD double knn_d2(const double* zq, const double* zt, int D)
{
    double s = 0;
    for (int j = 0; j < D; j++) s = knn_d2_term(s, zq[j], zt[j], j == 0);
    return knn_d2_close(s);
}

// ---- the order -----------------------------------------------------------------------------------
// (a, ta) before (b, tb): the smaller d2, a NaN after every number, the smaller index on a tie
GNSS_KNN_HD bool knn_before(double a, int ta, double b, int tb)
{
    if (a < b) return true;
    if (a > b) return false;
    const bool an = a != a, bn = b != b;
    if (an != bn) return bn;
    return ta < tb;  // equal numbers, or both NaN
}

// A candidate that cannot be before the list's last entry (kd, kt) when the rows are scanned in
// ascending t and every entry of the list came from an earlier row: d2 >= kd (then an equal d2
// loses the tie, kt being smaller). Otherwise knn_before decides. One compare per row on the
// common path.
GNSS_KNN_HD bool knn_scan_admits(double d2, int t, double kd, int kt)
{
    return !(d2 >= kd) && knn_before(d2, t, kd, kt);
}

// ---- the sorted k-list -----------------------------------------------------------------------------
// L: d2(i), t(i), set(i, d2, t) over the slots 0..k-1 of one query
template <class L>
GNSS_KNN_HD void knn_list_clear(L& l, int k)
{
    for (int i = 0; i < k; i++) l.set(i, knn_nan(), kKnnEmpty);
}

// (d2, t), known to be before the last entry, into its place; the last entry drops out
template <class L>
GNSS_KNN_HD void knn_list_insert(L& l, int k, double d2, int t)
{
    int i = k - 1;
    while (i > 0) {
        const double pd = l.d2(i - 1);
        const int pt = l.t(i - 1);
        if (!knn_before(d2, t, pd, pt)) break;
        l.set(i, pd, pt);
        i--;
    }
    l.set(i, d2, t);
}

// ---- the vote ----------------------------------------------------------------------------------------
// votes of up to 8 classes, a byte each (k <= 32)
GNSS_KNN_HD uint64_t knn_vote_add(uint64_t v, int c)
{
    return v + ((uint64_t)1 << (8 * c));
}
GNSS_KNN_HD int knn_vote_of(uint64_t v, int c)
{
    return (int)((v >> (8 * c)) & 0xff);
}

// L as above, filled and sorted (every slot a training row: k <= M); label[t] in 0..n_class-1.
// Returns the class with the most votes, among tied classes the one of the nearest neighbour.
template <class L>
GNSS_KNN_HD int knn_vote(const L& l, int k, const int32_t* label, int n_class, uint64_t* votes)
{
    uint64_t v = 0;
    for (int i = 0; i < k; i++) v = knn_vote_add(v, label[l.t(i)]);
    int most = 0;
    for (int c = 0; c < n_class; c++) most = knn_vote_of(v, c) > most ? knn_vote_of(v, c) : most;
    int win = -1;
    for (int i = 0; i < k && win < 0; i++) {
        const int c = label[l.t(i)];
        if (knn_vote_of(v, c) == most) win = c;
    }
    *votes = v;
    return win;
}

// ---- the host's k-list and one query on the host -----------------------------------------------------
struct KnnHostList {
    double* d;
    int32_t* i;
    double d2(int s) const { return d[s]; }
    int t(int s) const { return i[s]; }
    void set(int s, double v, int t_) { d[s] = v; i[s] = t_; }
};

// One query q[D] against z[M][D]: nn_d2[k], nn_index[k] (ascending under the order) and
// votes[n_class]; returns the label. A non-finite q[j]: -1, votes 0, indices -1, d2 NaN.
inline int knn_query(const double* q, const double* mu, const double* inv, const double* z, const int32_t* label,
                     int64_t M, int D, int k, int n_class, double* nn_d2, int32_t* nn_index, int32_t* votes)
{
    KnnHostList l{nn_d2, nn_index};
    bool ok = true;
    double zq[kKnnMaxD];
    for (int j = 0; j < D; j++) {
        ok = ok && knn_finite(q[j]);
        zq[j] = knn_z(q[j], mu[j], inv[j]);
    }
    if (!ok) {
        for (int i = 0; i < k; i++) l.set(i, knn_nan(), -1);
        for (int c = 0; c < n_class; c++) votes[c] = 0;
        return -1;
    }
    knn_list_clear(l, k);
    for (int64_t t = 0; t < M; t++) {
        const double d2 = knn_d2(zq, z + t * D, D);
        if (knn_scan_admits(d2, (int)t, l.d2(k - 1), l.t(k - 1))) knn_list_insert(l, k, d2, (int)t);
    }
    uint64_t v;
    const int win = knn_vote(l, k, label, n_class, &v);
    for (int c = 0; c < n_class; c++) votes[c] = knn_vote_of(v, c);
    return win;
}

// ---- the device plan ------------------------------------------------------------------------------------
// LDS bytes of a block of the two kernels: the lanes' k-lists, and in the scan the tile
inline size_t knn_lds_scan(int D, int k)
{
    return (size_t)k * kKnnLanes * (sizeof(double) + sizeof(int32_t)) + (size_t)kKnnTile * D * sizeof(double);
}
inline size_t knn_lds_merge(int k)
{
    return (size_t)k * kKnnLanes * (sizeof(double) + sizeof(int32_t));
}

// blocks of the scan that are resident at once on `cus` compute units
inline int64_t knn_block_slots(int D, int k, int cus)
{
    const int64_t per_cu = (int64_t)(kKnnLdsPerCu / knn_lds_scan(D, k));
    return (int64_t)cus * (per_cu > kKnnMaxBlocksPerCu ? kKnnMaxBlocksPerCu : per_cu < 1 ? 1 : per_cu);
}

// Training rows per split. The grid is (query tiles) x (splits). Every split starts its lists
// empty, and while a list is young some lane of a wave inserts at nearly every row (64 lanes x
// k / t per row t of the split), so splits are not free: as many as fill the resident block
// `slots` once and no more (a second, nearly empty round would double the time), each a whole
// number of tiles and kKnnShareMin rows at least, kKnnMaxSplits at most.
inline int64_t knn_split_share(int64_t M, int64_t Q, int64_t slots)
{
    const int64_t qt = (Q + kKnnLanes - 1) / kKnnLanes;
    int64_t want = slots / (qt > 0 ? qt : 1);
    want = want < 1 ? 1 : want > kKnnMaxSplits ? kKnnMaxSplits : want;
    int64_t share = (M + want - 1) / want;
    share = (share + kKnnTile - 1) / kKnnTile * kKnnTile;
    return share < kKnnShareMin ? kKnnShareMin : share;
}

// What the kernels take (knn.hip). Every extent was checked by the host.
struct KnnDev {
    const double* q;        // [Q][D], raw
    const double* z;        // [M][D]
    const int32_t* label;   // [M], each in 0..n_class-1
    double mu[kKnnMaxD], inv[kKnnMaxD];
    int64_t Q, M;
    int D, k, n_class;
    int64_t share;          // training rows per split
    int splits;             // ceil(M / share)
    double* part_d2;        // [splits][k][Q]: the splits' sorted lists, queries along the rows
    int32_t* part_t;        // [splits][k][Q]
    int32_t* out_label;     // [Q]
    int32_t* out_votes;     // [Q][n_class]
    int32_t* out_index;     // [Q][k]
    double* out_d2;         // [Q][k]
};

// Both kernels on `stream` (a hipStream_t) of the current device. Returns the hipError_t of the
// launches (0: none).
int knn_launch(const KnnDev& d, void* stream);

}  // namespace gnss
