// knn.hip — gnss_knn_classify on the device (knn.h): Q query rows against M standardised training
// rows of D columns, the k nearest under the total order (d2, t), then the vote. Two kernels.
//   1. knn_scan_kernel<D>, grid (query tiles) x (training splits), kKnnLanes lanes, one query per
//      lane with its D standardised values in registers. The split's training rows go through
//      LDS in tiles of kKnnTile rows (a coalesced copy); every lane reads the same row, so each
//      read is a broadcast. A lane's running k-list lies in LDS as [slot][lane] (a run-time slot
//      index in registers would be scratch; along the lanes the 8-byte and 4-byte columns fall
//      on distinct banks), its last entry (kd, kt) in registers as the admission test: after
//      the first tiles an insertion is rare and a row costs D subtract-multiply-add triples and
//      one compare. The block writes the split's sorted list per query, [split][slot][query].
//   2. knn_merge_kernel, one query per lane: the splits' lists in split order into one k-list by
//      the same insertion (a split's candidates ascend, so the first that is not admitted ends
//      the split), the vote, and the rows of the outputs written along the lanes.
// LDS per block: k * 256 * 12 B for the lists, and in the scan kKnnTile * D * 8 B for the tile:
// k = 15, D = 11: 50.5 KiB, three blocks per CU of 160 KiB; k = 32, D = 16: 104 KiB, one; k = 5:
// the 32 waves of a CU bound it (eight blocks).
// The order is total, so the result does not depend on the splits or the tiles; no atomics, no
// data-dependent grid: two runs give the same bits. The arithmetic is knn.h's, shared with the
// host path, without contraction: the outputs equal the host's bit for bit.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "knn.h"

namespace gnss {
namespace {

// a lane's k-list: column `lane` of the block's [slot][lane] arrays
struct KnnLdsList {
    double* d;
    int32_t* i;
    __device__ double d2(int s) const { return d[s * kKnnLanes]; }
    __device__ int t(int s) const { return i[s * kKnnLanes]; }
    __device__ void set(int s, double v, int t_)
    {
        d[s * kKnnLanes] = v;
        i[s * kKnnLanes] = t_;
    }
};

// Block (x, y): the queries x * 256 .. of split y, the training rows [y * share, (y + 1) * share)
// below M. Lanes past Q work on query Q - 1 and store nothing; every load is inside q [Q][D] and
// z [M][D], every store inside part [splits][k][Q].
template <int D>
__global__ __launch_bounds__(kKnnLanes) void knn_scan_kernel(KnnDev d)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds[];
    const int k = d.k, lane = threadIdx.x;
    double* ld = reinterpret_cast<double*>(knn_lds);            // [k][256]
    double* tile = ld + (size_t)k * kKnnLanes;                  // [kKnnTile][D]
    int32_t* lt = reinterpret_cast<int32_t*>(tile + kKnnTile * D);  // [k][256]

    const int64_t qi = (int64_t)blockIdx.x * kKnnLanes + lane;
    const bool live = qi < d.Q;
    const int64_t qr = live ? qi : d.Q - 1;
    double zq[D];
#pragma unroll
    for (int j = 0; j < D; j++) zq[j] = knn_z(d.q[qr * D + j], d.mu[j], d.inv[j]);

    KnnLdsList l{ld + lane, lt + lane};
    knn_list_clear(l, k);
    double kd = knn_nan();
    int kt = kKnnEmpty;

    const int64_t t0 = (int64_t)blockIdx.y * d.share;
    const int64_t t1 = t0 + d.share < d.M ? t0 + d.share : d.M;
    for (int64_t tb = t0; tb < t1; tb += kKnnTile) {
        const int n = t1 - tb < kKnnTile ? (int)(t1 - tb) : kKnnTile;
        __syncthreads();  // the last tile is read
        for (int i = lane; i < n * D; i += kKnnLanes) tile[i] = d.z[tb * D + i];
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < n; r++) {
            double s = 0;
#pragma unroll
            for (int j = 0; j < D; j++) s = knn_d2_term(s, zq[j], tile[r * D + j], j == 0);
            const double d2 = knn_d2_close(s);
            const int t = (int)(tb + r);
            if (knn_scan_admits(d2, t, kd, kt)) {
                knn_list_insert(l, k, d2, t);
                kd = l.d2(k - 1);
                kt = l.t(k - 1);
            }
        }
    }
    if (live)
        for (int i = 0; i < k; i++) {
            const int64_t o = ((int64_t)blockIdx.y * k + i) * d.Q + qi;
            d.part_d2[o] = l.d2(i);
            d.part_t[o] = l.t(i);
        }
}

// Block x: the queries x * 256 .. . The lists hold training rows only (k <= M and the splits
// cover every row), so label[t] is inside label [M].
__global__ __launch_bounds__(kKnnLanes) void knn_merge_kernel(KnnDev d)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds[];
    const int k = d.k, lane = threadIdx.x;
    double* ld = reinterpret_cast<double*>(knn_lds);                          // [k][256]
    int32_t* lt = reinterpret_cast<int32_t*>(ld + (size_t)k * kKnnLanes);     // [k][256]

    const int64_t q0 = (int64_t)blockIdx.x * kKnnLanes;
    const int64_t qi = q0 + lane;
    const bool live = qi < d.Q;
    const int64_t qr = live ? qi : d.Q - 1;

    KnnLdsList l{ld + lane, lt + lane};
    knn_list_clear(l, k);
    for (int s = 0; s < d.splits; s++)
        for (int i = 0; i < k; i++) {
            const int64_t o = ((int64_t)s * k + i) * d.Q + qr;
            const double cd = d.part_d2[o];
            const int ct = d.part_t[o];
            if (!knn_before(cd, ct, l.d2(k - 1), l.t(k - 1))) break;
            knn_list_insert(l, k, cd, ct);
        }

    bool ok = true;
    for (int j = 0; j < d.D; j++) ok = ok && knn_finite(d.q[qr * d.D + j]);
    uint64_t v = 0;
    int win = -1;
    if (ok) {
        win = knn_vote(l, k, d.label, d.n_class, &v);
    } else {
        for (int i = 0; i < k; i++) l.set(i, knn_nan(), -1);
    }
    if (live) {
        d.out_label[qi] = win;
        for (int c = 0; c < d.n_class; c++) d.out_votes[qi * d.n_class + c] = knn_vote_of(v, c);
    }
    __syncthreads();
    // the block's rows of nn_index / nn_d2 [Q][k] are one contiguous run: along the lanes
    const int64_t rest = d.Q - q0;
    const int nq = rest < kKnnLanes ? (int)rest : kKnnLanes;
    for (int i = lane; i < nq * k; i += kKnnLanes) {
        const int ql = i / k, r = i % k;
        d.out_index[q0 * k + i] = lt[r * kKnnLanes + ql];
        d.out_d2[q0 * k + i] = ld[r * kKnnLanes + ql];
    }
}

template <int D>
hipError_t scan_launch(const KnnDev& d, dim3 grid, hipStream_t stream)
{
    const size_t lds = knn_lds_scan(D, d.k);
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&knn_scan_kernel<D>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(knn_scan_kernel<D>, grid, dim3(kKnnLanes), lds, stream, d);
    return hipGetLastError();
}

}  // namespace

int knn_launch(const KnnDev& d, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (d.Q <= 0) return 0;
    const unsigned qt = (unsigned)((d.Q + kKnnLanes - 1) / kKnnLanes);
    const dim3 grid(qt, (unsigned)d.splits);
    hipError_t e = hipErrorInvalidValue;
    switch (d.D) {
#define GNSS_KNN_CASE(n) \
    case n: e = scan_launch<n>(d, grid, stream); break;
        GNSS_KNN_CASE(1) GNSS_KNN_CASE(2) GNSS_KNN_CASE(3) GNSS_KNN_CASE(4)
        GNSS_KNN_CASE(5) GNSS_KNN_CASE(6) GNSS_KNN_CASE(7) GNSS_KNN_CASE(8)
        GNSS_KNN_CASE(9) GNSS_KNN_CASE(10) GNSS_KNN_CASE(11) GNSS_KNN_CASE(12)
        GNSS_KNN_CASE(13) GNSS_KNN_CASE(14) GNSS_KNN_CASE(15) GNSS_KNN_CASE(16)
#undef GNSS_KNN_CASE
    }
    if (e != hipSuccess) return (int)e;
    const size_t lds = knn_lds_merge(d.k);
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&knn_merge_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(knn_merge_kernel, dim3(qt), dim3(kKnnLanes), lds, stream, d);
    return (int)hipGetLastError();
}

}  // namespace gnss
