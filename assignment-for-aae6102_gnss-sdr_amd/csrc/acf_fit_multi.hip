// acf_fit_multi.hip — the multi-ray fit of an ACF on any tap grid over device-resident sums
// (acf_fit_multi.h; GNSS_OUT_DEVICE), in the layout gnss_replay_correlate writes:
// [n][2][n_taps][max_rows]. One kernel, one block of kThreads lanes per (channel, window), no
// hand-off between blocks, no persistent loop, two stages:
//   1. the coherent sums: acf_fit_taps.hip's tiled stage, the same code (acf_fit_taps_dev.h).
//   2. the searches. The tap coordinates (us), the coherent vector (zs), the slots' r vectors (rs,
//      4 x n_taps; the searched slot's row idles during its search and takes the winner after it)
//      and the window's state (AcfFmmWork) stay in LDS and are read as broadcasts. A search: up to
//      24 lanes form the sums among the fixed slots and with z once (fmm_sys_fill); lane t takes
//      the candidates t, t + kThreads, ..., forms its own r on the fly and keeps the lexicographic
//      minimum of (res, i) of its share; the block takes the minimum of those by shuffles within a
//      wave and through LDS across the waves, where every lane reads all four entries, so every
//      lane holds the winner and the sweeps' early exit is uniform over the block. No float
//      atomics: a total order's minimum does not depend on the order it is taken in, and two runs
//      give the same bits. The lanes then write the winner's r vector into its row of rs.
// The order of the searches (fmm_orders), the selection and the row (fmm_row, lane 0) are
// acf_fit_multi.h's, shared with the host path; loops are bounded by q_count, max_paths and sweeps,
// which the host checked (acf_fit_multi.cpp). The arithmetic is compiled without contraction: the
// outputs equal the host's bit for bit.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "acf_fit_multi.h"
#include "acf_fit_taps_dev.h"

namespace gnss {
namespace {

using namespace fttdev;

// the block's side of a search (fmm_orders' Ops); every lane of the block calls every member
struct BlockOps {
    const AcfFmmPar& p;
    AcfFmmWork& w;
    double* rs;
    const double *us, *zI, *zQ;
    double* wres;
    int* wh;

    __device__ AcfFttBest search(int m, int k)
    {
        const int tid = threadIdx.x;
        fmm_sys_fill(w, rs, m, k, p.n_taps, zI, zQ, tid, kThreads);
        __syncthreads();
        AcfFttBest b = wave_best(fmm_search_share(p, w, rs, m, k, us, zI, zQ, tid, kThreads));
        if ((tid & 63) == 0) {
            wres[tid >> 6] = b.res;
            wh[tid >> 6] = b.h;
        }
        __syncthreads();
        b = AcfFttBest{wres[0], wh[0]};
        for (int v = 1; v < kWaves; v++) ftt_best_merge(b, wres[v], wh[v]);
        if (b.h != kFttNone) fmm_place(p, w, rs, k, b.h, us, tid, kThreads);  // (uniform over the block)
        __syncthreads();  // rs, w.pos; wres / wh are free again
        return b;
    }
    __device__ void sync() { __syncthreads(); }
};

// window blockIdx.x of all channels' windows in channel order (block_window)
__global__ __launch_bounds__(kThreads) void acf_fit_multi_kernel(AcfFmmDev d)
{
    __shared__ double tile[kGroup * kStride];
    __shared__ double sg[kTile];             // the row tile's signs
    __shared__ double zs[2 * kFttMaxTaps];   // zI[n_taps] then zQ[n_taps]
    __shared__ double us[kFttMaxTaps];
    __shared__ double rs[kFmmMaxPaths * kFttMaxTaps];  // the slots' r vectors, [slot][n_taps]
    __shared__ AcfFmmWork work;
    __shared__ double wres[kWaves];
    __shared__ int wh[kWaves];

    const int tid = threadIdx.x;
    const int nt = d.par.n_taps;

    // stage 1
    block_window(d.io, nt, d.par.prompt, tile, sg, zs, us);
    for (int i = tid; i < kFmmMaxPaths * nt; i += kThreads) rs[i] = 0.0;
    if (tid < kFmmMaxPaths) work.pos[tid] = 0;  // (a slot's row and index are read, and masked, before it is placed)
    __syncthreads();

    // stage 2
    const double* zI = zs;
    const double* zQ = zs + nt;
    const bool finite = ftt_all_finite(nt, zI, zQ);  // (uniform over the block)
    int formed = 0, searches = 0, sel = 0;
    if (finite) {
        if (tid == 0) work.res[0] = ftt_energy(nt, zI, zQ);
        BlockOps ops{d.par, work, rs, us, zI, zQ, wres, wh};
        formed = fmm_orders(d.par, work, ops, tid == 0, &searches);
        sel = fmm_paths(d.par, work, formed);
        for (int l = 0; l < sel; l++) fmm_place(d.par, work, rs, l, work.kept[sel - 1][l], us, tid, kThreads);
        __syncthreads();
        fmm_sys_fill(work, rs, sel, -1, nt, zI, zQ, tid, kThreads);
        __syncthreads();
    }
    if (tid == 0) fmm_row(d.par, work, rs, finite, formed, sel, searches, us, zI, zQ,
                          d.io.rows + (int64_t)blockIdx.x * kFmmRow);
}

}  // namespace

int acf_fit_multi_launch(const AcfFmmDev& d, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int64_t total = d.io.win_base[d.io.n];
    if (total > 0) hipLaunchKernelGGL(acf_fit_multi_kernel, dim3((unsigned)total), dim3(kThreads), 0, stream, d);
    return (int)hipGetLastError();
}

}  // namespace gnss
