// acf_fit_taps_dev.h — what the kernels over [n][2][n_taps][max_rows] sums share (acf_fit_taps.hip,
// acf_fit_multi.hip): a block's tiled coherent sums of one window, the kernels' head around them
// and the block's minimum of the lanes' (res, index). Device code, included by .hip files only,
// each compiled without contraction.
#pragma once

#include <hip/hip_runtime.h>

#include "acf_fit_taps.h"

namespace gnss {
namespace fttdev {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 64;           // rows per LDS tile: one wave's load of one series
constexpr int kStride = kTile + 1;  // doubles; odd: lanes along the series hit distinct banks
constexpr int kGroup = 64;          // series per LDS tile: one wave adds them

// The coherent sums of the N rows from base[0] of 2 * nt series (a tap's I or Q, max_rows apart)
// into zs (zI[nt] then zQ[nt]); every lane of the block calls it, zs is complete for all on return.
// The window is tiled over rows (kTile) and over groups of kGroup series, so the LDS need is a
// constant whatever N and nt are. Per row tile the rows' signs come from the prompt's I once and
// serve every series group. A group's tile is staged with lanes along the rows (a wave loads one
// series' 512-B run per step); then lanes 0..kGroup-1 add one series each, rows ascending, reading
// LDS at the odd row stride kStride (distinct banks) and the signs as broadcasts. A series' running
// sum waits in zs between row tiles. tile: kGroup * kStride doubles, sg: kTile doubles of LDS.
__device__ inline void block_sums(const double* base, int64_t max_rows, int N, int nt, int prompt, double* tile,
                                  double* sg, double* zs)
{
    const int tid = threadIdx.x;
    const int S = 2 * nt;  // the series: I then Q of every tap
    for (int t0 = 0; t0 < N; t0 += kTile) {
        const int nr = N - t0 < kTile ? N - t0 : kTile;
        if (tid < nr) sg[tid] = ftt_sign(base[(int64_t)prompt * max_rows + t0 + tid]);
        for (int s0 = 0; s0 < S; s0 += kGroup) {
            const int ns = S - s0 < kGroup ? S - s0 : kGroup;
            for (int i = tid; i < ns * kTile; i += kThreads) {
                const int s = i / kTile, r = i % kTile;
                if (r < nr) tile[s * kStride + r] = base[(int64_t)(s0 + s) * max_rows + t0 + r];
            }
            __syncthreads();  // (the signs too, in the row tile's first group)
            if (tid < ns) {
                double acc = t0 ? zs[s0 + tid] : 0.0;
                for (int r = 0; r < nr; r++) acc = ftt_accum(acc, sg[r], tile[tid * kStride + r], t0 + r == 0);
                zs[s0 + tid] = acc;
            }
            __syncthreads();
        }
    }
}

// A kernel's head, called by every lane: block blockIdx.x takes that window of all channels'
// windows in channel order; its rows lie below n_rows[c] <= max_rows (host check), so every load
// is inside channel c's series. The window's coherent sums into zs (block_sums) and, if wanted,
// into d.z; the tap coordinates into us. us is complete for all after the caller's next barrier.
__device__ inline void block_window(const AcfFttIo& d, int nt, int prompt, double* tile, double* sg, double* zs,
                                    double* us)
{
    const int tid = threadIdx.x;
    const int64_t w = blockIdx.x;
    int c = 0;
    while (c + 1 < d.n && w >= d.win_base[c + 1]) c++;
    const int64_t row = ftt_window_row(w - d.win_base[c], d.ind_start, d.numOverLap);
    const int S = 2 * nt;  // the series: I then Q of every tap
    const double* base = d.taps + (int64_t)c * S * d.max_rows + row;
    block_sums(base, d.max_rows, (int)d.numOverLap, nt, prompt, tile, sg, zs);
    for (int s = tid; s < S; s += kThreads)
        if (d.z) d.z[w * S + s] = zs[s];
    for (int j = tid; j < nt; j += kThreads) us[j] = d.u[j];
}

// the wave's minimum of the lanes' (res, index) in every lane of the wave
__device__ inline AcfFttBest wave_best(AcfFttBest b)
{
    for (int off = 32; off; off >>= 1) {
        const double r = __shfl_xor(b.res, off);
        const int h = __shfl_xor(b.h, off);
        ftt_best_merge(b, r, h);
    }
    return b;
}

// the block's minimum of the lanes' (res, index), valid in lane 0 of the block; `wres` / `wh`
// hold one entry per wave and are free again on return
__device__ inline AcfFttBest block_best(AcfFttBest b, double* wres, int* wh)
{
    b = wave_best(b);
    if ((threadIdx.x & 63) == 0) {
        wres[threadIdx.x >> 6] = b.res;
        wh[threadIdx.x >> 6] = b.h;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int v = 1; v < kWaves; v++) ftt_best_merge(b, wres[v], wh[v]);
    __syncthreads();
    return b;
}

}  // namespace fttdev
}  // namespace gnss
