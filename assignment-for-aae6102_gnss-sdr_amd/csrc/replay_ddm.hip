// replay_ddm.hip — the delay-Doppler map over device-resident replayed sums (replay_ddm.h;
// GNSS_OUT_DEVICE), in the layout gnss_replay_correlate writes: [n][2][n_taps][max_rows]. Two
// kernels, no hand-off between blocks within either, no atomics, every loop bounded by values the
// host checked (replay_ddm.cpp):
//   1. ddm_map_kernel: one block of kDdmLanes lanes per (window, tile of kDdmBinTile bins, tile of
//      kDdmTapTile taps). A lane owns one tap and kDdmLaneBins bins, wave v the bins v*16..v*16+15
//      of the tile: 32 fp64 sums in registers. The window's rows go through LDS kDdmRowTile at a
//      time: the tile's taps' (I, Q) times the row's sign, read along the rows (the input's
//      contiguous axis) and stored transposed, [row][tap] with the tap index XORed by the row's low
//      four bits so that the stores of 16 rows and the loads of 64 taps both fall on distinct
//      banks without padding; and the tile's (sn, cs) per (row, bin), eight per lane, formed once
//      per row tile. Then a lane walks the rows in ascending order: its tap's pair from LDS, the 16
//      (sn, cs) pairs as broadcasts. 64 KB of LDS: two blocks per CU.
//   2. ddm_peak_kernel: one block per window over the stored map: the lanes' shares of the cells,
//      then the block's winner by shuffles within a wave and through LDS across waves. The rule is
//      a total order (the largest power, the lowest cell number among equals), so its maximum does
//      not depend on the order it is taken in. Twice: all cells, then those outside the box.
// The arithmetic is replay_ddm.h's, shared with the host path, without contraction: the outputs
// equal the host's bit for bit.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "replay_ddm.h"

namespace gnss {
namespace {

constexpr int kWaves = kDdmLanes / 64;
constexpr int kTile = kDdmRowTile * kDdmTapTile;  // doubles of one transposed tile (I or Q)
constexpr int kRot = kDdmRowTile * kDdmBinTile;   // (sn, cs) pairs of a row tile
static_assert(kDdmTapTile == 64, "a lane of a wave owns one tap of the tile");
static_assert(kWaves * kDdmLaneBins == kDdmBinTile, "a wave owns kDdmLaneBins bins of the tile");
static_assert(kDdmLanes % kDdmRowTile == 0 && kDdmLanes % kDdmBinTile == 0, "a lane keeps its row / its bin while staging");
static_assert(kDdmRowTile % 16 == 0 && kDdmTapTile % 16 == 0, "the swizzle permutes within 16 taps");
static_assert((2 * kTile + 2 * kRot) * sizeof(double) <= 65536, "LDS per block at most 64 KB");

// where tap `tap` of row `row` lies in a transposed tile
__device__ __forceinline__ int tile_at(int row, int tap)
{
    return row * kDdmTapTile + (tap ^ (row & 15));
}

__device__ __forceinline__ int channel_of(const DdmArgs& a, int64_t w)
{
    int c = 0;
    while (c + 1 < a.n && w >= a.win_base[c + 1]) c++;
    return c;
}

__device__ __forceinline__ int64_t slot_of(const DdmArgs& a, int c, int64_t w)
{
    return a.slot_cap > 0 ? (int64_t)c * a.slot_cap + (w - a.win_base[c]) : w;
}

// window blockIdx.x of all channels' windows in channel order; its rows lie below n_rows[c] <=
// max_rows (host check), so every load is inside channel c's series and time table
__global__ __launch_bounds__(kDdmLanes) void ddm_map_kernel(DdmArgs a)
{
    __shared__ double tI[kTile];
    __shared__ double tQ[kTile];
    __shared__ double2 rot[kRot];  // [row][bin] (sn, cs)

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t w = blockIdx.x;
    const int c = channel_of(a, w);
    const int64_t row0 = (w - a.win_base[c]) * a.R;
    const int nt = a.n_taps, nd = a.n_dopp, R = a.R;
    const int b0 = blockIdx.y * kDdmBinTile, j0 = blockIdx.z * kDdmTapTile;
    const int nb = nd - b0 < kDdmBinTile ? nd - b0 : kDdmBinTile;
    const int ntp = nt - j0 < kDdmTapTile ? nt - j0 : kDdmTapTile;
    const double* base = a.taps + (int64_t)c * 2 * nt * a.max_rows + row0;
    const double* tt = a.t + (int64_t)c * a.max_rows + row0;
    const bool mine = wave * kDdmLaneBins < nb && lane < ntp;  // (the first half is uniform over the wave)

    // what a lane stages: row srow of every eighth tap; bin sbin of every fourth row
    const int srow = tid % kDdmRowTile, stap0 = tid / kDdmRowTile;
    const int sbin = tid % kDdmBinTile, srot0 = tid / kDdmBinTile;
    const double nu = sbin < nb ? a.hz[b0 + sbin] : 0.0;

    double zi[kDdmLaneBins], zq[kDdmLaneBins];
#pragma unroll
    for (int q = 0; q < kDdmLaneBins; q++) zi[q] = zq[q] = 0.0;

    for (int r0 = 0; r0 < R; r0 += kDdmRowTile) {
        const int nr = R - r0 < kDdmRowTile ? R - r0 : kDdmRowTile;
        if (srow < nr) {
            const double s = a.prompt >= 0 ? ddm_sign(base[(int64_t)a.prompt * a.max_rows + r0 + srow]) : 1.0;
            for (int tap = stap0; tap < ntp; tap += kDdmLanes / kDdmRowTile) {
                const double I = base[(int64_t)(j0 + tap) * a.max_rows + r0 + srow];
                const double Q = base[(int64_t)(nt + j0 + tap) * a.max_rows + r0 + srow];
                tI[tile_at(srow, tap)] = s * I;
                tQ[tile_at(srow, tap)] = s * Q;
            }
        }
        for (int row = srot0; row < nr; row += kDdmLanes / kDdmBinTile) {
            double sn = 0.0, cs = 0.0;
            if (sbin < nb) ddm_rotation(nu, tt[r0 + row], &sn, &cs);
            rot[row * kDdmBinTile + sbin] = make_double2(sn, cs);
        }
        __syncthreads();
        if (mine) {
            const double2* rw = rot + wave * kDdmLaneBins;
            for (int i = 0; i < nr; i++) {
                const double sI = tI[tile_at(i, lane)], sQ = tQ[tile_at(i, lane)];
#pragma unroll
                for (int q = 0; q < kDdmLaneBins; q++) {
                    const double2 r = rw[i * kDdmBinTile + q];
                    ddm_cell(sI, sQ, r.x, r.y, &zi[q], &zq[q]);
                }
            }
        }
        __syncthreads();
    }
    if (mine) {
        const int64_t cells = (int64_t)nd * nt;
        double* out = a.map + slot_of(a, c, w) * 2 * cells + j0 + lane;
#pragma unroll
        for (int q = 0; q < kDdmLaneBins; q++) {
            const int m = b0 + wave * kDdmLaneBins + q;
            if (m < nd) {
                out[(int64_t)m * nt] = zi[q];
                out[cells + (int64_t)m * nt] = zq[q];
            }
        }
    }
}

// the block's winner of the lanes' shares, in every lane; wp / wk hold one entry per wave and are
// free again on return
__device__ DdmBest block_best(DdmBest b, double* wp, int* wk)
{
    for (int off = 32; off; off >>= 1) {
        const double p = __shfl_xor(b.pow, off);
        const int k = __shfl_xor(b.k, off);
        ddm_best_merge(b, p, k);
    }
    if ((threadIdx.x & 63) == 0) {
        wp[threadIdx.x >> 6] = b.pow;
        wk[threadIdx.x >> 6] = b.k;
    }
    __syncthreads();
    DdmBest r = ddm_best_none();
    for (int v = 0; v < kWaves; v++) ddm_best_merge(r, wp[v], wk[v]);
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(kDdmLanes) void ddm_peak_kernel(DdmArgs a)
{
    __shared__ double us[kDdmMaxTaps];
    __shared__ double hs[kDdmMaxDopp];
    __shared__ double wp[kWaves];
    __shared__ int wk[kWaves];

    const int tid = threadIdx.x;
    const int64_t w = blockIdx.x;
    const int c = channel_of(a, w);
    const int nt = a.n_taps, nd = a.n_dopp, cells = nd * nt;
    const double* zI = a.map + slot_of(a, c, w) * 2 * cells;
    const double* zQ = zI + cells;
    for (int j = tid; j < nt; j += kDdmLanes) us[j] = a.u[j];
    for (int m = tid; m < nd; m += kDdmLanes) hs[m] = a.hz[m];
    DdmBest p = ddm_best_none(), s = ddm_best_none();
    for (int k = tid; k < cells; k += kDdmLanes) ddm_best_take(p, ddm_power(zI[k], zQ[k]), k);
    p = block_best(p, wp, wk);  // (its barrier also covers us / hs)
    if (p.k >= 0) {             // (uniform over the block)
        const int pm = p.k / nt, pj = p.k % nt;
        for (int k = tid; k < cells; k += kDdmLanes)
            if (ddm_outside(us, hs, k / nt, k % nt, pm, pj, a.excl_chips, a.excl_hz))
                ddm_best_take(s, ddm_power(zI[k], zQ[k]), k);
    }
    s = block_best(s, wp, wk);
    if (tid == 0) a.peaks[w] = ddm_peaks_of(p, s, nt);
}

}  // namespace

int replay_ddm_launch(const DdmArgs& a, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int64_t total = a.win_base[a.n];
    if (total <= 0) return (int)hipSuccess;
    const dim3 grid((unsigned)total, (unsigned)((a.n_dopp + kDdmBinTile - 1) / kDdmBinTile),
                    (unsigned)((a.n_taps + kDdmTapTile - 1) / kDdmTapTile));
    hipLaunchKernelGGL(ddm_map_kernel, grid, dim3(kDdmLanes), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(ddm_peak_kernel, dim3((unsigned)total), dim3(kDdmLanes), 0, stream, a);
    return (int)hipGetLastError();
}

}  // namespace gnss
