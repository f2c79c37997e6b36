// acf_fit.hip — the two-path fit of the 25-tap ACF on device-resident records (acf_fit.h;
// GNSS_OUT_DEVICE): a 32-channel x 91-s record set has about 29 000 windows of 7 776 two-path
// hypotheses each, over 1.16 GB of tap sums that already lie in HBM. One kernel, one block of
// kThreads lanes per (channel, window), two stages:
//   1. the coherent sums. A window's rows of one series (a tap's I or Q) are contiguous in time,
//      so tiles of kTile rows of all 50 series are staged into LDS with lanes along the rows (a
//      wave loads one series' 512-B run per step); then lanes 0..49 add one series each, left to
//      right, the sign from tap 12's I of the same row (one LDS address for all lanes: a
//      broadcast). The tile's row stride is odd, so the 50 lanes' reads fall on distinct banks.
//      The tile loop makes the LDS need independent of numOverLap.
//   2. the hypotheses. The 25 tap coordinates and the coherent vector stay in LDS and are read as
//      broadcasts. The one-path hypotheses, then the two-path ones, are dealt over the lanes
//      (lane t takes t, t + kThreads, ...); each lane keeps the lexicographic minimum of
//      (res, index) of its share, the block takes the minimum of those by shuffles within a wave
//      and through LDS across waves. The minimum of a total order does not depend on the order
//      it is taken in, so no float atomics are needed and two runs give the same bits. Lane 0
//      forms the winners' amplitudes again from their indices and stores the window's row.
// The arithmetic is acf_fit.h's, shared with the host path, without contraction (and no fast-math
// anywhere in the build): the outputs equal the host's bit for bit.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "acf.h"
#include "acf_fit.h"

namespace gnss {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSeries = 2 * kFitTaps;  // I then Q of every tap
constexpr int kTile = 64;              // rows per LDS tile: one wave's load of one series
constexpr int kStride = kTile + 1;     // doubles; odd: lanes along the series hit distinct banks

// the block's minimum of the lanes' (res, index), valid in lane 0 of the block; `wres` / `wh`
// hold one entry per wave and are free again on return
__device__ AcfFitBest block_best(AcfFitBest b, double* wres, int* wh)
{
    for (int off = 32; off; off >>= 1) {
        const double r = __shfl_xor(b.res, off);
        const int h = __shfl_xor(b.h, off);
        fit_best_merge(b, r, h);
    }
    if ((threadIdx.x & 63) == 0) {
        wres[threadIdx.x >> 6] = b.res;
        wh[threadIdx.x >> 6] = b.h;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int v = 1; v < kWaves; v++) fit_best_merge(b, wres[v], wh[v]);
    __syncthreads();
    return b;
}

// window blockIdx.x of all channels' windows in channel order; its rows lie below len[c] <=
// max_len (host check), so every load is inside channel c's series
__global__ __launch_bounds__(kThreads) void acf_fit_kernel(AcfFitDev d)
{
    __shared__ double tile[kSeries * kStride];
    __shared__ double zs[kSeries];  // zI[25] then zQ[25]
    __shared__ double us[kFitTaps];
    __shared__ double wres[kWaves];
    __shared__ int wh[kWaves];

    const int tid = threadIdx.x;
    const int64_t w = blockIdx.x;
    int c = 0;
    while (c + 1 < d.n && w >= d.win_base[c + 1]) c++;
    const int64_t m = w - d.win_base[c];
    const int64_t row = acf_window_row(m, d.ind_start, d.numOverLap);
    const double* base = d.taps + (int64_t)c * kSeries * d.max_len + row;
    const int N = (int)d.numOverLap;

    // stage 1
    double acc = 0;
    for (int t0 = 0; t0 < N; t0 += kTile) {
        const int nr = N - t0 < kTile ? N - t0 : kTile;
        for (int i = tid; i < kSeries * kTile; i += kThreads) {
            const int s = i / kTile, r = i % kTile;
            if (r < nr) tile[s * kStride + r] = base[(int64_t)s * d.max_len + t0 + r];
        }
        __syncthreads();
        if (tid < kSeries)
            for (int r = 0; r < nr; r++) {
                const double sg = fit_sign(tile[kFitPrompt * kStride + r]);
                acc = fit_accum(acc, sg, tile[tid * kStride + r], t0 + r == 0);
            }
        __syncthreads();
    }
    if (tid < kSeries) {
        zs[tid] = acc;
        if (d.z) d.z[w * kSeries + tid] = acc;
    }
    if (tid < kFitTaps) us[tid] = fit_u(d.grid, tid);
    __syncthreads();

    // stage 2
    const double* zI = zs;
    const double* zQ = zs + kFitTaps;
    AcfFitBest b1 = fit_best_none(), b2 = fit_best_none();
    if (fit_all_finite(zI, zQ)) {  // (uniform over the block)
        for (int ip = tid; ip < d.grid.p_count; ip += kThreads)
            fit_best_take(b1, fit_one(us, zI, zQ, fit_p(d.grid, ip)), ip);
        const int H = d.grid.p_count * d.grid.e_count;
#pragma unroll 1
        for (int h = tid; h < H; h += kThreads) fit_best_take(b2, fit_two_at(d.grid, us, zI, zQ, h), h);
    }
    b1 = block_best(b1, wres, wh);
    b2 = block_best(b2, wres, wh);
    if (tid == 0) {
        reinterpret_cast<AcfFitRow*>(d.rows)[w] = fit_select(d.grid, us, zI, zQ, b1.h, b2.h);
    }
}

}  // namespace

int acf_fit_launch(const AcfFitDev& d, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int64_t total = d.win_base[d.n];
    if (total > 0) hipLaunchKernelGGL(acf_fit_kernel, dim3((unsigned)total), dim3(kThreads), 0, stream, d);
    return (int)hipGetLastError();
}

}  // namespace gnss
