// acf_fit_taps.hip — the two-path fit of an ACF on any tap grid over device-resident sums
// (acf_fit_taps.h; GNSS_OUT_DEVICE), in the layout gnss_replay_correlate writes:
// [n][2][n_taps][max_rows]. One kernel, one block of kThreads lanes per (channel, window), no
// hand-off between blocks, two stages:
//   1. the coherent sums. Up to 512 series (a tap's I or Q), each contiguous along the rows. The
//      window is tiled over rows (kTile) and over groups of kGroup series, so the LDS need is a
//      constant whatever numOverLap and n_taps are. Per row tile the rows' signs come from the
//      prompt's I once and serve every series group. A group's tile is staged with lanes along the
//      rows (a wave loads one series' 512-B run per step); then lanes 0..kGroup-1 add one series
//      each, rows ascending, reading LDS at the odd row stride kStride (distinct banks) and the
//      signs as broadcasts. A series' running sum waits in LDS (zs) between row tiles.
//   2. the hypotheses. The tap coordinates (us) and the coherent vector (zs) stay in LDS and are
//      read as broadcasts. The one-path hypotheses, then the two-path ones, are dealt over the
//      lanes (lane t takes t, t + kThreads, ...); each lane keeps the lexicographic minimum of
//      (res, index) of its share, the block takes the minimum of those by shuffles within a wave
//      and through LDS across waves: a total order's minimum does not depend on the order it is
//      taken in, so no float atomics are needed and two runs give the same bits. Lane 0 forms the
//      winners' amplitudes again from their indices and stores the window's row.
// Every sum runs over every tap: R = 0 outside a triangle is not exploited. Every loop is bounded
// by values the host checked (acf_fit_taps.cpp). The arithmetic is acf_fit_taps.h's, shared with
// the host path, without contraction: the outputs equal the host's bit for bit.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "acf_fit_taps.h"
#include "acf_fit_taps_dev.h"

namespace gnss {
namespace {

using namespace fttdev;  // stage 1 and the block's minimum, shared with acf_fit_multi.hip

// window blockIdx.x of all channels' windows in channel order (block_window)
__global__ __launch_bounds__(kThreads) void acf_fit_taps_kernel(AcfFttDev d)
{
    __shared__ double tile[kGroup * kStride];
    __shared__ double sg[kTile];             // the row tile's signs
    __shared__ double zs[2 * kFttMaxTaps];   // zI[n_taps] then zQ[n_taps]
    __shared__ double us[kFttMaxTaps];
    __shared__ double wres[kWaves];
    __shared__ int wh[kWaves];

    const int tid = threadIdx.x;
    const int nt = d.grid.n_taps;

    // stage 1
    block_window(d.io, nt, d.grid.prompt, tile, sg, zs, us);
    __syncthreads();

    // stage 2
    const double* zI = zs;
    const double* zQ = zs + nt;
    AcfFttBest b1 = ftt_best_none(), b2 = ftt_best_none();
    if (ftt_all_finite(nt, zI, zQ)) {  // (uniform over the block)
        for (int ip = tid; ip < d.grid.p_count; ip += kThreads)
            ftt_best_take(b1, ftt_one(nt, us, zI, zQ, ftt_p(d.grid, ip)), ip);
        const int H = d.grid.p_count * d.grid.e_count;
#pragma unroll 1
        for (int h = tid; h < H; h += kThreads) ftt_best_take(b2, ftt_two_at(d.grid, us, zI, zQ, h), h);
    }
    b1 = block_best(b1, wres, wh);
    b2 = block_best(b2, wres, wh);
    if (tid == 0) {
        reinterpret_cast<AcfFttRow*>(d.io.rows)[blockIdx.x] = ftt_select(d.grid, us, zI, zQ, b1.h, b2.h);
    }
}

}  // namespace

int acf_fit_taps_launch(const AcfFttDev& d, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int64_t total = d.io.win_base[d.io.n];
    if (total > 0) hipLaunchKernelGGL(acf_fit_taps_kernel, dim3((unsigned)total), dim3(kThreads), 0, stream, d);
    return (int)hipGetLastError();
}

}  // namespace gnss
