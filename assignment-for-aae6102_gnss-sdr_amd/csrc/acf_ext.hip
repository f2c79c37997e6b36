// acf_ext.hip — F6-F8 of ACF/CalculateFeatures.m on device-resident 25-tap records (acf_ext.h;
// gnss_acf_features_ext with GNSS_OUT_DEVICE). The per-row counts of interior local maxima come
// from acf.hip's row pass (its MLC form), the windows' meanMax from acf_window_kernel; this file
// holds the third launch of the stream, acf_spectrum_kernel: one block of kThreads lanes per
// (channel, window), three stages:
//   0. the lanes add the window's count bytes (integers: any order is exact), the block adds the
//      lanes' sums by shuffles within a wave and through LDS across waves;
//   1. the channel's last H meanMax values go to LDS, every lane forms their mean by the same
//      left-to-right sum (broadcast reads), the lanes subtract it in place; the twiddle table goes
//      to LDS as (cos, sin) pairs, N of them (32 KB at the bound);
//   2. the bins 0 .. N / 2 are dealt over the lanes (lane t takes t, t + kThreads, ...); the inner
//      loop runs over the history with y[i] read as a broadcast and the twiddle index stepped by
//      k modulo N; each lane keeps the best (mag, k) of its share, the block takes the best of
//      those: the larger mag, then the lower k. That is a total order, so no float atomics are
//      needed and two runs give the same bits. Lane 0 stores the window's three outputs.
// All LDS is dynamic, 2 N + fft_hist doubles and the waves' hand-over (18.8 KB at the defaults),
// the table first so that its pairs stay 16-B aligned whatever H is. The arithmetic
// is acf_ext.h's, shared with the host path, without contraction (and no fast-math anywhere in
// the build): the outputs equal the host's bit for bit.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "acf.h"
#include "acf_ext.h"

namespace gnss {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

// window blockIdx.x of all channels' windows in channel order; its rows lie below len[c] <=
// max_len and its history inside the channel's windows (host checks)
__global__ __launch_bounds__(kThreads) void acf_spectrum_kernel(AcfExtDev d)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];  // (the launch sizes it: lds_bytes)

    const int tid = threadIdx.x;
    const int64_t w = blockIdx.x, total = d.win_base[d.n];
    int c = 0;
    while (c + 1 < d.n && w >= d.win_base[c + 1]) c++;
    const int64_t m = w - d.win_base[c];
    const int H = acf_ext_len(m, d.hist, d.fill), N = d.N;
    double* tw = static_cast<double*>(__builtin_assume_aligned(lds, 16));  // [N] pairs
    double* y = lds + 2 * N;                                             // [hist], H of them used
    double* wmag = y + d.hist;                                           // one entry per wave, as wk and wsum
    int* wk = reinterpret_cast<int*>(wmag + kWaves);
    int* wsum = wk + kWaves;

    // stage 0
    const uint8_t* cnt = d.cnt + (int64_t)c * d.max_len + acf_window_row(m, d.ind_start, d.numOverLap);
    int sum = 0;
    for (int i = tid; i < (int)d.numOverLap; i += kThreads) sum += cnt[i];
    for (int off = 32; off; off >>= 1) sum += __shfl_xor(sum, off);
    if ((tid & 63) == 0) wsum[tid >> 6] = sum;

    // stage 1
    const double* mm = d.meanMax + d.win_base[c];
    for (int i = tid; i < H; i += kThreads) y[i] = acf_ext_hist(mm, m, H, i);
    for (int i = tid; i < 2 * N; i += kThreads) tw[i] = d.tw[i];
    __syncthreads();
    const double mean = acf_ext_mean(y, H);
    __syncthreads();
    for (int i = tid; i < H; i += kThreads) y[i] = y[i] - mean;
    __syncthreads();

    // stage 2
    AcfExtBest b;
#pragma unroll 1
    for (int k = tid; k <= N / 2; k += kThreads) acf_ext_take(b, acf_ext_bin(y, H, tw, k, N), k);
    for (int off = 32; off; off >>= 1) {
        const double mg = __shfl_xor(b.mag, off);
        const int k = __shfl_xor(b.k, off);
        acf_ext_merge(b, mg, k);
    }
    if ((tid & 63) == 0) {
        wmag[tid >> 6] = b.mag;
        wk[tid >> 6] = b.k;
    }
    __syncthreads();
    if (tid == 0) {
        int64_t s = wsum[0];
        for (int v = 1; v < kWaves; v++) {
            acf_ext_merge(b, wmag[v], wk[v]);
            s += wsum[v];
        }
        const AcfExtRow r = acf_ext_row(s, d.numOverLap, b, d.fs, N);
        d.out[0 * total + w] = r.numMLC;
        d.out[1 * total + w] = r.fftFreq;
        d.out[2 * total + w] = r.fftMag;
    }
}

size_t lds_bytes(const AcfExtDev& d)
{
    return (size_t)(2 * d.N + d.hist + kWaves) * sizeof(double) + 2 * kWaves * sizeof(int);
}

}  // namespace

int acf_spectrum_launch(const AcfExtDev& d, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int64_t total = d.win_base[d.n];
    if (total > 0)
        hipLaunchKernelGGL(acf_spectrum_kernel, dim3((unsigned)total), dim3(kThreads), lds_bytes(d), stream, d);
    return (int)hipGetLastError();
}

}  // namespace gnss
