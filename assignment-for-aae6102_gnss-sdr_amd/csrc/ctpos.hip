// ctpos.hip — the measurement table of the positioning pass (ctpos.h) from device-resident
// tracking records (GNSS_OUT_DEVICE): a 32-channel x 90-s 25-tap record set is ~1.5 GB in HBM and
// the solver needs 4 values per channel and epoch, so only those cross PCIe. Three small kernels
// in stream order (no hand-off inside a launch):
//   1. ct_first_kernel   F[k][s] = the first step with absoluteSample > currMeasSample_k (binary
//                        search; trackingCT_POS_updated.m:427,442-446), one thread per (k, s);
//   2. ct_schedule_kernel  Index_k = max(max_s F[k][s], Index_{k-1} + 1) = k + prefixmax_{j<=k}
//                        (F_j - j) (:427-436: at most one epoch per tracking step), one block, a
//                        wave-level then LDS prefix-max over chunks of the block's width with a
//                        running carry; rows = the number of Index_k <= L;
//   3. ct_measure_kernel  per (k, s) of the first `rows` epochs: index (:447), codePhaseMeas
//                        (:450-453) and carrFreq(Index_k) (:514).
// codePhaseMeas needs a true IEEE fp64 division and a separately rounded multiply and add: no
// contraction in this file (and no fast-math anywhere in the build), the arithmetic is ctpos.h's,
// shared with the host extraction, so the two tables are equal bit for bit.
#pragma clang fp contract(off)

#include "ctpos.h"

namespace gnss {
namespace {

constexpr int kCtThreads = 256;
constexpr int kCtSchedThreads = 1024;  // 16 waves of 64

// hdr[0] rows, hdr[1] a record index outside its series (bound-check miss), hdr[2] index = 0
struct CtDev {
    const double* base;  // rec[n][GNSS_NFIELDS][max_len]
    int64_t max_len, L, K;
    int n;
    double start, step, Fs, dataType;
    int64_t* F;      // [K][n]: first-after (kernel 1), then `index` (kernel 3)
    int64_t* Index;  // [K]
    double* cpm;     // [K][n]
    double* cf;      // [K][n]
    long long* hdr;  // [4]
};

__device__ __forceinline__ const double* ct_series(const CtDev& d, int s, int f)
{
    return d.base + ((int64_t)s * GNSS_NFIELDS + f) * d.max_len;
}

__global__ __launch_bounds__(kCtThreads) void ct_first_kernel(CtDev d)
{
    const int64_t i = (int64_t)blockIdx.x * kCtThreads + threadIdx.x;
    if (i >= d.K * d.n) return;
    const int64_t k = i / d.n;
    const int s = (int)(i - k * d.n);
    // (the search reads a[mid] with 0 <= mid < L <= max_len only)
    d.F[i] = ct_first_after(ct_series(d, s, GNSS_F_absoluteSample), d.L, ct_curr_sample(d.start, d.step, k));
}

__global__ __launch_bounds__(kCtSchedThreads) void ct_schedule_kernel(CtDev d)
{
    __shared__ long long wave_max[kCtSchedThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr long long kNone = -(1LL << 62);
    long long carry = kNone, rows = 0;
    auto mx = [](long long a, long long b) { return a > b ? a : b; };
    for (int64_t k0 = 0; k0 < d.K; k0 += kCtSchedThreads) {
        const int64_t k = k0 + tid;
        long long v = kNone;
        if (k < d.K) {
            long long F = 0;
            for (int s = 0; s < d.n; s++) F = mx(F, (long long)d.F[k * d.n + s]);
            v = F - k;
        }
        for (int off = 1; off < 64; off <<= 1) {  // inclusive prefix-max within the wave
            const long long t = __shfl_up(v, off, 64);
            if (lane >= off) v = mx(v, t);
        }
        if (lane == 63) wave_max[wave] = v;
        __syncthreads();
        long long before = carry, all = carry;  // the earlier chunks and this chunk's earlier waves
        for (int w = 0; w < kCtSchedThreads / 64; w++) {
            if (w < wave) before = mx(before, wave_max[w]);
            all = mx(all, wave_max[w]);
        }
        if (k < d.K) {
            const long long Index = k + mx(v, before);
            d.Index[k] = Index;
            if (Index <= d.L) rows = mx(rows, (long long)(k + 1));  // (Index_k increases strictly)
        }
        carry = all;
        __syncthreads();  // (wave_max is rewritten by the next chunk)
    }
    for (int off = 32; off > 0; off >>= 1) rows = mx(rows, __shfl_xor(rows, off, 64));
    if (lane == 0) wave_max[wave] = rows;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kCtSchedThreads / 64; w++) rows = mx(rows, wave_max[w]);
        d.hdr[0] = rows;
    }
}

__global__ __launch_bounds__(kCtThreads) void ct_measure_kernel(CtDev d)
{
    const int64_t i = (int64_t)blockIdx.x * kCtThreads + threadIdx.x;
    const int64_t rows = d.hdr[0];
    if (i >= rows * d.n) return;
    const int64_t k = i / d.n;
    const int s = (int)(i - k * d.n);
    const int64_t index = d.F[i] - 1;  // :447
    const int64_t Index = d.Index[k];
    if (index < 1) {  // MATLAB raises at :450
        d.hdr[2] = 1;
        return;
    }
    if (index > d.L || Index < 1 || Index > d.L) {  // the bound check of every record index
        d.hdr[1] = 1;
        return;
    }
    const double curr = ct_curr_sample(d.start, d.step, k);
    d.cpm[i] = ct_code_phase(ct_series(d, s, GNSS_F_remChip)[index - 1], ct_series(d, s, GNSS_F_codeFreq)[index - 1],
                             ct_series(d, s, GNSS_F_absoluteSample)[index - 1], curr, d.Fs, d.dataType);
    d.cf[i] = ct_series(d, s, GNSS_F_carrFreq)[Index - 1];
    d.F[i] = index;
}

struct DevMem {  // hipFree on scope exit
    void* p = nullptr;
    ~DevMem()
    {
        if (p) (void)hipFree(p);
    }
};

}  // namespace

int ct_extract_device(const gnss_ct_pos_cfg& c, const CtRecords& r, int64_t cap, hipStream_t stream, CtTable* t,
                      std::string* err)
{
    auto hip_fail = [&](const char* what, hipError_t e) {
        *err = std::string("positioning (device extraction): ") + what + ": " + hipGetErrorString(e);
        return GNSS_EDEVICE;
    };
    t->n = r.n;
    t->rows = 0;
    // at most one epoch per step; one candidate beyond cap tells "more than cap" apart
    const int64_t K = std::min(cap + 1, r.L);
    if (K <= 0) return GNSS_OK;
    const size_t cells = (size_t)K * r.n;
    DevMem mF, mI, mC, mV, mH;
    hipError_t e;
    if ((e = hipMalloc(&mF.p, cells * 8)) || (e = hipMalloc(&mI.p, (size_t)K * 8)) ||
        (e = hipMalloc(&mC.p, cells * 8)) || (e = hipMalloc(&mV.p, cells * 8)) || (e = hipMalloc(&mH.p, 4 * 8)))
        return hip_fail("hipMalloc", e);
    CtDev d{r.base, r.max_len, r.L, K, r.n, ct_sample_start(c), ct_meas_step(c), c.Fs, (double)c.dataType,
            (int64_t*)mF.p, (int64_t*)mI.p, (double*)mC.p, (double*)mV.p, (long long*)mH.p};
    if ((e = hipMemsetAsync(d.hdr, 0, 4 * 8, stream))) return hip_fail("hipMemsetAsync", e);
    const unsigned blocks = (unsigned)((cells + kCtThreads - 1) / kCtThreads);
    hipLaunchKernelGGL(ct_first_kernel, dim3(blocks), dim3(kCtThreads), 0, stream, d);
    hipLaunchKernelGGL(ct_schedule_kernel, dim3(1), dim3(kCtSchedThreads), 0, stream, d);
    hipLaunchKernelGGL(ct_measure_kernel, dim3(blocks), dim3(kCtThreads), 0, stream, d);
    if ((e = hipGetLastError())) return hip_fail("kernel launch", e);
    long long hdr[4] = {};
    if ((e = hipMemcpyAsync(hdr, d.hdr, sizeof hdr, hipMemcpyDeviceToHost, stream)) ||
        (e = hipStreamSynchronize(stream)))
        return hip_fail("the table's header", e);
    if (hdr[1]) {
        *err = "positioning (device extraction): a record index fell outside its series (bound check)";
        return GNSS_EDEVICE;
    }
    const int64_t rows = hdr[0];
    if (rows < 0 || rows > K) {
        *err = "positioning (device extraction): the schedule's row count is out of range";
        return GNSS_EDEVICE;
    }
    if (rows > cap) {
        *err = "gnss_nav_sol_ct.cap is smaller than the epochs the records hold";
        return GNSS_EARG;
    }
    if (rows > 0 && hdr[2]) {
        *err = "positioning: index = 0 (the measurement sample lies at or before a channel's first record; "
               "MATLAB raises at trackingCT_POS_updated.m:450)";
        return GNSS_EINDEX;
    }
    if (rows == 0) return GNSS_OK;
    const size_t rc = (size_t)rows * r.n;
    t->Index.resize(rows);
    t->index.resize(rc);
    t->cpm.resize(rc);
    t->carrFreq.resize(rc);
    if ((e = hipMemcpyAsync(t->Index.data(), d.Index, (size_t)rows * 8, hipMemcpyDeviceToHost, stream)) ||
        (e = hipMemcpyAsync(t->index.data(), d.F, rc * 8, hipMemcpyDeviceToHost, stream)) ||
        (e = hipMemcpyAsync(t->cpm.data(), d.cpm, rc * 8, hipMemcpyDeviceToHost, stream)) ||
        (e = hipMemcpyAsync(t->carrFreq.data(), d.cf, rc * 8, hipMemcpyDeviceToHost, stream)) ||
        (e = hipStreamSynchronize(stream)))
        return hip_fail("the table's download", e);
    t->rows = rows;
    return GNSS_OK;
}

}  // namespace gnss
