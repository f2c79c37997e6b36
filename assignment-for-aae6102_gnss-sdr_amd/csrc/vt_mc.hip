// vt_mc.hip — the correlator of the 25-tap vector-tracking step for gfx950
// (trackingVT_POS_updated_multicorrelator.m:230-350). Unlike the plain loop (vt.hip), whose
// linear-indexing quirk turns E / P / L into one chip times sum(InphaseSignal), this loop
// despreads every sample against 25 real replicas: per sample the carrier wipe of
// vt_block_sums (the reference's own Wave(k) rounding, IEEE k/Fs, sincos_small of the
// 2*pi-reduced phase), per tap Code(ceil(t_k) + 2) with t_k MATLAB's colon element, and 50 sums
// sum(Code_j .* InphaseSignal), sum(Code_j .* QuadratureSignal).
// The grid and the hand-off are vt_step_kernel's: nb x n blocks of 256 lanes, block b of channel
// ch over a contiguous slice of the read, a fixed-order block reduction, the block's partials
// through device-coherent stores drained before a ticket, and the grid's last block adds each
// channel's partials in block order and writes the 50 sums and the step's number to the
// caller's coherent host memory. No float atomics: the same bits from run to run.
// The straight form (every sample of every tap looked up) is kept: ~12 fp64 operations per tap
// and sample, 7.3 M tap-samples per 5-channel step, far below what binds a step.
#include "vt_mc.h"

namespace gnss {

namespace {

__device__ __forceinline__ int16_t ld_i16(const uint8_t* p)
{
    return (int16_t)((unsigned)p[0] | ((unsigned)p[1] << 8));
}

__global__ __launch_bounds__(kVtStepThreads) void vt_mc_step_kernel(VtMcStepArgs a)
{
    __shared__ unsigned s_ca[32];
    __shared__ double s_a[kVtMcTaps], s_c[kVtMcTaps];
    __shared__ double s_w[kVtStepThreads / 64][kVtMcSums];
    __shared__ int s_last;
    // (the last block's tile of partials: kTile blocks x 50 words, kTileLoads words per lane)
    constexpr int kTile = 32, kTileLoads = (kTile * kVtMcSums + kVtStepThreads - 1) / kVtStepThreads;
    __shared__ double s_p[kTile * kVtMcSums];
    const int b = blockIdx.x, ch = blockIdx.y, nb = gridDim.x, nch = gridDim.y, tid = threadIdx.x;
    const int64_t n = a.ns[ch];
    const int64_t chunk = (n + nb - 1) / nb;
    const int64_t k0 = (int64_t)b * chunk, k1 = k0 + chunk < n ? k0 + chunk : n;
    const uint8_t* r = a.rec + a.off[ch];
    const double Fs = a.Fs, f = a.f[ch], phi0 = a.phi0[ch], rfs = a.rfs[ch], d = a.cps[ch];
    const int fmt = a.fmt;
    if (tid < 32) s_ca[tid] = a.ca_bits[32 * ch + tid];
    if (tid >= 64 && tid < 64 + kVtMcTaps && n > 0) {
        // tap j's colon ends (vt_mc_prepare's arithmetic; the host has checked its element count)
        const int j = tid - 64;
        const double spc = vt_mc_spacing(j), rc = a.remChip[ch];
        const double ta = (0 + spc) + rc;
        s_a[j] = ta;
        s_c[j] = colon_make(ta, d, ((double)(n - 1) * d + spc) + rc).c;
    }
    // int16: rawsignal = (I - mean(I)) + 1i*(Q - mean(Q)) over this read (:157-162); the integer
    // sums are exact, the mean one fp64 division as MATLAB's mean
    double mu_i = 0.0, mu_q = 0.0;
    if (fmt == 2 && n > 0) {
        mu_i = (double)a.isum[2 * ch] / (double)n;
        mu_q = (double)a.isum[2 * ch + 1] / (double)n;
    }
    __syncthreads();
    double accI[kVtMcTaps], accQ[kVtMcTaps];
#pragma unroll
    for (int j = 0; j < kVtMcTaps; j++) accI[j] = accQ[j] = 0.0;
    const int64_t nn = n - 1;  // the colons' interval count
    for (int64_t k = k0 + tid; k < k1; k += kVtStepThreads) {
        // the sample's carrier-wiped pair: vt_block_sums' term (vt.hip), operation for operation
        const double t = rfs != 0.0 ? div_markstein((double)k, Fs, rfs) : (double)k / Fs;
        const double W = kTwoPi * (f * t) + phi0;  // Wave(k+1) (:285-286)
        const double q = rint(W * (1.0 / kTwoPi));
        double rr = __builtin_fma(-q, kTwoPi, W);
        rr = __builtin_fma(-q, kTwoPiLo, rr);
        double sn, cs;
        sincos_small(rr, &sn, &cs);
        double xr, xi;
        if (fmt == 2) {
            xr = (double)ld_i16(r + 4 * k) - mu_i;
            xi = (double)ld_i16(r + 4 * k + 2) - mu_q;
        } else if (fmt == 1) {
            xr = (double)(int8_t)r[k];
            xi = 0.0;
        } else {
            xr = (double)(int8_t)r[2 * k];
            xi = (double)(int8_t)r[2 * k + 1];
        }
        const double tI = xr * sn + xi * cs;  // imag(raw .* carrsig) (:290)
        const double tQ = xr * cs - xi * sn;  // real(raw .* carrsig) (:291)
        // MATLAB's colon element k of every tap (colon_elem: the lower half counts up from a, the
        // upper half down from c, the middle element is their mean), its chip, the two products
        const bool mid = 2 * k == nn, low = k <= nn / 2;
        const double kd = (double)k * d, rd = (double)(nn - k) * d;
#pragma unroll
        for (int j = 0; j < kVtMcTaps; j++) {
            const double ta = s_a[j], tc = s_c[j];
            const double tk = mid ? (ta + tc) / 2 : (low ? ta + kd : tc - rd);
            const unsigned i = vt_mc_chip((int)ceil(tk));
            const bool neg = (s_ca[i >> 5] >> (i & 31)) & 1u;
            accI[j] += neg ? -tI : tI;
            accQ[j] += neg ? -tQ : tQ;
        }
    }
    // the block's 50 sums: a fixed butterfly within each wave (xor 32, 16, ..., 1), then the four
    // wave sums in order -- the same bits for the same terms
#pragma unroll
    for (int j = 0; j < kVtMcTaps; j++) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            accI[j] += __shfl_xor(accI[j], m);
            accQ[j] += __shfl_xor(accQ[j], m);
        }
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int j = 0; j < kVtMcTaps; j++) {
            s_w[tid >> 6][j] = accI[j];
            s_w[tid >> 6][kVtMcTaps + j] = accQ[j];
        }
    }
    __syncthreads();
    if (tid < 64) {
        // wave 0 alone stores the block's partials (lane v: sum v), device-coherent (past this
        // XCD's L2) and drained before its lane 0 takes the block's ticket: the grid's last block
        // reads them with device-coherent loads (vt_step_block's form)
        if (tid < kVtMcSums) {
            double v = s_w[0][tid];
#pragma unroll
            for (int w = 1; w < kVtStepThreads / 64; w++) v += s_w[w][tid];
            __hip_atomic_store(a.part + ((int64_t)ch * nb + b) * kVtMcSums + tid, v, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (tid == 0) {
            const unsigned total = (unsigned)nb * nch;
            s_last = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == total - 1;
        }
    }
    __syncthreads();
    if (!s_last) return;
    // the grid's last block: a channel's nb x 50 partials come into LDS kTile blocks at a time
    // (lane k loads words k, k + 256, ..., all in flight together), lane v < 50 adds sum v over the
    // tile's blocks in block order (the same sequential sum for every nb) and writes it through to
    // the caller's host memory, and once every lane's are drained, lane 0 re-arms the ticket
    // (drained too: a later step's first ticket must see it) and posts the step's number
    for (int c = 0; c < nch; c++) {
        double sum = 0.0;
        for (int b0 = 0; b0 < nb; b0 += kTile) {
            const int m = nb - b0 < kTile ? nb - b0 : kTile, cnt = m * kVtMcSums;
            const double* pp = a.part + ((int64_t)c * nb + b0) * kVtMcSums;
            double t[kTileLoads];
#pragma unroll
            for (int u = 0; u < kTileLoads; u++) {  // (a word past the tile: the tile's first again, not kept)
                const int e = tid + u * kVtStepThreads;
                t[u] = __hip_atomic_load(pp + (e < cnt ? e : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __syncthreads();  // (the last tile's adds are done before its words are replaced)
#pragma unroll
            for (int u = 0; u < kTileLoads; u++) {
                const int e = tid + u * kVtStepThreads;
                if (e < cnt) s_p[e] = t[u];
            }
            __syncthreads();
            if (tid < kVtMcSums)
                for (int u = 0; u < m; u++) sum += s_p[u * kVtMcSums + tid];
        }
        if (tid < kVtMcSums)
            __hip_atomic_store(a.sums + c * kVtMcSums + tid, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(a.done, a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// int16 records: each channel's exact integer sums of I and Q over its read, for the means
struct VtMcIsumArgs {
    const uint8_t* rec;
    long long* isum;
    int64_t off[GNSS_VT_MAX_CH], ns[GNSS_VT_MAX_CH];
};
__global__ __launch_bounds__(kVtStepThreads) void vt_mc_isum_kernel(VtMcIsumArgs a)
{
    const int ch = blockIdx.y, tid = threadIdx.x;
    const int64_t n = a.ns[ch];
    const uint8_t* r = a.rec + a.off[ch];
    long long si = 0, sq = 0;
    for (int64_t k = (int64_t)blockIdx.x * kVtStepThreads + tid; k < n; k += (int64_t)gridDim.x * kVtStepThreads) {
        si += ld_i16(r + 4 * k);
        sq += ld_i16(r + 4 * k + 2);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        si += __shfl_xor(si, m);
        sq += __shfl_xor(sq, m);
    }
    if ((tid & 63) == 0 && n > 0) {  // (two's complement: the unsigned add is the signed one)
        atomicAdd(reinterpret_cast<unsigned long long*>(a.isum + 2 * ch), (unsigned long long)si);
        atomicAdd(reinterpret_cast<unsigned long long*>(a.isum + 2 * ch + 1), (unsigned long long)sq);
    }
}

}  // namespace

hipError_t launch_vt_mc_step(const VtMcStepArgs& a, int n, int nb, hipStream_t s)
{
    if (n < 1 || n > GNSS_VT_MAX_CH || nb < 1 || nb > GNSS_VT_MAX_BLOCKS || !a.rec || !a.ca_bits || !a.part || !a.sums ||
        !a.done || !a.ticket || a.fmt < 0 || a.fmt > 2 || (a.fmt == 2 && !a.isum))
        return hipErrorInvalidValue;
    for (int i = 0; i < n; i++)
        if (a.ns[i] < 0 || a.off[i] < 0 || (a.ns[i] > 0 && !(a.cps[i] > 0))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vt_mc_step_kernel, dim3(nb, n), dim3(kVtStepThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_vt_mc_isum(const uint8_t* rec, const int64_t* off, const int64_t* ns, int n, long long* isum,
                             hipStream_t s)
{
    if (n < 1 || n > GNSS_VT_MAX_CH || !rec || !isum) return hipErrorInvalidValue;
    VtMcIsumArgs a{};
    a.rec = rec;
    a.isum = isum;
    int64_t most = 0;
    for (int i = 0; i < n; i++) {
        if (ns[i] < 0 || off[i] < 0) return hipErrorInvalidValue;
        a.off[i] = off[i];
        a.ns[i] = ns[i];
        most = ns[i] > most ? ns[i] : most;
    }
    const int nb = (int)((most + 8 * kVtStepThreads - 1) / (8 * kVtStepThreads));
    hipLaunchKernelGGL(vt_mc_isum_kernel, dim3(nb < 1 ? 1 : (nb > 256 ? 256 : nb), n), dim3(kVtStepThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace gnss
