// replay.hip — the replay correlator's kernel for gfx950 (gnss_replay_correlate; the arithmetic
// is replay.h's). One workgroup of 256 lanes per (row, channel, tile of kReplayTile = 32 taps):
// rows are independent of each other, so nothing here waits on another block -- no tickets, no
// spin waits, no persistent loop; every loop is bounded by the row's numSample, which the host
// has checked together with the row's read (inside the staged window) and every tap's colon.
//   - lane l takes samples k = l, l + 256, ... in ascending k: per sample the carrier wipe once
//     (~60 fp64 operations), per tap its colon element, the chip and two signed adds (~7);
//   - the 2 x 32 sums of a lane stay in registers (128 of the kernel's 256 VGPRs; the tile is as
//     wide as two waves per SIMD allow, so the wipe is paid once per 32 taps);
//   - the C/A code lies in LDS as a periodic byte table over the chips the tile's taps reach in
//     this row, so a tap-sample pays one LDS byte read and no integer modulus;
//     a launch with a (row, tile) of more than kReplayTabMax chips runs the modulus form instead
//     (kTab = false: the 32-word bit table of vt_mc.hip), the same chips and so the same bits;
//   - the block's sums: a fixed butterfly within each wave (xor 32, 16, ..., 1), then the four
//     wave sums in order, stored by wave 0. No float atomics: a row's bits depend on the row alone.
#include <hip/hip_runtime.h>

#include "replay.h"

namespace gnss {

namespace {

constexpr int kT = kReplayTile;
constexpr int kWaves = kReplayLanes / 64;

template <bool kTab>
__global__ __launch_bounds__(kReplayLanes, 2) void replay_kernel(ReplayArgs a)
{
    __shared__ unsigned s_ca[32];
    __shared__ double s_ac[2][kT], s_p[kT];
    __shared__ int s_lo[kT], s_hi[kT];
    __shared__ double s_w[kWaves][2 * kT];
    __shared__ uint8_t s_tab[kTab ? kReplayTabMax : 4];
    const int tid = threadIdx.x, ch = blockIdx.y, j0 = blockIdx.z * kT;
    const int64_t row = a.row0 + blockIdx.x;
    if (row >= a.n_rows[ch]) return;  // (the whole block)
    const int64_t at = (int64_t)ch * a.max_rows + row;
    RpRow r;
    r.n = a.ns[at];
    r.dtype = a.dtype;
    r.x = a.rec + (a.pos[at] - a.base);
    r.Fs = a.Fs;
    r.rfs = a.rfs;
    r.f = a.carrFreq[at];
    r.phi0 = a.remPhase[at];
    r.d = a.codeFreq[at] / a.Fs;
    const int nt = a.n_taps - j0 < kT ? a.n_taps - j0 : kT;
    if (tid < 32) s_ca[tid] = a.ca_bits[32 * ch + tid];
    if (tid >= 64 && tid < 64 + kT) {
        // tap j's colon ends (the host has checked the element count) and the chips it reaches
        const int j = tid - 64;
        double ta = 0.0, tc = 0.0, tp = 0.0;
        int lo = 0x7fffffff, hi = -0x7fffffff;
        if (j < nt) {
            const RpColon col = rp_tap_colon(a.taps[j0 + j], a.remChip[at], r.d, r.n);
            ta = col.a;
            tc = col.c;
            tp = a.post ? a.post[j0 + j] : 0.0;
            rp_chip_range(ta, tc, tp, &lo, &hi);
        }
        s_ac[0][j] = ta;
        s_ac[1][j] = tc;
        s_p[j] = tp;
        s_lo[j] = lo;
        s_hi[j] = hi;
    }
    __syncthreads();
    int base = 0;
    if (kTab) {
        int lo = s_lo[0], hi = s_hi[0];
        for (int j = 1; j < nt; j++) {
            lo = s_lo[j] < lo ? s_lo[j] : lo;
            hi = s_hi[j] > hi ? s_hi[j] : hi;
        }
        const int size = hi - lo + 1;
        if (size > kReplayTabMax) return;  // (the host launches this form only where every tile fits)
        base = lo;
        for (int i = tid; i < size; i += kReplayLanes) {
            const int c = rp_chip_index((int64_t)(base + i) + a.chip_off);
            s_tab[i] = (uint8_t)((s_ca[c >> 5] >> (c & 31)) & 1u);
        }
        __syncthreads();
    }
    const double* tp = a.post ? s_p : nullptr;
    double accI[kT], accQ[kT];
#pragma unroll
    for (int j = 0; j < kT; j++) accI[j] = accQ[j] = 0.0;
    if (kTab) {
        replay_lane(r, s_ac, tp, nt, tid, kReplayLanes, [&](int chip) { return s_tab[chip - base] != 0; }, accI,
                    accQ);
    } else {
        const int off = a.chip_off;
        replay_lane(r, s_ac, tp, nt, tid, kReplayLanes,
                    [&](int chip) {
                        const int c = rp_chip_index((int64_t)chip + off);
                        return ((s_ca[c >> 5] >> (c & 31)) & 1u) != 0;
                    },
                    accI, accQ);
    }
#pragma unroll
    for (int j = 0; j < kT; j++) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            accI[j] += __shfl_xor(accI[j], m);
            accQ[j] += __shfl_xor(accQ[j], m);
        }
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int j = 0; j < kT; j++) {
            s_w[tid >> 6][j] = accI[j];
            s_w[tid >> 6][kT + j] = accQ[j];
        }
    }
    __syncthreads();
    if (tid < 2 * kT) {
        const int j = tid < kT ? tid : tid - kT, iq = tid < kT ? 0 : 1;
        if (j < nt) {
            double v = s_w[0][tid];
#pragma unroll
            for (int w = 1; w < kWaves; w++) v += s_w[w][tid];
            a.out[(((int64_t)ch * 2 + iq) * a.n_taps + (j0 + j)) * a.max_rows + row] = v;
        }
    }
}

}  // namespace

int replay_launch(const ReplayArgs& a, int64_t rows, bool table, void* stream)
{
    if (rows < 1 || rows > 0x7fffffff || a.n_chan < 1 || a.n_chan > kReplayMaxChan || a.n_taps < 1 ||
        a.n_taps > kReplayMaxTaps || !a.rec || !a.out || !a.pos || !a.ns || !a.taps || !a.ca_bits)
        return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)rows, (unsigned)a.n_chan, (unsigned)((a.n_taps + kT - 1) / kT));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (table)
        hipLaunchKernelGGL(replay_kernel<true>, grid, dim3(kReplayLanes), 0, s, a);
    else
        hipLaunchKernelGGL(replay_kernel<false>, grid, dim3(kReplayLanes), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace gnss
