// acf.hip — ACF/CalculateFeatures.m on device-resident 25-tap records (acf.h; GNSS_OUT_DEVICE):
// a 32-channel x 91-s record set holds 1.16 GB of tap sums in HBM and the script reduces them to
// 5 numbers per 100-ms window, so one streaming pass reads them where they lie and only the
// features cross PCIe. Two kernels in stream order (no atomics, no hand-off inside a launch):
//   1. acf_row_kernel     lanes along time, grid.y = channel. Each of a channel's 50 series is
//                         contiguous in time, so a wave's load of one series is one contiguous
//                         run (512 B, or 1 KiB with two rows per lane as 16-B loads where max_len
//                         and the base pointers allow). A lane loads kGroup taps' I and Q before
//                         the first use, forms the magnitudes and carries the first-index
//                         arg-max; it writes the prompt magnitude (8 B) and the index (1 B) per
//                         row and, if asked for, the 25 magnitudes. Every tap value is read from
//                         HBM exactly once. For gnss_acf_features_ext the same pass also counts
//                         the row's interior local maxima (acf_ext.h) into one more byte.
//   2. acf_window_kernel  one lane per window over those compact per-row values and the code
//                         discriminator's series, summing left to right as the host does.
// The arithmetic is acf.h's, shared with the host path, without contraction (and no fast-math
// anywhere in the build): the outputs equal the host's bit for bit.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "acf.h"
#include "acf_ext.h"

namespace gnss {
namespace {

constexpr int kRowThreads = 256;
constexpr int kWinThreads = 64;
constexpr int kGroup = 5;  // taps whose I and Q loads are in flight per lane (25 = 5 groups)

typedef double double2_t __attribute__((ext_vector_type(2)));

template <int VEC> struct RowVec;
template <> struct RowVec<1> {
    using type = double;
    static __device__ __forceinline__ double at(double v, int) { return v; }
};
template <> struct RowVec<2> {
    using type = double2_t;
    static __device__ __forceinline__ double at(double2_t v, int e) { return e ? v.y : v.x; }
};

// rows [i, i + VEC) of channel blockIdx.y, i < len (the host checked len <= max_len; with VEC = 2
// max_len is even and i is even, so row i + 1 < max_len is inside every series even when it is
// past len: it is loaded, never stored). MLC (gnss_acf_features_ext): the lane also carries
// acf_ext.h's local-maximum counter, two magnitudes per row across the groups, and writes one
// more byte per row; without it the kernel is the one gnss_acf_features always had.
template <int VEC, bool CORR, bool MLC>
__global__ __launch_bounds__(kRowThreads) void acf_row_kernel(AcfDev d)
{
    using V = typename RowVec<VEC>::type;
    const int c = blockIdx.y;
    const int64_t len = d.len[c];
    const int64_t i = ((int64_t)blockIdx.x * kRowThreads + threadIdx.x) * VEC;
    if (i >= len) return;
    const double* base = d.taps + (int64_t)c * 2 * kAcfTaps * d.max_len + i;
    const int64_t q_off = (int64_t)kAcfTaps * d.max_len;
    AcfPeak peak[VEC];
    double prompt[VEC] = {};
    AcfMlc mlc[VEC];
    // (the group loop stays rolled: unrolled, the compiler hoists all 50 loads to the top, 200
    // VGPRs at two rows per lane, and spills under any occupancy bound)
#pragma unroll 1
    for (int g = 0; g < kAcfTaps / kGroup; g++) {
        V I[kGroup], Q[kGroup];
#pragma unroll
        for (int k = 0; k < kGroup; k++) {
            const double* p = base + (int64_t)(g * kGroup + k) * d.max_len;
            I[k] = *reinterpret_cast<const V*>(p);
            Q[k] = *reinterpret_cast<const V*>(p + q_off);
        }
#pragma unroll
        for (int k = 0; k < kGroup; k++) {
            const int j = g * kGroup + k;
            double m[VEC];
#pragma unroll
            for (int e = 0; e < VEC; e++) {
                m[e] = acf_mag(RowVec<VEC>::at(I[k], e), RowVec<VEC>::at(Q[k], e));
                acf_peak_take(peak[e], m[e], j + 1);
                if (j == kAcfPrompt) prompt[e] = m[e];
                if (MLC) acf_mlc_take(mlc[e], m[e]);
            }
            if (CORR) {
                double* o = d.corr + ((int64_t)c * kAcfTaps + j) * d.max_len + i;
                if (VEC == 2 && i + 1 < len) {
                    double2_t v;
                    v.x = m[0];
                    v.y = m[VEC - 1];
                    *reinterpret_cast<double2_t*>(o) = v;
                } else {
                    o[0] = m[0];
                }
            }
        }
    }
    const int64_t r = (int64_t)c * d.max_len + i;
    if (VEC == 2 && i + 1 < len) {
        double2_t v;
        v.x = prompt[0];
        v.y = prompt[VEC - 1];
        *reinterpret_cast<double2_t*>(d.pm + r) = v;
        d.idx[r] = (uint8_t)peak[0].idx;
        d.idx[r + 1] = (uint8_t)peak[VEC - 1].idx;
        if (MLC) {
            d.cnt[r] = (uint8_t)mlc[0].cnt;
            d.cnt[r + 1] = (uint8_t)mlc[VEC - 1].cnt;
        }
    } else {
        d.pm[r] = prompt[0];
        d.idx[r] = (uint8_t)peak[0].idx;
        if (MLC) d.cnt[r] = (uint8_t)mlc[0].cnt;
    }
}

template <int VEC, bool CORR>
void launch_rows(const AcfDev& d, dim3 grid, hipStream_t stream)
{
    if (d.cnt)
        hipLaunchKernelGGL((acf_row_kernel<VEC, CORR, true>), grid, dim3(kRowThreads), 0, stream, d);
    else
        hipLaunchKernelGGL((acf_row_kernel<VEC, CORR, false>), grid, dim3(kRowThreads), 0, stream, d);
}

// window w of all channels' windows in channel order; its rows lie below len[c] (host check)
__global__ __launch_bounds__(kWinThreads) void acf_window_kernel(AcfDev d)
{
    const int64_t total = d.win_base[d.n];
    const int64_t w = (int64_t)blockIdx.x * kWinThreads + threadIdx.x;
    if (w >= total) return;
    int c = 0;
    while (c + 1 < d.n && w >= d.win_base[c + 1]) c++;
    const int64_t m = w - d.win_base[c];
    const int64_t row = acf_window_row(m, d.ind_start, d.numOverLap);
    const int64_t r = (int64_t)c * d.max_len + row;
    const double* disc = d.rec + ((int64_t)c * d.nfields + d.field_d) * d.max_len + row;
    const AcfWindow f = acf_window(d.pm + r, d.idx + r, disc, d.numOverLap, m == 0, d.corrSpacing, d.cenDelay);
    d.feat[0 * total + w] = f.meanMax;
    d.feat[1 * total + w] = f.meanDelay;
    d.feat[2 * total + w] = f.varDelay;
    d.feat[3 * total + w] = f.meanCodeDisc;
    d.feat[4 * total + w] = f.varCodeDisc;
}

}  // namespace

int acf_launch(const AcfDev& d, bool vec2, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int64_t rows = 0;
    for (int c = 0; c < d.n; c++) rows = d.len[c] > rows ? d.len[c] : rows;
    if (rows > 0) {
        const int per_block = kRowThreads * (vec2 ? 2 : 1);
        const dim3 grid((unsigned)((rows + per_block - 1) / per_block), (unsigned)d.n);
        if (vec2 && d.corr)
            launch_rows<2, true>(d, grid, stream);
        else if (vec2)
            launch_rows<2, false>(d, grid, stream);
        else if (d.corr)
            launch_rows<1, true>(d, grid, stream);
        else
            launch_rows<1, false>(d, grid, stream);
    }
    const int64_t total = d.win_base[d.n];
    if (total > 0)
        hipLaunchKernelGGL(acf_window_kernel, dim3((unsigned)((total + kWinThreads - 1) / kWinThreads)),
                           dim3(kWinThreads), 0, stream, d);
    return (int)hipGetLastError();
}

}  // namespace gnss
