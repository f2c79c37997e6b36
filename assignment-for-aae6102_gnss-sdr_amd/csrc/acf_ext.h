// acf_ext.h — the features ACF/CalculateFeatures.m keeps behind comment marks, over the windows of
// gnss_acf_features (gnss_acf_features_ext; the definition, with the script's line cites, is in
// include/gnss_mi355x.h):
//   F6  numMLC   the mean number of interior local maxima of the 25 magnitudes per row (:243-257);
//   F7  fftFreq  and
//   F8  fftMag   the largest line of an N-point spectrum of the last fft_hist meanMax values of the
//                channel (:262-268), bins 0 .. N/2 as direct sums against one twiddle table.
// One source for the arithmetic (below), called in loops by the host path (acf_ext.cpp, and the
// row loop of acf.cpp) and by the kernels for GNSS_OUT_DEVICE records (acf.hip's row pass,
// acf_ext.hip), compiled without contraction and without fast-math on both sides: the two paths
// give the same bits. No HIP include and no project include: tests/native/acf_ext_host.cpp calls
// these functions on the CPU under AddressSanitizer and UBSan.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define GNSS_ACF_EXT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define GNSS_ACF_EXT_HD inline
#endif

namespace gnss {

constexpr int kExtMaxCh = 32;      // = GNSS_VT_MAX_CH
constexpr int kExtMaxHist = 512;   // fft_hist's bound
constexpr int kExtMaxN = 2048;     // fft_n's bound

// cnt(r) (:247-251) taken one column at a time, in column order: when column j arrives, column
// j - 1 is tested against its two neighbours. p1 and p2 start at +inf, against which no value
// compares greater, so columns 1 and 25 are never tested as a middle and never count; a NaN
// compares false on either side.
struct AcfMlc {
    double p2 = HUGE_VAL;  // corr(r, j - 2)
    double p1 = HUGE_VAL;  // corr(r, j - 1)
    int cnt = 0;
};
GNSS_ACF_EXT_HD void acf_mlc_take(AcfMlc& s, double v)
{
    if (s.p1 > s.p2 && s.p1 > v) s.cnt++;
    s.p2 = s.p1;
    s.p1 = v;
}

// H: the history's length at window m (0-based) of a channel (:262; fft_fill = 1: the windows
// that exist only)
GNSS_ACF_EXT_HD int acf_ext_len(int64_t m, int hist, int fill)
{
    return fill && m + 1 < hist ? (int)(m + 1) : hist;
}

// x[i], oldest first: meanMax(m - H + 1 + i) of the channel, 0 before its first window
GNSS_ACF_EXT_HD double acf_ext_hist(const double* meanMax, int64_t m, int H, int i)
{
    const int64_t w = m - H + 1 + i;
    return w < 0 ? 0.0 : meanMax[w];
}

// mean(x) (:263): one left-to-right sum, one division
GNSS_ACF_EXT_HD double acf_ext_mean(const double* x, int H)
{
    double s = x[0];
    for (int i = 1; i < H; i++) s = s + x[i];
    return s / (double)H;
}

// mag[k] (:264-265) as a direct sum: y the H values less their mean, tw the table as pairs
// (c[t], s[t]), t = 0 .. N - 1; t = (k * i) mod N by stepping (k <= N / 2 < N)
GNSS_ACF_EXT_HD double acf_ext_bin(const double* y, int H, const double* tw, int k, int N)
{
    double re = y[0] * tw[0], im = y[0] * tw[1];
    int t = k;
    for (int i = 1; i < H; i++) {
        const double a = y[i] * tw[2 * t], b = y[i] * tw[2 * t + 1];
        re = re + a;
        im = im + b;
        t += k;
        if (t >= N) t -= N;
    }
    const double rr = re * re, ii = im * im;
    return sqrt(rr + ii);
}

// [M, I] = max(mag) (:266) over the bins 0 .. N / 2: the larger magnitude, then the lower bin; a
// NaN counts as missing. The magnitudes are >= 0, so -1 stands for "none yet" (acf.h's AcfPeak).
// A scan in rising k needs `take` alone; `merge` joins two scans and is a total order on the pairs,
// so the result does not depend on how the bins were dealt out.
struct AcfExtBest {
    double mag = -1.0;
    int k = 0;
};
GNSS_ACF_EXT_HD void acf_ext_take(AcfExtBest& b, double v, int k)
{
    if (v > b.mag) {
        b.mag = v;
        b.k = k;
    }
}
GNSS_ACF_EXT_HD void acf_ext_merge(AcfExtBest& b, double mag, int k)
{
    if (mag > b.mag || (mag == b.mag && k < b.k)) {
        b.mag = mag;
        b.k = k;
    }
}

struct AcfExtRow {
    double numMLC, fftFreq, fftMag;
};

// The window's outputs: numMLC = sum(cnt) / numOverLap (:256), fftFreq = ((I - 1) * fs) / N
// (:267), fftMag = M / (N / 2) (:268, whatever H is). No bin taken: I = 1, M = NaN.
GNSS_ACF_EXT_HD AcfExtRow acf_ext_row(int64_t cnt_sum, int64_t numOverLap, AcfExtBest b, double fs, int N)
{
    const bool none = b.mag < 0;
    const double M = none ? (double)NAN : b.mag;
    const int I0 = none ? 0 : b.k;  // I - 1
    AcfExtRow r;
    r.numMLC = (double)cnt_sum / (double)numOverLap;
    r.fftFreq = ((double)I0 * fs) / (double)N;
    r.fftMag = M / ((double)N / 2);
    return r;
}

// The checked parameters of a call, the table both paths read and the caller's arrays
// ([n][cap] each, as gnss_acf_out's)
struct AcfExtPlan {
    int hist, N, fill;
    double fs;
    const double* tw;  // [N] pairs (c[t], s[t]) on the host
    double *numMLC, *fftFreq, *fftMag;
};

// What acf_spectrum_kernel takes (acf_ext.hip). Every extent was checked by the host: the rows
// of a channel's windows lie below len[c] <= max_len, 2 <= hist <= kExtMaxHist, hist <= N <=
// kExtMaxN.
struct AcfExtDev {
    const double* meanMax;  // [win_base[n]]: acf_window_kernel's, all channels' windows in channel order
    const uint8_t* cnt;     // [n][max_len]: the row pass's counts
    const double* tw;       // [N] pairs (c[t], s[t]) in device memory
    int64_t max_len;
    int n;
    int64_t win_base[kExtMaxCh + 1];
    int64_t ind_start, numOverLap;
    int hist, N, fill;
    double fs;
    double* out;  // [3][win_base[n]]: numMLC, fftFreq, fftMag
};

// The launch on `stream` (a hipStream_t) of the current device, after acf_launch's two on the
// same stream: one block per window. Returns the hipError_t of the launch (0: none).
int acf_spectrum_launch(const AcfExtDev& d, void* stream);

}  // namespace gnss
