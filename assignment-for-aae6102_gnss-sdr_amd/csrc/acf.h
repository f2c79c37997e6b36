// acf.h — ACF/CalculateFeatures.m as a pass over the 25-tap records (gnss_acf_features; the
// definition, with the script's line cites, is in include/gnss_mi355x.h). Two stages:
//   1. the row pass: per record row the 25 magnitudes sqrt(I*I + Q*Q), of them the prompt
//      magnitude and the first-index arg-max (:197-225, :236-237);
//   2. the window sums: per window of numOverLap rows meanMax, meanDelay, varDelay, meanCodeDisc
//      and varCodeDisc (:238-274), every sum left to right.
// One source for the arithmetic of both stages (below), called in loops by the host path (acf.cpp)
// and by the kernels for GNSS_OUT_DEVICE records (acf.hip), compiled without contraction and
// without fast-math on both sides: the two paths give the same bits. No HIP include and no
// project include: tests/native/acf_host.cpp calls these functions on the CPU under
// AddressSanitizer and UBSan.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define GNSS_ACF_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define GNSS_ACF_HD inline
#endif

namespace gnss {

constexpr int kAcfTaps = 25;    // = GNSS_MC_TAPS
constexpr int kAcfPrompt = 12;  // corr(r, 13), 0-based (:237)
constexpr int kAcfMaxCh = 32;   // = GNSS_VT_MAX_CH

// corr(i, j) (:199-223): the squares, the add and a correctly rounded square root
GNSS_ACF_HD double acf_mag(double I, double Q)
{
    const double ii = I * I, qq = Q * Q;
    return sqrt(ii + qq);
}

// [~, maxCorrInd] = max(corr(r, :)) (:236) taken one column at a time: the first index of the
// largest value, NaN as missing (a comparison with NaN is false), 1 for an all-NaN row. The
// magnitudes are >= 0, so -1 stands for "none yet".
struct AcfPeak {
    double best = -1.0;
    int idx = 1;
};
GNSS_ACF_HD void acf_peak_take(AcfPeak& p, double v, int j1)  // j1: the 1-based column
{
    if (v > p.best) {
        p.best = v;
        p.idx = j1;
    }
}

// cenDelay = maxDelay / corrSpacing + 1 (:176), 12.999999999999998 for 0.6 and 0.05
GNSS_ACF_HD double acf_cen_delay(double maxDelay, double corrSpacing)
{
    return maxDelay / corrSpacing + 1;
}

// windows of a channel with L rows (:234): floor((L - ind_start) / numOverLap), none below 0
GNSS_ACF_HD int64_t acf_windows(int64_t L, int64_t ind_start, int64_t numOverLap)
{
    return L > ind_start ? (L - ind_start) / numOverLap : 0;
}

// the first row (0-based) of window m (0-based): r = ind_start - 1 + n + (m - 1) * numOverLap
GNSS_ACF_HD int64_t acf_window_row(int64_t m, int64_t ind_start, int64_t numOverLap)
{
    return ind_start - 1 + m * numOverLap;
}

struct AcfWindow {
    double meanMax, meanDelay, varDelay, meanCodeDisc, varCodeDisc;
};

// One window (:235-274) from its N = numOverLap rows: pm the prompt magnitudes, idx the arg-max
// indices, d the code discriminator. `first`: the channel's first window, whose
// mean(maxCorrInd(m, :)) runs over the n entries the row has so far; later windows divide by N.
GNSS_ACF_HD AcfWindow acf_window(const double* pm, const uint8_t* idx, const double* d, int64_t N, bool first,
                                 double corrSpacing, double cenDelay)
{
    const double dN = (double)N;
    int64_t S = 0;
    double sumMax = 0, sumDelay = 0, sumSq = 0, sumD = 0;
    for (int64_t n = 0; n < N; n++) {
        const double ind = (double)idx[n];
        S += idx[n];
        const double mean = (double)S / (first ? (double)(n + 1) : dN);
        const double t = (ind - mean) * corrSpacing;  // tmpDelay(n) (:238)
        const double sq = t * t;
        const double dl = (ind - cenDelay) * corrSpacing;
        sumMax = n ? sumMax + pm[n] : pm[n];
        sumDelay = n ? sumDelay + dl : dl;
        sumSq = n ? sumSq + sq : sq;
        sumD = n ? sumD + d[n] : d[n];
    }
    AcfWindow w;
    w.meanMax = sumMax / dN;      // :260
    w.meanDelay = sumDelay / dN;  // :270
    w.varDelay = sumSq / dN;      // :271
    w.meanCodeDisc = sumD / dN;   // :273
    double ss = 0;                // var (:274): about the mean, n - 1 below
    for (int64_t n = 0; n < N; n++) {
        const double e = d[n] - w.meanCodeDisc;
        const double e2 = e * e;
        ss = n ? ss + e2 : e2;
    }
    w.varCodeDisc = ss / (double)(N - 1);
    return w;
}

// What the kernels take (acf.hip). Every extent was checked by the host: len[c] <= max_len and
// the rows of windows[c] windows lie below len[c].
struct AcfDev {
    const double* taps;  // [n][2][25][max_len]
    const double* rec;   // [n][nfields][max_len]
    int64_t max_len;
    int n, nfields, field_d;  // field_d: the code discriminator's series
    int64_t len[kAcfMaxCh];
    int64_t windows[kAcfMaxCh];
    int64_t win_base[kAcfMaxCh + 1];  // windows before channel c; [n] = all of them
    int64_t ind_start, numOverLap;
    double corrSpacing, cenDelay;
    double* pm;       // [n][max_len] prompt magnitudes
    uint8_t* idx;     // [n][max_len] arg-max indices
    double* corr;     // [n][25][max_len] or null
    double* feat;     // [5][win_base[n]]: meanMax, meanDelay, varDelay, meanCodeDisc, varCodeDisc
    uint8_t* cnt;     // [n][max_len] interior local maxima per row (acf_ext.h), or null: not wanted
};

// The two launches on `stream` (a hipStream_t) of the current device: the row pass over
// max(len) rows, then, if any window exists, one lane per window. `vec2`: max_len is even and
// taps, pm and corr are 16-B aligned, so the row pass may load and store two rows at a time.
// Returns the hipError_t of the launches (0: none).
int acf_launch(const AcfDev& d, bool vec2, void* stream);

}  // namespace gnss
