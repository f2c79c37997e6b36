// acf_fit_taps.h — the two-path fit of an ACF on any tap grid (gnss_acf_fit_taps; the definition
// is gnss_acf_fit's in include/gnss_mi355x.h with three substitutions: 25 taps become n_taps in
// 1..256, the prompt index 12 becomes `prompt`, and u[j] = (orient*(j-12))*corrSpacing becomes
// u[j] as the caller gives it, in orient = +1's convention). Everything else is acf_fit.h's,
// operation for operation: the windows, the first-row rule of the coherent sums, every sum left to
// right from its first term, the skip rules, the lexicographic minimum of (res, index), the
// winners formed again from their indices, paths = 0 / 1 / 2 and the NaN outputs. With n_taps =
// 25, prompt = 12 and u[j] = (orient*(j-12))*corrSpacing every output equals gnss_acf_fit's bit
// for bit. acf_fit.h itself is left as it is for its kernel, whose tap count is a compile-time 25;
// gnss_acf_fit's host path runs on this file (acf_fit.cpp).
// One source for the arithmetic, called in loops by the host paths (acf_fit_host.h's driver for
// acf_fit.cpp and acf_fit_taps.cpp) and by the kernel (acf_fit_taps.hip), compiled without
// contraction and without fast-math on both sides.
// No HIP include and no project include: tests/native/acf_fit_taps_host.cpp calls these functions
// on the CPU under AddressSanitizer and UBSan.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define GNSS_FTT_HD __host__ __device__ inline __attribute__((always_inline))
// the tap loops have a run-time trip count: four taps per trip give the seven sums of a
// hypothesis independent work to overlap, and the remainder loop stays short
#define GNSS_FTT_TAP_LOOP _Pragma("unroll 4")
#else
#define GNSS_FTT_HD inline
#define GNSS_FTT_TAP_LOOP
#endif

namespace gnss {

constexpr int kFttMaxTaps = 256;      // = GNSS_REPLAY_MAX_TAPS
constexpr int kFttMaxCh = 32;         // = GNSS_VT_MAX_CH
constexpr int kFttMaxHyp = 65536;     // p_count * e_count at most
constexpr int kFttNone = 0x7fffffff;  // the hypothesis index of "none survived"
constexpr int kFttRow = 16;           // doubles per window in the kernel's output (AcfFttRow)

// the taps, the grid and the two thresholds (gnss_acf_fit_taps_cfg's fields; u travels beside it)
struct AcfFttGrid {
    int n_taps, prompt;
    double p_min, p_step, e_min, e_step;
    int p_count, e_count;
    double ratio_max, gain_min;
};

// one window's result; the kernel writes it as kFttRow doubles in this order (acf_fit.h's AcfFitRow)
struct AcfFttRow {
    double paths;                // 0, 1 or 2
    double bias;                 // p of the selected model
    double p1, A1p_re, A1p_im, res1;
    double p0, e, A0_re, A0_im, A1_re, A1_im, res2;
    double energy;
    double spare[2];
};
static_assert(sizeof(AcfFttRow) == kFttRow * sizeof(double), "the kernel stores AcfFttRow as kFttRow doubles");

// windows of a channel with L rows and the first row (0-based) of window m: acf.h's acf_windows
// and acf_window_row
GNSS_FTT_HD int64_t ftt_windows(int64_t L, int64_t ind_start, int64_t numOverLap)
{
    return L > ind_start ? (L - ind_start) / numOverLap : 0;
}
GNSS_FTT_HD int64_t ftt_window_row(int64_t m, int64_t ind_start, int64_t numOverLap)
{
    return ind_start - 1 + m * numOverLap;
}

// s_r: +1 if the prompt's I sum is >= 0, else -1 (a NaN compares false: -1)
GNSS_FTT_HD double ftt_sign(double promptI)
{
    return promptI >= 0 ? 1.0 : -1.0;
}

// one more row into a coherent sum: acc + s * v, the first row's term as it is
GNSS_FTT_HD double ftt_accum(double acc, double s, double v, bool first)
{
    const double t = s * v;
    return first ? t : acc + t;
}

GNSS_FTT_HD double ftt_p(const AcfFttGrid& g, int ip)
{
    return g.p_min + (double)ip * g.p_step;
}

GNSS_FTT_HD double ftt_e(const AcfFttGrid& g, int ie)
{
    return g.e_min + (double)ie * g.e_step;
}

// R(x) = max(0, 1 - |x|)
GNSS_FTT_HD double ftt_R(double x)
{
    const double t = 1.0 - fabs(x);
    return t > 0 ? t : 0.0;
}

GNSS_FTT_HD bool ftt_finite(double x)
{
    return x - x == 0;
}

// energy = sum_j (zI*zI + zQ*zQ), j ascending
GNSS_FTT_HD double ftt_energy(int n, const double* zI, const double* zQ)
{
    double s = 0;
    for (int j = 0; j < n; j++) {
        const double t = zI[j] * zI[j] + zQ[j] * zQ[j];
        s = j ? s + t : t;
    }
    return s;
}

GNSS_FTT_HD bool ftt_all_finite(int n, const double* zI, const double* zQ)
{
    bool ok = true;
    for (int j = 0; j < n; j++) ok = ok && ftt_finite(zI[j]) && ftt_finite(zQ[j]);
    return ok;
}

// (res, h) below (bres, bh) lexicographically; a NaN res is below nothing
GNSS_FTT_HD bool ftt_better(double res, int h, double bres, int bh)
{
    return res < bres || (res == bres && h < bh);
}

// a hypothesis' amplitudes and residual; ok: it was not skipped
struct AcfFttHyp {
    bool ok;
    double A0_re, A0_im, A1_re, A1_im, res;
};

// the one-path hypothesis p (its amplitude in A0); every sum over all n taps
GNSS_FTT_HD AcfFttHyp ftt_one(int n, const double* u, const double* zI, const double* zQ, double p)
{
    AcfFttHyp o{};
    double a = 0, hI = 0, hQ = 0;
    GNSS_FTT_TAP_LOOP
    for (int j = 0; j < n; j++) {
        const double r = ftt_R(u[j] - p);
        const double rr = r * r, tI = r * zI[j], tQ = r * zQ[j];
        a = j ? a + rr : rr;
        hI = j ? hI + tI : tI;
        hQ = j ? hQ + tQ : tQ;
    }
    if (a == 0) return o;
    o.ok = true;
    o.A0_re = hI / a;
    o.A0_im = hQ / a;
    double res = 0;
    GNSS_FTT_TAP_LOOP
    for (int j = 0; j < n; j++) {
        const double r = ftt_R(u[j] - p);
        const double dI = zI[j] - o.A0_re * r, dQ = zQ[j] - o.A0_im * r;
        const double t = dI * dI + dQ * dQ;
        res = j ? res + t : t;
    }
    o.res = res;
    return o;
}

// the two-path hypothesis: the direct path at p, the reflected one at q = p - e
GNSS_FTT_HD AcfFttHyp ftt_two(const AcfFttGrid& g, const double* u, const double* zI, const double* zQ, double p,
                              double q)
{
    AcfFttHyp o{};
    const int n = g.n_taps;
    double a = 0, b = 0, c = 0, h0I = 0, h0Q = 0, h1I = 0, h1Q = 0;
    GNSS_FTT_TAP_LOOP
    for (int j = 0; j < n; j++) {
        const double r0 = ftt_R(u[j] - p), r1 = ftt_R(u[j] - q);
        const double t_a = r0 * r0, t_b = r1 * r1, t_c = r0 * r1;
        const double t0I = r0 * zI[j], t0Q = r0 * zQ[j], t1I = r1 * zI[j], t1Q = r1 * zQ[j];
        a = j ? a + t_a : t_a;
        b = j ? b + t_b : t_b;
        c = j ? c + t_c : t_c;
        h0I = j ? h0I + t0I : t0I;
        h0Q = j ? h0Q + t0Q : t0Q;
        h1I = j ? h1I + t1I : t1I;
        h1Q = j ? h1Q + t1Q : t1Q;
    }
    const double det = a * b - c * c;
    if (a == 0 || b == 0 || !(det > (1e-9 * a) * b)) return o;  // a path outside the tap span
    o.A0_re = (b * h0I - c * h1I) / det;
    o.A0_im = (b * h0Q - c * h1Q) / det;
    o.A1_re = (a * h1I - c * h0I) / det;
    o.A1_im = (a * h1Q - c * h0Q) / det;
    const double m0 = o.A0_re * o.A0_re + o.A0_im * o.A0_im;
    const double m1 = o.A1_re * o.A1_re + o.A1_im * o.A1_im;
    if (m1 > (g.ratio_max * g.ratio_max) * m0) return o;  // the reflection above the direct path
    o.ok = true;
    double res = 0;
    GNSS_FTT_TAP_LOOP
    for (int j = 0; j < n; j++) {
        const double r0 = ftt_R(u[j] - p), r1 = ftt_R(u[j] - q);
        const double dI = (zI[j] - o.A0_re * r0) - o.A1_re * r1;
        const double dQ = (zQ[j] - o.A0_im * r0) - o.A1_im * r1;
        const double t = dI * dI + dQ * dQ;
        res = j ? res + t : t;
    }
    o.res = res;
    return o;
}

// hypothesis h of the two-path grid, h = ip * e_count + ie
GNSS_FTT_HD AcfFttHyp ftt_two_at(const AcfFttGrid& g, const double* u, const double* zI, const double* zQ, int h)
{
    const double p = ftt_p(g, h / g.e_count);
    return ftt_two(g, u, zI, zQ, p, p - ftt_e(g, h % g.e_count));
}

// the best hypothesis of a grid so far: the lexicographic minimum of (res, index)
struct AcfFttBest {
    double res;
    int h;
};
GNSS_FTT_HD AcfFttBest ftt_best_none()
{
    return AcfFttBest{INFINITY, kFttNone};
}
GNSS_FTT_HD void ftt_best_take(AcfFttBest& b, const AcfFttHyp& y, int h)
{
    if (y.ok && ftt_better(y.res, h, b.res, b.h)) {
        b.res = y.res;
        b.h = h;
    }
}
GNSS_FTT_HD void ftt_best_merge(AcfFttBest& b, double res, int h)
{
    if (ftt_better(res, h, b.res, b.h)) {
        b.res = res;
        b.h = h;
    }
}

// The window's row from its coherent vector and the winners of both grids (kFttNone: none). The
// winners' amplitudes are formed again from their indices: the same operations, the same bits.
// paths = 0 (every field NaN) for a non-finite z or when no one-path hypothesis survived.
GNSS_FTT_HD AcfFttRow ftt_select(const AcfFttGrid& g, const double* u, const double* zI, const double* zQ, int best1,
                                 int best2)
{
    const double nan = NAN;
    const bool fit = ftt_all_finite(g.n_taps, zI, zQ) && best1 != kFttNone;
    const bool two = fit && best2 != kFttNone;
    const int i1 = fit ? best1 : 0, i2 = two ? best2 : 0;  // (index 0 stands in where nothing is reported)
    const double p1 = ftt_p(g, i1), p0 = ftt_p(g, i2 / g.e_count), e = ftt_e(g, i2 % g.e_count);
    const AcfFttHyp y1 = ftt_one(g.n_taps, u, zI, zQ, p1);
    const AcfFttHyp y2 = ftt_two(g, u, zI, zQ, p0, p0 - e);
    const double energy = ftt_energy(g.n_taps, zI, zQ);
    const double paths = !fit ? 0.0 : (two && y1.res > g.gain_min * y2.res) ? 2.0 : 1.0;
    return AcfFttRow{paths,
                     !fit ? nan : paths == 2 ? p0 : p1,
                     fit ? p1 : nan,
                     fit ? y1.A0_re : nan,
                     fit ? y1.A0_im : nan,
                     fit ? y1.res : nan,
                     two ? p0 : nan,
                     two ? e : nan,
                     two ? y2.A0_re : nan,
                     two ? y2.A0_im : nan,
                     two ? y2.A1_re : nan,
                     two ? y2.A1_im : nan,
                     two ? y2.res : nan,
                     fit ? energy : nan,
                     {0.0, 0.0}};
}

// the whole fit of one coherent vector, in hypothesis order (the host path)
GNSS_FTT_HD AcfFttRow ftt_window(const AcfFttGrid& g, const double* u, const double* zI, const double* zQ)
{
    AcfFttBest b1 = ftt_best_none(), b2 = ftt_best_none();
    if (ftt_all_finite(g.n_taps, zI, zQ)) {
        for (int ip = 0; ip < g.p_count; ip++) ftt_best_take(b1, ftt_one(g.n_taps, u, zI, zQ, ftt_p(g, ip)), ip);
        const int H = g.p_count * g.e_count;
        for (int h = 0; h < H; h++) ftt_best_take(b2, ftt_two_at(g, u, zI, zQ, h), h);
    }
    return ftt_select(g, u, zI, zQ, b1.h, b2.h);
}

// What a kernel over these sums takes beside its own parameters (acf_fit_taps.hip,
// acf_fit_multi.hip); the host driver fills it (acf_fit_host.h). Every extent was checked there: the
// rows of channel c's windows lie below n_rows[c] <= max_rows, n_taps in 1..kFttMaxTaps, prompt
// below it.
struct AcfFttIo {
    const double* taps;  // [n][2][n_taps][max_rows]
    const double* u;     // [n_taps]
    int64_t max_rows;
    int n;
    int64_t win_base[kFttMaxCh + 1];  // windows before channel c; [n] = all of them (< 2^31)
    int64_t ind_start, numOverLap;
    double* rows;  // [win_base[n]][the kernel's doubles per window]
    double* z;     // [win_base[n]][2][n_taps]: zI then zQ per window, or null
};

struct AcfFttDev {
    AcfFttIo io;
    AcfFttGrid grid;
};

// One block per window on `stream` (a hipStream_t) of the current device. Returns the hipError_t
// of the launch (0: none).
int acf_fit_taps_launch(const AcfFttDev& d, void* stream);

}  // namespace gnss
