// acf_fit.h — the two-path fit of the 25-tap ACF (gnss_acf_fit; the definition is in
// include/gnss_mi355x.h). Per feature window (acf.h's windows):
//   1. the coherent tap vector: the window's rows summed per tap with the sign of the prompt's I
//      sum of the same row (the navigation bit wiped by the prompt itself), and its energy;
//   2. the one-path grid  z[j] ~ A R(u[j] - p)  and the two-path grid
//      z[j] ~ A0 R(u[j] - p) + A1 R(u[j] - (p - e)),  R(x) = max(0, 1 - |x|), the amplitudes by
//      least squares per hypothesis, the smallest residual kept (lowest index on a tie);
//   3. the selection between the two.
// One source for the arithmetic, called in loops by the host path (acf_fit.cpp) and by the kernel
// for GNSS_OUT_DEVICE records (acf_fit.hip), compiled without contraction and without fast-math on
// both sides; every sum runs left to right from its first term: the two paths give the same bits.
// No HIP include and no project include: tests/native/acf_fit_host.cpp calls these functions on
// the CPU under AddressSanitizer and UBSan.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define GNSS_FIT_HD __host__ __device__ inline __attribute__((always_inline))
// the tap loops of a hypothesis five taps at a time: unrolled whole, the kernel's compiler keeps
// all 50 z values and all 50 R values of a hypothesis in registers (256 VGPRs, one wave per SIMD)
#define GNSS_FIT_TAP_LOOP _Pragma("unroll 5")
#else
#define GNSS_FIT_HD inline
#define GNSS_FIT_TAP_LOOP
#endif

namespace gnss {

constexpr int kFitTaps = 25;          // = GNSS_MC_TAPS
constexpr int kFitPrompt = 12;        // the prompt tap, storage order
constexpr int kFitMaxCh = 32;         // = GNSS_VT_MAX_CH
constexpr int kFitMaxHyp = 65536;     // p_count * e_count at most
constexpr int kFitNone = 0x7fffffff;  // the hypothesis index of "none survived"
constexpr int kFitRow = 16;           // doubles per window in the kernel's output (AcfFitRow)

// the grid and the two thresholds (gnss_acf_fit_cfg's fields)
struct AcfFitGrid {
    double orient;  // +1 or -1
    double corrSpacing;
    double p_min, p_step, e_min, e_step;
    int p_count, e_count;
    double ratio_max, gain_min;
};

// one window's result; the kernel writes it as kFitRow doubles in this order
struct AcfFitRow {
    double paths;                // 0, 1 or 2
    double bias;                 // p of the selected model
    double p1, A1p_re, A1p_im, res1;
    double p0, e, A0_re, A0_im, A1_re, A1_im, res2;
    double energy;
    double spare[2];
};
static_assert(sizeof(AcfFitRow) == kFitRow * sizeof(double), "the kernel stores AcfFitRow as kFitRow doubles");

// s_r: +1 if the prompt's I sum is >= 0, else -1 (a NaN compares false: -1)
GNSS_FIT_HD double fit_sign(double promptI)
{
    return promptI >= 0 ? 1.0 : -1.0;
}

// one more row into a coherent sum: acc + s * v, the first row's term as it is
GNSS_FIT_HD double fit_accum(double acc, double s, double v, bool first)
{
    const double t = s * v;
    return first ? t : acc + t;
}

// u[j] = orient * (j - 12) * corrSpacing; the fits take the 25 of them as an array
GNSS_FIT_HD double fit_u(const AcfFitGrid& g, int j)
{
    return (g.orient * (double)(j - kFitPrompt)) * g.corrSpacing;
}

GNSS_FIT_HD double fit_p(const AcfFitGrid& g, int ip)
{
    return g.p_min + (double)ip * g.p_step;
}

GNSS_FIT_HD double fit_e(const AcfFitGrid& g, int ie)
{
    return g.e_min + (double)ie * g.e_step;
}

// R(x) = max(0, 1 - |x|)
GNSS_FIT_HD double fit_R(double x)
{
    const double t = 1.0 - fabs(x);
    return t > 0 ? t : 0.0;
}

GNSS_FIT_HD bool fit_finite(double x)
{
    return x - x == 0;
}

// energy = sum_j (zI*zI + zQ*zQ), j ascending
GNSS_FIT_HD double fit_energy(const double* zI, const double* zQ)
{
    double s = 0;
    for (int j = 0; j < kFitTaps; j++) {
        const double t = zI[j] * zI[j] + zQ[j] * zQ[j];
        s = j ? s + t : t;
    }
    return s;
}

GNSS_FIT_HD bool fit_all_finite(const double* zI, const double* zQ)
{
    bool ok = true;
    for (int j = 0; j < kFitTaps; j++) ok = ok && fit_finite(zI[j]) && fit_finite(zQ[j]);
    return ok;
}

// (res, h) below (bres, bh) lexicographically; a NaN res is below nothing
GNSS_FIT_HD bool fit_better(double res, int h, double bres, int bh)
{
    return res < bres || (res == bres && h < bh);
}

// a hypothesis' amplitudes and residual; ok: it was not skipped
struct AcfFitHyp {
    bool ok;
    double A0_re, A0_im, A1_re, A1_im, res;
};

// the one-path hypothesis p (its amplitude in A0)
GNSS_FIT_HD AcfFitHyp fit_one(const double* u, const double* zI, const double* zQ, double p)
{
    AcfFitHyp o{};
    double a = 0, hI = 0, hQ = 0;
    GNSS_FIT_TAP_LOOP
    for (int j = 0; j < kFitTaps; j++) {
        const double r = fit_R(u[j] - p);
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
    GNSS_FIT_TAP_LOOP
    for (int j = 0; j < kFitTaps; j++) {
        const double r = fit_R(u[j] - p);
        const double dI = zI[j] - o.A0_re * r, dQ = zQ[j] - o.A0_im * r;
        const double t = dI * dI + dQ * dQ;
        res = j ? res + t : t;
    }
    o.res = res;
    return o;
}

// the two-path hypothesis: the direct path at p, the reflected one at q = p - e
GNSS_FIT_HD AcfFitHyp fit_two(const AcfFitGrid& g, const double* u, const double* zI, const double* zQ, double p,
                              double q)
{
    AcfFitHyp o{};
    double a = 0, b = 0, c = 0, h0I = 0, h0Q = 0, h1I = 0, h1Q = 0;
    GNSS_FIT_TAP_LOOP
    for (int j = 0; j < kFitTaps; j++) {
        const double r0 = fit_R(u[j] - p), r1 = fit_R(u[j] - q);
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
    GNSS_FIT_TAP_LOOP
    for (int j = 0; j < kFitTaps; j++) {
        const double r0 = fit_R(u[j] - p), r1 = fit_R(u[j] - q);
        const double dI = (zI[j] - o.A0_re * r0) - o.A1_re * r1;
        const double dQ = (zQ[j] - o.A0_im * r0) - o.A1_im * r1;
        const double t = dI * dI + dQ * dQ;
        res = j ? res + t : t;
    }
    o.res = res;
    return o;
}

// hypothesis h of the two-path grid, h = ip * e_count + ie
GNSS_FIT_HD AcfFitHyp fit_two_at(const AcfFitGrid& g, const double* u, const double* zI, const double* zQ, int h)
{
    const double p = fit_p(g, h / g.e_count);
    return fit_two(g, u, zI, zQ, p, p - fit_e(g, h % g.e_count));
}

// the best hypothesis of a grid so far: the lexicographic minimum of (res, index)
struct AcfFitBest {
    double res;
    int h;
};
GNSS_FIT_HD AcfFitBest fit_best_none()
{
    return AcfFitBest{INFINITY, kFitNone};
}
GNSS_FIT_HD void fit_best_take(AcfFitBest& b, const AcfFitHyp& y, int h)
{
    if (y.ok && fit_better(y.res, h, b.res, b.h)) {
        b.res = y.res;
        b.h = h;
    }
}
GNSS_FIT_HD void fit_best_merge(AcfFitBest& b, double res, int h)
{
    if (fit_better(res, h, b.res, b.h)) {
        b.res = res;
        b.h = h;
    }
}

// The window's row from its coherent vector and the winners of both grids (kFitNone: none). The
// winners' amplitudes are formed again from their indices: the same operations, the same bits.
// paths = 0 (every field NaN) for a non-finite z or when no one-path hypothesis survived.
GNSS_FIT_HD AcfFitRow fit_select(const AcfFitGrid& g, const double* u, const double* zI, const double* zQ, int best1,
                                 int best2)
{
    const double nan = NAN;
    const bool fit = fit_all_finite(zI, zQ) && best1 != kFitNone;
    const bool two = fit && best2 != kFitNone;
    const int i1 = fit ? best1 : 0, i2 = two ? best2 : 0;  // (index 0 stands in where nothing is reported)
    const double p1 = fit_p(g, i1), p0 = fit_p(g, i2 / g.e_count), e = fit_e(g, i2 % g.e_count);
    const AcfFitHyp y1 = fit_one(u, zI, zQ, p1);
    const AcfFitHyp y2 = fit_two(g, u, zI, zQ, p0, p0 - e);
    const double energy = fit_energy(zI, zQ);
    const double paths = !fit ? 0.0 : (two && y1.res > g.gain_min * y2.res) ? 2.0 : 1.0;
    return AcfFitRow{paths,
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
GNSS_FIT_HD AcfFitRow fit_window(const AcfFitGrid& g, const double* zI, const double* zQ)
{
    AcfFitBest b1 = fit_best_none(), b2 = fit_best_none();
    double u[kFitTaps];
    for (int j = 0; j < kFitTaps; j++) u[j] = fit_u(g, j);
    if (fit_all_finite(zI, zQ)) {
        for (int ip = 0; ip < g.p_count; ip++) fit_best_take(b1, fit_one(u, zI, zQ, fit_p(g, ip)), ip);
        const int H = g.p_count * g.e_count;
        for (int h = 0; h < H; h++) fit_best_take(b2, fit_two_at(g, u, zI, zQ, h), h);
    }
    return fit_select(g, u, zI, zQ, b1.h, b2.h);
}

// What the kernel takes (acf_fit.hip). Every extent was checked by the host: the rows of
// windows[c] windows lie below len[c] <= max_len.
struct AcfFitDev {
    const double* taps;  // [n][2][25][max_len]
    int64_t max_len;
    int n;
    int64_t win_base[kFitMaxCh + 1];  // windows before channel c; [n] = all of them (< 2^31)
    int64_t ind_start, numOverLap;
    AcfFitGrid grid;
    double* rows;  // [win_base[n]][kFitRow]
    double* z;     // [win_base[n]][2][25]: zI then zQ per window, or null
};

// One block per window on `stream` (a hipStream_t) of the current device. Returns the hipError_t
// of the launch (0: none).
int acf_fit_launch(const AcfFitDev& d, void* stream);

}  // namespace gnss
