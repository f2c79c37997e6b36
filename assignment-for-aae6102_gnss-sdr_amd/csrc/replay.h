// replay.h — the replay correlator (gnss_replay_correlate; the definition is in
// include/gnss_mi355x.h): one recorded tracking row correlated again on any tap grid, with no loop
// closed. One source for the arithmetic of a row, called by the host path (replay.cpp), by the
// kernel (replay.hip) and by tests/native/replay_host.cpp, compiled without contraction on every
// side so each operation rounds on its own:
//   - MATLAB's colon per tap (MathWorks' colonop construction, as gnss_internal.h's colon_make);
//   - the sample's carrier wipe: the reference's Wave(k) = 2*pi*(carrFreq*(k/Fs)) + remPhase with
//     its own roundings, reduced by 2*pi in two parts, then sin / cos by the fdlibm kernels
//     (gnss_internal.h's sincos_small restated for host and device);
//   - per tap the element of its colon, the chip CA[(ceil(t) + chip_off + 1022) mod 1023] with a
//     true modulus, and the two signed sums.
// replay_lane() walks samples k0, k0 + stride, ... of a row for a tile of kReplayTile taps: the
// host path calls it with (0, 1), a kernel lane with (lane, 256). The code lookup is the caller's
// (a modulus on the host, an LDS table in the kernel), handed in as a functor.
// No HIP include and no project include: the stand-alone test program builds with a plain C++
// compiler, also under AddressSanitizer and UBSan.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GNSS_RP_HD __host__ __device__ __forceinline__
#else
#define GNSS_RP_HD inline
#endif

namespace gnss {

constexpr int kReplayMaxTaps = 256;                   // GNSS_REPLAY_MAX_TAPS
constexpr int kReplayTile = 32;                       // taps whose sums a lane keeps in registers
constexpr int kReplayLanes = 256;                     // lanes of the kernel's workgroup
constexpr int64_t kReplayMaxSamples = (int64_t)1 << 22;
constexpr double kReplayMaxTap = 1023.0;              // |tap_offsets[s]| and |post[s]| at most
constexpr double kReplayMaxChips = 1073741824.0 / 4;  // a row's code advance (n - 1) * d at most (2^28)
// the kernel's periodic code table: chips a (row, tile) may span and still use it (1 byte each);
// ten code periods and taps at +-1023 fit
constexpr int kReplayTabMax = 16384;

constexpr double kRpTwoPi = 2.0 * 3.14159265358979323846;  // MATLAB 2*pi
constexpr double kRpTwoPiLo = 2.4492935982947064e-16;      // 2*pi - kRpTwoPi

struct RpColon {
    double a, d, c;
    int64_t n;  // intervals; elements = n + 1 (-1: no such colon)
};

// MATLAB colon a:d:b (gnss_internal.h colon_make, operation for operation)
GNSS_RP_HD RpColon rp_colon_make(double a, double d, double b)
{
    RpColon r{a, d, b, -1};
    if (!(a - a == 0) || !(d - d == 0) || !(b - b == 0)) return r;
    if (d == 0 || (a < b && d < 0) || (b < a && d > 0)) return r;
    const double tol = 2.0 * 2.220446049250313e-16 * fmax(fabs(a), fabs(b));
    const double sig = d > 0 ? 1.0 : -1.0;
    double n;
    if (a == floor(a) && d == 1) {
        n = floor(b) - a;
    } else if (a == floor(a) && d == floor(d)) {
        const double q = floor(a / d);
        const double rr = a - q * d;
        n = floor((b - rr) / d) - q;
    } else {
        n = round((b - a) / d);
        if (sig * (a + n * d - b) > tol) n = n - 1;
    }
    double c = a + n * d;
    if (sig * (c - b) > -tol) c = b;
    r.c = c;
    r.n = (int64_t)n;
    return r;
}

// tap offset `tap` of a row of n samples: (0 + tap + remChip) : d : ((n-1)*d + tap + remChip)
GNSS_RP_HD RpColon rp_tap_colon(double tap, double remChip, double d, int64_t n)
{
    const double a = (0 + tap) + remChip;
    return rp_colon_make(a, d, ((double)(n - 1) * d + tap) + remChip);
}

// element k of a colon with nn intervals between a and c (gnss_internal.h colon_elem)
GNSS_RP_HD double rp_colon_elem(double a, double c, double d, int64_t nn, int64_t k)
{
    if (2 * k == nn) return (a + c) / 2;
    if (k <= nn / 2) return a + (double)k * d;
    return c - (double)(nn - k) * d;
}

// CA index of chip number `chip` (= ceil(t) + chip_off): (chip + 1022) mod 1023, true modulus
GNSS_RP_HD int rp_chip_index(int64_t chip)
{
    const int64_t r = (chip + 1022) % 1023;
    return (int)(r < 0 ? r + 1023 : r);
}

// sin and cos of a 2*pi-reduced phase (gnss_internal.h sincos_small, operation for operation)
GNSS_RP_HD void rp_sincos(double x, double* sn, double* cs)
{
    constexpr double kTwoOverPi = 6.36619772367581382433e-01;
    constexpr double kPio2Hi = 1.57079632673412561417e+00;
    constexpr double kPio2Lo = 6.07710050650619224932e-11;
    const double q = rint(x * kTwoOverPi);
    double y = __builtin_fma(-q, kPio2Hi, x);
    const double t = q * kPio2Lo;
    const double yh = y - t;
    const double yl = (y - yh) - t;
    y = yh;
    const double z = y * y;
    const double rs = __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, __builtin_fma(z,
        1.58969099521155010221e-10, -2.50507602534068634195e-08), 2.75573137070700676789e-06),
        -1.98412698298579493134e-04), 8.33333333332248946124e-03);
    const double rc = z * __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, __builtin_fma(z,
        __builtin_fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09),
        -2.75573143513906633035e-07), 2.48015872894767294178e-05), -1.38888888888741095749e-03),
        4.16666666666666019037e-02);
    const double v = z * y;
    const double s = y - ((z * (0.5 * yl - v * rs) - yl) - v * -1.66666666666666324348e-01);
    const double hz = 0.5 * z;
    const double w = 1.0 - hz;
    const double c = w + (((1.0 - w) - hz) + (z * rc - y * yl));
    const int n = (int)q & 3;
    const double a = (n & 1) ? c : s, b = (n & 1) ? s : c;
    *sn = (n & 2) ? -a : a;
    *cs = ((n + 1) & 2) ? -b : b;
}

// What a row's samples and carrier need: x = the row's first byte, dtype 2 (int8 I/Q pairs) or 1
// (int8 real, xi = 0); rfs = RN(1/Fs) where the caller has verified that the FMA-corrected
// k * rfs is the IEEE quotient k / Fs for every k < n, else 0 (then the division itself).
struct RpRow {
    const uint8_t* x;
    int64_t n;
    int dtype;
    double Fs, rfs, f, phi0, d;  // f = carrFreq, phi0 = remPhase, d = codeFreq / Fs
};

// sample k carrier-wiped: I = xr*sin + xi*cos, Q = xr*cos - xi*sin (trackingCT.m:96-118)
GNSS_RP_HD void rp_wipe(const RpRow& r, int64_t k, double* tI, double* tQ)
{
    double t;
    if (r.rfs != 0.0) {  // (gnss_internal.h div_markstein)
        const double q = (double)k * r.rfs;
        t = __builtin_fma(__builtin_fma(-q, r.Fs, (double)k), r.rfs, q);
    } else {
        t = (double)k / r.Fs;
    }
    const double W = kRpTwoPi * (r.f * t) + r.phi0;
    const double q = rint(W * (1.0 / kRpTwoPi));
    double rr = __builtin_fma(-q, kRpTwoPi, W);
    rr = __builtin_fma(-q, kRpTwoPiLo, rr);
    double sn, cs;
    rp_sincos(rr, &sn, &cs);
    double xr, xi;
    if (r.dtype == 1) {
        xr = (double)(int8_t)r.x[k];
        xi = 0.0;
    } else {
        xr = (double)(int8_t)r.x[2 * k];
        xi = (double)(int8_t)r.x[2 * k + 1];
    }
    *tI = xr * sn + xi * cs;
    *tQ = xr * cs - xi * sn;
}

// Samples k0, k0 + stride, ... < n of row r against nt <= kReplayTile taps: tac[0][j] / tac[1][j]
// tap j's colon ends a / c, tp what is added to an element before ceil (null: nothing), neg(chip)
// whether the replica at chip number ceil(t) is -1 (chip_off is the functor's business). accI /
// accQ [kReplayTile] are added to, ascending k. A sample reads one end per tap, the one its half
// of the colon counts from (c - (nn-k)*d is c + -((nn-k)*d) exactly); the one middle sample of an
// odd-length row reads both.
template <class CodeNeg>
GNSS_RP_HD void replay_lane(const RpRow& r, const double (*tac)[kReplayTile], const double* tp, int nt, int64_t k0,
                            int64_t stride, CodeNeg neg, double* accI, double* accQ)
{
    const int64_t nn = r.n - 1;
    for (int64_t k = k0; k < r.n; k += stride) {
        double tI, tQ;
        rp_wipe(r, k, &tI, &tQ);
        const bool mid = 2 * k == nn, low = k <= nn / 2;
        const double e = low ? (double)k * r.d : -((double)(nn - k) * r.d);
        const double* end = tac[low ? 0 : 1];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < kReplayTile; j++) {
            if (j < nt) {
                double tk = end[j] + e;
                if (mid) tk = (tac[0][j] + tac[1][j]) / 2;
                if (tp) tk = tk + tp[j];
                const bool ng = neg((int)ceil(tk));
                accI[j] += ng ? -tI : tI;
                accQ[j] += ng ? -tQ : tQ;
            }
        }
    }
}

// The first tap (0-based) whose colon has not exactly n elements, or -1
inline int replay_bad_tap(const double* taps, int ntaps, double remChip, double d, int64_t n)
{
    for (int s = 0; s < ntaps; s++)
        if (rp_tap_colon(taps[s], remChip, d, n).n != n - 1) return s;
    return -1;
}

// One row on the host: every tap's (I, Q) sum, each a plain ascending sum over the samples, to
// outI[s * out_stride], outQ[s * out_stride]. ca_neg[1023]: 1 where the C/A chip is -1. post may
// be null. The caller has checked the row (replay_bad_tap, the bounds of include/gnss_mi355x.h).
inline void replay_row_host(const RpRow& r, double remChip, const uint8_t* ca_neg, int ntaps, const double* taps,
                            const double* post, int chip_off, double* outI, double* outQ, int64_t out_stride)
{
    for (int j0 = 0; j0 < ntaps; j0 += kReplayTile) {
        const int nt = ntaps - j0 < kReplayTile ? ntaps - j0 : kReplayTile;
        double tac[2][kReplayTile], tp[kReplayTile], accI[kReplayTile], accQ[kReplayTile];
        for (int j = 0; j < kReplayTile; j++) {
            tac[0][j] = tac[1][j] = tp[j] = accI[j] = accQ[j] = 0.0;
            if (j >= nt) continue;
            const RpColon col = rp_tap_colon(taps[j0 + j], remChip, r.d, r.n);
            tac[0][j] = col.a;
            tac[1][j] = col.c;
            tp[j] = post ? post[j0 + j] : 0.0;
        }
        replay_lane(r, tac, post ? tp : nullptr, nt, 0, 1,
                    [&](int chip) { return ca_neg[rp_chip_index((int64_t)chip + chip_off)] != 0; }, accI, accQ);
        for (int j = 0; j < nt; j++) {
            outI[(int64_t)(j0 + j) * out_stride] = accI[j];
            outQ[(int64_t)(j0 + j) * out_stride] = accQ[j];
        }
    }
}

// ---- the kernel's launch (replay.hip); host code sees only this ----------------------------------
constexpr int kReplayMaxChan = 64;  // GNSS_MAX_SV
struct ReplayArgs {
    const uint8_t* rec;       // staged record window: file byte b at rec[b - base]
    int64_t base;
    const int64_t* pos;       // [n_chan][max_rows] the rows' first file byte   (device arrays)
    const int64_t* ns;        //                    numSample
    const double* remChip;    //                    NCO state at the row's start
    const double* codeFreq;
    const double* carrFreq;
    const double* remPhase;
    const unsigned* ca_bits;  // [n_chan][32] C/A chips, bit set = -1
    const double* taps;       // [n_taps]
    const double* post;       // [n_taps], or null
    double* out;              // [n_chan][2][n_taps][max_rows]
    int64_t max_rows, row0;   // the launch covers rows row0 .. row0 + grid.x - 1
    int32_t n_taps, chip_off, dtype, n_chan;
    double Fs, rfs;
    int64_t n_rows[kReplayMaxChan];
};

// The chip numbers ceil(t) a tap with colon ends a, c and post p can take, one chip of margin on
// either side: every element lies in [a, c] up to the colon's end tolerance of a few ulps, and
// adding p and rounding are monotone. The kernel's table covers the union over a tile's taps; the
// host asks the same function whether every (row, tile) of a launch fits kReplayTabMax.
GNSS_RP_HD void rp_chip_range(double a, double c, double p, int* lo, int* hi)
{
    *lo = (int)ceil(a + p) - 1;
    *hi = (int)ceil(c + p) + 1;
}

// rows blocks x n_chan x tiles of kReplayLanes lanes on `stream` (a hipStream_t); table: every
// (row, tile) of the launch spans at most kReplayTabMax chips, so the code is looked up in the LDS
// table, else by modulus (the same chips either way). Returns the hipError_t as an int.
int replay_launch(const ReplayArgs& a, int64_t rows, bool table, void* stream);

}  // namespace gnss
