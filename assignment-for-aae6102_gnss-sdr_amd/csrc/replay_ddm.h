// replay_ddm.h — the delay-Doppler map over replayed rows (gnss_replay_ddm; the definition is in
// include/gnss_mi355x.h). One source for the arithmetic of a row's time and rotation, a cell's
// update, its power and the peak rule, called by the host path (replay_ddm.cpp), by the kernels
// (replay_ddm.hip) and by tests/native/replay_ddm_host.cpp, compiled without contraction on every
// side so each operation rounds on its own. The sine and cosine are replay.h's rp_sincos.
// No HIP include and no project include beyond replay.h: the stand-alone test program builds with
// a plain C++ compiler, also under AddressSanitizer and UBSan.
#pragma once

#include "replay.h"

namespace gnss {

constexpr int kDdmMaxTaps = 256;   // GNSS_REPLAY_MAX_TAPS
constexpr int kDdmMaxDopp = 256;   // GNSS_DDM_MAX_DOPP
constexpr int kDdmMaxChan = 64;    // GNSS_MAX_SV
constexpr int kDdmMaxRows = 4096;  // rows_per_window at most
constexpr double kDdmMaxHz = 1e5;  // |dopp_hz[m]| at most
constexpr int64_t kDdmMaxSpan = (int64_t)1 << 50;  // bytes from a window's first row at most

// the kernel's tiling (replay_ddm.hip); the tests place their shapes around these
constexpr int kDdmLanes = 256;     // lanes of a workgroup: kDdmBinTile / kDdmLaneBins waves of kDdmTapTile
constexpr int kDdmTapTile = 64;    // taps of a workgroup: a lane owns one
constexpr int kDdmLaneBins = 16;   // bins whose two sums a lane keeps in registers
constexpr int kDdmBinTile = 64;    // bins of a workgroup: wave v owns bins v*16 .. v*16+15 of them
constexpr int kDdmRowTile = 32;    // rows that go through LDS at a time

// the row's middle sample in seconds from the window's first sample: s = samples from the
// window's first sample to the row's first, n = numSample
GNSS_RP_HD double ddm_row_time(int64_t s, int64_t n, double Fs)
{
    return ((double)(2 * s + n - 1) / 2.0) / Fs;
}

// (sn, cs) of the rotation by nu Hz at row time t
GNSS_RP_HD void ddm_rotation(double nu, double t, double* sn, double* cs)
{
    const double th = nu * t;
    const double r = th - rint(th);
    rp_sincos(kRpTwoPi * r, sn, cs);
}

// the row's sign from the prompt tap's I (acf_fit_taps.h ftt_sign): a NaN gives -1
GNSS_RP_HD double ddm_sign(double promptI)
{
    return promptI >= 0 ? 1.0 : -1.0;
}

// one more row into a cell: sI, sQ the row's sums times its sign (s*(I*cs + Q*sn) is
// (s*I)*cs + (s*Q)*sn bit for bit: negation is exact and rounding is symmetric)
GNSS_RP_HD void ddm_cell(double sI, double sQ, double sn, double cs, double* ZI, double* ZQ)
{
    *ZI += sI * cs + sQ * sn;
    *ZQ += sQ * cs - sI * sn;
}

GNSS_RP_HD double ddm_power(double ZI, double ZQ)
{
    return ZI * ZI + ZQ * ZQ;
}

// ---- the peak rule: the largest power, the lowest cell number among equals; a NaN is no candidate
struct DdmBest {
    double pow;
    int k;  // cell number m * n_taps + j, -1: none
};

GNSS_RP_HD DdmBest ddm_best_none()
{
    return DdmBest{0.0, -1};
}

// whether candidate (p, k), k >= 0, comes before b in the rule's order
GNSS_RP_HD bool ddm_best_before(const DdmBest& b, double p, int k)
{
    if (!(p == p)) return false;
    return b.k < 0 || p > b.pow || (p == b.pow && k < b.k);
}

GNSS_RP_HD void ddm_best_take(DdmBest& b, double p, int k)
{
    if (ddm_best_before(b, p, k)) b = DdmBest{p, k};
}

// another share's best into b (any order of merging gives the same winner: the rule is a total order)
GNSS_RP_HD void ddm_best_merge(DdmBest& b, double p, int k)
{
    if (k >= 0) ddm_best_take(b, p, k);
}

// whether cell (m, j) lies outside the exclusion box around the peak (pm, pj)
GNSS_RP_HD bool ddm_outside(const double* u, const double* hz, int m, int j, int pm, int pj, double excl_chips,
                            double excl_hz)
{
    return fabs(u[j] - u[pj]) >= excl_chips || fabs(hz[m] - hz[pm]) >= excl_hz;
}

// a window's six peak outputs
struct DdmPeaks {
    int32_t peak_bin, peak_tap, sec_bin, sec_tap;
    double peak_pow, sec_pow;
};

GNSS_RP_HD DdmPeaks ddm_peaks_of(const DdmBest& p, const DdmBest& s, int n_taps)
{
    const double nan = __builtin_nan("");
    DdmPeaks r;
    r.peak_bin = p.k < 0 ? -1 : p.k / n_taps;
    r.peak_tap = p.k < 0 ? -1 : p.k % n_taps;
    r.peak_pow = p.k < 0 ? nan : p.pow;
    r.sec_bin = s.k < 0 ? -1 : s.k / n_taps;
    r.sec_tap = s.k < 0 ? -1 : s.k % n_taps;
    r.sec_pow = s.k < 0 ? nan : s.pow;
    return r;
}

// the peaks of one window's map zI, zQ [n_dopp][n_taps], cells ascending (the host path)
inline DdmPeaks ddm_peaks_host(const double* zI, const double* zQ, int n_dopp, int n_taps, const double* u,
                               const double* hz, double excl_chips, double excl_hz)
{
    DdmBest p = ddm_best_none(), s = ddm_best_none();
    const int cells = n_dopp * n_taps;
    for (int k = 0; k < cells; k++) ddm_best_take(p, ddm_power(zI[k], zQ[k]), k);
    if (p.k >= 0)
        for (int k = 0; k < cells; k++)
            if (ddm_outside(u, hz, k / n_taps, k % n_taps, p.k / n_taps, p.k % n_taps, excl_chips, excl_hz))
                ddm_best_take(s, ddm_power(zI[k], zQ[k]), k);
    return ddm_peaks_of(p, s, n_taps);
}

// One window on the host: I / Q the window's first row of tap 0's series (tap j's at j * stride),
// prompt the prompt tap's I series or null, t the rows' times -> zI, zQ [n_dopp][n_taps]. sg, sn,
// cs: R doubles of scratch each. Every cell is a plain ascending sum over the rows.
inline void ddm_window_host(const double* I, const double* Q, int64_t stride, const double* prompt, const double* t,
                            int R, int n_taps, int n_dopp, const double* hz, double* sg, double* sn, double* cs,
                            double* zI, double* zQ)
{
    for (int i = 0; i < R; i++) sg[i] = prompt ? ddm_sign(prompt[i]) : 1.0;
    for (int m = 0; m < n_dopp; m++) {
        for (int i = 0; i < R; i++) ddm_rotation(hz[m], t[i], &sn[i], &cs[i]);
        for (int j = 0; j < n_taps; j++) {
            const double* Ij = I + (int64_t)j * stride;
            const double* Qj = Q + (int64_t)j * stride;
            double aI = 0.0, aQ = 0.0;
            for (int i = 0; i < R; i++) ddm_cell(sg[i] * Ij[i], sg[i] * Qj[i], sn[i], cs[i], &aI, &aQ);
            zI[(int64_t)m * n_taps + j] = aI;
            zQ[(int64_t)m * n_taps + j] = aQ;
        }
    }
}

// ---- the kernels' launch (replay_ddm.hip); host code sees only this ------------------------------
struct DdmArgs {
    const double* taps;   // [n][2][n_taps][max_rows]                         (device arrays)
    const double* t;      // [n][max_rows] the rows' times
    const double* hz;     // [n_dopp]
    const double* u;      // [n_taps]
    double* map;          // window slot s: [s][2][n_dopp][n_taps]
    DdmPeaks* peaks;      // [windows of all channels]
    int64_t max_rows;
    int64_t slot_cap;     // > 0: channel c's window m has slot c * slot_cap + m; 0: its number w
    int32_t n, n_taps, n_dopp, prompt, R;
    double excl_chips, excl_hz;
    int64_t win_base[kDdmMaxChan + 1];  // channel c's windows are numbers win_base[c] .. win_base[c+1]-1
};

// the map kernel over (windows, bin tiles, tap tiles), then the peak kernel over the windows, on
// `stream` (a hipStream_t). Returns the hipError_t as an int.
int replay_ddm_launch(const DdmArgs& a, void* stream);

}  // namespace gnss
