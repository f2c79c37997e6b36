// replay_ddm_host.cpp -- csrc/replay_ddm.h's functions (the arithmetic shared by the host path and
// the kernels of gnss_replay_ddm) on the CPU: built once plainly and once under AddressSanitizer and
// UBSan (tests/test_native_replay_ddm.py). Every array is a heap array of exactly the stated size
// (the series n_taps * stride doubles with the window's R rows at its end, the times, signs and
// rotations R, the map n_dopp * n_taps twice), so a read or write past one is an error there. The
// expected cells are a naive long-double restatement with libm's sinl / cosl; the expected peaks a
// plain scan of the map the header's functions made.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../assignment-for-aae6102_gnss-sdr_amd/csrc/replay_ddm.h"

using namespace gnss;

static int mismatches = 0;
static int cases = 0;

static void check(bool ok, const char* what, int a = 0, int b = 0)
{
    cases++;
    if (!ok) {
        mismatches++;
        std::printf("MISMATCH %s (%d, %d)\n", what, a, b);
    }
}

static uint64_t lcg = 6113;
static double next_unit()  // in [-1, 1)
{
    lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(int32_t)(lcg >> 32) / 2147483648.0;
}

// one window against the naive sums; 1e-12 of the scale R * max|term| is far above the rounding of R
// <= 100 terms and of the rotation (a few 1e-16) and far below one wrong sign or a swapped sin / cos
static void run_window(int R, int nt, int nd, int prompt, double Fs)
{
    const int64_t stride = R;  // the window is the whole series: nothing before or after it
    std::vector<double> I((size_t)nt * R), Q((size_t)nt * R), t((size_t)R), hz((size_t)nd), u((size_t)nt);
    std::vector<double> sg((size_t)R), sn((size_t)R), cs((size_t)R), zI((size_t)nd * nt, -7.0), zQ((size_t)nd * nt, -7.0);
    for (auto& v : I) v = 1000.0 * next_unit();
    for (auto& v : Q) v = 1000.0 * next_unit();
    int64_t s = 0;
    for (int i = 0; i < R; i++) {
        const int64_t n = 2047 + (i % 5);
        t[(size_t)i] = ddm_row_time(s, n, Fs);
        s += n + (i % 3);
    }
    for (int m = 0; m < nd; m++) hz[(size_t)m] = -500.0 + 37.7 * m;
    for (int j = 0; j < nt; j++) u[(size_t)j] = 0.05 * (j - nt / 2);
    ddm_window_host(I.data(), Q.data(), stride, prompt >= 0 ? I.data() + (size_t)prompt * R : nullptr, t.data(), R, nt, nd,
                    hz.data(), sg.data(), sn.data(), cs.data(), zI.data(), zQ.data());
    const long double twopi = 6.283185307179586476925286766559L;
    double worst = 0.0;
    for (int m = 0; m < nd; m++)
        for (int j = 0; j < nt; j++) {
            long double aI = 0, aQ = 0;
            for (int i = 0; i < R; i++) {
                const long double sgn = prompt < 0 || I[(size_t)prompt * R + i] >= 0 ? 1.0L : -1.0L;
                const long double ph = twopi * (long double)hz[(size_t)m] * (long double)t[(size_t)i];
                const long double c = cosl(ph), sv = sinl(ph);
                const long double vi = I[(size_t)j * R + i], vq = Q[(size_t)j * R + i];
                aI += sgn * (vi * c + vq * sv);
                aQ += sgn * (vq * c - vi * sv);
            }
            worst = std::fmax(worst, std::fabs((double)(aI - zI[(size_t)m * nt + j])));
            worst = std::fmax(worst, std::fabs((double)(aQ - zQ[(size_t)m * nt + j])));
        }
    check(worst <= 1e-12 * R * 2000.0, "cells against the naive sums", R, nt * 1000 + nd);

    // the peaks: a plain scan, strictly-greater keeps the first of equals
    for (const double ex : {0.0, 0.12, 1e9}) {
        const DdmPeaks p = ddm_peaks_host(zI.data(), zQ.data(), nd, nt, u.data(), hz.data(), ex, 40.0);
        int pk = -1, sk = -1;
        double pp = -1, sp = -1;
        for (int k = 0; k < nd * nt; k++) {
            const double P = zI[(size_t)k] * zI[(size_t)k] + zQ[(size_t)k] * zQ[(size_t)k];
            if (P > pp) pp = P, pk = k;
        }
        for (int k = 0; k < nd * nt; k++) {
            const double P = zI[(size_t)k] * zI[(size_t)k] + zQ[(size_t)k] * zQ[(size_t)k];
            const bool out = std::fabs(u[(size_t)(k % nt)] - u[(size_t)(pk % nt)]) >= ex ||
                             std::fabs(hz[(size_t)(k / nt)] - hz[(size_t)(pk / nt)]) >= 40.0;
            if (out && P > sp) sp = P, sk = k;
        }
        check(p.peak_bin == pk / nt && p.peak_tap == pk % nt && p.peak_pow == pp, "peak", R, nt);
        if (sk < 0)
            check(p.sec_bin == -1 && p.sec_tap == -1 && p.sec_pow != p.sec_pow, "no secondary peak", R, nt);
        else
            check(p.sec_bin == sk / nt && p.sec_tap == sk % nt && p.sec_pow == sp, "secondary peak", R, nt);
    }
}

int main()
{
    // the row time: the middle sample of rows of odd and even length, exactly
    check(ddm_row_time(0, 1, 1.0) == 0.0 && ddm_row_time(0, 2, 1.0) == 0.5 && ddm_row_time(10, 5, 2.0) == 6.0, "row time");
    // the rotation: whole cycles are the identity, quarter cycles exact
    double sn, cs;
    ddm_rotation(1000.0, 0.003, &sn, &cs);
    check(std::fabs(sn) < 1e-12 && std::fabs(cs - 1.0) < 1e-12, "whole cycles");
    ddm_rotation(250.0, 0.001, &sn, &cs);
    check(std::fabs(sn - 1.0) < 1e-15 && std::fabs(cs) < 1e-15, "a quarter cycle");
    ddm_rotation(-250.0, 0.001, &sn, &cs);
    check(std::fabs(sn + 1.0) < 1e-15 && std::fabs(cs) < 1e-15, "a quarter cycle back");
    // the sign rule: zero and -0 are +1, a NaN is -1
    check(ddm_sign(0.0) == 1.0 && ddm_sign(-0.0) == 1.0 && ddm_sign(-1e-300) == -1.0 && ddm_sign(std::nan("")) == -1.0, "sign");
    // a cell: (I + iQ) * (cs - i sn)
    double ZI = 1.0, ZQ = 2.0;
    ddm_cell(3.0, 4.0, 0.5, 0.25, &ZI, &ZQ);
    check(ZI == 1.0 + (3.0 * 0.25 + 4.0 * 0.5) && ZQ == 2.0 + (4.0 * 0.25 - 3.0 * 0.5), "cell");
    // the order of the peak rule: larger first, then the lower cell; a NaN and "none" never win
    DdmBest b = ddm_best_none();
    ddm_best_take(b, std::nan(""), 0);
    check(b.k == -1, "a NaN is no candidate");
    ddm_best_take(b, 0.0, 5);
    ddm_best_take(b, 0.0, 7);
    check(b.k == 5, "the first of equals");
    ddm_best_merge(b, 0.0, 3);
    check(b.k == 3, "merging takes the lower cell of equals");
    ddm_best_merge(b, 9.0, -1);
    check(b.k == 3, "merging none changes nothing");
    ddm_best_merge(b, 1.0, 100);
    check(b.k == 100 && b.pow == 1.0, "the larger power");
    const DdmPeaks none = ddm_peaks_of(ddm_best_none(), ddm_best_none(), 4);
    check(none.peak_bin == -1 && none.peak_tap == -1 && none.peak_pow != none.peak_pow && none.sec_bin == -1, "no peak");
    // an all-NaN map has no peak and no secondary peak
    {
        std::vector<double> z(6, std::nan("")), u(3, 0.0), hz(2, 0.0);
        const DdmPeaks p = ddm_peaks_host(z.data(), z.data(), 2, 3, u.data(), hz.data(), 0.0, 0.0);
        check(p.peak_bin == -1 && p.sec_tap == -1, "an all-NaN map");
    }
    for (int R : {2, 3, 31, 100})
        for (int nt : {1, 5, 61})
            for (int nd : {1, 11})
                for (int prompt : {-1, 0, nt - 1}) run_window(R, nt, nd, prompt, 58e6);
    std::printf("cases %d, mismatches %d\n", cases, mismatches);
    return mismatches ? 1 : 0;
}
