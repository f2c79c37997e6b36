// acf_fit_host.cpp -- csrc/acf_fit.h's functions (the arithmetic of gnss_acf_fit's kernel; the host
// path runs csrc/acf_fit_taps.h's twins of them, which tests/native/acf_fit_taps_host.cpp covers)
// on the CPU: built once plainly and once under AddressSanitizer and UBSan
// (tests/test_native_acf_fit.py). The vectors are heap arrays of exactly 25 elements, so a read
// past a tap is an error there.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../assignment-for-aae6102_gnss-sdr_amd/csrc/acf_fit.h"

using namespace gnss;

static int mismatches = 0;
static int cases = 0;

static void check(bool ok, const char* what)
{
    cases++;
    if (!ok) {
        mismatches++;
        std::printf("MISMATCH %s\n", what);
    }
}

static AcfFitGrid defaults()
{
    return AcfFitGrid{1.0, 0.05, -0.40, 0.01, 0.05, 0.01, 81, 96, 1.0, 16.0};
}

// z[j] = A0 R(u[j] - p) + A1 R(u[j] - (p - e)) per component
static void model(const AcfFitGrid& g, double p, double e, double a0r, double a0i, double a1r, double a1i,
                  std::vector<double>& zI, std::vector<double>& zQ)
{
    zI.assign(kFitTaps, 0.0);
    zQ.assign(kFitTaps, 0.0);
    for (int j = 0; j < kFitTaps; j++) {
        const double r0 = fit_R(fit_u(g, j) - p), r1 = fit_R(fit_u(g, j) - (p - e));
        zI[j] = a0r * r0 + a1r * r1;
        zQ[j] = a0i * r0 + a1i * r1;
    }
}

int main()
{
    const AcfFitGrid g = defaults();
    std::vector<double> zI, zQ;

    // the pieces
    check(fit_sign(0.0) == 1.0 && fit_sign(-0.0) == 1.0 && fit_sign(-1e-300) == -1.0 && fit_sign(NAN) == -1.0, "sign");
    check(fit_R(0) == 1 && fit_R(0.25) == 0.75 && fit_R(-0.25) == 0.75 && fit_R(1) == 0 && fit_R(-7) == 0, "R");
    check(fit_u(g, 12) == 0 && fit_u(g, 0) == -12 * 0.05 && fit_u(g, 24) == 12 * 0.05, "u");
    check(fit_p(g, 0) == -0.40 && fit_e(g, 95) == 0.05 + 95 * 0.01, "grid");
    check(fit_finite(1e308) && !fit_finite(INFINITY) && !fit_finite(-INFINITY) && !fit_finite(NAN), "finite");
    check(fit_better(1.0, 5, 2.0, 1) && fit_better(1.0, 1, 1.0, 5) && !fit_better(1.0, 5, 1.0, 5) &&
              !fit_better(NAN, 0, INFINITY, kFitNone) && fit_better(INFINITY, 3, INFINITY, kFitNone),
          "lexicographic order");
    double acc = fit_accum(123.0, -1.0, 2.0, true);
    acc = fit_accum(acc, 1.0, 0.5, false);
    check(acc == -1.5, "coherent sum");

    // a two-path vector on grid points, the reflected path in phase, opposed and in quadrature
    const int ip = 56, ie = 45;
    const double p = fit_p(g, ip), e = fit_e(g, ie);
    const double ph[3][2] = {{1, 0}, {-1, 0}, {0, 1}};
    for (int k = 0; k < 3; k++) {
        const double a1r = 0.5 * 3000.0 * ph[k][0], a1i = 0.5 * 3000.0 * ph[k][1];
        model(g, p, e, 3000.0, 0.0, a1r, a1i, zI, zQ);
        const AcfFitRow o = fit_window(g, zI.data(), zQ.data());
        check(o.paths == 2 && o.p0 == p && o.e == e && o.bias == p, "two paths: the grid point");
        check(std::fabs(o.A0_re - 3000.0) <= 3e-9 && std::fabs(o.A0_im) <= 3e-9 && std::fabs(o.A1_re - a1r) <= 3e-9 &&
                  std::fabs(o.A1_im - a1i) <= 3e-9,
              "two paths: the amplitudes");
        check(o.res2 <= 1e-24 * o.energy && o.res1 > 16.0 * o.res2, "two paths: the residuals");
    }

    // one path, exact, then with about 1 % of deterministic clutter per tap: the two-path fit does
    // not do better by gain_min
    model(g, fit_p(g, 30), 0.5, 2000.0, -1000.0, 0, 0, zI, zQ);
    {
        const AcfFitRow o = fit_window(g, zI.data(), zQ.data());
        check(o.p1 == fit_p(g, 30) && std::fabs(o.A1p_re - 2000.0) <= 3e-9 && std::fabs(o.A1p_im + 1000.0) <= 3e-9 &&
                  o.res1 <= 1e-24 * o.energy,
              "one path: exact");
        for (int j = 0; j < kFitTaps; j++) {
            zI[j] += 20.0 * (double)((j * 7) % 5 - 2);
            zQ[j] += 20.0 * (double)((j * 3) % 5 - 2);
        }
        const AcfFitRow n = fit_window(g, zI.data(), zQ.data());
        check(n.paths == 1 && n.bias == n.p1 && std::fabs(n.p1 - fit_p(g, 30)) <= 0.0100001, "one path: selected");
    }

    // all zero: the first hypothesis of each grid, residuals 0
    zI.assign(kFitTaps, 0.0);
    zQ.assign(kFitTaps, 0.0);
    {
        const AcfFitRow o = fit_window(g, zI.data(), zQ.data());
        check(o.paths == 1 && o.p1 == g.p_min && o.res1 == 0 && o.res2 == 0 && o.p0 == g.p_min && o.e == g.e_min &&
                  o.energy == 0,
              "all zero");
    }

    // a non-finite tap: no fit
    zQ[24] = NAN;
    {
        const AcfFitRow o = fit_window(g, zI.data(), zQ.data());
        check(o.paths == 0 && std::isnan(o.bias) && std::isnan(o.p1) && std::isnan(o.res2) && std::isnan(o.energy),
              "a NaN tap");
    }
    zQ[24] = 0;

    // every two-path hypothesis skipped (the second path beyond the taps); a one-hypothesis grid
    AcfFitGrid far = g;
    far.e_min = 3.0;
    far.e_count = 2;
    model(g, 0.0, 0.5, 1000.0, 0, 0, 0, zI, zQ);
    {
        const AcfFitRow o = fit_window(far, zI.data(), zQ.data());
        check(o.paths == 1 && o.p1 == 0.0 && std::isnan(o.p0) && std::isnan(o.res2), "no two-path hypothesis");
        AcfFitGrid one = g;
        one.p_count = one.e_count = 1;
        const AcfFitRow q = fit_window(one, zI.data(), zQ.data());
        check(q.p1 == g.p_min && q.p0 == g.p_min && q.e == g.e_min && q.paths >= 1, "a 1 x 1 grid");
        AcfFitGrid off = g;  // no tap inside any triangle: no one-path hypothesis either
        off.p_min = 5.0;
        check(fit_window(off, zI.data(), zQ.data()).paths == 0, "a grid beyond the taps");
    }

    // the reflected path never above ratio_max times the direct one
    model(g, p, e, 1000.0, 0, 2000.0, 0, zI, zQ);
    {
        const AcfFitRow o = fit_window(g, zI.data(), zQ.data());
        const double m0 = o.A0_re * o.A0_re + o.A0_im * o.A0_im, m1 = o.A1_re * o.A1_re + o.A1_im * o.A1_im;
        check(std::isnan(o.res2) || m1 <= m0, "ratio_max = 1");
        AcfFitGrid wide = g;
        wide.ratio_max = 10.0;
        const AcfFitRow w = fit_window(wide, zI.data(), zQ.data());
        check(w.paths == 2 && w.p0 == p && w.e == e && std::fabs(w.A1_re - 2000.0) <= 3e-9, "ratio_max = 10");
    }

    // the other orientation mirrors the taps
    AcfFitGrid rev = g;
    rev.orient = -1.0;
    model(rev, p, e, 3000.0, 0.0, 0.0, 1500.0, zI, zQ);
    {
        const AcfFitRow o = fit_window(rev, zI.data(), zQ.data());
        check(o.paths == 2 && o.p0 == p && o.e == e, "orient = -1");
    }

    std::printf("cases %d, mismatches %d\n", cases, mismatches);
    return mismatches ? 1 : 0;
}
