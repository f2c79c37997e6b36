// acf_fit_taps_host.cpp -- csrc/acf_fit_taps.h's functions (the arithmetic shared by the host path
// and the kernel of gnss_acf_fit_taps) on the CPU: built once plainly and once under
// AddressSanitizer and UBSan (tests/test_native_acf_fit_taps.py). The tap coordinates are a heap
// array of exactly n_taps elements and the coherent vector one of exactly 2 * n_taps (zI then zQ,
// as the kernel holds it), so a read past a tap is an error there. The expected values come from
// a second, straightforward loop below that shares nothing with the header but R's formula.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../assignment-for-aae6102_gnss-sdr_amd/csrc/acf_fit_taps.h"

using namespace gnss;

static int mismatches = 0;
static int cases = 0;

static void check(bool ok, const char* what, int nt = 0, int prompt = 0)
{
    cases++;
    if (!ok) {
        mismatches++;
        std::printf("MISMATCH %s (n_taps %d, prompt %d)\n", what, nt, prompt);
    }
}

static bool same(double a, double b)
{
    return (std::isnan(a) && std::isnan(b)) || std::memcmp(&a, &b, sizeof a) == 0;
}

static double tri(double x)
{
    const double t = 1.0 - std::fabs(x);
    return t > 0 ? t : 0.0;
}

// the definition, hypothesis by hypothesis, with the taps' R values in arrays of their own
struct Plain {
    double paths, bias, p1, A1p_re, A1p_im, res1, p0, e, A0_re, A0_im, A1_re, A1_im, res2, energy;
};
static Plain plain_fit(const AcfFttGrid& g, const std::vector<double>& u, const std::vector<double>& zI,
                       const std::vector<double>& zQ)
{
    const int n = g.n_taps;
    const double nan = NAN;
    Plain o{0, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan};
    for (int j = 0; j < n; j++)
        if (!std::isfinite(zI[j]) || !std::isfinite(zQ[j])) return o;
    std::vector<double> r0((size_t)n), r1((size_t)n);
    bool have1 = false, have2 = false;
    for (int ip = 0; ip < g.p_count; ip++) {
        const double p = g.p_min + (double)ip * g.p_step;
        double a = 0, hI = 0, hQ = 0;
        for (int j = 0; j < n; j++) {
            r0[(size_t)j] = tri(u[(size_t)j] - p);
            a = j ? a + r0[(size_t)j] * r0[(size_t)j] : r0[(size_t)j] * r0[(size_t)j];
            hI = j ? hI + r0[(size_t)j] * zI[(size_t)j] : r0[(size_t)j] * zI[(size_t)j];
            hQ = j ? hQ + r0[(size_t)j] * zQ[(size_t)j] : r0[(size_t)j] * zQ[(size_t)j];
        }
        if (a == 0) continue;
        const double Ar = hI / a, Ai = hQ / a;
        double res = 0;
        for (int j = 0; j < n; j++) {
            const double dI = zI[(size_t)j] - Ar * r0[(size_t)j], dQ = zQ[(size_t)j] - Ai * r0[(size_t)j];
            res = j ? res + (dI * dI + dQ * dQ) : dI * dI + dQ * dQ;
        }
        if (!have1 ? res <= INFINITY : res < o.res1) {
            have1 = true;
            o.p1 = p, o.A1p_re = Ar, o.A1p_im = Ai, o.res1 = res;
        }
    }
    if (!have1) return Plain{0, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan};
    for (int ip = 0; ip < g.p_count; ip++)
        for (int ie = 0; ie < g.e_count; ie++) {
            const double p = g.p_min + (double)ip * g.p_step, e = g.e_min + (double)ie * g.e_step, q = p - e;
            double a = 0, b = 0, c = 0, h0I = 0, h0Q = 0, h1I = 0, h1Q = 0;
            for (int j = 0; j < n; j++) {
                const size_t k = (size_t)j;
                r0[k] = tri(u[k] - p);
                r1[k] = tri(u[k] - q);
                a = j ? a + r0[k] * r0[k] : r0[k] * r0[k];
                b = j ? b + r1[k] * r1[k] : r1[k] * r1[k];
                c = j ? c + r0[k] * r1[k] : r0[k] * r1[k];
                h0I = j ? h0I + r0[k] * zI[k] : r0[k] * zI[k];
                h0Q = j ? h0Q + r0[k] * zQ[k] : r0[k] * zQ[k];
                h1I = j ? h1I + r1[k] * zI[k] : r1[k] * zI[k];
                h1Q = j ? h1Q + r1[k] * zQ[k] : r1[k] * zQ[k];
            }
            const double det = a * b - c * c;
            if (a == 0 || b == 0 || !(det > (1e-9 * a) * b)) continue;
            const double A0r = (b * h0I - c * h1I) / det, A0i = (b * h0Q - c * h1Q) / det;
            const double A1r = (a * h1I - c * h0I) / det, A1i = (a * h1Q - c * h0Q) / det;
            if (A1r * A1r + A1i * A1i > (g.ratio_max * g.ratio_max) * (A0r * A0r + A0i * A0i)) continue;
            double res = 0;
            for (int j = 0; j < n; j++) {
                const size_t k = (size_t)j;
                const double dI = (zI[k] - A0r * r0[k]) - A1r * r1[k], dQ = (zQ[k] - A0i * r0[k]) - A1i * r1[k];
                res = j ? res + (dI * dI + dQ * dQ) : dI * dI + dQ * dQ;
            }
            if (!have2 ? res <= INFINITY : res < o.res2) {
                have2 = true;
                o.p0 = p, o.e = e, o.A0_re = A0r, o.A0_im = A0i, o.A1_re = A1r, o.A1_im = A1i, o.res2 = res;
            }
        }
    double en = 0;
    for (int j = 0; j < n; j++) {
        const double t = zI[(size_t)j] * zI[(size_t)j] + zQ[(size_t)j] * zQ[(size_t)j];
        en = j ? en + t : t;
    }
    o.energy = en;
    o.paths = have2 && o.res1 > g.gain_min * o.res2 ? 2 : 1;
    o.bias = o.paths == 2 ? o.p0 : o.p1;
    return o;
}

static bool rows_equal(const AcfFttRow& a, const Plain& b)
{
    return same(a.paths, b.paths) && same(a.bias, b.bias) && same(a.p1, b.p1) && same(a.A1p_re, b.A1p_re) &&
           same(a.A1p_im, b.A1p_im) && same(a.res1, b.res1) && same(a.p0, b.p0) && same(a.e, b.e) &&
           same(a.A0_re, b.A0_re) && same(a.A0_im, b.A0_im) && same(a.A1_re, b.A1_re) && same(a.A1_im, b.A1_im) &&
           same(a.res2, b.res2) && same(a.energy, b.energy);
}

// a deterministic value in [-1, 1)
static double noise(unsigned& s)
{
    s = s * 1664525u + 1013904223u;
    return (double)(s >> 8) / 8388608.0 - 1.0;
}

// One tap count and prompt position: sums of `rows` rows in [2][n_taps][rows], exactly that long;
// the coherent vector through ftt_sign / ftt_accum into exactly 2 * n_taps doubles; the fit.
static void run(int nt, int prompt, double spacing, bool poison)
{
    const int rows = 37;
    AcfFttGrid g{nt, prompt, -0.2, 0.05, 0.1, 0.15, 9, 14, 1.0, 16.0};
    std::vector<double> u((size_t)nt);
    for (int j = 0; j < nt; j++) u[(size_t)j] = (double)(j - prompt) * spacing;
    std::vector<double> taps((size_t)2 * nt * rows);
    unsigned seed = 12345u + (unsigned)nt * 7u + (unsigned)prompt;
    for (int r = 0; r < rows; r++) {
        const double bit = (r * 5) % 3 ? 1.0 : -1.0;
        for (int j = 0; j < nt; j++) {
            const double shape = j == prompt ? 1.0 : tri(u[(size_t)j] - 0.05) + 0.5 * tri(u[(size_t)j] + 0.4);
            taps[((size_t)j) * rows + (size_t)r] = bit * 4000.0 * shape + 40.0 * noise(seed);
            taps[((size_t)(nt + j)) * rows + (size_t)r] = bit * 900.0 * shape + 40.0 * noise(seed);
        }
    }
    if (poison) taps[((size_t)(2 * nt - 1)) * rows + 11] = NAN;
    std::vector<double> zs((size_t)2 * nt);
    for (int s = 0; s < 2 * nt; s++) {
        double acc = 0;
        for (int r = 0; r < rows; r++)
            acc = ftt_accum(acc, ftt_sign(taps[(size_t)prompt * rows + (size_t)r]), taps[(size_t)s * rows + (size_t)r], r == 0);
        zs[(size_t)s] = acc;
    }
    // the plain sums: sign times value, added in row order
    std::vector<double> eI((size_t)nt), eQ((size_t)nt);
    for (int j = 0; j < nt; j++)
        for (int r = 0; r < rows; r++) {
            const double sg = taps[(size_t)prompt * rows + (size_t)r] >= 0 ? 1.0 : -1.0;
            const double tI = sg * taps[(size_t)j * rows + (size_t)r], tQ = sg * taps[(size_t)(nt + j) * rows + (size_t)r];
            eI[(size_t)j] = r ? eI[(size_t)j] + tI : tI;
            eQ[(size_t)j] = r ? eQ[(size_t)j] + tQ : tQ;
        }
    bool zok = true;
    for (int j = 0; j < nt; j++) zok = zok && same(zs[(size_t)j], eI[(size_t)j]) && same(zs[(size_t)(nt + j)], eQ[(size_t)j]);
    check(zok, "coherent sums", nt, prompt);
    const AcfFttRow o = ftt_window(g, u.data(), zs.data(), zs.data() + nt);
    const Plain e = plain_fit(g, u, eI, eQ);
    check(rows_equal(o, e), "the fit against the plain loops", nt, prompt);
    check(poison ? o.paths == 0 : o.paths >= 1, "paths", nt, prompt);
    // the kernel's split: each grid's best over interleaved shares, merged, then ftt_select
    AcfFttBest b1 = ftt_best_none(), b2 = ftt_best_none();
    if (ftt_all_finite(nt, zs.data(), zs.data() + nt))
        for (int lane = 3; lane >= 0; lane--) {
            AcfFttBest l1 = ftt_best_none(), l2 = ftt_best_none();
            for (int ip = lane; ip < g.p_count; ip += 4)
                ftt_best_take(l1, ftt_one(nt, u.data(), zs.data(), zs.data() + nt, ftt_p(g, ip)), ip);
            for (int h = lane; h < g.p_count * g.e_count; h += 4)
                ftt_best_take(l2, ftt_two_at(g, u.data(), zs.data(), zs.data() + nt, h), h);
            ftt_best_merge(b1, l1.res, l1.h);
            ftt_best_merge(b2, l2.res, l2.h);
        }
    const AcfFttRow k = ftt_select(g, u.data(), zs.data(), zs.data() + nt, b1.h, b2.h);
    check(std::memcmp(&k, &o, sizeof k) == 0 || (poison && k.paths == 0 && o.paths == 0), "the dealt grids", nt, prompt);
}

int main()
{
    // the pieces
    check(ftt_sign(0.0) == 1.0 && ftt_sign(-0.0) == 1.0 && ftt_sign(-1e-300) == -1.0 && ftt_sign(NAN) == -1.0, "sign");
    check(ftt_R(0) == 1 && ftt_R(0.25) == 0.75 && ftt_R(-0.25) == 0.75 && ftt_R(1) == 0 && ftt_R(-7) == 0, "R");
    check(ftt_finite(1e308) && !ftt_finite(INFINITY) && !ftt_finite(-INFINITY) && !ftt_finite(NAN), "finite");
    check(ftt_better(1.0, 5, 2.0, 1) && ftt_better(1.0, 1, 1.0, 5) && !ftt_better(1.0, 5, 1.0, 5) &&
              !ftt_better(NAN, 0, INFINITY, kFttNone) && ftt_better(INFINITY, 3, INFINITY, kFttNone),
          "lexicographic order");
    check(ftt_windows(101, 1, 100) == 1 && ftt_windows(100, 1, 100) == 0 && ftt_windows(0, 1, 100) == 0 &&
              ftt_window_row(2, 7, 64) == 134,
          "windows");

    // n_taps 1, 25 and 256 (a coarse grid: the span stays a few chips), the prompt at both ends
    // and inside, and a NaN in the last series' sums
    const int nts[3] = {1, 25, 256};
    for (int k = 0; k < 3; k++) {
        const int nt = nts[k];
        const double spacing = nt == 256 ? 0.0125 : 0.05;
        run(nt, 0, spacing, false);
        run(nt, nt - 1, spacing, false);
        run(nt, nt / 2, spacing, false);
        run(nt, nt - 1, spacing, true);
    }

    // a model vector on grid points of 71 taps at -2.5:0.05:1.0: e = 1.7 is found exactly
    {
        const int nt = 71, prompt = 50;
        AcfFttGrid g{nt, prompt, -0.40, 0.01, 0.05, 0.01, 81, 196, 1.0, 16.0};
        std::vector<double> u((size_t)nt), zs((size_t)2 * nt);
        for (int j = 0; j < nt; j++) u[(size_t)j] = (double)(j - prompt) * 0.05;
        const double p = ftt_p(g, 47), e = ftt_e(g, 165);
        for (int j = 0; j < nt; j++) {
            zs[(size_t)j] = 4096.0 * ftt_R(u[(size_t)j] - p);
            zs[(size_t)(nt + j)] = 2048.0 * ftt_R(u[(size_t)j] - (p - e));
        }
        const AcfFttRow o = ftt_window(g, u.data(), zs.data(), zs.data() + nt);
        check(o.paths == 2 && o.p0 == p && o.e == e && o.bias == p, "a ray 1.7 chips late", nt, prompt);
        check(std::fabs(o.A0_re - 4096.0) <= 4e-9 && std::fabs(o.A1_im - 2048.0) <= 4e-9 && std::fabs(o.A0_im) <= 4e-9 &&
                  std::fabs(o.A1_re) <= 4e-9,
              "its amplitudes", nt, prompt);
    }

    std::printf("cases %d, mismatches %d\n", cases, mismatches);
    return mismatches ? 1 : 0;
}
