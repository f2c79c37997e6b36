// acf_host.cpp -- csrc/acf.h's functions (the arithmetic shared by the host path and the kernels
// of gnss_acf_features) on a hand-made record, on the CPU: built once plainly and once under
// AddressSanitizer and UBSan (tests/test_native_acf.py). The arrays are exactly as long as the
// rows the functions may touch, so a read past a window or a row is an error there.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../assignment-for-aae6102_gnss-sdr_amd/csrc/acf.h"

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

// the row pass of one record row: 25 (I, Q) pairs -> index, prompt magnitude
static int row_index(const std::vector<double>& I, const std::vector<double>& Q, double* prompt)
{
    AcfPeak p;
    for (int j = 0; j < kAcfTaps; j++) {
        const double m = acf_mag(I[j], Q[j]);
        acf_peak_take(p, m, j + 1);
        if (j == kAcfPrompt) *prompt = m;
    }
    return p.idx;
}

int main()
{
    double pr = 0;
    std::vector<double> I(kAcfTaps, 1.0), Q(kAcfTaps, 1.0);
    // exact ties: (3,4), (5,0), (4,3) at columns 1 / 13 / 25
    I[0] = 3, Q[0] = 4, I[12] = 5, Q[12] = 0, I[24] = 4, Q[24] = 3;
    check(acf_mag(3, 4) == 5.0 && acf_mag(5, 0) == 5.0 && acf_mag(4, 3) == 5.0, "3-4-5");
    check(row_index(I, Q, &pr) == 1 && pr == 5.0, "tie 1/13/25 -> 1");
    I[0] = 1, Q[0] = 1;
    check(row_index(I, Q, &pr) == 13, "tie 13/25 -> 13");
    I[12] = 1, Q[12] = 1;
    check(row_index(I, Q, &pr) == 25 && pr == std::sqrt(2.0), "peak at 25");
    I[4] = NAN, Q[4] = 50;
    check(row_index(I, Q, &pr) == 25, "a NaN tap is missing");
    for (int j = 0; j < kAcfTaps; j++) I[j] = NAN;
    check(row_index(I, Q, &pr) == 1 && std::isnan(pr), "an all-NaN row gives 1");

    // the parameters
    const double cs = 0.05, cen = acf_cen_delay(0.6, cs);
    check(cen == 12.999999999999998, "cenDelay");
    check(acf_windows(1000, 1, 100) == 9 && acf_windows(1001, 1, 100) == 10 && acf_windows(100, 1, 100) == 0 &&
              acf_windows(0, 1, 100) == 0 && acf_windows(3, 7, 2) == 0 && acf_windows(107, 7, 100) == 1,
          "window count");
    check(acf_window_row(0, 1, 100) == 0 && acf_window_row(2, 7, 64) == 134, "window row");

    // three windows of a record of exactly ind_start - 1 + 3 N rows: the last window ends at the
    // arrays' end
    const int64_t N = 100, start = 7, W = 3, L = start - 1 + W * N;
    std::vector<double> pm((size_t)L), d((size_t)L);
    std::vector<uint8_t> idx((size_t)L);
    for (int64_t i = 0; i < L; i++) {
        pm[i] = 100.0 + (double)(i % 7);
        d[i] = 0.25 * (double)((i * 5) % 11) - 1.0;
        idx[i] = 13;
    }
    for (int64_t m = 0; m < W; m++) {
        const int64_t r = acf_window_row(m, start, N);
        const AcfWindow w = acf_window(&pm[r], &idx[r], &d[r], N, m == 0, cs, cen);
        // (the sum of 100 terms of 8.881784197001253e-17 rounds on the way: ...236e-17)
        check(-(w.meanDelay + 0.00) * 1 == -8.881784197001236e-17, "prompt peak: F2 over 100 rows");
        double s = 0, sd = 0;
        for (int64_t n = 0; n < N; n++) s += pm[r + n], sd += d[r + n];
        check(w.meanMax == s / 100 && w.meanCodeDisc == sd / 100, "means");
        double ss = 0;
        for (int64_t n = 0; n < N; n++) ss += (d[r + n] - sd / 100) * (d[r + n] - sd / 100);
        check(w.varCodeDisc == ss / 99, "var");
        if (m == 0) {
            check(w.varDelay == 0.0, "window 1: the running mean of a constant index");
        } else {
            double v = 0;
            for (int64_t n = 1; n <= N; n++) {
                const double t = (13.0 - (double)(13 * n) / 100.0) * cs;
                v += t * t;
            }
            check(w.varDelay == v / 100, "later windows: the zero-filled row");
        }
    }
    // the narrowest window
    const uint8_t two[2] = {25, 1};
    const double p2[2] = {3, 4}, d2[2] = {1, -1};
    const AcfWindow a = acf_window(p2, two, d2, 2, true, cs, cen);
    check(a.meanMax == 3.5 && a.meanCodeDisc == 0 && a.varCodeDisc == 2.0, "N = 2");
    const uint8_t on[2] = {13, 13};  // a prompt peak where the sum is exact: F2 = -(13 - cenDelay) * 0.05
    check(-(acf_window(p2, on, d2, 2, false, cs, cen).meanDelay + 0.00) * 1 == -8.881784197001253e-17,
          "prompt peak: F2 over 2 rows");
    check(a.varDelay == ((1 - 13.0) * cs) * ((1 - 13.0) * cs) / 2, "N = 2 first window");
    const AcfWindow b = acf_window(p2, two, d2, 2, false, cs, cen);
    check(b.varDelay == (((25 - 12.5) * cs) * ((25 - 12.5) * cs) + ((1 - 13.0) * cs) * ((1 - 13.0) * cs)) / 2,
          "N = 2 later window");

    std::printf("cases %d, mismatches %d\n", cases, mismatches);
    return mismatches ? 1 : 0;
}
