// acf_ext_host.cpp -- csrc/acf_ext.h's functions (the arithmetic shared by the host path and the
// kernels of gnss_acf_features_ext) on hand-made values, on the CPU: built once plainly and once
// under AddressSanitizer and UBSan (tests/test_native_acf_ext.py). The arrays are exactly as long
// as what the functions may touch -- the meanMax series ends at the last window, the history at
// H, the table at its last pair -- so a read past any of them is an error there.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../assignment-for-aae6102_gnss-sdr_amd/csrc/acf_ext.h"

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

static int count_row(const std::vector<double>& v)
{
    AcfMlc s;
    for (double x : v) acf_mlc_take(s, x);
    return s.cnt;
}

static std::vector<double> table(int N)
{
    std::vector<double> tw((size_t)2 * N);
    for (int t = 0; t < N; t++) {
        const double a = (2.0 * 3.141592653589793238 * (double)t) / (double)N;
        tw[2 * t] = std::cos(a);
        tw[2 * t + 1] = std::sin(a);
    }
    return tw;
}

// the window's spectrum as the host path forms it: exact-size history, every bin 0 .. N / 2
static AcfExtBest window_best(const std::vector<double>& meanMax, int64_t m, int hist, int fill,
                              const std::vector<double>& tw, int N)
{
    const int H = acf_ext_len(m, hist, fill);
    std::vector<double> y((size_t)H);
    for (int i = 0; i < H; i++) y[i] = acf_ext_hist(meanMax.data(), m, H, i);
    const double mean = acf_ext_mean(y.data(), H);
    for (int i = 0; i < H; i++) y[i] = y[i] - mean;
    AcfExtBest b;
    for (int k = 0; k <= N / 2; k++) acf_ext_take(b, acf_ext_bin(y.data(), H, tw.data(), k, N), k);
    return b;
}

int main()
{
    // the local-maximum count
    std::vector<double> v(25, 1.0);
    check(count_row(v) == 0, "a flat row");
    v[12] = 9;
    check(count_row(v) == 1, "a single peak");
    v[4] = 4;
    check(count_row(v) == 2, "two interior peaks");
    v[11] = NAN;
    check(count_row(v) == 1, "a NaN neighbour");
    v.assign(25, 1.0);
    v[0] = 9, v[24] = 9;
    check(count_row(v) == 0, "peaks on the edge columns");
    v[1] = 10, v[23] = 10;
    check(count_row(v) == 2, "columns 2 and 24 can count");
    v.assign(25, 1.0);
    v[6] = 5, v[7] = 5;
    check(count_row(v) == 0, "a plateau of two");
    for (int j = 0; j < 25; j++) v[j] = j % 2 ? 2.0 : 1.0;
    check(count_row(v) == 12, "every second column");
    v.assign(25, NAN);
    check(count_row(v) == 0, "an all-NaN row");

    // the history
    check(acf_ext_len(0, 300, 0) == 300 && acf_ext_len(0, 300, 1) == 1 && acf_ext_len(298, 300, 1) == 299 &&
              acf_ext_len(299, 300, 1) == 300 && acf_ext_len(5000, 300, 1) == 300,
          "H");
    const std::vector<double> mm = {3, 4, 5};  // ends at window 2
    check(acf_ext_hist(mm.data(), 2, 5, 0) == 0 && acf_ext_hist(mm.data(), 2, 5, 1) == 0 &&
              acf_ext_hist(mm.data(), 2, 5, 2) == 3 && acf_ext_hist(mm.data(), 2, 5, 4) == 5,
          "zero fill before the first window");
    check(acf_ext_hist(mm.data(), 2, 2, 0) == 4 && acf_ext_hist(mm.data(), 2, 2, 1) == 5, "the last two");
    check(acf_ext_mean(mm.data(), 3) == 4.0 && acf_ext_mean(mm.data(), 1) == 3.0, "mean");

    // a cosine over H = N = 64 windows comes back at its bin; the series ends at the last window
    const int N = 64;
    const std::vector<double> tw = table(N);
    for (int k0 : {1, 5, 31}) {
        std::vector<double> s((size_t)N);
        for (int i = 0; i < N; i++) s[i] = 3000.0 + 1000.0 * tw[2 * ((k0 * i) % N)];
        const AcfExtBest b = window_best(s, N - 1, N, 0, tw, N);
        const AcfExtRow r = acf_ext_row(128, 64, b, 25.0, N);
        check(b.k == k0 && r.fftFreq == (k0 * 25.0) / N && std::fabs(r.fftMag - 1000.0) <= 1e-9, "cosine");
        check(r.numMLC == 2.0, "numMLC");
        // the same with fewer windows than the history, both fill modes
        s.resize(10);
        const AcfExtBest z = window_best(s, 9, N, 0, tw, N), f = window_best(s, 9, N, 1, tw, N);
        check(z.mag > 0 && f.mag > 0 && z.k <= N / 2 && f.k <= N / 2, "short series");
    }
    // N not a power of two, N = H = 3, and the narrowest N = H = 2 (bins 0 and 1)
    {
        const std::vector<double> t3 = table(3), t2 = table(2), t1000 = table(1000);
        const std::vector<double> s = {1, 5, 2, 8, 3};
        const AcfExtBest a = window_best(s, 4, 3, 0, t3, 3), b = window_best(s, 4, 2, 0, t2, 2);
        check(a.k == 1 && b.k == 1 && b.mag == 5.0, "N = 3 and N = 2");
        const AcfExtBest c = window_best(s, 4, 5, 1, t1000, 1000);
        check(c.k >= 0 && c.k <= 500 && c.mag > 0, "N = 1000");
    }
    // a constant history: every bin 0, the first taken; a NaN in it: none taken
    {
        const std::vector<double> s(8, 37.5);
        const AcfExtBest b = window_best(s, 7, 5, 0, tw, N);
        const AcfExtRow r = acf_ext_row(0, 2, b, 10.0, N);
        check(b.k == 0 && b.mag == 0.0 && r.fftFreq == 0.0 && r.fftMag == 0.0 && r.numMLC == 0.0, "constant");
        std::vector<double> n = s;
        n[6] = NAN;
        const AcfExtBest x = window_best(n, 7, 5, 0, tw, N);
        const AcfExtRow q = acf_ext_row(3, 2, x, 10.0, N);
        check(x.mag < 0 && q.fftFreq == 0.0 && std::isnan(q.fftMag) && q.numMLC == 1.5, "all bins NaN: I = 1, M = NaN");
    }
    // the order of (mag, k): the larger magnitude, then the lower bin, whatever the order of merging
    {
        AcfExtBest a, b;
        acf_ext_merge(a, 2.0, 7), acf_ext_merge(a, 2.0, 3), acf_ext_merge(a, 1.0, 0), acf_ext_merge(a, -1.0, 0);
        acf_ext_merge(b, -1.0, 0), acf_ext_merge(b, 1.0, 0), acf_ext_merge(b, 2.0, 3), acf_ext_merge(b, 2.0, 7);
        check(a.mag == 2.0 && a.k == 3 && b.mag == 2.0 && b.k == 3, "merge");
        AcfExtBest c;
        acf_ext_take(c, NAN, 0), acf_ext_take(c, 0.0, 1), acf_ext_take(c, 0.0, 2);
        check(c.mag == 0.0 && c.k == 1, "take: the first of equals, a NaN is missing");
    }

    std::printf("cases %d, mismatches %d\n", cases, mismatches);
    return mismatches ? 1 : 0;
}
