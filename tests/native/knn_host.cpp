// knn_host.cpp -- csrc/knn.h's functions (the arithmetic shared by the host path and the kernels of
// gnss_knn_classify) on the CPU: built once plainly and once under AddressSanitizer and UBSan
// (tests/test_native_knn.py). Every array is a heap array of exactly the stated size (x and z
// M * D, mu and inv D, label M, the lists k, the votes n_class), so a read or write past one is an
// error there. The expected neighbours come from a full sort of all M rows under the same order.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../assignment-for-aae6102_gnss-sdr_amd/csrc/knn.h"

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

static uint64_t lcg = 12345;
static double uniform()  // in [-1, 1)
{
    lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(int64_t)(lcg >> 11) / 4503599627370496.0 - 1.0;
}

static bool same_bits(double a, double b)
{
    return std::memcmp(&a, &b, sizeof a) == 0;
}

// one table, its model, a few queries, knn_query against the full sort
static void run_table(int64_t M, int D, int k, int n_class, bool grid)
{
    std::vector<double> x((size_t)(M * D)), z((size_t)(M * D)), mu((size_t)D), inv((size_t)D);
    std::vector<int32_t> label((size_t)M);
    for (auto& v : x) v = grid ? std::floor(uniform() * 3.0) * 0.5 : uniform();
    for (int64_t t = 0; t < M; t++) label[(size_t)t] = (int32_t)((t * 7 + 3) % n_class);
    if (M > 2) std::memcpy(&x[(size_t)((M - 1) * D)], &x[0], sizeof(double) * D);  // the last row repeats the first
    bool ok = true;
    for (int j = 0; j < D; j++) ok = ok && knn_column_stats(x.data(), M, D, j, &mu[j], &inv[j]);
    check(ok, "column stats");
    for (int64_t t = 0; t < M; t++)
        for (int j = 0; j < D; j++) z[(size_t)(t * D + j)] = knn_z(x[(size_t)(t * D + j)], mu[j], inv[j]);

    for (int qi = 0; qi < 6; qi++) {
        std::vector<double> q((size_t)D), zq((size_t)D), nn_d2((size_t)k);
        std::vector<int32_t> nn_index((size_t)k), votes((size_t)n_class);
        for (int j = 0; j < D; j++) q[j] = qi == 0 ? x[j] : grid ? std::floor(uniform() * 3.0) * 0.5 : uniform() * 1.5;
        if (qi == 5) q[D - 1] = NAN;
        const int got = knn_query(q.data(), mu.data(), inv.data(), z.data(), label.data(), M, D, k, n_class,
                                  nn_d2.data(), nn_index.data(), votes.data());
        if (qi == 5) {
            bool bad = got == -1;
            for (int i = 0; i < k; i++) bad = bad && nn_index[i] == -1 && nn_d2[i] != nn_d2[i];
            for (int c = 0; c < n_class; c++) bad = bad && votes[c] == 0;
            check(bad, "a non-finite query");
            continue;
        }
        for (int j = 0; j < D; j++) zq[j] = knn_z(q[j], mu[j], inv[j]);
        std::vector<double> d2((size_t)M);
        std::vector<int> order((size_t)M);
        for (int64_t t = 0; t < M; t++) {
            d2[(size_t)t] = knn_d2(zq.data(), &z[(size_t)(t * D)], D);
            order[(size_t)t] = (int)t;
        }
        std::sort(order.begin(), order.end(), [&](int a, int b) { return knn_before(d2[a], a, d2[b], b); });
        bool same = true;
        std::vector<int> count((size_t)n_class, 0);
        for (int i = 0; i < k; i++) {
            same = same && nn_index[i] == order[i] && same_bits(nn_d2[i], d2[order[i]]);
            count[label[order[i]]]++;
        }
        check(same, "the k nearest against the full sort");
        int most = 0, want = -1;
        for (int c = 0; c < n_class; c++) most = std::max(most, count[c]);
        for (int i = 0; i < k && want < 0; i++)
            if (count[label[order[i]]] == most) want = label[order[i]];
        bool v = got == want;
        for (int c = 0; c < n_class; c++) v = v && votes[c] == count[c];
        check(v, "the vote");
        if (qi == 0) check(nn_index[0] == 0 && nn_d2[0] == 0.0, "a training row finds itself first");
    }
}

int main()
{
    // the pieces
    check(knn_finite(1e308) && !knn_finite(INFINITY) && !knn_finite(-INFINITY) && !knn_finite(NAN), "finite");
    check(knn_before(1.0, 5, 2.0, 1) && knn_before(1.0, 1, 1.0, 5) && !knn_before(1.0, 5, 1.0, 5) &&
              !knn_before(2.0, 0, 1.0, 9),
          "order: numbers");
    check(knn_before(INFINITY, 9, NAN, 0) && !knn_before(NAN, 0, INFINITY, 9) && knn_before(NAN, 1, NAN, 2) &&
              !knn_before(NAN, 2, NAN, 1) && knn_before(1e300, 3, INFINITY, 0) && knn_before(INFINITY, 0, INFINITY, 1),
          "order: inf and NaN");
    check(knn_scan_admits(1.0, 7, 2.0, 3) && !knn_scan_admits(2.0, 7, 2.0, 3) && !knn_scan_admits(3.0, 7, 2.0, 3) &&
              knn_scan_admits(5.0, 7, knn_nan(), kKnnEmpty) && knn_scan_admits(NAN, 7, knn_nan(), kKnnEmpty) &&
              !knn_scan_admits(NAN, 7, NAN, 3) && !knn_scan_admits(NAN, 7, INFINITY, 3) &&
              knn_scan_admits(INFINITY, 7, NAN, 3),
          "scan admission");
    {
        const double n = knn_d2_close(-NAN);
        uint64_t b;
        std::memcpy(&b, &n, 8);
        check(b == 0x7ff8000000000000ull && knn_d2_close(4.0) == 4.0 && knn_d2_close(INFINITY) == INFINITY, "the one NaN");
    }
    {
        double a = knn_d2_term(99.0, 3.0, 1.0, true);
        a = knn_d2_term(a, 1.0, 4.0, false);
        check(a == 13.0, "distance terms");
    }
    {
        uint64_t v = 0;
        for (int i = 0; i < 32; i++) v = knn_vote_add(v, 7);
        v = knn_vote_add(v, 0);
        check(knn_vote_of(v, 7) == 32 && knn_vote_of(v, 0) == 1 && knn_vote_of(v, 3) == 0, "packed votes");
    }
    {
        // a constant column, a NaN value, an overflowing sum
        std::vector<double> x = {1.0, 7.0, 3.0, 7.0};
        double mu, inv;
        check(knn_column_stats(x.data(), 2, 2, 0, &mu, &inv) && mu == 2.0 && inv == 1.0, "stats: mu 2, sd 1");
        check(knn_column_stats(x.data(), 2, 2, 1, &mu, &inv) && mu == 7.0 && inv == 0.0, "stats: a constant column");
        x[2] = NAN;
        check(!knn_column_stats(x.data(), 2, 2, 0, &mu, &inv), "stats: a NaN value");
        x[0] = x[2] = 1.7e308;
        check(!knn_column_stats(x.data(), 2, 2, 0, &mu, &inv), "stats: the sum overflows");
    }
    // the split plan: whole tiles, the floor, at most kKnnMaxSplits splits, one round of the slots
    check(knn_lds_scan(11, 15) == 51712 && knn_block_slots(11, 15, 256) == 768 && knn_block_slots(16, 32, 256) == 256 &&
              knn_block_slots(1, 1, 256) == 2048,
          "block slots");
    check(knn_split_share(1, 1, 768) == kKnnShareMin && knn_split_share(65536, 257, 256) == 1024 &&
              knn_split_share(65537, 1, 256) == 1088 && knn_split_share(290880, 29088, 768) == 48512 &&
              knn_split_share(290880, 1000000, 768) == 290880,
          "split shares");
    for (int64_t M : {1, 1000, 65536, 65537, 290880, 1 << 24})
        for (int64_t Q : {1, 257, 29088, 1000000})
            for (int64_t slots : {256, 768, 2048}) {
                const int64_t s = knn_split_share(M, Q, slots), n = (M + s - 1) / s, qt = (Q + kKnnLanes - 1) / kKnnLanes;
                check(s % kKnnTile == 0 && s >= kKnnShareMin && n >= 1 && n <= kKnnMaxSplits &&
                          (n == 1 || n * qt <= slots),
                      "split plan");
            }

    // tables: M = k, k + 1 and more; D = 1, 11, 16; k = 1, 5, 32; with and without exact ties
    const int Ds[] = {1, 11, 16}, ks[] = {1, 5, 32};
    for (int D : Ds)
        for (int k : ks)
            for (int64_t M : {(int64_t)k, (int64_t)k + 1, (int64_t)300})
                for (int grid = 0; grid < 2; grid++) run_table(M, D, k, 3, grid != 0);
    run_table(40, 4, 32, 8, true);
    run_table(9, 2, 9, 1, false);

    std::printf("cases %d, mismatches %d\n", cases, mismatches);
    return mismatches != 0;
}
