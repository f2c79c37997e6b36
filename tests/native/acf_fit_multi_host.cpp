// acf_fit_multi_host.cpp -- csrc/acf_fit_multi.h's functions (the arithmetic and the order of the
// searches shared by the host path and the kernel of gnss_acf_fit_multi) on the CPU: built once
// plainly and once under AddressSanitizer and UBSan (tests/test_native_acf_fit_multi.py). The tap
// coordinates are a heap array of exactly n_taps elements, the coherent vector one of exactly
// 2 * n_taps (zI then zQ, as the kernel holds it) and the slots' r vectors one of exactly
// 4 * n_taps, so a read past a tap is an error there. The expected values come from a second,
// straightforward implementation below with run-time loops over explicit r vectors, which shares
// nothing with the header but R's formula and the definition.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../assignment-for-aae6102_gnss-sdr_amd/csrc/acf_fit_multi.h"

using namespace gnss;

static int mismatches = 0;
static int cases = 0;

static void check(bool ok, const char* what, int nt = 0, int variant = 0)
{
    cases++;
    if (!ok) {
        mismatches++;
        std::printf("MISMATCH %s (n_taps %d, variant %d)\n", what, nt, variant);
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

typedef std::vector<double> Vec;

// the joint fit of explicit r vectors, slot order; false: unusable (slot k) or singular
static bool plain_joint(const std::vector<Vec>& r, int k, const Vec& zI, const Vec& zQ, Vec& Ar, Vec& Ai, double& res)
{
    const size_t m = r.size(), n = zI.size();
    std::vector<Vec> G(m, Vec(m));
    Vec hI(m), hQ(m), g0(m);
    for (size_t a = 0; a < m; a++) {
        for (size_t b = 0; b < m; b++) {
            double s = 0;
            for (size_t j = 0; j < n; j++) s = j ? s + r[a][j] * r[b][j] : r[a][j] * r[b][j];
            G[a][b] = s;
        }
        double sI = 0, sQ = 0;
        for (size_t j = 0; j < n; j++) {
            sI = j ? sI + r[a][j] * zI[j] : r[a][j] * zI[j];
            sQ = j ? sQ + r[a][j] * zQ[j] : r[a][j] * zQ[j];
        }
        hI[a] = sI, hQ[a] = sQ, g0[a] = G[a][a];
    }
    if (g0[(size_t)k] == 0) return false;
    for (size_t e = 0; e < m; e++) {
        const double d = G[e][e];
        if (!(d > 1e-9 * g0[e])) return false;
        for (size_t i = e + 1; i < m; i++) {
            const double f = G[i][e] / d;
            for (size_t l = e + 1; l < m; l++) G[i][l] = G[i][l] - f * G[e][l];
            hI[i] = hI[i] - f * hI[e];
            hQ[i] = hQ[i] - f * hQ[e];
        }
    }
    Ar.assign(m, 0), Ai.assign(m, 0);
    for (size_t e = m; e-- > 0;) {
        double sI = hI[e], sQ = hQ[e];
        for (size_t l = e + 1; l < m; l++) {
            sI = sI - G[e][l] * Ar[l];
            sQ = sQ - G[e][l] * Ai[l];
        }
        Ar[e] = sI / G[e][e], Ai[e] = sQ / G[e][e];
    }
    res = 0;
    for (size_t j = 0; j < n; j++) {
        double dI = zI[j], dQ = zQ[j];
        for (size_t l = 0; l < m; l++) {
            dI = dI - Ar[l] * r[l][j];
            dQ = dQ - Ai[l] * r[l][j];
        }
        res = j ? res + (dI * dI + dQ * dQ) : dI * dI + dQ * dQ;
    }
    return true;
}

// the definition, search by search -> the row in AcfFmmRow's order
static void plain_fit(const AcfFmmPar& p, const Vec& u, const Vec& zI, const Vec& zQ, double* row)
{
    const size_t n = u.size();
    for (int i = 0; i < kFmmRow; i++) row[i] = NAN;
    row[0] = row[1] = 0;
    for (size_t j = 0; j < n; j++)
        if (!std::isfinite(zI[j]) || !std::isfinite(zQ[j])) return;
    auto rvec = [&](int i) {
        Vec r(n);
        const double q = p.q_min + (double)i * p.q_step;
        for (size_t j = 0; j < n; j++) r[j] = tri(u[j] - q);
        return r;
    };
    std::vector<int> pos;
    std::vector<std::vector<int>> kept;
    Vec res(1, 0.0), Ar, Ai;
    for (size_t j = 0; j < n; j++) res[0] = j ? res[0] + (zI[j] * zI[j] + zQ[j] * zQ[j]) : zI[j] * zI[j] + zQ[j] * zQ[j];
    int searches = 0;
    auto search = [&](size_t k, double& best) {  // -> the winner or -1; pos[k] moved
        std::vector<Vec> r;
        for (size_t l = 0; l < pos.size(); l++) r.push_back(l == k ? Vec() : rvec(pos[l]));
        int win = -1;
        best = INFINITY;
        for (int i = 0; i < p.q_count; i++) {
            bool close = false;
            for (size_t l = 0; l < pos.size(); l++) close = close || (l != k && std::abs(i - pos[l]) < p.sep_min);
            if (close) continue;
            r[k] = rvec(i);
            double rr;
            if (!plain_joint(r, (int)k, zI, zQ, Ar, Ai, rr)) continue;
            if (win < 0 ? rr <= INFINITY : rr < best) win = i, best = rr;
        }
        searches++;
        if (win >= 0) pos[k] = win;
        return win;
    };
    for (int m = 1; m <= p.max_paths; m++) {
        double rm, rr;
        pos.push_back(0);
        if (search((size_t)m - 1, rm) < 0) {
            pos.pop_back();
            break;
        }
        for (int s = 0; s < p.sweeps; s++) {
            bool moved = false;
            for (size_t k = 0; k < (size_t)m; k++) {
                const int before = pos[k];
                const int win = search(k, rr);
                if (win >= 0) rm = rr, moved = moved || win != before;
            }
            if (!moved) break;
        }
        kept.push_back(pos);
        res.push_back(rm);
    }
    const size_t formed = kept.size();
    size_t sel = formed ? 1 : 0;
    for (size_t m = 1; m <= formed; m++)
        if (res[m - 1] > p.gain_min * res[m]) sel = m;
    row[0] = (double)sel, row[1] = (double)searches;
    for (size_t m = 0; m <= formed; m++) row[14 + m] = res[m];
    row[19] = res[0];
    if (!sel) return;
    const std::vector<int>& at = kept[sel - 1];
    std::vector<Vec> r;
    for (size_t l = 0; l < sel; l++) r.push_back(rvec(at[l]));
    double rr;
    plain_joint(r, 0, zI, zQ, Ar, Ai, rr);
    for (size_t a = 0; a < sel; a++) {
        size_t rank = 0;
        for (size_t b = 0; b < sel; b++) rank += at[b] > at[a];
        row[2 + rank] = p.q_min + (double)at[a] * p.q_step;
        row[6 + rank] = Ar[a];
        row[10 + rank] = Ai[a];
    }
}

// a deterministic value in [-1, 1)
static double noise(unsigned& s)
{
    s = s * 1664525u + 1013904223u;
    return (double)(s >> 8) / 8388608.0 - 1.0;
}

// One tap count and one variant of the search: a coherent vector of exactly 2 * n_taps doubles
// (a direct path and two rays plus noise, summed over `rows` signed rows), the fit by the header
// with a workspace of exactly 4 * n_taps doubles, and the plain fit.
static void run(int nt, int variant, bool poison)
{
    const int rows = 9, prompt = nt - 1 - nt / 4;
    const double spacing = nt == 256 ? 0.0125 : nt == 1 ? 0.05 : 2.4 / (nt - 1);
    AcfFmmPar p{nt, prompt, -1.9, 0.03, 80, 3, 2, 5, 16.0};
    if (variant == 1) p.max_paths = 4, p.sweeps = 0, p.sep_min = 1;
    if (variant == 2) p.max_paths = 1, p.sweeps = 4, p.q_count = 1, p.q_min = 0.0;
    if (variant == 3) p.max_paths = 4, p.sweeps = 1, p.q_min = 5.0;  // every candidate outside the taps
    Vec u((size_t)nt), zs((size_t)2 * nt), rs((size_t)kFmmMaxPaths * nt);
    for (int j = 0; j < nt; j++) u[(size_t)j] = (double)(j - prompt) * spacing;
    unsigned seed = 4321u + (unsigned)nt * 11u + (unsigned)variant;
    for (int j = 0; j < nt; j++) {
        const double x = u[(size_t)j];
        const double sI = tri(x) - 0.5 * tri(x + 0.6), sQ = 0.4 * tri(x + 1.4);
        double aI = 0, aQ = 0;
        for (int r = 0; r < rows; r++) {
            const double bit = (r * 5) % 3 ? 1.0 : -1.0;
            const double s = ftt_sign(bit * 4000.0);
            aI = ftt_accum(aI, s, bit * 4000.0 * sI + 40.0 * noise(seed), r == 0);
            aQ = ftt_accum(aQ, s, bit * 4000.0 * sQ + 40.0 * noise(seed), r == 0);
        }
        zs[(size_t)j] = aI;
        zs[(size_t)(nt + j)] = aQ;
    }
    if (poison) zs[(size_t)(2 * nt - 1)] = NAN;
    const Vec zI(zs.begin(), zs.begin() + nt), zQ(zs.begin() + nt, zs.end());
    double got[kFmmRow], want[kFmmRow];
    fmm_window(p, u.data(), zs.data(), zs.data() + nt, rs.data(), got);
    plain_fit(p, u, zI, zQ, want);
    bool eq = true;
    for (int i = 0; i < kFmmRow; i++) eq = eq && same(got[i], want[i]);
    check(eq, "the fit against the plain loops", nt, variant);
    check(poison || variant == 3 ? got[0] == 0 : got[0] >= 1, "paths", nt, variant);
    // the kernel's split of a search: the sums and the candidates dealt over four workers in any
    // order, the shares merged -> the sequential search's winner
    if (!poison && variant == 0) {
        AcfFmmWork w{}, w4{};
        for (size_t i = 0; i < rs.size(); i++) rs[i] = 0;
        fmm_place(p, w, rs.data(), 0, 37, u.data(), 0, 1);
        fmm_place(p, w, rs.data(), 1, 11, u.data(), 0, 1);
        w4 = w;
        fmm_sys_fill(w, rs.data(), 3, 2, nt, zs.data(), zs.data() + nt, 0, 1);
        const AcfFttBest one = fmm_search_share(p, w, rs.data(), 3, 2, u.data(), zs.data(), zs.data() + nt, 0, 1);
        for (int lane = 3; lane >= 0; lane--) fmm_sys_fill(w4, rs.data(), 3, 2, nt, zs.data(), zs.data() + nt, lane, 4);
        AcfFttBest b = ftt_best_none();
        for (int lane = 3; lane >= 0; lane--) {
            const AcfFttBest l = fmm_search_share(p, w4, rs.data(), 3, 2, u.data(), zs.data(), zs.data() + nt, lane, 4);
            ftt_best_merge(b, l.res, l.h);
        }
        check(std::memcmp(&w.sys, &w4.sys, sizeof w.sys) == 0, "the dealt sums", nt, variant);
        check(b.h == one.h && same(b.res, one.res), "the dealt candidates", nt, variant);
    }
}

int main()
{
    const int nts[5] = {1, 2, 25, 71, 256};
    for (int k = 0; k < 5; k++)
        for (int variant = 0; variant < 4; variant++) {
            run(nts[k], variant, false);
            if (variant == 0) run(nts[k], variant, true);
        }

    // three paths on grid points of 71 taps at -2.5:0.05:1.0 come back exactly
    {
        const int nt = 71, prompt = 50;
        AcfFmmPar p{nt, prompt, -2.40, 0.01, 281, 3, 4, 5, 16.0};
        Vec u((size_t)nt), zs((size_t)2 * nt), rs((size_t)kFmmMaxPaths * nt);
        for (int j = 0; j < nt; j++) u[(size_t)j] = (double)(j - prompt) * 0.05;
        const double q0 = fmm_q(p, 240), q1 = fmm_q(p, 180), q2 = fmm_q(p, 100);
        for (int j = 0; j < nt; j++) {
            zs[(size_t)j] = 4096.0 * ftt_R(u[(size_t)j] - q0) - 2048.0 * ftt_R(u[(size_t)j] - q1);
            zs[(size_t)(nt + j)] = 1024.0 * ftt_R(u[(size_t)j] - q2);
        }
        double row[kFmmRow];
        fmm_window(p, u.data(), zs.data(), zs.data() + nt, rs.data(), row);
        check(row[0] == 3 && row[2] == q0 && row[3] == q1 && row[4] == q2 && std::isnan(row[5]), "three paths on the grid", nt);
        check(std::fabs(row[6] - 4096.0) <= 4e-6 && std::fabs(row[7] + 2048.0) <= 4e-6 && std::fabs(row[12] - 1024.0) <= 4e-6,
              "their amplitudes", nt);
    }

    std::printf("cases %d, mismatches %d\n", cases, mismatches);
    return mismatches ? 1 : 0;
}
