// acf_fit_multi.h — the multi-ray fit of an ACF on any tap grid (gnss_acf_fit_multi; the definition
// is in include/gnss_mi355x.h): up to four triangles fitted by alternating projection, a path's
// position searched on a 1-D grid while the others stay, the amplitudes of all paths solved jointly
// for every candidate. The windows, the rows' signs, the coherent sums and the energy are
// acf_fit_taps.h's (ftt_*); this file adds the joint fit, the search, the orders and the selection.
// One source for the arithmetic and for the order of the searches, called by the host path
// (acf_fit_multi.cpp), by the kernel (acf_fit_multi.hip) and by tests/native/acf_fit_multi_host.cpp,
// compiled without contraction and without fast-math on every side. No HIP include and no project
// include beyond acf_fit_taps.h.
//
// The joint fit of the ordered slots 0..m-1 (fmm_try<M>), operation for operation; every sum runs
// over all n taps, j ascending, from its first term (s = j ? s + t : t):
//   r_l[j]  = R(u[j] - q_l)
//   G[a][b] = sum_j r_a[j] * r_b[j]      (G[b][a] is the same sum: the products commute)
//   hI[a]   = sum_j r_a[j] * zI[j],  hQ[a] = sum_j r_a[j] * zQ[j]
//   g0[a]   = G[a][a]
//   for e = 0..m-1:                                   (elimination, no pivoting, slot order)
//       d = G[e][e];  singular unless d > (1e-9 * g0[e])
//       for i = e+1..m-1:
//           f = G[i][e] / d
//           for l = e+1..m-1:  G[i][l] = G[i][l] - f * G[e][l]
//           hI[i] = hI[i] - f * hI[e];  hQ[i] = hQ[i] - f * hQ[e]
//   for e = m-1..0:                                   (back-substitution)
//       sI = hI[e];  for l = e+1..m-1 ascending:  sI = sI - G[e][l] * A_re[l];  A_re[e] = sI / G[e][e]
//       (A_im from hQ alike)
//   res = sum_j (dI*dI + dQ*dQ),  dI = ((zI[j] - A_re[0]*r_0[j]) - A_re[1]*r_1[j]) - ...,  dQ alike
// For m = 1 these are ftt_one's operations. In a search the r vector of the searched slot is formed
// on the fly from u, the others are read from `rs` ([slot][n_taps]) and the sums among them from
// AcfFmmSys; the values are the same sums whoever forms them.
#pragma once

#include "acf_fit_taps.h"

#if defined(__HIPCC__)
#define GNSS_FMM_UNROLL _Pragma("unroll")  // the slot loops: their indices must be constants
#else
#define GNSS_FMM_UNROLL
#endif

namespace gnss {

constexpr int kFmmMaxPaths = 4;   // = GNSS_ACF_MULTI_MAX_PATHS
constexpr int kFmmMaxQ = 4096;    // q_count at most
constexpr int kFmmMaxSweeps = 16;
constexpr int kFmmRow = 20;       // doubles per window in the kernel's output (AcfFmmRow)
constexpr int kFmmSysSums = 24;   // AcfFmmSys' sums: 16 of G (10 distinct), 4 of hI, 4 of hQ

// the candidate grid and the search's parameters (gnss_acf_fit_multi_cfg's fields; u travels beside it)
struct AcfFmmPar {
    int n_taps, prompt;
    double q_min, q_step;
    int q_count, max_paths, sweeps, sep_min;
    double gain_min;
};

// the sums among the slots' r vectors and with z
struct AcfFmmSys {
    double G[kFmmMaxPaths][kFmmMaxPaths], hI[kFmmMaxPaths], hQ[kFmmMaxPaths];
};

// a window's state: the slots' present candidate indices, each formed order's indices and residual
// (res[0] = energy). The kernel keeps it in LDS; one lane writes, every lane reads.
struct AcfFmmWork {
    AcfFmmSys sys;
    int pos[kFmmMaxPaths];
    int kept[kFmmMaxPaths][kFmmMaxPaths];  // [m - 1][slot]
    double res[kFmmMaxPaths + 1];
};

// one window's result; the kernel writes it as kFmmRow doubles in this order
struct AcfFmmRow {
    double paths, searches;
    double q[kFmmMaxPaths], A_re[kFmmMaxPaths], A_im[kFmmMaxPaths];  // by descending q
    double res[kFmmMaxPaths + 1];
    double energy;
};
static_assert(sizeof(AcfFmmRow) == kFmmRow * sizeof(double), "the kernel stores AcfFmmRow as kFmmRow doubles");

GNSS_FTT_HD double fmm_q(const AcfFmmPar& p, int i)
{
    return p.q_min + (double)i * p.q_step;
}

// a joint fit's amplitudes (slot order) and residual; ok: the set was usable and not singular
struct AcfFmmFit {
    bool ok;
    double A_re[kFmmMaxPaths], A_im[kFmmMaxPaths], res;
};

// The joint fit of M slots with slot k at q and the other slots as rs / s hold them (the file's
// head has the operations). k's row of rs and k's entries of s are not used.
template <int M>
GNSS_FTT_HD AcfFmmFit fmm_try(const AcfFmmSys& s, const double* rs, int n, const double* u, const double* zI,
                              const double* zQ, int k, double q)
{
    AcfFmmFit o{};
    double c[M], cI = 0, cQ = 0;
    GNSS_FMM_UNROLL
    for (int l = 0; l < M; l++) c[l] = 0;
    GNSS_FTT_TAP_LOOP
    for (int j = 0; j < n; j++) {
        const double rc = ftt_R(u[j] - q);
        GNSS_FMM_UNROLL
        for (int l = 0; l < M; l++) {
            const double rl = l == k ? rc : rs[l * n + j];
            const double t = rc * rl;
            c[l] = j ? c[l] + t : t;
        }
        const double tI = rc * zI[j], tQ = rc * zQ[j];
        cI = j ? cI + tI : tI;
        cQ = j ? cQ + tQ : tQ;
    }
    double G[M][M], hI[M], hQ[M], g0[M];
    GNSS_FMM_UNROLL
    for (int a = 0; a < M; a++) {
        GNSS_FMM_UNROLL
        for (int b = 0; b < M; b++) G[a][b] = a == k ? c[b] : b == k ? c[a] : s.G[a][b];
        hI[a] = a == k ? cI : s.hI[a];
        hQ[a] = a == k ? cQ : s.hQ[a];
        g0[a] = G[a][a];
    }
    GNSS_FMM_UNROLL
    for (int a = 0; a < M; a++)
        if (a == k && g0[a] == 0) return o;  // the candidate is not usable: its triangle touches no tap
    GNSS_FMM_UNROLL
    for (int e = 0; e < M; e++) {
        const double d = G[e][e];
        if (!(d > (1e-9 * g0[e]))) return o;  // singular
        GNSS_FMM_UNROLL
        for (int i = e + 1; i < M; i++) {
            const double f = G[i][e] / d;
            GNSS_FMM_UNROLL
            for (int l = e + 1; l < M; l++) G[i][l] = G[i][l] - f * G[e][l];
            hI[i] = hI[i] - f * hI[e];
            hQ[i] = hQ[i] - f * hQ[e];
        }
    }
    GNSS_FMM_UNROLL
    for (int e = M - 1; e >= 0; e--) {
        double sI = hI[e], sQ = hQ[e];
        GNSS_FMM_UNROLL
        for (int l = e + 1; l < M; l++) {
            sI = sI - G[e][l] * o.A_re[l];
            sQ = sQ - G[e][l] * o.A_im[l];
        }
        o.A_re[e] = sI / G[e][e];
        o.A_im[e] = sQ / G[e][e];
    }
    double res = 0;
    GNSS_FTT_TAP_LOOP
    for (int j = 0; j < n; j++) {
        const double rc = ftt_R(u[j] - q);
        double dI = zI[j], dQ = zQ[j];
        GNSS_FMM_UNROLL
        for (int l = 0; l < M; l++) {
            const double rl = l == k ? rc : rs[l * n + j];
            dI = dI - o.A_re[l] * rl;
            dQ = dQ - o.A_im[l] * rl;
        }
        const double t = dI * dI + dQ * dQ;
        res = j ? res + t : t;
    }
    o.res = res;
    o.ok = true;
    return o;
}

GNSS_FTT_HD AcfFmmFit fmm_try_m(int m, const AcfFmmSys& s, const double* rs, int n, const double* u,
                                const double* zI, const double* zQ, int k, double q)
{
    switch (m) {
    case 1: return fmm_try<1>(s, rs, n, u, zI, zQ, k, q);
    case 2: return fmm_try<2>(s, rs, n, u, zI, zQ, k, q);
    case 3: return fmm_try<3>(s, rs, n, u, zI, zQ, k, q);
    default: return fmm_try<4>(s, rs, n, u, zI, zQ, k, q);
    }
}

// A search's first step: the sums among the slots 0..m-1 other than k (k = -1: all of them) and
// with z, dealt over `nth` workers (worker `tid` takes the sums tid, tid + nth, ...).
GNSS_FTT_HD void fmm_sys_fill(AcfFmmWork& w, const double* rs, int m, int k, int n, const double* zI,
                              const double* zQ, int tid, int nth)
{
    for (int e = tid; e < kFmmSysSums; e += nth) {
        const int a = e < 16 ? e >> 2 : (e - 16) & 3, b = e < 16 ? e & 3 : a;
        if (a > b || b >= m || a == k || b == k) continue;
        const double* x = rs + a * n;
        const double* y = e < 16 ? rs + b * n : e < 20 ? zI : zQ;
        double s = 0;
        for (int j = 0; j < n; j++) {
            const double t = x[j] * y[j];
            s = j ? s + t : t;
        }
        if (e < 16) {
            w.sys.G[a][b] = s;
            w.sys.G[b][a] = s;
        } else if (e < 20) {
            w.sys.hI[a] = s;
        } else {
            w.sys.hQ[a] = s;
        }
    }
}

// candidate i lies closer than sep_min grid steps to a slot other than k
GNSS_FTT_HD bool fmm_too_close(const AcfFmmPar& p, const AcfFmmWork& w, int m, int k, int i)
{
    bool close = false;
    for (int l = 0; l < m; l++) {
        const int d = i > w.pos[l] ? i - w.pos[l] : w.pos[l] - i;
        close = close || (l != k && d < p.sep_min);
    }
    return close;
}

// A search's second step: worker tid's share of the candidates (tid, tid + nth, ...) in slot k's
// place -> the lexicographic minimum of (res, i) of the share
GNSS_FTT_HD AcfFttBest fmm_search_share(const AcfFmmPar& p, const AcfFmmWork& w, const double* rs, int m, int k,
                                        const double* u, const double* zI, const double* zQ, int tid, int nth)
{
    AcfFttBest b = ftt_best_none();
    for (int i = tid; i < p.q_count; i += nth) {
        if (fmm_too_close(p, w, m, k, i)) continue;
        const AcfFmmFit y = fmm_try_m(m, w.sys, rs, p.n_taps, u, zI, zQ, k, fmm_q(p, i));
        if (y.ok && ftt_better(y.res, i, b.res, b.h)) {
            b.res = y.res;
            b.h = i;
        }
    }
    return b;
}

// A search's last step: slot k takes candidate i, its r vector into rs (dealt over the workers)
GNSS_FTT_HD void fmm_place(const AcfFmmPar& p, AcfFmmWork& w, double* rs, int k, int i, const double* u, int tid,
                           int nth)
{
    const double q = fmm_q(p, i);
    for (int j = tid; j < p.n_taps; j += nth) rs[k * p.n_taps + j] = ftt_R(u[j] - q);
    if (tid == 0) w.pos[k] = i;
}

// The orders m = 1..max_paths. ops.search(m, k) runs Search(k) among m slots and, if a candidate
// survived, has placed it (w.pos[k], rs) before it returns the winner to every worker; ops.sync()
// makes the lead's writes visible to all. -> the number of orders formed; *searches: the Search calls.
template <class Ops>
GNSS_FTT_HD int fmm_orders(const AcfFmmPar& p, AcfFmmWork& w, Ops& ops, bool lead, int* searches)
{
    int formed = 0, count = 0;
    for (int m = 1; m <= p.max_paths; m++) {
        count++;
        AcfFttBest b = ops.search(m, m - 1);  // slot m - 1 is appended
        if (b.h == kFttNone) break;
        double res = b.res;
        for (int s = 0; s < p.sweeps; s++) {
            bool moved = false;
            for (int k = 0; k < m; k++) {
                const int before = w.pos[k];
                count++;
                b = ops.search(m, k);
                if (b.h != kFttNone) {  // (the present position survives unless a residual overflows)
                    res = b.res;
                    moved = moved || b.h != before;
                }
            }
            if (!moved) break;
        }
        if (lead) {
            for (int l = 0; l < m; l++) w.kept[m - 1][l] = w.pos[l];
            w.res[m] = res;
        }
        formed = m;
    }
    ops.sync();
    *searches = count;
    return formed;
}

// paths: the largest formed m with res[m - 1] > gain_min * res[m]; 1 if none passes but order 1
// was formed; 0 if it was not
GNSS_FTT_HD int fmm_paths(const AcfFmmPar& p, const AcfFmmWork& w, int formed)
{
    int sel = formed ? 1 : 0;
    for (int m = 1; m <= formed; m++)
        if (w.res[m - 1] > p.gain_min * w.res[m]) sel = m;
    return sel;
}

// The window's row into `row` (kFmmRow doubles, AcfFmmRow's order). finite: ftt_all_finite(z). For
// sel > 0 the slots, rs and w.sys hold the selected order (kept[sel - 1]); its amplitudes are formed
// again from them, the same operations as in the search, and stored by descending q.
GNSS_FTT_HD void fmm_row(const AcfFmmPar& p, const AcfFmmWork& w, const double* rs, bool finite, int formed, int sel,
                         int searches, const double* u, const double* zI, const double* zQ, double* row)
{
    const double nan = NAN;
    for (int i = 0; i < kFmmRow; i++) row[i] = nan;
    row[0] = (double)sel;
    row[1] = (double)searches;
    if (!finite) return;
    for (int m = 0; m <= formed; m++) row[14 + m] = w.res[m];
    row[19] = w.res[0];
    if (sel == 0) return;
    const AcfFmmFit y = fmm_try_m(sel, w.sys, rs, p.n_taps, u, zI, zQ, 0, fmm_q(p, w.pos[0]));
    GNSS_FMM_UNROLL
    for (int a = 0; a < kFmmMaxPaths; a++) {
        if (a >= sel) continue;
        int rank = 0;
        for (int b = 0; b < sel; b++) rank += w.pos[b] > w.pos[a] ? 1 : 0;
        row[2 + rank] = fmm_q(p, w.pos[a]);
        row[6 + rank] = y.A_re[a];
        row[10 + rank] = y.A_im[a];
    }
}

// the host's side of a search: one worker
struct AcfFmmHostOps {
    const AcfFmmPar& p;
    AcfFmmWork& w;
    double* rs;
    const double *u, *zI, *zQ;
    AcfFttBest search(int m, int k)
    {
        fmm_sys_fill(w, rs, m, k, p.n_taps, zI, zQ, 0, 1);
        const AcfFttBest b = fmm_search_share(p, w, rs, m, k, u, zI, zQ, 0, 1);
        if (b.h != kFttNone) fmm_place(p, w, rs, k, b.h, u, 0, 1);
        return b;
    }
    void sync() {}
};

// The whole fit of one coherent vector on one worker (the host path). rs: 4 * n_taps doubles of
// workspace; row: kFmmRow doubles.
inline void fmm_window(const AcfFmmPar& p, const double* u, const double* zI, const double* zQ, double* rs,
                       double* row)
{
    AcfFmmWork w{};
    const int n = p.n_taps;
    for (int i = 0; i < kFmmMaxPaths * n; i++) rs[i] = 0;
    const bool finite = ftt_all_finite(n, zI, zQ);
    int formed = 0, searches = 0, sel = 0;
    if (finite) {
        w.res[0] = ftt_energy(n, zI, zQ);
        AcfFmmHostOps ops{p, w, rs, u, zI, zQ};
        formed = fmm_orders(p, w, ops, true, &searches);
        sel = fmm_paths(p, w, formed);
        for (int l = 0; l < sel; l++) fmm_place(p, w, rs, l, w.kept[sel - 1][l], u, 0, 1);
        fmm_sys_fill(w, rs, sel, -1, n, zI, zQ, 0, 1);
    }
    fmm_row(p, w, rs, finite, formed, sel, searches, u, zI, zQ, row);
}

// What the kernel takes (acf_fit_multi.hip)
struct AcfFmmDev {
    AcfFttIo io;  // rows: [win_base[n]][kFmmRow]
    AcfFmmPar par;
};

// One block per window on `stream` (a hipStream_t) of the current device. Returns the hipError_t
// of the launch (0: none).
int acf_fit_multi_launch(const AcfFmmDev& d, void* stream);

}  // namespace gnss
