// ctpos.cpp — the positioning half of trackingCT_POS_updated.m (:147-171, :420-565; the 25-tap
// sibling's :446-590 differs in transmitTime and the refresh cadence only) with olspos.m, hmat.m
// and LS_SA_code_Vel.m, as a pass over the tracking records: the measurement table from host
// records, and the solver on a table (ctpos.h). Host code beside vtnav.cpp, whose svPosVel.m and
// geo helpers it calls through their exports (gnss_sv_pos_vel, gnss_geo). Built with
// -ffp-contract=off: every operation rounds separately, in the reference's association order
// (line cites of trackingCT_POS_updated.m inline). MATLAB's `\`, inv() and matrix products are
// LAPACK / BLAS backed and round differently in the last place; the bounds are in
// tests/test_ctpos_kat.py.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "ctpos.h"
#include "host.h"

namespace {

constexpr double kPi = 3.14159265358979323846;  // MATLAB pi
constexpr int kMaxCh = GNSS_VT_MAX_CH;
constexpr int kOlsMaxIter = 50;  // olspos.m:44 has no cap (maxiter = 10 is commented out)

// x = A \ y for a tall full-rank A (m x 4, row-major, destroyed; y destroyed): Householder QR with
// column pivoting (the largest remaining column norm first), Q' applied to y, back substitution,
// the permutation undone -- what MATLAB's mldivide does for a non-square A (xGEQP3). NaN inputs
// give a NaN x, which ends olspos's loop as in MATLAB.
void lstsq_qr(double* A, double* y, int m, double* x)
{
    int perm[4] = {0, 1, 2, 3};
    for (int j = 0; j < 4; j++) {
        int p = j;
        double best = -1;
        for (int c = j; c < 4; c++) {
            double s = 0;
            for (int i = j; i < m; i++) s += A[i * 4 + c] * A[i * 4 + c];
            if (s > best) {
                best = s;
                p = c;
            }
        }
        if (p != j) {
            for (int i = 0; i < m; i++) std::swap(A[i * 4 + j], A[i * 4 + p]);
            std::swap(perm[j], perm[p]);
        }
        const double norm = std::sqrt(best);
        const double alpha = A[j * 4 + j] > 0 ? -norm : norm;
        double v[kMaxCh];  // the reflector I - 2 v v' / (v' v), v = a - alpha e1
        double vv = 0;
        for (int i = j; i < m; i++) {
            v[i] = A[i * 4 + j] - (i == j ? alpha : 0.0);
            vv += v[i] * v[i];
        }
        if (vv > 0) {
            for (int c = j + 1; c < 4; c++) {
                double d = 0;
                for (int i = j; i < m; i++) d += v[i] * A[i * 4 + c];
                const double f = 2 * d / vv;
                for (int i = j; i < m; i++) A[i * 4 + c] = A[i * 4 + c] - f * v[i];
            }
            double d = 0;
            for (int i = j; i < m; i++) d += v[i] * y[i];
            const double f = 2 * d / vv;
            for (int i = j; i < m; i++) y[i] = y[i] - f * v[i];
        }
        A[j * 4 + j] = alpha;
    }
    // the rank as mldivide takes it: diagonal entries above max(m, n) * eps(|R(1,1)|); a rank
    // deficient A gets the basic solution (zeros for the columns beyond the rank), with MATLAB's
    // warning and no error
    int exp2 = 0;
    std::frexp(std::fabs(A[0]), &exp2);
    const double tol = (m > 4 ? m : 4) * std::ldexp(1.0, exp2 - 53);
    int rank = 0;
    while (rank < 4 && std::fabs(A[rank * 4 + rank]) > tol) rank++;
    if (!(std::fabs(A[0]) - std::fabs(A[0]) == 0)) rank = 4;  // Inf / NaN: let them through
    double z[4] = {0, 0, 0, 0};
    for (int i = rank - 1; i >= 0; i--) {
        double s = y[i];
        for (int c = i + 1; c < rank; c++) s = s - A[i * 4 + c] * z[c];
        z[i] = s / A[i * 4 + i];
    }
    for (int i = 0; i < 4; i++) x[perm[i]] = z[i];
}

// inv() of a 4 x 4 (row-major, destroyed): LU with partial pivoting, then the identity's columns
// through L and U. A zero pivot divides: Inf / NaN, as MATLAB's inv of a singular matrix.
void inv4(double* A, double* X)
{
    int piv[4] = {0, 1, 2, 3};
    for (int j = 0; j < 4; j++) {
        int p = j;
        for (int i = j + 1; i < 4; i++)
            if (std::fabs(A[i * 4 + j]) > std::fabs(A[p * 4 + j])) p = i;
        if (p != j) {
            for (int k = 0; k < 4; k++) std::swap(A[j * 4 + k], A[p * 4 + k]);
            std::swap(piv[j], piv[p]);
        }
        for (int i = j + 1; i < 4; i++) {
            const double l = A[i * 4 + j] / A[j * 4 + j];
            A[i * 4 + j] = l;
            for (int k = j + 1; k < 4; k++) A[i * 4 + k] = A[i * 4 + k] - l * A[j * 4 + k];
        }
    }
    for (int c = 0; c < 4; c++) {
        double y[4];
        for (int i = 0; i < 4; i++) {
            double s = piv[i] == c ? 1.0 : 0.0;
            for (int k = 0; k < i; k++) s = s - A[i * 4 + k] * y[k];
            y[i] = s;
        }
        for (int i = 3; i >= 0; i--) {
            double s = y[i];
            for (int k = i + 1; k < 4; k++) s = s - A[i * 4 + k] * X[k * 4 + c];
            X[i * 4 + c] = s / A[i * 4 + i];
        }
    }
}

// G = A' * A for A (m x 4), each sum left to right
void gram4(const double* A, int m, double* G)
{
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double s = A[i] * A[j];
            for (int q = 1; q < m; q++) s = s + A[q * 4 + i] * A[q * 4 + j];
            G[i * 4 + j] = s;
        }
}

// olspos.m:30-61: est[4] in (the warm start) and out, dop[4]. GNSS_ENOCONV past kOlsMaxIter.
int olspos(const double* prvec, const double (*sv)[3], int n, double* est, double* dop, int* iters)
{
    double H[kMaxCh * 4], Hw[kMaxCh * 4], y[kMaxCh];
    double beta[4] = {1e9, 1e9, 1e9, 1e9};
    int it = 0;
    auto norm4 = [](const double* b) { return std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2] + b[3] * b[3]); };
    while (norm4(beta) > 1e-3) {  // tol (olspos.m:30,44); a NaN norm compares false
        if (it >= kOlsMaxIter) return GNSS_ENOCONV;
        for (int s = 0; s < n; s++) {
            // hmat.m:18-19: tmpvec = usrpos - svmat(i,:), h(i,1:3) = tmpvec ./ norm(tmpvec)
            const double d0 = est[0] - sv[s][0], d1 = est[1] - sv[s][1], d2 = est[2] - sv[s][2];
            const double r = std::sqrt(d0 * d0 + d1 * d1 + d2 * d2);
            y[s] = prvec[s] - r - est[3];  // olspos.m:46-47 (norm(sv - est) = norm(est - sv))
            H[s * 4 + 0] = d0 / r;
            H[s * 4 + 1] = d1 / r;
            H[s * 4 + 2] = d2 / r;
            H[s * 4 + 3] = 1;
        }
        std::memcpy(Hw, H, sizeof(double) * n * 4);
        lstsq_qr(Hw, y, n, beta);  // beta = H \ y (olspos.m:50)
        for (int k = 0; k < 4; k++) est[k] = est[k] + beta[k];
        it++;
    }
    double G[16], Q[16];
    gram4(H, n, G);  // Q = inv(H' * H) of the last H (olspos.m:57-61)
    inv4(G, Q);
    dop[0] = std::sqrt(Q[0] + Q[5] + Q[10] + Q[15]);
    dop[1] = std::sqrt(Q[0] + Q[5] + Q[10]);
    dop[2] = std::sqrt(Q[0] + Q[5]);
    dop[3] = std::sqrt(Q[10]);
    *iters = it;
    return GNSS_OK;
}

// LS_SA_code_Vel.m:61-95: VR[3], dtRV from the fitted position XR, the rotated satellite positions
// XS, their velocities VS, the Doppler dop_R = carrFreq - IF and dtSV = sv_clk_vel
void ls_vel(const double* XR, const double (*XS)[3], const double (*VS)[3], const double* dop_R, double lambda,
            const double* dtSV, int n, double* x)
{
    double A[kMaxCh * 4], rhs[kMaxCh];
    for (int s = 0; s < n; s++) {
        const double e0 = XS[s][0] - XR[0], e1 = XS[s][1] - XR[1], e2 = XS[s][2] - XR[2];
        const double dist = std::sqrt(e0 * e0 + e1 * e1 + e2 * e2);  // :68
        A[s * 4 + 0] = (XR[0] - XS[s][0]) / dist;                    // :71-74
        A[s * 4 + 1] = (XR[1] - XS[s][1]) / dist;
        A[s * 4 + 2] = (XR[2] - XS[s][2]) / dist;
        A[s * 4 + 3] = 1;
        const double b = (A[s * 4] * VS[s][0] + A[s * 4 + 1] * VS[s][1] + A[s * 4 + 2] * VS[s][2]) - dtSV[s];  // :77
        const double y0 = dop_R[s] * lambda;                                                                      // :81
        rhs[s] = y0 - b;
    }
    double N[16], Ni[16], M[4 * kMaxCh];
    gram4(A, n, N);  // N = A' * invQ * A with invQ = I (:85-89)
    inv4(N, Ni);
    for (int i = 0; i < 4; i++)  // x = (N^-1) * A' * invQ * (y0 - b), left to right (:92)
        for (int s = 0; s < n; s++) {
            double m = Ni[i * 4] * A[s * 4];
            for (int q = 1; q < 4; q++) m = m + Ni[i * 4 + q] * A[s * 4 + q];
            M[i * n + s] = m;
        }
    for (int i = 0; i < 4; i++) {
        double v = M[i * n] * rhs[0];
        for (int s = 1; s < n; s++) v = v + M[i * n + s] * rhs[s];
        x[i] = v;
    }
}

}  // namespace

double gnss::ct_meas_step(const gnss_ct_pos_cfg& c)
{
    return std::trunc(c.Fs * c.navSolPeriod / 1000) * c.dataType;  // :164
}

double gnss::ct_sample_start(const gnss_ct_pos_cfg& c)
{
    int64_t m = c.sampleStart[0];
    for (int s = 1; s < c.n; s++) m = std::max(m, c.sampleStart[s]);
    return (double)(m + 1);  // :160
}

// :423-453 over host records: the loop over the tracking steps collapsed to its epochs. Step Index
// fires epoch posIndex iff every channel's absoluteSample(Index) > currMeasSample, i.e. Index >=
// F = max over the channels of (the first i with absoluteSample(i) > currMeasSample); one epoch per
// step, so it fires at max(F, the last epoch's step + 1).
int gnss::ct_extract_host(const gnss_ct_pos_cfg& c, const CtRecords& r, int64_t cap, CtTable* t, std::string* err)
{
    const int n = r.n;
    const double start = ct_sample_start(c), step = ct_meas_step(c);
    auto series = [&](int s, int f) { return r.base + ((int64_t)s * GNSS_NFIELDS + f) * r.max_len; };
    t->n = n;
    t->rows = 0;
    int64_t last = 0;
    for (int64_t k = 0;; k++) {
        const double curr = ct_curr_sample(start, step, k);
        int64_t first[kMaxCh], F = 0;
        for (int s = 0; s < n; s++) {
            first[s] = ct_first_after(series(s, GNSS_F_absoluteSample), r.L, curr);
            F = std::max(F, first[s]);
        }
        const int64_t Index = std::max(F, last + 1);
        if (Index > r.L) break;
        if (k >= cap) {
            *err = "gnss_nav_sol_ct.cap is smaller than the epochs the records hold";
            return GNSS_EARG;
        }
        t->Index.push_back(Index);
        for (int s = 0; s < n; s++) {
            const int64_t index = first[s] - 1;  // :447
            if (index < 1) {
                *err = "positioning: index = 0 (the measurement sample lies at or before a channel's first "
                       "record; MATLAB raises at trackingCT_POS_updated.m:450)";
                return GNSS_EINDEX;
            }
            t->index.push_back(index);
            t->cpm.push_back(ct_code_phase(series(s, GNSS_F_remChip)[index - 1], series(s, GNSS_F_codeFreq)[index - 1],
                                           series(s, GNSS_F_absoluteSample)[index - 1], curr, c.Fs,
                                           (double)c.dataType));
            t->carrFreq.push_back(series(s, GNSS_F_carrFreq)[Index - 1]);  // the loop's current value (:514)
        }
        t->rows = k + 1;
        last = Index;
    }
    return GNSS_OK;
}

// :455-565 on the measurement table
int gnss::ct_solve_table(const gnss_ct_pos_cfg& c, const CtTable& t, gnss_nav_sol_ct* out, std::string* err)
{
    const int n = c.n;
    const double cS = c.cSpeed;
    const double measSampleStep = ct_meas_step(c);
    const int64_t ms1 = c.msToProcessCT_1ms;
    int64_t cx_min = c.countinx[0];
    for (int s = 1; s < n; s++) cx_min = std::min<int64_t>(cx_min, c.countinx[s]);
    // corrUpt = corrUpdateSec / (pdi * t), counter_corr = corrUpt - 1 (:47,128-130: pdi = 1 there;
    // the 25-tap file's :46,120-122: pdi = track.pdi)
    double corrUpt = 0.01 / ((c.mode == GNSS_CT_POS_MULTICORR ? c.pdi : 1) * c.ms);
    double counter[kMaxCh];
    for (int s = 0; s < n; s++) counter[s] = corrUpt - 1;
    double el[kMaxCh] = {}, az[kMaxCh] = {}, ionodel[kMaxCh] = {}, tropodel[kMaxCh] = {};
    double est[4] = {c.cnslxyz[0], c.cnslxyz[1], c.cnslxyz[2], 0};  // estusr_wls (:36; olspos.m:38)
    double localTime = INFINITY;                                    // :147
    out->rows = 0;
    for (int64_t k = 0; k < t.rows; k++) {
        const int64_t Index = t.Index[k];
        const int64_t* index = &t.index[k * n];
        const double* cpm = &t.cpm[k * n];
        double tt[kMaxCh];
        if (c.mode == GNSS_CT_POS_UPDATED) {
            // pdi as the last channel's branch left it at this step (:183-184,294-295)
            const int64_t pdi = Index <= ms1 + c.countinx[n - 1] ? 1 : 10;
            if (Index > ms1 + cx_min) {  // a channel ran the 10-ms branch this step (:301-302)
                corrUpt = 0.01 / (10 * c.ms);
                for (int s = 0; s < n; s++) counter[s] = corrUpt - 1;
            }
            for (int s = 0; s < n; s++) {  // :455-457
                const int64_t cx = c.countinx[s];
                const int64_t w = (index[s] - ms1 - cx) * pdi + (ms1 + cx) - (c.nav1[s] + c.sfb1[s] * 20);
                tt[s] = cpm[s] / c.codelength / 1000 + (double)w / 1000 + c.TOW1[s];
            }
        } else {
            for (int s = 0; s < n; s++) {  // trackingCT_POS_updated_multicorrelator.m:481-483
                const int64_t w = index[s] - (c.nav1[s] + c.sfb1[s] * 20);
                tt[s] = cpm[s] / c.codelength / 1000 + (double)w / 1000 + c.TOW1[s];
            }
        }
        if (localTime == INFINITY) {  // :462-465
            double maxTime = tt[0];
            for (int s = 1; s < n; s++) maxTime = std::max(maxTime, tt[s]);
            localTime = maxTime + 75.0 / 1000;
        }
        double pr[kMaxCh], prvec[kMaxCh], svr[kMaxCh][3], svv[kMaxCh][3], clkv[kMaxCh];
        for (int s = 0; s < n; s++) pr[s] = (localTime - tt[s]) * cS;  // :466
        for (int s = 0; s < n; s++) {                                  // :472-505
            double sv[3], clkm, grp, in[15];
            int st = gnss_sv_pos_vel(&c.eph[s], tt[s], sv, svv[s], &clkm, &clkv[s], &grp);  // :479-480
            if (st) {
                *err = "positioning: svPosVel rejects the transmit time";
                return st;
            }
            prvec[s] = pr[s] + clkm - grp * cS;  // :483
            in[0] = sv[0], in[1] = sv[1], in[2] = sv[2], in[3] = prvec[s];
            gnss_geo(GNSS_GEO_EROTCORR, in, svr[s]);  // :486
            counter[s] = counter[s] + 1;              // :489
            if (counter[s] == corrUpt) {
                double enu[3], llh[3], trop;
                for (int q = 0; q < 3; q++) in[q] = svr[s][q], in[3 + q] = est[q];
                gnss_geo(GNSS_GEO_XYZ2ENU, in, enu);  // :491
                const double el_rad = std::atan(enu[2] / std::sqrt(enu[0] * enu[0] + enu[1] * enu[1]));  // :492
                const double az_rad = std::atan2(enu[0], enu[1]);                                        // :494
                az[s] = az_rad * 180 / kPi;
                el[s] = el_rad * 180 / kPi;
                gnss_geo(GNSS_GEO_XYZ2LLH, est, llh);  // :497-498
                in[0] = tt[s];
                for (int q = 0; q < 3; q++) in[1 + q] = svr[s][q], in[4 + q] = est[q];
                for (int q = 0; q < 4; q++) in[7 + q] = c.ALPHA[q], in[11 + q] = c.BETA[q];
                gnss_geo(GNSS_GEO_IONO, in, &ionodel[s]);  // :499
                const double tin[4] = {c.doy, llh[0] * 180 / kPi, llh[2], el[s]};
                // (a NaN latitude, after a fit that ended on a NaN beta, indexes Get_UNB3_Model.m's
                // table with NaN: MATLAB raises)
                st = std::isfinite(tin[1]) ? gnss_geo(GNSS_GEO_TROP, tin, &trop) : GNSS_EINDEX;  // :500
                if (st) {
                    *err = "positioning: trop_UNB3's table lookup fails at this latitude";
                    return st;
                }
                tropodel[s] = std::fabs(trop);
                counter[s] = 0;
            }
            prvec[s] = prvec[s] - ionodel[s] - tropodel[s];  // :504
        }
        double dop[4], x[4], dopR[kMaxCh];
        int iters = 0;
        const int st = olspos(prvec, svr, n, est, dop, &iters);  // :512
        if (st) {
            *err = "positioning: olspos did not converge within 50 iterations";
            out->rows = 0;
            return st;
        }
        for (int s = 0; s < n; s++) dopR[s] = t.carrFreq[k * n + s] - c.IF;
        ls_vel(est, svr, svv, dopR, 0.190293672798365, clkv, n, x);  // :513-514
        double in[6] = {est[0], est[1], est[2], c.cnslxyz[0], c.cnslxyz[1], c.cnslxyz[2]};
        double enu[3], llh[3], venu[3];
        gnss_geo(GNSS_GEO_XYZ2ENU, in, enu);   // :517
        gnss_geo(GNSS_GEO_XYZ2LLH, est, llh);  // :520-526
        const double Lb = llh[0], lb = llh[1];
        const double Cen[3][3] = {{-std::sin(lb), std::cos(lb), 0},
                                  {-std::sin(Lb) * std::cos(lb), -std::sin(Lb) * std::sin(lb), std::cos(Lb)},
                                  {-std::cos(Lb) * std::cos(lb), -std::cos(Lb) * std::sin(lb), -std::sin(Lb)}};
        for (int i = 0; i < 3; i++) venu[i] = Cen[i][0] * x[0] + Cen[i][1] * x[1] + Cen[i][2] * x[2];
        localTime = localTime - est[3] / cS;  // :550
        for (int s = 0; s < n; s++) {         // :509-551
            out->rawPseudorange[k * n + s] = pr[s];
            out->satEA[k * n + s] = el[s];
            out->satAZ[k * n + s] = az[s];
            out->timeTransmit[k * n + s] = tt[s];
            out->codePhaseMeas[k * n + s] = cpm[s];
            if (out->index) out->index[k * n + s] = index[s];
            if (out->carrFreqMeas) out->carrFreqMeas[k * n + s] = t.carrFreq[k * n + s];
        }
        for (int q = 0; q < 3; q++) {
            out->usrPos[k * 3 + q] = est[q];
            out->usrVel[k * 3 + q] = x[q];
            out->usrPosENU[k * 3 + q] = enu[q];
            out->usrVelENU[k * 3 + q] = venu[q];
        }
        out->usrPosLLH[k * 3 + 0] = llh[0] * 180 / kPi;  // :529-530
        out->usrPosLLH[k * 3 + 1] = llh[1] * 180 / kPi;
        out->usrPosLLH[k * 3 + 2] = llh[2];
        out->clkBias[k] = est[3];
        out->clkDrift[k] = x[3];
        for (int q = 0; q < 4; q++) out->DOP[k * 4 + q] = dop[q];
        out->localTime[k] = localTime;
        out->Index[k] = Index;
        if (out->iters) out->iters[k] = iters;
        localTime = localTime + measSampleStep / c.Fs;  // :554
    }
    out->rows = t.rows;
    return GNSS_OK;
}

using namespace gnss;
using namespace gnss::host;

extern "C" {

// trackingCT_POS_updated.m:147-171,420-565 as a pass over the tracking records (ctpos.h): the
// measurement table on the host or, for GNSS_OUT_DEVICE records, on the GPU, then the solver
int gnss_ct_pos_solve(gnss_ctx* ctx, const gnss_ct_pos_cfg* cfg, const gnss_track_out* rec, gnss_nav_sol_ct* out)
{
    if (out) out->rows = 0;
    if (!cfg || !rec || !out) return fail(ctx, GNSS_EARG, "gnss_ct_pos_solve: a null argument");
    const bool on_device = (rec->flags & GNSS_OUT_DEVICE) != 0;
    const int n = cfg->n;
    if (n >= 1 && n < 4) return fail(ctx, GNSS_EARG, "insufficient number of satellites (hmat.m:10): %d", n);
    if (n < 1 || n > GNSS_VT_MAX_CH) return fail(ctx, GNSS_EARG, "gnss_ct_pos_cfg.n outside 4..%d", GNSS_VT_MAX_CH);
    if ((cfg->mode != GNSS_CT_POS_UPDATED && cfg->mode != GNSS_CT_POS_MULTICORR) ||
        (cfg->dataType != 1 && cfg->dataType != 2) || !(cfg->Fs > 0) || !(cfg->codelength > 0) || !(cfg->ms > 0) ||
        !(cfg->cSpeed > 0) || !(cfg->navSolPeriod > 0) || !(ct_meas_step(*cfg) >= 1) ||
        (cfg->mode == GNSS_CT_POS_MULTICORR && cfg->pdi < 1))
        return fail(ctx, GNSS_EARG, "gnss_ct_pos_cfg: mode, dataType, Fs, codelength, ms, cSpeed, navSolPeriod or pdi");
    if (!rec->rec || !rec->len || rec->max_len < 1) return fail(ctx, GNSS_EARG, "gnss_ct_pos_solve: records");
    if (out->cap < 0 || !out->rawPseudorange || !out->usrPos || !out->usrVel || !out->usrPosENU || !out->usrPosLLH ||
        !out->clkBias || !out->usrVelENU || !out->clkDrift || !out->DOP || !out->satEA || !out->satAZ ||
        !out->timeTransmit || !out->codePhaseMeas || !out->localTime || !out->Index)
        return fail(ctx, GNSS_EARG, "gnss_nav_sol_ct: a null array");
    CtRecords r{rec->rec, rec->max_len, rec->len[0], n};
    for (int s = 0; s < n; s++) {
        if (rec->len[s] < 0 || rec->len[s] > rec->max_len)
            return fail(ctx, GNSS_EARG, "gnss_ct_pos_solve: len[%d] outside 0..max_len", s);
        r.L = std::min(r.L, rec->len[s]);
    }
    CtTable table;
    std::string err;
    int st;
    if (on_device) {
        if (!ctx) return GNSS_EARG;
        if (!ctx->members.empty())
            return fail(ctx, GNSS_EARG, "gnss_ct_pos_solve: device records on a multi-device context");
        HIP_TRY(hipSetDevice(ctx->device));
        st = ct_extract_device(*cfg, r, out->cap, ctx->stream, &table, &err);
    } else {
        st = ct_extract_host(*cfg, r, out->cap, &table, &err);
    }
    if (st == GNSS_OK) st = ct_solve_table(*cfg, table, out, &err);
    if (st != GNSS_OK) {
        out->rows = 0;
        return fail(ctx, st, "%s", err.c_str());
    }
    return GNSS_OK;
}

}  // extern "C"
