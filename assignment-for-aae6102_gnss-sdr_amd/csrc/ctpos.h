// ctpos.h — the positioning half of trackingCT_POS_updated.m (:147-171, :420-565) and of its
// 25-tap sibling (trackingCT_POS_updated_multicorrelator.m:446-590) as a pass over the tracking
// records (positioning does not feed back into the scalar loops). Two stages:
//   1. the measurement table: per epoch the tracking step `Index` at which it fires and, per
//      channel, `index`, codePhaseMeas and carrFreq(Index) (:423-453, :514) -- from host records
//      (ctpos.cpp) or, for GNSS_OUT_DEVICE records, by three kernels so that only the table
//      crosses PCIe (ctpos.hip). One source for both (below), compiled with -ffp-contract=off on
//      both sides: the two tables are equal bit for bit;
//   2. the solver on the table (ctpos.cpp): transmitTime, pseudoranges, olspos.m, LS_SA_code_Vel.m.
#pragma once

#include <string>
#include <vector>

#include "gnss_internal.h"

namespace gnss {

// (first i, 1-based, with a[i] > curr) over a[1..L], L + 1 when there is none: the `break` of
// :442-446 and the flag of :427. absoluteSample increases, so this is a binary search.
GNSS_HD int64_t ct_first_after(const double* a, int64_t L, double curr)
{
    int64_t lo = 0, hi = L;  // a[0 .. lo) <= curr < a[hi .. L)
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (a[mid] > curr)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo + 1;
}

// currMeasSample = sampleStartMea + measSampleStep * posIndex (:423), an exact integer in a
// double (< 2^53)
GNSS_HD double ct_curr_sample(double sampleStartMea, double measSampleStep, int64_t posIndex)
{
    return sampleStartMea + measSampleStep * (double)posIndex;
}

// codePhaseMeas (:450-453): remChip(index) + (codeFreq(index) / Fs) * ((curr - absoluteSample(index))
// / dataType), every operation rounded on its own
GNSS_HD double ct_code_phase(double remChip, double codeFreq, double absoluteSample, double curr, double Fs,
                             double dataType)
{
    const double codePhaseStepX = codeFreq / Fs;
    return remChip + codePhaseStepX * ((curr - absoluteSample) / dataType);
}

// The measurement table, `rows` epochs of n channels.
struct CtTable {
    int n = 0;
    int64_t rows = 0;
    std::vector<int64_t> Index;    // [rows]    the tracking step of the epoch (1-based)
    std::vector<int64_t> index;    // [rows][n] :447 (1-based; >= 1)
    std::vector<double> cpm;       // [rows][n] codePhaseMeas
    std::vector<double> carrFreq;  // [rows][n] carrFreq(Index) (:514)
};

// The four series of one record set: series f of channel s at base[(s * GNSS_NFIELDS + f) * max_len].
struct CtRecords {
    const double* base;
    int64_t max_len;
    int64_t L;  // steps: min over the channels' len
    int n;
};

// measSampleStep = fix(Fs * navSolPeriod / 1000) * dataType (:164)
double ct_meas_step(const gnss_ct_pos_cfg& c);
// sampleStartMea = max(sampleStart) + 1 (:160)
double ct_sample_start(const gnss_ct_pos_cfg& c);

// Stage 1 from host records. GNSS_EINDEX where `index` = 0 (MATLAB raises at :450), GNSS_EARG when
// more than `cap` epochs fire.
int ct_extract_host(const gnss_ct_pos_cfg& c, const CtRecords& r, int64_t cap, CtTable* t, std::string* err);
// Stage 1 from device records (ctpos.hip), on `stream` of the current device. GNSS_EDEVICE on a HIP
// error or when a kernel's bound check refused a record index (the context stays usable).
int ct_extract_device(const gnss_ct_pos_cfg& c, const CtRecords& r, int64_t cap, hipStream_t stream, CtTable* t,
                      std::string* err);
// Stage 2.
int ct_solve_table(const gnss_ct_pos_cfg& c, const CtTable& t, gnss_nav_sol_ct* out, std::string* err);

}  // namespace gnss
