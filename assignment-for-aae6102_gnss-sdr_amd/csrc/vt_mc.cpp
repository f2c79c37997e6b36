// vt_mc.cpp — the host half of a 25-tap vector-tracking step
// (trackingVT_POS_updated_multicorrelator.m:151-470): read sizing, the 25 replica colons and
// their table-index range, and the scalar end from the 50 sums (vt_mc_prepare / vt_mc_finish in
// vt_mc.h: the source the loop in api_vt.cpp runs). Compiled with -ffp-contract=off like the
// rest of the library, so every operation rounds as MATLAB's does.
// Reference: SDR_MATLAB-main/acqtckpos/trackingVT_POS_updated_multicorrelator.m.
#include <cmath>

#include "vt_mc.h"

using namespace gnss;

extern "C" {

int gnss_vt_mc_prepare(const gnss_signal* sg, int32_t pdi, const gnss_vt_chan* c, double codeFreq_new,
                       double tap_a[GNSS_VT_MC_TAPS], double tap_c[GNSS_VT_MC_TAPS], int64_t* numSample)
{
    if (!sg || !(sg->Fs > 0) || !(sg->codeFreqBasis > 0) || pdi < 1 || !c || c->prn < 1 || c->prn > 51 ||
        !(c->codeFreq > 0) || !(codeFreq_new > 0))
        return GNSS_EARG;
    const VtMcPrep p = vt_mc_prepare(sg->Fs, sg->codelength, pdi, c->remChip, c->codeFreq, codeFreq_new);
    if (p.bad) return p.bad;
    if (numSample) *numSample = p.n;
    for (int j = 0; j < kVtMcTaps; j++) {
        if (tap_a) tap_a[j] = p.a[j];
        if (tap_c) tap_c[j] = p.c[j];
    }
    return GNSS_OK;
}

int gnss_vt_mc_nco_step(const gnss_signal* sg, const gnss_track* tr, int32_t pdi, gnss_vt_chan* c,
                        double codeFreq_new, const double tap_i[GNSS_VT_MC_TAPS],
                        const double tap_q[GNSS_VT_MC_TAPS], gnss_vt_mc_out* out)
{
    if (!tr || !out || !c || !tap_i || !tap_q) return GNSS_EARG;
    // the C/N0 window index vt_mc_finish writes Zk[index_int] at (:364-365)
    if (c->index_int < 0 || c->index_int > 19 || c->snrIndex < 1) return GNSS_EARG;
    const int st = gnss_vt_mc_prepare(sg, pdi, c, codeFreq_new, nullptr, nullptr, nullptr);
    if (st) return st;
    const VtMcPrep p = vt_mc_prepare(sg->Fs, sg->codelength, pdi, c->remChip, c->codeFreq, codeFreq_new);
    double t1, t2;
    calc_loop_coef(tr->PLLBW, tr->PLLDamp, tr->PLLGain, t1, t2);
    *out = gnss_vt_mc_out{};
    // int8 I/Q byte offsets (dataPrecision * dataType = 2)
    return vt_mc_finish(sg->Fs, sg->ms, pdi, 2, t1, t2, c, p, codeFreq_new, tap_i, tap_q, out);
}

}  // extern "C"
