// acf.cpp — gnss_acf_features: ACF/CalculateFeatures.m as a pass over the 25-tap records (the
// definition is in include/gnss_mi355x.h, the arithmetic in acf.h). The argument and bound
// checks, the host path (acf.h's functions in loops) and, for GNSS_OUT_DEVICE records, the
// scratch, the launches of acf.hip and the features' download. F1 and expectedCorr are computed
// here on both paths. gnss_acf_features_ext (acf_ext.cpp) runs the same pass with the row pass
// counting acf_ext.h's local maxima as well. Built with -ffp-contract=off: every operation
// rounds on its own.
#include <cmath>
#include <cstring>

#include "acf.h"
#include "acf_ext.h"
#include "host.h"

using namespace gnss;
using namespace gnss::host;

static_assert(kAcfTaps == GNSS_MC_TAPS && kAcfMaxCh == GNSS_VT_MAX_CH, "acf.h restates the header's sizes");

namespace {

// expectedCorr = a(1) + a(2)*ele^1 + a(3)*ele^2 + a(4)*ele^3 (CalculateFeatures.m:188)
double expected_corr(const double* a, double ele)
{
    return a[0] + a[1] * std::pow(ele, 1) + a[2] * std::pow(ele, 2) + a[3] * std::pow(ele, 3);
}

// the window's five sums into the output row, with F1 and F2 (:276-282)
void store_window(const gnss_acf_cfg& cfg, gnss_acf_out* out, int c, int64_t m, const AcfWindow& w)
{
    const int64_t k = (int64_t)c * out->cap + m;
    out->meanMax[k] = w.meanMax;
    out->F1[k] = w.meanMax / expected_corr(cfg.a, cfg.ele[c]);
    out->F2[k] = -(w.meanDelay + 0.00) * 1;
    out->varDelay[k] = w.varDelay;
    out->meanCodeDisc[k] = w.meanCodeDisc;
    out->varCodeDisc[k] = w.varCodeDisc;
}

// one channel on the host: the row pass a tap at a time (each series is contiguous), then the
// windows; with `ext` the rows' local-maximum counts beside the arg-max, and F6-F8 after the windows
void host_channel(const gnss_acf_cfg& cfg, const gnss_track_out& r, gnss_acf_out* out, int c, double cenDelay,
                  const AcfExtPlan* ext)
{
    const int64_t L = r.len[c], ml = r.max_len;
    std::vector<double> pm((size_t)L);
    std::vector<AcfPeak> peak((size_t)L);
    std::vector<AcfMlc> mlc(ext ? (size_t)L : 0);
    std::vector<uint8_t> idx_own;
    uint8_t* idx = out->maxCorrInd ? out->maxCorrInd + (int64_t)c * ml : nullptr;
    if (!idx) {
        idx_own.resize((size_t)L);
        idx = idx_own.data();
    }
    for (int j = 0; j < kAcfTaps; j++) {
        const double* I = r.taps + (((int64_t)c * 2 + 0) * kAcfTaps + j) * ml;
        const double* Q = r.taps + (((int64_t)c * 2 + 1) * kAcfTaps + j) * ml;
        double* corr = out->corr ? out->corr + ((int64_t)c * kAcfTaps + j) * ml : nullptr;
        for (int64_t i = 0; i < L; i++) {
            const double m = acf_mag(I[i], Q[i]);
            acf_peak_take(peak[i], m, j + 1);
            if (j == kAcfPrompt) pm[i] = m;
            if (corr) corr[i] = m;
            if (ext) acf_mlc_take(mlc[i], m);
        }
    }
    for (int64_t i = 0; i < L; i++) idx[i] = (uint8_t)peak[i].idx;
    const double* disc = r.rec + ((int64_t)c * GNSS_NFIELDS + GNSS_F_DLLdiscri) * ml;
    for (int64_t m = 0; m < out->windows[c]; m++) {
        const int64_t row = acf_window_row(m, cfg.ind_start, cfg.numOverLap);
        store_window(cfg, out, c, m,
                     acf_window(pm.data() + row, idx + row, disc + row, cfg.numOverLap, m == 0, cfg.corrSpacing,
                                cenDelay));
    }
    if (ext) {
        std::vector<uint8_t> cnt((size_t)L);
        for (int64_t i = 0; i < L; i++) cnt[i] = (uint8_t)mlc[i].cnt;
        acf_ext_host_channel(*ext, c, out->cap, out->windows[c], cfg.ind_start, cfg.numOverLap, cnt.data(),
                             out->meanMax + (int64_t)c * out->cap);
    }
}

}  // namespace

int gnss::host::acf_features_run(gnss_ctx* ctx, const gnss_acf_cfg* cfg, const gnss_track_out* rec, int32_t n_taps,
                                 gnss_acf_out* out, const AcfExtPlan* ext)
{
    if (!cfg || !rec || !out) return fail(ctx, GNSS_EARG, "gnss_acf_features: a null argument");
    const int n = cfg->n;
    if (n < 1 || n > GNSS_VT_MAX_CH) return fail(ctx, GNSS_EARG, "gnss_acf_cfg.n outside 1..%d", GNSS_VT_MAX_CH);
    if (n_taps != GNSS_MC_TAPS)
        return fail(ctx, GNSS_EARG, "gnss_acf_features: %d taps (the script reads %d)", n_taps, GNSS_MC_TAPS);
    if (cfg->numOverLap < 2 || cfg->numOverLap > 4096)
        return fail(ctx, GNSS_EARG, "gnss_acf_cfg.numOverLap outside 2..4096");
    if (cfg->ind_start < 1) return fail(ctx, GNSS_EARG, "gnss_acf_cfg.ind_start below 1");
    if (!(cfg->corrSpacing > 0)) return fail(ctx, GNSS_EARG, "gnss_acf_cfg.corrSpacing is not positive");
    if (!rec->rec || !rec->taps || !rec->len || rec->max_len < 1)
        return fail(ctx, GNSS_EARG, "gnss_acf_features: records (rec, taps, len, max_len)");
    if (out->cap < 0 || !out->windows || !out->meanMax || !out->F1 || !out->F2 || !out->varDelay ||
        !out->meanCodeDisc || !out->varCodeDisc)
        return fail(ctx, GNSS_EARG, "gnss_acf_out: a null array");
    // every extent the loops and the kernels index with: len[c] rows of a max_len series, and the
    // rows of a channel's windows below len[c] (acf_windows)
    AcfDev d{};
    for (int c = 0; c < n; c++) {
        if (rec->len[c] < 0 || rec->len[c] > rec->max_len)
            return fail(ctx, GNSS_EARG, "gnss_acf_features: len[%d] outside 0..max_len", c);
        d.len[c] = rec->len[c];
        d.windows[c] = acf_windows(rec->len[c], cfg->ind_start, cfg->numOverLap);
        if (d.windows[c] > out->cap)
            return fail(ctx, GNSS_EARG, "gnss_acf_out.cap is smaller than channel %d's %lld windows", c,
                        (long long)d.windows[c]);
        d.win_base[c + 1] = d.win_base[c] + d.windows[c];
    }
    if (ext && d.win_base[n] > 0x7fffffff)  // (acf_spectrum_kernel: one block per window)
        return fail(ctx, GNSS_EARG, "gnss_acf_features_ext: more than 2^31 - 1 windows");
    const bool on_device = (rec->flags & GNSS_OUT_DEVICE) != 0;
    if (on_device) {
        if (!ctx) return GNSS_EARG;
        if (!ctx->members.empty())
            return fail(ctx, GNSS_EARG, "gnss_acf_features: device records on a multi-device context");
    }
    const double cenDelay = acf_cen_delay(cfg->maxDelay, cfg->corrSpacing);
    for (int c = 0; c < n; c++) out->windows[c] = d.windows[c];
    if (!on_device) {
        parallel_for(n, [&](int c) { host_channel(*cfg, *rec, out, c, cenDelay, ext); });
        return GNSS_OK;
    }

    HIP_TRY(hipSetDevice(ctx->device));
    const int64_t ml = rec->max_len, total = d.win_base[n];
    DevBuf pm, idx, feat, cnt;
    HIP_TRY(pm.alloc(ctx, "acf_pm", (size_t)n * ml * sizeof(double)));
    if (!out->maxCorrInd) HIP_TRY(idx.alloc(ctx, "acf_idx", (size_t)n * ml));
    HIP_TRY(feat.alloc(ctx, "acf_feat", (size_t)5 * total * sizeof(double)));
    if (ext) HIP_TRY(cnt.alloc(ctx, "acf_cnt", (size_t)n * ml));
    d.taps = rec->taps;
    d.rec = rec->rec;
    d.max_len = ml;
    d.n = n;
    d.nfields = GNSS_NFIELDS;
    d.field_d = GNSS_F_DLLdiscri;
    d.ind_start = cfg->ind_start;
    d.numOverLap = cfg->numOverLap;
    d.corrSpacing = cfg->corrSpacing;
    d.cenDelay = cenDelay;
    d.pm = pm.as<double>();
    d.idx = out->maxCorrInd ? out->maxCorrInd : idx.as<uint8_t>();
    d.corr = out->corr;
    d.feat = feat.as<double>();
    d.cnt = ext ? cnt.as<uint8_t>() : nullptr;
    auto aligned16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool vec2 = ml % 2 == 0 && aligned16(d.taps) && aligned16(d.pm) && aligned16(d.corr);
    const int le = acf_launch(d, vec2, ctx->stream);
    if (le)
        return fail(ctx, GNSS_EDEVICE, "gnss_acf_features: kernel launch: %s", hipGetErrorString((hipError_t)le));
    double* h = nullptr;
    if (total > 0) {
        h = pinned_buffer<double>(ctx, "acf_feat", (size_t)5 * total);
        if (!h) return fail(ctx, GNSS_EDEVICE, "gnss_acf_features: pinned staging");
        HIP_TRY(hipMemcpyAsync(h, d.feat, (size_t)5 * total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (ext)
        if (const int st = acf_ext_device(ctx, *ext, d, out->cap)) return st;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int c = 0; c < n; c++)
        for (int64_t m = 0; m < d.windows[c]; m++) {
            const int64_t w = d.win_base[c] + m;
            store_window(*cfg, out, c, m,
                         AcfWindow{h[w], h[total + w], h[2 * total + w], h[3 * total + w], h[4 * total + w]});
        }
    return GNSS_OK;
}

extern "C" {

int gnss_acf_features(gnss_ctx* ctx, const gnss_acf_cfg* cfg, const gnss_track_out* rec, int32_t n_taps,
                      gnss_acf_out* out)
{
    return acf_features_run(ctx, cfg, rec, n_taps, out, nullptr);
}

}  // extern "C"
