// acf_ext.cpp — gnss_acf_features_ext / gnss_acf_twiddle: F6-F8 of ACF/CalculateFeatures.m beside
// gnss_acf_features' outputs (the definition is in include/gnss_mi355x.h, the arithmetic in
// acf_ext.h). The checks of the added parameters and the twiddle table here; the pass itself is
// gnss_acf_features' (acf.cpp: acf_features_run, channels over up to 16 threads), which calls back
// for a channel's windows on the host path and, for GNSS_OUT_DEVICE records, for the table's
// upload, the launch of acf_ext.hip and the download. Built with -ffp-contract=off: every
// operation rounds on its own.
#include <cmath>
#include <vector>

#include "acf.h"
#include "acf_ext.h"
#include "host.h"

using namespace gnss;
using namespace gnss::host;

static_assert(kExtMaxCh == GNSS_VT_MAX_CH && kExtMaxCh == kAcfMaxCh, "acf_ext.h restates the header's sizes");

namespace {

// the table as pairs (c[t], s[t]): cos and sin of (2 pi t) / N from the C library
void twiddle_pairs(int N, double* tw)
{
    for (int t = 0; t < N; t++) {
        const double a = (2.0 * 3.141592653589793238 * (double)t) / (double)N;
        tw[2 * t] = std::cos(a);
        tw[2 * t + 1] = std::sin(a);
    }
}

}  // namespace

void gnss::host::acf_ext_host_channel(const AcfExtPlan& p, int c, int64_t cap, int64_t windows, int64_t ind_start,
                                      int64_t numOverLap, const uint8_t* cnt, const double* meanMax)
{
    std::vector<double> y((size_t)p.hist);
    for (int64_t m = 0; m < windows; m++) {
        const uint8_t* rc = cnt + acf_window_row(m, ind_start, numOverLap);
        int64_t sum = 0;
        for (int64_t i = 0; i < numOverLap; i++) sum += rc[i];
        const int H = acf_ext_len(m, p.hist, p.fill);
        for (int i = 0; i < H; i++) y[i] = acf_ext_hist(meanMax, m, H, i);
        const double mean = acf_ext_mean(y.data(), H);
        for (int i = 0; i < H; i++) y[i] = y[i] - mean;
        AcfExtBest b;
        for (int k = 0; k <= p.N / 2; k++) acf_ext_take(b, acf_ext_bin(y.data(), H, p.tw, k, p.N), k);
        const AcfExtRow r = acf_ext_row(sum, numOverLap, b, p.fs, p.N);
        const int64_t o = (int64_t)c * cap + m;
        p.numMLC[o] = r.numMLC;
        p.fftFreq[o] = r.fftFreq;
        p.fftMag[o] = r.fftMag;
    }
}

int gnss::host::acf_ext_device(gnss_ctx* ctx, const AcfExtPlan& p, const AcfDev& d, int64_t cap)
{
    const int64_t total = d.win_base[d.n];
    if (total == 0) return GNSS_OK;
    DevBuf tw, out;
    HIP_TRY(tw.alloc(ctx, "acf_ext_tw", (size_t)2 * p.N * sizeof(double)));
    HIP_TRY(out.alloc(ctx, "acf_ext_out", (size_t)3 * total * sizeof(double)));
    double* h = pinned_buffer<double>(ctx, "acf_ext", (size_t)2 * p.N + (size_t)3 * total);
    if (!h) return fail(ctx, GNSS_EDEVICE, "gnss_acf_features_ext: pinned staging");
    double* htw = h + (size_t)3 * total;
    for (int i = 0; i < 2 * p.N; i++) htw[i] = p.tw[i];
    HIP_TRY(hipMemcpyAsync(tw.p, htw, (size_t)2 * p.N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    AcfExtDev e{};
    e.meanMax = d.feat;  // the first of acf_window_kernel's five series
    e.cnt = d.cnt;
    e.tw = tw.as<double>();
    e.max_len = d.max_len;
    e.n = d.n;
    for (int c = 0; c <= d.n; c++) e.win_base[c] = d.win_base[c];
    e.ind_start = d.ind_start;
    e.numOverLap = d.numOverLap;
    e.hist = p.hist;
    e.N = p.N;
    e.fill = p.fill;
    e.fs = p.fs;
    e.out = out.as<double>();
    const int le = acf_spectrum_launch(e, ctx->stream);
    if (le)
        return fail(ctx, GNSS_EDEVICE, "gnss_acf_features_ext: kernel launch: %s", hipGetErrorString((hipError_t)le));
    HIP_TRY(hipMemcpyAsync(h, e.out, (size_t)3 * total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int c = 0; c < d.n; c++)
        for (int64_t m = 0; m < d.windows[c]; m++) {
            const int64_t w = d.win_base[c] + m, o = (int64_t)c * cap + m;
            p.numMLC[o] = h[w];
            p.fftFreq[o] = h[total + w];
            p.fftMag[o] = h[2 * total + w];
        }
    return GNSS_OK;
}

extern "C" {

int gnss_acf_twiddle(int32_t fft_n, double* c, double* s)
{
    if (fft_n < 2 || fft_n > kExtMaxN || !c || !s) return GNSS_EARG;
    std::vector<double> tw((size_t)2 * fft_n);
    twiddle_pairs(fft_n, tw.data());
    for (int t = 0; t < fft_n; t++) {
        c[t] = tw[2 * t];
        s[t] = tw[2 * t + 1];
    }
    return GNSS_OK;
}

int gnss_acf_features_ext(gnss_ctx* ctx, const gnss_acf_cfg* cfg, const gnss_acf_ext_cfg* xcfg,
                          const gnss_track_out* rec, int32_t n_taps, gnss_acf_out* out, gnss_acf_ext_out* ext)
{
    if (!cfg || !xcfg || !rec || !out || !ext) return fail(ctx, GNSS_EARG, "gnss_acf_features_ext: a null argument");
    if (xcfg->fft_hist < 2 || xcfg->fft_hist > kExtMaxHist)
        return fail(ctx, GNSS_EARG, "gnss_acf_ext_cfg.fft_hist outside 2..%d", kExtMaxHist);
    if (xcfg->fft_n < xcfg->fft_hist || xcfg->fft_n > kExtMaxN)
        return fail(ctx, GNSS_EARG, "gnss_acf_ext_cfg.fft_n outside fft_hist..%d", kExtMaxN);
    if (xcfg->fft_fill != 0 && xcfg->fft_fill != 1) return fail(ctx, GNSS_EARG, "gnss_acf_ext_cfg.fft_fill is not 0 or 1");
    if (!std::isfinite(xcfg->fs) || !(xcfg->fs > 0)) return fail(ctx, GNSS_EARG, "gnss_acf_ext_cfg.fs is not positive");
    if (!ext->numMLC || !ext->fftFreq || !ext->fftMag) return fail(ctx, GNSS_EARG, "gnss_acf_ext_out: a null array");
    std::vector<double> tw((size_t)2 * xcfg->fft_n);
    twiddle_pairs(xcfg->fft_n, tw.data());
    const AcfExtPlan plan{xcfg->fft_hist, xcfg->fft_n, xcfg->fft_fill, xcfg->fs,
                          tw.data(),      ext->numMLC, ext->fftFreq,   ext->fftMag};
    return acf_features_run(ctx, cfg, rec, n_taps, out, &plan);
}

}  // extern "C"
