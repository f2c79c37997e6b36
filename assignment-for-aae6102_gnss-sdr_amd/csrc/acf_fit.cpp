// acf_fit.cpp — gnss_acf_fit / gnss_acf_fit_window: the two-path fit of the 25-tap ACF (the
// definition is in include/gnss_mi355x.h, the arithmetic in acf_fit.h). The argument and bound
// checks, the host path (acf_fit.h's functions over the windows on up to 16 threads) and, for
// GNSS_OUT_DEVICE records, the scratch, the launch of acf_fit.hip and the rows' download. Built
// with -ffp-contract=off: every operation rounds on its own.
#include <cmath>
#include <cstring>

#include "acf.h"
#include "acf_fit.h"
#include "host.h"

using namespace gnss;
using namespace gnss::host;

static_assert(kFitTaps == GNSS_MC_TAPS && kFitMaxCh == GNSS_VT_MAX_CH, "acf_fit.h restates the header's sizes");

namespace {

// the grid's checks; nullptr: fine
const char* grid_fault(const gnss_acf_fit_cfg& c)
{
    if (c.orient != 1 && c.orient != -1) return "orient is not +1 or -1";
    if (!(c.corrSpacing > 0) || !std::isfinite(c.corrSpacing)) return "corrSpacing is not positive";
    if (!(c.p_step > 0) || !std::isfinite(c.p_step) || !(c.e_step > 0) || !std::isfinite(c.e_step))
        return "a grid step is not positive";
    if (!std::isfinite(c.p_min) || !std::isfinite(c.e_min)) return "p_min or e_min is not finite";
    if (c.p_count < 1 || c.e_count < 1) return "a grid count below 1";
    if ((int64_t)c.p_count * c.e_count > kFitMaxHyp) return "p_count * e_count above 65536";
    if (!(c.ratio_max >= 0) || !(c.gain_min >= 0)) return "ratio_max or gain_min is negative or NaN";
    return nullptr;
}

AcfFitGrid grid_of(const gnss_acf_fit_cfg& c)
{
    return AcfFitGrid{(double)c.orient, c.corrSpacing, c.p_min, c.p_step, c.e_min, c.e_step,
                      c.p_count,        c.e_count,     c.ratio_max, c.gain_min};
}

bool out_complete(const gnss_acf_fit_out* o)
{
    return o->cap >= 0 && o->windows && o->paths && o->bias && o->p1 && o->A1p_re && o->A1p_im && o->res1 && o->p0 &&
           o->e && o->A0_re && o->A0_im && o->A1_re && o->A1_im && o->res2 && o->energy;
}

// a window's row, and its coherent vector if wanted, into the output arrays
void store_row(gnss_acf_fit_out* out, int c, int64_t m, const AcfFitRow& w, const double* zI, const double* zQ)
{
    const int64_t k = (int64_t)c * out->cap + m;
    out->paths[k] = (int32_t)w.paths;
    out->bias[k] = w.bias;
    out->p1[k] = w.p1;
    out->A1p_re[k] = w.A1p_re;
    out->A1p_im[k] = w.A1p_im;
    out->res1[k] = w.res1;
    out->p0[k] = w.p0;
    out->e[k] = w.e;
    out->A0_re[k] = w.A0_re;
    out->A0_im[k] = w.A0_im;
    out->A1_re[k] = w.A1_re;
    out->A1_im[k] = w.A1_im;
    out->res2[k] = w.res2;
    out->energy[k] = w.energy;
    for (int j = 0; j < kFitTaps; j++) {
        const int64_t kz = ((int64_t)c * kFitTaps + j) * out->cap + m;
        if (out->zI) out->zI[kz] = zI[j];
        if (out->zQ) out->zQ[kz] = zQ[j];
    }
}

// window m of channel c on the host: the coherent sums a tap at a time, then the grids
void host_window(const gnss_acf_fit_cfg& cfg, const AcfFitGrid& g, const gnss_track_out& r, gnss_acf_fit_out* out,
                 int c, int64_t m)
{
    const int64_t ml = r.max_len, row = acf_window_row(m, cfg.ind_start, cfg.numOverLap);
    const double* base = r.taps + (int64_t)c * 2 * kFitTaps * ml + row;
    const double* prompt = base + (int64_t)kFitPrompt * ml;
    double zI[kFitTaps], zQ[kFitTaps];
    for (int j = 0; j < kFitTaps; j++) {
        const double* I = base + (int64_t)j * ml;
        const double* Q = base + (int64_t)(kFitTaps + j) * ml;
        double aI = 0, aQ = 0;
        for (int64_t i = 0; i < cfg.numOverLap; i++) {
            const double s = fit_sign(prompt[i]);
            aI = fit_accum(aI, s, I[i], i == 0);
            aQ = fit_accum(aQ, s, Q[i], i == 0);
        }
        zI[j] = aI;
        zQ[j] = aQ;
    }
    store_row(out, c, m, fit_window(g, zI, zQ), zI, zQ);
}

}  // namespace

extern "C" {

int gnss_acf_fit_window(const gnss_acf_fit_cfg* cfg, const double* zI, const double* zQ, gnss_acf_fit_out* out)
{
    if (!cfg || !zI || !zQ || !out || grid_fault(*cfg) || !out_complete(out) || out->cap < 1) return GNSS_EARG;
    out->windows[0] = 1;
    store_row(out, 0, 0, fit_window(grid_of(*cfg), zI, zQ), zI, zQ);
    return GNSS_OK;
}

int gnss_acf_fit(gnss_ctx* ctx, const gnss_acf_fit_cfg* cfg, const gnss_track_out* rec, int32_t n_taps,
                 gnss_acf_fit_out* out)
{
    if (!cfg || !rec || !out) return fail(ctx, GNSS_EARG, "gnss_acf_fit: a null argument");
    const int n = cfg->n;
    if (n < 1 || n > GNSS_VT_MAX_CH) return fail(ctx, GNSS_EARG, "gnss_acf_fit_cfg.n outside 1..%d", GNSS_VT_MAX_CH);
    if (n_taps != GNSS_MC_TAPS)
        return fail(ctx, GNSS_EARG, "gnss_acf_fit: %d taps (the fit reads %d)", n_taps, GNSS_MC_TAPS);
    if (cfg->numOverLap < 2 || cfg->numOverLap > 4096)
        return fail(ctx, GNSS_EARG, "gnss_acf_fit_cfg.numOverLap outside 2..4096");
    if (cfg->ind_start < 1) return fail(ctx, GNSS_EARG, "gnss_acf_fit_cfg.ind_start below 1");
    if (const char* why = grid_fault(*cfg)) return fail(ctx, GNSS_EARG, "gnss_acf_fit_cfg: %s", why);
    if (!rec->taps || !rec->len || rec->max_len < 1)
        return fail(ctx, GNSS_EARG, "gnss_acf_fit: records (taps, len, max_len)");
    if (!out_complete(out)) return fail(ctx, GNSS_EARG, "gnss_acf_fit_out: a null array");
    // every extent the loops and the kernel index with: the rows of a channel's windows lie below
    // len[c] (acf_windows), len[c] rows of a max_len series
    AcfFitDev d{};
    int64_t windows[kFitMaxCh];
    for (int c = 0; c < n; c++) {
        if (rec->len[c] < 0 || rec->len[c] > rec->max_len)
            return fail(ctx, GNSS_EARG, "gnss_acf_fit: len[%d] outside 0..max_len", c);
        windows[c] = acf_windows(rec->len[c], cfg->ind_start, cfg->numOverLap);
        if (windows[c] > out->cap)
            return fail(ctx, GNSS_EARG, "gnss_acf_fit_out.cap is smaller than channel %d's %lld windows", c,
                        (long long)windows[c]);
        d.win_base[c + 1] = d.win_base[c] + windows[c];
    }
    const int64_t total = d.win_base[n];
    if (total > 0x7fffffff) return fail(ctx, GNSS_EARG, "gnss_acf_fit: more than 2^31 - 1 windows");
    const bool on_device = (rec->flags & GNSS_OUT_DEVICE) != 0;
    if (on_device) {
        if (!ctx) return GNSS_EARG;
        if (!ctx->members.empty())
            return fail(ctx, GNSS_EARG, "gnss_acf_fit: device records on a multi-device context");
    }
    const AcfFitGrid g = grid_of(*cfg);
    for (int c = 0; c < n; c++) out->windows[c] = windows[c];
    auto channel_of = [&](int64_t w) {
        int c = 0;
        while (c + 1 < n && w >= d.win_base[c + 1]) c++;
        return c;
    };
    if (!on_device) {
        parallel_for((int)total, [&](int w) {
            const int c = channel_of(w);
            host_window(*cfg, g, *rec, out, c, w - d.win_base[c]);
        });
        return GNSS_OK;
    }
    if (total == 0) return GNSS_OK;

    HIP_TRY(hipSetDevice(ctx->device));
    const bool want_z = out->zI || out->zQ;
    DevBuf rows, z;
    HIP_TRY(rows.alloc(ctx, "acf_fit_rows", (size_t)total * kFitRow * sizeof(double)));
    if (want_z) HIP_TRY(z.alloc(ctx, "acf_fit_z", (size_t)total * 2 * kFitTaps * sizeof(double)));
    d.taps = rec->taps;
    d.max_len = rec->max_len;
    d.n = n;
    d.ind_start = cfg->ind_start;
    d.numOverLap = cfg->numOverLap;
    d.grid = g;
    d.rows = rows.as<double>();
    d.z = want_z ? z.as<double>() : nullptr;
    const int le = acf_fit_launch(d, ctx->stream);
    if (le) return fail(ctx, GNSS_EDEVICE, "gnss_acf_fit: kernel launch: %s", hipGetErrorString((hipError_t)le));
    const size_t per = (size_t)kFitRow + (want_z ? 2 * kFitTaps : 0);
    double* h = pinned_buffer<double>(ctx, "acf_fit", (size_t)total * per);
    if (!h) return fail(ctx, GNSS_EDEVICE, "gnss_acf_fit: pinned staging");
    double* hz = h + (size_t)total * kFitRow;
    HIP_TRY(hipMemcpyAsync(h, d.rows, (size_t)total * kFitRow * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (want_z)
        HIP_TRY(hipMemcpyAsync(hz, d.z, (size_t)total * 2 * kFitTaps * sizeof(double), hipMemcpyDeviceToHost,
                               ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int64_t w = 0; w < total; w++) {
        const int c = channel_of(w);
        AcfFitRow row;
        std::memcpy(&row, h + w * kFitRow, sizeof(row));
        const double* zw = hz + w * 2 * kFitTaps;  // (read by store_row only if wanted)
        store_row(out, c, w - d.win_base[c], row, zw, zw + kFitTaps);
    }
    return GNSS_OK;
}

}  // extern "C"
