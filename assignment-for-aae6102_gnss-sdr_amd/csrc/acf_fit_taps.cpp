// acf_fit_taps.cpp — gnss_acf_fit_taps / gnss_acf_fit_taps_window: the two-path fit of an ACF on
// any tap grid (the definition is in include/gnss_mi355x.h, the arithmetic in acf_fit_taps.h). The
// argument and bound checks (all before any launch), the host path (acf_fit_taps.h's functions
// over the windows on up to 16 threads, a window by one thread: the bits do not depend on the
// thread count) and, for GNSS_OUT_DEVICE sums, the scratch, the launch of acf_fit_taps.hip and the
// rows' download. Built with -ffp-contract=off: every operation rounds on its own.
#include <cmath>
#include <cstring>

#include "acf_fit_taps.h"
#include "host.h"

using namespace gnss;
using namespace gnss::host;

static_assert(kFttMaxTaps == GNSS_REPLAY_MAX_TAPS && kFttMaxCh == GNSS_VT_MAX_CH,
              "acf_fit_taps.h restates the header's sizes");
static_assert(sizeof(AcfFttDev) <= 1024, "AcfFttDev goes to the kernel by value");

namespace {

// the taps', the grid's and the thresholds' checks; nullptr: fine
const char* grid_fault(const gnss_acf_fit_taps_cfg& c)
{
    if (c.n_taps < 1 || c.n_taps > GNSS_REPLAY_MAX_TAPS) return "n_taps outside 1..256";
    if (c.prompt < 0 || c.prompt >= c.n_taps) return "prompt outside 0..n_taps-1";
    if (!c.u) return "u is null";
    for (int j = 0; j < c.n_taps; j++)
        if (!std::isfinite(c.u[j])) return "a u[j] is not finite";
    if (!(c.p_step > 0) || !std::isfinite(c.p_step) || !(c.e_step > 0) || !std::isfinite(c.e_step))
        return "a grid step is not positive";
    if (!std::isfinite(c.p_min) || !std::isfinite(c.e_min)) return "p_min or e_min is not finite";
    if (c.p_count < 1 || c.e_count < 1) return "a grid count below 1";
    if ((int64_t)c.p_count * c.e_count > kFttMaxHyp) return "p_count * e_count above 65536";
    if (!(c.ratio_max >= 0) || !(c.gain_min >= 0)) return "ratio_max or gain_min is negative or NaN";
    return nullptr;
}

AcfFttGrid grid_of(const gnss_acf_fit_taps_cfg& c)
{
    return AcfFttGrid{c.n_taps, c.prompt, c.p_min, c.p_step, c.e_min, c.e_step, c.p_count, c.e_count, c.ratio_max, c.gain_min};
}

bool out_complete(const gnss_acf_fit_out* o)
{
    return o->cap >= 0 && o->windows && o->paths && o->bias && o->p1 && o->A1p_re && o->A1p_im && o->res1 && o->p0 &&
           o->e && o->A0_re && o->A0_im && o->A1_re && o->A1_im && o->res2 && o->energy;
}

// a window's row, and its coherent vector if wanted, into the output arrays
void store_row(gnss_acf_fit_out* out, int nt, int c, int64_t m, const AcfFttRow& w, const double* zI, const double* zQ)
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
    for (int j = 0; j < nt; j++) {
        const int64_t kz = ((int64_t)c * nt + j) * out->cap + m;
        if (out->zI) out->zI[kz] = zI[j];
        if (out->zQ) out->zQ[kz] = zQ[j];
    }
}

// window m of channel c on the host: the coherent sums a tap at a time, then the grids
void host_window(const gnss_acf_fit_taps_cfg& cfg, const AcfFttGrid& g, const gnss_acf_fit_taps_in& in,
                 gnss_acf_fit_out* out, int c, int64_t m)
{
    const int nt = g.n_taps;
    const int64_t mr = in.max_rows, row = ftt_window_row(m, cfg.ind_start, cfg.numOverLap);
    const double* base = in.taps + (int64_t)c * 2 * nt * mr + row;
    const double* prompt = base + (int64_t)g.prompt * mr;
    double zI[kFttMaxTaps], zQ[kFttMaxTaps];
    for (int j = 0; j < nt; j++) {
        const double* I = base + (int64_t)j * mr;
        const double* Q = base + (int64_t)(nt + j) * mr;
        double aI = 0, aQ = 0;
        for (int64_t i = 0; i < cfg.numOverLap; i++) {
            const double s = ftt_sign(prompt[i]);
            aI = ftt_accum(aI, s, I[i], i == 0);
            aQ = ftt_accum(aQ, s, Q[i], i == 0);
        }
        zI[j] = aI;
        zQ[j] = aQ;
    }
    store_row(out, nt, c, m, ftt_window(g, cfg.u, zI, zQ), zI, zQ);
}

}  // namespace

extern "C" {

int gnss_acf_fit_taps_window(const gnss_acf_fit_taps_cfg* cfg, const double* zI, const double* zQ,
                             gnss_acf_fit_out* out)
{
    if (!cfg || !zI || !zQ || !out || grid_fault(*cfg) || !out_complete(out) || out->cap < 1) return GNSS_EARG;
    out->windows[0] = 1;
    store_row(out, cfg->n_taps, 0, 0, ftt_window(grid_of(*cfg), cfg->u, zI, zQ), zI, zQ);
    return GNSS_OK;
}

int gnss_acf_fit_taps(gnss_ctx* ctx, const gnss_acf_fit_taps_cfg* cfg, const gnss_acf_fit_taps_in* in,
                      gnss_acf_fit_out* out)
{
    if (!cfg || !in || !out) return fail(ctx, GNSS_EARG, "gnss_acf_fit_taps: a null argument");
    const int n = cfg->n;
    if (n < 1 || n > GNSS_VT_MAX_CH)
        return fail(ctx, GNSS_EARG, "gnss_acf_fit_taps_cfg.n outside 1..%d", GNSS_VT_MAX_CH);
    if (cfg->numOverLap < 2 || cfg->numOverLap > 4096)
        return fail(ctx, GNSS_EARG, "gnss_acf_fit_taps_cfg.numOverLap outside 2..4096");
    if (cfg->ind_start < 1) return fail(ctx, GNSS_EARG, "gnss_acf_fit_taps_cfg.ind_start below 1");
    if (cfg->flags & ~GNSS_OUT_DEVICE) return fail(ctx, GNSS_EARG, "gnss_acf_fit_taps_cfg: an unknown flag");
    if (const char* why = grid_fault(*cfg)) return fail(ctx, GNSS_EARG, "gnss_acf_fit_taps_cfg: %s", why);
    if (!in->taps || !in->n_rows || in->max_rows < 1)
        return fail(ctx, GNSS_EARG, "gnss_acf_fit_taps_in: the sums (taps, n_rows, max_rows)");
    if (!out_complete(out)) return fail(ctx, GNSS_EARG, "gnss_acf_fit_out: a null array");
    const int nt = cfg->n_taps;
    // every extent the loops and the kernel index with: the rows of a channel's windows lie below
    // n_rows[c] (ftt_windows), n_rows[c] rows of a max_rows series
    AcfFttDev d{};
    int64_t windows[kFttMaxCh];
    for (int c = 0; c < n; c++) {
        if (in->n_rows[c] < 0 || in->n_rows[c] > in->max_rows)
            return fail(ctx, GNSS_EARG, "gnss_acf_fit_taps_in.n_rows[%d] outside 0..max_rows", c);
        windows[c] = ftt_windows(in->n_rows[c], cfg->ind_start, cfg->numOverLap);
        if (windows[c] > out->cap)
            return fail(ctx, GNSS_EARG, "gnss_acf_fit_out.cap is smaller than channel %d's %lld windows", c,
                        (long long)windows[c]);
        d.win_base[c + 1] = d.win_base[c] + windows[c];
    }
    const int64_t total = d.win_base[n];
    if (total > 0x7fffffff) return fail(ctx, GNSS_EARG, "gnss_acf_fit_taps: more than 2^31 - 1 windows");
    const bool on_device = (cfg->flags & GNSS_OUT_DEVICE) != 0;
    if (on_device) {
        if (!ctx) return fail(ctx, GNSS_EARG, "gnss_acf_fit_taps: GNSS_OUT_DEVICE needs a context");
        if (!ctx->members.empty())
            return fail(ctx, GNSS_EARG, "gnss_acf_fit_taps: device sums on a multi-device context");
        HIP_TRY(hipSetDevice(ctx->device));
        const size_t bytes = (size_t)n * 2 * (size_t)nt * (size_t)in->max_rows * sizeof(double);
        if (!device_memory_of(in->taps, bytes, ctx->device))
            return fail(ctx, GNSS_EARG, "gnss_acf_fit_taps_in.taps is not [n][2][n_taps][max_rows] of the context's device");
    }
    const AcfFttGrid g = grid_of(*cfg);
    for (int c = 0; c < n; c++) out->windows[c] = windows[c];
    auto channel_of = [&](int64_t w) {
        int c = 0;
        while (c + 1 < n && w >= d.win_base[c + 1]) c++;
        return c;
    };
    if (!on_device) {
        parallel_for((int)total, [&](int w) {
            const int c = channel_of(w);
            host_window(*cfg, g, *in, out, c, w - d.win_base[c]);
        });
        return GNSS_OK;
    }
    ctx->timing = gnss_timing{};
    if (total == 0) return GNSS_OK;

    const bool want_z = out->zI || out->zQ;
    DevBuf rows, z, u;
    HIP_TRY(rows.alloc(ctx, "acf_fit_taps_rows", (size_t)total * kFttRow * sizeof(double)));
    if (want_z) HIP_TRY(z.alloc(ctx, "acf_fit_taps_z", (size_t)total * 2 * nt * sizeof(double)));
    HIP_TRY(u.alloc(ctx, "acf_fit_taps_u", (size_t)nt * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(u.p, cfg->u, (size_t)nt * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // (the host array is pageable: the copy has left it)
    d.taps = in->taps;
    d.u = u.as<double>();
    d.max_rows = in->max_rows;
    d.n = n;
    d.ind_start = cfg->ind_start;
    d.numOverLap = cfg->numOverLap;
    d.grid = g;
    d.rows = rows.as<double>();
    d.z = want_z ? z.as<double>() : nullptr;
    Events ev;
    HIP_TRY(hipEventRecord(ev.a, ctx->stream));
    const int le = acf_fit_taps_launch(d, ctx->stream);
    if (le) return fail(ctx, GNSS_EDEVICE, "gnss_acf_fit_taps: kernel launch: %s", hipGetErrorString((hipError_t)le));
    HIP_TRY(hipEventRecord(ev.b, ctx->stream));
    const size_t per = (size_t)kFttRow + (want_z ? 2 * (size_t)nt : 0);
    double* h = pinned_buffer<double>(ctx, "acf_fit_taps", (size_t)total * per);
    if (!h) return fail(ctx, GNSS_EDEVICE, "gnss_acf_fit_taps: pinned staging");
    double* hz = h + (size_t)total * kFttRow;
    HIP_TRY(hipMemcpyAsync(h, d.rows, (size_t)total * kFttRow * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (want_z)
        HIP_TRY(hipMemcpyAsync(hz, d.z, (size_t)total * 2 * nt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->timing.track_kernel_ms = ev.ms();
    ctx->timing.track_launches = 1;
    for (int64_t w = 0; w < total; w++) {
        const int c = channel_of(w);
        AcfFttRow row;
        std::memcpy(&row, h + w * kFttRow, sizeof(row));
        const double* zw = hz + w * 2 * nt;  // (read by store_row only if wanted)
        store_row(out, nt, c, w - d.win_base[c], row, zw, zw + nt);
    }
    return GNSS_OK;
}

}  // extern "C"
