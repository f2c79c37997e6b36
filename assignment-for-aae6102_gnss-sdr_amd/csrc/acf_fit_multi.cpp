// acf_fit_multi.cpp — gnss_acf_fit_multi / gnss_acf_fit_multi_window: the multi-ray fit of an ACF
// on any tap grid (the definition is in include/gnss_mi355x.h, the arithmetic and the order of the
// searches in acf_fit_multi.h). The argument and bound checks (all before any launch), the host
// path (acf_fit_multi.h's fmm_window over the windows on up to 16 threads, a window by one thread:
// the bits do not depend on the thread count) and, for GNSS_OUT_DEVICE sums, the scratch, the
// launch of acf_fit_multi.hip and the rows' download. Built with -ffp-contract=off: every operation
// rounds on its own.
#include <cmath>
#include <cstring>

#include "acf_fit_multi.h"
#include "host.h"

using namespace gnss;
using namespace gnss::host;

static_assert(kFmmMaxPaths == GNSS_ACF_MULTI_MAX_PATHS, "acf_fit_multi.h restates the header's size");
static_assert(sizeof(AcfFmmDev) <= 1024, "AcfFmmDev goes to the kernel by value");

namespace {

// the taps', the grid's and the search parameters' checks; nullptr: fine
const char* par_fault(const gnss_acf_fit_multi_cfg& c)
{
    if (c.n_taps < 1 || c.n_taps > GNSS_REPLAY_MAX_TAPS) return "n_taps outside 1..256";
    if (c.prompt < 0 || c.prompt >= c.n_taps) return "prompt outside 0..n_taps-1";
    if (!c.u) return "u is null";
    for (int j = 0; j < c.n_taps; j++)
        if (!std::isfinite(c.u[j])) return "a u[j] is not finite";
    if (!(c.q_step > 0) || !std::isfinite(c.q_step)) return "q_step is not positive and finite";
    if (!std::isfinite(c.q_min)) return "q_min is not finite";
    if (c.q_count < 1 || c.q_count > kFmmMaxQ) return "q_count outside 1..4096";
    if (c.max_paths < 1 || c.max_paths > kFmmMaxPaths) return "max_paths outside 1..4";
    if (c.sweeps < 0 || c.sweeps > kFmmMaxSweeps) return "sweeps outside 0..16";
    if (c.sep_min < 1 || c.sep_min > c.q_count) return "sep_min outside 1..q_count";
    if (!(c.gain_min >= 0)) return "gain_min is negative or NaN";
    return nullptr;
}

AcfFmmPar par_of(const gnss_acf_fit_multi_cfg& c)
{
    return AcfFmmPar{c.n_taps, c.prompt, c.q_min, c.q_step, c.q_count, c.max_paths, c.sweeps, c.sep_min, c.gain_min};
}

bool out_complete(const gnss_acf_fit_multi_out* o)
{
    return o->cap >= 0 && o->windows && o->paths && o->searches && o->bias && o->q && o->A_re && o->A_im && o->res &&
           o->energy;
}

// a window's row, and its coherent vector if wanted, into the output arrays
void store_row(gnss_acf_fit_multi_out* out, int nt, int c, int64_t m, const double* row, const double* zI,
               const double* zQ)
{
    AcfFmmRow w;
    std::memcpy(&w, row, sizeof(w));
    const int64_t cap = out->cap, k = (int64_t)c * cap + m;
    out->paths[k] = (int32_t)w.paths;
    out->searches[k] = (int32_t)w.searches;
    out->bias[k] = w.q[0];
    out->energy[k] = w.energy;
    for (int l = 0; l < kFmmMaxPaths; l++) {
        const int64_t kl = ((int64_t)c * kFmmMaxPaths + l) * cap + m;
        out->q[kl] = w.q[l];
        out->A_re[kl] = w.A_re[l];
        out->A_im[kl] = w.A_im[l];
    }
    for (int l = 0; l <= kFmmMaxPaths; l++) out->res[((int64_t)c * (kFmmMaxPaths + 1) + l) * cap + m] = w.res[l];
    for (int j = 0; j < nt; j++) {
        const int64_t kz = ((int64_t)c * nt + j) * cap + m;
        if (out->zI) out->zI[kz] = zI[j];
        if (out->zQ) out->zQ[kz] = zQ[j];
    }
}

// window m of channel c on the host: the coherent sums a tap at a time, then the fit
void host_window(const gnss_acf_fit_multi_cfg& cfg, const AcfFmmPar& p, const gnss_acf_fit_taps_in& in,
                 gnss_acf_fit_multi_out* out, int c, int64_t m)
{
    const int nt = p.n_taps;
    const int64_t mr = in.max_rows, row = ftt_window_row(m, cfg.ind_start, cfg.numOverLap);
    const double* base = in.taps + (int64_t)c * 2 * nt * mr + row;
    const double* prompt = base + (int64_t)p.prompt * mr;
    double zI[kFttMaxTaps], zQ[kFttMaxTaps], rs[kFmmMaxPaths * kFttMaxTaps], r[kFmmRow];
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
    fmm_window(p, cfg.u, zI, zQ, rs, r);
    store_row(out, nt, c, m, r, zI, zQ);
}

}  // namespace

extern "C" {

int gnss_acf_fit_multi_window(const gnss_acf_fit_multi_cfg* cfg, const double* zI, const double* zQ,
                              gnss_acf_fit_multi_out* out)
{
    if (!cfg || !zI || !zQ || !out || par_fault(*cfg) || !out_complete(out) || out->cap < 1) return GNSS_EARG;
    double rs[kFmmMaxPaths * kFttMaxTaps], r[kFmmRow];
    fmm_window(par_of(*cfg), cfg->u, zI, zQ, rs, r);
    out->windows[0] = 1;
    store_row(out, cfg->n_taps, 0, 0, r, zI, zQ);
    return GNSS_OK;
}

int gnss_acf_fit_multi(gnss_ctx* ctx, const gnss_acf_fit_multi_cfg* cfg, const gnss_acf_fit_taps_in* in,
                       gnss_acf_fit_multi_out* out)
{
    if (!cfg || !in || !out) return fail(ctx, GNSS_EARG, "gnss_acf_fit_multi: a null argument");
    const int n = cfg->n;
    if (n < 1 || n > GNSS_VT_MAX_CH)
        return fail(ctx, GNSS_EARG, "gnss_acf_fit_multi_cfg.n outside 1..%d", GNSS_VT_MAX_CH);
    if (cfg->numOverLap < 2 || cfg->numOverLap > 4096)
        return fail(ctx, GNSS_EARG, "gnss_acf_fit_multi_cfg.numOverLap outside 2..4096");
    if (cfg->ind_start < 1) return fail(ctx, GNSS_EARG, "gnss_acf_fit_multi_cfg.ind_start below 1");
    if (cfg->flags & ~GNSS_OUT_DEVICE) return fail(ctx, GNSS_EARG, "gnss_acf_fit_multi_cfg: an unknown flag");
    if (const char* why = par_fault(*cfg)) return fail(ctx, GNSS_EARG, "gnss_acf_fit_multi_cfg: %s", why);
    if (!in->taps || !in->n_rows || in->max_rows < 1)
        return fail(ctx, GNSS_EARG, "gnss_acf_fit_taps_in: the sums (taps, n_rows, max_rows)");
    if (!out_complete(out)) return fail(ctx, GNSS_EARG, "gnss_acf_fit_multi_out: a null array");
    const int nt = cfg->n_taps;
    // every extent the loops and the kernel index with: the rows of a channel's windows lie below
    // n_rows[c] (ftt_windows), n_rows[c] rows of a max_rows series
    AcfFmmDev d{};
    int64_t windows[kFttMaxCh];
    for (int c = 0; c < n; c++) {
        if (in->n_rows[c] < 0 || in->n_rows[c] > in->max_rows)
            return fail(ctx, GNSS_EARG, "gnss_acf_fit_taps_in.n_rows[%d] outside 0..max_rows", c);
        windows[c] = ftt_windows(in->n_rows[c], cfg->ind_start, cfg->numOverLap);
        if (windows[c] > out->cap)
            return fail(ctx, GNSS_EARG, "gnss_acf_fit_multi_out.cap is smaller than channel %d's %lld windows", c,
                        (long long)windows[c]);
        d.win_base[c + 1] = d.win_base[c] + windows[c];
    }
    const int64_t total = d.win_base[n];
    if (total > 0x7fffffff) return fail(ctx, GNSS_EARG, "gnss_acf_fit_multi: more than 2^31 - 1 windows");
    const bool on_device = (cfg->flags & GNSS_OUT_DEVICE) != 0;
    if (on_device) {
        if (!ctx) return fail(ctx, GNSS_EARG, "gnss_acf_fit_multi: GNSS_OUT_DEVICE needs a context");
        if (!ctx->members.empty())
            return fail(ctx, GNSS_EARG, "gnss_acf_fit_multi: device sums on a multi-device context");
        HIP_TRY(hipSetDevice(ctx->device));
        const size_t bytes = (size_t)n * 2 * (size_t)nt * (size_t)in->max_rows * sizeof(double);
        if (!device_memory_of(in->taps, bytes, ctx->device))
            return fail(ctx, GNSS_EARG, "gnss_acf_fit_taps_in.taps is not [n][2][n_taps][max_rows] of the context's device");
    }
    const AcfFmmPar p = par_of(*cfg);
    for (int c = 0; c < n; c++) out->windows[c] = windows[c];
    auto channel_of = [&](int64_t w) {
        int c = 0;
        while (c + 1 < n && w >= d.win_base[c + 1]) c++;
        return c;
    };
    if (!on_device) {
        parallel_for((int)total, [&](int w) {
            const int c = channel_of(w);
            host_window(*cfg, p, *in, out, c, w - d.win_base[c]);
        });
        return GNSS_OK;
    }
    ctx->timing = gnss_timing{};
    if (total == 0) return GNSS_OK;

    const bool want_z = out->zI || out->zQ;
    DevBuf rows, z, u;
    HIP_TRY(rows.alloc(ctx, "acf_fit_multi_rows", (size_t)total * kFmmRow * sizeof(double)));
    if (want_z) HIP_TRY(z.alloc(ctx, "acf_fit_multi_z", (size_t)total * 2 * nt * sizeof(double)));
    HIP_TRY(u.alloc(ctx, "acf_fit_multi_u", (size_t)nt * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(u.p, cfg->u, (size_t)nt * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // (the host array is pageable: the copy has left it)
    d.taps = in->taps;
    d.u = u.as<double>();
    d.max_rows = in->max_rows;
    d.n = n;
    d.ind_start = cfg->ind_start;
    d.numOverLap = cfg->numOverLap;
    d.par = p;
    d.rows = rows.as<double>();
    d.z = want_z ? z.as<double>() : nullptr;
    Events ev;
    HIP_TRY(hipEventRecord(ev.a, ctx->stream));
    const int le = acf_fit_multi_launch(d, ctx->stream);
    if (le) return fail(ctx, GNSS_EDEVICE, "gnss_acf_fit_multi: kernel launch: %s", hipGetErrorString((hipError_t)le));
    HIP_TRY(hipEventRecord(ev.b, ctx->stream));
    const size_t per = (size_t)kFmmRow + (want_z ? 2 * (size_t)nt : 0);
    double* h = pinned_buffer<double>(ctx, "acf_fit_multi", (size_t)total * per);
    if (!h) return fail(ctx, GNSS_EDEVICE, "gnss_acf_fit_multi: pinned staging");
    double* hz = h + (size_t)total * kFmmRow;
    HIP_TRY(hipMemcpyAsync(h, d.rows, (size_t)total * kFmmRow * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (want_z)
        HIP_TRY(hipMemcpyAsync(hz, d.z, (size_t)total * 2 * nt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->timing.track_kernel_ms = ev.ms();
    ctx->timing.track_launches = 1;
    for (int64_t w = 0; w < total; w++) {
        const int c = channel_of(w);
        const double* zw = hz + w * 2 * nt;  // (read by store_row only if wanted)
        store_row(out, nt, c, w - d.win_base[c], h + w * kFmmRow, zw, zw + nt);
    }
    return GNSS_OK;
}

}  // extern "C"
