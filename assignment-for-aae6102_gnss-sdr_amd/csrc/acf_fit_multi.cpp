// acf_fit_multi.cpp — gnss_acf_fit_multi / gnss_acf_fit_multi_window: the multi-ray fit of an ACF
// on any tap grid (the definition is in include/gnss_mi355x.h, the arithmetic and the order of the
// searches in acf_fit_multi.h). Its cfg checks, gnss_acf_fit_multi_out's rows, the fit of one
// window (fmm_window) and the launch of acf_fit_multi.hip, handed to the driver (acf_fit_host.h has
// the checks on the windows, the host path and the device path). Built with -ffp-contract=off:
// every operation rounds on its own.
#include <cmath>

#include "acf_fit_host.h"
#include "acf_fit_multi.h"

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

// the fit of one coherent vector, stored as window m of channel c
void fit_store(const AcfFmmPar& p, const double* u, gnss_acf_fit_multi_out* out, int c, int64_t m, const double* zI,
               const double* zQ)
{
    double rs[kFmmMaxPaths * kFttMaxTaps], r[kFmmRow];
    fmm_window(p, u, zI, zQ, rs, r);
    store_row(out, p.n_taps, c, m, r, zI, zQ);
}

}  // namespace

extern "C" {

int gnss_acf_fit_multi_window(const gnss_acf_fit_multi_cfg* cfg, const double* zI, const double* zQ,
                              gnss_acf_fit_multi_out* out)
{
    if (!cfg || !zI || !zQ || !out || par_fault(*cfg) || !out_complete(out) || out->cap < 1) return GNSS_EARG;
    out->windows[0] = 1;
    fit_store(par_of(*cfg), cfg->u, out, 0, 0, zI, zQ);
    return GNSS_OK;
}

int gnss_acf_fit_multi(gnss_ctx* ctx, const gnss_acf_fit_multi_cfg* cfg, const gnss_acf_fit_taps_in* in,
                       gnss_acf_fit_multi_out* out)
{
    if (!cfg || !in || !out) return fail(ctx, GNSS_EARG, "gnss_acf_fit_multi: a null argument");
    AcfFitCall k{};
    k.fn = "gnss_acf_fit_multi", k.cfg = "gnss_acf_fit_multi_cfg", k.out = "gnss_acf_fit_multi_out";
    k.rows = "gnss_acf_fit_taps_in.n_rows", k.max = "max_rows", k.sums = "sums";
    k.cfg_fault = (cfg->flags & ~GNSS_OUT_DEVICE) ? "an unknown flag" : par_fault(*cfg);
    if (!in->taps || !in->n_rows || in->max_rows < 1)
        k.in_fault = "gnss_acf_fit_taps_in: the sums (taps, n_rows, max_rows)";
    k.out_complete = out_complete(out);
    k.n = cfg->n, k.n_taps = cfg->n_taps, k.prompt = cfg->prompt;
    k.ind_start = cfg->ind_start, k.numOverLap = cfg->numOverLap;
    k.u = cfg->u, k.taps = in->taps, k.n_rows = in->n_rows, k.max_rows = in->max_rows;
    k.on_device = (cfg->flags & GNSS_OUT_DEVICE) != 0;
    k.check_taps = k.timing = true;
    k.cap = out->cap, k.windows = out->windows, k.want_z = out->zI || out->zQ;
    k.row = kFmmRow;
    k.key = "acf_fit_multi";
    const AcfFmmPar p = par_of(*cfg);
    const double* u = cfg->u;
    const int nt = cfg->n_taps;
    return acf_fit_run(
        ctx, k, [=](int c, int64_t m, const double* zI, const double* zQ) { fit_store(p, u, out, c, m, zI, zQ); },
        [&](const AcfFttIo& io, void* stream) { return acf_fit_multi_launch(AcfFmmDev{io, p}, stream); },
        [=](int c, int64_t m, const double* row, const double* zI, const double* zQ) {
            store_row(out, nt, c, m, row, zI, zQ);
        });
}

}  // extern "C"
