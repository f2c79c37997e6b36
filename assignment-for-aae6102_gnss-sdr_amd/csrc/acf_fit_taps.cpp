// acf_fit_taps.cpp — gnss_acf_fit_taps / gnss_acf_fit_taps_window: the two-path fit of an ACF on
// any tap grid (the definition is in include/gnss_mi355x.h, the arithmetic in acf_fit_taps.h), and
// what gnss_acf_fit shares with it: gnss_acf_fit_out's rows and the fit of one window on the host.
// They and the launch of acf_fit_taps.hip are handed to the driver (acf_fit_host.h has the checks
// on the windows, the host path and the device path). Built with -ffp-contract=off: every operation
// rounds on its own.
#include <cmath>

#include "acf_fit_host.h"

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

}  // namespace

int gnss::host::acf_fit_two_path_window(const AcfFttGrid& g, const double* u, const double* zI, const double* zQ,
                                        gnss_acf_fit_out* out)
{
    if (!zI || !zQ || !out_complete(out) || out->cap < 1) return GNSS_EARG;
    out->windows[0] = 1;
    store_row(out, g.n_taps, 0, 0, ftt_window(g, u, zI, zQ), zI, zQ);
    return GNSS_OK;
}

int gnss::host::acf_fit_two_path(gnss_ctx* ctx, AcfFitCall k, const AcfFttGrid& g, const double* u,
                                 gnss_acf_fit_out* out, const AcfFitLaunch& launch)
{
    const int nt = g.n_taps;
    k.out = "gnss_acf_fit_out";
    k.out_complete = out_complete(out);
    k.cap = out->cap;
    k.windows = out->windows;
    k.want_z = out->zI || out->zQ;
    k.row = kFttRow;
    return acf_fit_run(
        ctx, k,
        [=](int c, int64_t m, const double* zI, const double* zQ) {
            store_row(out, nt, c, m, ftt_window(g, u, zI, zQ), zI, zQ);
        },
        launch,
        [=](int c, int64_t m, const double* row, const double* zI, const double* zQ) {
            AcfFttRow w;
            std::memcpy(&w, row, sizeof(w));
            store_row(out, nt, c, m, w, zI, zQ);
        });
}

extern "C" {

int gnss_acf_fit_taps_window(const gnss_acf_fit_taps_cfg* cfg, const double* zI, const double* zQ,
                             gnss_acf_fit_out* out)
{
    if (!cfg || !out || grid_fault(*cfg)) return GNSS_EARG;
    return acf_fit_two_path_window(grid_of(*cfg), cfg->u, zI, zQ, out);
}

int gnss_acf_fit_taps(gnss_ctx* ctx, const gnss_acf_fit_taps_cfg* cfg, const gnss_acf_fit_taps_in* in,
                      gnss_acf_fit_out* out)
{
    if (!cfg || !in || !out) return fail(ctx, GNSS_EARG, "gnss_acf_fit_taps: a null argument");
    AcfFitCall k{};
    k.fn = "gnss_acf_fit_taps", k.cfg = "gnss_acf_fit_taps_cfg";
    k.rows = "gnss_acf_fit_taps_in.n_rows", k.max = "max_rows", k.sums = "sums";
    k.cfg_fault = (cfg->flags & ~GNSS_OUT_DEVICE) ? "an unknown flag" : grid_fault(*cfg);
    if (!in->taps || !in->n_rows || in->max_rows < 1)
        k.in_fault = "gnss_acf_fit_taps_in: the sums (taps, n_rows, max_rows)";
    k.n = cfg->n, k.n_taps = cfg->n_taps, k.prompt = cfg->prompt;
    k.ind_start = cfg->ind_start, k.numOverLap = cfg->numOverLap;
    k.u = cfg->u, k.taps = in->taps, k.n_rows = in->n_rows, k.max_rows = in->max_rows;
    k.on_device = (cfg->flags & GNSS_OUT_DEVICE) != 0;
    k.check_taps = k.timing = true;
    k.key = "acf_fit_taps";
    const AcfFttGrid g = grid_of(*cfg);
    return acf_fit_two_path(ctx, k, g, cfg->u, out, [&](const AcfFttIo& io, void* stream) {
        return acf_fit_taps_launch(AcfFttDev{io, g}, stream);
    });
}

}  // extern "C"
