// acf_fit.cpp — gnss_acf_fit / gnss_acf_fit_window: the two-path fit of the 25-tap ACF (the
// definition is in include/gnss_mi355x.h). Its cfg checks and the mapping onto the fit of any tap
// grid: 25 taps, prompt 12, u from orient and corrSpacing (acf_fit.h's fit_u). The records
// [n][2][25][max_len] are that fit's sums as they are, so the windows' checks, the host path
// (acf_fit_taps.h's ftt_window) and the device path's shell are the shared ones (acf_fit_host.h,
// acf_fit_taps.cpp); for GNSS_OUT_DEVICE records the launch is acf_fit.hip's 25-tap kernel, whose
// rows equal the host path's bit for bit. Built with -ffp-contract=off: every operation rounds on
// its own.
#include <cmath>
#include <cstdio>

#include "acf_fit.h"
#include "acf_fit_host.h"

using namespace gnss;
using namespace gnss::host;

static_assert(kFitTaps == GNSS_MC_TAPS && kFitMaxCh == kFttMaxCh, "acf_fit.h restates the header's sizes");
static_assert(kFitRow == kFttRow && kFitMaxHyp == kFttMaxHyp, "the two kernels' rows and grids are one layout");

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

// the kernel's grid, and the same as a 25-tap grid of the general fit with its tap coordinates
AcfFitGrid grid_of(const gnss_acf_fit_cfg& c)
{
    return AcfFitGrid{(double)c.orient, c.corrSpacing, c.p_min, c.p_step, c.e_min, c.e_step,
                      c.p_count,        c.e_count,     c.ratio_max, c.gain_min};
}

AcfFttGrid taps_grid(const AcfFitGrid& g, double* u)
{
    for (int j = 0; j < kFitTaps; j++) u[j] = fit_u(g, j);
    return AcfFttGrid{kFitTaps, kFitPrompt, g.p_min,   g.p_step,    g.e_min,
                      g.e_step, g.p_count,  g.e_count, g.ratio_max, g.gain_min};
}

}  // namespace

extern "C" {

int gnss_acf_fit_window(const gnss_acf_fit_cfg* cfg, const double* zI, const double* zQ, gnss_acf_fit_out* out)
{
    if (!cfg || !out || grid_fault(*cfg)) return GNSS_EARG;
    double u[kFitTaps];
    const AcfFttGrid g = taps_grid(grid_of(*cfg), u);
    return acf_fit_two_path_window(g, u, zI, zQ, out);
}

int gnss_acf_fit(gnss_ctx* ctx, const gnss_acf_fit_cfg* cfg, const gnss_track_out* rec, int32_t n_taps,
                 gnss_acf_fit_out* out)
{
    if (!cfg || !rec || !out) return fail(ctx, GNSS_EARG, "gnss_acf_fit: a null argument");
    char taps_fault[64];
    std::snprintf(taps_fault, sizeof taps_fault, "gnss_acf_fit: %d taps (the fit reads %d)", n_taps, GNSS_MC_TAPS);
    double u[kFitTaps];
    const AcfFitGrid g25 = grid_of(*cfg);
    const AcfFttGrid g = taps_grid(g25, u);
    AcfFitCall k{};
    k.fn = "gnss_acf_fit", k.cfg = "gnss_acf_fit_cfg";
    k.rows = "gnss_acf_fit: len", k.max = "max_len", k.sums = "records";
    k.n_fault = n_taps != GNSS_MC_TAPS ? taps_fault : nullptr;
    k.cfg_fault = grid_fault(*cfg);
    if (!rec->taps || !rec->len || rec->max_len < 1) k.in_fault = "gnss_acf_fit: records (taps, len, max_len)";
    k.n = cfg->n, k.n_taps = kFitTaps, k.prompt = kFitPrompt;
    k.ind_start = cfg->ind_start, k.numOverLap = cfg->numOverLap;
    k.taps = rec->taps, k.n_rows = rec->len, k.max_rows = rec->max_len;
    k.on_device = (rec->flags & GNSS_OUT_DEVICE) != 0;
    // (u, check_taps and timing stay off: the 25-tap kernel forms u itself, and this entry never
    // checked the pointer or wrote ctx->timing)
    k.key = "acf_fit";
    return acf_fit_two_path(ctx, k, g, u, out, [&](const AcfFttIo& io, void* stream) {
        AcfFitDev d{};
        d.taps = io.taps;
        d.max_len = io.max_rows;
        d.n = io.n;
        std::memcpy(d.win_base, io.win_base, sizeof(d.win_base));
        d.ind_start = io.ind_start;
        d.numOverLap = io.numOverLap;
        d.grid = g25;
        d.rows = io.rows;
        d.z = io.z;
        return acf_fit_launch(d, stream);
    });
}

}  // extern "C"
