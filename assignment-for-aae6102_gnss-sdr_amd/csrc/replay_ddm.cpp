// replay_ddm.cpp — gnss_replay_ddm: the delay-Doppler map over replayed rows (the definition is in
// include/gnss_mi355x.h, the arithmetic in replay_ddm.h). Here: every check (all before any
// launch), the rows' time table, the host path (replay_ddm.h's functions over the windows on up to
// 16 threads, a window by one thread: the bits do not depend on the thread count) and, for
// GNSS_OUT_DEVICE sums, the uploads, the launch of replay_ddm.hip and the download of the map and
// the peaks. Built with -ffp-contract=off: every operation rounds on its own.
#include <cmath>
#include <cstring>
#include <vector>

#include "host.h"
#include "replay_ddm.h"

using namespace gnss;
using namespace gnss::host;

static_assert(kDdmMaxTaps == GNSS_REPLAY_MAX_TAPS && kDdmMaxDopp == GNSS_DDM_MAX_DOPP && kDdmMaxChan == GNSS_MAX_SV,
              "replay_ddm.h restates the header's sizes");
static_assert(sizeof(DdmArgs) <= 1024, "DdmArgs goes to the kernels by value");

namespace {

// the configuration's checks; nullptr: fine
const char* cfg_fault(const gnss_replay_ddm_cfg& c)
{
    if (c.n < 1 || c.n > GNSS_MAX_SV) return "n outside 1..64";
    if (c.n_taps < 1 || c.n_taps > GNSS_REPLAY_MAX_TAPS) return "n_taps outside 1..256";
    if (c.prompt < -1 || c.prompt >= c.n_taps) return "prompt outside -1..n_taps-1";
    if (c.rows_per_window < 2 || c.rows_per_window > kDdmMaxRows) return "rows_per_window outside 2..4096";
    if (c.n_dopp < 1 || c.n_dopp > GNSS_DDM_MAX_DOPP) return "n_dopp outside 1..256";
    if (c.flags & ~(GNSS_OUT_DEVICE | GNSS_DDM_MAP_DEVICE)) return "an unknown flag";
    if ((c.flags & GNSS_DDM_MAP_DEVICE) && !(c.flags & GNSS_OUT_DEVICE)) return "GNSS_DDM_MAP_DEVICE without GNSS_OUT_DEVICE";
    if (!c.dopp_hz || !c.u) return "dopp_hz or u is null";
    for (int m = 0; m < c.n_dopp; m++)
        if (!std::isfinite(c.dopp_hz[m]) || std::fabs(c.dopp_hz[m]) > kDdmMaxHz) return "a dopp_hz[m] is not finite within +-1e5";
    for (int j = 0; j < c.n_taps; j++)
        if (!std::isfinite(c.u[j])) return "a u[j] is not finite";
    if (!(c.excl_chips >= 0) || !(c.excl_hz >= 0)) return "excl_chips or excl_hz is negative or NaN";
    if (!std::isfinite(c.Fs) || !(c.Fs > 0)) return "Fs is not a positive finite value";
    if (c.bytes_per_sample != 1 && c.bytes_per_sample != 2) return "bytes_per_sample is not 1 or 2";
    return nullptr;
}

void store_peaks(gnss_replay_ddm_out* out, int64_t k, const DdmPeaks& p)
{
    out->peak_bin[k] = p.peak_bin;
    out->peak_tap[k] = p.peak_tap;
    out->peak_pow[k] = p.peak_pow;
    out->sec_bin[k] = p.sec_bin;
    out->sec_tap[k] = p.sec_tap;
    out->sec_pow[k] = p.sec_pow;
}

}  // namespace

extern "C" int gnss_replay_ddm(gnss_ctx* ctx, const gnss_replay_ddm_cfg* cfg, const gnss_replay_ddm_in* in,
                               gnss_replay_ddm_out* out)
{
    if (!cfg || !in || !out) return fail(ctx, GNSS_EARG, "gnss_replay_ddm: a null argument");
    if (ctx && !ctx->members.empty()) return fail(ctx, GNSS_EARG, "gnss_replay_ddm: a multi-device context (one device only)");
    if (const char* why = cfg_fault(*cfg)) return fail(ctx, GNSS_EARG, "gnss_replay_ddm_cfg: %s", why);
    if (!in->taps || !in->n_rows || !in->pos_bytes || !in->numSample || in->max_rows < 1)
        return fail(ctx, GNSS_EARG, "gnss_replay_ddm_in: a null array or max_rows below 1");
    if (out->cap < 0 || !out->peak_bin || !out->peak_tap || !out->peak_pow || !out->sec_bin || !out->sec_tap ||
        !out->sec_pow || !out->n_win)
        return fail(ctx, GNSS_EARG, "gnss_replay_ddm_out: a null array or a negative cap");
    const int n = cfg->n, nt = cfg->n_taps, nd = cfg->n_dopp, R = cfg->rows_per_window, bps = cfg->bytes_per_sample;
    const int64_t MR = in->max_rows, cap = out->cap, cells = (int64_t)nd * nt;
    const bool on_device = (cfg->flags & GNSS_OUT_DEVICE) != 0, map_device = (cfg->flags & GNSS_DDM_MAP_DEVICE) != 0;
    if (map_device && !out->map) return fail(ctx, GNSS_EARG, "gnss_replay_ddm: GNSS_DDM_MAP_DEVICE without a map");
    DdmArgs a{};
    for (int c = 0; c < n; c++) {
        if (in->n_rows[c] < 0 || in->n_rows[c] > MR)
            return fail(ctx, GNSS_EARG, "gnss_replay_ddm_in.n_rows[%d] outside 0..max_rows", c);
        const int64_t wins = in->n_rows[c] / R;
        if (wins > cap)
            return fail(ctx, GNSS_EARG, "gnss_replay_ddm_out.cap is smaller than channel %d's %lld windows", c, (long long)wins);
        a.win_base[c + 1] = a.win_base[c] + wins;
    }
    const int64_t total = a.win_base[n];
    if (total > 0x7fffffff) return fail(ctx, GNSS_EARG, "gnss_replay_ddm: more than 2^31 - 1 windows");
    if (on_device) {
        if (!ctx) return fail(ctx, GNSS_EARG, "gnss_replay_ddm: GNSS_OUT_DEVICE needs a context");
        HIP_TRY(hipSetDevice(ctx->device));
        if (!device_memory_of(in->taps, (size_t)n * 2 * (size_t)nt * (size_t)MR * sizeof(double), ctx->device))
            return fail(ctx, GNSS_EARG, "gnss_replay_ddm_in.taps is not [n][2][n_taps][max_rows] of the context's device");
        if (map_device && !device_memory_of(out->map, (size_t)n * (size_t)cap * 2 * (size_t)cells * sizeof(double), ctx->device))
            return fail(ctx, GNSS_EARG, "gnss_replay_ddm_out.map is not [n][cap][2][n_dopp][n_taps] of the context's device");
    }
    // the rows' times, [n][max_rows]; rows outside a whole window keep 0 and are never read
    std::vector<double> t((size_t)n * (size_t)MR, 0.0);
    for (int c = 0; c < n; c++)
        for (int64_t i = 0; i < (a.win_base[c + 1] - a.win_base[c]) * R; i++) {
            const int64_t at = (int64_t)c * MR + i, first = at - i % R, ns = in->numSample[at];
            if (ns < 1 || ns > kReplayMaxSamples)
                return fail(ctx, GNSS_EARG, "channel %d row %lld: numSample outside 1..2^22", c, (long long)i);
            const int64_t p = in->pos_bytes[at], p0 = in->pos_bytes[first];
            if (p < 0 || (at > first && p < in->pos_bytes[at - 1]))
                return fail(ctx, GNSS_EIO, "channel %d row %lld: pos_bytes is negative or decreases within the window", c,
                            (long long)i);
            if ((p - p0) % bps != 0 || p - p0 > kDdmMaxSpan)
                return fail(ctx, GNSS_EIO, "channel %d row %lld: %lld bytes from the window's first row are no multiple of "
                            "bytes_per_sample or over 2^50", c, (long long)i, (long long)(p - p0));
            t[(size_t)at] = ddm_row_time((p - p0) / bps, ns, cfg->Fs);
        }

    auto channel_of = [&](int64_t w) {
        int c = 0;
        while (c + 1 < n && w >= a.win_base[c + 1]) c++;
        return c;
    };
    for (int c = 0; c < n; c++) out->n_win[c] = a.win_base[c + 1] - a.win_base[c];
    out->kernel_ms = 0;
    if (!on_device) {
        parallel_for((int)total, [&](int w) {
            const int c = channel_of(w);
            const int64_t m = w - a.win_base[c], k = (int64_t)c * cap + m;
            const double* I = in->taps + (int64_t)c * 2 * nt * MR + m * R;
            std::vector<double> tmp((size_t)3 * R + (out->map ? 0 : 2 * (size_t)cells));
            double* zI = out->map ? out->map + k * 2 * cells : tmp.data() + 3 * R;
            ddm_window_host(I, I + (int64_t)nt * MR, MR, cfg->prompt >= 0 ? I + (int64_t)cfg->prompt * MR : nullptr,
                            t.data() + (int64_t)c * MR + m * R, R, nt, nd, cfg->dopp_hz, tmp.data(), tmp.data() + R,
                            tmp.data() + 2 * R, zI, zI + cells);
            store_peaks(out, k, ddm_peaks_host(zI, zI + cells, nd, nt, cfg->u, cfg->dopp_hz, cfg->excl_chips, cfg->excl_hz));
        });
        return GNSS_OK;
    }

    // ---- the device path --------------------------------------------------------------------------
    ctx->timing = gnss_timing{};
    if (total == 0) return GNSS_OK;
    DevBuf bt, bhz, bu, bmap, bpk;
    HIP_TRY(bt.alloc(ctx, "replay_ddm_t", t.size() * sizeof(double)));
    HIP_TRY(bhz.alloc(ctx, "replay_ddm_hz", (size_t)nd * sizeof(double)));
    HIP_TRY(bu.alloc(ctx, "replay_ddm_u", (size_t)nt * sizeof(double)));
    HIP_TRY(bpk.alloc(ctx, "replay_ddm_peaks", (size_t)total * sizeof(DdmPeaks)));
    if (!map_device) HIP_TRY(bmap.alloc(ctx, "replay_ddm_map", (size_t)total * 2 * (size_t)cells * sizeof(double)));
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(bt.p, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(bhz.p, cfg->dopp_hz, (size_t)nd * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(bu.p, cfg->u, (size_t)nt * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // (the host arrays are pageable: the copies have left them)
    a.taps = in->taps;
    a.t = bt.as<double>();
    a.hz = bhz.as<double>();
    a.u = bu.as<double>();
    a.map = map_device ? out->map : bmap.as<double>();
    a.peaks = bpk.as<DdmPeaks>();
    a.max_rows = MR;
    a.slot_cap = map_device ? cap : 0;
    a.n = n;
    a.n_taps = nt;
    a.n_dopp = nd;
    a.prompt = cfg->prompt;
    a.R = R;
    a.excl_chips = cfg->excl_chips;
    a.excl_hz = cfg->excl_hz;
    Events ev;
    HIP_TRY(hipEventRecord(ev.a, st));
    const int le = replay_ddm_launch(a, st);
    if (le) return fail(ctx, GNSS_EDEVICE, "gnss_replay_ddm: kernel launch: %s", hipGetErrorString((hipError_t)le));
    HIP_TRY(hipEventRecord(ev.b, st));
    DdmPeaks* h = pinned_buffer<DdmPeaks>(ctx, "replay_ddm_peaks", (size_t)total);
    if (!h) return fail(ctx, GNSS_EDEVICE, "gnss_replay_ddm: pinned staging");
    HIP_TRY(hipMemcpyAsync(h, a.peaks, (size_t)total * sizeof(DdmPeaks), hipMemcpyDeviceToHost, st));
    if (out->map && !map_device)
        for (int c = 0; c < n; c++) {
            const int64_t wins = a.win_base[c + 1] - a.win_base[c];
            if (wins > 0)
                HIP_TRY(hipMemcpyAsync(out->map + (int64_t)c * cap * 2 * cells, a.map + a.win_base[c] * 2 * cells,
                                       (size_t)wins * 2 * (size_t)cells * sizeof(double), hipMemcpyDeviceToHost, st));
        }
    HIP_TRY(hipStreamSynchronize(st));
    out->kernel_ms = ev.ms();
    ctx->timing.track_kernel_ms = out->kernel_ms;
    ctx->timing.track_launches = 2;
    for (int64_t w = 0; w < total; w++) {
        const int c = channel_of(w);
        store_peaks(out, (int64_t)c * cap + (w - a.win_base[c]), h[w]);
    }
    return GNSS_OK;
}
