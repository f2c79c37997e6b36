// acf_fit_host.h — the host side that gnss_acf_fit, gnss_acf_fit_taps and gnss_acf_fit_multi share
// (acf_fit.cpp, acf_fit_taps.cpp, acf_fit_multi.cpp): the window plan and its checks, the device
// preconditions, a window's coherent sums on the host, and the run: the host path over the windows
// on up to 16 threads (a window by one thread: the bits do not depend on the thread count) or, for
// GNSS_OUT_DEVICE sums, the scratch, the launch and the rows' download. An entry point keeps its
// cfg checks, its fit of one window, its kernel's launch and its output arrays, and hands them in.
// Every check runs before any launch and before any output is written. Host only.
#pragma once

#include <cstring>
#include <functional>
#include <optional>
#include <string>

#include "acf_fit_taps.h"
#include "host.h"

namespace gnss {
namespace host {

// One call as the driver sees it: sums [n][2][n_taps][max_rows], n_rows[c] of them per channel.
// The entry point fills the first group; whoever owns the output struct fills the second (the
// entry itself for gnss_acf_fit_multi_out, acf_fit_two_path for gnss_acf_fit_out).
struct AcfFitCall {
    // the error texts' names: the entry point, its cfg struct, the rows' count ("...n_rows"), its
    // bound ("max_rows") and what lies on the device ("sums")
    const char *fn, *cfg, *rows, *max, *sums;
    const char* n_fault;    // an entry's check that ranks right after n's: the whole text, or null
    const char* cfg_fault;  // the entry's own cfg check: the text, or null
    const char* in_fault;   // a null array or max_rows < 1 in the sums' struct: the text, or null
    int n, n_taps, prompt;
    int64_t ind_start, numOverLap;
    const double* u;  // [n_taps], host, uploaded for the kernel; null: the entry's kernel takes none
    const double* taps;
    const int64_t* n_rows;
    int64_t max_rows;
    bool on_device;
    bool check_taps;     // device sums: taps must be that many doubles of the context's device
    bool timing;         // device sums: ctx->timing takes the kernel's time
    const char* key;     // the stem of the context's scratch names
    // the output
    const char* out;     // its struct's name, for the error texts
    bool out_complete;   // no output array is null, cap >= 0
    int64_t cap;         // the output's windows per channel
    int64_t* windows;    // the output's [n]
    bool want_z;         // the output takes the coherent vectors
    int row;             // doubles per window in the kernel's output
};

// window m of channel c on the host: the coherent sums a tap at a time into zI / zQ [n_taps]
inline void acf_fit_host_sums(const AcfFitCall& k, int c, int64_t m, double* zI, double* zQ)
{
    const int nt = k.n_taps;
    const int64_t mr = k.max_rows, row = ftt_window_row(m, k.ind_start, k.numOverLap);
    const double* base = k.taps + (int64_t)c * 2 * nt * mr + row;
    const double* prompt = base + (int64_t)k.prompt * mr;
    for (int j = 0; j < nt; j++) {
        const double* I = base + (int64_t)j * mr;
        const double* Q = base + (int64_t)(nt + j) * mr;
        double aI = 0, aQ = 0;
        for (int64_t i = 0; i < k.numOverLap; i++) {
            const double s = ftt_sign(prompt[i]);
            aI = ftt_accum(aI, s, I[i], i == 0);
            aQ = ftt_accum(aQ, s, Q[i], i == 0);
        }
        zI[j] = aI;
        zQ[j] = aQ;
    }
}

// The call. fit(c, m, zI, zQ): the entry's fit of window m of channel c from its coherent vector,
// stored (the host path). launch(io, stream): the entry's kernel, one block per window -> the
// hipError_t. store(c, m, row, zI, zQ): a downloaded row stored (zI / zQ are read only if the
// output wants them).
template <class Fit, class Launch, class Store>
int acf_fit_run(gnss_ctx* ctx, const AcfFitCall& k, Fit fit, Launch launch, Store store)
{
    const int n = k.n, nt = k.n_taps;
    if (n < 1 || n > GNSS_VT_MAX_CH) return fail(ctx, GNSS_EARG, "%s.n outside 1..%d", k.cfg, GNSS_VT_MAX_CH);
    if (k.n_fault) return fail(ctx, GNSS_EARG, "%s", k.n_fault);
    if (k.numOverLap < 2 || k.numOverLap > 4096) return fail(ctx, GNSS_EARG, "%s.numOverLap outside 2..4096", k.cfg);
    if (k.ind_start < 1) return fail(ctx, GNSS_EARG, "%s.ind_start below 1", k.cfg);
    if (k.cfg_fault) return fail(ctx, GNSS_EARG, "%s: %s", k.cfg, k.cfg_fault);
    if (k.in_fault) return fail(ctx, GNSS_EARG, "%s", k.in_fault);
    if (!k.out_complete) return fail(ctx, GNSS_EARG, "%s: a null array", k.out);
    // every extent the loops and the kernel index with: the rows of a channel's windows lie below
    // n_rows[c] (ftt_windows), n_rows[c] rows of a max_rows series
    AcfFttIo d{};
    int64_t windows[kFttMaxCh];
    for (int c = 0; c < n; c++) {
        if (k.n_rows[c] < 0 || k.n_rows[c] > k.max_rows)
            return fail(ctx, GNSS_EARG, "%s[%d] outside 0..%s", k.rows, c, k.max);
        windows[c] = ftt_windows(k.n_rows[c], k.ind_start, k.numOverLap);
        if (windows[c] > k.cap)
            return fail(ctx, GNSS_EARG, "%s.cap is smaller than channel %d's %lld windows", k.out, c,
                        (long long)windows[c]);
        d.win_base[c + 1] = d.win_base[c] + windows[c];
    }
    const int64_t total = d.win_base[n];
    if (total > 0x7fffffff) return fail(ctx, GNSS_EARG, "%s: more than 2^31 - 1 windows", k.fn);
    if (k.on_device) {
        if (!ctx) return fail(ctx, GNSS_EARG, "%s: GNSS_OUT_DEVICE needs a context", k.fn);
        if (!ctx->members.empty())
            return fail(ctx, GNSS_EARG, "%s: device %s on a multi-device context", k.fn, k.sums);
        HIP_TRY(hipSetDevice(ctx->device));
        const size_t bytes = (size_t)n * 2 * (size_t)nt * (size_t)k.max_rows * sizeof(double);
        if (k.check_taps && !device_memory_of(k.taps, bytes, ctx->device))
            return fail(ctx, GNSS_EARG,
                        "gnss_acf_fit_taps_in.taps is not [n][2][n_taps][max_rows] of the context's device");
    }
    for (int c = 0; c < n; c++) k.windows[c] = windows[c];
    auto channel_of = [&](int64_t w) {
        int c = 0;
        while (c + 1 < n && w >= d.win_base[c + 1]) c++;
        return c;
    };
    if (!k.on_device) {
        parallel_for((int)total, [&](int w) {
            const int c = channel_of(w);
            double zI[kFttMaxTaps], zQ[kFttMaxTaps];
            acf_fit_host_sums(k, c, w - d.win_base[c], zI, zQ);
            fit(c, w - d.win_base[c], zI, zQ);
        });
        return GNSS_OK;
    }
    if (k.timing) ctx->timing = gnss_timing{};
    if (total == 0) return GNSS_OK;

    const bool want_z = k.want_z;
    const std::string key = k.key;
    const size_t row_bytes = (size_t)total * k.row * sizeof(double), z_bytes = (size_t)total * 2 * nt * sizeof(double);
    DevBuf rows, z, u;
    HIP_TRY(rows.alloc(ctx, (key + "_rows").c_str(), row_bytes));
    if (want_z) HIP_TRY(z.alloc(ctx, (key + "_z").c_str(), z_bytes));
    if (k.u) {
        HIP_TRY(u.alloc(ctx, (key + "_u").c_str(), (size_t)nt * sizeof(double)));
        HIP_TRY(hipMemcpyAsync(u.p, k.u, (size_t)nt * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));  // (the host array is pageable: the copy has left it)
    }
    d.taps = k.taps;
    d.u = u.as<double>();
    d.max_rows = k.max_rows;
    d.n = n;
    d.ind_start = k.ind_start;
    d.numOverLap = k.numOverLap;
    d.rows = rows.as<double>();
    d.z = want_z ? z.as<double>() : nullptr;
    std::optional<Events> ev;
    if (k.timing) HIP_TRY(hipEventRecord(ev.emplace().a, ctx->stream));
    const int le = launch(d, ctx->stream);
    if (le) return fail(ctx, GNSS_EDEVICE, "%s: kernel launch: %s", k.fn, hipGetErrorString((hipError_t)le));
    if (k.timing) HIP_TRY(hipEventRecord(ev->b, ctx->stream));
    double* h = pinned_buffer<double>(ctx, k.key, (size_t)total * ((size_t)k.row + (want_z ? 2 * (size_t)nt : 0)));
    if (!h) return fail(ctx, GNSS_EDEVICE, "%s: pinned staging", k.fn);
    double* hz = h + (size_t)total * k.row;
    HIP_TRY(hipMemcpyAsync(h, d.rows, row_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (want_z) HIP_TRY(hipMemcpyAsync(hz, d.z, z_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (k.timing) {
        ctx->timing.track_kernel_ms = ev->ms();
        ctx->timing.track_launches = 1;
    }
    for (int64_t w = 0; w < total; w++) {
        const int c = channel_of(w);
        const double* zw = hz + w * 2 * nt;  // (read by store only if wanted)
        store(c, w - d.win_base[c], h + w * k.row, zw, zw + nt);
    }
    return GNSS_OK;
}

// (acf_fit_taps.cpp) The two-path entries, gnss_acf_fit at 25 taps among them, on grid g and tap
// coordinates u into gnss_acf_fit_out: the call k, whose output fields are filled there, with the
// host path on ftt_window and the entry's kernel behind `launch`; and the fit of one coherent
// vector (GNSS_EARG for a null vector or an incomplete out).
using AcfFitLaunch = std::function<int(const AcfFttIo&, void*)>;
int acf_fit_two_path(gnss_ctx* ctx, AcfFitCall k, const AcfFttGrid& g, const double* u, gnss_acf_fit_out* out,
                     const AcfFitLaunch& launch);
int acf_fit_two_path_window(const AcfFttGrid& g, const double* u, const double* zI, const double* zQ,
                            gnss_acf_fit_out* out);

}  // namespace host
}  // namespace gnss
