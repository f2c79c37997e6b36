// api_vt.cpp -- the vector-tracking loops on the host side of the C-ABI:
// trackingVT_POS_updated.m (gnss_tracking_vt_run / _step / gnss_tracking_vt) and
// trackingVT_POS_updated_multicorrelator.m (gnss_tracking_vt_mc_run / gnss_tracking_vt_mc).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "host.h"
#include "vt_mc.h"

using namespace gnss;
using namespace gnss::host;

namespace {

// The record formats of trackingVT_POS_updated.m:163-176 -- int8 I/Q, int8 real, int16 I/Q (means
// removed) -- and the record's length: one gate for the three loops.
int vt_record(gnss_ctx* ctx, const gnss_file* file, int* bps, int64_t* flen)
{
    const int prec = file->dataPrecision, dtyp = file->dataType;
    if (!((prec == 1 && (dtyp == 1 || dtyp == 2)) || (prec == 2 && dtyp == 2)))
        return fail(ctx, GNSS_EARG, "vector tracking: int8 I/Q, int8 real or int16 I/Q records");
    *bps = prec * dtyp;
    *flen = file_length(file);
    if (*flen < 0) return fail(ctx, GNSS_EIO, "cannot open IF record");
    return GNSS_OK;
}

// The channel states' checks, per channel in this order. Each entry runs the ones it always ran:
//   prn_range  PRN in 1..51 (gnss_tracking_vt_run, the 25-tap loop; gnss_tracking_vt takes nav's)
//   nav        chans[i].prn == nav->prn[i] (the EKF-driven entries)
//   code_freq  the channel's code frequency > 0 (not gnss_tracking_vt_run, which bounds the
//              smallest frequency of the whole series instead)
int vt_check_chans(gnss_ctx* ctx, const gnss_vt_chan* chans, int n, int bps, bool prn_range, const gnss_vt_nav* nav,
                   bool code_freq)
{
    for (int i = 0; i < n; i++) {
        if (prn_range && (chans[i].prn < 1 || chans[i].prn > 51)) return fail(ctx, GNSS_EARG, "bad PRN");
        if (nav && chans[i].prn != nav->prn[i]) return fail(ctx, GNSS_EARG, "chans[i].prn != nav->prn[i]");
        if (chans[i].file_ptr < 0 || chans[i].file_ptr % bps) return fail(ctx, GNSS_EARG, "file_ptr");
        if (chans[i].index_int < 0 || chans[i].index_int > 19 || chans[i].snrIndex < 1)
            return fail(ctx, GNSS_EARG, "C/N0 state (index_int 0..19, snrIndex >= 1)");
        if (code_freq && !(chans[i].codeFreq > 0)) return fail(ctx, GNSS_EARG, "code frequency must be positive");
    }
    return GNSS_OK;
}

std::vector<unsigned> vt_ca_table(const gnss_vt_chan* chans, int n)
{
    std::vector<unsigned> cab((size_t)n * 32);
    for (int i = 0; i < n; i++) ca_bits(chans[i].prn, &cab[(size_t)i * 32]);
    return cab;
}

// The IF window of the EKF-driven loops: the steps' reads are sized by code frequencies the EKF
// has not predicted yet, so a window is staged for `span` steps at half the nominal code rate
// (twice the nominal read) and re-staged when a read would leave it -- from `lo`, and at least up
// to need_hi where the caller gives one. A resident record is used as is.
struct VtWindow {
    gnss_ctx* ctx;
    const gnss_file* file;
    int64_t flen, nominal, bytes;  // nominal: a step's samples at the nominal code rate
    IfWindow w;
    VtWindow(gnss_ctx* ctx_, const gnss_file* file_, const gnss_signal* sg, int pdi, int nsteps, int bps, int64_t flen_)
        : ctx(ctx_), file(file_), flen(flen_)
    {
        nominal = (int64_t)std::ceil(sg->codelength * pdi / (sg->codeFreqBasis / sg->Fs));
        const int64_t span =
            std::min<int64_t>(nsteps, ctx->opt[GNSS_OPT_VT_SPAN] > 0 ? ctx->opt[GNSS_OPT_VT_SPAN] : kVtSpan);
        bytes = (span * 2 * nominal + 64) * bps;
    }
    int restage(int64_t lo, int64_t need_hi = 0)
    {
        const int64_t hi = std::max(lo + bytes, need_hi);
        w.own.release();
        w.ptr = nullptr;
        w.base = w.len = 0;
        return stage_window(ctx, file, lo, std::min(hi, flen), w);
    }
    int stage_first(const gnss_vt_chan* chans, int n)  // from the earliest file_ptr
    {
        int64_t lo0 = INT64_MAX;
        for (int i = 0; i < n; i++) lo0 = std::min(lo0, chans[i].file_ptr);
        return restage(lo0);
    }
};

// k/Fs by Markstein's correction where it is the IEEE quotient (exhaustively verified up to four
// nominal reads, cached per Fs): the reciprocal for a read of ns samples; 0 = a longer read divides
struct VtRecip {
    int64_t kmax = 0;
    double rfs = 0;
    double of(int64_t ns) const { return ns - 1 <= kmax ? rfs : 0.0; }
};

// What the one-launch-per-step loops share (VtStepArgs / VtMcStepArgs): the step's sums (`nsums`
// doubles, buffer `sums_key`) and its completion word in coherent host memory, the blocks'
// ticket, and the reciprocal of Fs.
template <class Args>
int vt_step_setup(gnss_ctx* ctx, const char* sums_key, size_t nsums, double Fs, int64_t nominal, Args& B,
                  DevBuf& d_ticket, VtRecip& recip)
{
    B.sums = pinned_buffer<double>(ctx, sums_key, nsums, hipHostMallocCoherent);
    B.done = pinned_buffer<unsigned>(ctx, "vt.done", 1, hipHostMallocCoherent);
    if (!B.sums || !B.done) return fail(ctx, GNSS_EDEVICE, "pinned VT step buffers");
    __atomic_store_n(B.done, 0u, __ATOMIC_RELAXED);
    HIP_TRY(d_ticket.alloc(ctx, "vt.ticket", sizeof(unsigned)));
    HIP_TRY(hipMemsetAsync(d_ticket.p, 0, sizeof(unsigned), ctx->stream));
    B.ticket = d_ticket.as<unsigned>();
    B.Fs = Fs;
    recip.kmax = 4 * nominal;
    recip.rfs = fast_div_exact(Fs, recip.kmax) ? 1.0 / Fs : 0.0;
    return GNSS_OK;
}

// ... and their timing: the kernels' time (summed in profiling mode only) and the loop's wall time
void vt_loop_timing(gnss_ctx* ctx, double kernel_ms, std::chrono::steady_clock::time_point t_loop)
{
    ctx->timing.track_kernel_ms = kernel_ms;
    ctx->timing.track_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_loop).count();
}

// Wait until posted() holds for something a kernel on `stream` writes to coherent host memory.
// The stream is polled now and then, so a grid that ends without posting (a fault) surfaces as
// its error rather than a hang.
template <class Pred>
inline hipError_t wait_until(hipStream_t stream, Pred posted)
{
    for (unsigned k = 1;; k++) {
        if (posted()) return hipSuccess;
        __builtin_ia32_pause();
        if ((k & 255) == 0) {
            const hipError_t e = hipStreamQuery(stream);
            if (e == hipErrorNotReady) continue;
            if (e != hipSuccess) return e;
            return posted() ? hipSuccess : hipErrorLaunchFailure;  // (retired: its posts are visible)
        }
    }
}

// ... until VT step `seq` is posted (the step kernels' completion word)
inline hipError_t wait_posted(hipStream_t stream, const unsigned* done, unsigned seq)
{
    return wait_until(stream, [&] { return __atomic_load_n(done, __ATOMIC_ACQUIRE) == seq; });
}

// ... until the loop mode's n granules all carry `seq`, their values to `out` (a granule seen
// once is not read again: the scan resumes where it stopped)
inline hipError_t wait_granules(hipStream_t stream, const VtGran* g, int n, unsigned seq, double* out)
{
    int i = 0;
    return wait_until(stream, [&] {
        uint64_t bits;
        while (i < n && vt_gran_get(g + i, seq, &bits)) {
            std::memcpy(out + i, &bits, sizeof bits);
            i++;
        }
        return i == n;
    });
}

inline uint64_t bits_of(double v)
{
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}

// Channel i's read of step `seq` into the loop mode's mailbox, as granules tagged with the step's
// number (VtBlockStep's word order). f == nullptr: the early post, which leaves out word 2 -- the
// carrier frequency follows once the step before has its sums (post_step_freq).
inline void post_step_words(VtGran* mail, unsigned seq, int n, int i, int64_t off, int64_t ns, const double* f,
                            double phi0, double rfs)
{
    VtGran* g = mail + (size_t)kVtStepWords * ((seq & 1) * n + i);
    vt_gran_put(g + 0, (uint64_t)off, seq);
    vt_gran_put(g + 1, (uint64_t)ns, seq);
    if (f) vt_gran_put(g + 2, bits_of(*f), seq);
    vt_gran_put(g + 3, bits_of(phi0), seq);
    vt_gran_put(g + 4, bits_of(rfs), seq);
}

inline void post_step_freq(VtGran* mail, unsigned seq, int n, int i, double f)
{
    vt_gran_put(mail + (size_t)kVtStepWords * ((seq & 1) * n + i) + 2, bits_of(f), seq);
}

// (probe builds, GNSS_VT_STAMPS set) the host's share of a step by phase: mark(k) adds the time
// since the last mark to phase k
struct VtStamps {
    enum { kPre, kShadow, kWait, kPost, kPhases };
    const bool on = probe_env("GNSS_VT_STAMPS") != nullptr;
    double acc[kPhases] = {0, 0, 0, 0}, last = on ? now_us() : 0;
    static double now_us()
    {
        return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
    }
    void mark(int k)
    {
        if (!on) return;
        const double t = now_us();
        acc[k] += t - last;
        last = t;
    }
};

// The GNSS_VT_STAMPS report on stderr: the host's phases per step, and the loop kernel's own
// marks (d_vtst; GNSS_VT_PROBE & 4 builds, zeros otherwise) once the loop has stopped.
int report_vt_stamps(gnss_ctx* ctx, int nsteps, const VtStamps& hs, const DevBuf& d_vtst)
{
    if (nsteps > 0)
        fprintf(stderr, "vt stamps (us per step): predict+post %.2f, shadow %.2f, wait %.2f, finish+correct %.2f\n",
                hs.acc[VtStamps::kPre] / nsteps, hs.acc[VtStamps::kShadow] / nsteps, hs.acc[VtStamps::kWait] / nsteps,
                hs.acc[VtStamps::kPost] / nsteps);
    if (!d_vtst.p) return GNSS_OK;
    std::vector<unsigned long long> m((size_t)kVtStampSteps * (8 + 4 * kVtLoopMaxBlocks));
    HIP_TRY(hipMemcpy(m.data(), d_vtst.p, m.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    int khz = 0;
    HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device));
    const double us = 1e3 / std::max(khz, 1);
    double d[6] = {0, 0, 0, 0, 0, 0}, d6 = 0, d7 = 0;
    int cnt = 0;
    // the per-block marks as their maximum over the blocks (the step's last block)
    for (int k = 0; k < std::min(nsteps, kVtStampSteps); k++)
        for (int q = 0; q < 4; q++) {
            unsigned long long mx = 0;
            const unsigned long long* bm = &m[(size_t)kVtStampSteps * 8 + ((size_t)k * 4 + q) * kVtLoopMaxBlocks];
            for (int bl = 0; bl < kVtLoopMaxBlocks; bl++) mx = std::max(mx, bm[bl]);
            m[(size_t)8 * k + (q == 0 ? 2 : q == 1 ? 3 : q == 2 ? 6 : 7)] = mx;
        }
    for (int k = 10; k + 1 < std::min(nsteps, kVtStampSteps); k++) {
        const unsigned long long* r = &m[(size_t)8 * k];
        const unsigned long long* r1 = &m[(size_t)8 * (k + 1)];
        if (!r[0] || !r[5] || !r1[0]) continue;
        for (int j = 0; j < 5; j++) d[j] += (double)(long long)(r[j + 1] - r[j]) * us;
        d[5] += (double)(long long)(r1[0] - r[5]) * us;
        if (r[6] && r[7]) {
            d6 += (double)(long long)(r[6] - r[2]) * us;
            d7 += (double)(long long)(r[7] - r[6]) * us;
        }
        cnt++;
    }
    if (cnt)
        fprintf(stderr, "vt loop marks (us per step, %d steps): relay %.2f, to last block %.2f, to last sums %.2f "
                        "(last terms %.2f after the last block had the step, butterfly %.2f), gather %.2f, "
                        "sums out %.2f, sums out -> next mailbox seen %.2f\n",
                cnt, d[0] / cnt, d[1] / cnt, d[2] / cnt, d6 / cnt, d7 / cnt, d[3] / cnt, d[4] / cnt, d[5] / cnt);
    return GNSS_OK;
}

}  // namespace

extern "C" {

// trackingVT_POS_updated.m:157-349, one step of n channels (include/gnss_mi355x.h): the
// reads and replica chips sized on the host (gnss_vt_prepare), the carrier-wiped sums on
// the GPU (vt.hip), the NCO / PLL / DLL discriminator on the host (gnss_vt_nco_step).
int gnss_tracking_vt_run(gnss_ctx* ctx, const gnss_file* file, const gnss_signal* sg, const gnss_track* tr,
                         int32_t pdi, int32_t n, int32_t nsteps, gnss_vt_chan* chans, const double* codeFreq_new,
                         gnss_vt_out* out)
{
    if (!ctx || !file || !sg || !tr || !chans || !codeFreq_new || !out || n < 1 || n > GNSS_MAX_SV || pdi < 1 ||
        nsteps < 1 || !(sg->Fs > 0) || !(sg->codeFreqBasis > 0))
        return fail(ctx, GNSS_EARG, "bad arguments");
    ctx->err.clear();
    ctx->timing = gnss_timing{};
    HIP_TRY(hipSetDevice(ctx->device));
    const int prec = file->dataPrecision, dtyp = file->dataType;
    int bps, st;
    int64_t flen;
    if ((st = vt_record(ctx, file, &bps, &flen))) return st;
    if ((st = vt_check_chans(ctx, chans, n, bps, true, nullptr, false))) return st;
    // the read range of every step: from the earliest file_ptr, at most nsteps reads of the
    // largest size any step can ask for (the slowest code frequency of the series)
    double cf_min = 1e300;
    for (int i = 0; i < n; i++) cf_min = std::min(cf_min, chans[i].codeFreq);
    for (int64_t k = 0; k < (int64_t)nsteps * n; k++) cf_min = std::min(cf_min, codeFreq_new[k]);
    if (!(cf_min > 0)) return fail(ctx, GNSS_EARG, "code frequencies must be positive");
    const double nmax = std::ceil((sg->codelength * pdi + 2.0) / (cf_min / sg->Fs)) + 2;
    int64_t lo = INT64_MAX, hi = 0;
    for (int i = 0; i < n; i++) {
        lo = std::min(lo, chans[i].file_ptr);
        hi = std::max(hi, chans[i].file_ptr + (int64_t)(nsteps * nmax) * bps);
    }
    IfWindow w;
    if ((st = stage_window(ctx, file, lo, std::min(hi, flen), w))) return st;
    const std::vector<unsigned> cab = vt_ca_table(chans, n);
    DevBuf d_chan, d_cf, d_out, d_ca;
    const size_t nrec = (size_t)nsteps * n;
    HIP_TRY(d_chan.alloc(ctx, "vt.chan", sizeof(gnss_vt_chan) * (size_t)n));
    HIP_TRY(d_cf.alloc(ctx, "vt.cf", sizeof(double) * nrec));
    HIP_TRY(d_out.alloc(ctx, "vt.out", sizeof(gnss_vt_out) * nrec));
    HIP_TRY(d_ca.alloc(ctx, "vt.ca", sizeof(unsigned) * cab.size()));
    HIP_TRY(hipMemcpyAsync(d_chan.p, chans, sizeof(gnss_vt_chan) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_cf.p, codeFreq_new, sizeof(double) * nrec, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_ca.p, cab.data(), sizeof(unsigned) * cab.size(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(d_out.p, 0, sizeof(gnss_vt_out) * nrec, ctx->stream));
    double t1, t2;
    calc_loop_coef(tr->PLLBW, tr->PLLDamp, tr->PLLGain, t1, t2);
    VtRunArgs A{};
    A.rec = reinterpret_cast<const uint8_t*>(w.ptr);
    A.base = w.base;
    A.len = w.len;
    A.file_len = flen;
    A.chans = d_chan.as<gnss_vt_chan>();
    A.codeFreq = d_cf.as<double>();
    A.out = d_out.as<gnss_vt_out>();
    A.ca_bits = d_ca.as<unsigned>();
    A.Fs = sg->Fs;
    A.ms = sg->ms;
    A.codelength = sg->codelength;
    A.tau1carr = t1;
    A.tau2carr = t2;
    A.n = n;
    A.nsteps = nsteps;
    A.pdi = pdi;
    A.prec = prec;
    A.dtype = dtyp;
    Events ev;
    HIP_TRY(hipEventRecord(ev.a, ctx->stream));
    HIP_TRY(launch_vt_run(A, ctx->stream));
    HIP_TRY(hipEventRecord(ev.b, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out, d_out.p, sizeof(gnss_vt_out) * nrec, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(chans, d_chan.p, sizeof(gnss_vt_chan) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->timing.track_ms = ev.ms();
    ctx->timing.track_kernel_ms = ctx->timing.track_ms;
    ctx->timing.track_launches = 1;
    int first = GNSS_OK;
    for (int s = 0; s < nsteps; s++)
        for (int i = 0; i < n; i++) {
            const gnss_vt_out& o = out[(size_t)s * n + i];
            if (o.status) {
                if (!first) first = o.status;
            } else if (o.numSample > 0) {
                ctx->timing.track_channel_samples += o.numSample;
            }
        }
    if (first) return fail(ctx, first, "a channel stopped (its record's status): replica index / read past EOF");
    return GNSS_OK;
}

int gnss_tracking_vt_step(gnss_ctx* ctx, const gnss_file* file, const gnss_signal* sg, const gnss_track* tr,
                          int32_t pdi, int32_t n, gnss_vt_chan* chans, const double* codeFreq_new,
                          gnss_vt_out* out)
{
    return gnss_tracking_vt_run(ctx, file, sg, tr, pdi, n, 1, chans, codeFreq_new, out);
}

// trackingVT_POS_updated.m:157-476, the whole EKF-driven loop: per step, each channel's read
// size (:164) and predicted code frequency (:180-227, gnss_vt_nav_predict, host), the
// correlations of all channels in ONE launch of the VT kernel, each channel's scalar end
// (vt_finish, :284-347), then the EKF (:357-467, gnss_vt_nav_update, host). int8 records: the
// channel states stay on the host and the kernel returns each channel's sums (vt_step_kernel);
// int16 (per-read means first): vt_run_kernel runs the whole step, states in HBM.
int gnss_tracking_vt(gnss_ctx* ctx, const gnss_file* file, const gnss_signal* sg, const gnss_track* tr, int32_t n,
                     int32_t nsteps, gnss_vt_chan* chans, gnss_vt_nav* nav, gnss_vt_out* out, gnss_vt_navsol* sol)
{
    if (!ctx || !file || !sg || !tr || !chans || !nav || !out || n < 1 || n > GNSS_VT_MAX_CH || n != nav->n ||
        nsteps < 0 || !(sg->Fs > 0) || !(sg->codeFreqBasis > 0) || sg->Fs != nav->Fs)
        return fail(ctx, GNSS_EARG, "bad arguments (n in 1..GNSS_VT_MAX_CH and equal to nav->n, signal as at gnss_vt_nav_init)");
    ctx->err.clear();
    ctx->timing = gnss_timing{};
    if (nsteps == 0) return GNSS_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const int pdi = nav->pdi;
    const int prec = file->dataPrecision, dtyp = file->dataType;
    int bps, st;
    int64_t flen;
    if ((st = vt_record(ctx, file, &bps, &flen))) return st;
    if ((st = vt_check_chans(ctx, chans, n, bps, false, nav, true))) return st;
    VtWindow win(ctx, file, sg, pdi, nsteps, bps, flen);  // (need_hi is never given: a window is `bytes` long)
    IfWindow& w = win.w;
    const int64_t nominal = win.nominal;
    if ((st = win.stage_first(chans, n))) return st;
    const std::vector<unsigned> cab = vt_ca_table(chans, n);
    double t1, t2;
    calc_loop_coef(tr->PLLBW, tr->PLLDamp, tr->PLLGain, t1, t2);
    // int8 records: each step over nb blocks per channel (vt_step_kernel), the step's reads
    // in the kernel arguments and each channel's two sums posted to coherent host memory (no
    // copy commands per step); int16 (per-read means first): one block per channel (vt_run_kernel)
    const bool multi = prec == 1;
    DevBuf d_chan, d_cf, d_out, d_ca, d_part, d_ticket, d_loop;
    double* h_cf = pinned_buffer<double>(ctx, "vt.cf", (size_t)n);
    gnss_vt_out* h_out = pinned_buffer<gnss_vt_out>(ctx, "vt.out", (size_t)n);
    if (!h_cf || !h_out) return fail(ctx, GNSS_EDEVICE, "pinned VT step buffers");
    std::vector<gnss_vt_chan> hc(chans, chans + n);  // (int8: the channel states)
    std::vector<VtPrep> pk((size_t)n);
    std::vector<int> bad((size_t)n, 0);
    VtStepArgs B{};
    int nb = 1;
    int loop_cap = 0;  // blocks a loop grid may have (0: no loop mode)
    VtRecip recip;
    if (multi) {
        // blocks per channel, the engine's choice per path (r06_vt_loop_nb*.txt): one launch per
        // step pays a ticket per block, the loop's lead gathers every block's granules at once
        const bool loop_ok = !ctx->profiling && !ctx->opt[GNSS_OPT_NO_PERSIST];
        loop_cap = loop_ok ? vt_loop_resident_blocks(ctx->device) : 0;
        nb = loop_cap >= n ? (int)std::min<int64_t>(std::max<int64_t>(1, (nominal + kVtLoopSamples - 1) / kVtLoopSamples),
                                                    loop_cap / n)
                     : (int)std::min<int64_t>(std::max<int64_t>(1, (nominal + kVtStepSamples - 1) / kVtStepSamples),
                                              GNSS_VT_MAX_BLOCKS);
        if (ctx->opt[GNSS_OPT_VT_BLOCKS] > 0) nb = (int)ctx->opt[GNSS_OPT_VT_BLOCKS];
        if ((st = vt_step_setup(ctx, "vt.sums", 2 * (size_t)n, sg->Fs, nominal, B, d_ticket, recip))) return st;
        B.real8 = dtyp == 1;
        HIP_TRY(d_part.alloc(ctx, "vt.part", sizeof(double) * 2 * (size_t)n * nb));
        B.part = d_part.as<double>();
    } else {
        HIP_TRY(d_chan.alloc(ctx, "vt.chan", sizeof(gnss_vt_chan) * (size_t)n));
        HIP_TRY(d_cf.alloc(ctx, "vt.cf", sizeof(double) * (size_t)n));
        HIP_TRY(d_out.alloc(ctx, "vt.out", sizeof(gnss_vt_out) * (size_t)n));
        HIP_TRY(d_ca.alloc(ctx, "vt.ca", sizeof(unsigned) * cab.size()));
        HIP_TRY(hipMemcpyAsync(d_chan.p, chans, sizeof(gnss_vt_chan) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_ca.p, cab.data(), sizeof(unsigned) * cab.size(), hipMemcpyHostToDevice, ctx->stream));
    }
    VtRunArgs A{};
    A.file_len = flen;
    A.chans = d_chan.as<gnss_vt_chan>();
    A.codeFreq = d_cf.as<double>();
    A.out = d_out.as<gnss_vt_out>();
    A.ca_bits = d_ca.as<unsigned>();
    A.Fs = sg->Fs;
    A.ms = sg->ms;
    A.codelength = sg->codelength;
    A.tau1carr = t1;
    A.tau2carr = t2;
    A.n = n;
    A.nsteps = 1;
    A.pdi = pdi;
    A.prec = prec;
    A.dtype = dtyp;
    // Loop mode (int8 records, not profiling, the grid fits on the chip at once): ONE
    // vt_loop_kernel launch runs the steps, each posted through a mailbox in coherent host
    // memory, so a step costs no launch; stopped before a re-staging of the IF window and at
    // the end (also on every early return: `loop_guard`).
    const bool loop_mode = multi && loop_cap > 0 && (int64_t)n * nb <= loop_cap;
    VtGran *mail = nullptr, *gsums = nullptr;
    std::vector<double> loop_sums(2 * (size_t)n);
    bool running = false;
    // the loop's 16-B granules: each channel's relayed read, then every block's two sums
    const size_t gstep_bytes = (size_t)16 * kVtStepWords * n, loop_bytes = gstep_bytes + (size_t)16 * 2 * n * nb;
    uint64_t loop_timeout = 0;
    if (loop_mode) {
        mail = pinned_buffer<VtGran>(ctx, "vt.mail", 2 * (size_t)kVtStepWords * n, hipHostMallocCoherent);
        gsums = pinned_buffer<VtGran>(ctx, "vt.gsums", 2 * (size_t)n, hipHostMallocCoherent);
        if (!mail || !gsums) return fail(ctx, GNSS_EDEVICE, "pinned VT mailbox");
        for (int k = 0; k < 2 * kVtStepWords * n; k++) vt_gran_put(mail + k, 0, 0);
        for (int k = 0; k < 2 * n; k++) vt_gran_put(gsums + k, 0, 0);
        int khz = 0;
        HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device));
        loop_timeout = (uint64_t)(std::max(khz, 1) * 1e3 * kVtLoopTimeoutS);
        HIP_TRY(d_loop.alloc(ctx, "vt.loop", loop_bytes));
    }
    auto stop_loop = [&]() -> hipError_t {  // (the mailbox's stop tags, then its tags back to 0)
        if (!running) return hipSuccess;
        for (int k = 0; k < 2 * kVtStepWords * n; k++) vt_gran_put(mail + k, 0, kVtLoopStop);
        running = false;
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        for (int k = 0; k < 2 * kVtStepWords * n; k++) vt_gran_put(mail + k, 0, 0);
        return e;
    };
    struct LoopGuard {
        decltype(stop_loop)& stop;
        ~LoopGuard() { (void)stop(); }
    } loop_guard{stop_loop};
    // the host's view of what sizes the next read (:164): remChip / codeFreq / file_ptr of the
    // last step, from the records the kernel returns
    std::vector<double> remChip(n), cf_old(n), codeError(n), carrFreq(n), cf_new(n);
    std::vector<int64_t> fptr(n);
    for (int i = 0; i < n; i++) {
        remChip[i] = chans[i].remChip;
        cf_old[i] = chans[i].codeFreq;
        fptr[i] = chans[i].file_ptr;
    }
    // While a step's kernel runs, the host does the navigation work that needs none of its
    // correlations (bit for bit the work it replaces: the same functions on the same inputs):
    // the EKF's geometry half of this step (vt_nav_gain) and every channel's orbit for the next
    // step, whose read size follows from this step's without its samples (vt_remchip_next).
    // An orbit is used only at the transmit time it was computed for.
    std::vector<VtOrbit> ahead((size_t)n);
    std::vector<char> have_ahead((size_t)n, 0);
    std::unique_ptr<VtGain> gain(new VtGain);
    // Loop mode posts the next step early: of a channel's read only the carrier frequency waits
    // for the step's sums (the PLL, :305-311); its start, size, phase and divisor follow from the
    // step's own read (:161-176, :284-285), so those four words go out while the kernel runs and
    // the frequency right after vt_finish -- the EKF update and the next prediction then run
    // beside the next step's kernel. `early`: step s's words are all out; e_*: what was posted,
    // held against what the step computes when it comes (the same functions: the same bits).
    bool early = false;
    std::vector<int64_t> e_off((size_t)n), e_ns((size_t)n);
    std::vector<double> e_phi0((size_t)n), e_rfs((size_t)n), e_f((size_t)n);
    Events ev;
    double kernel_ms = 0;
    int result = GNSS_OK;
    const auto t_loop = std::chrono::steady_clock::now();
    VtStamps stamps;  // (probe builds, GNSS_VT_STAMPS set: the host's share of a step, printed at the end)
    DevBuf d_vtst;    // (... and the loop kernel's per-step marks)
    if (stamps.on && loop_mode) {
        const size_t nst = (size_t)kVtStampSteps * (8 + 4 * kVtLoopMaxBlocks);
        HIP_TRY(d_vtst.alloc(ctx, "vt.stamps", sizeof(unsigned long long) * nst));
        HIP_TRY(hipMemsetAsync(d_vtst.p, 0, sizeof(unsigned long long) * nst, ctx->stream));
    }
    for (int s = 0; s < nsteps && result == GNSS_OK; s++) {
        int64_t need_lo = INT64_MAX, need_hi = 0;
        for (int i = 0; i < n; i++) {
            const VtPrep p = vt_prepare(sg->Fs, sg->codelength, pdi, remChip[i], cf_old[i], cf_old[i]);
            if (p.n < 1) {  // ceil(...) <= 0: an index MATLAB rejects
                result = fail(ctx, GNSS_EINDEX, "step %d channel %d: read size %lld", s + 1, i, (long long)p.n);
                break;
            }
            double cf = cf_old[i], dpr = 0, vel[3];
            st = vt_nav_predict_at(nav, i, p.n, have_ahead[(size_t)i] ? &ahead[(size_t)i] : nullptr, &cf, &dpr, vel);
            if (st) {
                result = fail(ctx, st, "step %d channel %d: svPosVel / trop_UNB3 failed", s + 1, i);
                break;
            }
            cf_new[i] = cf;
            h_cf[i] = cf;
            gnss_vt_out& o = out[(size_t)s * n + i];
            o.deltaPr = dpr;
            o.prRate = 0;
            for (int k = 0; k < 3; k++) o.sv_vel[k] = vel[k];
            need_lo = std::min(need_lo, fptr[i]);
            need_hi = std::max(need_hi, fptr[i] + p.n * bps);
        }
        if (result) break;
        if (!file->dev_data && (need_lo < w.base || need_hi > w.base + w.len) && need_hi <= flen) {
            if (early)  // (an early post checked the same reads against this window)
                return fail(ctx, GNSS_EDEVICE, "step %d: posted early, then re-staged", s + 1);
            HIP_TRY(stop_loop());
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            if ((st = win.restage(need_lo))) return st;
            if (need_lo < w.base || need_hi > w.base + w.len)
                return fail(ctx, GNSS_EDEVICE, "step %d: the restaged IF window [%lld, %lld) does not cover the reads [%lld, %lld)",
                            s + 1, (long long)w.base, (long long)(w.base + w.len), (long long)need_lo, (long long)need_hi);
        }
        A.rec = reinterpret_cast<const uint8_t*>(w.ptr);
        A.base = w.base;
        A.len = w.len;
        if (multi) {  // (per-step events only in profiling mode: each is a queue command)
            // the step's reads (:161-176, :217-249): what vt_step_kernel sums, and what stops a
            // channel (a replica index MATLAB rejects, a read past the end of the record)
            for (int i = 0; i < n; i++) {
                const gnss_vt_chan& c = hc[(size_t)i];
                const double cf = cf_new[i];
                const VtPrep p = vt_prepare(sg->Fs, sg->codelength, pdi, c.remChip, c.codeFreq, cf);
                int b = !(cf > 0) ? GNSS_EARG : p.bad;
                if (!b) {
                    const int64_t a0 = c.file_ptr, need = p.n * bps;
                    if (a0 + need > flen) b = GNSS_EIO;
                    else if (a0 < w.base || a0 + need > w.base + w.len) b = GNSS_EIO;  // (outside the window)
                }
                pk[(size_t)i] = p;
                bad[(size_t)i] = b;
                B.ns[i] = b ? 0 : p.n;
                B.off[i] = b ? 0 : c.file_ptr - w.base;
                B.f[i] = c.carrFreq;
                B.phi0[i] = c.remCarrPhase;
                B.rfs[i] = recip.of(B.ns[i]);
            }
            B.rec = A.rec;
            B.seq = (unsigned)s + 1;
            if (loop_mode && early) {  // (the kernel has the step: its words were posted early)
                for (int i = 0; i < n; i++) {
                    if (bad[(size_t)i]) continue;  // (it sums the read; the channel stops below)
                    if (B.off[i] != e_off[(size_t)i] || B.ns[i] != e_ns[(size_t)i] ||
                        std::memcmp(&B.phi0[i], &e_phi0[(size_t)i], 8) || std::memcmp(&B.rfs[i], &e_rfs[(size_t)i], 8))
                        return fail(ctx, GNSS_EDEVICE, "step %d channel %d: the early post differs from the step", s + 1,
                                    i);
                }
            } else if (loop_mode) {
                if (!running) {  // (every device tag back to 0: a stopped launch left kVtLoopStop, a former call its steps)
                    HIP_TRY(hipMemsetAsync(d_loop.p, 0, loop_bytes, ctx->stream));
                    const VtLoopArgs L{B.rec, w.len, B.Fs, B.real8, B.seq, mail, gsums, loop_timeout, d_loop.p,
                                       d_loop.as<char>() + gstep_bytes, d_vtst.as<unsigned long long>()};
                    HIP_TRY(launch_vt_loop(L, n, nb, ctx->stream));
                    running = true;
                }
                // the step's reads as granules tagged with its number (VtBlockStep's word order)
                for (int i = 0; i < n; i++)
                    post_step_words(mail, B.seq, n, i, B.off[i], B.ns[i], &B.f[i], B.phi0[i], B.rfs[i]);
            } else {
                if (ctx->profiling) HIP_TRY(hipEventRecord(ev.a, ctx->stream));
                HIP_TRY(launch_vt_step(B, n, nb, ctx->stream));
                if (ctx->profiling) HIP_TRY(hipEventRecord(ev.b, ctx->stream));
            }
        } else {
            HIP_TRY(hipMemcpyAsync(d_cf.p, h_cf, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(hipEventRecord(ev.a, ctx->stream));
            HIP_TRY(launch_vt_run(A, ctx->stream));
            HIP_TRY(hipEventRecord(ev.b, ctx->stream));
            HIP_TRY(hipMemcpyAsync(h_out, d_out.p, sizeof(gnss_vt_out) * (size_t)n, hipMemcpyDeviceToHost,
                                   ctx->stream));
        }
        stamps.mark(VtStamps::kPre);
        vt_nav_gain(*nav, gain.get());
        for (int i = 0; i < n && s + 1 < nsteps; i++) {
            const int64_t ns = nav->numSample[i];
            const double rc = vt_remchip_next(sg->Fs, pdi, remChip[i], cf_new[i], ns);
            const VtPrep q = vt_prepare(sg->Fs, sg->codelength, pdi, rc, cf_new[i], cf_new[i]);
            have_ahead[(size_t)i] = q.n >= 1;
            if (q.n >= 1) vt_orbit(*nav, i, vt_transmit_next(*nav, i, q.n), &ahead[(size_t)i]);
        }
        // the next step's words that need no sums of this one (`early` above)
        bool early_next = loop_mode && s + 1 < nsteps;
        for (int i = 0; i < n && early_next; i++) {
            const gnss_vt_chan& c = hc[(size_t)i];
            if (bad[(size_t)i]) {
                early_next = false;
                break;
            }
            const int64_t n0 = pk[(size_t)i].n;
            const double rc = vt_remchip_next(sg->Fs, pdi, c.remChip, cf_new[i], n0);
            const VtPrep q = vt_prepare(sg->Fs, sg->codelength, pdi, rc, cf_new[i], cf_new[i]);
            const int64_t a0 = c.file_ptr + n0 * bps, need = q.n * bps;
            if (q.n < 1 || a0 + need > flen || a0 < w.base || a0 + need > w.base + w.len) {
                early_next = false;
                break;
            }
            e_off[(size_t)i] = a0 - w.base;
            e_ns[(size_t)i] = q.n;
            e_phi0[(size_t)i] = vt_rem_carr_phase(c.carrFreq, n0, sg->Fs, c.remCarrPhase);
            e_rfs[(size_t)i] = recip.of(q.n);
        }
        for (int i = 0; i < n && early_next; i++)
            post_step_words(mail, B.seq + 1, n, i, e_off[(size_t)i], e_ns[(size_t)i], nullptr, e_phi0[(size_t)i],
                            e_rfs[(size_t)i]);
        stamps.mark(VtStamps::kShadow);
        if (!multi || ctx->profiling) HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (loop_mode) HIP_TRY(wait_granules(ctx->stream, gsums, 2 * n, (unsigned)s + 1, loop_sums.data()));
        else if (multi) HIP_TRY(wait_posted(ctx->stream, B.done, (unsigned)s + 1));
        stamps.mark(VtStamps::kWait);
        if (ctx->profiling || !multi) kernel_ms += ev.ms();
        // loop mode, the next step posted early: its carrier frequencies first (the PLL alone; the
        // rest of vt_finish and the EKF run beside the next step's kernel)
        early = false;
        if (early_next) {
            for (int i = 0; i < n; i++) {
                const double I = loop_sums[2 * i], Q = loop_sums[2 * i + 1];
                const int cp = vt_code_at(pk[(size_t)i].j[1], pdi, [&](int j) {
                    return ((cab[(size_t)i * 32 + (j >> 5)] >> (j & 31)) & 1u) ? -1 : 1;
                });
                e_f[(size_t)i] = vt_pll(hc[(size_t)i], pdi, t1, t2, cp * I, cp * Q).carrFreq;
                post_step_freq(mail, B.seq + 1, n, i, e_f[(size_t)i]);
            }
            early = true;
        }
        for (int i = 0; multi && i < n; i++) {  // each channel's scalar end
            gnss_vt_out& h = h_out[i];
            h = gnss_vt_out{};
            if (bad[(size_t)i]) {
                h.status = bad[(size_t)i];
                continue;
            }
            const double* sum = loop_mode ? loop_sums.data() : B.sums;
            const double I = sum[2 * i], Q = sum[2 * i + 1];
            const unsigned* cb = &cab[(size_t)i * 32];
            int code[3];
            for (int t = 0; t < 3; t++)
                code[t] = vt_code_at(pk[(size_t)i].j[t], pdi, [&](int j) { return ((cb[j >> 5] >> (j & 31)) & 1u) ? -1 : 1; });
            const int st2 = vt_finish(sg->Fs, sg->ms, pdi, bps, t1, t2, &hc[(size_t)i], pk[(size_t)i], code, cf_new[i],
                                      I, Q, &h);
            if (st2) h.status = st2;
        }
        for (int i = 0; early && i < n; i++)  // (vt_finish's frequency is the one posted: the same vt_pll)
            if (!h_out[i].status && std::memcmp(&hc[(size_t)i].carrFreq, &e_f[(size_t)i], 8))
                return fail(ctx, GNSS_EDEVICE, "step %d channel %d: the early carrier frequency differs", s + 1, i);
        for (int i = 0; i < n; i++) {
            gnss_vt_out& o = out[(size_t)s * n + i];
            const gnss_vt_out& h = h_out[i];
            const double dpr = o.deltaPr, vel[3] = {o.sv_vel[0], o.sv_vel[1], o.sv_vel[2]};
            o = h;
            o.deltaPr = dpr;
            o.prRate = 0;
            for (int k = 0; k < 3; k++) o.sv_vel[k] = vel[k];
            if (h.status) {
                if (!result) result = fail(ctx, h.status, "step %d channel %d stopped (replica index / read past EOF)",
                                           s + 1, i);
                continue;
            }
            ctx->timing.track_channel_samples += h.numSample;
            remChip[i] = h.remChip;
            cf_old[i] = h.codeFreq;
            fptr[i] = h.absoluteSample;
            codeError[i] = h.codeError;
            carrFreq[i] = h.carrFreq;
        }
        ctx->timing.track_launches += 1;
        if (result) break;
        st = vt_nav_correct(nav, *gain, codeError.data(), cf_new.data(), carrFreq.data(), sol ? sol + s : nullptr);
        if (st) result = fail(ctx, st, "step %d: navigation update failed (singular innovation covariance)", s + 1);
        stamps.mark(VtStamps::kPost);
    }
    if (stamps.on) {
        if (d_vtst.p) HIP_TRY(stop_loop());
        if ((st = report_vt_stamps(ctx, nsteps, stamps, d_vtst))) return st;
    }
    HIP_TRY(stop_loop());
    if (!multi) HIP_TRY(hipMemcpyAsync(chans, d_chan.p, sizeof(gnss_vt_chan) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (multi) std::copy(hc.begin(), hc.end(), chans);
    vt_loop_timing(ctx, kernel_ms, t_loop);  // (int8 records: the kernels' time in profiling mode only)
    return result;
}

namespace {
// trackingVT_POS_updated_multicorrelator.m:151-609, the 25-tap loop behind gnss_tracking_vt_mc_run
// (nav == nullptr: each step's code frequency is the caller's, series[s * n + i]) and
// gnss_tracking_vt_mc (the EKF predicts it, :172-218, and takes the step's discriminators,
// :472-609, with prr_measured from carrFreq - IF). Per step the host sizes each channel's read
// and its 25 colons (vt_mc_prepare), clears the read against the file's length and the staged
// window, launches the correlator once for all channels (vt_mc_step_kernel; int16 records: the
// read's integer sums first), waits for the step's number in coherent host memory
// (wait_posted) and runs each channel's scalar end on the 50 sums (vt_mc_finish). The channel
// states stay on the host. A channel whose step fails gets the status in its record and reads
// nothing; under the EKF the loop ends at that step, else the channel sits the later steps out.
int vt_mc_loop(gnss_ctx* ctx, const gnss_file* file, const gnss_signal* sg, const gnss_track* tr, int pdi, int n,
               int nsteps, gnss_vt_chan* chans, const double* series, gnss_vt_nav* nav, gnss_vt_mc_out* out,
               gnss_vt_navsol* sol)
{
    ctx->err.clear();
    ctx->timing = gnss_timing{};
    HIP_TRY(hipSetDevice(ctx->device));
    const int prec = file->dataPrecision, dtyp = file->dataType;
    int bps, st;
    int64_t flen;
    if ((st = vt_record(ctx, file, &bps, &flen))) return st;
    if ((st = vt_check_chans(ctx, chans, n, bps, true, nav, true))) return st;
    for (int64_t k = 0; series && k < (int64_t)nsteps * n; k++)
        if (!(series[k] > 0)) return fail(ctx, GNSS_EARG, "code frequencies must be positive");
    std::memset(out, 0, sizeof(gnss_vt_mc_out) * (size_t)nsteps * n);
    // The IF window, as gnss_tracking_vt's, re-staged at least as long as the step's reads need
    VtWindow win(ctx, file, sg, pdi, nsteps, bps, flen);
    IfWindow& w = win.w;
    const int64_t nominal = win.nominal;
    if ((st = win.stage_first(chans, n))) return st;
    const std::vector<unsigned> cab = vt_ca_table(chans, n);
    double t1, t2;
    calc_loop_coef(tr->PLLBW, tr->PLLDamp, tr->PLLGain, t1, t2);
    int nb = (int)std::min<int64_t>(std::max<int64_t>(1, (nominal + kVtMcStepSamples - 1) / kVtMcStepSamples),
                                    GNSS_VT_MAX_BLOCKS);
    if (ctx->opt[GNSS_OPT_VT_BLOCKS] > 0) nb = (int)ctx->opt[GNSS_OPT_VT_BLOCKS];
    DevBuf d_ca, d_part, d_ticket, d_isum;
    VtMcStepArgs B{};
    VtRecip recip;
    if ((st = vt_step_setup(ctx, "vtmc.sums", (size_t)kVtMcSums * n, sg->Fs, nominal, B, d_ticket, recip))) return st;
    HIP_TRY(d_ca.alloc(ctx, "vt.ca", sizeof(unsigned) * cab.size()));
    HIP_TRY(hipMemcpyAsync(d_ca.p, cab.data(), sizeof(unsigned) * cab.size(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(d_part.alloc(ctx, "vtmc.part", sizeof(double) * kVtMcSums * (size_t)n * nb));
    if (prec == 2) HIP_TRY(d_isum.alloc(ctx, "vtmc.isum", sizeof(long long) * 2 * GNSS_VT_MAX_CH));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // (cab is read by the copy until here)
    B.ca_bits = d_ca.as<unsigned>();
    B.part = d_part.as<double>();
    B.isum = prec == 2 ? d_isum.as<long long>() : nullptr;
    B.fmt = prec == 2 ? 2 : (dtyp == 1 ? 1 : 0);
    std::vector<gnss_vt_chan> hc(chans, chans + n);
    std::vector<VtMcPrep> pk((size_t)n);
    std::vector<int> bad((size_t)n, 0), stopped((size_t)n, 0);
    std::vector<double> cf_new((size_t)n), dpr((size_t)n, 0.0), vel(3 * (size_t)n, 0.0), codeError((size_t)n),
        carrFreq((size_t)n);
    std::unique_ptr<VtGain> gain(nav ? new VtGain : nullptr);
    Events ev;
    double kernel_ms = 0;
    int result = GNSS_OK, first = GNSS_OK;  // (first: the first channel status, and its message)
    std::string first_err;
    const auto t_loop = std::chrono::steady_clock::now();
    for (int s = 0; s < nsteps && result == GNSS_OK; s++) {
        // this step's code frequencies: the caller's, or the EKF's prediction from the read size
        // the LAST code frequency gives (:155, :172-218)
        for (int i = 0; i < n; i++) {
            if (!nav) {
                cf_new[(size_t)i] = series[(size_t)s * n + i];
                continue;
            }
            const gnss_vt_chan& c = hc[(size_t)i];
            const VtMcPrep p = vt_mc_prepare(sg->Fs, sg->codelength, pdi, c.remChip, c.codeFreq, c.codeFreq);
            if (p.n < 1) {
                result = fail(ctx, GNSS_EINDEX, "step %d channel %d: read size %lld", s + 1, i, (long long)p.n);
                break;
            }
            double cf = c.codeFreq;
            st = vt_nav_predict_at(nav, i, p.n, nullptr, &cf, &dpr[(size_t)i], &vel[3 * (size_t)i]);
            if (st) {
                result = fail(ctx, st, "step %d channel %d: svPosVel / trop_UNB3 failed", s + 1, i);
                break;
            }
            cf_new[(size_t)i] = cf;
        }
        if (result) break;
        // the step's reads: sized and cleared here, before anything is launched
        int64_t need_lo = INT64_MAX, need_hi = 0;
        for (int i = 0; i < n; i++) {
            const gnss_vt_chan& c = hc[(size_t)i];
            int b = 0;
            if (stopped[(size_t)i]) {
                pk[(size_t)i] = VtMcPrep{};
            } else {
                pk[(size_t)i] = vt_mc_prepare(sg->Fs, sg->codelength, pdi, c.remChip, c.codeFreq, cf_new[(size_t)i]);
                b = !(cf_new[(size_t)i] > 0) ? GNSS_EARG : pk[(size_t)i].bad;
                // a short fread makes `rawsignal .* carrsig` fail in MATLAB (:158-164, :290)
                if (!b && c.file_ptr + pk[(size_t)i].n * bps > flen) b = GNSS_EIO;
            }
            bad[(size_t)i] = b;
            if (!b && !stopped[(size_t)i]) {
                need_lo = std::min(need_lo, c.file_ptr);
                need_hi = std::max(need_hi, c.file_ptr + pk[(size_t)i].n * bps);
            }
        }
        if (need_hi > 0 && !file->dev_data && (need_lo < w.base || need_hi > w.base + w.len)) {
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            if ((st = win.restage(need_lo, need_hi))) return st;
        }
        int live = 0;
        for (int i = 0; i < n; i++) {
            const gnss_vt_chan& c = hc[(size_t)i];
            const bool run = !bad[(size_t)i] && !stopped[(size_t)i];
            if (run && (c.file_ptr < w.base || c.file_ptr + pk[(size_t)i].n * bps > w.base + w.len))
                return fail(ctx, GNSS_EDEVICE, "step %d channel %d: the staged IF window [%lld, %lld) does not cover the read",
                            s + 1, i, (long long)w.base, (long long)(w.base + w.len));
            B.ns[i] = run ? pk[(size_t)i].n : 0;
            B.off[i] = run ? c.file_ptr - w.base : 0;
            B.f[i] = c.carrFreq;
            B.phi0[i] = c.remCarrPhase;
            B.rfs[i] = recip.of(B.ns[i]);
            B.remChip[i] = c.remChip;
            B.cps[i] = cf_new[(size_t)i] / sg->Fs;
            live += run;
        }
        B.rec = reinterpret_cast<const uint8_t*>(w.ptr);
        B.seq = (unsigned)s + 1;
        if (live) {
            if (ctx->profiling) HIP_TRY(hipEventRecord(ev.a, ctx->stream));
            if (prec == 2) {
                HIP_TRY(hipMemsetAsync(d_isum.p, 0, sizeof(long long) * 2 * GNSS_VT_MAX_CH, ctx->stream));
                HIP_TRY(launch_vt_mc_isum(B.rec, B.off, B.ns, n, d_isum.as<long long>(), ctx->stream));
            }
            HIP_TRY(launch_vt_mc_step(B, n, nb, ctx->stream));
            if (ctx->profiling) HIP_TRY(hipEventRecord(ev.b, ctx->stream));
            if (nav) vt_nav_gain(*nav, gain.get());  // (needs the predictions only: beside the kernel)
            if (ctx->profiling) HIP_TRY(hipStreamSynchronize(ctx->stream));
            HIP_TRY(wait_posted(ctx->stream, B.done, B.seq));
            if (ctx->profiling) kernel_ms += ev.ms();
            ctx->timing.track_launches += 1;
        }
        for (int i = 0; i < n; i++) {  // each channel's scalar end
            gnss_vt_mc_out& o = out[(size_t)s * n + i];
            if (stopped[(size_t)i]) continue;
            if (bad[(size_t)i]) {
                o.status = bad[(size_t)i];
                stopped[(size_t)i] = 1;
                if (!first) {
                    first = fail(ctx, o.status, "step %d channel %d stopped (replica index / read past EOF)", s + 1, i);
                    first_err = ctx->err;
                }
                continue;
            }
            const double* sum = B.sums + (size_t)kVtMcSums * i;
            vt_mc_finish(sg->Fs, sg->ms, pdi, bps, t1, t2, &hc[(size_t)i], pk[(size_t)i], cf_new[(size_t)i], sum,
                         sum + kVtMcTaps, &o);
            o.deltaPr = dpr[(size_t)i];
            for (int k = 0; k < 3; k++) o.sv_vel[k] = vel[3 * (size_t)i + k];
            ctx->timing.track_channel_samples += o.numSample;
            codeError[(size_t)i] = o.codeError;
            carrFreq[(size_t)i] = o.carrFreq;
        }
        // (the tracking half alone: the other channels go on while any is left)
        if (first && (nav || std::find(stopped.begin(), stopped.end(), 0) == stopped.end())) break;
        if (!nav) continue;
        st = vt_nav_correct(nav, *gain, codeError.data(), cf_new.data(), carrFreq.data(), sol ? sol + s : nullptr, true);
        if (st) result = fail(ctx, st, "step %d: navigation update failed (singular innovation covariance)", s + 1);
    }
    if (!result && first) {
        ctx->err = first_err;
        result = first;
    }
    std::copy(hc.begin(), hc.end(), chans);
    vt_loop_timing(ctx, kernel_ms, t_loop);
    return result;
}
}  // namespace

int gnss_tracking_vt_mc_run(gnss_ctx* ctx, const gnss_file* file, const gnss_signal* sg, const gnss_track* tr,
                            int32_t pdi, int32_t n, int32_t nsteps, gnss_vt_chan* chans, const double* codeFreq_new,
                            gnss_vt_mc_out* out)
{
    if (!ctx || !file || !sg || !tr || !chans || !codeFreq_new || !out || n < 1 || n > GNSS_VT_MAX_CH || pdi < 1 ||
        nsteps < 1 || !(sg->Fs > 0) || !(sg->codeFreqBasis > 0))
        return fail(ctx, GNSS_EARG, "bad arguments (n in 1..GNSS_VT_MAX_CH)");
    return vt_mc_loop(ctx, file, sg, tr, pdi, n, nsteps, chans, codeFreq_new, nullptr, out, nullptr);
}

int gnss_tracking_vt_mc(gnss_ctx* ctx, const gnss_file* file, const gnss_signal* sg, const gnss_track* tr, int32_t n,
                        int32_t nsteps, gnss_vt_chan* chans, gnss_vt_nav* nav, gnss_vt_mc_out* out, gnss_vt_navsol* sol)
{
    if (!ctx || !file || !sg || !tr || !chans || !nav || !out || n < 1 || n > GNSS_VT_MAX_CH || n != nav->n ||
        nsteps < 0 || !(sg->Fs > 0) || !(sg->codeFreqBasis > 0) || sg->Fs != nav->Fs)
        return fail(ctx, GNSS_EARG, "bad arguments (n in 1..GNSS_VT_MAX_CH and equal to nav->n, signal as at gnss_vt_nav_init)");
    if (nsteps == 0) {
        ctx->err.clear();
        ctx->timing = gnss_timing{};
        return GNSS_OK;
    }
    return vt_mc_loop(ctx, file, sg, tr, nav->pdi, n, nsteps, chans, nullptr, nav, out, sol);
}

}  // extern "C"
