// api_track.cpp -- trackingCT.m and its siblings on the host side of the C-ABI:
//   trackingCT.m   : phase A (1 ms) -> bit-edge search -> phase B (= A continued,
//                    quirk A.9) -> phase C (10 ms) per channel, channels batched.
// Stages the IF window (host.h), chooses the lane geometry (track_geom.h) and drives the
// kernels in track.hip; a multi-device context deals the channels over its members (group.h).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "host.h"
#include "track_geom.h"

using namespace gnss;
using namespace gnss::host;

static_assert(geom::kLaneThreads == kTrkThreads && geom::kVpbMax == kMaxVpb, "track_geom.h restates the kernels' constants");

namespace gnss {
namespace host {

// The sampling-rate floor of the tracking kernels (gnss_tracking_ct and its variants,
// gnss_correlate_step): a lane correlates 8 samples at least and may hold one chip boundary
// per tap, so 8 * codeFreq / Fs must stay below 1 for every code rate of the call -- the
// nominal rate with 1 % for the DLL's excursions, and a caller-given code frequency where
// there is one. The kernels flag a violating step with GNSS_EINDEX (d * M >= 1), which the
// header keeps for indices MATLAB would reject; MATLAB runs such a rate, so the host
// refuses it before any launch with GNSS_EARG. One predicate for every entry point: what it
// admits, the kernels run.
bool lane_rate_admitted(const gnss_signal* sg, double codeFreq_max)
{
    return sg->Fs > 0 && 8.0 * std::max(sg->codeFreqBasis * 1.01, codeFreq_max) / sg->Fs < 1.0;
}

int refuse_lane_rate(gnss_ctx* ctx, const gnss_signal* sg, double codeFreq_max)
{
    return fail(ctx, GNSS_EARG,
                "Fs = %.9g Hz is below the sampling-rate floor of the tracking kernels: Fs must exceed "
                "8 x the code rate (%.9g Hz with the 1 %% margin, i.e. Fs > %.9g Hz)",
                sg->Fs, std::max(sg->codeFreqBasis * 1.01, codeFreq_max),
                8.0 * std::max(sg->codeFreqBasis * 1.01, codeFreq_max));
}

}  // namespace host
}  // namespace gnss

// The sibling loop of trackingCT_POS_updated.m (its tracking half): steps and countinx.
struct PosCfg {
    int32_t ctPOS;            // track.ctPOS (datalength, trackingCT_POS_updated.m:50)
    const int32_t* countinx;  // countinx(svIndex) of countinx.mat (:29), by channel position
    // 0: trackingCT_POS_updated.m. 1 or 10: trackingCT_POS_updated_multicorrelator.m, every
    // step at this pdi (track.pdi, :46), 25 taps, ctPOS = datalength/pdi steps (:170)
    int32_t mc_pdi;
};

// trackingCT_multiCorr-GIVEN.m (function trackingCT_multiCorr): `datalength` 1-ms steps
// per channel (:27, hard-coded 50000 there), trackingCT conventions otherwise
struct GivenCfg {
    int32_t datalength;
};

static int tracking_impl(gnss_ctx* ctx, const gnss_file* file, const gnss_signal* sg, const gnss_track* tr,
                         const gnss_acquired* acq, gnss_track_out* out, const PosCfg* pos,
                         const GivenCfg* gv, const int32_t* dev_slot);

// trackingCT.m's channel loop (:22-528) dealt over the members. Host outputs: every member
// writes its channels' rows of the caller's arrays (disjoint). GNSS_OUT_DEVICE: a member on
// the output's device expands into it directly; another expands into a buffer of its own HBM
// and copies each channel's contiguous row block over xGMI.
static int group_tracking(gnss_ctx* g, const gnss_file* file, const gnss_signal* sg, const gnss_track* tr,
                          const gnss_acquired* acq, gnss_track_out* out, const PosCfg* pos)
{
    if (!file || !sg || !tr || !acq || !out) return GNSS_EARG;
    g->timing = gnss_timing{};
    const int nsv = acq->n;
    std::vector<int32_t> chans;
    if (tr->chan && tr->n_chan > 0) chans.assign(tr->chan, tr->chan + tr->n_chan);
    else for (int i = 0; i < nsv; i++) chans.push_back(i);
    bool ok = nsv > 0 && nsv <= GNSS_MAX_SV;
    for (int c : chans) ok = ok && c >= 0 && c < nsv;
    if (!ok) return tracking_impl(g, file, sg, tr, acq, out, pos, nullptr, nullptr);  // (its own error)
    const int M = (int)g->members.size();
    const auto shards = group::deal((int)chans.size(), M);
    const bool odev = (out->flags & GNSS_OUT_DEVICE) != 0;
    int outdev = g->device;
    if (odev && (out->rec || out->taps)) {
        const int d = pointer_device(out->rec ? (const void*)out->rec : (const void*)out->taps);
        if (d >= 0) outdev = d;
    }
    const int ntaps = pos ? (pos->mc_pdi ? GNSS_MC_TAPS : 3) : (tr->n_taps > 0 ? tr->n_taps : 3);
    const int64_t ML = out->max_len;
    const size_t rec_blk = (size_t)GNSS_NFIELDS * (size_t)ML, tap_blk = (size_t)2 * ntaps * (size_t)ML;
    std::vector<group::TrackStatus> ts((size_t)M, group::TrackStatus{GNSS_OK, 0});
    std::vector<int32_t> rows((size_t)M, 0);
    std::vector<char> ran((size_t)M, 0);
    for_members(g, [&](int k) {
        gnss_ctx* m = g->members[(size_t)k];
        std::vector<int32_t> mine;
        for (int i : shards[(size_t)k]) mine.push_back(chans[(size_t)i]);
        if (mine.empty()) return;
        ran[(size_t)k] = 1;
        gnss_track t = *tr;
        t.chan = mine.data();
        t.n_chan = (int32_t)mine.size();
        gnss_track_out o = *out;
        const bool remote = odev && (m->device != outdev || m->opt[GNSS_OPT_FORCE_PEER] != 0);
        DevBuf lrec, ltap;
        std::vector<int32_t> slot(mine.size());
        auto set_err = [&](int st, const char* what) {
            ts[(size_t)k] = group::TrackStatus{st, -1};
            m->err = what;
        };
        if (remote) {
            for (size_t i = 0; i < mine.size(); i++) slot[i] = (int32_t)i;
            if (hipSetDevice(m->device) != hipSuccess ||
                (out->rec && lrec.alloc(m, "grp.rec", sizeof(double) * rec_blk * mine.size()) != hipSuccess) ||
                (out->taps && ltap.alloc(m, "grp.taps", sizeof(double) * tap_blk * mine.size()) != hipSuccess)) {
                set_err(GNSS_EDEVICE, "multi-device tracking: member output buffers");
                return;
            }
            o.rec = out->rec ? lrec.as<double>() : nullptr;
            o.taps = out->taps ? ltap.as<double>() : nullptr;
        }
        const int st = tracking_impl(m, file, sg, &t, acq, &o, pos, nullptr, remote ? slot.data() : nullptr);
        // the failing channel's POSITION in the call's channel list (the one-context rule picks the
        // first failing channel in tr->chan order, which need not be ascending)
        ts[(size_t)k] = group::TrackStatus{st, group::fail_position(shards[(size_t)k], chans, m->fail_chan)};
        rows[(size_t)k] = o.cn0_rows;
        if (st != GNSS_OK || !remote) return;
        bool copied = true;
        for (size_t i = 0; i < mine.size() && copied; i++) {
            const int64_t c = mine[i];
            if (out->rec)
                copied = hipMemcpyPeerAsync(out->rec + c * (int64_t)rec_blk, outdev, lrec.as<double>() + i * rec_blk,
                                            m->device, sizeof(double) * rec_blk, m->stream) == hipSuccess;
            if (copied && out->taps)
                copied = hipMemcpyPeerAsync(out->taps + c * (int64_t)tap_blk, outdev, ltap.as<double>() + i * tap_blk,
                                            m->device, sizeof(double) * tap_blk, m->stream) == hipSuccess;
        }
        if (!copied || hipStreamSynchronize(m->stream) != hipSuccess) set_err(GNSS_EDEVICE, "multi-device tracking: peer copy of the rows");
    });
    std::vector<gnss_timing> tm;
    for (int k = 0; k < M; k++)
        if (ran[(size_t)k]) tm.push_back(g->members[(size_t)k]->timing);
    g->timing = group::combine_timing(tm);
    const int status = group::tracking_status(ts);
    if (status != GNSS_OK) {
        if (out->len) for (int c : chans) out->len[c] = 0;
        for (int k = 0; k < M; k++)
            if (ts[(size_t)k].status == status)
                return fail(g, status, "member %d (device %d): %s", k, g->members[(size_t)k]->device,
                            g->members[(size_t)k]->err.c_str());
        return fail(g, status, "multi-device tracking failed");
    }
    int32_t r = 0;
    for (int k = 0; k < M; k++)
        if (ran[(size_t)k]) r = std::max(r, rows[(size_t)k]);
    out->cn0_rows = r;
    return GNSS_OK;
}

// ---------------------------------------------------------------------------
// trackingCT.m
// ---------------------------------------------------------------------------
namespace {

struct StepGraph {
    hipGraphExec_t exec = nullptr;
    hipGraph_t graph = nullptr;
    int count = 0;
    ~StepGraph()
    {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
    }
};

// GNSS_HOSTPROF (probe builds): the host-side phases of a call on stderr
struct HostProf {
    const bool on = probe_env("GNSS_HOSTPROF") != nullptr;
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void mark(const char* phase) const
    {
        if (!on) return;
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        fprintf(stderr, "hostprof %s %.3f ms\n", phase, ms);
    }
};

// GNSS_STAMPS (probe builds): channel 0's per-launch wall-clock stamps into the file `path`
int write_stamps(gnss_ctx* ctx, const char* path, const DevBuf& d_stamps)
{
    std::vector<unsigned long long> st(d_stamps.n / sizeof(unsigned long long));
    HIP_TRY(hipMemcpy(st.data(), d_stamps.p, d_stamps.n, hipMemcpyDeviceToHost));
    if (FILE* fp = fopen(path, "wb")) {
        fwrite(st.data(), sizeof(unsigned long long), st.size(), fp);
        fclose(fp);
    }
    return GNSS_OK;
}

// The MATLAB layout of the compact per-step records: one row per millisecond, each 10-ms step's
// value on its ten rows (trackingCT.m:507-524). Channel i (chans[i], n1[i] rows before the 10-ms
// values) from the host copies rec / tp into out->rec / out->taps, or (GNSS_OUT_DEVICE) expanded
// on the GPU from d_rec / d_taps straight into the caller's device arrays, row block slot[i].
int expand_records(gnss_ctx* ctx, const gnss_track_out* out, const std::vector<int32_t>& chans,
                   const std::vector<int64_t>& n1, int n10, int ntaps, int64_t rec_cap, const double* rec,
                   const double* tp, const DevBuf& d_rec, const DevBuf& d_taps, const int32_t* dev_slot)
{
    const int nch = (int)chans.size();
    const int64_t ML = out->max_len;
    const int nrf = out->rec ? GNSS_NFIELDS : 0, ntf = out->taps ? 2 * ntaps : 0;
    if (out->flags & GNSS_OUT_DEVICE) {
        std::vector<int64_t> job(2 * (size_t)nch);
        for (int i = 0; i < nch; i++) {
            job[2 * i] = n1[i];
            job[2 * i + 1] = dev_slot ? dev_slot[i] : chans[i];
        }
        DevBuf d_job;
        HIP_TRY(d_job.alloc(ctx, "trk.d_job", sizeof(int64_t) * job.size()));
        HIP_TRY(hipMemcpyAsync(d_job.p, job.data(), sizeof(int64_t) * job.size(), hipMemcpyHostToDevice, ctx->stream));
        if (nrf)
            HIP_TRY(launch_track_expand(d_rec.as<double>(), rec_cap, GNSS_NFIELDS, GNSS_NFIELDS, nch,
                                        d_job.as<int64_t>(), out->rec, ML, n10, 0, ctx->stream));
        if (ntf)
            HIP_TRY(launch_track_expand(d_taps.as<double>(), rec_cap, 2 * ntaps, 2 * ntaps, nch,
                                        d_job.as<int64_t>(), out->taps, ML, n10, ntaps, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return GNSS_OK;
    }
    parallel_for(nch * (nrf + ntf), [&](int task) {
        const int i = task / (nrf + ntf), f = task % (nrf + ntf);
        const int c = chans[i];
        const int64_t n1i = n1[i];
        double* dst;
        const double* src;
        int64_t stride;
        if (f < nrf) {
            dst = out->rec + ((int64_t)c * GNSS_NFIELDS + f) * ML;
            src = rec + (size_t)i * rec_cap * GNSS_NFIELDS + f;
            stride = GNSS_NFIELDS;
        } else {
            const int tq = f - nrf, sidx = tq / 2, iq = tq % 2;
            dst = out->taps + (((int64_t)c * 2 + iq) * ntaps + sidx) * ML;
            src = tp + (size_t)i * rec_cap * 2 * ntaps + tq;
            stride = 2 * ntaps;
        }
        for (int64_t k = 0; k < n1i; k++) dst[k] = src[k * stride];
        for (int64_t q = 0; q < n10; q++) {
            const double v = src[(n1i + q) * stride];
            for (int r = 0; r < 10; r++) dst[n1i + 10 * q + r] = v;
        }
        for (int64_t k = n1i + 10 * n10; k < ML; k++) dst[k] = 0;  // (a reused buffer's tail)
    });
    return GNSS_OK;
}

// codedelay = Codedelay + sum(delayValue(1:msIndex)) (trackingCT_multiCorr-GIVEN.m:297):
// delayValue is ONE nsv x datalength matrix (:29) filled channel after channel, so the
// linear (column-major) sum takes the earlier channels' rows whole and this channel's
// own row up to msIndex (rows of later channels are still zero)
void given_codedelay(const gnss_track_out* out, const gnss_acquired* acq, int nsv, int N1)
{
    const int64_t ML = out->max_len;
    for (int c = 0; c < nsv; c++) {
        double* cdr = out->rec + ((int64_t)c * GNSS_NFIELDS + GNSS_F_codedelay) * ML;
        double sum = 0;
        for (int64_t k = 0; k < N1; k++) {  // linear position k + 1
            const int r = (int)(k % nsv);
            if (r <= c) sum += out->rec[((int64_t)r * GNSS_NFIELDS + GNSS_F_delayValue) * ML + k / nsv];
            cdr[k] = (double)acq->codedelay[c] + sum;
        }
    }
}

// CN0_Eph: channel i's r1[i] rows of the 1-ms phases' C/N0, its first r10 rows overwritten by the
// 10-ms phase's (trackingCT.m:420-470), zeros up to cn0_cap
void copy_cn0(const gnss_track_out* out, const std::vector<int32_t>& chans, int nsv, const std::vector<int>& r1,
              int r10, const std::vector<double>& cn1, const std::vector<double>& cn10, int64_t cn0_cap)
{
    for (size_t i = 0; i < chans.size(); i++) {
        const int c = chans[i];
        for (int r = 0; r < out->cn0_cap; r++) {
            double v = 0;
            if (r < r10) v = cn10[i * cn0_cap + r];
            else if (r < r1[i]) v = cn1[i * cn0_cap + r];
            out->CN0_Eph[(int64_t)r * nsv + c] = v;
        }
    }
}

}  // namespace

// trackingCT.m (pos == gv == nullptr), the tracking loop of trackingCT_POS_updated.m (pos)
// or of trackingCT_multiCorr-GIVEN.m (gv)
// dev_slot (a group member whose GNSS_OUT_DEVICE rows go through a buffer of its own): channel
// i of the call expands into row block dev_slot[i] of out->rec / out->taps instead of chans[i].
static int tracking_impl(gnss_ctx* ctx, const gnss_file* file, const gnss_signal* sg, const gnss_track* tr,
                         const gnss_acquired* acq, gnss_track_out* out, const PosCfg* pos,
                         const GivenCfg* gv = nullptr, const int32_t* dev_slot = nullptr)
{
    if (ctx) ctx->fail_chan = -1;
    const HostProf hp;
    if (!ctx || !file || !sg || !tr || !acq || !out) return GNSS_EARG;
    HIP_TRY(hipSetDevice(ctx->device));
    ctx->timing = gnss_timing{};
    const int prec = file->dataPrecision, dtyp = file->dataType;
    if ((prec != 1 && prec != 2) || (dtyp != 1 && dtyp != 2))
        return fail(ctx, GNSS_EARG, "dataPrecision must be 1 (int8) or 2 (int16), dataType 1 (I) or 2 (I/Q)");
    if (pos && prec != 1)
        // trackingCT_POS_updated.m:196,207 reads numSample*dataType int16 values but advances
        // file_ptr by numSample*dataType BYTES: overlapping, misaligned reads (not reproduced)
        return fail(ctx, GNSS_EARG, "trackingCT_POS_updated: int8 records only");
    if (gv && (prec != 1 || dtyp != 2 || gv->datalength <= 0 || tr->n_taps != 0 || (tr->chan && tr->n_chan > 0)))
        // :47-48 forms every int8 record as I/Q pairs; codedelay sums the other channels' rows
        // (the whole channel set, below)
        return fail(ctx, GNSS_EARG, "trackingCT_multiCorr: int8 I/Q, datalength > 0, all channels");
    if (pos && (pos->ctPOS <= 0 || (!pos->countinx && !pos->mc_pdi) || tr->n_taps != 0))
        return fail(ctx, GNSS_EARG, "trackingCT_POS_updated: ctPOS > 0, countinx and E/P/L taps required");
    if (prec == 2 && dtyp == 1) {
        // fread(numSample, 'int16') de-interleaved as I/Q (trackingCT.m:84-88): an odd
        // numSample gives I and Q halves of unequal length (MATLAB raises), an even one
        // numSample/2 samples against numSample carrier values -> "Not enough raw data"
        // (:108-112). Every channel's first step has remChip 0 and codeFreq = codeFreqBasis.
        const double n0 = std::round((sg->codelength * 1 - 0.0) / (sg->codeFreqBasis / sg->Fs));
        if (out->len) for (int c = 0; c < acq->n; c++) out->len[c] = 0;
        if (std::fmod(n0, 2.0) != 0) return fail(ctx, GNSS_EINDEX, "int16 real record: odd numSample (MATLAB error)");
        return fail(ctx, GNSS_ENODATA, "Not enough raw data");
    }
    const int nsv = acq->n;
    if (nsv <= 0 || nsv > GNSS_MAX_SV) return fail(ctx, GNSS_EARG, "no channels");
    const int64_t S = sg->Sample;
    const int N1 = gv ? gv->datalength : tr->msToProcessCT_1ms;
    const int n10 = (pos || gv) ? 0 : tr->msToProcessCT_10ms / 10;
    if (!pos && !gv && N1 < 24) return fail(ctx, GNSS_EARG, "msToProcessCT_1ms must be >= 24 (bit-edge search window)");
    if (N1 < 0) return fail(ctx, GNSS_EARG, "msToProcessCT_1ms < 0");
    if (out->max_len < (pos ? (int64_t)pos->ctPOS : gv ? (int64_t)N1 : (int64_t)N1 + 19 + (int64_t)tr->msToProcessCT_10ms))
        return fail(ctx, GNSS_EARG, "max_len too small");
    const bool odev = (out->flags & GNSS_OUT_DEVICE) != 0;  // rec / taps in device memory
    if (odev && gv) return fail(ctx, GNSS_EARG, "GNSS_OUT_DEVICE: not for trackingCT_multiCorr (host codedelay pass)");
    // trackingCT_POS_updated.m: per channel, steps 1..n1 at 1 ms (msIndex <= 1000 +
    // countinx(svIndex), :183), then 10 ms up to ctPOS steps (:294)
    auto pos_n1 = [&](int c) -> int64_t {
        if (pos->mc_pdi) return pos->mc_pdi == 1 ? pos->ctPOS : 0;
        return std::max<int64_t>(0, std::min<int64_t>(pos->ctPOS, (int64_t)N1 + pos->countinx[c]));
    };
    if (!lane_rate_admitted(sg, 0.0)) return refuse_lane_rate(ctx, sg, 0.0);

    // taps (trackingCT.m:24; ACF taps per trackingCT_multiCorr-GIVEN.m:25)
    TrkParams P{};
    double taps3[3] = {-tr->CorrelatorSpacing, 0, tr->CorrelatorSpacing};
    const double* taps = taps3;
    int ntaps = 3;
    // trackingCT_POS_updated.m:42,210-217: Spacing = 0.6:-0.05:-0.6 (colon values 0.5, 0,
    // -0.5 exactly at 3, 13, 23); Early at Spacing(3) = +0.5, Late at Spacing(23) = -0.5,
    // Prompt Code(ceil(t + 0.05) + 1)
    const double taps_pos[3] = {0.5, 0.0, -0.5};
    // trackingCT_POS_updated_multicorrelator.m:41,207-258: all 25 Spacing values as taps,
    // Code(ceil(t) + 2) with Code = [CA(end) CA.. CA(1) CA(2)] (:94,233), no +0.05 on the
    // prompt; E/P/L = Spacing(3)/(13)/(23) feed the loops (:348-359)
    double taps_mc[25];
    if (pos && pos->mc_pdi) {
        const Colon sp = colon_make(0.6, -0.05, -0.6);
        if (sp.n != 24) return fail(ctx, GNSS_EDEVICE, "Spacing colon");
        for (int k = 0; k < 25; k++) taps_mc[k] = colon_elem(sp, k);
        taps = taps_mc;
        ntaps = 25;
        P.conv = 1;
        P.chip_off = 1;
    } else if (gv) {  // Spacing = -0.6:0.05:0.6 (:25), E/P/L = Spacing(3)/(13)/(23) (:94,106,118)
        const Colon sp = colon_make(-0.6, 0.05, 0.6);
        if (sp.n != 24) return fail(ctx, GNSS_EDEVICE, "Spacing colon");
        for (int k = 0; k < 25; k++) taps_mc[k] = colon_elem(sp, k);
        taps = taps_mc;
        ntaps = 25;
        P.given = 1;
    } else if (pos) {
        taps = taps_pos;
        P.conv = 1;
        P.tap_post[1] = 0.05;
    } else if (tr->n_taps > 0) {
        if (!tr->tap_offsets) return fail(ctx, GNSS_EARG, "tap_offsets missing");
        ntaps = tr->n_taps;
        taps = tr->tap_offsets;
    }
    // 25: the taps of trackingCT_multiCorr-GIVEN.m:25 (-0.6:0.05:0.6) and of
    // trackingCT_POS_updated_multicorrelator.m (int8 records: the step kernel's 25-tap build)
    if (ntaps != 3 && ntaps != 11 && ntaps != 25) return fail(ctx, GNSS_EARG, "n_taps must be 3, 11 or 25");
    if (ntaps == 25 && prec != 1) return fail(ctx, GNSS_EARG, "25 taps: int8 records only");
    P.iE = P.iP = P.iL = -1;
    for (int s = 0; s < ntaps; s++) {
        P.taps[s] = taps[s];
        if (pos) continue;
        if (taps[s] == -tr->CorrelatorSpacing && P.iE < 0) P.iE = s;
        if (taps[s] == 0 && P.iP < 0) P.iP = s;
        if (taps[s] == tr->CorrelatorSpacing && P.iL < 0) P.iL = s;
    }
    if (pos) { P.iE = 0; P.iP = 1; P.iL = 2; }
    if ((pos && pos->mc_pdi) || gv) { P.iE = 2; P.iP = 12; P.iL = 22; }
    if (P.iE < 0 || P.iP < 0 || P.iL < 0) return fail(ctx, GNSS_EARG, "taps must contain -spacing, 0, +spacing");
    bool wide_taps = false;
    {
        double lo_t = 1e300, hi_t = -1e300;
        for (int s = 0; s < ntaps; s++) {
            lo_t = std::min(lo_t, taps[s] + P.tap_post[s]);
            hi_t = std::max(hi_t, taps[s] + P.tap_post[s]);
        }
        // the persistent loop's tap window needs every tap's chip at a lane start within one
        // 32-chip run; a wider tap set runs on the per-step path (a path choice, not
        // an argument error)
        wide_taps = !(hi_t - lo_t <= kTapSpan);
    }
    P.ntaps = ntaps;

    std::vector<int32_t> chans;
    if (tr->chan && tr->n_chan > 0) chans.assign(tr->chan, tr->chan + tr->n_chan);
    else for (int i = 0; i < nsv; i++) chans.push_back(i);
    for (int c : chans) if (c < 0 || c >= nsv) return fail(ctx, GNSS_EARG, "channel index out of range");
    const int nch = (int)chans.size();

    // loop coefficients, calcLoopCoef.m:41-45 (trackingCT.m:26-27)
    auto coef = [](double LBW, double zeta, double k, double& t1, double& t2) {
        double Wn = LBW * 8 * zeta / (4 * (zeta * zeta) + 1);
        t1 = k / (Wn * Wn);
        t2 = 2.0 * zeta / Wn;
    };
    coef(tr->DLLBW, tr->DLLDamp, tr->DLLGain, P.tau1code, P.tau2code);
    coef(tr->PLLBW, tr->PLLDamp, tr->PLLGain, P.tau1carr, P.tau2carr);
    {   // the loop filters' constant quotients (device: loop_update_i); T as the kernel forms it
        // (multicorrelator: (pdi*t)/tau1, :352,361)
        const double T1 = pos ? (pos->mc_pdi ? 1 * sg->ms : sg->ms) : 0.001 * 1;
        const double T10 = pos ? (pos->mc_pdi ? 10 * sg->ms : sg->ms) : 0.001;
        P.dll_r = P.tau2code / P.tau1code;
        P.pll_r = P.tau2carr / P.tau1carr;
        P.dll_t1 = T1 / P.tau1code;
        P.dll_t10 = T10 / P.tau1code;
        P.pll_t1 = T1 / P.tau1carr;
        P.pll_t10 = T10 / P.tau1carr;
    }
    P.Fs = sg->Fs;
    P.codeFreqBasis = sg->codeFreqBasis;
    P.ms = sg->ms;
    P.codelength = sg->codelength;
    P.S = (double)S;
    P.dataBytesPerSample = (double)(file->dataPrecision * file->dataType);
    P.bps = prec * dtyp;
    P.fmt = prec == 2 ? 1 : 0;  // int16 I/Q: staged as is with mean removal; int8 real: as I/Q
    P.inv_Fs = 1.0 / sg->Fs;
    P.exact_div = fast_div_exact(sg->Fs, (int64_t)(S * 10 * 1.02) + 64) ? 0 : 1;
    P.nsv = pos ? 1 : nsv;  // (POS: codedelay sums the channel's own row)
    P.nch = nch;
    P.rec_cap = pos ? pos->ctPOS : N1 + 19 + n10;
    P.cn0_cap = pos ? pos->ctPOS / 20 + 1 : std::max(N1 + 19, n10) / 20 + 1;

    // IF window resident in HBM: from the earliest channel start to the latest
    // possible phase-C end (countinx <= 18, numSample within 1%)
    const int64_t bps = file->dataPrecision * file->dataType;
    int64_t lo = INT64_MAX, hi = 0, hiA = 0;  // hiA: the end of the 1-ms phases' reads
    for (int c : chans) {
        const int64_t cd = acq->codedelay[c];
        lo = std::min(lo, (S - cd + 1 + file->skip * S) * bps);
        if (gv) {  // fseek(S - codedelay - 1 + skip*S) (:57), then one continuous read
            const int64_t a0 = (S - cd - 1 + file->skip * S) * bps;
            lo = std::min(lo, a0);
            hi = std::max(hi, a0 + (int64_t)((double)N1 * S * 1.01 + 4096) * bps);
            continue;
        }
        if (pos) {  // one continuous read: n1 1-ms steps, then 10-ms steps (no re-seek)
            const int64_t n1 = pos_n1(c);
            const double ns = (double)n1 * S + (double)(pos->ctPOS - n1) * 10.0 * S;
            hi = std::max(hi, (S - cd + 1 + file->skip * S) * bps + (int64_t)(ns * 1.01 + 4096) * bps);
            continue;
        }
        const int64_t c0 = (S - cd + 1 + (file->skip + N1 + 18) * S) * bps;
        const int64_t a1 = (S - cd + 1 + file->skip * S) * bps + (int64_t)((N1 + 18) * S * 1.01 + 64) * bps;
        hi = std::max(hi, std::max(c0 + (int64_t)(n10 * 10 * S * 1.01 + 4096) * bps, a1));
        hiA = std::max(hiA, a1);
    }
    P.file_len = file_length(file);
    if (P.file_len < 0) return fail(ctx, GNSS_EIO, "cannot open IF record");
    IfWindow w;
    lo &= ~(int64_t)31;  // whole 8-sample groups of any format
    // Streaming (gnss_ctx_set_window): with a window budget below the read range, the 1-ms
    // phases' range is staged first and the 10-ms phase in segments, each staged (through the
    // pinned double buffer) into the same HBM window before its launch
    const bool seg = ctx->window > 0 && !file->dev_data && !pos && !gv && prec == 1 && dtyp == 2 && n10 > 0 &&
                     (uint64_t)(hi - lo) > ctx->window;
    int st;
    if (seg) {
        if ((uint64_t)(hiA - lo) > ctx->window || ctx->window < (uint64_t)(12 * S * bps * 1.01 + 8192))
            return fail(ctx, GNSS_EARG, "window budget below the 1-ms phases' span");
        HIP_TRY(w.own.alloc(ctx->window + 64));
        w.ptr = w.own.as<int8_t>();
        w.base = lo;
        w.len = std::min<int64_t>(hiA, P.file_len) - lo;
        if ((st = stage_into(ctx, file, w.base, w.base + w.len, w.own.as<int8_t>()))) return st;
    } else if ((st = stage_window(ctx, file, lo, hi, w))) {
        return st;
    }
    const int8_t* iq_dev = w.ptr;
    P.buf_base = w.base;
    P.buf_len = w.len;
    // formats (ifmt.hip): the correlator reads int8 I/Q pairs (fmt 0) or int16 I/Q pairs
    // (fmt 1); staged byte of sample k = 2k / 4k
    DevBuf d_conv, d_pref, d_pscr;
    {
        const int64_t s0 = std::max<int64_t>(lo, w.base);             // file bytes
        const int64_t s1 = std::min<int64_t>(hi, w.base + w.len);
        const int8_t* src = w.ptr + (s0 - w.base);
        if (prec == 1 && dtyp == 1) {  // samples = bytes; staged as (x, 0) pairs
            const int64_t n = std::max<int64_t>(s1 - s0, 0);
            HIP_TRY(d_conv.alloc(ctx, "trk.d_conv", (size_t)(2 * n + 64)));
            HIP_TRY(launch_real8_to_iq8(src, n, d_conv.as<int8_t>(), ctx->stream));
            iq_dev = d_conv.as<int8_t>();
            P.buf_base = 2 * s0;
            P.buf_len = 2 * n;
        } else if (prec == 2) {  // int16 I/Q: the file bytes, plus group prefix sums
            iq_dev = src;
            P.buf_base = s0;
            P.buf_len = std::max<int64_t>(s1 - s0, 0);
            const int64_t ng = P.buf_len / 32;
            HIP_TRY(d_pref.alloc(ctx, "trk.d_pref", 2 * sizeof(long long) * (size_t)(ng + 1)));
            const size_t scr = prefix16_scratch_bytes(ng);
            HIP_TRY(d_pscr.alloc(ctx, "trk.d_pscr", scr));
            long long* pi = d_pref.as<long long>();
            HIP_TRY(launch_prefix16(reinterpret_cast<const short*>(src), ng, pi, pi + ng + 1, d_pscr.p, scr,
                                    ctx->stream));
            P.pref_i = pi;
            P.pref_q = pi + ng + 1;
            P.stage16 = reinterpret_cast<const short*>(iq_dev - P.buf_base);
        }
    }

    // geometry (track_geom.h): the lane spans of the 1-ms and 10-ms steps, for code rates up to
    // the nominal one with 10 % for the DLL's excursions
    const double cps_max = 1.1 * sg->codeFreqBasis / sg->Fs;
    const geom::LaneRule lane{cps_max, P.fmt, ntaps, P.exact_div != 0};
    // probe hooks: the 1-ms / the 10-ms lane span alone
    const char *fs1 = probe_env("GNSS_FORCE_SUB1"), *fs10 = probe_env("GNSS_FORCE_SUB10");
    const int force_sub = (int)ctx->opt[GNSS_OPT_FORCE_SUB];
    const int sub1 = geom::sub_override(lane, geom::sub_for(lane, 1), fs1 ? atoi(fs1) : 0, force_sub);
    const int sub10 = geom::sub_override(lane, geom::sub_for(lane, 10), fs10 ? atoi(fs10) : 0, force_sub);
    const int bpc1 = geom::bpc_for(S, 1, sub1), bpc10 = geom::bpc_for(S, 10, sub10);
    // Persistent step loop (track_run_kernel) when every block of its grid can be
    // resident: one launch per phase run. Residency from the occupancy query; the kernel's
    // own census confirms it (the query can over-report, guide section 1) and a launch
    // that finds a block missing changes nothing and is re-run one launch per step, as is
    // everything with GNSS_NO_PERSIST. Both paths give the same bits.
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    // Virtual blocks per resident block (vpb): where nch x bpc blocks cannot all be
    // resident (config 5: 32 channels x 11 taps), each block correlates vpb of the step's
    // blocks in turn -- the lane geometry and so the bits stay those of bpc blocks.
    // GNSS_OPT_FORCE_VPB (test hook) asks for at least that many.
    P.cps_max = cps_max;
    // <= 3 taps: tap prefixes from the capture register wherever a lane holds at most
    // kRegCapMax distinct boundary samples (lane_boundaries), else through the LDS slots
    P.regcap = regcap_mask(P, cps_max, ctx->opt[GNSS_OPT_SLOT_PATH]);
    auto vpb_for = [&](int bpc, int sub) {
        const bool no_persist = ctx->opt[GNSS_OPT_NO_PERSIST] || P.fmt != 0 || wide_taps ||
                                bpc > run_bpc_cap(P.ntaps);
        return geom::vpb_for(no_persist, nch, bpc, cus, ctx->opt[GNSS_OPT_FORCE_VPB],
                             [&] { return track_run_blocks_per_cu(P, sub, false); },
                             [&] { return track_run_blocks_per_cu(P, sub, true); });
    };
    const int vpb1 = vpb_for(bpc1, sub1), vpb10 = vpb_for(bpc10, sub10);
    bool persist1 = vpb1 > 0, persist10 = vpb10 > 0;
    if (const char* pr = probe_env("GNSS_PROBE")) P.probe = atoi(pr);
    ctx->lane_path = lane_regcap(P, sub1) && lane_regcap(P, sub10);
    if (bpc10 > kMaxBpc) return fail(ctx, GNSS_EARG, "Sample too large for the step geometry");

    // device state
    std::vector<TrkChan> ch0((size_t)nch);
    std::vector<unsigned> cab((size_t)nch * 32);
    for (int i = 0; i < nch; i++) {
        const int c = chans[i];
        TrkChan& t = ch0[i];
        memset(&t, 0, sizeof(t));
        t.codeFreq = sg->codeFreqBasis;  // trackingCT.m:56-58
        t.carrierFreqBasis = acq->fineFreq[c];
        t.carrierFreq = acq->fineFreq[c];
        t.codedelay0 = acq->codedelay[c];
        t.pos = (S - acq->codedelay[c] + 1 + file->skip * S) * bps;  // :63
        t.snrIndex = 1;
        t.sv1 = c + 1;
        t.prn = acq->sv[c];
        t.n1_target = N1;
        if (pos) {  // trackingCT_POS_updated.m:108-110,290 (file_ptr; codedelay base S - cd + 1)
            t.pos = (int64_t)(((double)S - acq->codedelay[c] + 1 + (double)file->skip * sg->Fs * sg->ms) * bps);
            t.codedelay0 = S - acq->codedelay[c] + 1;
            t.sv1 = 1;
            t.n1_target = pos_n1(c);
            t.countinx = pos->countinx ? pos->countinx[c] : 0;
        }
        if (gv) t.pos = (S - acq->codedelay[c] - 1 + file->skip * S) * bps;  // :57 (Codedelay = cd, :55)
        if (acq->sv[c] < 1 || acq->sv[c] > 51) return fail(ctx, GNSS_EARG, "bad PRN");
        ca_bits(acq->sv[c], &cab[(size_t)i * 32]);
    }
    DevBuf d_chan, d_snap, d_desc, d_ca, d_part, d_arrive, d_rec, d_taps, d_cn1, d_cn10, d_dv, d_pi;
    HIP_TRY(d_chan.alloc(ctx, "trk.d_chan", sizeof(TrkChan) * nch));
    HIP_TRY(d_snap.alloc(ctx, "trk.d_snap", sizeof(TrkChan) * nch));
    HIP_TRY(d_desc.alloc(ctx, "trk.d_desc", sizeof(StepDesc) * nch));
    HIP_TRY(d_ca.alloc(ctx, "trk.d_ca", sizeof(unsigned) * cab.size()));
    HIP_TRY(d_part.alloc(ctx, "trk.d_part", sizeof(double) * (size_t)nch * kMaxBpc * 2 * ntaps));
    const size_t arrive_bytes = sizeof(unsigned) * kArrivePerChan * kArriveStride * nch;
    HIP_TRY(d_arrive.alloc(ctx, "trk.d_arrive", arrive_bytes));
    HIP_TRY(d_rec.alloc(ctx, "trk.d_rec", sizeof(double) * (size_t)nch * P.rec_cap * GNSS_NFIELDS));
    if (out->taps) HIP_TRY(d_taps.alloc(ctx, "trk.d_taps", sizeof(double) * (size_t)nch * P.rec_cap * 2 * ntaps));
    HIP_TRY(d_cn1.alloc(ctx, "trk.d_cn1", sizeof(double) * (size_t)nch * P.cn0_cap));
    HIP_TRY(d_cn10.alloc(ctx, "trk.d_cn10", sizeof(double) * (size_t)nch * P.cn0_cap));
    HIP_TRY(d_dv.alloc(ctx, "trk.d_dv", sizeof(int64_t) * (size_t)nch * (P.rec_cap + 1)));
    HIP_TRY(d_pi.alloc(ctx, "trk.d_pi", sizeof(double) * (size_t)nch * N1));
    HIP_TRY(hipMemcpyAsync(d_chan.p, ch0.data(), sizeof(TrkChan) * nch, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_ca.p, cab.data(), sizeof(unsigned) * cab.size(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(d_arrive.p, 0, arrive_bytes, ctx->stream));
    HIP_TRY(hipMemsetAsync(d_cn1.p, 0, d_cn1.n, ctx->stream));
    HIP_TRY(hipMemsetAsync(d_cn10.p, 0, d_cn10.n, ctx->stream));
    HIP_TRY(hipMemsetAsync(d_dv.p, 0, d_dv.n, ctx->stream));
    HIP_TRY(hipMemsetAsync(d_rec.p, 0, d_rec.n, ctx->stream));

    TrkBuffers B{};
    B.iq = iq_dev;
    B.chan = d_chan.as<TrkChan>();
    B.snap = d_snap.as<TrkChan>();
    B.desc = d_desc.as<StepDesc>();
    B.ca_bits = d_ca.as<unsigned>();
    B.partial = d_part.as<double>();
    B.arrive = d_arrive.as<unsigned>();
    B.rec = d_rec.as<double>();
    B.taps_rec = out->taps ? d_taps.as<double>() : nullptr;
    B.cn0_1 = d_cn1.as<double>();
    B.cn0_10 = d_cn10.as<double>();
    B.dvpre = d_dv.as<int64_t>();
    B.p_i_1ms = d_pi.as<double>();
    B.n1 = N1;

    DevBuf d_stamps;  // timing probe: per-launch wall-clock stamps of channel 0
    const char* stamp_path = probe_env("GNSS_STAMPS");
    if (stamp_path) {
        HIP_TRY(d_stamps.alloc(ctx, "trk.d_stamps", sizeof(unsigned long long) * ((size_t)kStampSlots * (8 + 3 * kMaxBpc) + 1)));
        HIP_TRY(hipMemsetAsync(d_stamps.p, 0, d_stamps.n, ctx->stream));
        B.stamps = d_stamps.as<unsigned long long>();
    }

    DevBuf d_pgran, d_err;
    if (persist1 || persist10) {
        HIP_TRY(d_pgran.alloc(ctx, "trk.d_pgran", sizeof(unsigned long long) * 2 * (size_t)nch * gran_per_chan(ntaps)));
        HIP_TRY(d_err.alloc(ctx, "trk.d_err", 16));
        HIP_TRY(hipMemsetAsync(d_pgran.p, 0, d_pgran.n, ctx->stream));
        HIP_TRY(hipMemsetAsync(d_err.p, 0, 16, ctx->stream));
        B.pgran = d_pgran.as<unsigned long long>();
        B.run_err = d_err.as<unsigned>();
    }
    unsigned tag = 0;  // hand-off tags grow across the launches of this call

    DevBuf d_args;  // the kernels' TrkParams / TrkBuffers
    HIP_TRY(d_args.alloc(ctx, "trk.d_args", sizeof(TrkParams) + sizeof(TrkBuffers)));
    HIP_TRY(hipMemcpyAsync(d_args.p, &P, sizeof(TrkParams), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(static_cast<char*>(d_args.p) + sizeof(TrkParams), &B, sizeof(TrkBuffers),
                           hipMemcpyHostToDevice, ctx->stream));
    const TrkDev TD{d_args.as<TrkParams>(),
                    reinterpret_cast<const TrkBuffers*>(static_cast<char*>(d_args.p) + sizeof(TrkParams))};


    // step launches: one persistent launch per phase run, else K-launch graphs replayed
    // (no host launch cost per step); in profiling mode every launch is bracketed by events.
    std::vector<hipEvent_t> pev;
    std::vector<char> pev10;  // launch of the 10-ms phase
    int64_t launches = 0;
    std::function<int(int, int)> run_steps_ref;
    auto run_steps = [&](int pdi, int count) -> int {
        const int bpc = pdi == 1 ? bpc1 : bpc10, sub = pdi == 1 ? sub1 : sub10;
        if (count <= 0) return GNSS_OK;
        ctx->timing.track_channel_samples += (int64_t)count * nch * (int64_t)S * pdi;
        if (pdi == 1 ? persist1 : persist10) {
            hipEvent_t a = nullptr, b = nullptr;
            if (ctx->profiling) {
                HIP_TRY(hipEventCreate(&a));
                HIP_TRY(hipEventCreate(&b));
                HIP_TRY(hipEventRecord(a, ctx->stream));
            }
            HIP_TRY(hipMemsetAsync(d_err.p, 0, 16, ctx->stream));  // timeout word + census
            HIP_TRY(launch_track_run(P, B, TD, bpc, pdi == 1 ? vpb1 : vpb10, sub, count, tag, ctx->stream));
            tag += (unsigned)count + 1;
            unsigned err[3] = {0, 0, 0};
            HIP_TRY(hipMemcpyAsync(err, d_err.p, sizeof err, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            if (err[0] == 2) {  // census: not every block was resident -> one launch per step
                (pdi == 1 ? persist1 : persist10) = false;
                if (a) (void)hipEventDestroy(a);
                ctx->timing.track_channel_samples -= (int64_t)count * nch * (int64_t)S * pdi;
                return run_steps_ref(pdi, count);
            }
            if (err[0]) return fail(ctx, GNSS_EDEVICE, "persistent tracking kernel: a hand-off wait timed out");
            launches += 1;
            if (ctx->profiling) {
                HIP_TRY(hipEventRecord(b, ctx->stream));
                pev.push_back(a);
                pev.push_back(b);
                pev10.push_back(pdi == 10);
                if (pdi == 10) {
                    ctx->timing.track10_launches += 1;
                    ctx->timing.track10_channel_samples += (int64_t)count * nch * (int64_t)S * pdi;
                }
            }
            return GNSS_OK;
        }
        launches += count;
        if (ctx->profiling) {
            for (int i = 0; i < count; i++) {
                hipEvent_t a, b;
                HIP_TRY(hipEventCreate(&a));
                HIP_TRY(hipEventCreate(&b));
                HIP_TRY(hipEventRecord(a, ctx->stream));
                HIP_TRY(launch_track_step(P, B, TD, bpc, sub, ctx->stream));
                HIP_TRY(hipEventRecord(b, ctx->stream));
                pev.push_back(a);
                pev.push_back(b);
                pev10.push_back(pdi == 10);
            }
            if (pdi == 10) {
                ctx->timing.track10_launches += count;
                ctx->timing.track10_channel_samples += (int64_t)count * nch * (int64_t)S * pdi;
            }
            return GNSS_OK;
        }
        const int K = 50;
        if (count >= K) {
            StepGraph g;
            HIP_TRY(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
            for (int i = 0; i < K; i++) {
                hipError_t e = launch_track_step(P, B, TD, bpc, sub, ctx->stream);
                if (e != hipSuccess) {
                    hipGraph_t junk;
                    (void)hipStreamEndCapture(ctx->stream, &junk);
                    if (junk) (void)hipGraphDestroy(junk);
                    return fail(ctx, GNSS_EDEVICE, "capture: %s", hipGetErrorString(e));
                }
            }
            HIP_TRY(hipStreamEndCapture(ctx->stream, &g.graph));
            HIP_TRY(hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0));
            for (int r = 0; r < count / K; r++) HIP_TRY(hipGraphLaunch(g.exec, ctx->stream));
            for (int i = 0; i < count % K; i++) HIP_TRY(launch_track_step(P, B, TD, bpc, sub, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));  // graph objects die with this scope
        } else {
            for (int i = 0; i < count; i++) HIP_TRY(launch_track_step(P, B, TD, bpc, sub, ctx->stream));
        }
        return GNSS_OK;
    };
    run_steps_ref = run_steps;

    Events e_all;
    if (hp.on) HIP_TRY(hipStreamSynchronize(ctx->stream));
    hp.mark("setup");
    HIP_TRY(hipEventRecord(e_all.a, ctx->stream));
    std::vector<TrkChan> chh((size_t)nch);
    if (gv) {
        // trackingCT_multiCorr-GIVEN.m:52-314: datalength 1-ms steps, no bit-edge search, no
        // 10-ms phase
        HIP_TRY(launch_track_prepare(P, B, TD, 1, 0, ctx->stream));
        if ((st = run_steps(1, N1))) return st;
    } else if (pos) {
        // trackingCT_POS_updated.m:179-413: every channel continues from its own state and
        // file pointer; 1-ms steps while msIndex <= 1000 + countinx(svIndex), then 10 ms
        int64_t n1max = 0, n1min = INT64_MAX;
        for (int c : chans) { n1max = std::max(n1max, pos_n1(c)); n1min = std::min(n1min, pos_n1(c)); }
        HIP_TRY(launch_track_prepare(P, B, TD, 1, 0, ctx->stream));
        if ((st = run_steps(1, (int)n1max))) return st;
        if (n1min < pos->ctPOS) {
            HIP_TRY(hipMemcpyAsync(chh.data(), d_chan.p, sizeof(TrkChan) * nch, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            for (auto& t : chh) t.n1_target = pos->ctPOS;  // (Index + 1 per step: the last step)
            HIP_TRY(hipMemcpyAsync(d_chan.p, chh.data(), sizeof(TrkChan) * nch, hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(launch_track_prepare(P, B, TD, 10, 0, ctx->stream));
            if ((st = run_steps(10, (int)(pos->ctPOS - n1min)))) return st;
        }
    } else {
        // phase A: steps 1..N1-1, snapshot (for countinx = -1), step N1, bit-edge search
        HIP_TRY(launch_track_prepare(P, B, TD, 1, 0, ctx->stream));
        if ((st = run_steps(1, N1 - 1))) return st;
        HIP_TRY(launch_track_snapshot(P, B, TD, ctx->stream));
        if ((st = run_steps(1, 1))) return st;
        HIP_TRY(launch_track_bitedge(P, B, TD, ctx->stream));
        HIP_TRY(hipMemcpyAsync(chh.data(), d_chan.p, sizeof(TrkChan) * nch, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        int cxmax = 0;
        for (auto& t : chh) cxmax = std::max(cxmax, t.countinx);
        if (hp.on)
            for (auto& t : chh)
                fprintf(stderr, "hostprof bitedge prn %d status %d countinx %d n1_target %lld\n", t.prn, t.status,
                        t.countinx, (long long)t.n1_target);
        // phase B continues phase A up to 1000 + countinx (inactive channels skip)
        if ((st = run_steps(1, cxmax))) return st;
        HIP_TRY(launch_track_phase_c_init(P, B, TD, file->skip, ctx->stream));
        // phase C
        if (!seg) {
            if ((st = run_steps(10, n10))) return st;
        } else {
            // segments: from the channels' file positions, as many 10-ms steps as the window
            // holds (numSample <= 10*S*1.01 + 64 per step, the kernels' own bound), staged
            // into the window before their launch (the stream orders the previous launch's
            // reads before the new bytes land)
            const int64_t per_step = (int64_t)(10 * S * 1.01 + 64) * bps;
            for (int done = 0; done < n10;) {
                HIP_TRY(hipMemcpyAsync(chh.data(), d_chan.p, sizeof(TrkChan) * nch, hipMemcpyDeviceToHost,
                                       ctx->stream));
                HIP_TRY(hipStreamSynchronize(ctx->stream));
                int64_t pmin = INT64_MAX, pmax = 0;
                for (auto& t : chh) {
                    if (t.status != GNSS_OK) continue;
                    pmin = std::min(pmin, t.pos);
                    pmax = std::max(pmax, t.pos);
                }
                if (pmin == INT64_MAX) break;  // no channel left
                const int64_t base = (pmin & ~(int64_t)31);
                const int64_t room = (int64_t)ctx->window - (pmax - base) - 4096;
                int k = (int)std::min<int64_t>(n10 - done, room / per_step);
                if (k < 1) return fail(ctx, GNSS_EARG, "window budget below one 10-ms step of every channel");
                const int64_t end = std::min<int64_t>(P.file_len, pmax + (int64_t)k * per_step + 4096);
                if ((st = stage_into(ctx, file, base, end, w.own.as<int8_t>()))) return st;
                P.buf_base = base;
                P.buf_len = end - base;
                B.iq = w.own.as<int8_t>();
                HIP_TRY(hipMemcpyAsync(d_args.p, &P, sizeof(TrkParams), hipMemcpyHostToDevice, ctx->stream));
                HIP_TRY(hipMemcpyAsync(static_cast<char*>(d_args.p) + sizeof(TrkParams), &B, sizeof(TrkBuffers),
                                       hipMemcpyHostToDevice, ctx->stream));
                // the pending descriptors were checked against the previous window: rebuild
                // them from the channels' state (the same fields, the new staging check)
                HIP_TRY(launch_track_prepare(P, B, TD, 10, 1, ctx->stream));
                if ((st = run_steps(10, k))) return st;
                done += k;
                ctx->timing.track_segments += 1;
            }
        }
    }
    HIP_TRY(hipEventRecord(e_all.b, ctx->stream));
    HIP_TRY(hipEventSynchronize(e_all.b));
    ctx->timing.track_ms = e_all.ms();

    ctx->timing.track_launches = launches;
    double ksum = 0, ksum10 = 0;
    for (size_t i = 0; i + 1 < pev.size(); i += 2) {
        float f = 0;
        (void)hipEventElapsedTime(&f, pev[i], pev[i + 1]);
        ksum += f;
        if (pev10[i / 2]) ksum10 += f;
    }
    ctx->timing.track10_kernel_ms = ksum10;
    for (auto e : pev) (void)hipEventDestroy(e);
    ctx->timing.track_kernel_ms = ksum;
    if (stamp_path && (st = write_stamps(ctx, stamp_path, d_stamps))) return st;

    // results
    hp.mark("kernels done");
    HIP_TRY(hipMemcpyAsync(chh.data(), d_chan.p, sizeof(TrkChan) * nch, hipMemcpyDeviceToHost, ctx->stream));
    const size_t nrec = (size_t)nch * P.rec_cap * GNSS_NFIELDS;
    const size_t ntp = out->taps ? (size_t)nch * P.rec_cap * 2 * ntaps : 0;
    double* rec = odev ? nullptr : pinned_buffer<double>(ctx, "trk.h_rec", nrec);
    double* tp = ntp && !odev ? pinned_buffer<double>(ctx, "trk.h_taps", ntp) : nullptr;
    if (!odev && (!rec || (ntp && !tp))) return fail(ctx, GNSS_EDEVICE, "hipHostMalloc of the record staging failed");
    std::vector<double> cn1((size_t)nch * P.cn0_cap), cn10((size_t)nch * P.cn0_cap);
    if (!odev) {
        HIP_TRY(hipMemcpyAsync(rec, d_rec.p, nrec * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (out->taps) HIP_TRY(hipMemcpyAsync(tp, d_taps.p, ntp * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipMemcpyAsync(cn1.data(), d_cn1.p, cn1.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(cn10.data(), d_cn10.p, cn10.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));

    hp.mark("d2h done");
    int status = GNSS_OK;
    for (int i = 0; i < nch; i++) {
        const TrkChan& t = chh[i];
        if (t.status && ctx->fail_chan < 0) ctx->fail_chan = chans[i];  // (the first failing channel)
        if (t.status && (status == GNSS_OK || t.status == GNSS_ENODATA)) status = t.status;
    }
    if (status != GNSS_OK) {
        if (out->len) for (int c : chans) out->len[c] = 0;
        return fail(ctx, status, status == GNSS_ENODATA ? "Not enough raw data" : "tracking failed: %s",
                    gnss_strerror(status));
    }

    int rows = pos ? pos->ctPOS / 20 : N1 / 20;
    // series length before the 10-ms values (POS: every step has its own row)
    std::vector<int64_t> n1s((size_t)nch);
    for (int i = 0; i < nch; i++) {
        const int c = chans[i];
        const int64_t n1 = pos ? (int64_t)pos->ctPOS : (int64_t)N1 + chh[i].countinx;
        n1s[i] = n1;
        if (out->len) out->len[c] = n1 + 10LL * n10;
        if (out->countinx) out->countinx[c] = chh[i].countinx;
        rows = std::max(rows, (int)(n1 / 20));
    }
    if ((st = expand_records(ctx, out, chans, n1s, n10, ntaps, P.rec_cap, rec, tp, d_rec, d_taps, dev_slot))) return st;
    hp.mark("expanded");
    if (gv && out->rec) given_codedelay(out, acq, nsv, N1);
    rows = std::max(rows, n10 / 20);
    out->cn0_rows = rows;  // (POS: CN0_CT, one row per 20 steps of either pdi)
    if (out->CN0_Eph) {
        std::vector<int> r1((size_t)nch);
        for (int i = 0; i < nch; i++) r1[i] = pos ? rows : std::max(N1, N1 + chh[i].countinx) / 20;
        copy_cn0(out, chans, nsv, r1, n10 / 20, cn1, cn10, P.cn0_cap);
    }
    return GNSS_OK;
}

extern "C" {

int gnss_tracking_ct(gnss_ctx* ctx, const gnss_file* file, const gnss_signal* sg, const gnss_track* tr,
                     const gnss_acquired* acq, gnss_track_out* out)
{
    if (ctx && !ctx->members.empty()) return group_tracking(ctx, file, sg, tr, acq, out, nullptr);
    return tracking_impl(ctx, file, sg, tr, acq, out, nullptr);
}

int gnss_tracking_ct_pos(gnss_ctx* ctx, const gnss_file* file, const gnss_signal* sg, const gnss_track* tr,
                         const gnss_acquired* acq, int32_t ctPOS, const int32_t* countinx, gnss_track_out* out)
{
    const PosCfg pc{ctPOS, countinx, 0};
    if (ctx && !ctx->members.empty()) return group_tracking(ctx, file, sg, tr, acq, out, &pc);
    return tracking_impl(ctx, file, sg, tr, acq, out, &pc);
}

int gnss_tracking_ct_multicorr(gnss_ctx* ctx, const gnss_file* file, const gnss_signal* sg,
                               const gnss_track* tr, const gnss_acquired* acq, int32_t datalength,
                               gnss_track_out* out)
{
    const GivenCfg g{datalength};
    return tracking_impl(ctx, file, sg, tr, acq, out, nullptr, &g);
}

int gnss_tracking_ct_mc(gnss_ctx* ctx, const gnss_file* file, const gnss_signal* sg, const gnss_track* tr,
                        const gnss_acquired* acq, int32_t msPosCT, int32_t pdi, gnss_track_out* out)
{
    if (!ctx) return GNSS_EARG;
    if (pdi != 1 && pdi != 10) return fail(ctx, GNSS_EARG, "multicorrelator: pdi must be 1 or 10");
    if (msPosCT < pdi) return fail(ctx, GNSS_EARG, "multicorrelator: msPosCT/pdi must be >= 1");
    const PosCfg pc{msPosCT / pdi, nullptr, pdi};  // msIndex = 1:datalength/pdi (:170)
    if (!ctx->members.empty()) return group_tracking(ctx, file, sg, tr, acq, out, &pc);
    return tracking_impl(ctx, file, sg, tr, acq, out, &pc);
}

int gnss_lane_boundaries(const double* taps, const double* post, int n_taps, int lane_samples, double cps_max)
{
    if (!taps || n_taps < 1 || n_taps > GNSS_MAX_TAPS || lane_samples < 1 || !(cps_max > 0.0)) return -1;
    return lane_boundaries(taps, post, n_taps, lane_samples, cps_max);
}

int gnss_ctx_lane_path(const gnss_ctx* ctx) { return ctx ? ctx->lane_path : 0; }

int gnss_correlate_step(gnss_ctx* ctx, const gnss_file* file, const gnss_signal* sg, int prn, int pdi,
                        double remChip, double codeFreq, double carrierFreq, double remPhase,
                        int64_t pos_bytes, int n_taps, const double* taps, double* sums_out,
                        int64_t* numSample_out)
{
    if (!ctx || !file || !sg || !taps || !sums_out || (n_taps != 3 && n_taps != 11) || prn < 1 || prn > 51)
        return GNSS_EARG;
    if (pdi != 1 && pdi != 10) return GNSS_EARG;
    if (!lane_rate_admitted(sg, codeFreq)) return refuse_lane_rate(ctx, sg, codeFreq);
    HIP_TRY(hipSetDevice(ctx->device));
    const int64_t S = sg->Sample;
    TrkParams P{};
    P.Fs = sg->Fs;
    P.codeFreqBasis = sg->codeFreqBasis;
    P.ms = sg->ms;
    P.codelength = sg->codelength;
    P.S = (double)S;
    P.dataBytesPerSample = 2;
    P.bps = 2;  // int8 I/Q records only
    P.fmt = 0;
    P.inv_Fs = 1.0 / sg->Fs;
    P.exact_div = fast_div_exact(sg->Fs, (int64_t)(S * 10 * 1.02) + 64) ? 0 : 1;
    P.ntaps = n_taps;
    P.iE = 0; P.iP = n_taps / 2; P.iL = n_taps - 1;
    for (int s = 0; s < n_taps; s++) P.taps[s] = taps[s];
    P.nsv = P.nch = 1;
    P.rec_cap = 1;
    P.cn0_cap = 1;
    P.file_len = file_length(file);
    IfWindow w;
    int st = stage_window(ctx, file, pos_bytes, pos_bytes + (int64_t)(2.1 * S * pdi) + 64, w);
    if (st) return st;
    P.buf_base = w.base;
    P.buf_len = w.len;
    TrkChan c{};
    c.remChip = remChip;
    c.codeFreq = codeFreq;
    c.carrierFreq = carrierFreq;
    c.remPhase = remPhase;
    c.pos = pos_bytes;
    c.n1_target = 1 << 30;
    c.sv1 = 1;
    c.prn = prn;
    unsigned cab[32];
    ca_bits(prn, cab);
    // one step at the caller's code rate: 8-sample lanes unless the test hook asks for more
    const geom::LaneRule lane{codeFreq / sg->Fs, P.fmt, n_taps, P.exact_div != 0};
    const int sub = geom::sub_override(lane, 1, 0, (int)ctx->opt[GNSS_OPT_FORCE_SUB]);
    P.regcap = regcap_mask(P, codeFreq / sg->Fs, ctx->opt[GNSS_OPT_SLOT_PATH]);
    ctx->lane_path = lane_regcap(P, sub);
    const int bpc = geom::bpc_for(S, pdi, sub);
    DevBuf d_chan, d_desc, d_ca, d_part, d_arrive, d_sums;
    HIP_TRY(d_chan.alloc(sizeof(TrkChan)));
    HIP_TRY(d_desc.alloc(sizeof(StepDesc)));
    HIP_TRY(d_ca.alloc(sizeof(cab)));
    HIP_TRY(d_part.alloc(sizeof(double) * kMaxBpc * 2 * n_taps));
    HIP_TRY(d_arrive.alloc(sizeof(unsigned) * kArrivePerChan * kArriveStride));
    HIP_TRY(d_sums.alloc(sizeof(double) * 2 * n_taps));
    HIP_TRY(hipMemcpyAsync(d_chan.p, &c, sizeof c, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_ca.p, cab, sizeof cab, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(d_arrive.p, 0, sizeof(unsigned) * kArrivePerChan * kArriveStride, ctx->stream));
    TrkBuffers B{};
    B.iq = w.ptr;
    B.chan = d_chan.as<TrkChan>();
    B.desc = d_desc.as<StepDesc>();
    B.ca_bits = d_ca.as<unsigned>();
    B.partial = d_part.as<double>();
    B.arrive = d_arrive.as<unsigned>();
    B.dbg_sums = d_sums.as<double>();
    DevBuf d_args;  // the kernels' TrkParams / TrkBuffers
    HIP_TRY(d_args.alloc(sizeof(TrkParams) + sizeof(TrkBuffers)));
    HIP_TRY(hipMemcpyAsync(d_args.p, &P, sizeof(TrkParams), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(static_cast<char*>(d_args.p) + sizeof(TrkParams), &B, sizeof(TrkBuffers),
                           hipMemcpyHostToDevice, ctx->stream));
    const TrkDev TD{d_args.as<TrkParams>(),
                    reinterpret_cast<const TrkBuffers*>(static_cast<char*>(d_args.p) + sizeof(TrkParams))};

    HIP_TRY(launch_track_prepare(P, B, TD, pdi, 0, ctx->stream));
    HIP_TRY(launch_track_step(P, B, TD, bpc, sub, ctx->stream));
    HIP_TRY(hipMemcpyAsync(sums_out, d_sums.p, sizeof(double) * 2 * n_taps, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(&c, d_chan.p, sizeof c, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (c.status) return fail(ctx, c.status, "correlate step failed");
    if (numSample_out) {
        const double cps = codeFreq / sg->Fs;
        *numSample_out = (int64_t)round((sg->codelength * pdi - remChip) / cps);
    }
    return GNSS_OK;
}

}  // extern "C"
