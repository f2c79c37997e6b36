// api_acq.cpp -- acquisition.m on the host side of the C-ABI: read block -> PRN search ->
// threshold -> fine frequency. Drives the kernels in acq.hip / acq_fft.hip (or batched rocFFT).
#include <cmath>
#include <cstring>
#include <vector>

#include "host.h"

using namespace gnss;
using namespace gnss::host;

namespace {
// The acquisition's split correlator pipelines its batches over two streams by default
// (GNSS_OPT_ACQ_PIPE; config-2 fp64 correlation 10.10-10.18 -> 9.75-9.88 ms on MI355X,
// profiles/r03_ab_acq_pipe.txt).
constexpr int kAcqPipeDefault = 2;
// the paired launch's row blocks sit in the grid's first kAcqPairFront percent (acq_fft.hip)
constexpr int kAcqPairFront = 60;
// SVs per launch of the fine-frequency search (scratch ~186 MB per SV at config 2)
constexpr int kFineBatch = 16;

template <class V> struct CplxReal;
template <> struct CplxReal<float2> { using T = float; };
template <> struct CplxReal<double2> { using T = double; };

// The PRN x bin x ms search of acquisition.m:47-61 into corr[p][bin][.] (sum over the ms of
// |ifft(fft(code) .* conj(fft(signal .* carrier)))|^2), V = float2 (fast mode) or double2
// (the reference's precision): the own P x 2000 FFT correlator (acq_fft.hip) where S = P * 2000,
// batched rocFFT otherwise. e_all.a is recorded when the timed work starts; *perm = P for
// the own correlator's tau2-major surface, 0 for natural order.
template <class V>
int acq_search(gnss_ctx* ctx, const int8_t* blk, const double2* xa, int64_t S, int dl, int nb, int np,
               const gnss_signal* sg, const gnss_acq* acq, const float* ca, typename CplxReal<V>::T* corr,
               Events& e_all, int* perm, DevBuf& fsync)
{
    const int dbl = sizeof(V) == sizeof(double2) ? 1 : 0;
    const size_t csz = sizeof(V);
    const int nsig = dl * nb;
    int st = GNSS_OK;
    if (acq_fft_supported(S) && !ctx->opt[GNSS_OPT_ACQ_ROCFFT]) {
        DevBuf d_twr, d_twc, B, X, A;  // (freed after the stream drains)
        const int P = (int)(S / 2000);
        *perm = P;
        // twiddles (fp64 on the host; rounded to fp32 in the fast mode), kept in the
        // context per S and precision
        const bool have_tw = ctx->acq_tw_S == S && ctx->acq_tw_dbl == dbl;
        HIP_TRY(d_twr.alloc(ctx, "acq.d_twr", 2000 * csz));
        HIP_TRY(d_twc.alloc(ctx, "acq.d_twc", (size_t)P * 2000 * csz));
        if (!have_tw) {
            std::vector<V> twr(2000), twc((size_t)P * 2000);
            for (int m = 0; m < 2000; m++) {
                const double a = -2.0 * M_PI * (double)m / 2000.0;
                twr[m].x = std::cos(a);
                twr[m].y = std::sin(a);
            }
            for (int m = 0; m < P; m++)
                for (int k = 0; k < 2000; k++) {
                    const double a = -2.0 * M_PI * (double)((int64_t)m * k % S) / (double)S;
                    twc[(size_t)m * 2000 + k].x = std::cos(a);
                    twc[(size_t)m * 2000 + k].y = std::sin(a);
                }
            HIP_TRY(hipMemcpyAsync(d_twr.p, twr.data(), twr.size() * csz, hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(hipMemcpyAsync(d_twc.p, twc.data(), twc.size() * csz, hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));  // (the host vectors go out of scope)
            ctx->acq_tw_S = S;
            ctx->acq_tw_dbl = dbl;
        }
        const size_t ntr = (size_t)nsig + np;
        HIP_TRY(B.alloc(ctx, "acq.B", csz * ntr * S));
        HIP_TRY(X.alloc(ctx, "acq.X", csz * ntr * S));
        const int npairs = nb * np;
        if (dbl && ctx->opt[GNSS_OPT_ACQ_FUSED]) {
            // fp64: one persistent launch, the intermediate in each XCD's L2 (acq_fft.hip);
            // the caller reads fsync's error word once the stream has drained
            DevBuf ring;
            const int nslot = ctx->opt[GNSS_OPT_ACQ_RING] ? (int)ctx->opt[GNSS_OPT_ACQ_RING] : 3;
            HIP_TRY(ring.alloc(ctx, "acq.ring", acq_fused_ring_bytes(S)));
            HIP_TRY(fsync.alloc(ctx, "acq.fsync", acq_fused_sync_bytes()));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            HIP_TRY(hipEventRecord(e_all.a, ctx->stream));
            HIP_TRY(launch_acq_fft_forward<V>(blk, xa, S, dl, nb, sg->IF, acq->freqMin, acq->freqStep, sg->Fs, ca,
                                              np, sg->codeFreqBasis, d_twr.as<V>(), d_twc.as<V>(), B.as<V>(),
                                              X.as<V>(), ctx->stream));
            const V* C = X.as<V>() + (size_t)nsig * S;
            HIP_TRY(launch_acq_fft_correlate_fused(reinterpret_cast<const double2*>(C), X.as<double2>(), S, dl, nb,
                                                   np, nslot, d_twr.as<double2>(), d_twc.as<double2>(),
                                                   ring.as<double2>(), fsync.p, reinterpret_cast<double*>(corr),
                                                   ctx->stream));
            return GNSS_OK;
        }
        // (bin, PRN) pairs per batch: the inverse intermediate leaves the L2 either way (PMC
        // FETCH / WRITE, which count Infinity-Cache hits too, profiles/acq_traffic_r01.json),
        // and smaller batches measured slower, so batches of ~1 GiB, balanced (no
        // small tail batch that leaves the chip idle): config 2 (fp32) measured 7.94 ms of
        // correlation at 28 pairs per batch (256 MB), 7.09-7.29 at 112, 7.15-7.30 at 232
        // (tools/gpu_acq_batch.sh). Pairs are independent: the bits do not depend on it.
        const int target = (int)std::max<int64_t>(1, ((int64_t)1 << 30) / ((int64_t)dl * S * (int64_t)csz));
        const int nbat = (npairs + target - 1) / target;
        int batch = (npairs + nbat - 1) / nbat;
        // the test hook, clamped before the narrowing (2^32 would become 0)
        if (ctx->opt[GNSS_OPT_ACQ_BATCH] > 0)
            batch = (int)std::min<int64_t>(ctx->opt[GNSS_OPT_ACQ_BATCH], (int64_t)npairs);
        batch = std::max(1, std::min(batch, npairs));
        // Two streams: batch b's row pass (LDS-bound fp64 transforms, reading the intermediate)
        // runs beside batch b+1's column pass (bound by the intermediate's writes), each batch
        // in its own half of a double intermediate; the column pass of b+2 waits for the rows
        // of b. Every pair is in one batch and its corr entries are written by its row pass
        // alone, so the surface is bit-identical to the one-stream order.
        // Paired launches (fp64, = 3): one launch per batch boundary holding batch b's column
        // blocks and batch b-1's row blocks interleaved, so the two passes share every CU.
        const int64_t pipe = ctx->opt[GNSS_OPT_ACQ_PIPE] ? ctx->opt[GNSS_OPT_ACQ_PIPE] : kAcqPipeDefault;
        const bool pair = dbl && pipe == 3 && npairs > batch;
        const bool two = (pipe == 2 || (pipe == 3 && !dbl)) && npairs > batch;
        hipStream_t s_cols = ctx->stream, s_rows = ctx->stream2;
        const size_t abuf = (size_t)batch * dl * S;
        HIP_TRY(A.alloc(ctx, "acq.A", csz * abuf * (two || pair ? 2 : 1)));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        HIP_TRY(hipEventRecord(e_all.a, ctx->stream));
        // the forward spectra: all at once, or (the two-stream pipeline) the
        // codes and the bins batch 0 reads first and each later batch's new bins just before its
        // column pass, on the column stream, where they run beside the previous batch's row pass
        // (the column stream waits on the rows anyway); every spectrum is the same transform of the
        // same data, so the bits do not change (profiles/r05_ab_fwd_split.txt)
        const bool fwd_split = two;
        auto fwd = [&](int bin0, int nbc, bool codes) {
            return launch_acq_fft_forward<V>(blk, xa, S, dl, nb, sg->IF, acq->freqMin, acq->freqStep, sg->Fs, ca, np,
                                             sg->codeFreqBasis, d_twr.as<V>(), d_twc.as<V>(), B.as<V>(), X.as<V>(),
                                             ctx->stream, bin0, nbc, codes);
        };
        int fwd_bins = 0;  // bins [0, fwd_bins) transformed so far
        if (fwd_split) {
            const int need = std::min(nb, (std::min(batch, npairs) - 1) / np + 1);
            HIP_TRY(fwd(0, need, true));
            fwd_bins = need;
        } else {
            HIP_TRY(fwd(0, -1, true));
            fwd_bins = nb;
        }
        const V* C = X.as<V>() + (size_t)nsig * S;
        if (pair) {
            const int nbt = (npairs + batch - 1) / batch;
            double2* Ah[2] = {reinterpret_cast<double2*>(A.p), reinterpret_cast<double2*>(A.p) + abuf};
            for (int b = 0; b <= nbt; b++) {
                const int cq = b * batch, rq = (b - 1) * batch;
                const int nc = b < nbt ? std::min(batch, npairs - cq) : 0;
                const int nr = b > 0 ? std::min(batch, npairs - rq) : 0;
                HIP_TRY(launch_acq_fft_pair(reinterpret_cast<const double2*>(C), X.as<double2>(), S, dl, nb, np, cq,
                                            nc, Ah[b & 1], rq, nr, Ah[(b + 1) & 1], d_twr.as<double2>(),
                                            d_twc.as<double2>(), reinterpret_cast<double*>(corr), kAcqPairFront,
                                            ctx->stream));
            }
            return GNSS_OK;
        }
        if (!two) {
            for (int q0 = 0; q0 < npairs; q0 += batch) {
                const int nq = std::min(batch, npairs - q0);
                HIP_TRY(launch_acq_fft_correlate(C, X.as<V>(), S, dl, nb, np, q0, nq, d_twr.as<V>(),
                                                 d_twc.as<V>(), A.as<V>(), corr, ctx->stream));
            }
            return GNSS_OK;
        }
        // A launch error part way leaves row passes queued on stream2 that still write acq.A /
        // corr: drain it before the error returns, so the next call's pooled buffers are free.
        auto pipelined = [&]() -> int {
            int last = 0;
            for (int q0 = 0, b = 0; q0 < npairs; q0 += batch, b++) {
                const int nq = std::min(batch, npairs - q0);
                const int h = b & 1;
                V* Ah = A.as<V>() + (size_t)h * abuf;
                if (fwd_split) {  // this batch's bins not transformed yet (pairs q0 .. q0 + nq - 1)
                    const int need = std::min(nb, (q0 + nq - 1) / np + 1);
                    if (need > fwd_bins) HIP_TRY(fwd(fwd_bins, need - fwd_bins, false));
                    fwd_bins = std::max(fwd_bins, need);
                }
                if (b >= 2) HIP_TRY(hipStreamWaitEvent(s_cols, ctx->ev_rows[h], 0));  // rows of b-2 read Ah
                HIP_TRY(launch_acq_fft_correlate(C, X.as<V>(), S, dl, nb, np, q0, nq, d_twr.as<V>(), d_twc.as<V>(),
                                                 Ah, corr, s_cols, kAcqCols));
                HIP_TRY(hipEventRecord(ctx->ev_cols[h], s_cols));
                HIP_TRY(hipStreamWaitEvent(s_rows, ctx->ev_cols[h], 0));
                HIP_TRY(launch_acq_fft_correlate(C, X.as<V>(), S, dl, nb, np, q0, nq, d_twr.as<V>(), d_twc.as<V>(),
                                                 Ah, corr, s_rows, kAcqRows));
                HIP_TRY(hipEventRecord(ctx->ev_rows[h], s_rows));
                last = h;
            }
            // the caller's stream owns the result again (stream2 is in order: its last event covers all)
            HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_rows[last], 0));
            return GNSS_OK;
        };
        const int pst = pipelined();
        if (pst != GNSS_OK) (void)hipStreamSynchronize(s_rows);
        return pst;
    }
    // batched rocFFT (sample counts that are not P x 2000)
    *perm = 0;
    DevBuf sig, code, y;
    HIP_TRY(sig.alloc(ctx, "acq.sig", csz * (size_t)nsig * S));
    HIP_TRY(code.alloc(ctx, "acq.code", csz * (size_t)np * S));
    // PRN chunk so the product/IFFT buffer stays <= ~4 GB
    const size_t per_prn = csz * (size_t)nsig * S;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)np, ((size_t)4 << 30) / per_prn));
    HIP_TRY(y.alloc(ctx, "acq.y", per_prn * (size_t)chunk));
    // plans outside the timed region
    rocfft_plan pl;
    if ((st = get_plan(ctx, S, nsig, dbl, 0, &pl))) return st;
    if ((st = get_plan(ctx, S, np, dbl, 0, &pl))) return st;
    for (int p0 = 0; p0 < np; p0 += chunk) {
        const int pc = std::min(chunk, np - p0);
        if ((st = get_plan(ctx, S, (size_t)pc * nsig, dbl, 1, &pl))) return st;
    }
    HIP_TRY(hipEventRecord(e_all.a, ctx->stream));
    HIP_TRY(launch_acq_wipe(blk, xa, S, dl, nb, sg->IF, acq->freqMin, acq->freqStep, sg->Fs, sig.as<V>(), ctx->stream));
    if ((st = run_fft(ctx, sig.p, S, nsig, dbl, 0))) return st;
    HIP_TRY(launch_acq_code(ca, nullptr, np, S, sg->codeFreqBasis, sg->Fs, code.as<V>(), ctx->stream));
    if ((st = run_fft(ctx, code.p, S, np, dbl, 0))) return st;
    for (int p0 = 0; p0 < np; p0 += chunk) {
        const int pc = std::min(chunk, np - p0);
        HIP_TRY(launch_acq_mul(code.as<V>() + (size_t)p0 * S, sig.as<V>(), pc, nsig, S, y.as<V>(), ctx->stream));
        if ((st = run_fft(ctx, y.p, S, (size_t)pc * nsig, dbl, 1))) return st;
        HIP_TRY(launch_acq_power(y.as<V>(), pc, nb, dl, S, 0, corr + (size_t)p0 * nb * S, ctx->stream));
    }
    return GNSS_OK;
}
}  // namespace

// acquisition.m's PRN loop (:47-80) dealt over the members; Acquired / diag merged in list order
static int group_acquisition(gnss_ctx* g, const gnss_file* file, const gnss_signal* sg, const gnss_acq* acq,
                             gnss_acquired* out, gnss_acq_diag* diag)
{
    if (!file || !sg || !acq || !out) return GNSS_EARG;
    memset(out, 0, sizeof(*out));
    if (diag) memset(diag, 0, sizeof(*diag));
    g->timing = gnss_timing{};
    std::vector<int32_t> prns;
    if (acq->n_prn > 0 && acq->prn_list) prns.assign(acq->prn_list, acq->prn_list + acq->n_prn);
    else for (int i = 1; i <= 32; i++) prns.push_back(i);  // acquisition.m:47
    if (prns.size() > GNSS_MAX_SV) return fail(g, GNSS_EARG, "too many PRNs");
    const int M = (int)g->members.size();
    const auto shards = group::deal((int)prns.size(), M);
    std::vector<std::vector<int32_t>> plist((size_t)M);
    for (int k = 0; k < M; k++)
        for (int i : shards[(size_t)k]) plist[(size_t)k].push_back(prns[(size_t)i]);
    std::vector<gnss_acquired> outs((size_t)M);
    std::vector<gnss_acq_diag> diags((size_t)M);
    std::vector<int> st((size_t)M, GNSS_ENODATA);
    std::vector<char> ran((size_t)M, 0);
    for_members(g, [&](int k) {
        memset(&outs[(size_t)k], 0, sizeof(gnss_acquired));
        memset(&diags[(size_t)k], 0, sizeof(gnss_acq_diag));
        if (plist[(size_t)k].empty()) return;  // (more members than PRNs)
        gnss_acq a = *acq;
        a.n_prn = (int32_t)plist[(size_t)k].size();
        a.prn_list = plist[(size_t)k].data();
        st[(size_t)k] = gnss_acquisition(g->members[(size_t)k], file, sg, &a, &outs[(size_t)k],
                                         diag ? &diags[(size_t)k] : nullptr);
        ran[(size_t)k] = 1;
    });
    std::vector<gnss_timing> tm;
    for (int k = 0; k < M; k++)
        if (ran[(size_t)k]) tm.push_back(g->members[(size_t)k]->timing);
    g->timing = group::combine_timing(tm);
    for (int k = 0; k < M; k++)
        if (st[(size_t)k] != GNSS_OK && st[(size_t)k] != GNSS_ENODATA)
            return fail(g, st[(size_t)k], "member %d (device %d): %s", k, g->members[(size_t)k]->device,
                        g->members[(size_t)k]->err.c_str());
    if (!group::merge_acquired(prns, shards, outs, diag ? &diags : nullptr, out, diag))
        return fail(g, GNSS_EDEVICE, "multi-device acquisition: member results do not match their PRN shards");
    const int status = group::acquisition_status(st, out->n);
    if (status == GNSS_ENODATA) return fail(g, GNSS_ENODATA, "No satellites acquired");  // :84-85
    return status;
}

namespace {
// What the coarse half of the acquisition hands to what follows it, while its buffers, its IF
// window and its events are alive.
struct AcqCoarse {
    const int8_t* blk;   // the staged IF bytes at the block's first sample
    const double2* xf;   // the fine block's samples (formats other than int8 I/Q), or nullptr
    int64_t flen, off, bps, S;
    int np, nb, dl, L, dtyp;
    bool iq8;
    int dbl, perm;       // the surface's precision and storage order (perm = P: tau2-major)
    const void* corr;    // the surface on the device: [np][nb][S] double (dbl) or float
    Events &e_conv, &e_all, &e_corr;
};

// acquisition.m:27-80: read block -> PRN x bin x ms search -> detector -> threshold into *out and
// *diag, then rest(AcqCoarse) on the same stream (gnss_acquisition: the fine search;
// gnss_acquisition_surface: the surface's download). One body, so both entries issue the same
// launches, allocations and events up to that point.
template <class Rest>
int acq_coarse(gnss_ctx* ctx, const gnss_file* file, const gnss_signal* sg, const gnss_acq* acq, gnss_acquired* out,
               gnss_acq_diag* diag, Rest&& rest)
{
    memset(out, 0, sizeof(*out));
    if (diag) memset(diag, 0, sizeof(*diag));
    ctx->timing = gnss_timing{};
    HIP_TRY(hipSetDevice(ctx->device));
    const int prec = file->dataPrecision, dtyp = file->dataType;
    if ((prec != 1 && prec != 2) || (dtyp != 1 && dtyp != 2))
        return fail(ctx, GNSS_EARG, "dataPrecision must be 1 (int8) or 2 (int16), dataType 1 (I) or 2 (I/Q)");
    // int16 values are de-interleaved into I/Q whatever dataType says (acquisition.m:28-32):
    // with dataType 1 the block holds half the samples and rawsignal(..idx*Sample) fails
    if (prec == 2 && dtyp == 1)
        return fail(ctx, GNSS_EINDEX, "int16 real record: rawsignal has Sample*datalen/2 samples (MATLAB index error)");
    const int64_t bps = (int64_t)prec * dtyp;  // file bytes per sample
    const bool iq8 = prec == 1 && dtyp == 2;   // the kernels' native input
    const int64_t S = sg->Sample;
    const int nb = acq->freqNum, dl = acq->datalen, L = acq->L;
    if (S <= 0 || nb <= 0 || dl <= 0 || L <= 0) return fail(ctx, GNSS_EARG, "bad acquisition sizes");

    std::vector<int32_t> prns;
    if (acq->n_prn > 0 && acq->prn_list) prns.assign(acq->prn_list, acq->prn_list + acq->n_prn);
    else for (int i = 1; i <= 32; i++) prns.push_back(i);  // acquisition.m:47
    if (prns.size() > GNSS_MAX_SV) return fail(ctx, GNSS_EARG, "too many PRNs");
    for (int p : prns) if (p < 1 || p > 51) return fail(ctx, GNSS_EARG, "PRN %d out of range", p);
    const int np = (int)prns.size();

    const int64_t off = file->skip * S * file->dataPrecision * file->dataType;  // :27
    const int64_t need = S * bps * std::max<int64_t>(dl, L + 1);
    const int64_t flen = file_length(file);
    if (flen < off + S * bps * dl) return fail(ctx, GNSS_EIO, "IF record too short for acquisition");
    IfWindow w;
    int st = stage_window(ctx, file, off, off + need, w);
    if (st) return st;
    const int8_t* blk = w.ptr + (off - w.base);
    // other formats: the samples of each fread as fp64 complex (ifmt.hip): the 20-ms block
    // (:28-37) and, with its own means, the (L+1)-ms fine block (:90-99)
    DevBuf xs_acq, xs_fine, xs_sums;
    Events e_conv;
    if (!iq8) {
        const int64_t nfine = flen >= off + S * bps * (L + 1) ? S * (L + 1) : 0;
        HIP_TRY(xs_acq.alloc(ctx, "acq.xs", sizeof(double2) * (size_t)(S * dl)));
        if (nfine) HIP_TRY(xs_fine.alloc(ctx, "acq.xs_fine", sizeof(double2) * (size_t)nfine));
        HIP_TRY(xs_sums.alloc(ctx, "acq.xs_sums", 32));
        HIP_TRY(hipEventRecord(e_conv.a, ctx->stream));
        HIP_TRY(launch_stage_cpx(blk, prec, dtyp, S * dl, xs_acq.as<double2>(), xs_sums.as<unsigned long long>(),
                                 ctx->stream));
        if (nfine)
            HIP_TRY(launch_stage_cpx(blk, prec, dtyp, nfine, xs_fine.as<double2>(),
                                     xs_sums.as<unsigned long long>() + 2, ctx->stream));
        HIP_TRY(hipEventRecord(e_conv.b, ctx->stream));
    }
    const double2* xa = iq8 ? nullptr : xs_acq.as<double2>();
    const double2* xf = iq8 ? nullptr : xs_fine.as<double2>();

    std::vector<float> cah((size_t)np * 1023);
    for (int i = 0; i < np; i++) generate_ca(prns[i], &cah[(size_t)i * 1023]);
    DevBuf ca, corr, peaks, scratch;
    HIP_TRY(ca.alloc(ctx, "acq.ca", cah.size() * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(ca.p, cah.data(), cah.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    // correlation precision: fp64 = the reference's (MATLAB's fft / ifft / abs().^2 in
    // double, acquisition.m:56-61), the default; fp32 = the fast mode
    // (gnss_ctx_set_acq_precision)
    const int dbl = ctx->acq_fp64 ? 1 : 0;
    HIP_TRY(corr.alloc(ctx, "acq.corr", (dbl ? sizeof(double) : sizeof(float)) * (size_t)np * nb * S));
    HIP_TRY(peaks.alloc(ctx, "acq.peaks", sizeof(AcqPeak) * (size_t)np));
    HIP_TRY(scratch.alloc(ctx, "acq.scratch", acq_scratch_bytes(np, np)));
    Events e_all, e_corr;  // e_corr.b marks the end of the PRN search
    int perm = 0;
    DevBuf fsync;  // the fused correlator's counters (its error word is read below)
    if (dbl)
        st = acq_search<double2>(ctx, blk, xa, S, dl, nb, np, sg, acq, ca.as<float>(), corr.as<double>(), e_all,
                                 &perm, fsync);
    else
        st = acq_search<float2>(ctx, blk, xa, S, dl, nb, np, sg, acq, ca.as<float>(), corr.as<float>(), e_all,
                                &perm, fsync);
    if (st) return st;
    const int cshift = (int)std::ceil(sg->Fs / sg->codeFreqBasis);  // :66
    if (dbl)
        HIP_TRY(launch_acq_peak(corr.as<double>(), np, nb, S, cshift, perm, peaks.as<AcqPeak>(), scratch.p,
                                ctx->stream));
    else
        HIP_TRY(launch_acq_peak(corr.as<float>(), np, nb, S, cshift, perm, peaks.as<AcqPeak>(), scratch.p,
                                ctx->stream));
    HIP_TRY(hipEventRecord(e_corr.b, ctx->stream));
    std::vector<AcqPeak> ph((size_t)np);
    HIP_TRY(hipMemcpyAsync(ph.data(), peaks.p, sizeof(AcqPeak) * (size_t)np, hipMemcpyDeviceToHost, ctx->stream));
    unsigned fused_err = 0;
    if (fsync.p)
        HIP_TRY(hipMemcpyAsync(&fused_err, static_cast<char*>(fsync.p) + acq_fused_err_offset(), sizeof(unsigned),
                               hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (fused_err)
        return fail(ctx, GNSS_EDEVICE, "fused correlator: a pipeline wait timed out (grid not resident)");
    ctx->timing.acq_hypothesis_samples = (int64_t)np * nb * dl * S;

    std::vector<int> acq_idx;
    for (int i = 0; i < np; i++) {
        if (diag) {
            int k = diag->n++;
            diag->prn[k] = prns[i];
            diag->SNR[k] = ph[i].snr;
            diag->fbin[k] = ph[i].fbin + 1;
            diag->codePhase[k] = ph[i].cp + 1;
            diag->peak[k] = ph[i].peak;
            diag->peak2[k] = ph[i].peak2;
        }
        if (ph[i].snr >= 12) {  // :70-74
            int k = out->n++;
            out->sv[k] = prns[i];
            out->SNR[k] = ph[i].snr;
            out->Doppler[k] = acq->freqMin + acq->freqStep * (double)ph[i].fbin;
            out->codedelay[k] = ph[i].cp;  // codePhase - 1
            acq_idx.push_back(i);
        }
    }
    const AcqCoarse c{blk, xf, flen, off, bps, S, np, nb, dl, L, dtyp, iq8, dbl, perm, corr.p, e_conv, e_all, e_corr};
    return rest(c);
}

// gnss_acquisition after its coarse half: the empty result (acquisition.m:84-85) or the fine
// frequency of every acquired SV (:89-126) into out->fineFreq, and the call's timing.
int acq_fine(gnss_ctx* ctx, const gnss_file* file, const gnss_signal* sg, gnss_acquired* out,
                    const AcqCoarse& c)
{
    const int8_t* blk = c.blk;
    const double2* xf = c.xf;
    const int64_t flen = c.flen, off = c.off, bps = c.bps, S = c.S;
    const int dl = c.dl, L = c.L, dtyp = c.dtyp;
    const bool iq8 = c.iq8;
    Events &e_conv = c.e_conv, &e_all = c.e_all, &e_corr = c.e_corr;
    int st = GNSS_OK;
    if (out->n == 0) {
        HIP_TRY(hipEventRecord(e_all.b, ctx->stream));
        HIP_TRY(hipEventSynchronize(e_all.b));
        ctx->timing.acq_ms = e_all.ms();
        ctx->timing.acq_corr_ms = ctx->timing.acq_ms;
        return fail(ctx, GNSS_ENODATA, "No satellites acquired");  // :84-85
    }

    // fine frequency (:89-126)
    if (flen < off + S * bps * (L + 1)) return fail(ctx, GNSS_EIO, "IF record too short for fine search");
    const int fshift = dtyp == 2 ? 1 : 2;  // fftshift (:109) / real: first of a mirror pair
    const int na = out->n;
    const int64_t N = (int64_t)L * S * dl;  // :108
    if (N % 2) return fail(ctx, GNSS_EINDEX, "odd fftlength: MATLAB indexes past the end (:116)");
    std::vector<float> caf((size_t)na * 1023);
    std::vector<int32_t> cdh((size_t)na);
    for (int k = 0; k < na; k++) {
        generate_ca(out->sv[k], &caf[(size_t)k * 1023]);
        cdh[k] = out->codedelay[k];
    }
    DevBuf fca, fcd, fx, kb;
    HIP_TRY(fca.alloc(ctx, "acq.fca", caf.size() * sizeof(float)));
    HIP_TRY(fcd.alloc(ctx, "acq.fcd", cdh.size() * sizeof(int32_t)));
    HIP_TRY(kb.alloc(ctx, "acq.kb", sizeof(int64_t) * (size_t)na));
    HIP_TRY(hipMemcpyAsync(fca.p, caf.data(), caf.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(fcd.p, cdh.data(), cdh.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    const bool own_fine = fine_fft_supported(S, L) && !ctx->opt[GNSS_OPT_FINE_ROCFFT];
    Events e_fine;
    if (own_fine) {
        // per-SV zero-padded FFT as datalen three-level transforms (acq_fft.hip), up to
        // kFineBatch SVs per launch (each SV's N-point slab, 186 MB at config 2, in one scratch)
        const int fb = std::min(na, kFineBatch);
        HIP_TRY(fx.alloc(ctx, "acq.fx", fine_fft_scratch_bytes(S, L, dl, fb)));
        HIP_TRY(hipEventRecord(e_fine.a, ctx->stream));
        HIP_TRY(launch_fine_fft_tables(S, L, dl, fx.p, ctx->stream));
        for (int k0 = 0; k0 < na; k0 += fb) {
            const int nk = std::min(fb, na - k0);
            HIP_TRY(launch_fine_fft_argmax(blk, xf, S, L, dl, fcd.as<int32_t>() + k0, nk,
                                           fca.as<float>() + (size_t)k0 * 1023, sg->Fs, sg->codeFreqBasis,
                                           sg->codelength, fshift, fx.p, kb.as<int64_t>() + k0, ctx->stream));
        }
    } else {
        HIP_TRY(fx.alloc(ctx, "acq.fx", sizeof(double2) * (size_t)na * N));
        rocfft_plan pl;
        if ((st = get_plan(ctx, N, na, 1, 0, &pl))) return st;
        HIP_TRY(hipEventRecord(e_fine.a, ctx->stream));
        HIP_TRY(launch_fine_build(blk, xf, S, L, fcd.as<int32_t>(), fca.as<float>(), na, sg->Fs, sg->codeFreqBasis,
                                  sg->codelength, N, fx.as<double2>(), ctx->stream));
        if ((st = run_fft(ctx, fx.p, N, na, 1, 0))) return st;
        DevBuf fscr;
        HIP_TRY(fscr.alloc(ctx, "acq.fscr", acq_scratch_bytes(1, na)));
        HIP_TRY(launch_fine_argmax(fx.as<double2>(), na, N, fshift, fscr.p, kb.as<int64_t>(), ctx->stream));
    }
    HIP_TRY(hipEventRecord(e_fine.b, ctx->stream));
    HIP_TRY(hipEventRecord(e_all.b, ctx->stream));
    std::vector<int64_t> kh((size_t)na);
    HIP_TRY(hipMemcpyAsync(kh.data(), kb.p, sizeof(int64_t) * (size_t)na, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < na; k++) {
        const double K = (double)kh[k];
        out->fineFreq[k] = (file->dataType == 2) ? (-K * (sg->Fs / (double)N) + sg->Fs / 2) : (K * (sg->Fs / (double)N));
    }
    {
        float f = 0;
        (void)hipEventElapsedTime(&f, e_all.a, e_corr.b);
        ctx->timing.acq_corr_ms = f;
    }
    ctx->timing.acq_fine_ms = e_fine.ms();
    ctx->timing.acq_ms = e_all.ms() + (iq8 ? 0.0 : e_conv.ms());
    return GNSS_OK;
}

// gnss_acquisition_surface after the same coarse half: corr back to the host, widened to double
// and, where the own correlator stored it tau2-major (perm = P: storage k holds column
// k / 2000 + P * (k % 2000), acq.hip natural_col), put in natural column order.
int acq_surface_out(gnss_ctx* ctx, double* surface_out, const AcqCoarse& c)
{
    const size_t cells = (size_t)c.np * c.nb * (size_t)c.S;
    std::vector<char> h(cells * (c.dbl ? sizeof(double) : sizeof(float)));
    HIP_TRY(hipMemcpyAsync(h.data(), c.corr, h.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipEventRecord(c.e_all.b, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->timing.acq_corr_ms = c.e_all.ms();
    ctx->timing.acq_ms = ctx->timing.acq_corr_ms + (c.iq8 ? 0.0 : c.e_conv.ms());
    const double* hd = reinterpret_cast<const double*>(h.data());
    const float* hf = reinterpret_cast<const float*>(h.data());
    const int64_t S = c.S;
    parallel_for(c.np * c.nb, [&](int r) {
        double* o = surface_out + (size_t)r * S;
        for (int64_t k = 0; k < S; k++) {
            const int64_t col = c.perm ? k / 2000 + (int64_t)c.perm * (k % 2000) : k;
            o[col] = c.dbl ? hd[(size_t)r * S + k] : (double)hf[(size_t)r * S + k];
        }
    });
    return GNSS_OK;
}
}  // namespace

extern "C" {

// ---------------------------------------------------------------------------
// acquisition.m
// ---------------------------------------------------------------------------
int gnss_acquisition(gnss_ctx* ctx, const gnss_file* file, const gnss_signal* sg,
                     const gnss_acq* acq, gnss_acquired* out, gnss_acq_diag* diag)
{
    if (!ctx || !file || !sg || !acq || !out) return GNSS_EARG;
    if (!ctx->members.empty()) return group_acquisition(ctx, file, sg, acq, out, diag);
    return acq_coarse(ctx, file, sg, acq, out, diag,
                      [&](const AcqCoarse& c) { return acq_fine(ctx, file, sg, out, c); });
}

// The parity hook of the correlation surface (tests): gnss_acquisition's coarse half under the
// context's precision and options, then the whole surface in natural column order; no fine search.
int gnss_acquisition_surface(gnss_ctx* ctx, const gnss_file* file, const gnss_signal* sg, const gnss_acq* acq,
                             double* surface_out, gnss_acq_diag* diag)
{
    if (!ctx || !file || !sg || !acq || !surface_out) return GNSS_EARG;
    if (!ctx->members.empty()) return fail(ctx, GNSS_EARG, "gnss_acquisition_surface: single-device contexts only");
    gnss_acquired acquired;  // (the 12 dB gate's list: not reported here)
    return acq_coarse(ctx, file, sg, acq, &acquired, diag,
                      [&](const AcqCoarse& c) { return acq_surface_out(ctx, surface_out, c); });
}

}  // extern "C"
