// replay.cpp — gnss_replay_correlate: recorded tracking rows correlated again on any tap grid (the
// definition is in include/gnss_mi355x.h, the arithmetic of a row in replay.h). Here: every check
// (all before any launch), the host path (the rows dealt over up to 16 threads, each row summed by
// one thread in ascending sample order, so the bits do not depend on the thread count) and the
// device path: the row table's upload, the record's staging through stage_window -- in consecutive
// row segments when the rows' byte range exceeds the context's window --, the launches of
// replay.hip and the sums' download. Built with -ffp-contract=off.
#include <fcntl.h>
#include <unistd.h>

#include <cstring>
#include <vector>

#include "host.h"
#include "replay.h"

using namespace gnss;
using namespace gnss::host;

static_assert(kReplayMaxTaps == GNSS_REPLAY_MAX_TAPS && kReplayMaxChan == GNSS_MAX_SV, "replay.h restates the header");
static_assert(sizeof(ReplayArgs) <= 1024, "ReplayArgs goes to the kernel by value");

namespace {

bool is_finite(double x) { return x - x == 0; }

// bit i set <-> chip i is -1, as bytes
void ca_neg_bytes(int prn, uint8_t* out1023)
{
    unsigned w[32];
    ca_bits(prn, w);
    for (int i = 0; i < 1023; i++) out1023[i] = (uint8_t)((w[i >> 5] >> (i & 31)) & 1u);
}

// the bytes [lo, hi) of a host record or a file
int read_range(const gnss_file* f, int64_t lo, int64_t hi, std::vector<uint8_t>& buf, const uint8_t** base)
{
    if (f->data) {
        *base = reinterpret_cast<const uint8_t*>(f->data) + lo;
        return GNSS_OK;
    }
    buf.resize((size_t)(hi - lo));
    const int fd = open(f->path, O_RDONLY);
    if (fd < 0) return GNSS_EIO;
    int64_t got = 0;
    while (got < hi - lo) {
        const ssize_t r = pread(fd, buf.data() + got, (size_t)(hi - lo - got), lo + got);
        if (r <= 0) break;
        got += r;
    }
    close(fd);
    *base = buf.data();
    return got == hi - lo ? GNSS_OK : GNSS_EIO;
}

}  // namespace

extern "C" int gnss_replay_correlate(gnss_ctx* ctx, const gnss_file* file, const gnss_signal* signal,
                                     const gnss_replay_cfg* cfg, const gnss_replay_rows* rows, gnss_replay_out* out)
{
    if (!file || !signal || !cfg || !rows || !out) return fail(ctx, GNSS_EARG, "gnss_replay_correlate: a null argument");
    if (ctx && !ctx->members.empty())
        return fail(ctx, GNSS_EARG, "gnss_replay_correlate: a multi-device context (one device only)");
    const int nt = cfg->n_taps;
    if (nt < 1 || nt > GNSS_REPLAY_MAX_TAPS)
        return fail(ctx, GNSS_EARG, "gnss_replay_cfg.n_taps outside 1..%d", GNSS_REPLAY_MAX_TAPS);
    if (cfg->chip_off != 0 && cfg->chip_off != 1) return fail(ctx, GNSS_EARG, "gnss_replay_cfg.chip_off is not 0 or 1");
    if (cfg->flags & ~GNSS_OUT_DEVICE) return fail(ctx, GNSS_EARG, "gnss_replay_cfg: an unknown flag");
    if (!cfg->tap_offsets) return fail(ctx, GNSS_EARG, "gnss_replay_cfg.tap_offsets is null");
    for (int s = 0; s < nt; s++) {
        if (!is_finite(cfg->tap_offsets[s]) || fabs(cfg->tap_offsets[s]) > kReplayMaxTap)
            return fail(ctx, GNSS_EARG, "gnss_replay_cfg.tap_offsets[%d] is not a finite value within +-1023", s);
        if (cfg->post && (!is_finite(cfg->post[s]) || fabs(cfg->post[s]) > kReplayMaxTap))
            return fail(ctx, GNSS_EARG, "gnss_replay_cfg.post[%d] is not a finite value within +-1023", s);
    }
    if (file->dataPrecision != 1 || (file->dataType != 1 && file->dataType != 2))
        return fail(ctx, GNSS_EARG, "gnss_replay_correlate: int8 records only (dataPrecision 1, dataType 1 or 2)");
    if (!file->dev_data && !file->data && !file->path) return fail(ctx, GNSS_EARG, "gnss_file names no record");
    if (!ctx && file->dev_data) return fail(ctx, GNSS_EARG, "gnss_replay_correlate: a device record needs a context");
    const double Fs = signal->Fs;
    if (!is_finite(Fs) || !(Fs > 0)) return fail(ctx, GNSS_EARG, "gnss_signal.Fs is not a positive finite value");
    const int nch = rows->n_chan;
    const int64_t MR = rows->max_rows;
    if (nch < 1 || nch > GNSS_MAX_SV) return fail(ctx, GNSS_EARG, "gnss_replay_rows.n_chan outside 1..%d", GNSS_MAX_SV);
    if (MR < 0 || MR > 0x7fffffff / GNSS_MAX_SV) return fail(ctx, GNSS_EARG, "gnss_replay_rows.max_rows outside 0..2^25-1");
    if (!rows->prn || !rows->n_rows || !rows->pos_bytes || !rows->numSample || !rows->remChip || !rows->codeFreq ||
        !rows->carrFreq || !rows->remPhase)
        return fail(ctx, GNSS_EARG, "gnss_replay_rows: a null array");
    if (!out->taps) return fail(ctx, GNSS_EARG, "gnss_replay_out.taps is null");
    const bool dev_out = (cfg->flags & GNSS_OUT_DEVICE) != 0;
    if (dev_out && !ctx) return fail(ctx, GNSS_EARG, "gnss_replay_correlate: GNSS_OUT_DEVICE needs a context");
    int64_t most = 0, total = 0;
    for (int c = 0; c < nch; c++) {
        if (rows->prn[c] < 1 || rows->prn[c] > 51) return fail(ctx, GNSS_EARG, "gnss_replay_rows.prn[%d] outside 1..51", c);
        if (rows->n_rows[c] < 0 || rows->n_rows[c] > MR)
            return fail(ctx, GNSS_EARG, "gnss_replay_rows.n_rows[%d] outside 0..max_rows", c);
        most = std::max(most, rows->n_rows[c]);
        total += rows->n_rows[c];
    }
    const size_t out_bytes = (size_t)nch * 2 * (size_t)nt * (size_t)MR * sizeof(double);
    if (dev_out) {
        HIP_TRY(hipSetDevice(ctx->device));
        if (!device_memory_of(out->taps, out_bytes, ctx->device))
            return fail(ctx, GNSS_EARG, "gnss_replay_out.taps is not [n_chan][2][n_taps][max_rows] of the context's device");
    }
    // the rows: values (GNSS_EARG), then the reads (GNSS_EIO), then the colons (GNSS_EINDEX)
    const int bps = file->dataType;  // int8: bytes per sample
    int64_t nmax = 0;
    for (int c = 0; c < nch; c++)
        for (int64_t i = 0; i < rows->n_rows[c]; i++) {
            const int64_t at = (int64_t)c * MR + i, n = rows->numSample[at];
            if (n < 1 || n > kReplayMaxSamples)
                return fail(ctx, GNSS_EARG, "channel %d row %lld: numSample outside 1..2^22", c, (long long)i);
            const double cf = rows->codeFreq[at];
            if (!is_finite(rows->remChip[at]) || !is_finite(cf) || !is_finite(rows->carrFreq[at]) || !is_finite(rows->remPhase[at]) ||
                fabs(rows->remChip[at]) > kReplayMaxChips)
                return fail(ctx, GNSS_EARG, "channel %d row %lld: a non-finite NCO state", c, (long long)i);
            if (!(cf > 0) || !((double)(n - 1) * (cf / Fs) <= kReplayMaxChips))
                return fail(ctx, GNSS_EARG, "channel %d row %lld: codeFreq is not positive or the row spans over 2^28 chips",
                            c, (long long)i);
            nmax = std::max(nmax, n);
        }
    const int64_t flen = file_length(file);
    if (flen < 0) return fail(ctx, GNSS_EIO, "cannot open IF record '%s'", file->path ? file->path : "");
    int64_t lo_all = flen, hi_all = 0;
    for (int c = 0; c < nch; c++)
        for (int64_t i = 0; i < rows->n_rows[c]; i++) {
            const int64_t at = (int64_t)c * MR + i, p = rows->pos_bytes[at], n = rows->numSample[at];
            if (p < 0 || p % bps != 0 || p > flen || n * bps > flen - p)
                return fail(ctx, GNSS_EIO, "channel %d row %lld: the read [%lld, +%lld samples) is misaligned or outside the record",
                            c, (long long)i, (long long)p, (long long)n);
            lo_all = std::min(lo_all, p);
            hi_all = std::max(hi_all, p + n * bps);
        }
    bool table = true;  // every (row, tile) within the kernel's code table
    for (int c = 0; c < nch; c++)
        for (int64_t i = 0; i < rows->n_rows[c]; i++) {
            const int64_t at = (int64_t)c * MR + i, n = rows->numSample[at];
            const double d = rows->codeFreq[at] / Fs;
            for (int j0 = 0; j0 < nt; j0 += kReplayTile) {
                int lo = 0x7fffffff, hi = -0x7fffffff;
                for (int s = j0; s < nt && s < j0 + kReplayTile; s++) {
                    const RpColon col = rp_tap_colon(cfg->tap_offsets[s], rows->remChip[at], d, n);
                    if (col.n != n - 1)
                        return fail(ctx, GNSS_EINDEX, "channel %d row %lld tap %d: the colon has %lld elements, not numSample = %lld",
                                    c, (long long)i, s, (long long)(col.n + 1), (long long)n);
                    int l, h;
                    rp_chip_range(col.a, col.c, cfg->post ? cfg->post[s] : 0.0, &l, &h);
                    lo = std::min(lo, l);
                    hi = std::max(hi, h);
                }
                if ((int64_t)hi - lo + 1 > kReplayTabMax) table = false;
            }
        }
    out->kernel_ms = 0;
    if (total == 0) return GNSS_OK;

    if (!ctx) {
        std::vector<uint8_t> buf;
        const uint8_t* rec = nullptr;
        if (read_range(file, lo_all, hi_all, buf, &rec) != GNSS_OK) return GNSS_EIO;
        std::vector<uint8_t> neg((size_t)nch * 1023);
        std::vector<std::pair<int, int64_t>> work;
        work.reserve((size_t)total);
        for (int c = 0; c < nch; c++) {
            if (rows->n_rows[c] > 0) ca_neg_bytes(rows->prn[c], &neg[(size_t)c * 1023]);
            for (int64_t i = 0; i < rows->n_rows[c]; i++) work.emplace_back(c, i);
        }
        parallel_for((int)work.size(), [&](int w) {
            const int c = work[(size_t)w].first;
            const int64_t i = work[(size_t)w].second, at = (int64_t)c * MR + i;
            RpRow r;
            r.x = rec + (rows->pos_bytes[at] - lo_all);
            r.n = rows->numSample[at];
            r.dtype = file->dataType;
            r.Fs = Fs;
            r.rfs = 0.0;
            r.f = rows->carrFreq[at];
            r.phi0 = rows->remPhase[at];
            r.d = rows->codeFreq[at] / Fs;
            double* oI = out->taps + ((int64_t)c * 2 * nt) * MR + i;
            replay_row_host(r, rows->remChip[at], &neg[(size_t)c * 1023], nt, cfg->tap_offsets, cfg->post, cfg->chip_off, oI,
                            oI + (int64_t)nt * MR, MR);
        });
        return GNSS_OK;
    }

    // ---- the device path --------------------------------------------------------------------------
    HIP_TRY(hipSetDevice(ctx->device));
    ctx->timing = gnss_timing{};
    // row segments [r0, r1): one when the record is resident or the window holds the whole range
    std::vector<std::pair<int64_t, int64_t>> seg;
    const int64_t window = (int64_t)ctx->window;
    if (file->dev_data || window == 0 || hi_all - (lo_all & ~(int64_t)15) <= window) {
        seg.emplace_back(0, most);
    } else {
        int64_t r0 = 0, lo = flen, hi = 0;
        for (int64_t i = 0; i < most; i++) {
            int64_t l = flen, h = 0;
            for (int c = 0; c < nch; c++)
                if (i < rows->n_rows[c]) {
                    const int64_t at = (int64_t)c * MR + i;
                    l = std::min(l, rows->pos_bytes[at]);
                    h = std::max(h, rows->pos_bytes[at] + rows->numSample[at] * bps);
                }
            if (h - (l & ~(int64_t)15) > window)
                return fail(ctx, GNSS_EARG, "row %lld of all channels spans %lld bytes, over the context's window of %lld",
                            (long long)i, (long long)(h - l), (long long)window);
            if (i > r0 && std::max(hi, h) - (std::min(lo, l) & ~(int64_t)15) > window) {
                seg.emplace_back(r0, i);
                r0 = i;
                lo = flen;
                hi = 0;
            }
            lo = std::min(lo, l);
            hi = std::max(hi, h);
        }
        seg.emplace_back(r0, most);
    }

    ctx->timing.track_segments = (int64_t)seg.size();
    const size_t cells = (size_t)nch * (size_t)MR;
    DevBuf bpos, bns, brc, bcf, bcr, brp, bca, btap, bpost, bout;
    HIP_TRY(bpos.alloc(ctx, "replay_pos", cells * 8));
    HIP_TRY(bns.alloc(ctx, "replay_ns", cells * 8));
    HIP_TRY(brc.alloc(ctx, "replay_remChip", cells * 8));
    HIP_TRY(bcf.alloc(ctx, "replay_codeFreq", cells * 8));
    HIP_TRY(bcr.alloc(ctx, "replay_carrFreq", cells * 8));
    HIP_TRY(brp.alloc(ctx, "replay_remPhase", cells * 8));
    HIP_TRY(bca.alloc(ctx, "replay_ca", (size_t)nch * 32 * sizeof(unsigned)));
    HIP_TRY(btap.alloc(ctx, "replay_taps", (size_t)nt * 8));
    HIP_TRY(bpost.alloc(ctx, "replay_post", (size_t)nt * 8));
    if (!dev_out) HIP_TRY(bout.alloc(ctx, "replay_out", out_bytes));
    std::vector<unsigned> ca((size_t)nch * 32, 0u);
    for (int c = 0; c < nch; c++)
        if (rows->n_rows[c] > 0) ca_bits(rows->prn[c], &ca[(size_t)c * 32]);
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(bpos.p, rows->pos_bytes, cells * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(bns.p, rows->numSample, cells * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(brc.p, rows->remChip, cells * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(bcf.p, rows->codeFreq, cells * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(bcr.p, rows->carrFreq, cells * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(brp.p, rows->remPhase, cells * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(bca.p, ca.data(), ca.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(btap.p, cfg->tap_offsets, (size_t)nt * 8, hipMemcpyHostToDevice, st));
    if (cfg->post) HIP_TRY(hipMemcpyAsync(bpost.p, cfg->post, (size_t)nt * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // (the host arrays are pageable: the copies have left them)

    ReplayArgs a{};
    a.pos = bpos.as<int64_t>();
    a.ns = bns.as<int64_t>();
    a.remChip = brc.as<double>();
    a.codeFreq = bcf.as<double>();
    a.carrFreq = bcr.as<double>();
    a.remPhase = brp.as<double>();
    a.ca_bits = bca.as<unsigned>();
    a.taps = btap.as<double>();
    a.post = cfg->post ? bpost.as<double>() : nullptr;
    a.out = dev_out ? out->taps : bout.as<double>();
    a.max_rows = MR;
    a.n_taps = nt;
    a.chip_off = cfg->chip_off;
    a.dtype = file->dataType;
    a.n_chan = nch;
    a.Fs = Fs;
    a.rfs = fast_div_exact(Fs, nmax) ? 1.0 / Fs : 0.0;
    for (int c = 0; c < nch; c++) a.n_rows[c] = rows->n_rows[c];
    Events ev;
    double ms = 0;
    for (const auto& sg : seg) {
        int64_t lo = flen, hi = 0;
        for (int c = 0; c < nch; c++)
            for (int64_t i = sg.first; i < sg.second && i < rows->n_rows[c]; i++) {
                const int64_t at = (int64_t)c * MR + i;
                lo = std::min(lo, rows->pos_bytes[at]);
                hi = std::max(hi, rows->pos_bytes[at] + rows->numSample[at] * bps);
            }
        if (hi <= lo) continue;
        IfWindow w;
        const int ws = stage_window(ctx, file, lo, hi, w);
        if (ws) return ws;
        if (w.base > lo || w.base + w.len < hi) return fail(ctx, GNSS_EIO, "the staged window does not hold the rows' reads");
        a.rec = reinterpret_cast<const uint8_t*>(w.ptr);
        a.base = w.base;
        a.row0 = sg.first;
        HIP_TRY(hipEventRecord(ev.a, st));
        const int le = replay_launch(a, sg.second - sg.first, table, st);
        if (le) return fail(ctx, GNSS_EDEVICE, "gnss_replay_correlate: kernel launch: %s", hipGetErrorString((hipError_t)le));
        HIP_TRY(hipEventRecord(ev.b, st));
        HIP_TRY(hipEventSynchronize(ev.b));  // (the window is freed when w leaves scope)
        ms += ev.ms();
    }
    if (!dev_out) {
        for (int c = 0; c < nch; c++) {
            if (rows->n_rows[c] == 0) continue;
            const size_t off = (size_t)c * 2 * (size_t)nt * (size_t)MR;
            HIP_TRY(hipMemcpy2DAsync(out->taps + off, (size_t)MR * 8, bout.as<double>() + off, (size_t)MR * 8,
                                     (size_t)rows->n_rows[c] * 8, (size_t)2 * nt, hipMemcpyDeviceToHost, st));
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    out->kernel_ms = ms;
    return GNSS_OK;
}
