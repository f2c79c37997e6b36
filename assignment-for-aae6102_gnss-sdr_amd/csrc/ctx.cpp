// ctx.cpp -- the context of the C-ABI (include/gnss_mi355x.h) and what every entry point shares
// (host.h): the HIP streams, the device and pinned pools, the resident-record cache of a group's
// members, IF staging (one window into HBM, or a caller-resident record), the rocFFT plan cache
// and the C/A codes.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <fcntl.h>
#include <unistd.h>

#include "host.h"

namespace gnss {
namespace host {

// frees a member's resident record copy (on that member's device)
static void release_resident(void* p)
{
    if (p) (void)hipFree(p);
}

int drop_resident(gnss_ctx* ctx, const void* p, uint64_t n)
{
    int k = 0;
    for (gnss_ctx* m : ctx->members) {
        (void)hipSetDevice(m->device);
        if (m->stream) (void)hipStreamSynchronize(m->stream);  // (no kernel still reads a copy)
        if (!p) {
            k += (int)m->resident.m.size();
            m->resident.clear(release_resident);
        } else {
            k += m->resident.drop_overlapping(p, n, release_resident);
        }
    }
    (void)hipSetDevice(ctx->device);
    return k;
}

int fail(gnss_ctx* ctx, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}

int64_t file_length(const gnss_file* f)
{
    if (f->dev_data || f->data) return (int64_t)f->nbytes;
    if (!f->path) return -1;
    int fd = open(f->path, O_RDONLY);
    if (fd < 0) return -1;
    int64_t s = lseek(fd, 0, SEEK_END);
    close(fd);
    return s;
}

// The file bytes [lo, hi) into device memory dst (returns once they have landed). Streaming staging (trackingCT.m:84-93 reads each step's block from the file;
// here windows are staged whole): chunks of kStageChunk bytes through two pinned host buffers
// of the context -- the disk read (or host copy) of chunk i+1 runs while the DMA engine moves
// chunk i into HBM; a buffer is refilled only after its previous DMA has completed.
int stage_into(gnss_ctx* ctx, const gnss_file* f, int64_t lo, int64_t hi, int8_t* dst)
{
    const int64_t n = hi - lo;
    if (n <= 0) return GNSS_OK;
    Events ev;
    HIP_TRY(hipEventRecord(ev.a, ctx->stream));
    constexpr int64_t kStageChunk = (int64_t)64 << 20;
    int8_t* pb[2] = {pinned_buffer<int8_t>(ctx, "stage.0", (size_t)kStageChunk),
                     pinned_buffer<int8_t>(ctx, "stage.1", (size_t)kStageChunk)};
    if (!pb[0] || !pb[1]) return fail(ctx, GNSS_EDEVICE, "pinned staging buffers");
    hipEvent_t done[2] = {nullptr, nullptr};
    HIP_TRY(hipEventCreateWithFlags(&done[0], hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&done[1], hipEventDisableTiming));
    struct EvGuard {
        hipEvent_t* e;
        ~EvGuard() { (void)hipEventDestroy(e[0]); (void)hipEventDestroy(e[1]); }
    } guard{done};
    // the descriptor is closed on every return; an early return (a failed HIP call or a short
    // read) first drains the stream, so no DMA still reads a pinned buffer the next call refills
    struct FdGuard {
        int fd;
        hipStream_t s;
        bool drained;
        ~FdGuard()
        {
            if (fd >= 0) close(fd);
            if (!drained) (void)hipStreamSynchronize(s);
        }
    } fg{-1, ctx->stream, false};
    if (!f->data) {
        fg.fd = open(f->path, O_RDONLY);
        if (fg.fd < 0) return fail(ctx, GNSS_EIO, "cannot open '%s'", f->path);
    }
    const int fd = fg.fd;
    int64_t off = 0;
    for (int i = 0; off < n; i++, off += kStageChunk) {
        const int64_t len = std::min(kStageChunk, n - off);
        int8_t* buf = pb[i & 1];
        if (i >= 2) HIP_TRY(hipEventSynchronize(done[i & 1]));  // its last DMA has drained
        if (f->data) {
            memcpy(buf, f->data + lo + off, (size_t)len);
        } else {
            int64_t got = 0;
            while (got < len) {
                const ssize_t r = pread(fd, buf + got, (size_t)(len - got), lo + off + got);
                if (r <= 0) break;
                got += r;
            }
            if (got != len) return fail(ctx, GNSS_EIO, "short read of '%s'", f->path);
        }
        HIP_TRY(hipMemcpyAsync(dst + off, buf, (size_t)len, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipEventRecord(done[i & 1], ctx->stream));
    }
    ctx->timing.h2d_bytes += n;
    HIP_TRY(hipEventRecord(ev.b, ctx->stream));
    HIP_TRY(hipEventSynchronize(ev.b));
    fg.drained = true;
    ctx->timing.h2d_ms += ev.ms();
    return GNSS_OK;
}

int pointer_device(const void* p)
{
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return a.device;
}

int stage_window(gnss_ctx* ctx, const gnss_file* f, int64_t lo, int64_t hi, IfWindow& w)
{
    const int64_t flen = file_length(f);
    if (flen < 0) return fail(ctx, GNSS_EIO, "cannot open IF record '%s'", f->path ? f->path : "");
    lo = std::max<int64_t>(0, lo & ~(int64_t)15);
    hi = std::min<int64_t>(hi, flen);
    if (hi <= lo) { hi = lo; }
    if (f->dev_data) {
        if ((reinterpret_cast<uintptr_t>(f->dev_data) & 15) != 0)
            return fail(ctx, GNSS_EARG, "dev_data must be 16-byte aligned");
        const int pd = ctx->member ? pointer_device(f->dev_data) : ctx->device;
        if (pd == ctx->device && !(ctx->member && ctx->opt[GNSS_OPT_FORCE_PEER])) {
            w.ptr = static_cast<const int8_t*>(f->dev_data);
            w.base = 0;
            w.len = flen;
            return GNSS_OK;
        }
        // a group member whose record lives on another device of the node (devices[0]): the
        // whole record into this device's HBM by one peer copy over xGMI, on the first call that
        // reads it; it stays resident for the later calls (group.h ResidentCache) until the
        // library writes into the record or the caller drops it (gnss_ctx_drop_record)
        const void* const* hit = ctx->resident.find(f->dev_data, (uint64_t)flen);
        if (!hit) {
            DevBuf copy;  // (freed on every early return; the cache takes it below)
            HIP_TRY(copy.alloc((size_t)flen + 64));
            Events ev;
            HIP_TRY(hipEventRecord(ev.a, ctx->stream));
            if (flen > 0 && hipMemcpyPeerAsync(copy.p, ctx->device, f->dev_data, pd < 0 ? ctx->device : pd,
                                               (size_t)flen, ctx->stream) != hipSuccess) {
                (void)hipStreamSynchronize(ctx->stream);
                return fail(ctx, GNSS_EDEVICE, "peer copy of the IF record (%lld bytes)", (long long)flen);
            }
            HIP_TRY(hipEventRecord(ev.b, ctx->stream));
            HIP_TRY(hipEventSynchronize(ev.b));
            ctx->timing.h2d_bytes += flen;
            ctx->timing.h2d_ms += ev.ms();
            ctx->resident.put(f->dev_data, (uint64_t)flen, copy.p, release_resident);
            copy.p = nullptr;  // (the cache owns it now)
            hit = ctx->resident.find(f->dev_data, (uint64_t)flen);
        }
        w.ptr = static_cast<const int8_t*>(*hit);
        w.base = 0;
        w.len = flen;
        return GNSS_OK;
    }
    const int64_t n = hi - lo;
    HIP_TRY(w.own.alloc((size_t)n + 64));
    const int st = stage_into(ctx, f, lo, hi, w.own.as<int8_t>());
    if (st) return st;
    w.ptr = w.own.as<int8_t>();
    w.base = lo;
    w.len = n;
    return GNSS_OK;
}

int get_plan(gnss_ctx* ctx, size_t len, size_t batch, int dbl, int inverse, rocfft_plan* out)
{
    auto key = std::make_tuple(len, batch, dbl, inverse);
    auto it = ctx->plans.find(key);
    if (it != ctx->plans.end()) { *out = it->second; return GNSS_OK; }
    rocfft_plan plan = nullptr;
    rocfft_status st = rocfft_plan_create(
        &plan, rocfft_placement_inplace,
        inverse ? rocfft_transform_type_complex_inverse : rocfft_transform_type_complex_forward,
        dbl ? rocfft_precision_double : rocfft_precision_single, 1, &len, batch, nullptr);
    if (st != rocfft_status_success)
        return fail(ctx, GNSS_EDEVICE, "rocfft_plan_create(len=%zu, batch=%zu) failed: %d", len, batch, (int)st);
    size_t ws = 0;
    rocfft_plan_get_work_buffer_size(plan, &ws);
    if (ws > ctx->fft_work_size) {
        if (ctx->fft_work) (void)hipFree(ctx->fft_work);
        ctx->fft_work = nullptr;
        HIP_TRY(hipMalloc(&ctx->fft_work, ws));
        ctx->fft_work_size = ws;
    }
    ctx->plans[key] = plan;
    *out = plan;
    return GNSS_OK;
}

int run_fft(gnss_ctx* ctx, void* data, size_t len, size_t batch, int dbl, int inverse)
{
    rocfft_plan plan;
    int st = get_plan(ctx, len, batch, dbl, inverse, &plan);
    if (st) return st;
    rocfft_execution_info info = nullptr;
    rocfft_execution_info_create(&info);
    rocfft_execution_info_set_stream(info, ctx->stream);
    if (ctx->fft_work_size) rocfft_execution_info_set_work_buffer(info, ctx->fft_work, ctx->fft_work_size);
    void* bufs[1] = {data};
    rocfft_status rs = rocfft_execute(plan, bufs, nullptr, info);
    rocfft_execution_info_destroy(info);
    if (rs != rocfft_status_success) return fail(ctx, GNSS_EDEVICE, "rocfft_execute failed: %d", (int)rs);
    return GNSS_OK;
}

// C/A chips as 32 words of bits (bit i set <-> chip i is -1), read by the kernels
// through lane shuffles
void ca_bits(int prn, unsigned* out32)
{
    float f[1023];
    generate_ca(prn, f);
    for (int w = 0; w < 32; w++) out32[w] = 0;
    for (int i = 0; i < 1023; i++)
        if (f[i] < 0) out32[i >> 5] |= 1u << (i & 31);
}

// generateCAcode.m:16-64 (host copy; the oracle has its own independent one)
void generate_ca(int prn, float* out)
{
    static const int g2s[51] = {5,   6,   7,   8,   17,  18,  139, 140, 141, 251, 252, 254, 255,
                                256, 257, 258, 469, 470, 471, 472, 473, 474, 509, 512, 513, 514,
                                515, 516, 859, 860, 861, 862, 145, 175, 52,  21,  237, 235, 886,
                                657, 634, 762, 355, 1012, 176, 603, 130, 359, 595, 68,  386};
    int g1[1023], g2[1023];
    unsigned r1 = 0x3FF, r2 = 0x3FF;  // bit i = stage i+1, all stages start at "-1" (= 1 here)
    for (int i = 0; i < 1023; i++) {
        g1[i] = (r1 >> 9) & 1;
        g2[i] = (r2 >> 9) & 1;
        unsigned f1 = ((r1 >> 2) ^ (r1 >> 9)) & 1;
        unsigned f2 = ((r2 >> 1) ^ (r2 >> 2) ^ (r2 >> 5) ^ (r2 >> 7) ^ (r2 >> 8) ^ (r2 >> 9)) & 1;
        r1 = ((r1 << 1) | f1) & 0x3FF;
        r2 = ((r2 << 1) | f2) & 0x3FF;
    }
    // +-1 product of "-1" states == XOR of bits; CA = -(g1 .* g2) -> +1 when bits differ... in
    // the reference's -1 -> bit 1 mapping: value(x) = -1 if bit 1 else +1.
    const int s = g2s[prn - 1];
    for (int i = 0; i < 1023; i++) {
        const int src = (i < s) ? (1023 - s + i) : (i - s);
        const int v1 = g1[i] ? -1 : 1, v2 = g2[src] ? -1 : 1;
        out[i] = (float)(-(v1 * v2));
    }
}

}  // namespace host

// generateCAcode.m chips for the other host translation units (vt.cpp)
void ca_chips(int prn, float* out) { host::generate_ca(prn, out); }

}  // namespace gnss

using namespace gnss;
using namespace gnss::host;

extern "C" {

int gnss_abi_version(void) { return GNSS_ABI_VERSION; }

const char* gnss_strerror(int s)
{
    switch (s) {
    case GNSS_OK: return "ok";
    case GNSS_ENODATA: return "no data (no satellites acquired / not enough raw data)";
    case GNSS_EIO: return "I/O error or read past end of IF record";
    case GNSS_EARG: return "invalid or unsupported argument";
    case GNSS_EDEVICE: return "HIP/rocFFT device error";
    case GNSS_EINDEX: return "index out of range (MATLAB would raise an error)";
    case GNSS_ENOCONV: return "the position fit did not converge (olspos.m has no iteration cap)";
    default: return "unknown status";
    }
}

int gnss_ctx_create(int device, gnss_ctx** out)
{
    if (!out) return GNSS_EARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return GNSS_EDEVICE;
    if (device < 0 || device >= n) return GNSS_EARG;
    if (hipSetDevice(device) != hipSuccess) return GNSS_EDEVICE;
    gnss_ctx* ctx = new gnss_ctx();
    ctx->device = device;
    bool ok = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; i < 2 && ok; i++)
        ok = hipEventCreateWithFlags(&ctx->ev_cols[i], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&ctx->ev_rows[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        gnss_ctx_destroy(ctx);
        return GNSS_EDEVICE;
    }
    rocfft_setup();
    *out = ctx;
    return GNSS_OK;
}

int gnss_ctx_create_multi(const int* devices, int n, gnss_ctx** out)
{
    if (!out) return GNSS_EARG;
    *out = nullptr;
    if (!devices || n < 1 || n > GNSS_MAX_DEVICES) return GNSS_EARG;
    gnss_ctx* g = nullptr;
    int st = gnss_ctx_create(devices[0], &g);
    if (st) return st;
    for (int k = 0; k < n; k++) {
        gnss_ctx* m = nullptr;
        if ((st = gnss_ctx_create(devices[k], &m))) {
            gnss_ctx_destroy(g);
            return st;
        }
        m->member = true;
        g->members.push_back(m);
    }
    // peer access between the distinct devices (the xGMI copies of records and rows; a pair
    // without it still copies, staged by the runtime)
    std::vector<int> ds(devices, devices + n);
    std::sort(ds.begin(), ds.end());
    ds.erase(std::unique(ds.begin(), ds.end()), ds.end());
    for (int a : ds)
        for (int b : ds) {
            int can = 0;
            if (a == b || hipDeviceCanAccessPeer(&can, a, b) != hipSuccess || !can) continue;
            if (hipSetDevice(a) == hipSuccess) (void)hipDeviceEnablePeerAccess(b, 0);
            (void)hipGetLastError();  // (hipErrorPeerAccessAlreadyEnabled is fine)
        }
    (void)hipSetDevice(devices[0]);
    *out = g;
    return GNSS_OK;
}

int gnss_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int gnss_ctx_members(const gnss_ctx* ctx)
{
    if (!ctx) return 0;
    return ctx->members.empty() ? 1 : (int)ctx->members.size();
}

void gnss_ctx_destroy(gnss_ctx* ctx)
{
    if (!ctx) return;
    for (gnss_ctx* m : ctx->members) gnss_ctx_destroy(m);
    ctx->members.clear();
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    ctx->resident.clear(release_resident);
    if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
    for (auto& kv : ctx->plans) rocfft_plan_destroy(kv.second);
    if (ctx->fft_work) (void)hipFree(ctx->fft_work);
    for (auto& kv : ctx->pool)
        if (kv.second.first) (void)hipFree(kv.second.first);
    for (auto& kv : ctx->pinned)
        if (kv.second.first) (void)hipHostFree(kv.second.first);
    for (int i = 0; i < 2; i++) {
        if (ctx->ev_cols[i]) (void)hipEventDestroy(ctx->ev_cols[i]);
        if (ctx->ev_rows[i]) (void)hipEventDestroy(ctx->ev_rows[i]);
    }
    if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char* gnss_last_error(const gnss_ctx* ctx) { return ctx ? ctx->err.c_str() : "no context"; }

int gnss_last_timing(const gnss_ctx* ctx, gnss_timing* out)
{
    if (!ctx || !out) return GNSS_EARG;
    *out = ctx->timing;
    return GNSS_OK;
}

int gnss_ctx_set_profiling(gnss_ctx* ctx, int enable)
{
    if (!ctx) return GNSS_EARG;
    ctx->profiling = enable;
    for (gnss_ctx* m : ctx->members) m->profiling = enable;
    return GNSS_OK;
}

int gnss_ctx_set_window(gnss_ctx* ctx, uint64_t bytes)
{
    if (!ctx) return GNSS_EARG;
    ctx->window = bytes;
    for (gnss_ctx* m : ctx->members) m->window = bytes;
    return GNSS_OK;
}

int gnss_ctx_set_option(gnss_ctx* ctx, int key, int64_t value)
{
    if (!ctx || key < 0 || key >= GNSS_OPT_COUNT) return GNSS_EARG;
    if (key == GNSS_OPT_VT_BLOCKS && (value < 0 || value > GNSS_VT_MAX_BLOCKS))
        return fail(ctx, GNSS_EARG, "GNSS_OPT_VT_BLOCKS outside 0..%d", GNSS_VT_MAX_BLOCKS);
    if (key == GNSS_OPT_SLOT_PATH && (value < 0 || value > 2))
        return fail(ctx, GNSS_EARG, "GNSS_OPT_SLOT_PATH outside 0..2");
    if (key == GNSS_OPT_VT_SPAN && (value < 0 || value > kVtSpan))
        return fail(ctx, GNSS_EARG, "GNSS_OPT_VT_SPAN outside 0..%d", kVtSpan);
    ctx->opt[key] = value;
    for (gnss_ctx* m : ctx->members) m->opt[key] = value;
    return GNSS_OK;
}

int gnss_ctx_set_acq_precision(gnss_ctx* ctx, int fp64)
{
    if (!ctx || (fp64 != 0 && fp64 != 1)) return GNSS_EARG;
    ctx->acq_fp64 = fp64;
    for (gnss_ctx* m : ctx->members) m->acq_fp64 = fp64;
    return GNSS_OK;
}

int gnss_dev_alloc(gnss_ctx* ctx, uint64_t nbytes, void** dev_ptr)
{
    if (!ctx || !dev_ptr) return GNSS_EARG;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMalloc(dev_ptr, nbytes ? nbytes : 16));
    return GNSS_OK;
}

int gnss_ctx_drop_record(gnss_ctx* ctx, const void* dev_ptr)
{
    if (!ctx) return GNSS_EARG;
    drop_resident(ctx, dev_ptr, 0);
    return GNSS_OK;
}

int gnss_ctx_resident_records(const gnss_ctx* ctx)
{
    if (!ctx) return 0;
    int k = 0;
    for (const gnss_ctx* m : ctx->members) k += (int)m->resident.m.size();
    return k;
}

int gnss_dev_free(gnss_ctx* ctx, void* p)
{
    if (!ctx) return GNSS_EARG;
    drop_resident(ctx, p, 0);  // (the pointer may be handed out again by a later allocation)
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipFree(p));
    return GNSS_OK;
}

int gnss_dev_upload(gnss_ctx* ctx, void* dst, const void* src, uint64_t n)
{
    if (!ctx) return GNSS_EARG;
    drop_resident(ctx, dst, n);  // (a member's copy of these bytes is stale now)
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return GNSS_OK;
}

int gnss_dev_download(gnss_ctx* ctx, void* dst, const void* src, uint64_t n)
{
    if (!ctx) return GNSS_EARG;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return GNSS_OK;
}

int gnss_ca_code(int prn, int8_t* out1023)
{
    if (prn < 1 || prn > 51 || !out1023) return GNSS_EARG;
    float f[1023];
    generate_ca(prn, f);
    for (int i = 0; i < 1023; i++) out1023[i] = (int8_t)f[i];
    return GNSS_OK;
}

int gnss_synth_if_device(gnss_ctx* ctx, const gnss_synth* cfg, uint64_t sample0, uint64_t nsamples,
                         void* dev_dst)
{
    if (!ctx || !cfg || !dev_dst || cfg->n_sv < 0 || cfg->n_sv > GNSS_MAX_SV) return GNSS_EARG;
    drop_resident(ctx, dev_dst, 2 * nsamples);  // (int8 I/Q: a member's copy of these bytes is stale now)
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<float> cah((size_t)std::max(1, cfg->n_sv) * 1023);
    for (int i = 0; i < cfg->n_sv; i++) {
        if (cfg->sv[i].prn < 1 || cfg->sv[i].prn > 51) return GNSS_EARG;
        generate_ca(cfg->sv[i].prn, &cah[(size_t)i * 1023]);
    }
    DevBuf ca;
    HIP_TRY(ca.alloc(cah.size() * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(ca.p, cah.data(), cah.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(launch_synth_if(*cfg, ca.as<float>(), sample0, nsamples, static_cast<int8_t*>(dev_dst), ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return GNSS_OK;
}

}  // extern "C"
