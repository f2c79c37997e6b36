// host.h -- what the host translation units of the C-ABI share (ctx.cpp, api_acq.cpp,
// api_track.cpp, api_vt.cpp, ctpos.cpp): the context, error reporting, RAII device / pinned
// buffers, IF staging, the rocFFT plan cache and the C/A codes. Host only: no .hip includes it.
#pragma once

#include <hip/hip_runtime.h>
#include <rocfft/rocfft.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <string>
#include <thread>
#include <tuple>
#include <utility>
#include <vector>

#include "gnss_internal.h"
#include "group.h"

struct gnss_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;       // the acquisition's row passes beside the column passes
    hipEvent_t ev_cols[2] = {}, ev_rows[2] = {};  // their hand-offs, per intermediate buffer
    std::string err;
    gnss_timing timing{};
    int profiling = 0;
    std::map<std::tuple<size_t, size_t, int, int>, rocfft_plan> plans;
    void* fft_work = nullptr;
    size_t fft_work_size = 0;
    // device scratch kept across calls (hipMalloc/hipFree per call cost ~1 ms and hipFree
    // synchronises): name -> (pointer, bytes)
    std::map<std::string, std::pair<void*, size_t>> pool;
    // pinned host staging kept across calls (the per-step records' download): name ->
    // (pointer, bytes); a pageable std::vector re-faults and bounces every call
    std::map<std::string, std::pair<void*, size_t>> pinned;
    int64_t acq_tw_S = 0;  // the acquisition twiddle tables in the pool are for this S
    int acq_tw_dbl = -1;   //   ... and this precision
    int acq_fp64 = 1;      // acquisition correlation precision: 1 = fp64 (reference), 0 = fp32
    uint64_t window = 0;   // trackingCT: max IF bytes resident in HBM (0: the whole read range)
    int64_t opt[GNSS_OPT_COUNT] = {};  // gnss_ctx_set_option (test hooks; all 0 by default)
    int lane_path = 0;                 // gnss_ctx_lane_path
    // multi-device context (gnss_ctx_create_multi): the member contexts (empty: a plain one);
    // the group itself is also a context on devices[0], for the entry points that do not shard
    std::vector<gnss_ctx*> members;
    bool member = false;  // a group's member: dev_data on another device is copied in (xGMI)
    int fail_chan = -1;   // tracking: the channel whose status the last call returned (group.h)
    // (a member) its resident copies of dev_data records on another device: one peer copy per
    // record, kept across calls (group.h ResidentCache; the copy is a hipMalloc of this device)
    gnss::group::ResidentCache<void*> resident;
};

namespace gnss {
struct AcfDev;      // acf.h
struct AcfExtPlan;  // acf_ext.h
namespace host {

// Timing-probe hooks read from the environment in probe builds only (tools/build_probe.sh
// passes -DGNSS_PROBE_BUILD=1 to every host file); the product library reads no environment
// variable.
inline const char* probe_env(const char* name)
{
    return GNSS_PROBE_BUILD ? getenv(name) : nullptr;
}

// steps of gnss_tracking_vt per staged IF window of a host record (GNSS_OPT_VT_SPAN: fewer)
constexpr int kVtSpan = 2000;

int fail(gnss_ctx* ctx, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));

#define HIP_TRY(expr)                                                                         \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return ::gnss::host::fail(ctx, GNSS_EDEVICE, "%s:%d %s: %s", __FILE__, __LINE__,   \
                                      #expr, hipGetErrorString(e_));                           \
    } while (0)

// The context's pinned host buffer `key`, at least `bytes` (contents undefined).
// (`flags`: hipHostMalloc's; a key is always asked for with the same flags)
template <class T>
T* pinned_buffer(gnss_ctx* ctx, const char* key, size_t count, unsigned flags = hipHostMallocDefault)
{
    auto& e = ctx->pinned[key];
    const size_t want = std::max<size_t>(count * sizeof(T), 16);
    if (e.second < want) {
        if (e.first) (void)hipHostFree(e.first);
        e = {nullptr, 0};
        if (hipHostMalloc(&e.first, want, flags) != hipSuccess) return nullptr;
        e.second = want;
    }
    return static_cast<T*>(e.first);
}

// RAII device buffer
struct DevBuf {
    void* p = nullptr;
    size_t n = 0;
    bool pooled = false;  // borrowed from the context's pool: not freed here
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release()
    {
        if (p && !pooled) (void)hipFree(p);
        p = nullptr;
        pooled = false;
    }
    hipError_t alloc(size_t bytes)
    {
        release();
        n = bytes;
        return hipMalloc(&p, bytes ? bytes : 16);
    }
    // The context's buffer `key` (grown when too small; contents undefined, as hipMalloc).
    // One key per live buffer; calls on a context are serialised on its stream.
    hipError_t alloc(gnss_ctx* ctx, const char* key, size_t bytes)
    {
        release();
        auto& e = ctx->pool[key];
        const size_t want = bytes ? bytes : 16;
        if (e.second < want) {
            if (e.first) (void)hipFree(e.first);
            e = {nullptr, 0};
            const hipError_t r = hipMalloc(&e.first, want);
            if (r != hipSuccess) {
                e.first = nullptr;
                return r;
            }
            e.second = want;
        }
        p = e.first;
        n = bytes;
        pooled = true;
        return hipSuccess;
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// f(0..n-1) over up to 16 host threads (the output expansion writes tens of MB into
// fresh pages; one thread is bound by page faults and a single core's bandwidth).
template <class F>
void parallel_for(int n, F f)
{
    const int nt = std::max(1, std::min({n, 16, (int)std::thread::hardware_concurrency()}));
    if (nt <= 1) {
        for (int i = 0; i < n; i++) f(i);
        return;
    }
    std::vector<std::thread> th;
    th.reserve((size_t)nt);
    for (int t = 0; t < nt; t++)
        th.emplace_back([&, t]() {
            for (int i = t; i < n; i += nt) f(i);
        });
    for (auto& x : th) x.join();
}

struct Events {
    hipEvent_t a = nullptr, b = nullptr;
    Events() { (void)hipEventCreate(&a); (void)hipEventCreate(&b); }
    ~Events() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); }
    double ms() const { float f = 0; (void)hipEventElapsedTime(&f, a, b); return f; }
};

int64_t file_length(const gnss_file* f);

// The IF bytes [lo, hi) resident in HBM; base = file byte at ptr[0] (16-B aligned).
struct IfWindow {
    DevBuf own;
    const int8_t* ptr = nullptr;
    int64_t base = 0, len = 0;
};

// (ctx.cpp) the file bytes [lo, hi) into device memory dst, through the pinned double buffer
int stage_into(gnss_ctx* ctx, const gnss_file* f, int64_t lo, int64_t hi, int8_t* dst);
// (ctx.cpp) the IF bytes [lo, hi) resident in HBM: a caller-resident record as is (a group
// member: its peer copy), a host record or file staged into w.own
int stage_window(gnss_ctx* ctx, const gnss_file* f, int64_t lo, int64_t hi, IfWindow& w);
// The HIP device a device pointer belongs to (-1 if HIP does not know it).
int pointer_device(const void* p);
// [p, p + bytes) is device memory of `device` inside one allocation, as HIP knows it (a host
// pointer, registered or not, is not: the kernels would read it as a device address)
inline bool device_memory_of(const void* p, size_t bytes, int device)
{
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    if (a.type != hipMemoryTypeDevice || a.device != device || a.devicePointer == nullptr) return false;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    const char* lo = static_cast<const char*>(base);
    const char* q = static_cast<const char*>(p);
    return q >= lo && bytes <= size && (size_t)(q - lo) <= size - bytes;
}

// drops the resident copies of every member of ctx that overlap [p, p + n) (n == 0: the records
// containing p; p == nullptr: all of them); returns how many were dropped
int drop_resident(gnss_ctx* ctx, const void* p, uint64_t n);

// (ctx.cpp) the context's rocFFT plans, kept per (length, batch, precision, direction)
int get_plan(gnss_ctx* ctx, size_t len, size_t batch, int dbl, int inverse, rocfft_plan* out);
int run_fft(gnss_ctx* ctx, void* data, size_t len, size_t batch, int dbl, int inverse);

// The kernels form CarrTime = k/Fs (trackingCT.m:104) as q = k*RN(1/Fs) corrected by
// one FMA; that equals the IEEE quotient for every k we check here (exhaustive over
// the step's sample range, cached per Fs). Otherwise they divide.
inline int fast_div_exact(double Fs, int64_t kmax) { return group::reciprocal_exact_cached(Fs, kmax); }

// generateCAcode.m:16-64 as 1023 chips of +-1, and as 32 words of bits (bit i set <-> chip i
// is -1), read by the kernels through lane shuffles
void generate_ca(int prn, float* out);
void ca_bits(int prn, unsigned* out32);

// The sampling-rate floor of the tracking kernels (api_track.cpp)
bool lane_rate_admitted(const gnss_signal* sg, double codeFreq_max);
int refuse_lane_rate(gnss_ctx* ctx, const gnss_signal* sg, double codeFreq_max);

// (acf.cpp) gnss_acf_features' pass. ext == nullptr: that call as it is; otherwise the pass of
// gnss_acf_features_ext (acf_ext.cpp, which checked *ext): the row pass also counts the local
// maxima and the windows' F6-F8 go to ext's arrays, `out` being the same bits either way.
int acf_features_run(gnss_ctx* ctx, const gnss_acf_cfg* cfg, const gnss_track_out* rec, int32_t n_taps,
                     gnss_acf_out* out, const AcfExtPlan* ext);
// (acf_ext.cpp) the host path's F6-F8 of channel c: cnt [len] the rows' counts, meanMax the
// channel's `windows` values, the outputs at [c * cap + m]
void acf_ext_host_channel(const AcfExtPlan& p, int c, int64_t cap, int64_t windows, int64_t ind_start,
                          int64_t numOverLap, const uint8_t* cnt, const double* meanMax);
// (acf_ext.cpp) the device path's: after acf_launch on ctx->stream with d.cnt set, the table's
// upload, acf_spectrum_kernel, the download and the stores at [c * cap + m]; synchronises the stream
int acf_ext_device(gnss_ctx* ctx, const AcfExtPlan& p, const AcfDev& d, int64_t cap);

// Multi-device contexts (gnss_ctx_create_multi): the group's member contexts run their shards
// side by side, one host thread per device (group.h has the dealing and merging).
template <class F>
void for_members(gnss_ctx* g, F fn)
{
    std::vector<int> devs;
    for (gnss_ctx* m : g->members) devs.push_back(m->device);
    std::vector<std::thread> th;
    for (const std::vector<int>& ks : group::by_device(devs))
        th.emplace_back([&fn, ks]() {
            for (int k : ks) fn(k);
        });
    for (auto& t : th) t.join();
}

}  // namespace host
}  // namespace gnss
