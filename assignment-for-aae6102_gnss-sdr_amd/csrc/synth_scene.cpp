// synth_scene.cpp — gnss_synth_scene_host and gnss_synth_scene_device (the definitions and the
// model are in include/gnss_mi355x.h, the per-sample arithmetic in synth_scene.h): the argument
// checks, the scene flattened into paths, the code table, the host loop over CPU threads and, for
// the device, the upload of paths and table and the launch of synth_scene.hip. Built with
// -ffp-contract=off: every operation rounds on its own.
#include <cmath>
#include <cstring>

#include "host.h"
#include "synth_scene.h"

using namespace gnss;
using namespace gnss::host;

static_assert(kSceneMaxPaths == GNSS_MAX_SV + GNSS_MAX_RAYS, "synth_scene.h restates the header's sizes");

namespace {

const char* scene_refusal(const gnss_synth_scene* sc)
{
    if (!sc) return "a null scene";
    if (sc->n_sv < 0 || sc->n_sv > GNSS_MAX_SV) return "n_sv outside 0..GNSS_MAX_SV";
    if (sc->n_ray < 0 || sc->n_ray > GNSS_MAX_RAYS) return "n_ray outside 0..GNSS_MAX_RAYS";
    for (int s = 0; s < sc->n_sv; s++) {
        if (sc->sv[s].prn < 1 || sc->sv[s].prn > 51) return "a PRN outside 1..51";
        if (!std::isfinite(sc->los_gain[s]) || sc->los_gain[s] < 0) return "a negative or non-finite los_gain";
    }
    for (int r = 0; r < sc->n_ray; r++) {
        const gnss_synth_ray& y = sc->ray[r];
        if (y.sv < 0 || y.sv >= sc->n_sv) return "a ray's sv outside 0..n_sv-1";
        if (!std::isfinite(y.delay_chips) || y.delay_chips < 0) return "a negative or non-finite delay_chips";
        if (!std::isfinite(y.gain) || y.gain < 0) return "a negative or non-finite gain";
        if (!std::isfinite(y.phase0_cycles) || !std::isfinite(y.fade_hz)) return "a non-finite phase0_cycles or fade_hz";
        if (y.t_off < y.t_on) return "a ray with t_off < t_on";
    }
    return nullptr;
}

// A checked scene as paths and tables. A path of amplitude 0 (an NLOS SV's direct signal, a ray
// of gain 0) is left out: its term is +-0 and leaves both sums as they are.
struct Packed {
    std::vector<ScenePath> path;
    std::vector<int8_t> tab;  // n_sv code rows, then the LNAV bits
    size_t lnav_at = 0;
};

void pack(const gnss_synth_scene& sc, Packed& k)
{
    const double fL1 = 1575.42e6, fc = 1.023e6;
    double amp[GNSS_MAX_SV];
    auto of_sv = [&](int s) {
        const gnss_synth_sv& v = sc.sv[s];
        ScenePath p{};
        p.crate = fc * (1.0 + v.doppler_hz / fL1) / sc.Fs;
        p.frate = (sc.IF + v.doppler_hz) / sc.Fs;
        p.code_phase0 = v.code_phase0;
        p.carr_phase0 = v.carr_phase0;
        p.bit_phase = v.bit_phase_chips;
        p.bit_seed = v.bit_seed;
        p.t_on = 0;
        p.t_len = ~0ULL;
        p.code = s;
        p.lnav = v.lnav;
        return p;
    };
    for (int s = 0; s < sc.n_sv; s++) {
        const double snr_lin = pow(10.0, sc.sv[s].cn0_dbhz / 10.0);
        amp[s] = sqrt(2.0 * sc.noise_sigma * sc.noise_sigma * snr_lin / sc.Fs);
        ScenePath p = of_sv(s);
        p.amp = amp[s] * sc.los_gain[s];
        if (p.amp != 0) k.path.push_back(p);
    }
    for (int r = 0; r < sc.n_ray; r++) {
        const gnss_synth_ray& y = sc.ray[r];
        ScenePath p = of_sv(y.sv);
        p.amp = amp[y.sv] * y.gain;
        p.frate = (sc.IF + sc.sv[y.sv].doppler_hz + y.fade_hz) / sc.Fs;
        p.carr_phase0 = sc.sv[y.sv].carr_phase0 + y.phase0_cycles;
        p.delay = y.delay_chips;
        p.t_on = y.t_on;
        p.t_len = y.t_off - y.t_on;
        if (p.amp != 0 && p.t_len != 0) k.path.push_back(p);
    }
    k.lnav_at = (size_t)std::max(1, sc.n_sv) * kSceneCodePitch;
    k.tab.assign(k.lnav_at + kSceneLnavPitch, 0);
    float f[kSceneChips];
    for (int s = 0; s < sc.n_sv; s++) {
        generate_ca(sc.sv[s].prn, f);
        for (int i = 0; i < kSceneChips; i++) k.tab[(size_t)s * kSceneCodePitch + i] = (int8_t)f[i];
    }
    (void)gnss_lnav_bits(1, kSceneLnavBits, k.tab.data() + k.lnav_at);  // (the same message on every SV)
}

}  // namespace

extern "C" {

int gnss_synth_scene_host(const gnss_synth_scene* scene, uint64_t sample0, uint64_t nsamples, void* dst,
                          int nthreads)
{
    if (scene_refusal(scene) || (!dst && nsamples) || nthreads < 0) return GNSS_EARG;
    Packed k;
    pack(*scene, k);
    const SceneCodes codes{k.tab.data(), k.tab.data() + k.lnav_at};
    // whole blocks of 4096 samples dealt over the threads
    const uint64_t block = 4096, nblock = (nsamples + block - 1) / block;
    const int cap = nthreads > 0 ? nthreads : std::min(16, std::max(1, (int)std::thread::hardware_concurrency()));
    const int nt = (int)std::min<uint64_t>((uint64_t)cap, std::max<uint64_t>(nblock, 1));
    auto work = [&](int t) {
        for (uint64_t b = (uint64_t)t; b < nblock; b += (uint64_t)nt) {
            const uint64_t lo = b * block, n = std::min(block, nsamples - lo);
            scene_fill(k.path.data(), (int)k.path.size(), codes, scene->noise_sigma, scene->seed, sample0 + lo, n,
                       static_cast<int8_t*>(dst) + 2 * lo);
        }
    };
    if (nt <= 1) {
        work(0);
        return GNSS_OK;
    }
    std::vector<std::thread> th;
    th.reserve((size_t)nt);
    for (int t = 0; t < nt; t++) th.emplace_back(work, t);
    for (auto& x : th) x.join();
    return GNSS_OK;
}

int gnss_synth_scene_device(gnss_ctx* ctx, const gnss_synth_scene* scene, uint64_t sample0, uint64_t nsamples,
                            void* dev_dst)
{
    if (!ctx) return GNSS_EARG;
    if (const char* why = scene_refusal(scene)) return fail(ctx, GNSS_EARG, "gnss_synth_scene_device: %s", why);
    if (!dev_dst) return fail(ctx, GNSS_EARG, "gnss_synth_scene_device: a null destination");
    drop_resident(ctx, dev_dst, 2 * nsamples);  // (int8 I/Q: a member's copy of these bytes is stale now)
    HIP_TRY(hipSetDevice(ctx->device));
    if (nsamples == 0) return GNSS_OK;
    Packed k;
    pack(*scene, k);
    // paths and table in one pooled buffer; the stream is drained before this call returns, so
    // the pageable sources outlive their copies
    const size_t path_bytes = sizeof(ScenePath) * kSceneMaxPaths;
    DevBuf buf;
    HIP_TRY(buf.alloc(ctx, "synth_scene", path_bytes + (size_t)GNSS_MAX_SV * kSceneCodePitch + kSceneLnavPitch));
    if (!k.path.empty())
        HIP_TRY(hipMemcpyAsync(buf.p, k.path.data(), sizeof(ScenePath) * k.path.size(), hipMemcpyHostToDevice,
                               ctx->stream));
    int8_t* tab = buf.as<int8_t>() + path_bytes;
    HIP_TRY(hipMemcpyAsync(tab, k.tab.data(), k.tab.size(), hipMemcpyHostToDevice, ctx->stream));
    const int le = scene_launch(buf.as<ScenePath>(), (int)k.path.size(), tab, std::max(1, scene->n_sv),
                                scene->noise_sigma, scene->seed, sample0, nsamples, static_cast<int8_t*>(dev_dst),
                                ctx->stream);
    if (le)
        return fail(ctx, GNSS_EDEVICE, "gnss_synth_scene_device: kernel launch: %s",
                    hipGetErrorString((hipError_t)le));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return GNSS_OK;
}

}  // extern "C"
