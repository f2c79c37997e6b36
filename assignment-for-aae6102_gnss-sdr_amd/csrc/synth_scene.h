// synth_scene.h — one sample of a multipath / NLOS scene (gnss_synth_scene; the model, with its
// simplification, is in include/gnss_mi355x.h). A scene is flattened on the host into paths
// (synth_scene.cpp): first every SV's direct signal in SV order, then the rays in array order. A
// direct signal is the path with delay 0, the SV's own carrier and no on/off time, which makes
// its operations those of synth.hip (th - 0.0 is th, carr_phase0 + 0.0 is carr_phase0): a ray-less
// scene gives that generator's bytes.
// One source for the arithmetic, called per sample by the host loop (scene_fill, below) and by
// the kernel (synth_scene.hip), compiled without contraction and without fast-math on both sides.
// The device takes sin and cos from sincos(), the host from libm's sin() and cos(): they differ
// in the last place at most, which reaches a byte only where the value before rint() lies within
// about 1e-14 of a half-integer. No HIP include and no project include:
// tests/native/scene_host.cpp calls these functions on the CPU under AddressSanitizer and UBSan.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define GNSS_SCENE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define GNSS_SCENE_HD inline
#endif

namespace gnss {

constexpr int kSceneChips = 1023;
constexpr int kSceneCodePitch = 1024;  // bytes between two codes of a table (16-byte rows)
constexpr int kSceneLnavBits = 3000;   // two LNAV frames (60 s), repeated
constexpr int kSceneLnavPitch = 3008;  // ... padded to 16 bytes
constexpr int kSceneMaxPaths = 64 + 128;  // = GNSS_MAX_SV + GNSS_MAX_RAYS
constexpr double kSceneTwoPi = 2.0 * 3.14159265358979323846;

// A direct signal or a ray, everything per-sample work needs in one place (88 bytes; the same
// for every lane of a wave, so the kernel reads it with scalar loads).
struct ScenePath {
    double amp;          // amp_s * los_gain, or amp_s * gain
    double crate;        // chips per sample
    double frate;        // carrier cycles per sample: (IF + fd [+ fade_hz]) / Fs
    double code_phase0;  // the SV's, chips at sample 0
    double carr_phase0;  // the SV's [+ phase0_cycles], cycles at sample 0
    double bit_phase;    // the SV's bit_phase_chips
    double delay;        // chips; 0 for a direct signal
    uint64_t bit_seed;
    uint64_t t_on;       // present for n - t_on < t_len in uint64 arithmetic, which is
    uint64_t t_len;      //   t_on <= n < t_off; a direct signal: 0 and 2^64 - 1
    int32_t code;        // row of the code table
    int32_t lnav;
};

// The codes, one int8 chip (+-1) per byte in rows of kSceneCodePitch, and the LNAV bits (0/1).
// Host memory on the host, LDS in the kernel.
struct SceneCodes {
    const int8_t* ca;
    const int8_t* lnav;
};

GNSS_SCENE_HD uint64_t scene_mix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

GNSS_SCENE_HD void scene_sincos(double x, double* sn, double* cs)
{
#if defined(__HIP_DEVICE_COMPILE__)
    sincos(x, sn, cs);
#else
    *sn = sin(x);
    *cs = cos(x);
#endif
}

// Sample n of the record into iq[0] (I) and iq[1] (Q). A path that is off costs its on/off test
// only.
GNSS_SCENE_HD void scene_sample(const ScenePath* __restrict__ path, int n_path, const SceneCodes& codes, double sigma,
                                uint64_t seed, uint64_t n, int8_t* iq)
{
    double re = 0, im = 0;
    for (int p = 0; p < n_path; p++) {
        const ScenePath& v = path[p];
        if (n - v.t_on >= v.t_len) continue;
        const double th = (v.code_phase0 + (double)n * v.crate) - v.delay;
        int64_t chip = (int64_t)floor(th) % kSceneChips;
        if (chip < 0) chip += kSceneChips;
        const double bitf = floor((th + v.bit_phase) / 20460.0);
        double D;
        if (v.lnav) {  // LNAV bit b -> (-1)^b (gnss_lnav_bits, kSceneLnavBits-bit cycle)
            int64_t k = (int64_t)bitf % kSceneLnavBits;
            if (k < 0) k += kSceneLnavBits;
            D = codes.lnav[k] ? -1.0 : 1.0;
        } else {
            const uint64_t bh = scene_mix64(v.bit_seed ^ (uint64_t)(int64_t)bitf);
            D = (bh & 1) ? 1.0 : -1.0;
        }
        double ph = v.carr_phase0 - (double)n * v.frate;
        ph -= floor(ph);
        const double a = v.amp * D * (double)codes.ca[v.code * kSceneCodePitch + (int)chip];
        double sn, cs;
        scene_sincos(kSceneTwoPi * ph, &sn, &cs);
        re += a * cs;
        im += a * sn;
    }
    const uint64_t h1 = scene_mix64(seed ^ (n * 0xD1B54A32D192ED03ULL));
    const uint64_t h2 = scene_mix64(h1 ^ 0x8CB92BA72F3D8DD7ULL);
    const double u1 = ((double)(h1 >> 11) + 1.0) * (1.0 / 9007199254740992.0);
    const double u2 = (double)(h2 >> 11) * (1.0 / 9007199254740992.0);
    const double r = sqrt(-2.0 * log(u1)) * sigma;
    double sn, cs;
    scene_sincos(kSceneTwoPi * u2, &sn, &cs);
    double vi = rint(re + r * cs), vq = rint(im + r * sn);
    vi = fmin(127.0, fmax(-128.0, vi));
    vq = fmin(127.0, fmax(-128.0, vq));
    iq[0] = (int8_t)vi;
    iq[1] = (int8_t)vq;
}

// Samples [sample0, sample0 + nsamples) into dst, 2 * nsamples bytes (the host path's loop).
inline void scene_fill(const ScenePath* path, int n_path, const SceneCodes& codes, double sigma, uint64_t seed,
                       uint64_t sample0, uint64_t nsamples, int8_t* dst)
{
    for (uint64_t i = 0; i < nsamples; i++) scene_sample(path, n_path, codes, sigma, seed, sample0 + i, dst + 2 * i);
}

// The launch on `stream` (a hipStream_t) of the current device (synth_scene.hip). path: n_path
// paths in device memory; tab: n_code code rows, then the LNAV bits at n_code * kSceneCodePitch,
// device memory, 16-byte aligned. Returns the hipError_t of the launch (0: none).
int scene_launch(const ScenePath* path, int n_path, const int8_t* tab, int n_code, double sigma, uint64_t seed,
                 uint64_t sample0, uint64_t nsamples, int8_t* dst, void* stream);

}  // namespace gnss
