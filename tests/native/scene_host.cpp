// scene_host.cpp -- csrc/synth_scene.h's functions (the per-sample arithmetic and the host loop
// that gnss_synth_scene_host and the kernel of gnss_synth_scene_device share) on hand-made paths,
// on the CPU: built once plainly and once under AddressSanitizer and UBSan
// (tests/test_native_scene.py). Every record is a heap buffer of exactly 2 * nsamples bytes and the
// tables are exactly as long as the header says, so a write past a record or a read past a table
// is an error there.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../assignment-for-aae6102_gnss-sdr_amd/csrc/synth_scene.h"

using namespace gnss;

static int mismatches = 0;
static int cases = 0;

static void check(bool ok, const char* what)
{
    cases++;
    if (!ok) {
        mismatches++;
        std::printf("MISMATCH %s\n", what);
    }
}

struct Tables {
    std::vector<int8_t> ca, lnav;
    SceneCodes codes() const { return SceneCodes{ca.data(), lnav.data()}; }
};

static Tables tables(int n_code)
{
    Tables t;
    t.ca.assign((size_t)n_code * kSceneCodePitch - 1, 0);  // (the last row ends with its last chip)
    t.lnav.assign(kSceneLnavBits, 0);
    uint64_t z = 1;
    for (int c = 0; c < n_code; c++)
        for (int i = 0; i < kSceneChips; i++) t.ca[(size_t)c * kSceneCodePitch + i] = (scene_mix64(z++) & 1) ? 1 : -1;
    for (int i = 0; i < kSceneLnavBits; i++) t.lnav[i] = (int8_t)(scene_mix64(z++) & 1);
    return t;
}

static ScenePath direct(int code, double amp, double code_phase0, int lnav)
{
    ScenePath p{};
    p.amp = amp;
    p.crate = 1.023e6 * (1.0 + 990.0 / 1575.42e6) / 58e6;
    p.frate = (4.58e6 + 990.0) / 58e6;
    p.code_phase0 = code_phase0;
    p.carr_phase0 = 0.3125;
    p.bit_phase = 1234.5;
    p.delay = 0;
    p.bit_seed = 0x1234567ULL + (uint64_t)code;
    p.t_on = 0;
    p.t_len = ~0ULL;
    p.code = code;
    p.lnav = lnav;
    return p;
}

static ScenePath ray_of(ScenePath p, double gain, double delay, double phase, uint64_t t_on, uint64_t t_off)
{
    p.amp *= gain;
    p.delay = delay;
    p.carr_phase0 += phase;
    p.frate = (4.58e6 + 990.0 + 3.0) / 58e6;
    p.t_on = t_on;
    p.t_len = t_off - t_on;
    return p;
}

static std::vector<int8_t> whole(const std::vector<ScenePath>& path, const Tables& t, double sigma, uint64_t s0,
                                 uint64_t n)
{
    std::vector<int8_t> r((size_t)(2 * n));
    scene_fill(path.data(), (int)path.size(), t.codes(), sigma, 6102, s0, n, r.data());
    return r;
}

// the range in chunks of `step` samples, each into a buffer of its own size
static std::vector<int8_t> chunked(const std::vector<ScenePath>& path, const Tables& t, double sigma, uint64_t s0,
                                   uint64_t n, uint64_t step)
{
    std::vector<int8_t> r;
    for (uint64_t lo = 0; lo < n; lo += step) {
        const uint64_t k = n - lo < step ? n - lo : step;
        std::vector<int8_t> part = whole(path, t, sigma, s0 + lo, k);
        r.insert(r.end(), part.begin(), part.end());
    }
    return r;
}

// the samples at which two records of n samples differ
static std::vector<uint64_t> differing(const std::vector<int8_t>& a, const std::vector<int8_t>& b)
{
    std::vector<uint64_t> d;
    for (size_t i = 0; i + 1 < a.size(); i += 2)
        if (a[i] != b[i] || a[i + 1] != b[i + 1]) d.push_back(i / 2);
    return d;
}

int main()
{
    const Tables t = tables(2);
    const uint64_t starts[2] = {0, 5300000123ULL};
    const uint64_t n = 3001;
    for (uint64_t s0 : starts) {
        // two SVs (one on the LNAV bits, one with a code phase below 0), three rays: over the
        // whole range (edges on its first and one past its last sample), on its first sample
        // only and on its last only
        std::vector<ScenePath> base = {direct(0, 9.0, -2040.2, 1), direct(1, 7.0, -0.3, 0)};
        std::vector<ScenePath> path = base;
        path.push_back(ray_of(base[0], 0.5, 0.5, 0.5, s0, s0 + n));
        path.push_back(ray_of(base[1], 14.0, 1.7, 0.25, s0, s0 + 1));
        path.push_back(ray_of(base[1], 14.0, 0.0, 0.0, s0 + n - 1, s0 + n));
        const std::vector<int8_t> w = whole(path, t, 12.0, s0, n);
        check(w.size() == 2 * n, "record size");
        check(chunked(path, t, 12.0, s0, n, 1) == w, "chunks of 1");
        check(chunked(path, t, 12.0, s0, n, 63) == w, "chunks of 63");
        check(chunked(path, t, 12.0, s0, n, 1777) == w, "chunks of 1777");
        check(chunked(path, t, 12.0, s0, n, n) == w, "one chunk");
        // the one-sample rays (amplitude 98 against noise of sigma 12) reach their sample only
        std::vector<ScenePath> no_ends(path.begin(), path.begin() + 3);
        const std::vector<uint64_t> d = differing(w, whole(no_ends, t, 12.0, s0, n));
        check(d.size() == 2 && d[0] == 0 && d[1] == n - 1, "rays on the first and the last sample");
        // a ray one sample before and one after the range changes nothing
        std::vector<ScenePath> outside = path;
        if (s0 > 0) outside.push_back(ray_of(base[1], 14.0, 0.2, 0.0, s0 - 1, s0));
        outside.push_back(ray_of(base[1], 14.0, 0.2, 0.0, s0 + n, s0 + n + 1));
        check(whole(outside, t, 12.0, s0, n) == w, "rays next to the range");
        // the whole-range ray is there: without it the record differs at many samples
        std::vector<ScenePath> no_ray = base;
        no_ray.push_back(path[3]);
        no_ray.push_back(path[4]);
        check(differing(w, whole(no_ray, t, 12.0, s0, n)).size() > n / 4, "the whole-range ray");
    }

    // no noise (sigma 0), one path: the sample is rint(amp * D * chip * (cos, sin)), here with D
    // from the LNAV table, restated; amplitude 300 clips at -128 and 127
    {
        const ScenePath p = ray_of(direct(1, 300.0, 100.25, 1), 1.0, 0.75, 0.125, 0, ~0ULL);
        int bad = 0, clipped = 0;
        for (uint64_t k = 0; k < 500; k++) {
            const uint64_t s = 977 * k;
            int8_t iq[2];
            scene_sample(&p, 1, t.codes(), 0.0, 6102, s, iq);
            const double th = (100.25 + (double)s * p.crate) - 0.75;
            const int chip = (int)((long long)std::floor(th) % 1023);
            const long long bit = (long long)std::floor((th + 1234.5) / 20460.0) % 3000;
            const double D = t.lnav[(size_t)bit] ? -1.0 : 1.0;
            double ph = (0.3125 + 0.125) - (double)s * p.frate;
            ph -= std::floor(ph);
            const double a = 300.0 * D * t.ca[(size_t)kSceneCodePitch + chip];
            double vi = std::rint(a * std::cos(kSceneTwoPi * ph)), vq = std::rint(a * std::sin(kSceneTwoPi * ph));
            vi = vi > 127 ? 127 : vi < -128 ? -128 : vi;
            vq = vq > 127 ? 127 : vq < -128 ? -128 : vq;
            if (iq[0] != (int8_t)vi || iq[1] != (int8_t)vq) bad++;
            if (std::fabs(vi) >= 127 || std::fabs(vq) >= 127) clipped++;
        }
        check(bad == 0, "a noise-free path against its formula");
        check(clipped > 100, "clipping was exercised");
    }

    // no path at all: noise only, and a null path array is not read
    {
        std::vector<int8_t> a((size_t)2 * 257), b = a;
        scene_fill(nullptr, 0, t.codes(), 12.0, 6102, 9, 257, a.data());
        const ScenePath off = ray_of(direct(0, 50.0, 0.0, 0), 1.0, 0.0, 0.0, 5, 9);  // ends where the range starts
        scene_fill(&off, 1, t.codes(), 12.0, 6102, 9, 257, b.data());
        check(a == b, "noise only");
        double sum = 0, sq = 0;
        for (int8_t v : a) sum += v, sq += (double)v * v;
        const double mean = sum / a.size(), var = sq / a.size() - mean * mean;
        check(std::fabs(mean) < 3.0 && var > 100.0 && var < 200.0, "the noise has sigma 12");
    }

    std::printf("cases %d, mismatches %d\n", cases, mismatches);
    return mismatches ? 1 : 0;
}
