// synth_scene.hip — the kernel of gnss_synth_scene_device: a multipath / NLOS scene as an int8
// I/Q record straight into HBM. The arithmetic of a sample is scene_sample (synth_scene.h), the
// same code as the host path. What this file adds is where the data lives:
//   - the paths (direct signals, then rays) are read at a loop index every lane shares from a
//     const __restrict__ kernel argument, so they come through scalar loads into SGPRs: nothing
//     per-SV or per-ray is read per lane (synth.hip loads a 64-byte struct per SV and sample);
//   - the C/A codes, one int8 chip per byte, and the LNAV bits are staged into LDS once per
//     block, 16 bytes per lane and step; a wave's 64 samples cover two or three chips, so its
//     chip reads are broadcasts;
//   - a ray's on/off test is a scalar pair against the lane's n; where no lane of a wave has the
//     ray, the wave branches over its sincos;
//   - a lane makes two neighbouring samples and stores them as one 4-byte word, a wave 256
//     contiguous bytes; a destination that is not 4-byte aligned and an odd count leave a first
//     and a last single sample, which a launch of two lanes makes (scene_singles_kernel, reading
//     the tables where they lie), so that the main kernel carries no code for them;
//   - up to kMaxBlocks blocks, each striding over the record with 64-bit indices, so the record
//     may pass 2^32 samples. 1 s of the 8-SV Opensky scene took 2.80 ms with 1024 blocks, 2.60
//     with 2048, 2.49 with 4096, 2.42 with 16 384 and 2.41 with 65 536: blocks
//     that end at different times fill the CUs better than a grid that is resident at once, and
//     staging 11 KB per block stays small beside the seven pair-iterations a block then makes.
#include <hip/hip_runtime.h>

#include "synth_scene.h"

namespace gnss {

namespace {

constexpr int kThreads = 256;
constexpr unsigned kMaxBlocks = 16384;

// NCODE: the code rows the block's LDS holds (the launcher takes the smallest that fits n_code)
template <int NCODE>
__global__ __launch_bounds__(kThreads) void scene_kernel(const ScenePath* __restrict__ path, int n_path,
                                                         const int8_t* __restrict__ tab, int n_code, double sigma,
                                                         uint64_t seed, uint64_t sample0, uint64_t nsamples, int head,
                                                         int8_t* __restrict__ dst)
{
    __shared__ __attribute__((aligned(16))) int8_t lds[NCODE * kSceneCodePitch + kSceneLnavPitch];
    const int words = (n_code * kSceneCodePitch + kSceneLnavPitch) / 16;  // n_code <= NCODE
    for (int w = threadIdx.x; w < words; w += kThreads)
        reinterpret_cast<uint4*>(lds)[w] = reinterpret_cast<const uint4*>(tab)[w];
    __syncthreads();
    const SceneCodes codes{lds, lds + n_code * kSceneCodePitch};

    // samples [head, head + 2 * npair) in pairs: dst + 2 * head is 4-byte aligned
    const uint64_t npair = (nsamples - (uint64_t)head) / 2;
    const uint64_t tid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    for (uint64_t p = tid; p < npair; p += (uint64_t)gridDim.x * kThreads) {
        const uint64_t i = (uint64_t)head + 2 * p;
        int8_t iq[4];
        scene_sample(path, n_path, codes, sigma, seed, sample0 + i, iq);
        scene_sample(path, n_path, codes, sigma, seed, sample0 + i + 1, iq + 2);
        char4 o;
        o.x = iq[0];
        o.y = iq[1];
        o.z = iq[2];
        o.w = iq[3];
        *reinterpret_cast<char4*>(dst + 2 * i) = o;
    }
}

// the single samples before and after the pairs: lane 0 the first (head), lane 1 the last
__global__ void scene_singles_kernel(const ScenePath* __restrict__ path, int n_path, const int8_t* __restrict__ tab,
                                     int n_code, double sigma, uint64_t seed, uint64_t sample0, uint64_t nsamples,
                                     int head, int8_t* __restrict__ dst)
{
    const SceneCodes codes{tab, tab + n_code * kSceneCodePitch};
    const uint64_t last = (uint64_t)head + 2 * ((nsamples - (uint64_t)head) / 2);
    if (threadIdx.x == 0 && head) scene_sample(path, n_path, codes, sigma, seed, sample0, dst);
    if (threadIdx.x == 1 && last < nsamples)
        scene_sample(path, n_path, codes, sigma, seed, sample0 + last, dst + 2 * last);
}

template <int NCODE>
void launch(uint64_t want, hipStream_t stream, const ScenePath* path, int n_path, const int8_t* tab, int n_code,
            double sigma, uint64_t seed, uint64_t sample0, uint64_t nsamples, int head, int8_t* dst)
{
    const dim3 grid((unsigned)(want < kMaxBlocks ? want : kMaxBlocks));
    hipLaunchKernelGGL((scene_kernel<NCODE>), grid, dim3(kThreads), 0, stream, path, n_path, tab, n_code, sigma, seed,
                       sample0, nsamples, head, dst);
}

}  // namespace

int scene_launch(const ScenePath* path, int n_path, const int8_t* tab, int n_code, double sigma, uint64_t seed,
                 uint64_t sample0, uint64_t nsamples, int8_t* dst, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (nsamples == 0) return 0;
    if (n_code < 1 || n_code > 64 || n_path < 0 || n_path > kSceneMaxPaths) return (int)hipErrorInvalidValue;
    const int head = (reinterpret_cast<uintptr_t>(dst) & 2) ? 1 : 0;  // (nsamples >= 1)
    const uint64_t npair = (nsamples - (uint64_t)head) / 2;
    const uint64_t want = (npair + kThreads - 1) / kThreads;
    if (head || (nsamples - (uint64_t)head) % 2)
        hipLaunchKernelGGL(scene_singles_kernel, dim3(1), dim3(64), 0, stream, path, n_path, tab, n_code, sigma, seed,
                           sample0, nsamples, head, dst);
    if (want == 0) return (int)hipGetLastError();
    if (n_code <= 8)
        launch<8>(want, stream, path, n_path, tab, n_code, sigma, seed, sample0, nsamples, head, dst);
    else if (n_code <= 16)
        launch<16>(want, stream, path, n_path, tab, n_code, sigma, seed, sample0, nsamples, head, dst);
    else if (n_code <= 32)
        launch<32>(want, stream, path, n_path, tab, n_code, sigma, seed, sample0, nsamples, head, dst);
    else
        launch<64>(want, stream, path, n_path, tab, n_code, sigma, seed, sample0, nsamples, head, dst);
    return (int)hipGetLastError();
}

}  // namespace gnss
