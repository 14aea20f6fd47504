// tracer.hip -- CWavefrontPathTracer on MI355X: pool allocation, scene upload,
// the per-iteration launch sequence (captured into a hipGraph), image
// completion, film accumulation, and the extern "C" tracer API of dcrt.h.
// Reference: Source/WavefrontPathTracer.cpp:70-1162, Source/Scene.cpp:273-608,
// Source/SampleConvolution.cpp:89-170, Source/BxDFTexturesBuilding.cpp:106-475.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <limits>
#include <vector>

#include "../../../include/dcrt.h"
#include "../host/bvh_layout.h"
#include "../host/film_rows.h"
#include "kernels_impl.h"

namespace dcrt {
void SetLastError(const std::string& s);
int CheckFilterParams(const dcrt_filter_params& f);   // (capi_scene.cpp: the one rule for scene and tracer)
}
using dcrt::FilterSupportRows;
using dcrt::SetLastError;
using dcrt::ShadowCells;
using namespace dcrt::dev;

#define HIPCHECK(expr)                                                                              \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            SetLastError(std::string(#expr) + " failed: " + hipGetErrorString(e_));                 \
            return DCRT_E_HIP;                                                                      \
        }                                                                                           \
    } while (0)
#define CHECKED(expr)                      \
    do {                                   \
        const int r_ = (expr);             \
        if (r_ != DCRT_OK) return r_;      \
    } while (0)

namespace {

constexpr uint32_t kDefaultPoolSize = 1u << 20;      // 2^20 slots: 16 waves x 256 CUs x 256 (MI355X)
constexpr uint32_t kDefaultIterations = 8;
// RenderImages' chunks of iterations once its final batch is in flight: a chunk launched after
// the images completed finds no work, and two chunks are in flight when the host sees it
constexpr uint32_t kTailChunk = 4;
constexpr uint32_t kMaxImageBatch = 256;              // images in flight per RenderImages batch (sample textures: 24 B/px each)
#ifndef DCRT_MATERIAL_BLOCK
#define DCRT_MATERIAL_BLOCK 256
#endif
constexpr uint32_t kMaterialBlock = DCRT_MATERIAL_BLOCK;   // MATERIAL workgroup (one queue-append atomic each)
constexpr uint32_t kMaxPersistentBlocks = 256 * 8;   // CUs x resident workgroups

// (A/B knobs of AutoBatch)
uint32_t kMaxImageBatchAuto()
{
    static const uint32_t v = [] {
        const char* e = std::getenv("DCRT_MAX_BATCH");
        const int x = e ? std::atoi(e) : (int)kMaxImageBatch;
        return (uint32_t)std::min<int>(std::max<int>(x, 1), (int)kMaxImageBatch);
    }();
    return v;
}
bool BatchPoolLimit()
{
    static const bool v = [] { const char* e = std::getenv("DCRT_BATCH_POOL_LIMIT"); return !e || std::atoi(e) != 0; }();
    return v;
}

// The owner of a set of device allocations: a tracer's buffers that live and die together, or a
// function's temporaries (a local group frees them on every return path; hipFree waits for the device).
class DeviceGroup {
public:
    DeviceGroup() = default;
    DeviceGroup(const DeviceGroup&) = delete;
    DeviceGroup& operator=(const DeviceGroup&) = delete;
    ~DeviceGroup() { Free(); }
    template <typename T>
    int Alloc(T** p, size_t count)
    {
        *p = nullptr;
        if (count == 0) count = 1;
        void* q = nullptr;
        HIPCHECK(hipMalloc(&q, count * sizeof(T)));
        *p = (T*)q;
        ptrs.push_back(q);
        return DCRT_OK;
    }
    void Free()
    {
        for (void* p : ptrs) (void)hipFree(p);
        ptrs.clear();
    }

private:
    std::vector<void*> ptrs;
};

// Pinned host staging for one T or T[N]: what a device-to-host copy of a few words lands in before the
// stream is synchronised. Allocated once (Alloc: again is free), freed with its owner.
template <typename T, size_t N = 1>
class Pinned {
public:
    Pinned() = default;
    Pinned(const Pinned&) = delete;
    Pinned& operator=(const Pinned&) = delete;
    ~Pinned()
    {
        if (p) (void)hipHostFree(p);
    }
    int Alloc()
    {
        if (!p) HIPCHECK(hipHostMalloc((void**)&p, N * sizeof(T), hipHostMallocDefault));
        return DCRT_OK;
    }
    T* get() const { return p; }
    T& operator[](size_t i) const { return p[i]; }

private:
    T* p = nullptr;
};

// Events recorded between the kernels of one stage (ext_timing): mark i stands in front of kernel i, so
// kernel i took ElapsedBetween(i, i + 1). The events are created on first use and kept.
class EventMarks {
public:
    EventMarks() = default;
    EventMarks(const EventMarks&) = delete;
    EventMarks& operator=(const EventMarks&) = delete;
    ~EventMarks()
    {
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
    }
    void Reset() { used = 0; }
    uint32_t Count() const { return used; }
    int Mark(hipStream_t stream)
    {
        if (events.size() <= used) {
            hipEvent_t e;
            HIPCHECK(hipEventCreate(&e));
            events.push_back(e);
        }
        HIPCHECK(hipEventRecord(events[used++], stream));
        return DCRT_OK;
    }
    int ElapsedBetween(uint32_t i, uint32_t j, float* ms) const
    {
        HIPCHECK(hipEventElapsedTime(ms, events[i], events[j]));
        return DCRT_OK;
    }

private:
    std::vector<hipEvent_t> events;
    uint32_t used = 0;
};

FilterConsts MakeFilter(const dcrt_filter_params& p)   // SampleConvolution.cpp:100-130
{
    FilterConsts c;
    std::memset(&c, 0, sizeof(c));
    c.kind = p.filter;
    c.radius = p.radius;
    if (p.filter == DCRT_FILTER_GAUSSIAN) {
        c.gaussianAlpha = p.gaussian_alpha;
        c.gaussianExp = std::exp(-p.gaussian_alpha * p.radius * p.radius);
    } else if (p.filter == DCRT_FILTER_MITCHELL) {
        const float B = p.mitchell_b, C = p.mitchell_c;
        c.mf[0] = -B - 6 * C; c.mf[1] = 6 * B + 30 * C; c.mf[2] = -12 * B - 48 * C; c.mf[3] = 8 * B + 24 * C;
        c.mf[4] = 12 - 9 * B - 6 * C; c.mf[5] = -18 + 12 * B + 6 * C; c.mf[6] = 6 - 2 * B;
    } else if (p.filter == DCRT_FILTER_LANCZOS) {
        c.tau = p.lanczos_tau ? p.lanczos_tau : 3;
    }
    return c;
}

// roctx ranges around the host-side passes, named like the reference's PIX annotations
// (SCOPED_RENDER_ANNOTATION, WavefrontPathTracer.cpp:443-1083): visible in rocprofv3
// --marker-trace next to the kernels. rocprofiler-sdk's roctx (the one rocprofv3 intercepts;
// the legacy libroctx64 as a fallback) is opened at run time (no link dependency; absent, or
// DCRT_ROCTX=0: no ranges). Iterations captured into a hipGraph are annotated by
// their replay ("RenderImages" / graph chunks), not per kernel.
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx()
    {
        if (const char* e = std::getenv("DCRT_ROCTX")) {
            if (std::atoi(e) == 0) return;
        }
        void* h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
        pop = (int (*)())dlsym(h, "roctxRangePop");
        if (!push || !pop) push = nullptr, pop = nullptr;
    }
};
const Roctx& roctx()
{
    static const Roctx r;
    return r;
}
struct Annotation {
    bool on;
    explicit Annotation(const char* name, bool enabled = true) : on(enabled && roctx().push)
    {
        if (on) roctx().push(name);
    }
    ~Annotation()
    {
        if (on) roctx().pop();
    }
};

// ---- The three stages that work on any W x H device images once the samples exist. Each owns its device
// scratch, its pinned staging and its event marks, takes the stream (and whether ext_timing is on) per call,
// and knows nothing of the tracer that holds it.
// The filter of dcrt.h "film denoiser"
class FilmDenoiser {
public:
    int Run(hipStream_t stream, bool timing, const dcrt_denoise_params& p, uint32_t w, uint32_t h, const float4* color, const float4* normal,
            const float4* albedo, float4* out);
    // ms per kernel of the last Run that was timed (prologue, variance, passes): at most `capacity` of *outCount
    int Timings(float* outMs, uint32_t capacity, uint32_t* outCount) const;

private:
    int EnsureWork(hipStream_t stream, uint32_t w, uint32_t h);
    DeviceGroup allocs;
    float4* work[2] = { nullptr, nullptr };   // (c.rgb, var), ping-pong
    float4* guideN = nullptr;                 // decoded guides (n.xyz, 0), (a.xyz, 0)
    float4* guideA = nullptr;
    uint32_t width = 0, height = 0;           // of the working images
    EventMarks marks;                         // one per kernel boundary of the last Run
};
// The noise kernels over a film and its half film (dcrt.h "film noise estimate")
class NoiseEstimator {
public:
    int Run(hipStream_t stream, uint32_t w, uint32_t h, const float4* f, const float4* hf, float threshold, float* pixelMap, float* tileMap,
            dcrt_noise_stats* out);

private:
    DeviceGroup allocs;                       // grows with the tile count
    uint32_t tileCap = 0;
    float *sum = nullptr, *scratch[2] = { nullptr, nullptr }, *tileMax = nullptr, *tileErr = nullptr;
    uint32_t* counts = nullptr;
    NoiseTotals* totals = nullptr;
    Pinned<NoiseTotals> hostTotals;
};
// The block lists of dcrt.h "adaptive sampling": the mask and compaction kernels, and the sentinel fill
class BlockSampler {
public:
    int Run(hipStream_t stream, bool timing, uint32_t w, uint32_t h, const float4* f, const float4* hf, float threshold, uint32_t margin,
            uint32_t* flags, uint32_t* list, uint32_t* outCount, uint32_t* outPixels);
    // The sentinel sample into the inactive pixels of `slots` sample images
    int Fill(hipStream_t stream, bool timing, float2* pos, float4* val, const uint32_t* flags, uint32_t w, uint32_t h, uint32_t slots);
    // ms of the last Run's two kernels and the last Fill's, 0 where that one was not timed
    int Timings(float* maskMs, float* compactMs, float* fillMs) const;

private:
    DeviceGroup allocs;
    uint32_t* count = nullptr;                // [2]: compact_blocks_kernel's count and in-film pixels
    uint32_t* ownFlags = nullptr;             // when the caller passes none
    uint32_t flagCap = 0;
    Pinned<uint32_t, 2> hostCount;
    EventMarks maskMarks, fillMarks;          // 3 and 2 marks when timed, else none
};
// The cascade pass and the resolve of dcrt.h "firefly re-weighting". The cascade films belong to the caller.
class FireflyFilter {
public:
    // The kernels' constants of `p`: the scales by float32 products; refuses what dcrt.h refuses
    static int MakeConsts(const dcrt_firefly_params& p, FireflyConsts* out);
    // film_cascade_kernel beside a film pass of `film` (its sample textures, or the lists), on `grid` workgroups
    int Cascade(hipStream_t stream, bool timing, uint32_t grid, const Film& film, const CascadeFilms& cas, const FireflyConsts& k,
                const FilterConsts* filter, uint32_t images, const Globals* guard, const float2* const* posList, const float4* const* valList);
    int Resolve(hipStream_t stream, bool timing, const FireflyConsts& k, uint32_t w, uint32_t h, uint32_t imageCount, const float4* film,
                const CascadeFilms& cas, float4* out);
    // ms of the last Cascade and the last Resolve, 0 where that one was not timed
    int Timings(float* cascadeMs, float* resolveMs) const;

private:
    EventMarks cascadeMarks, resolveMarks;    // 2 marks each when timed, else none
};

int FireflyFilter::MakeConsts(const dcrt_firefly_params& p, FireflyConsts* out)
{
    if (p.cascades < 2u || p.cascades > (uint32_t)kFireflyMaxCascades) { SetLastError("firefly: cascades 2..8"); return DCRT_E_INVALID_ARG; }
    if (!std::isfinite(p.start) || !std::isfinite(p.base) || !std::isfinite(p.min_support) || !(p.start > 0.0f) || !(p.base > 1.0f) ||
        !(p.min_support > 0.0f)) {
        SetLastError("firefly: start > 0, base > 1 and min_support > 0, all finite");
        return DCRT_E_INVALID_ARG;
    }
    FireflyConsts k;
    std::memset(&k, 0, sizeof(k));
    volatile float s = p.start;   // (volatile: every product is rounded to float32, whatever the host's evaluation method)
    for (uint32_t j = 0; j < p.cascades; ++j) {
        k.scale[j] = s;
        s = s * p.base;
    }
    k.top = k.scale[p.cascades - 1u];
    if (!std::isfinite(k.top)) { SetLastError("firefly: the last cascade's scale start * base^(K-1) is not finite"); return DCRT_E_INVALID_ARG; }
    volatile float r = 1.0f / p.base;
    volatile float d = 1.0f - r;
    k.invBase = r;
    k.invSpan = d;
    k.minSupport = p.min_support;
    k.cascades = p.cascades;
    *out = k;
    return DCRT_OK;
}

int FireflyFilter::Cascade(hipStream_t stream, bool timing, uint32_t grid, const Film& film, const CascadeFilms& cas, const FireflyConsts& k,
                           const FilterConsts* filter, uint32_t images, const Globals* guard, const float2* const* posList,
                           const float4* const* valList)
{
    if (timing) {
        cascadeMarks.Reset();
        CHECKED(cascadeMarks.Mark(stream));
    }
    hipLaunchKernelGGL(film_cascade_kernel, dim3(grid), dim3(kFilmThreads), 0, stream, film, cas, k, filter, images, guard, posList, valList);
    if (timing) CHECKED(cascadeMarks.Mark(stream));
    return DCRT_OK;
}

// The resolve of dcrt.h over W x H device images in film convention, into `out` (not an input). Synchronous.
int FireflyFilter::Resolve(hipStream_t stream, bool timing, const FireflyConsts& k, uint32_t w, uint32_t h, uint32_t imageCount,
                           const float4* film, const CascadeFilms& cas, float4* out)
{
    Annotation an("Firefly resolve");
    if (w == 0 || h == 0 || w > 65535u || h > 65535u) { SetLastError("firefly: invalid image size"); return DCRT_E_INVALID_ARG; }
    if (imageCount == 0) { SetLastError("firefly: no image reached the film"); return DCRT_E_INVALID_ARG; }
    if (!film || !out) { SetLastError("firefly: null image"); return DCRT_E_INVALID_ARG; }
    const size_t bytes = (size_t)w * h * sizeof(float4);
    auto overlaps = [&](const void* in) {
        const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
        return a < b + bytes && b < a + bytes;
    };
    bool bad = overlaps(film);
    for (uint32_t j = 0; j < k.cascades; ++j) {
        if (!cas.film[j]) { SetLastError("firefly: null cascade image"); return DCRT_E_INVALID_ARG; }
        bad = bad || overlaps(cas.film[j]);
    }
    if (bad) { SetLastError("firefly: the output image overlaps an input"); return DCRT_E_INVALID_ARG; }
    resolveMarks.Reset();
    if (timing) CHECKED(resolveMarks.Mark(stream));
    const uint32_t T = (uint32_t)kFireflyTile;
    hipLaunchKernelGGL(firefly_resolve_kernel, dim3((w + T - 1) / T, (h + T - 1) / T), dim3(T * T), 0, stream, film, cas, k, (float)imageCount, w,
                       h, out);
    HIPCHECK(hipGetLastError());
    if (timing) CHECKED(resolveMarks.Mark(stream));
    HIPCHECK(hipStreamSynchronize(stream));
    return DCRT_OK;
}

int FireflyFilter::Timings(float* cascadeMs, float* resolveMs) const
{
    *cascadeMs = *resolveMs = 0.0f;
    if (cascadeMarks.Count() == 2u) CHECKED(cascadeMarks.ElapsedBetween(0, 1, cascadeMs));
    if (resolveMarks.Count() == 2u) CHECKED(resolveMarks.ElapsedBetween(0, 1, resolveMs));
    return DCRT_OK;
}

int FilmDenoiser::EnsureWork(hipStream_t stream, uint32_t w, uint32_t h)
{
    if (w == width && h == height && work[0]) return DCRT_OK;
    HIPCHECK(hipStreamSynchronize(stream));
    allocs.Free();
    width = height = 0;
    work[0] = work[1] = guideN = guideA = nullptr;
    const size_t n = (size_t)w * h;
    CHECKED(allocs.Alloc(&work[0], n));
    CHECKED(allocs.Alloc(&work[1], n));
    CHECKED(allocs.Alloc(&guideN, n));
    CHECKED(allocs.Alloc(&guideA, n));
    width = w; height = h;
    return DCRT_OK;
}

static int CheckDenoiseParams(const dcrt_denoise_params& p)
{
    if (p.iterations < 1u || p.iterations > 8u) { SetLastError("denoise: iterations 1..8"); return DCRT_E_INVALID_ARG; }
    for (const float s : { p.sigma_luminance, p.sigma_normal, p.sigma_albedo }) {
        if (!(s >= 0.0f) || !std::isfinite(s)) { SetLastError("denoise: sigmas are finite and >= 0 (0 switches a term off)"); return DCRT_E_INVALID_ARG; }
    }
    return DCRT_OK;
}

// The lattice stride L of the pass at `step` (DESIGN "Film denoiser", profiles/denoise_ab_pass.txt):
// 0 every tap from memory; 1 the LDS-staged pixel tile (halo 2 * step); L > 1 the LDS-staged
// lattice of every L-th pixel, its taps step / L points apart. DCRT_DENOISE_PASS=global | tile |
// lattice (L = step) | latticeN (L = min(N, step)) forces one for an A/B, where its span fits.
// All compute the same bits. The default is what measured fastest per step at 1920x1080
// (profiles/denoise_ab_pass.txt): the tile up to step 4; from memory at step 8 (the lattice's
// staging loads lie 128 B apart there and take twice as long); the lattice at 16 and 32; from
// memory again at 64 and 128, where most taps fall outside the image and most lattice
// workgroups hold a handful of points.
static uint32_t DenoisePassLattice(uint32_t step)
{
    uint32_t L = step <= 4u ? 1u : (step == 16u || step == 32u) ? step : 0u;
    if (const char* e = std::getenv("DCRT_DENOISE_PASS")) {
        uint32_t want = L;
        if (!std::strcmp(e, "global")) want = 0u;
        else if (!std::strcmp(e, "tile")) want = 1u;
        else if (!std::strcmp(e, "lattice")) want = step;
        else if (!std::strncmp(e, "lattice", 7)) want = std::min<uint32_t>(step, std::max(1, std::atoi(e + 7)));
        // (a stride that divides the step and leaves taps at most 4 lattice points apart: 48 KiB of LDS)
        if (want == 0u || (step % want == 0u && step / want <= 4u)) L = want;
    }
    return L;
}

// The filter of dcrt.h "film denoiser" over W x H device images in film convention, into `out`
// (c_N * d, 1): prologue (resolve + pack), variance estimate, `iterations` a-trous passes that
// ping-pong between the two working images, the last one remodulating into `out`. Synchronous.
// timing: a mark in front of every kernel and one behind the last.
int FilmDenoiser::Run(hipStream_t stream, bool timing, const dcrt_denoise_params& p, uint32_t w, uint32_t h, const float4* color,
                      const float4* normal, const float4* albedo, float4* out)
{
    Annotation an("Denoise");
    CHECKED(CheckDenoiseParams(p));
    if (w == 0 || h == 0 || w > 65535u || h > 65535u) { SetLastError("denoise: invalid image size"); return DCRT_E_INVALID_ARG; }
    if (!color || !normal || !albedo || !out) { SetLastError("denoise: null image"); return DCRT_E_INVALID_ARG; }
    const size_t n = (size_t)w * h, bytes = n * sizeof(float4);
    for (const float4* in : { color, normal, albedo }) {
        const char *a = (const char*)in, *b = (const char*)out;
        if (a < b + bytes && b < a + bytes) { SetLastError("denoise: the output image overlaps an input"); return DCRT_E_INVALID_ARG; }
    }
    CHECKED(EnsureWork(stream, w, h));
    DenoiseConsts k;
    k.sigmaL = p.sigma_luminance;
    k.kn = p.sigma_normal > 0.0f ? 1.0f / (p.sigma_normal * p.sigma_normal) : 0.0f;
    k.ka = p.sigma_albedo > 0.0f ? 1.0f / (p.sigma_albedo * p.sigma_albedo) : 0.0f;
    k.demodulate = p.demodulate ? 1u : 0u;
    marks.Reset();
    auto mark = [&] { return timing ? marks.Mark(stream) : (int)DCRT_OK; };
    const int W = (int)w, H = (int)h;
    const uint32_t tiles = ((w + kDnTile - 1) / kDnTile) * ((h + kDnTile - 1) / kDnTile);
    CHECKED(mark());
    hipLaunchKernelGGL(denoise_prologue_kernel, dim3(std::max<uint32_t>(1u, std::min<uint32_t>((uint32_t)((n + 255) / 256), kMaxPersistentBlocks * 4u))),
                       dim3(256), 0, stream, color, normal, albedo, (uint32_t)n, k.demodulate, work[0], guideN, guideA);
    CHECKED(mark());
    hipLaunchKernelGGL(denoise_variance_kernel, dim3(tiles), dim3(kDnThreads), 0, stream, k, (const float4*)work[0],
                       (const float4*)guideN, (const float4*)guideA, W, H, work[1]);
    CHECKED(mark());
    uint32_t src = 1;
    for (uint32_t i = 0; i < p.iterations; ++i) {
        const uint32_t step = 1u << i;
        float4* finalOut = i + 1 == p.iterations ? out : nullptr;
        uint32_t L = DenoisePassLattice(step);
        const uint32_t Ls = std::max(1u, L), t = step / Ls, span = (uint32_t)kDnTile + 4u * t;
        const uint64_t blocks = (uint64_t)Ls * Ls * (((w + Ls - 1) / Ls + kDnTile - 1) / kDnTile) * (((h + Ls - 1) / Ls + kDnTile - 1) / kDnTile);
        if (blocks > 0x7FFFFFFFull) L = 0u;   // (a lattice of a huge image at a large step: more classes than a grid holds)
        if (L == 0u) {
            hipLaunchKernelGGL(denoise_pass_global_kernel, dim3(tiles), dim3(kDnThreads), 0, stream, k, (const float4*)work[src],
                               (const float4*)guideN, (const float4*)guideA, W, H, (int)step, work[src ^ 1u], finalOut);
        } else {
            hipLaunchKernelGGL(denoise_pass_staged_kernel, dim3((uint32_t)blocks), dim3(kDnThreads), (size_t)3 * span * span * sizeof(float4),
                               stream, k, (const float4*)work[src], (const float4*)guideN, (const float4*)guideA, W, H, (int)step,
                               (int)L, work[src ^ 1u], finalOut);
        }
        CHECKED(mark());
        src ^= 1u;
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(stream));
    return DCRT_OK;
}

int FilmDenoiser::Timings(float* outMs, uint32_t capacity, uint32_t* outCount) const
{
    const uint32_t kernels = marks.Count() ? marks.Count() - 1u : 0u;
    *outCount = kernels;
    for (uint32_t i = 0; i < kernels && i < capacity; ++i) CHECKED(marks.ElapsedBetween(i, i + 1, &outMs[i]));
    return DCRT_OK;
}

// The noise kernels over a film and its half film (dcrt.h): tiles, the 128-group reduction of
// the tile sums with luminance_single_kernel, counts and maxima; one copy of the totals back.
int NoiseEstimator::Run(hipStream_t stream, uint32_t w, uint32_t h, const float4* f, const float4* hf, float threshold, float* pixelMap,
                        float* tileMap, dcrt_noise_stats* out)
{
    Annotation an("Noise estimate");
    if (!f || !hf || !out || w == 0 || h == 0 || w > 65535u || h > 65535u) return DCRT_E_INVALID_ARG;
    if (!(threshold >= 0.0f)) { SetLastError("noise: the threshold is negative or NaN"); return DCRT_E_INVALID_ARG; }
    const uint32_t T = (uint32_t)kNoiseTile, tilesX = (w + T - 1) / T, tilesY = (h + T - 1) / T, tiles = tilesX * tilesY;
    if (tiles > tileCap) {
        HIPCHECK(hipStreamSynchronize(stream));
        allocs.Free();
        tileCap = 0;
        CHECKED(allocs.Alloc(&sum, tiles));
        CHECKED(allocs.Alloc(&scratch[0], (tiles + 127) / 128));
        CHECKED(allocs.Alloc(&scratch[1], (tiles + 127) / 128));
        CHECKED(allocs.Alloc(&tileMax, tiles));
        CHECKED(allocs.Alloc(&tileErr, tiles));
        CHECKED(allocs.Alloc(&counts, (size_t)tiles * 2));
        CHECKED(allocs.Alloc(&totals, 1));
        tileCap = tiles;
    }
    hipLaunchKernelGGL(noise_tile_kernel, dim3(tilesX, tilesY), dim3(T * T), 0, stream, f, hf, w, h, threshold, pixelMap, tileMap, sum,
                       tileMax, tileErr, counts);
    const float* in = sum;
    uint32_t count = tiles, side = 0;
    while (count != 1) {
        const uint32_t groups = (count + 127) / 128;
        hipLaunchKernelGGL(luminance_single_kernel, dim3(groups), dim3(128), 0, stream, in, count, scratch[side]);
        in = scratch[side];
        side ^= 1u;
        count = groups;
    }
    hipLaunchKernelGGL(noise_finish_kernel, dim3(1), dim3(256), 0, stream, (const float*)tileMax, (const float*)tileErr,
                       (const uint32_t*)counts, tiles, in, totals);
    HIPCHECK(hipGetLastError());
    CHECKED(hostTotals.Alloc());
    const NoiseTotals* host = hostTotals.get();
    HIPCHECK(hipMemcpyAsync(hostTotals.get(), totals, sizeof(NoiseTotals), hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    out->images = 0;
    out->valid_pixels = host->valid;
    out->converged_pixels = host->converged;
    out->mean_error = host->valid ? host->total / (float)host->valid : 0.0f;
    out->max_error = host->maxError;
    out->max_tile_error = host->maxTileError;
    return DCRT_OK;
}

// sample_mask_kernel + compact_blocks_kernel over a film and its half film; the copy of the count
// (and the listed blocks' pixels) is the one synchronisation.
int BlockSampler::Run(hipStream_t stream, bool timing, uint32_t w, uint32_t h, const float4* f, const float4* hf, float threshold, uint32_t margin,
                      uint32_t* flags, uint32_t* list, uint32_t* outCount, uint32_t* outPixels)
{
    Annotation an("Sample blocks");
    if (!f || !hf || !list || !outCount || w == 0 || h == 0 || w > 65535u || h > 65535u) return DCRT_E_INVALID_ARG;
    if (!(threshold >= 0.0f)) { SetLastError("sample blocks: the threshold is negative or NaN"); return DCRT_E_INVALID_ARG; }
    const uint32_t blocksX = (w + kBlockW - 1) / kBlockW, blocks = blocksX * ((h + kBlockH - 1) / kBlockH);
    if (!count || (!flags && blocks > flagCap)) {
        HIPCHECK(hipStreamSynchronize(stream));
        allocs.Free();
        count = ownFlags = nullptr;
        flagCap = 0;
        CHECKED(allocs.Alloc(&count, 2));
        if (!flags) {
            CHECKED(allocs.Alloc(&ownFlags, blocks));
            flagCap = blocks;
        }
    }
    if (!flags) flags = ownFlags;
    CHECKED(hostCount.Alloc());
    maskMarks.Reset();
    if (timing) CHECKED(maskMarks.Mark(stream));
    hipLaunchKernelGGL(sample_mask_kernel, dim3((blocks + 3) / 4), dim3(256), 0, stream, f, hf, w, h, threshold, margin, blocksX, blocks, flags);
    if (timing) CHECKED(maskMarks.Mark(stream));
    hipLaunchKernelGGL(compact_blocks_kernel, dim3(1), dim3(256), 0, stream, (const uint32_t*)flags, blocks, blocksX, w, h, list, count);
    if (timing) CHECKED(maskMarks.Mark(stream));
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(hostCount.get(), count, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    *outCount = hostCount[0];
    if (outPixels) *outPixels = hostCount[1];
    return DCRT_OK;
}

int BlockSampler::Fill(hipStream_t stream, bool timing, float2* pos, float4* val, const uint32_t* flags, uint32_t w, uint32_t h, uint32_t slots)
{
    const uint32_t n = w * h;
    fillMarks.Reset();
    if (timing) CHECKED(fillMarks.Mark(stream));
    hipLaunchKernelGGL(fill_inactive_samples_kernel, dim3(std::min<uint32_t>((n + 255) / 256, 8u * kMaxPersistentBlocks)), dim3(256), 0, stream,
                       pos, val, flags, w, h, (w + kBlockW - 1) / kBlockW, slots);
    HIPCHECK(hipGetLastError());
    if (timing) CHECKED(fillMarks.Mark(stream));
    return DCRT_OK;
}

int BlockSampler::Timings(float* maskMs, float* compactMs, float* fillMs) const
{
    *maskMs = *compactMs = *fillMs = 0.0f;
    if (maskMarks.Count() == 3u) {
        CHECKED(maskMarks.ElapsedBetween(0, 1, maskMs));
        CHECKED(maskMarks.ElapsedBetween(1, 2, compactMs));
    }
    if (fillMarks.Count() == 2u) CHECKED(fillMarks.ElapsedBetween(0, 1, fillMs));
    return DCRT_OK;
}

// A cast_kernel variant, by its template parameters: instrumented counts x ALLOW_ANYHIT_SHADER x
// whole scene in the LDS cache x pair-expanding traversal (the non-counting kernels of scenes not
// in the LDS cache) x the world ray in every space (IDENT) x the spilling stack window (RING:
// non-counting, opaque, global-memory kernels) x the entry-free node order (FLAT) x the point
// light's direction cells for its shadow rays (CELLS)
struct CastVariant {
    bool instr, opacity, allCached, pair, ident, ring, flat, cells;
};
using CastFn = void (*)(PathPool, DeviceScene, const FrameConstants*, Counters*, Counters*, Globals*, unsigned long long*);

// The compiled kernel for what a launch asks for (DCRT_CAST_VARIANTS, kernels_impl.h). Not every
// combination is compiled; the fall-back drops, in this order, what the others rule out: FLAT is
// the cache-only IDENT kernel, CELLS goes with FLAT; RING, the counting and the any-hit kernels
// keep PackBVH's or the pair order; IDENT has no any-hit kernel and no pair kernel but the ring's.
// ... and that variant's traversal over a caller's ray batch (cast_rays_kernel: dcrt_tracer_cast_rays); the
// counting and the CELLS rows have none.
using CastRaysFn = void (*)(DeviceScene, const dcrt_ray*, const uint32_t*, const float*, uint32_t, uint32_t, uint32_t, uint32_t, dcrt_ray_hit*,
                            uint32_t*);
template <bool INSTR, bool OPACITY, bool ALL_CACHED, bool PAIR, bool IDENT, bool RING, bool FLAT, bool CELLS>
constexpr CastRaysFn CastRaysOf()
{
    if constexpr (INSTR || CELLS) return nullptr;
    else return cast_rays_kernel<OPACITY, ALL_CACHED, PAIR, IDENT, RING, FLAT>;
}
struct CastRow {
    CastVariant v;
    CastFn fn;
    CastRaysFn rays;
};
const CastRow* CastTableRow(const CastVariant& want)
{
    CastVariant v = want;
    v.flat = v.flat && v.ident && v.allCached && !v.opacity && !v.instr && !v.ring;
    v.cells = v.cells && v.flat;
    v.ring = v.ring && !v.instr && !v.opacity && !v.allCached;
    if (v.flat) {
        v.pair = false;
    } else if (v.ring) {
        v.ident = v.ident && !v.pair;
    } else {
        v.ident = v.ident && !v.opacity && (v.allCached || v.instr || !v.pair);
        v.pair = v.pair && !v.ident && !v.instr && !v.allCached;
    }
#define DCRT_CAST_ROW(...) { { __VA_ARGS__ }, cast_kernel<__VA_ARGS__>, CastRaysOf<__VA_ARGS__>() },
    static const CastRow table[] = { DCRT_CAST_VARIANTS(DCRT_CAST_ROW) };
#undef DCRT_CAST_ROW
    for (const CastRow& r : table) {
        if (r.v.instr == v.instr && r.v.opacity == v.opacity && r.v.allCached == v.allCached && r.v.pair == v.pair &&
            r.v.ident == v.ident && r.v.ring == v.ring && r.v.flat == v.flat && r.v.cells == v.cells)
            return &r;
    }
    return nullptr;   // (no input gets here: the fall-back above ends on a compiled variant)
}
CastFn CastKernel(const CastVariant& want)
{
    const CastRow* r = CastTableRow(want);
    return r ? r->fn : nullptr;
}

// ---- DCRT_* knobs: one reader per moment they are read at, one struct each -- the list of knobs,
// with their defaults (A/B experiments and tests; the static ones sit with their code:
// DCRT_MAX_BATCH, DCRT_BATCH_POOL_LIMIT, DCRT_ROCTX, DCRT_DENOISE_PASS) ------------------------
int EnvInt(const char* name, int unset)
{
    const char* e = std::getenv(name);
    return e ? std::atoi(e) : unset;
}
bool EnvFlag(const char* name, bool unset)
{
    const char* e = std::getenv(name);
    return e ? std::atoi(e) != 0 : unset;
}

struct CreateKnobs {
    bool mergedCasts = true;           // one cast_kernel per iteration (DCRT_SPLIT_CASTS=1: EXT then SHADOW)
    bool virtualStart = true;          // virtual batch starts where the cast kernel has them (DCRT_VIRTUAL_START=0: off)
    uint32_t drainPaths = 0;           // drain_kernel threshold (DCRT_DRAIN_PATHS; 0: no drain launches -- the default: profiles/r04_ab_virtual_drain.txt)
    // cast-kernel refill / park thresholds (persistent_trace): refill when 36 lanes are idle
    // in the LDS-only kernel, 28 in the global-memory one (round 3 sweep with the adaptive
    // park threshold); park at 24 (profiles/r01_tune_sweep.txt); DCRT_TRAVERSAL_TUNE=
    // "refill,park" overrides both
    uint32_t refillLanes = 36, parkLanes = 24;
    bool tuneOverride = false;
    // DCRT_CONTROL_GRID / DCRT_MATERIAL_GRID = k: k x resident; 0: one workgroup per virtual
    // workgroup. 2x / 4x resident (two A/B passes of the default bench on cornell / spaceship / coffee,
    // ms/spp: one workgroup per virtual workgroup 2.40 / 2.84 / 2.96; 1x / 1x 2.28-2.38 /
    // 2.63 / 3.02; 1x / 4x 2.37 / 2.58 / 2.95; 2x / 4x 2.35-2.38 / 2.54 / 2.92; 4x / 4x
    // 2.37 / 2.55 / 2.95; 2x / 8x 2.37-2.39 / 2.55 / 2.92)
    uint32_t controlGridMul = 2, materialGridMul = 4;
};
CreateKnobs ReadCreateKnobs()
{
    CreateKnobs k;
    k.mergedCasts = !EnvFlag("DCRT_SPLIT_CASTS", false);
    k.virtualStart = EnvFlag("DCRT_VIRTUAL_START", true);
    k.drainPaths = (uint32_t)std::max(0, EnvInt("DCRT_DRAIN_PATHS", 0));
    if (const char* tune = std::getenv("DCRT_TRAVERSAL_TUNE")) {
        unsigned r = 0, p = 0;
        if (std::sscanf(tune, "%u,%u", &r, &p) == 2 && r >= 1 && r <= 64 && p >= 1 && p <= 64) {
            k.refillLanes = r;
            k.parkLanes = p;
            k.tuneOverride = true;
        }
    }
    k.controlGridMul = (uint32_t)std::max(0, EnvInt("DCRT_CONTROL_GRID", (int)k.controlGridMul));
    k.materialGridMul = (uint32_t)std::max(0, EnvInt("DCRT_MATERIAL_GRID", (int)k.materialGridMul));
    return k;
}

#ifndef DCRT_CAST_LDS_RESERVE
#define DCRT_CAST_LDS_RESERVE 12288   // (A/B: coffee -2 to -3 %, lamp -1 %; profiles/r04_ab_round4.txt)
#endif
struct UploadKnobs {
    uint32_t castBlock = 0;            // DCRT_CAST_BLOCK = 64 / 128 / 256, at most the block the stack allows (else: that block)
    bool noLdsCache = false;           // DCRT_NO_LDS_CACHE=1: no LDS scene cache
    int pairTraversal = -1;            // DCRT_PAIR_TRAVERSAL=0/1 forces trav_visit_pair off / on (-1: by the scene's size)
    uint32_t topNodes = 4096;          // DCRT_TOP_NODES: PairLayout's breadth-first prefix
    bool nodeQuads = true;             // DCRT_NODE_QUADS=0: PairLayout without quads (profiles/r06_ab_log.md: spaceship -1.6 %, close framing -0.1 / -1.4 %)
    bool identCast = true;             // DCRT_IDENT_CAST=0: no IDENT kernel
    int stackRing = -1;                // DCRT_STACK_RING = K (a power of two, 8..64) forces a ring window of K rows, 0: never (-1: where it gains occupancy)
    size_t castLdsReserve = DCRT_CAST_LDS_RESERVE;   // DCRT_CAST_LDS_RESERVE: bytes per CU the LDS cache leaves free
    uint32_t skipRoot = 1;             // DCRT_SKIP_ROOT: trav_skip_root's levels of sure hits taken without their box tests (0..16)
    bool ldsTrim = true;               // DCRT_LDS_TRIM=0: the cache is not trimmed to the LDS granule
    bool flatCast = true;              // DCRT_FLAT_CAST=0: no entry-free node order
    bool flatMerge = true;             // DCRT_FLAT_MERGE=0: every TLAS leaf over an empty node
    uint32_t shadowCells = dcrt::kCellDefaultRes;   // DCRT_SHADOW_CELLS = the direction cells' cube map resolution R (0: off)
    int castBlocksPerCU = 0;           // DCRT_CAST_BLOCKS_PER_CU: fewer resident cast workgroups per CU than fit
    int castGridMul = 0;               // DCRT_CAST_GRID_MUL = k (2..16): k x resident, workgroups retire in k rounds
};
UploadKnobs ReadUploadKnobs()
{
    UploadKnobs k;
    k.castBlock = (uint32_t)EnvInt("DCRT_CAST_BLOCK", 0);
    k.noLdsCache = EnvFlag("DCRT_NO_LDS_CACHE", false);
    if (std::getenv("DCRT_PAIR_TRAVERSAL")) k.pairTraversal = EnvFlag("DCRT_PAIR_TRAVERSAL", false) ? 1 : 0;
    k.topNodes = (uint32_t)EnvInt("DCRT_TOP_NODES", (int)k.topNodes);
    k.nodeQuads = EnvFlag("DCRT_NODE_QUADS", true);
    k.identCast = EnvFlag("DCRT_IDENT_CAST", true);
    k.stackRing = EnvInt("DCRT_STACK_RING", -1);
    if (std::getenv("DCRT_CAST_LDS_RESERVE")) k.castLdsReserve = (size_t)std::max(0, EnvInt("DCRT_CAST_LDS_RESERVE", 0));
    k.skipRoot = (uint32_t)std::max(0, std::min(16, EnvInt("DCRT_SKIP_ROOT", (int)k.skipRoot)));
    k.ldsTrim = EnvFlag("DCRT_LDS_TRIM", true);
    k.flatCast = EnvFlag("DCRT_FLAT_CAST", true);
    k.flatMerge = EnvFlag("DCRT_FLAT_MERGE", true);
    k.shadowCells = (uint32_t)std::max(0, std::min((int)dcrt::kCellMaxRes, EnvInt("DCRT_SHADOW_CELLS", (int)k.shadowCells)));
    k.castBlocksPerCU = EnvInt("DCRT_CAST_BLOCKS_PER_CU", 0);
    k.castGridMul = EnvInt("DCRT_CAST_GRID_MUL", 0);
    return k;
}

struct ShadingKnobs {
    bool materialGeneric = false;      // DCRT_MATERIAL_GENERIC=1: always the generic MATERIAL variant
    uint32_t materialLds = 16384;      // DCRT_MATERIAL_LDS = bytes budget of MATERIAL's LDS scene copy, 0: off
    bool materialLdsPartial = true;    // DCRT_MATERIAL_LDS_PARTIAL=0: no mode 2 (everything but the triangles)
    // DCRT_FUSED_SHADOW: MATERIAL tests the shadow rays of a scene with direction cells itself
    // (material_kernel's FUSED); 0: every shadow ray takes the shadow queue. n > 1 (tests): fused, and
    // the path slots with (slot & (n - 1)) != 0 take the queue all the same, so a wave mixes both routes.
    uint32_t fusedShadow = 1;
    // DCRT_SHADING_TABLES: scene-constant shading work done at upload instead of per hit, one bit
    // each (kTableDeltaPdf, kTableDielRows of dscene.h); 0: every hit does it itself.
    uint32_t shadingTables = kTableAll;
    // DCRT_EARLY_FINISH: a MATERIAL variant without mesh and environment lights finishes a path at its last
    // shaded bounce (material_kernel's EARLY); 0: every path takes the pass that only completes it. 2 (tests):
    // on for the even path slots alone, so a wave mixes both routes.
    uint32_t earlyFinish = 1;
};
ShadingKnobs ReadShadingKnobs()
{
    ShadingKnobs k;
    k.materialGeneric = EnvFlag("DCRT_MATERIAL_GENERIC", false);
    k.materialLds = (uint32_t)std::max(0, EnvInt("DCRT_MATERIAL_LDS", (int)k.materialLds));
    k.materialLdsPartial = EnvFlag("DCRT_MATERIAL_LDS_PARTIAL", true);
    k.fusedShadow = (uint32_t)std::max(0, EnvInt("DCRT_FUSED_SHADOW", (int)k.fusedShadow));
    k.shadingTables = (uint32_t)std::max(0, EnvInt("DCRT_SHADING_TABLES", (int)k.shadingTables)) & kTableAll;
    k.earlyFinish = (uint32_t)std::max(0, std::min(2, EnvInt("DCRT_EARLY_FINISH", (int)k.earlyFinish)));
    return k;
}

// Workgroups per CU that a workgroup's LDS allocation allows. hipOccupancyMaxActiveBlocksPerMultiprocessor
// rounds the allocation to 512 B, but gfx950 allocates LDS in 1280-B granules (160 KiB / 128). Measured
// on the persistent cast grid (one workgroup per resident slot): 6 x 26944 B and 5 x 32768 B per CU
// ran with 5 and 4 workgroups resident (the last one as a tail: cast launches +26 % / +29 %), while
// 6 x 26608 B ran with 6 -- the 1280-B rounding predicts all three (profiles/r04_ab_round4.txt).
// `lds` counts a workgroup's dynamic LDS; the kernel's static LDS (hipFuncAttributes
// sharedSizeBytes, e.g. the megakernel's claim words) comes on top of it. The per-CU total is the
// device's (maxSharedMemoryPerMultiProcessor: 160 KiB on gfx950, the only target this library is
// built for); the 1280-B granule is gfx950's.
size_t g_ldsPerCU = 163840;
constexpr size_t kLdsGranule = 1280;
int LdsResident(size_t lds, const void* kernel = nullptr)
{
    if (kernel) {
        hipFuncAttributes attr{};
        if (hipFuncGetAttributes(&attr, kernel) == hipSuccess) lds += attr.sharedSizeBytes;
    }
    return lds ? (int)(g_ldsPerCU / ((lds + kLdsGranule - 1) / kLdsGranule * kLdsGranule)) : 1 << 20;
}
// Resident workgroups per CU of `kernel` with `block` threads and `lds` bytes of dynamic LDS: what its
// registers allow (the occupancy API) and what the LDS granules allow
int ResidentPerCU(const void* kernel, uint32_t block, size_t lds, int* out)
{
    int n = 0;
    HIPCHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, (int)block, lds));
    *out = std::min(n, LdsResident(lds, kernel));
    return DCRT_OK;
}

// What a launch of the cast needs
struct CastLaunch {
    CastFn kernel;
    size_t lds;                        // dynamic LDS bytes
    const DeviceScene& scene;
    uint32_t resident;                 // persistent grid: resident workgroups on the whole chip
    CastVariant asked;                 // what the plan asks CastKernel for (dcrt_tracer_cast_rays picks the ray-batch twin by it)
};

// How the uploaded scene is cast (PlanCast, SizeGrids): the one place that says which cast_kernel
// variant runs, on which copy of the scene and with how much LDS.
struct CastPlan {
    uint32_t block = 256;              // workgroup size of every traversal kernel
    uint32_t perCU = 0;                // resident workgroups per CU of the shipped kernel
    bool allCached = false;            // the scene fits the LDS cache: cast_kernel's ALL_CACHED
    bool pair = false;                 // trav_visit_pair: the scene outgrows an XCD's L2
    bool ident = false;                // no instance space (every instance the identity: dscene.h IDENT)
    bool flat = false;                 // the cache-only IDENT cast runs on the entry-free node order (EntryFreeLayout)
    uint32_t ringRows = 0;             // the ring cast kernel's LDS stack window (0: whole stack in LDS)
    // The point light's direction cells (shadow_cells.h) of a flat scene: the resolution asked for
    // (0: off, or the leaf words did not fit the cast's LDS without costing occupancy).
    // sceneFlat.shadowRes != 0 while a table stands (RebuildShadowCells).
    uint32_t cellsRes = 0;
    // a workgroup's dynamic LDS: the stack rows in front of the scene cache
    size_t ldsWholeStack = 0;          // stackSize + 2 rows: every kernel but the ring and the flat cast
    size_t ldsRing = 0;                // ringRows rows (ringRows != 0)
    size_t ldsFlat = 0;                // stackSize + 3 rows, the entry-free nodes, the cells' leaf words
    DeviceScene scene{};               // the uploaded scene (the PackBVH or the pair node order)
    DeviceScene sceneRing{};           // ... as the ring cast kernel sees it (stackRows = ringRows, spill column)
    DeviceScene sceneFlat{};           // ... as the flat cast kernel sees it (its nodes, one more stack row, the cells)
    uint32_t resident[2][2] = {};      // [instr][opacity] persistent grids; [0][0]: the shipped kernel's

    // The cast of a frame with or without counters and ALLOW_ANYHIT_SHADER. The ring and the flat
    // kernel are non-counting and opaque (the counting and any-hit kernels keep the whole stack
    // and the plain scene); the cells go with the flat kernel while a table stands.
    // (Cells: that launch is the CELLS cast -- MATERIAL's fused variant goes with exactly these launches)
    bool Cells(bool instr, bool opacity) const { return flat && !instr && !opacity && sceneFlat.shadowRes != 0u; }
    CastLaunch Launch(bool instr, bool opacity) const
    {
        const bool useFlat = flat && !instr && !opacity, useRing = ringRows != 0 && !instr && !opacity;
        const CastVariant v{ instr, opacity, allCached, pair, ident, useRing, useFlat, Cells(instr, opacity) };
        return { CastKernel(v), useFlat ? ldsFlat : useRing ? ldsRing : ldsWholeStack, useFlat ? sceneFlat : useRing ? sceneRing : scene,
                 resident[instr][opacity], v };
    }
};

using MaterialFn = void (*)(PathPool, DeviceScene, const FrameConstants*, Counters*, const Counters*, const SampleOut*, ShadowInline);

// How MATERIAL (and the drain kernel, which shades with the same variant) is launched for the uploaded
// scene with its current materials and lights (dcrt_tracer::PlanMaterial): the one place that says which
// material_kernel runs and with how much LDS.
struct MaterialPlan {
    // the compiled variant that covers the scene: kCapOpaqueDelta, kCapAll, or kCapAllEnvImportance -- the any-scene
    // variant that samples the environment cube by the table `envProb` names (dscene.h)
    uint32_t caps = kCapAll;
    uint32_t mode = 0;                 // material_kernel's SCENE_LDS: 0 no copy, 1 whole shading data, 2 all but the triangles
    uint32_t materials = 0, lights = 0;   // the counts the LDS copy holds (0 without one)
    // The sections of the dynamic LDS (dscene.h material_lds_layout; 0 bytes: not held). cells != 0: the fused
    // variant is sized for the scene; a launch takes it with the CELLS cast alone (dcrt_tracer::FusedShadow).
    MaterialLds lds{};
    // DCRT_SHADING_TABLES as it stands for the scene: the bits in force, and the buffers of the tables in force
    uint32_t tables = 0;
    const float* dielRows = nullptr;
    const float4* triFrames = nullptr;
    // The environment cube's sampling table in force (dcrt_tracer::BuildEnvTable), or null: the uniform sphere
    const float* envProb = nullptr;
    const float* envRowCdf = nullptr;
    const float* envMarginal = nullptr;
    // The light table in force (dcrt_tracer::BuildLightTable) with the light count it was built for, or null / 0:
    // uniform selection
    const float* lightProb = nullptr;
    const float* lightCdf = nullptr;
    const uint32_t* triBase = nullptr;
    const float* triProb = nullptr;
    const float* triCdf = nullptr;
    uint32_t lightTableCount = 0;
    uint32_t fusedMask = 0;            // DCRT_FUSED_SHADOW's path-slot mask (FrameConstants::shadowInlineMask: not baked into a graph)
    uint32_t drainGrid = 0;            // drain_kernel's grid: resident workgroups on the whole chip
    // DCRT_EARLY_FINISH as it stands for the variant: 0 unless its CAPS admit it (caps_early_finish). The same
    // kernel, grid and LDS either way: a scalar the kernel reads (DeviceScene::earlyFinish).
    uint32_t earlyFinish = 0;
    // ... and for a launch: not the probe's variant, not with ALLOW_ANYHIT_SHADER (material_kernel tests both itself)
    uint32_t EarlyFinish(bool probe, bool opacity) const { return probe || opacity ? 0u : earlyFinish; }

    // The one table from variant to compiled kernel. probe: the row-cost probe's variant (no LDS copy)
    MaterialFn Kernel(bool probe, bool fused) const
    {
        const bool od = caps == kCapOpaqueDelta;
        // (no fused form under the light table either: such a plan never launches it, as below)
        if (caps == kCapAllLightTable && !fused) {
            if (probe) return material_kernel<kCapAllLightTable, 0, true>;
            switch (mode) {
            case 1: return material_kernel<kCapAllLightTable, 1>;
            case 2: return material_kernel<kCapAllLightTable, 2>;
            default: return material_kernel<kCapAllLightTable, 0>;
            }
        }
        if (caps == kCapAllEnvImportance && !fused) {
            if (probe) return material_kernel<kCapAllEnvImportance, 0, true>;
            switch (mode) {
            case 1: return material_kernel<kCapAllEnvImportance, 1>;
            case 2: return material_kernel<kCapAllEnvImportance, 2>;
            default: return material_kernel<kCapAllEnvImportance, 0>;
            }
        }
        if (probe) return material_kernel<kCapAll, 0, true>;
        // (the fused form never runs beside an environment light -- it goes with one point light's cells -- so a
        // plan with the table sizes it with the any-scene variant and never launches it)
        if (fused) return od ? material_kernel<kCapOpaqueDelta, 1, false, true> : material_kernel<kCapAll, 1, false, true>;
        switch (mode) {
        case 1: return od ? material_kernel<kCapOpaqueDelta, 1> : material_kernel<kCapAll, 1>;
        case 2: return od ? material_kernel<kCapOpaqueDelta, 2> : material_kernel<kCapAll, 2>;
        default: return od ? material_kernel<kCapOpaqueDelta, 0> : material_kernel<kCapAll, 0>;
        }
    }
    auto DrainKernel() const
    {
        if (caps == kCapAllLightTable) return drain_kernel<kCapAllLightTable>;
        return caps == kCapOpaqueDelta ? drain_kernel<kCapOpaqueDelta> : caps == kCapAllEnvImportance ? drain_kernel<kCapAllEnvImportance> : drain_kernel<kCapAll>;
    }
    using MegaFn = void (*)(DeviceScene, const FrameConstants*, Film, Globals*, uint32_t);
    MegaFn Megakernel(bool opacity) const
    {
        if (caps == kCapAllLightTable) return opacity ? megakernel<true, kCapAllLightTable> : megakernel<false, kCapAllLightTable>;
        if (caps == kCapAllEnvImportance) return opacity ? megakernel<true, kCapAllEnvImportance> : megakernel<false, kCapAllEnvImportance>;
        return opacity ? megakernel<true> : megakernel<false>;
    }
    size_t LdsBytes(bool probe, bool fused) const { return probe ? 0u : lds.Bytes(fused); }
    // The shading fields of a DeviceScene (kernels take it by value)
    void Apply(DeviceScene* d) const
    {
        d->ldsMaterials = materials;
        d->ldsLights = lights;
        d->shadingTables = tables;
        d->dielRows = dielRows;
        d->ldsRows = lds.rows ? materials : 0u;
        d->triFrames = triFrames;
        d->ldsFrames = lds.frames ? 1u : 0u;
        d->envProb = envProb;
        d->envRowCdf = envRowCdf;
        d->envMarginal = envMarginal;
        d->lightProb = lightProb;
        d->lightCdf = lightCdf;
        d->triBase = triBase;
        d->triProb = triProb;
        d->triCdf = triCdf;
        d->earlyFinish = earlyFinish;
    }
    // What a captured graph bakes in: kernels, LDS bytes, the drain grid, what Apply writes (the pointers follow the bits)
    bool BakedEquals(const MaterialPlan& o) const
    {
        return caps == o.caps && mode == o.mode && materials == o.materials && lights == o.lights && lds.shading == o.lds.shading &&
               lds.rows == o.lds.rows && lds.frames == o.lds.frames && lds.cells == o.lds.cells && tables == o.tables && drainGrid == o.drainGrid &&
               envProb == o.envProb && envRowCdf == o.envRowCdf && envMarginal == o.envMarginal && earlyFinish == o.earlyFinish &&
               lightProb == o.lightProb && lightCdf == o.lightCdf && triBase == o.triBase && triProb == o.triProb && triCdf == o.triCdf &&
               lightTableCount == o.lightTableCount;
    }
};

// dcrt_roulette_default_params: off; on, from the third vertex on with the throughput as the survival probability
constexpr dcrt_roulette_params kRouletteDefaults = {0u, 2u, 0.05f, 1.0f};

// 0 < min_survival <= max_survival <= 1 (a NaN fails every comparison), start_bounce within the bounce limit
bool RouletteParamsValid(const dcrt_roulette_params& p)
{
    return p.min_survival > 0.0f && p.min_survival <= p.max_survival && p.max_survival <= 1.0f && p.start_bounce <= DCRT_MAX_RAY_BOUNCE;
}

}  // namespace

struct dcrt_tracer {
    int device = 0;
    hipStream_t stream = nullptr;
    bool ownsStream = false;
    // The first member, so the last to go: every member below frees what it owns (device groups, pinned staging,
    // the stages' scratch and marks) before the stream is destroyed, as ~dcrt_tracer always had it.
    struct StreamEnd {
        dcrt_tracer* t;
        ~StreamEnd()
        {
            if (t->ownsStream && t->stream) (void)hipStreamDestroy(t->stream);
        }
    } streamEnd{ this };
    uint32_t cuCount = 1;              // compute units (the persistent grids' factor)
    CreateKnobs knobs;
    uint32_t iterationsPerRender = kDefaultIterations;
    bool debugRng = false;
    int mode = 0;                      // 0 wavefront (WavefrontPathTracer), 1 megakernel (MegakernelPathTracer)
    // the "Output" view (dcrt_tracer_set_output): anything but PATH_TRACING renders first hits
    dcrt_output_params output{ DCRT_OUTPUT_PATH_TRACING, 20u };

    // ---- path pool ----
    uint32_t poolSize = 0;
    // CONTROL / MATERIAL grids (ResidentGrid): workgroups that loop over the pool's 256-slot
    // "virtual workgroups" vb = blockIdx.x + round * gridDim.x
    uint32_t controlGrid = 0, materialGrid = 0;
    DeviceGroup poolAllocs;
    PathPool pool{};                   // (queue pointers set per launch: LaunchIteration)
    float4* extRecs = nullptr;         // 2 parities x kShards x recCap extension-ray records (2 float4)
    PathStateA* stateRecsA = nullptr;  // 2 parities x kShards x recCap path state halves
    PathStateB* stateRecsB = nullptr;
    uint32_t* shadowHits = nullptr;    // 2 parities x kShards x recCap shadow results
    FinishRec* finRecs = nullptr;      // 2 parities x kFinShards x pool.finCap
    uint32_t* finHits = nullptr;       // 2 parities x kFinShards x pool.finCap
    FrameConstants* dFrame = nullptr;
    Counters* dCounters = nullptr;     // [2]
    Globals* dGlobals = nullptr;
    Pinned<uint32_t> hPoolIdle;        // ReadCompletion's copy of Globals::poolIdle
    dcrt_bxdf_luts* dLuts = nullptr;

    // ---- scene and cast plan ----
    DeviceGroup sceneAllocs;
    bool hasScene = false;
    CastPlan plan;
    dcrt_upload_stats uploadStats{};
    MaterialPlan material;
    // The tables' buffers (DCRT_SHADING_TABLES; material.tables says which are in force): the rows of
    // the dielectric LUT -- room for the scene's materials, null beyond kDielRowsMaxMaterials -- and
    // the triangles' world-space frames, built at upload where no BLAS has two instances (else null)
    float* dDielRows = nullptr;
    float4* dTriFrames = nullptr;
    // Environment importance sampling (dcrt.h): the mode asked for, which outlives the scene, and the uploaded
    // cube's table -- built when the mode is on and the scene has a cube, null when there is none or its
    // total weight is zero or not finite ("inactive": the uniform sphere) -- with its last build's time.
    int envSampling = DCRT_ENV_SAMPLING_UNIFORM;
    float* dEnvProb = nullptr;
    float* dEnvRowCdf = nullptr;
    float* dEnvMarginal = nullptr;
    float envBuildMs = 0.0f;
    bool EnvTableActive() const { return hasScene && envSampling == DCRT_ENV_SAMPLING_IMPORTANCE && dEnvProb != nullptr; }
    // Light selection (dcrt.h): the mode asked for, which outlives the scene, and the table of the lights as they
    // stand -- null when there is none ("inactive": no lights, one light that is no lamp, a total weight that is zero
    // or not finite, a lamp whose triangles lie outside the scene). The buffers live in a group of their own: a
    // rebuild for other lamps frees them, an edit of the colours alone rewrites lightProb and lightCdf in place.
    int lightSampling = DCRT_LIGHT_SAMPLING_UNIFORM;
    DeviceGroup lightAllocs;
    struct LightTable {
        float* prob = nullptr;
        float* cdf = nullptr;
        uint32_t* triBase = nullptr;
        float* triProb = nullptr;
        float* triCdf = nullptr;
        float* areas = nullptr;          // a_t per entry, and the float64 sums the finish pass normalises
        double* triSums = nullptr;
        double* lightAreas = nullptr;    // A_l: what the light-level kernel reads again after a colour edit
        double* weightSums = nullptr;    // n + 1: the unnormalised CDF and the total
        uint32_t entries = 0;
        double total = 0.0;
        std::vector<dcrt_light> lights;  // the lights it was built for
    } lightTable;
    double sceneRadius = 0.0;            // R: half the diagonal of the uploaded BVH root's box
    double envMeanY = 1.0;               // Ybar of the uploaded cube (1 without one), once envMeanYKnown
    bool envMeanYKnown = true;
    float lightBuildMs = 0.0f;
    bool LightTableActive() const { return hasScene && lightSampling == DCRT_LIGHT_SAMPLING_POWER && lightTable.prob != nullptr; }
    // Russian roulette (dcrt.h): the tracer's setting, kept across uploads and edits; BeginImage writes it into the
    // frame constants beside maxBounce, so a change costs no graph
    dcrt_roulette_params roulette = kRouletteDefaults;
    // MATERIAL of the next launch tests its shadow rays itself: where the cast is the CELLS kernel
    bool FusedShadow() const
    {
        return material.lds.cells != 0u && !rowProbe && plan.Cells(instrCounters, (frame.features & DCRT_FEATURE_ALLOW_ANYHIT) != 0);
    }
    // The arrays the partial updates replace (UpdateMaterials / UpdateLights / UpdateInstanceFlags):
    // their device buffers, and host copies of the two that PlanMaterial reads. The lights
    // buffer holds DCRT_MAX_LIGHT_COUNT entries, so a changed count never moves it.
    dcrt_material* dMaterials = nullptr;
    dcrt_light* dLights = nullptr;
    uint32_t* dInstanceFlags = nullptr;
    std::vector<dcrt_material> hostMaterials;
    std::vector<dcrt_light> hostLights;
    // The direction cells of a plan.cellsRes scene: the device buffers hold any table of that
    // resolution; the host copies of the geometry rebuild it when the lights change (RebuildShadowCells).
    uint64_t* dCells = nullptr;
    uint32_t* dCellLeaves = nullptr;
    ShadowCells cells;
    std::vector<dcrt_bvh_node> cellNodes;
    std::vector<dcrt_vertex> cellVertices;
    std::vector<uint32_t> cellTriangles;
    std::vector<dcrt_float4x3> cellTransforms;
    uint32_t megaResident = 0;         // persistent megakernel grid
    uint32_t viewResident = 0;         // persistent view_kernel grid
    uint32_t viewResidentOpacity = 0;  // the same for the ALLOW_ANYHIT_SHADER variant

    // ---- film, its rows and the sample textures ----
    DeviceGroup filmAllocs, sampleAllocs, rowAllocs;
    Film film{};
    uint32_t filmW = 0, filmH = 0;
    uint32_t rowCount = 0;             // rows this tracer path-traces (film.rowY)
    uint32_t bandCount = 0;            // ceil(rowCount / 8): block rows of an image
    dcrt_film_partition partition{ 1, 0, 64, 0 };
    std::vector<uint32_t> bands;       // explicit film bands [y0, y1) pairs (dcrt_tracer_set_film_bands), or empty
    uint32_t sampleImages = 0;         // images the sample textures hold (batch capacity)
    uint32_t batchImages = 0;          // RenderImages batch size (0: automatic)
    uint32_t lastSlot = 0;             // sample slot of the last completed image
    uint32_t seedStride = 1;           // RenderImages: image k has frame seed first + k * seedStride
    bool keptSlots = false;            // the last RenderImages left image k's samples in slot k (no film pass)
    uint32_t keptImages = 0;
    SampleOut* dSampleOut = nullptr;   // MATERIAL's copy of the sample pointers (EnsureSamples)
    SampleOut hSampleOut = {};
    void** dSourceLists = nullptr;     // accumulate_images: device copies of the caller's pointer lists
    DeviceGroup sourceAllocs;
    uint32_t sourceCap = 0;
    FilterConsts* dFilter = nullptr;
    Pinned<FilterConsts> hFilter;      // its staging
    dcrt_filter_params lastFilter{};   // the reconstruction filter on the device (UploadFilter)
    bool hasFilter = false;
    uint32_t filmImages = 0;           // images convolved into the film since the last clear
    bool filmClearTrigger = false;

    // ---- the image in flight and the captured graphs ----
    dcrt_frame_params frame{};
    bool hasFrame = false;
    bool newImage = true;
    bool imageComplete = false;
    uint32_t parity = 0;
    uint64_t imagesCompleted = 0;      // since the last ResetStats (counters())
    bool capturing = false;            // LaunchIteration is being captured into a graph (no host annotations)
    // graphs of `iters` iterations (even), rebuilt when launch parameters change
    struct GraphCache {
        hipGraphExec_t exec = nullptr;
        uint32_t iters = 0;
    } graphs[3];   // unsequenced (Render), sequenced (RenderImages), sequenced tail chunks
    Pinned<uint32_t, 8> hStop;         // [4][2]: Globals::stopped, imagesDone per poll
    hipEvent_t stopEvents[4] = {};

    // ---- instrumentation ----
    bool instrCounters = false;
    bool extTiming = false;
    unsigned long long* dInstr = nullptr;   // [8]
    bool rowProbe = false;             // the row-cost probe: MATERIAL's PROBE variant counts rays per film row
    uint32_t* dRowRays = nullptr;      // [filmH] (rowAllocs: follows the film)
    // timed launches (ext_timing): start / stop event pairs and the kernel each pair timed
    enum TimedKind : uint8_t { kTimedCast = 0, kTimedMaterial = 1, kTimedControl = 2, kTimedFilm = 3, kTimedKinds = 4 };
    std::vector<hipEvent_t> events;
    std::vector<uint8_t> eventKinds;   // per pair
    size_t eventsUsed = 0;
    double kindMs[kTimedKinds] = {};
    uint64_t kindLaunches[kTimedKinds] = {};

    // ---- the film denoiser (dcrt_tracer_render_guides / dcrt_tracer_denoise*): two guide films and the
    // denoised image follow the film (filmAllocs); the filter and its working images are `denoiser` ----
    float4* guideNormal = nullptr;
    float4* guideAlbedo = nullptr;
    float4* denoised = nullptr;
    bool guidesRendered = false, hasDenoised = false;
    FilmDenoiser denoiser;

    // ---- the film noise estimate (dcrt_tracer_set_convergence / dcrt_tracer_noise*): the half film takes
    // every other image of the film's (even film image counts); the maps of the last dcrt_tracer_noise
    // follow the film; the kernels and their working buffers are `noiseEstimator` ----
    bool convergence = false;
    float4* halfFilm = nullptr;
    DeviceGroup halfAllocs, noiseMapAllocs;
    float *noisePixelMap = nullptr, *noiseTileMap = nullptr;
    bool hasNoiseMaps = false;
    NoiseEstimator noiseEstimator;

    // ---- adaptive sampling (dcrt_tracer_set_adaptive): one flag per 8x8 block of the film and the
    // ascending list of the active ones, both with room for every block (adaptiveAllocs: they
    // follow the film's size); RenderImages' kernels get `dBlockList` and the list's length as
    // blocksPerImage, every other launch the plain film. The mask, compaction and fill kernels
    // are `blockSampler` ----
    bool adaptive = false;
    DeviceGroup adaptiveAllocs;
    uint32_t* dBlockFlags = nullptr;
    uint32_t* dBlockList = nullptr;
    BlockSampler blockSampler;
    uint32_t blockTotal = 0;           // blocks of the film: blocksX * ceil(H / 8)
    uint32_t listCount = 0;            // active blocks
    uint32_t listPixels = 0;           // their pixels inside the film: the paths an image starts
    bool inactiveFilled = false;       // every slot's inactive pixels hold the sentinel sample
    bool listFrame = false;            // BeginImage: the frame constants' blocksPerImage is the list's length
    uint64_t pathsSkipped = 0;         // pixels the lists left out since the last ResetStats (counters())

    // ---- firefly re-weighting (dcrt_tracer_set_firefly): the K cascade films and the re-weighted image of
    // the last resolve (cascadeAllocs: they follow the film's size, only while the feature is on); the
    // tracer's own film passes launch the cascade pass beside them (LaunchFilm). The kernels' launches and
    // their event marks are `fireflyFilter` ----
    bool firefly = false;
    dcrt_firefly_params fireflyParams{};
    FireflyConsts fireflyConsts{};
    DeviceGroup cascadeAllocs;
    CascadeFilms cascades{};
    float4* reweighted = nullptr;
    bool hasReweighted = false;
    FireflyFilter fireflyFilter;

    ~dcrt_tracer();
    int Create(const dcrt_tracer_config& cfg);
    int BuildLuts();
    // scene
    int UploadScene(const dcrt_flat_scene& s);
    int UploadArrays(const dcrt_flat_scene& s, std::vector<uint32_t>* identity);
    int PlanCast(const dcrt_flat_scene& s, const UploadKnobs& k, const std::vector<uint32_t>& identity);
    int PlanFlatCast(const dcrt_flat_scene& s, const UploadKnobs& k);
    int SizeGrids(const UploadKnobs& k);
    int CastOccupancy(CastFn k, size_t lds, int* out);
    int PlanMaterial(const MaterialPlan* before, MaterialPlan* out);
    int ApplyMaterialPlan(const MaterialPlan& p);
    int BuildEnvTable();
    int BuildLightTable();
    int LightWeights();
    int CubeMeanLuminance();
    int SetLightSampling(int mode);
    int SetEnvSampling(int mode);
    int BuildDielRows();
    int RederiveShading();
    int UpdateMaterials(const dcrt_material* materials, uint32_t count);
    int UpdateLights(const dcrt_light* lights, uint32_t count);
    int UpdateInstanceFlags(const uint32_t* flags, uint32_t count);
    int RebuildShadowCells();
    int CheckFrameLights() const;
    // film
    int SetFrame(const dcrt_frame_params& p);
    int SetPartition(const dcrt_film_partition& p);
    int SetBands(const uint32_t* b, uint32_t count, uint32_t halo);
    int EnsureFilm(uint32_t w, uint32_t h);
    int BuildRows();
    int UploadSampleOut();
    int SetRowProbe(bool on);
    int EnsureSamples(uint32_t images);
    int CheckHalo(float radius) const;
    // The sample textures' slot 0 holds another image now (a view or guide image): no kept slots, no sentinel fill
    void SlotZeroOverwritten()
    {
        keptSlots = false;
        inactiveFilled = false;
        lastSlot = 0;
    }
    int UploadFilter(const dcrt_filter_params& f);
    int ClearFilm();
    int LaunchFilm(const Film& target, float4* half, bool timed, uint32_t images, const Globals* guard, const float2* const* posList,
                   const float4* const* valList, uint32_t firstIndex);
    int LaunchFilm(uint32_t images, const Globals* guard, const float2* const* posList, const float4* const* valList,
                   uint32_t firstIndex)
    {
        CHECKED(LaunchFilm(film, convergence ? halfFilm : nullptr, extTiming && !capturing, images, guard, posList, valList, firstIndex));
        // firefly re-weighting: the cascades take the same images (timed outside the graph-shaped iteration only:
        // the in-graph pass returns at once unless a batch completed)
        if (firefly)
            return fireflyFilter.Cascade(stream, extTiming && !guard, FilmGrid(), film, cascades, fireflyConsts, dFilter, images, guard, posList,
                                         valList);
        return DCRT_OK;
    }
    int AddFilm(float4* dst, const void* src);
    int ReadImage(const float4* image, float* out);
    int NeedHalfFilm() const;
    int AccumulateImages(const void* const* pos, const void* const* val, uint32_t count, const dcrt_filter_params& filter);
    int Accumulate(const dcrt_filter_params& filter);
    // rendering
    uint32_t AutoBatch(uint32_t count) const;
    int BeginImage();
    int LaunchIteration(uint32_t par, bool timed, bool sequenced);
    int LaunchGraph(bool sequenced, uint32_t iters);
    int BuildGraph(bool sequenced, uint32_t iters);
    int PrepareImages(uint32_t count);
    int RunIterations(uint32_t n);
    int ReadCompletion(bool* complete);
    int Render(uint32_t maxIterations);
    int LaunchView();
    int LaunchView(uint32_t type, const Film& target);
    int RenderImages(uint32_t firstSeed, uint32_t count, const dcrt_filter_params& filter, uint32_t stride = 1,
                     bool convolve = true);
    // denoiser, noise estimate
    int EnsureGuides();
    int RenderGuides(uint32_t firstSeed, uint32_t count);
    int SetConvergence(bool on);
    int SetFirefly(const dcrt_firefly_params* p);
    int AllocCascades();
    int AllocCascadesOrOff();
    bool Partitioned() const { return partition.world_size > 1 || !bands.empty(); }
    int NoiseOwn(float threshold, dcrt_noise_stats* out);
    // render_converged, and with `adaptiveCall` render_adaptive
    struct AdaptiveCall {
        uint32_t margin;                 // 0xFFFFFFFF: the filter's window rows
        dcrt_adaptive_report* report;    // filled in once the call has started on every block, or null
    };
    int RenderConverged(uint32_t firstSeed, const dcrt_converge_params& p, const dcrt_filter_params& filter, dcrt_noise_stats* outStats,
                        int* outConverged, const AdaptiveCall* adaptiveCall = nullptr);
    // adaptive sampling
    int SetAdaptive(bool on);
    int AllocBlockList();
    int ResetBlockList();
    int SetSampleBlocks(const uint32_t* blocks, uint32_t count);
    int GetSampleBlocks(uint32_t* out, uint32_t capacity, uint32_t* outCount);
    int UpdateSampleBlocks(float threshold, uint32_t margin, uint32_t* outActive);
    int FillInactive();

    // One device array of the scene: allocated (sceneAllocs), filled from `src` and counted in `*counted`
    template <typename T>
    int Upload(T** dst, const T* src, size_t count, uint64_t* counted, size_t capacity = 0)
    {
        T* p = nullptr;
        CHECKED(sceneAllocs.Alloc(&p, std::max(count, capacity)));
        if (count && src) {
            HIPCHECK(hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, stream));
            *counted += count * sizeof(T);
        }
        *dst = p;
        return DCRT_OK;
    }
    int TimedPair(TimedKind kind, hipEvent_t* e0, hipEvent_t* e1)
    {
        while (events.size() < eventsUsed + 2) {
            hipEvent_t e;
            HIPCHECK(hipEventCreate(&e));
            events.push_back(e);
        }
        eventKinds.resize(events.size() / 2);
        eventKinds[eventsUsed / 2] = kind;
        *e0 = events[eventsUsed++];
        *e1 = events[eventsUsed++];
        return DCRT_OK;
    }
    int CollectTimes()   // fold the recorded pairs into kindMs / kindLaunches
    {
        for (size_t i = 0; i + 1 < eventsUsed; i += 2) {
            float e = 0.0f;
            HIPCHECK(hipEventElapsedTime(&e, events[i], events[i + 1]));
            kindMs[eventKinds[i / 2]] += e;
            ++kindLaunches[eventKinds[i / 2]];
        }
        eventsUsed = 0;
        return DCRT_OK;
    }
    void InvalidateGraph()
    {
        for (const GraphCache& g : graphs)
            if (g.exec) { ++uploadStats.graph_invalidations; break; }   // (a drop of captured graphs, not of none)
        for (GraphCache& g : graphs) {
            if (g.exec) (void)hipGraphExecDestroy(g.exec);
            g.exec = nullptr;
            g.iters = 0;
        }
    }
    // film_kernel: one 16x16 tile per workgroup (grid-stride beyond the cap)
    uint32_t FilmGrid() const
    {
        const uint32_t T = (uint32_t)kFilmTile;
        return std::max<uint32_t>(1u, std::min<uint32_t>(((filmW + T - 1) / T) * ((filmH + T - 1) / T), 8u * kMaxPersistentBlocks * (256u / kFilmThreads)));
    }
};

// (the members free what they own once this has made the device current, waited for the stream and dropped the
// graphs; `streamEnd` then destroys the stream)
dcrt_tracer::~dcrt_tracer()
{
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    InvalidateGraph();
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    for (hipEvent_t e : stopEvents) if (e) (void)hipEventDestroy(e);
}

int dcrt_tracer::Create(const dcrt_tracer_config& cfg)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
        SetLastError("no HIP device visible");
        return DCRT_E_NO_DEVICE;
    }
    device = cfg.device;
    if (device < 0 || device >= count) { SetLastError("invalid device ordinal"); return DCRT_E_INVALID_ARG; }
    HIPCHECK(hipSetDevice(device));
    if (cfg.stream) {
        stream = (hipStream_t)cfg.stream;
    } else {
        HIPCHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        ownsStream = true;
    }
    poolSize = cfg.path_pool_size ? cfg.path_pool_size : kDefaultPoolSize;
    // whole CONTROL workgroups of whole waves, and at least one CONTROL workgroup per
    // pixel-block shard (workgroup b claims the blocks of shard b % kShards)
    poolSize = std::max<uint32_t>(poolSize, kControlBlock * kShards);
    poolSize = (poolSize + kControlBlock - 1) / kControlBlock * kControlBlock;
    iterationsPerRender = cfg.iterations_per_render ? cfg.iterations_per_render : kDefaultIterations;
    debugRng = cfg.debug_rng != 0;
    knobs = ReadCreateKnobs();
    // pool arrays are addressed through 32-bit byte offsets (slot(): at most 16 B per slot), and
    // one parity's extension-ray records and path-state halves (ext_rec(), state_at(): 32 B at
    // position q = shard * recCap + entry) as well; this check bounds the pool at 2^26 slots,
    // the recCap check below keeps recCap * kShards * 32 B within 4 GiB
    if ((uint64_t)poolSize * 64u > (1ull << 32)) {
        SetLastError("path pool too large: at most 2^26 slots (32-bit pool offsets)");
        return DCRT_E_LIMIT;
    }
    // WavefrontPathTracer.cpp:120-264 (SoA instead of AoS)
    const size_t P = poolSize;
    CHECKED(poolAllocs.Alloc(&pool.hit, 2 * P));   // 2 float4 per extension-queue item
    CHECKED(poolAllocs.Alloc(&pool.pixel, P));
    CHECKED(poolAllocs.Alloc(&pool.flags, P));
    CHECKED(poolAllocs.Alloc(&pool.extOpacity, P));
    CHECKED(poolAllocs.Alloc(&pool.shadowOpacity, P));
    // the extension and finish queues: one per iteration parity (extRecs / finRecs)
    static_assert(kControlBlock == 256u && kMaterialBlock == 256u, "queue capacities assume 256-slot workgroups");
    const uint32_t V = poolSize / 256u;   // virtual workgroups (256 slots / items each)
    {
        // One workgroup per virtual workgroup would make a pass over an idle or nearly empty
        // pool cost the dispatch of P / 256 workgroups (2^26 slots: 262144 workgroups,
        // CONTROL 91 us and MATERIAL 57 us with nothing to do). The grids hold what is
        // resident instead, a multiple of kShards (= kFinShards), so a workgroup's virtual
        // workgroups all belong to its own shard: vb mod kShards = blockIdx.x mod kShards
        // (knobs.controlGridMul / materialGridMul x resident; 0: one workgroup per virtual workgroup).
        hipDeviceProp_t prop;
        HIPCHECK(hipGetDeviceProperties(&prop, device));
        if (prop.maxSharedMemoryPerMultiProcessor > 0) g_ldsPerCU = prop.maxSharedMemoryPerMultiProcessor;
        int cPerCU = 0, mPerCU = 0;
        HIPCHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&cPerCU, control_kernel, (int)kControlBlock, 0));
        HIPCHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&mPerCU, MaterialPlan{}.Kernel(false, false), (int)kMaterialBlock, 0));   // (the any-scene variant without an LDS copy)
        auto resident = [&](int perCU, uint32_t mul) {
            if (mul == 0) return V;
            const uint64_t r = (uint64_t)std::max(1, perCU) * (uint64_t)std::max(1, prop.multiProcessorCount) * mul;
            const uint32_t g = (uint32_t)std::max<uint64_t>(kShards, r / kShards * kShards);
            return std::min(g, V);   // (= V: one round, any V)
        };
        controlGrid = resident(cPerCU, knobs.controlGridMul);
        materialGrid = resident(mPerCU, knobs.materialGridMul);
        static_assert(kFinShards == kShards, "MATERIAL's grid is a multiple of both shard counts");
    }
    // The extension queue's shard s receives the new paths of CONTROL's virtual workgroups
    // vb = s mod kShards and the continuing paths of MATERIAL's (at most 256 each): at most
    // 2 ceil(V / kShards) 256 entries
    pool.recCap = std::min<uint32_t>(poolSize, 2u * ((V + kShards - 1) / kShards) * 256u);
    // (32-bit byte offsets address one parity's records: at most 2^32 bytes, e.g. 2^26 slots)
    if ((uint64_t)pool.recCap * kShards * 32u > (1ull << 32)) { SetLastError("path pool too large for the extension-queue records"); return DCRT_E_LIMIT; }
    CHECKED(poolAllocs.Alloc(&extRecs, (size_t)pool.recCap * kShards * 2 * 2));
    // the paths' state records and their shadow rays' results, at the same positions
    CHECKED(poolAllocs.Alloc(&stateRecsA, (size_t)pool.recCap * kShards * 2));
    CHECKED(poolAllocs.Alloc(&stateRecsB, (size_t)pool.recCap * kShards * 2));
    CHECKED(poolAllocs.Alloc(&shadowHits, (size_t)pool.recCap * kShards * 2));
    // the shadow queue (filled and cast within one iteration): records + path slots
    CHECKED(poolAllocs.Alloc(&pool.shRec, (size_t)pool.recCap * kShards * 2));
    CHECKED(poolAllocs.Alloc(&pool.shadowQueue, (size_t)pool.recCap * kShards));

    // MATERIAL's virtual workgroup vb appends the paths it ends with a shadow ray pending to
    // finish shard vb mod kFinShards
    pool.finCap = ((V + kFinShards - 1) / kFinShards) * kMaterialBlock;
    CHECKED(poolAllocs.Alloc(&finRecs, (size_t)pool.finCap * kFinShards * 2));
    CHECKED(poolAllocs.Alloc(&finHits, (size_t)pool.finCap * kFinShards * 2));
    pool.size = poolSize;
    CHECKED(poolAllocs.Alloc(&dFrame, 1));
    CHECKED(poolAllocs.Alloc(&dSampleOut, 1));
    CHECKED(poolAllocs.Alloc(&dCounters, 2));
    CHECKED(poolAllocs.Alloc(&dGlobals, 1));
    CHECKED(poolAllocs.Alloc(&dInstr, 8));
    CHECKED(poolAllocs.Alloc(&dLuts, 1));
    HIPCHECK(hipMemsetAsync(dCounters, 0, 2 * sizeof(Counters), stream));
    HIPCHECK(hipMemsetAsync(dGlobals, 0, sizeof(Globals), stream));
    HIPCHECK(hipMemsetAsync(dInstr, 0, 8 * sizeof(unsigned long long), stream));
    CHECKED(hPoolIdle.Alloc());
    CHECKED(poolAllocs.Alloc(&dFilter, 1));
    CHECKED(hFilter.Alloc());
    CHECKED(hStop.Alloc());
    for (hipEvent_t& e : stopEvents) HIPCHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    CHECKED(BuildLuts());
    HIPCHECK(hipStreamSynchronize(stream));
    return DCRT_OK;
}

// BxDFTexturesBuilding::Build (BxDFTexturesBuilding.cpp:106-475) as three
// integration launches + one conversion/average launch.
// The LUTs depend on nothing but the integration constants, so a process integrates
// them once per device (≈ 0.24 s of GPU time) and every further tracer copies them
// (the cache's device copies live until the process exits).
static std::mutex g_lutMutex;
static std::map<int, dcrt_bxdf_luts*> g_lutCache;

int dcrt_tracer::BuildLuts()
{
    std::lock_guard<std::mutex> lock(g_lutMutex);
    auto hit = g_lutCache.find(device);
    if (hit != g_lutCache.end()) {
        HIPCHECK(hipMemcpyAsync(dLuts, hit->second, sizeof(dcrt_bxdf_luts), hipMemcpyDeviceToDevice, stream));
        HIPCHECK(hipStreamSynchronize(stream));
        return DCRT_OK;
    }
    DeviceGroup scratch;
    float *brdf = nullptr, *brdfd = nullptr, *bsdf = nullptr;
    CHECKED(scratch.Alloc(&brdf, DCRT_LUT_BRDF_COUNT));
    CHECKED(scratch.Alloc(&brdfd, DCRT_LUT_BRDF_DIELECTRIC_COUNT));
    CHECKED(scratch.Alloc(&bsdf, DCRT_LUT_BSDF_COUNT));
    hipLaunchKernelGGL(lut_integrate_kernel, dim3((DCRT_LUT_BRDF_COUNT + 63) / 64), dim3(64), 0, stream, 0, (uint32_t)DCRT_LUT_BRDF_COUNT, brdf);
    hipLaunchKernelGGL(lut_integrate_kernel, dim3((DCRT_LUT_BRDF_DIELECTRIC_COUNT + 63) / 64), dim3(64), 0, stream, 1,
                       (uint32_t)DCRT_LUT_BRDF_DIELECTRIC_COUNT, brdfd);
    hipLaunchKernelGGL(lut_integrate_kernel, dim3((DCRT_LUT_BSDF_COUNT + 63) / 64), dim3(64), 0, stream, 2, (uint32_t)DCRT_LUT_BSDF_COUNT, bsdf);
    hipLaunchKernelGGL(lut_finalize_kernel, dim3((DCRT_LUT_BRDF_DIELECTRIC_COUNT + 255) / 256), dim3(256), 0, stream, brdf, brdfd, bsdf, dLuts);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(stream));
    scratch.Free();
    dcrt_bxdf_luts* cached = nullptr;
    if (hipMalloc((void**)&cached, sizeof(dcrt_bxdf_luts)) == hipSuccess) {
        if (hipMemcpy(cached, dLuts, sizeof(dcrt_bxdf_luts), hipMemcpyDeviceToDevice) == hipSuccess) g_lutCache[device] = cached;
        else (void)hipFree(cached);
    }
    return DCRT_OK;
}

// What UploadScene and the partial updates ask of the three arrays an edit replaces.
static int ValidateMaterials(const dcrt_material* materials, uint32_t count)
{
    if (!materials || count == 0) { SetLastError("no materials"); return DCRT_E_INVALID_ARG; }
    return DCRT_OK;
}
static int ValidateLights(const dcrt_light* lights, uint32_t count)
{
    if (count > DCRT_MAX_LIGHT_COUNT) { SetLastError("more than 5000 lights"); return DCRT_E_LIMIT; }
    if (!lights && count) { SetLastError("no light array"); return DCRT_E_INVALID_ARG; }
    return DCRT_OK;
}
static int ValidateInstanceFlags(const uint32_t* flags, uint32_t count)
{
    if (!flags || count == 0) { SetLastError("no instance flags"); return DCRT_E_INVALID_ARG; }
    return DCRT_OK;
}

// The rule every addition to MATERIAL's LDS is judged by (the fused variant's cells, the rows, the frames):
// `keeps` is cleared unless the variant keeps its resident workgroups per CU -- by registers and by LDS -- when
// the addition takes it from `before` (kernel, dynamic LDS bytes) to `after`, within 64 KiB of LDS (`cap`).
static int KeepsResident(MaterialFn before, size_t a, MaterialFn after, size_t b, bool cap, bool* keeps)
{
    int ra = 0, rb = 0;
    CHECKED(ResidentPerCU((const void*)before, kMaterialBlock, a, &ra));
    CHECKED(ResidentPerCU((const void*)after, kMaterialBlock, b, &rb));
    *keeps = *keeps && rb >= ra && rb > 0 && (!cap || b <= 65536);
    return DCRT_OK;
}

// The MaterialPlan of the scene as it stands (UploadScene once the grids are sized; every edit of the
// materials or the lights) from the shading knobs -- read here, once: tests set them between uploads --
// hostMaterials, hostLights, the scene's counts and cube, the CastPlan and the tables' buffers. Five
// decisions in this order, each judged against what the earlier ones settled. `before`: the plan in
// force (its drain grid stands while the variant does: no query), or null.
int dcrt_tracer::PlanMaterial(const MaterialPlan* before, MaterialPlan* out)
{
    const ShadingKnobs k = ReadShadingKnobs();
    const DeviceScene& scene = plan.scene;
    const uint32_t T = scene.triangleCount, I = scene.instanceCount;
    const uint32_t M = (uint32_t)hostMaterials.size(), L = (uint32_t)hostLights.size();
    MaterialPlan p;
    // 1. the variant: the smallest compiled one whose capabilities cover the scene
    uint32_t sceneCaps = scene.envCube ? kCapEnvCube : 0u;   // what the scene uses (kCap* of dscene.h)
    bool readsRows = false;   // (a plastic material, its roughness not under the checkerboard)
    for (const dcrt_material& m : hostMaterials) {
        const uint32_t type = m.flags & DCRT_MATERIAL_FLAG_TYPE_MASK;
        sceneCaps |= type <= DCRT_MATERIAL_TYPE_THIN_DIELECTRIC ? (1u << type) : kCapAll;
        if (m.flags & DCRT_MATERIAL_FLAG_MULTISCATTERING) sceneCaps |= kCapMultiscatter;
        if (m.albedo_texture_index != -1 || (m.flags & DCRT_MATERIAL_FLAG_ROUGHNESS_TEXTURE)) sceneCaps |= kCapTextures;
        readsRows = readsRows || (type == DCRT_MATERIAL_TYPE_PLASTIC && !(m.flags & DCRT_MATERIAL_FLAG_ROUGHNESS_TEXTURE));
    }
    for (const dcrt_light& l : hostLights) sceneCaps |= (l.flags & 0xFu) << kCapLightShift;
    p.caps = (sceneCaps & ~kCapOpaqueDelta) == 0u && !k.materialGeneric ? kCapOpaqueDelta : kCapAll;
    // (the cube's table, where the mode is on and one stands, for a scene with an environment light: its own any-scene variant)
    if (envSampling == DCRT_ENV_SAMPLING_IMPORTANCE && dEnvProb && scene.envCube && (sceneCaps & kCapLightEnv)) {
        p.caps = kCapAllEnvImportance;
        p.envProb = dEnvProb;
        p.envRowCdf = dEnvRowCdf;
        p.envMarginal = dEnvMarginal;
    }
    // (the light table, where the mode is on and one stands: the one any-scene variant that reads it, and the cube's
    // table through the same variant if that stands too)
    if (lightSampling == DCRT_LIGHT_SAMPLING_POWER && lightTable.prob) {
        p.caps = kCapAllLightTable;
        p.lightProb = lightTable.prob;
        p.lightCdf = lightTable.cdf;
        p.triBase = lightTable.triBase;
        p.triProb = lightTable.triProb;
        p.triCdf = lightTable.triCdf;
        p.lightTableCount = L;
    }
    // 2. the LDS scene copy within the knob's budget: the whole shading data (mode 1), else all but the triangles (mode 2)
    const bool counts = T > 0 && T < (1u << 20) && I < (1u << 20) && M < (1u << 20) && L < (1u << 20);
    const uint64_t whole = material_lds_layout(T, I, M, L, 0u, false, 0u, false).shading;
    const uint64_t rest = material_lds_layout(0u, I, M, L, 0u, false, 0u, false).shading;
    p.mode = !counts ? 0u : whole <= k.materialLds ? 1u : (k.materialLdsPartial && rest <= k.materialLds ? 2u : 0u);
    p.materials = p.mode ? M : 0u;
    p.lights = p.mode ? L : 0u;
    // (the layout with so many materials' rows, the frames and the cells: the counts are the copy's)
    auto layout = [&](uint32_t rowMaterials, bool frames, bool cells) {
        return p.mode ? material_lds_layout(p.mode == 1u ? T : 0u, I, M, L, rowMaterials, frames, plan.sceneFlat.cachedNodes, cells) : MaterialLds{};
    };
    // (the layout `bigger` is taken if neither variant the plan launches loses a resident workgroup to it)
    auto grow = [&](const MaterialLds& bigger, bool* taken) {
        *taken = true;
        for (const bool fused : { false, true })
            if (!fused || p.lds.cells) CHECKED(KeepsResident(p.Kernel(false, fused), p.lds.Bytes(fused), p.Kernel(false, fused), bigger.Bytes(fused), true, taken));
        if (*taken) p.lds = bigger;
        return (int)DCRT_OK;
    };
    p.lds = layout(0u, false, false);
    // 3. the fused variant for the flat cast's scene: the cells go behind the whole shading copy (mode 1) if
    // they fit the same budget again and cost no resident workgroup against the unfused variant they replace
    // (sized for any table of the scene: whether one stands is the launch's question, FusedShadow). No 64 KiB
    // cap: copy and cells are each within the budget, so up to a budget of 32 KiB (the default is 16) the sum
    // cannot pass it; with the knob raised beyond, the occupancy query alone decides, as it always has.
    p.fusedMask = k.fusedShadow > 1u ? k.fusedShadow - 1u : 0u;
    if (k.fusedShadow && plan.flat && plan.cellsRes && p.mode == 1u) {
        const MaterialLds fused = layout(0u, false, true);
        bool fits = fused.cells <= k.materialLds;
        if (fits) CHECKED(KeepsResident(p.Kernel(false, false), p.lds.Bytes(false), p.Kernel(false, true), fused.Bytes(true), false, &fits));
        if (fits) p.lds = fused;
    }
    // 4. the rows: only where a material reads them (a scene without one keeps its LDS to the byte); in the LDS
    // copy where that costs neither variant a resident workgroup, else the kernels read them from global memory
    p.tables = k.shadingTables;
    if (!dDielRows || !readsRows) p.tables &= ~kTableDielRows;
    bool taken = false;
    if ((p.tables & kTableDielRows) && p.mode != 0u) CHECKED(grow(layout(M, false, p.lds.cells != 0u), &taken));
    // 5. the frames: in the whole-scene LDS copy of the delta-only variant under the same rule, or not at all
    // (the any-scene variant takes a register more with the table in it, and spills it)
    if (!dTriFrames || p.mode != 1u || caps_any_scene(p.caps)) p.tables &= ~kTableFrames;
    if (p.tables & kTableFrames) {
        CHECKED(grow(layout(p.lds.rows ? M : 0u, true, p.lds.cells != 0u), &taken));
        if (!taken) p.tables &= ~kTableFrames;
    }
    p.earlyFinish = caps_early_finish(p.caps) ? k.earlyFinish : 0u;
    p.dielRows = (p.tables & kTableDielRows) ? dDielRows : nullptr;
    p.triFrames = (p.tables & kTableFrames) ? dTriFrames : nullptr;
    // drain_kernel's grid: resident workgroups of the variant's drain kernel, launched like the casts
    if (before && before->caps == p.caps) {
        p.drainGrid = before->drainGrid;
    } else {
        int perCU = 0;
        CHECKED(ResidentPerCU((const void*)p.DrainKernel(), plan.block, plan.ldsWholeStack, &perCU));
        p.drainGrid = (uint32_t)std::max(1, perCU) * cuCount;
    }
    *out = p;
    return DCRT_OK;
}

// `p` in force: written to all the DeviceScene copies (those not in use are rewritten with the next
// upload), and a scene's rows rebuilt from the materials and the LUTs as they stand on the device
int dcrt_tracer::ApplyMaterialPlan(const MaterialPlan& p)
{
    material = p;
    for (DeviceScene* d : { &plan.scene, &plan.sceneFlat, &plan.sceneRing }) material.Apply(d);
    if (material.tables & kTableDielRows) CHECKED(BuildDielRows());
    return DCRT_OK;
}

// The rows of the materials and the LUTs as they stand on the device (a scene with rows; set_luts needs it alone)
int dcrt_tracer::BuildDielRows()
{
    const uint32_t materialCount = (uint32_t)hostMaterials.size(), n = materialCount * kDielRowFloats;
    hipLaunchKernelGGL(build_diel_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (const dcrt_material*)dMaterials, materialCount,
                       (const uint16_t*)dLuts->brdf_dielectric, (const uint16_t*)dLuts->brdf_dielectric_avg, dDielRows);
    HIPCHECK(hipGetLastError());
    return DCRT_OK;
}

// After an update replaced the materials or the lights: the plan again, and the captured graphs
// dropped exactly when something they bake in changed (MaterialPlan::BakedEquals).
int dcrt_tracer::RederiveShading()
{
    MaterialPlan next;
    CHECKED(PlanMaterial(&material, &next));
    if (next.fusedMask != material.fusedMask) newImage = true;   // (the frame constants carry it)
    const bool baked = next.BakedEquals(material);
    CHECKED(ApplyMaterialPlan(next));
    if (!baked) {
        HIPCHECK(hipStreamSynchronize(stream));
        InvalidateGraph();
    }
    return DCRT_OK;
}

int dcrt_tracer::UpdateMaterials(const dcrt_material* materials, uint32_t count)
{
    Annotation an("UpdateMaterials");
    if (!hasScene) { SetLastError("no scene uploaded"); return DCRT_E_NO_SCENE; }
    CHECKED(ValidateMaterials(materials, count));
    if (count != hostMaterials.size()) { SetLastError("material count differs from the uploaded scene's"); return DCRT_E_INVALID_ARG; }
    // (the host copy is the copy's source: the caller's array is free on return)
    HIPCHECK(hipStreamSynchronize(stream));
    hostMaterials.assign(materials, materials + count);
    HIPCHECK(hipMemcpyAsync(dMaterials, hostMaterials.data(), (size_t)count * sizeof(dcrt_material), hipMemcpyHostToDevice, stream));
    uploadStats.shading_bytes += (uint64_t)count * sizeof(dcrt_material);
    ++uploadStats.material_updates;
    CHECKED(RederiveShading());
    HIPCHECK(hipStreamSynchronize(stream));
    return DCRT_OK;
}

int dcrt_tracer::UpdateLights(const dcrt_light* lights, uint32_t count)
{
    Annotation an("UpdateLights");
    if (!hasScene) { SetLastError("no scene uploaded"); return DCRT_E_NO_SCENE; }
    CHECKED(ValidateLights(lights, count));
    HIPCHECK(hipStreamSynchronize(stream));
    if (count) hostLights.assign(lights, lights + count);
    else hostLights.clear();
    if (count) HIPCHECK(hipMemcpyAsync(dLights, hostLights.data(), (size_t)count * sizeof(dcrt_light), hipMemcpyHostToDevice, stream));
    uploadStats.shading_bytes += (uint64_t)count * sizeof(dcrt_light);
    ++uploadStats.light_updates;
    if (lightSampling == DCRT_LIGHT_SAMPLING_POWER) CHECKED(BuildLightTable());
    CHECKED(RederiveShading());
    CHECKED(RebuildShadowCells());
    HIPCHECK(hipStreamSynchronize(stream));
    return DCRT_OK;
}

int dcrt_tracer::UpdateInstanceFlags(const uint32_t* flags, uint32_t count)
{
    Annotation an("UpdateInstanceFlags");
    if (!hasScene) { SetLastError("no scene uploaded"); return DCRT_E_NO_SCENE; }
    CHECKED(ValidateInstanceFlags(flags, count));
    if (count != plan.scene.instanceCount) { SetLastError("instance count differs from the uploaded scene's"); return DCRT_E_INVALID_ARG; }
    // nothing is derived from the flags; the copy is done on return (the caller's array is free)
    HIPCHECK(hipMemcpyAsync(dInstanceFlags, flags, (size_t)count * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    uploadStats.shading_bytes += (uint64_t)count * sizeof(uint32_t);
    ++uploadStats.instance_flag_updates;
    CHECKED(RebuildShadowCells());   // (the flags enter no mask today: the any-hit kernels keep the BVH)
    return DCRT_OK;
}

// The direction-cell table for the current lights (UploadScene, UpdateLights, UpdateInstanceFlags):
// built on the host from the copies UploadScene kept, written into the buffers it allocated. A moved
// light changes the buffers' contents only; a table that appears or goes changes the kernel and its
// DeviceScene, so the captured graphs are dropped.
int dcrt_tracer::RebuildShadowCells()
{
    if (!plan.flat || !plan.cellsRes) return DCRT_OK;
    DeviceScene& sceneFlat = plan.sceneFlat;
    dcrt_flat_scene s{};
    s.vertices = cellVertices.data();
    s.vertex_count = (uint32_t)cellVertices.size();
    s.triangles = cellTriangles.data();
    s.triangle_count = (uint32_t)(cellTriangles.size() / 3);
    s.instance_transforms = cellTransforms.data();
    s.instance_count = (uint32_t)(cellTransforms.size() / 2);
    s.lights = hostLights.data();
    s.light_count = (uint32_t)hostLights.size();
    dcrt::BuildShadowCells(cellNodes.data(), cellNodes.size(), s, plan.cellsRes, &cells);
    const uint32_t before = sceneFlat.shadowRes;
    HIPCHECK(hipStreamSynchronize(stream));
    if (cells.resolution) {
        HIPCHECK(hipMemcpyAsync(dCells, cells.cells.data(), cells.cells.size() * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
        HIPCHECK(hipMemcpyAsync(dCellLeaves, cells.leafWords.data(), dcrt::kCellWords * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        HIPCHECK(hipStreamSynchronize(stream));
    }
    sceneFlat.shadowCells = cells.resolution ? dCells : nullptr;
    sceneFlat.shadowLeaves = cells.resolution ? dCellLeaves : nullptr;
    sceneFlat.shadowRes = cells.resolution;
    if (before != sceneFlat.shadowRes) InvalidateGraph();
    return DCRT_OK;
}

// The frame's lights index the lights buffer (BeginImage: fc.lightCount): refuse more than it holds
int dcrt_tracer::CheckFrameLights() const
{
    if (hasScene && frame.light_count > hostLights.size()) {
        SetLastError("frame light_count " + std::to_string(frame.light_count) + " exceeds the " + std::to_string(hostLights.size()) +
                     " lights uploaded");
        return DCRT_E_INVALID_ARG;
    }
    // (the light table's CDF covers the lights uploaded, all of them)
    if (LightTableActive() && frame.light_count != hostLights.size()) {
        SetLastError("frame light_count " + std::to_string(frame.light_count) + " differs from the " + std::to_string(hostLights.size()) +
                     " lights the light table was built for");
        return DCRT_E_INVALID_ARG;
    }
    return DCRT_OK;
}

int dcrt_tracer::UploadScene(const dcrt_flat_scene& s)
{
    Annotation an("UploadScene");
    const UploadKnobs k = ReadUploadKnobs();   // (per upload: tests set the variables between uploads)
    std::vector<uint32_t> identity;
    CHECKED(UploadArrays(s, &identity));
    CHECKED(PlanCast(s, k, identity));
    CHECKED(SizeGrids(k));
    MaterialPlan shading;
    CHECKED(PlanMaterial(nullptr, &shading));
    CHECKED(ApplyMaterialPlan(shading));
    CHECKED(RebuildShadowCells());
    HIPCHECK(hipStreamSynchronize(stream));
    hasScene = true;
    newImage = true;
    return DCRT_OK;
}

// UploadScene's first job: the flat scene checked, the last one's buffers freed, every array but
// the BVH nodes on the device and plan.scene pointing at them. `identity`: IdentityInstances(s).
int dcrt_tracer::UploadArrays(const dcrt_flat_scene& s, std::vector<uint32_t>* identity)
{
    if (!s.vertices || !s.triangles || !s.bvh_nodes || !s.material_ids || !s.instance_transforms ||
        !s.instance_light_indices || !s.instance_material_overrides || s.triangle_count == 0 ||
        s.bvh_node_count == 0 || s.instance_count == 0 || ValidateMaterials(s.materials, s.material_count) != DCRT_OK ||
        ValidateInstanceFlags(s.instance_flags, s.instance_count) != DCRT_OK) {
        SetLastError("incomplete flat scene");
        return DCRT_E_INVALID_ARG;
    }
    CHECKED(ValidateLights(s.lights, s.light_count));
    HIPCHECK(hipStreamSynchronize(stream));
    InvalidateGraph();
    sceneAllocs.Free();
    hasScene = false;
    dEnvProb = dEnvRowCdf = dEnvMarginal = nullptr;   // (the last scene's table went with sceneAllocs)
    lightAllocs.Free();
    lightTable = LightTable{};
    ++uploadStats.scene_uploads;
    DeviceScene d{};
    // (shading_bytes: the three arrays an edit replaces)
    uint64_t* const geometry = &uploadStats.geometry_bytes;
    uint64_t* const shading = &uploadStats.shading_bytes;
    dcrt_vertex* vtx = nullptr;
    uint32_t* tris = nullptr;
    dcrt_float4x3* xf = nullptr;
    CHECKED(Upload(&vtx, s.vertices, s.vertex_count, geometry));
    CHECKED(Upload(&tris, s.triangles, (size_t)s.triangle_count * 3, geometry));
    // the traversal pushes without a bound check: refuse a stack size below what the
    // uploaded tree needs (TLAS leaf depth + BLAS depth, Scene.cpp:199-207); the walk also
    // checks every node reference
    uint32_t stackNeed = 0;
    if (!dcrt::RequiredTraversalStack(s, &stackNeed)) { SetLastError("malformed BVH node references"); return DCRT_E_INVALID_ARG; }
    if (s.bvh_traversal_stack_size < stackNeed) {
        SetLastError("bvh_traversal_stack_size " + std::to_string(s.bvh_traversal_stack_size) +
                     " is below the uploaded BVH's depth " + std::to_string(stackNeed));
        return DCRT_E_INVALID_ARG;
    }
    uint32_t* mids = nullptr; uint32_t* lidx = nullptr; uint32_t* iflags = nullptr; uint32_t* ovr = nullptr;
    dcrt_material* mats = nullptr; dcrt_light* lights = nullptr;
    CHECKED(Upload(&mids, s.material_ids, s.triangle_count, geometry));
    CHECKED(Upload(&xf, s.instance_transforms, (size_t)s.instance_count * 2, geometry));
    CHECKED(Upload(&lidx, s.instance_light_indices, s.instance_count, geometry));
    CHECKED(Upload(&iflags, s.instance_flags, s.instance_count, shading));
    CHECKED(Upload(&ovr, s.instance_material_overrides, s.instance_count, geometry));
    *identity = dcrt::IdentityInstances(s);
    uint32_t* ident = nullptr;
    CHECKED(Upload(&ident, (const uint32_t*)identity->data(), s.instance_count, geometry));
    CHECKED(Upload(&mats, s.materials, s.material_count, shading));
    // (room for DCRT_MAX_LIGHT_COUNT lights, 5000 x 28 B as the reference allocates: UpdateLights
    // changes the count in place)
    CHECKED(Upload(&lights, s.lights, s.light_count, shading, DCRT_MAX_LIGHT_COUNT));
    dMaterials = mats;
    dLights = lights;
    // (the materials' rows of the dielectric LUT: BuildDielRows fills them)
    dDielRows = nullptr;
    if (s.material_count <= kDielRowsMaxMaterials) CHECKED(sceneAllocs.Alloc(&dDielRows, (size_t)s.material_count * kDielRowFloats));
    dInstanceFlags = iflags;
    hostMaterials.assign(s.materials, s.materials + s.material_count);
    if (s.light_count) hostLights.assign(s.lights, s.lights + s.light_count);
    else hostLights.clear();
    float4* triVerts = nullptr;
    float4* triShade = nullptr;
    CHECKED(sceneAllocs.Alloc(&triVerts, (size_t)s.triangle_count * 3));
    CHECKED(sceneAllocs.Alloc(&triShade, (size_t)s.triangle_count * 6));
    if (s.triangle_count)
        hipLaunchKernelGGL(build_tri_verts_kernel, dim3((s.triangle_count + 255) / 256), dim3(256), 0, stream, vtx, tris, mids,
                           s.triangle_count, triVerts, triShade);
    HIPCHECK(hipGetLastError());
    // the triangles' world-space frames, where a triangle index names one (instance, triangle) pair
    dTriFrames = nullptr;
    std::vector<uint32_t> triInstance;
    if (s.triangle_count && dcrt::TriangleInstances(s, &triInstance)) {
        uint32_t* dTriInstance = nullptr;
        CHECKED(Upload(&dTriInstance, (const uint32_t*)triInstance.data(), s.triangle_count, geometry));
        CHECKED(sceneAllocs.Alloc(&dTriFrames, (size_t)s.triangle_count * 3));
        hipLaunchKernelGGL(build_tri_frames_kernel, dim3((s.triangle_count + 255) / 256), dim3(256), 0, stream, (const float4*)triVerts,
                           (const float4*)triShade, (const float4*)xf, (const uint32_t*)dTriInstance, s.triangle_count, dTriFrames);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipStreamSynchronize(stream));   // (triInstance ends with this function)
    }
    // textures: one texel blob + descriptors (Scene.cpp:586-608)
    std::vector<TextureDesc> descs(std::max<uint32_t>(s.texture_count, 1));
    std::vector<uint8_t> blob;
    for (uint32_t i = 0; i < s.texture_count; ++i) {
        const dcrt_texture& t = s.textures[i];
        TextureDesc& td = descs[i];
        const size_t bpp = t.format == DCRT_TEXTURE_FORMAT_R8_UNORM ? 1 : 4;
        td.width = t.pixels ? t.width : 0; td.height = t.pixels ? t.height : 0; td.format = t.format;
        td.offset = (uint32_t)blob.size();
        if (t.pixels) blob.insert(blob.end(), t.pixels, t.pixels + (size_t)t.width * t.height * bpp);
        while (blob.size() % 4) blob.push_back(0);
    }
    if (blob.empty()) blob.resize(4, 0);
    TextureDesc* dDescs = nullptr; uint8_t* dBlob = nullptr; float* dSrgb = nullptr;
    CHECKED(Upload(&dDescs, (const TextureDesc*)descs.data(), descs.size(), geometry));
    CHECKED(Upload(&dBlob, (const uint8_t*)blob.data(), blob.size(), geometry));
    float srgb[256];
    for (int i = 0; i < 256; ++i) {
        const double c = i / 255.0;
        srgb[i] = (float)(c <= 0.04045 ? c / 12.92 : std::pow((c + 0.055) / 1.055, 2.4));
    }
    CHECKED(Upload(&dSrgb, (const float*)srgb, 256, geometry));
    float* dEnv = nullptr;
    if (s.env_cube_rgb && s.env_cube_size) CHECKED(Upload(&dEnv, s.env_cube_rgb, (size_t)6 * s.env_cube_size * s.env_cube_size * 3, geometry));
    d.triVerts = triVerts;
    d.triShade = triShade;
    d.vertices = vtx;
    d.triangles = tris;
    d.materialIds = mids;
    d.transforms = (const float4*)xf;
    d.instanceLightIndices = lidx;
    d.instanceFlags = iflags;
    d.instanceIdentity = ident;
    d.overrides = ovr;
    d.materials = mats;
    d.lights = lights;
    d.textures = dDescs;
    d.texels = dBlob;
    d.srgbTable = dSrgb;
    d.envCube = dEnv;
    d.envCubeSize = dEnv ? s.env_cube_size : 0;
    d.lutBrdf = dLuts->brdf;
    d.lutBrdfAvg = dLuts->brdf_avg;
    d.lutBrdfDielectric = dLuts->brdf_dielectric;
    d.lutBrdfDielectricAvg = dLuts->brdf_dielectric_avg;
    d.lutBsdf = dLuts->bsdf;
    d.lutBsdfAvg = dLuts->bsdf_avg;
    d.instanceCount = s.instance_count;
    d.triangleCount = s.triangle_count;
    d.stackSize = std::max<uint32_t>(s.bvh_traversal_stack_size, 1u);
    d.singlePrimLeaves = dcrt::SingleTriangleLeaves(s) ? 1u : 0u;
    plan.scene = d;
    if (envSampling == DCRT_ENV_SAMPLING_IMPORTANCE) CHECKED(BuildEnvTable());
    // what the light table's weights take from the scene (dcrt.h, "light selection"): R of the BVH root's box here; Ybar of
    // the cube only once a table asks for it (CubeMeanLuminance: with the mode off an upload does none of that work)
    {
        const dcrt_bvh_node& root = s.bvh_nodes[0];
        double q = 0.0;
        for (int a = 0; a < 3; ++a) q += ((double)root.bbox_max[a] - (double)root.bbox_min[a]) * ((double)root.bbox_max[a] - (double)root.bbox_min[a]);
        sceneRadius = 0.5 * std::sqrt(q);
        envMeanY = 1.0;
        envMeanYKnown = dEnv == nullptr;
    }
    if (lightSampling == DCRT_LIGHT_SAMPLING_POWER) CHECKED(BuildLightTable());
    return DCRT_OK;
}

// The sampling table of plan.scene's cube (none: nothing to do), on the tracer's stream: env_rows_kernel,
// env_marginal_kernel, env_finish_kernel between two events, then the total read back -- zero or not finite:
// no table, the light stays uniformly sampled. The table depends on the cube alone, so it stands until the
// next upload whatever the lights' colours become.
int dcrt_tracer::BuildEnvTable()
{
    dEnvProb = dEnvRowCdf = dEnvMarginal = nullptr;
    envBuildMs = 0.0f;
    const uint32_t n = plan.scene.envCubeSize;
    if (!plan.scene.envCube || n == 0u) return DCRT_OK;
    const uint32_t rows = 6u * n;
    const size_t texels = (size_t)rows * n;
    DeviceGroup scratch;
    double *rowSums = nullptr, *rowTotals = nullptr, *marginalSums = nullptr;
    float *prob = nullptr, *rowCdf = nullptr, *marginal = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    double total = 0.0;
    auto build = [&]() -> int {
        CHECKED(scratch.Alloc(&rowSums, texels));
        CHECKED(scratch.Alloc(&rowTotals, (size_t)rows));
        CHECKED(scratch.Alloc(&marginalSums, (size_t)rows + 1));
        CHECKED(sceneAllocs.Alloc(&prob, texels));
        CHECKED(sceneAllocs.Alloc(&rowCdf, texels));
        CHECKED(sceneAllocs.Alloc(&marginal, (size_t)rows));
        HIPCHECK(hipEventCreate(&e0));
        HIPCHECK(hipEventCreate(&e1));
        HIPCHECK(hipEventRecord(e0, stream));
        hipLaunchKernelGGL(env_rows_kernel, dim3((rows + 3u) / 4u), dim3(256), 0, stream, plan.scene.envCube, n, rowSums, rowTotals);
        hipLaunchKernelGGL(env_marginal_kernel, dim3(1), dim3(256), 0, stream, (const double*)rowTotals, rows, marginalSums);
        hipLaunchKernelGGL(env_finish_kernel, dim3((uint32_t)((texels + 255) / 256)), dim3(256), 0, stream, plan.scene.envCube, n, (const double*)rowSums,
                           (const double*)rowTotals, (const double*)marginalSums, prob, rowCdf, marginal);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(e1, stream));
        HIPCHECK(hipMemcpyAsync(&total, marginalSums + rows, sizeof(double), hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
        HIPCHECK(hipEventElapsedTime(&envBuildMs, e0, e1));
        return DCRT_OK;
    };
    const int rc = build();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (rc != DCRT_OK) return rc;
    if (total > 0.0 && std::isfinite(total)) {
        dEnvProb = prob;
        dEnvRowCdf = rowCdf;
        dEnvMarginal = marginal;
    }
    return DCRT_OK;
}

// DCRT_ENV_SAMPLING_*: set on an uploaded scene, like the scene edits, and kept for it and every later scene. The
// table is built when the mode first asks for it, and the plan rederived: the variant and the table's pointers are
// among what a captured graph bakes in, so a toggle that changes them drops the graphs once. Film and path state
// stay as they are.
int dcrt_tracer::SetEnvSampling(int mode)
{
    if (mode != DCRT_ENV_SAMPLING_UNIFORM && mode != DCRT_ENV_SAMPLING_IMPORTANCE) { SetLastError("unknown environment sampling mode"); return DCRT_E_INVALID_ARG; }
    if (!hasScene) { SetLastError("no scene uploaded"); return DCRT_E_NO_SCENE; }
    if (mode == envSampling) return DCRT_OK;
    envSampling = mode;
    HIPCHECK(hipStreamSynchronize(stream));
    if (mode == DCRT_ENV_SAMPLING_IMPORTANCE && !dEnvProb) CHECKED(BuildEnvTable());
    CHECKED(RederiveShading());
    HIPCHECK(hipStreamSynchronize(stream));
    return DCRT_OK;
}

// Resident workgroups per CU of a cast kernel with `lds` bytes of dynamic LDS: registers and
// LDS (gfx950's 1280-B allocation granule, LdsResident). Split casts run extension_kernel's.
int dcrt_tracer::CastOccupancy(CastFn k, size_t lds, int* out)
{
    return ResidentPerCU(knobs.mergedCasts ? (const void*)k : (const void*)extension_kernel<false, false>, plan.block, lds, out);
}

// UploadScene's second job: the cast's workgroup size, its LDS scene cache, which traversal the
// scene gets (pair / ident / ring / flat / cells), and the node order that goes with it, uploaded.
int dcrt_tracer::PlanCast(const dcrt_flat_scene& s, const UploadKnobs& k, const std::vector<uint32_t>& identity)
{
    DeviceScene d = plan.scene;
    // LDS stack: [stackSize + 2][block] u32 (two spare rows per lane, see stack_at in
    // dscene.h); keep a workgroup's stack <= 32 KiB
    plan.block = 256;
    while (plan.block > 64 && (size_t)(d.stackSize + 2) * plan.block * 4 > 32768) plan.block >>= 1;
    if ((k.castBlock == 64 || k.castBlock == 128 || k.castBlock == 256) && k.castBlock <= plan.block) plan.block = k.castBlock;
    d.stackRows = d.stackSize + 2u;
    d.ringRows = 0u;
    d.spill = nullptr;
    plan.ringRows = 0;
    const size_t wholeStack = (size_t)(d.stackSize + 2) * plan.block * 4;
    if (wholeStack > 65536) { SetLastError("BVH traversal stack too deep for LDS"); return DCRT_E_LIMIT; }
    // LDS scene cache in what the cast kernel's register-limited occupancy leaves of the
    // CU's 160 KiB per workgroup: BVH nodes first, then pre-gathered triangles
    int regPerCU = 0;
    CHECKED(CastOccupancy(CastKernel(CastVariant{}), wholeStack, &regPerCU));
    const size_t perBlock = (g_ldsPerCU / (size_t)std::max(1, regPerCU)) & ~(size_t)15;
    size_t budget = wholeStack < perBlock ? perBlock - wholeStack : 0;
    uint32_t nodeCount = s.bvh_node_count;
    d.cachedNodes = (uint32_t)std::min<size_t>(nodeCount, budget / 32);
    d.cachedTris = (uint32_t)std::min<size_t>(s.triangle_count, (budget - d.cachedNodes * 32) / 48);
    if (k.noLdsCache) d.cachedNodes = d.cachedTris = 0;
    // (the LDS-only variant assumes 256-thread workgroups: its stack stride is a constant)
    // (the cache-only variant keeps three permuted copies of every triangle: 144 B each)
    plan.allCached = plan.block == 256 && d.cachedNodes == nodeCount && d.cachedTris == s.triangle_count &&
                     (size_t)d.cachedNodes * 32 + (size_t)s.triangle_count * 144 + (size_t)s.instance_count * 64 <= budget;
    d.cachedInstances = plan.allCached ? s.instance_count : 0u;
    // trav_visit_pair where the traversal's fetches miss L2: nodes + triangles beyond an
    // XCD's 4 MiB L2
    plan.pair = !plan.allCached && (size_t)nodeCount * 32 + (size_t)s.triangle_count * 48 > ((size_t)4 << 20);
    if (k.pairTraversal >= 0) plan.pair = !plan.allCached && k.pairTraversal != 0;
    // the node order goes with it (dscene.h kLayoutPairs: the pair kernels assume it, the
    // other non-counting cast kernels assume PackBVH's)
    std::vector<dcrt_bvh_node> pairNodes;
    if (plan.pair) {
        if (!dcrt::PairLayout(s, k.topNodes, &pairNodes, k.nodeQuads)) { SetLastError("malformed BVH: a node with two parents"); return DCRT_E_INVALID_ARG; }
        nodeCount = (uint32_t)pairNodes.size();
    }
    std::vector<dcrt_bvh_node> devNodes = plan.pair ? std::move(pairNodes) : std::vector<dcrt_bvh_node>(s.bvh_nodes, s.bvh_nodes + nodeCount);
    // every instance the identity: the cache-only kernel keeps no instance space (IDENT)
    plan.ident = (plan.allCached || !plan.pair) && knobs.mergedCasts && s.instance_count > 0;
    plan.ident = plan.ident && dcrt::AllInstancesBitwiseIdentity(s) && k.identCast;
    // a non-counting, opaque kernel this scene could run
    auto candidate = [&](bool ring, bool flat = false, bool cells = false) {
        return CastKernel({ false, false, plan.allCached, plan.pair, plan.ident, ring, flat, cells });
    };
    // The spilling stack (cast_kernel's RING: an LDS window of K rows over a per-lane global
    // column, kernels_impl.h ring_maintain) where the whole stack costs the launched kernel
    // resident workgroups: a deep BVH (spaceship: 30 entries = 32 KiB per 256-lane workgroup,
    // 4 workgroups per CU where its registers allow 6). A forced K below the scene's depth spills (tests).
    if (!plan.allCached && knobs.mergedCasts) {
        const int forced = k.stackRing;
        const uint32_t K = forced > 0 ? (uint32_t)forced : 16u;
        // (the window must take a batch of kVisitsPerCheck visits after a refill to half: kMinRingRows)
        const bool validK = K >= std::max(8u, kMinRingRows) && K <= 64u && (K & (K - 1u)) == 0u;
        if (forced > 0 && !validK) {
            SetLastError("DCRT_STACK_RING: a power of two in [max(8, 2 * (visits per check + 1)), 64]");
            return DCRT_E_INVALID_ARG;
        }
        if (forced > 0) {
            plan.ringRows = K;
        } else if (forced < 0 && validK && K < d.stackSize + 2u) {
            int whole = 0, ring = 0;
            CHECKED(CastOccupancy(candidate(false), wholeStack, &whole));
            CHECKED(CastOccupancy(candidate(true), (size_t)K * plan.block * 4, &ring));
            if (ring > whole) plan.ringRows = K;
        }
    }
    // A scene the cache does not hold whole: the cache leaves `reserve` bytes of each CU's LDS
    // free, so workgroups of the other pipeline's kernels (MATERIAL, CONTROL) can be resident
    // beside the cast's -- with the cache sized to the last byte they could not
    const size_t reserve = std::min<size_t>(k.castLdsReserve, g_ldsPerCU);
    const CastFn launched = candidate(plan.ringRows != 0);
    // the launched kernel's stack bytes: the ring window, or the whole stack
    const size_t stackLds = plan.ringRows ? (size_t)plan.ringRows * plan.block * 4 : wholeStack;
    if (!plan.allCached) {
        // the cache budget from the occupancy of the kernel that launches
        int perCU = 0;
        CHECKED(CastOccupancy(launched, stackLds, &perCU));
        const size_t perBlockR = ((g_ldsPerCU - reserve) / (size_t)std::max(1, perCU)) & ~(size_t)15;
        budget = stackLds < perBlockR ? perBlockR - stackLds : 0;
        d.cachedNodes = (uint32_t)std::min<size_t>(nodeCount, budget / 32);
        d.cachedTris = (uint32_t)std::min<size_t>(s.triangle_count, (budget - d.cachedNodes * 32) / 48);
        if (k.noLdsCache) d.cachedNodes = d.cachedTris = 0;
    }
    // the cache-only kernels enter identity instances' BLASes in phase A (dscene.h
    // kMiscIdentityLeaf): TLAS leaves carry the flag in their otherwise unused axis bits
    if (plan.allCached || plan.ident) {
        for (dcrt_bvh_node& n : devNodes) {
            if (!(n.misc & 0x4u)) continue;
            const uint32_t inst = (n.misc >> 3) & DCRT_BVHNODE_MISC_MASK_PRIMITIVE_COUNT;
            n.misc = (n.misc & ~0x3u) | (inst < s.instance_count && identity[inst] ? kMiscIdentityLeaf : 0u);
        }
    }
    dcrt_bvh_node* nodes = nullptr;
    CHECKED(Upload(&nodes, (const dcrt_bvh_node*)devNodes.data(), nodeCount, &uploadStats.geometry_bytes));
    HIPCHECK(hipStreamSynchronize(stream));   // (devNodes ends with this function)
    d.nodes = (const float4*)nodes;
    d.nodeCount = nodeCount;
    d.pairLayout = plan.pair ? 1u : 0u;
    d.skipRoot = k.skipRoot;
    const size_t cacheBytes = (size_t)d.cachedNodes * 32 + (size_t)d.cachedTris * (plan.allCached ? 144 : 48) + (size_t)d.cachedInstances * 64;
    size_t launchLds = stackLds + cacheBytes;
    // The budget above divides 160 KiB evenly among the workgroups the registers allow; the
    // LDS is allocated in granules (and the kernel's static LDS comes on top), so the cache
    // could cost a workgroup per CU (the spaceship pair kernel ran 5 of its 6). Trim the
    // cache -- triangles first, then nodes, a granule at a time -- until the launched kernel
    // keeps the occupancy the stack alone allows.
    if (!plan.allCached && k.ldsTrim) {
        int target = 0, now = 0;
        CHECKED(CastOccupancy(launched, stackLds, &target));
        for (;;) {
            CHECKED(CastOccupancy(launched, launchLds, &now));
            if (now >= target || (d.cachedTris == 0 && d.cachedNodes == 0)) break;
            if (d.cachedTris > 0) d.cachedTris -= std::min<uint32_t>(d.cachedTris, 11);   // 528 B
            else d.cachedNodes -= std::min<uint32_t>(d.cachedNodes, 16);                  // 512 B
            launchLds = stackLds + (size_t)d.cachedNodes * 32 + (size_t)d.cachedTris * 48;
        }
    }
    plan.scene = d;
    // every kernel but the ring cast launches with the whole stack in front of the same cache
    plan.ldsWholeStack = wholeStack + (launchLds - stackLds);
    plan.ldsRing = plan.ringRows ? launchLds : 0;
    return PlanFlatCast(s, k);
}

// ... and its last part: the entry-free node order for the cache-only IDENT kernel (EntryFreeLayout:
// no BLAS-entry step per node visit), where its nodes, the triangles and one more stack row still
// fit the LDS the IDENT kernel runs at; with it the buffers of the point light's direction cells.
int dcrt_tracer::PlanFlatCast(const dcrt_flat_scene& s, const UploadKnobs& k)
{
    const DeviceScene& d = plan.scene;
    plan.flat = false;
    plan.cellsRes = 0;
    dCells = nullptr;        // (sceneAllocs: freed by UploadArrays)
    dCellLeaves = nullptr;
    cells = ShadowCells{};
    if (!(k.flatCast && plan.allCached && plan.ident && knobs.mergedCasts && d.singlePrimLeaves)) return DCRT_OK;
    std::vector<dcrt_bvh_node> flat;
    if (!dcrt::EntryFreeLayout(s, &flat, k.flatMerge)) return DCRT_OK;
    auto kernel = [&](bool flatOrder, bool cellTable) { return CastKernel({ false, false, true, false, true, false, flatOrder, cellTable }); };
    const size_t flatLds = (size_t)(d.stackSize + 3u) * plan.block * 4 + flat.size() * 32 + (size_t)s.triangle_count * 144;
    int identPerCU = 0, flatPerCU = 0;
    CHECKED(CastOccupancy(kernel(false, false), plan.ldsWholeStack, &identPerCU));
    CHECKED(CastOccupancy(kernel(true, false), flatLds, &flatPerCU));
    if (!(flatPerCU >= identPerCU && flatLds <= 65536)) return DCRT_OK;
    dcrt_bvh_node* fn = nullptr;
    CHECKED(Upload(&fn, (const dcrt_bvh_node*)flat.data(), flat.size(), &uploadStats.geometry_bytes));
    HIPCHECK(hipStreamSynchronize(stream));   // (flat ends with this function)
    plan.sceneFlat = plan.scene;
    plan.sceneFlat.nodes = (const float4*)fn;
    plan.sceneFlat.nodeCount = (uint32_t)flat.size();
    plan.sceneFlat.cachedNodes = (uint32_t)flat.size();
    plan.sceneFlat.cachedInstances = 0u;
    plan.sceneFlat.stackSize = d.stackSize + 1u;
    plan.sceneFlat.stackRows = d.stackSize + 3u;
    plan.ldsFlat = flatLds;
    plan.flat = true;
    // The point light's direction cells for this kernel's shadow rays (RebuildShadowCells
    // decides per light set): the leaf words go behind the scene cache, where they and the
    // CELLS kernel's registers leave the occupancy alone.
    const uint32_t wanted = k.shadowCells;
    const size_t cellsLds = flatLds + dcrt::kCellWords * sizeof(uint32_t);
    int plainPerCU = 0, cellsPerCU = 0;
    if (wanted) {
        CHECKED(CastOccupancy(kernel(true, false), cellsLds, &plainPerCU));
        CHECKED(CastOccupancy(kernel(true, true), cellsLds, &cellsPerCU));
    }
    if (wanted && std::min(plainPerCU, cellsPerCU) >= flatPerCU && cellsLds <= 65536) {
        plan.cellsRes = wanted;
        plan.ldsFlat = cellsLds;
        CHECKED(sceneAllocs.Alloc(&dCells, (size_t)6 * plan.cellsRes * plan.cellsRes));
        CHECKED(sceneAllocs.Alloc(&dCellLeaves, dcrt::kCellWords));
        cellNodes = flat;
        cellVertices.assign(s.vertices, s.vertices + s.vertex_count);
        cellTriangles.assign(s.triangles, s.triangles + (size_t)s.triangle_count * 3);
        cellTransforms.assign(s.instance_transforms, s.instance_transforms + (size_t)s.instance_count * 2);
    }
    return DCRT_OK;
}

// UploadScene's third job: the persistent grids -- the traversal kernels run exactly one resident
// wave of workgroups -- and the ring cast's spill columns, which take the shipped grid's size.
int dcrt_tracer::SizeGrids(const UploadKnobs& k)
{
    hipDeviceProp_t prop;
    HIPCHECK(hipGetDeviceProperties(&prop, device));
    cuCount = (uint32_t)std::max(1, prop.multiProcessorCount);
    // (no cell table stands yet -- RebuildShadowCells follows -- so a flat plan is sized by the plain
    // FLAT kernel: PlanFlatCast saw to it that the CELLS kernel keeps that occupancy)
    const CastLaunch shipped = plan.Launch(false, false);
    int perCU = 0;
    CHECKED(CastOccupancy(shipped.kernel, shipped.lds, &perCU));
    // the two tuning knobs act on the shipped kernel's grid only
    if (k.castBlocksPerCU >= 1 && k.castBlocksPerCU < perCU) perCU = k.castBlocksPerCU;
    plan.perCU = (uint32_t)std::max(1, perCU);
    plan.resident[0][0] = plan.perCU * cuCount;
    if (k.castGridMul >= 2 && k.castGridMul <= 16) plan.resident[0][0] *= (uint32_t)k.castGridMul;
    // the any-hit and the counting kernels keep the whole stack: their own resident grids, so an
    // instrumented run has no second partial round of workgroups the shipped kernel lacks
    for (const bool instr : { false, true }) {
        for (const bool opacity : { false, true }) {
            if (!instr && !opacity) continue;
            const CastLaunch other = plan.Launch(instr, opacity);
            int own = 0;
            CHECKED(CastOccupancy(other.kernel, other.lds, &own));
            plan.resident[instr][opacity] = (uint32_t)std::max(1, std::min(own, perCU)) * cuCount;
        }
    }
    const uint32_t block = plan.block;
    const size_t lds = plan.ldsWholeStack;
    int megaPerCU = 0;
    CHECKED(ResidentPerCU((const void*)megakernel<false>, block, lds, &megaPerCU));
    megaResident = (uint32_t)std::max(1, megaPerCU) * cuCount;
    // the first-hit view kernel: the megakernel's launch shape, its own register budget
    int viewPerCU = 0, viewOpacityPerCU = 0;
    CHECKED(ResidentPerCU((const void*)view_kernel<false>, block, lds, &viewPerCU));
    CHECKED(ResidentPerCU((const void*)view_kernel<true>, block, lds, &viewOpacityPerCU));
    viewResident = (uint32_t)std::max(1, viewPerCU) * cuCount;
    viewResidentOpacity = (uint32_t)std::max(1, viewOpacityPerCU) * cuCount;
    if (plan.ringRows) {
        // the spill columns: stackSize entries per lane of the persistent ring grid
        const size_t words = (size_t)plan.resident[0][0] * block * plan.scene.stackSize;
        uint32_t* spill = nullptr;
        CHECKED(sceneAllocs.Alloc(&spill, words));
        HIPCHECK(hipMemsetAsync(spill, 0, words * 4, stream));
        plan.sceneRing = plan.scene;
        plan.sceneRing.stackRows = plan.ringRows;
        plan.sceneRing.ringRows = plan.ringRows;
        plan.sceneRing.spill = spill;
    }
    return DCRT_OK;
}

int dcrt_tracer::EnsureFilm(uint32_t w, uint32_t h)
{
    if (w == filmW && h == filmH && film.accum) return DCRT_OK;
    if (w == 0 || h == 0 || w > 65535 || h > 65535) { SetLastError("invalid film resolution"); return DCRT_E_INVALID_ARG; }
    HIPCHECK(hipStreamSynchronize(stream));
    InvalidateGraph();
    filmAllocs.Free();
    sampleAllocs.Free();
    sampleImages = 0;
    guideNormal = guideAlbedo = denoised = nullptr;   // (they follow the film: EnsureGuides)
    guidesRendered = hasDenoised = false;
    halfAllocs.Free();                                // (the half film and the noise maps too)
    noiseMapAllocs.Free();
    halfFilm = nullptr;
    noisePixelMap = noiseTileMap = nullptr;
    hasNoiseMaps = false;
    cascadeAllocs.Free();                             // (and the cascades)
    cascades = CascadeFilms{};
    reweighted = nullptr;
    hasReweighted = false;
    filmImages = 0;
    const size_t n = (size_t)w * h;
    CHECKED(filmAllocs.Alloc(&film.accum, n));
    HIPCHECK(hipMemsetAsync(film.accum, 0, n * sizeof(float4), stream));
    if (convergence) {
        CHECKED(halfAllocs.Alloc(&halfFilm, n));
        HIPCHECK(hipMemsetAsync(halfFilm, 0, n * sizeof(float4), stream));
    }
    filmW = w; filmH = h;
    film.width = w; film.height = h;
    if (firefly) CHECKED(AllocCascadesOrOff());
    CHECKED(EnsureSamples(1));
    CHECKED(BuildRows());
    return adaptive ? AllocBlockList() : DCRT_OK;   // (a new resolution: its own blocks, all of them active)
}

// Sample textures for `images` images (a RenderImages batch); grows only.
int dcrt_tracer::EnsureSamples(uint32_t images)
{
    if (images <= sampleImages) return DCRT_OK;
    HIPCHECK(hipStreamSynchronize(stream));
    InvalidateGraph();
    sampleAllocs.Free();
    const size_t n = (size_t)filmW * filmH * images;
    CHECKED(sampleAllocs.Alloc(&film.samplePosition, n));
    CHECKED(sampleAllocs.Alloc(&film.sampleValue, n));
    film.debugRng = nullptr;
    if (debugRng) CHECKED(sampleAllocs.Alloc(&film.debugRng, n));
    HIPCHECK(hipMemsetAsync(film.samplePosition, 0, n * sizeof(float2), stream));
    HIPCHECK(hipMemsetAsync(film.sampleValue, 0, n * sizeof(float4), stream));
    if (film.debugRng) HIPCHECK(hipMemsetAsync(film.debugRng, 0, n * sizeof(uint4), stream));
    hSampleOut = SampleOut{film.samplePosition, film.sampleValue, film.debugRng, rowProbe ? dRowRays : nullptr};
    HIPCHECK(hipMemcpyAsync(dSampleOut, &hSampleOut, sizeof(SampleOut), hipMemcpyHostToDevice, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    sampleImages = images;
    inactiveFilled = false;   // (adaptive sampling: the new slots hold no sentinel samples)
    return DCRT_OK;
}

// Images per RenderImages batch: as many as the path pool holds at once, so that a rank
// of a partitioned film (a fraction of every image) still runs full wavefronts. A batch
// that overflows the pool by a little is avoided: its last pixel blocks would start only
// when the first paths end and stretch the batch by a whole path length. Every batch ends
// in a drain (iterations with a shrinking path population), so large pools and batches of
// many images amortise it: a rank of an N-GPU film renders 1/N of each image, and gets N
// times as many images per batch.
uint32_t dcrt_tracer::AutoBatch(uint32_t count) const
{
    uint32_t b = batchImages;
    // (sample index p = image * W*H + y * W + x stays below 2^31)
    const uint32_t cap = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(kMaxImageBatchAuto(), ((uint64_t)1 << 31) / ((uint64_t)filmW * filmH)));
    if (b == 0) {
        // the slots an image takes: whole 8x8 pixel blocks (a wave each), partial bands and
        // columns included, so a batch that "fits" never waits for slots to free up
        // (adaptive sampling: the listed blocks alone)
        const uint64_t blocks = adaptive ? listCount : (uint64_t)bandCount * ((filmW + kBlockW - 1) / kBlockW);
        const uint64_t pixels = std::max<uint64_t>(1, blocks * kBlockH * kBlockW);
        b = (uint32_t)std::min<uint64_t>(cap, std::max<uint64_t>(1, poolSize / pixels));
        if (!BatchPoolLimit()) b = cap;
        // equal batches: as many batches as the cap needs, each as large as the others (a
        // small last batch would pay a whole drain for a sparse wavefront)
        const uint32_t batches = (count + b - 1) / b;
        b = (count + batches - 1) / batches;
    }
    return std::max<uint32_t>(1, std::min(std::min(b, cap), count));
}

// Rows this tracer renders. One tracer: every row. Partitioned film: the
// film is cut into K = N * k stripes of floor/ceil(H / K) rows, k = round(H / (N * S))
// for the target stripe height S, stripe j belongs to rank j mod N (every rank gets k
// stripes, equal row counts to one row); a rank renders its rows plus `halo` rows on
// either side of each stripe and convolves only its own rows. The rows are packed 8 per
// block row in ascending order (directcomputeraytracing_amd/partition.py mirrors this).
int dcrt_tracer::BuildRows()
{
    const uint32_t H = filmH;
    std::vector<uint32_t> rows;
    std::vector<uint32_t> owned;
    if (!bands.empty()) {
        // explicit film bands (dcrt_tracer_set_film_bands): their rows plus the halo beyond each
        const uint32_t halo = partition.halo_rows ? partition.halo_rows : 2u;
        owned.assign(H, 0);
        std::vector<uint8_t> need(H, 0);
        for (size_t i = 0; i + 1 < bands.size(); i += 2) {
            const uint32_t y0 = std::min(bands[i], H), y1 = std::min(bands[i + 1], H);
            for (uint32_t y = y0; y < y1; ++y) owned[y] = 1;
            if (y0 >= y1) continue;
            const uint32_t lo = y0 >= halo ? y0 - halo : 0, hi = std::min(H, y1 + halo);
            for (uint32_t y = lo; y < hi; ++y) need[y] = 1;
        }
        for (uint32_t y = 0; y < H; ++y) if (need[y]) rows.push_back(y);
    } else if (partition.world_size <= 1) {
        for (uint32_t y = 0; y < H; ++y) rows.push_back(y);
    } else {
        const uint32_t N = partition.world_size, halo = partition.halo_rows ? partition.halo_rows : 2u;
        const uint32_t k = std::max<uint32_t>(1, (uint32_t)((H + (N * partition.stripe_height) / 2) / (N * partition.stripe_height)));
        const uint64_t K = std::min<uint64_t>((uint64_t)N * k, H);
        owned.assign(H, 0);
        std::vector<uint8_t> need(H, 0);
        for (uint64_t j = partition.rank; j < K; j += N) {
            const uint32_t y0 = (uint32_t)(j * H / K), y1 = (uint32_t)((j + 1) * H / K);
            for (uint32_t y = y0; y < y1; ++y) owned[y] = 1;
            const uint32_t lo = y0 >= halo ? y0 - halo : 0, hi = std::min(H, y1 + halo);
            for (uint32_t y = lo; y < hi; ++y) need[y] = 1;
        }
        for (uint32_t y = 0; y < H; ++y) if (need[y]) rows.push_back(y);
    }
    if (rows.empty()) rows.push_back(0);
    HIPCHECK(hipStreamSynchronize(stream));
    rowAllocs.Free();
    rowCount = (uint32_t)rows.size();
    bandCount = (rowCount + kBlockH - 1) / kBlockH;
    uint32_t* dRows = nullptr;
    CHECKED(rowAllocs.Alloc(&dRows, rows.size()));
    HIPCHECK(hipMemcpyAsync(dRows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, stream));
    uint32_t* dOwned = nullptr;
    if (!owned.empty()) {
        CHECKED(rowAllocs.Alloc(&dOwned, owned.size()));
        HIPCHECK(hipMemcpyAsync(dOwned, owned.data(), owned.size() * 4, hipMemcpyHostToDevice, stream));
    }
    HIPCHECK(hipStreamSynchronize(stream));
    film.rowY = dRows;
    film.rowOwned = dOwned;
    film.rowCount = rowCount;
    dRowRays = nullptr;
    if (rowProbe) {   // (the probe's counters follow the film's height)
        CHECKED(rowAllocs.Alloc(&dRowRays, filmH));
        HIPCHECK(hipMemsetAsync(dRowRays, 0, (size_t)filmH * 4, stream));
        CHECKED(UploadSampleOut());
    }
    return DCRT_OK;
}

int dcrt_tracer::UploadSampleOut()
{
    hSampleOut.rowRays = rowProbe ? dRowRays : nullptr;
    HIPCHECK(hipMemcpyAsync(dSampleOut, &hSampleOut, sizeof(SampleOut), hipMemcpyHostToDevice, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    return DCRT_OK;
}

// The row-cost probe: while on, MATERIAL's PROBE variant adds each pass's rays (the extension ray
// it shades, the shadow ray it casts) to a counter per film row -- the per-row cost that
// partition.balanced_bands cuts equal-cost film bands from. Turning it on or off re-captures
// the iteration graphs; on clears the counters.
int dcrt_tracer::SetRowProbe(bool on)
{
    HIPCHECK(hipStreamSynchronize(stream));
    InvalidateGraph();
    rowProbe = on;
    if (on && filmH) return BuildRows();   // (allocates and clears the counters)
    return UploadSampleOut();
}

// A partitioned or banded film's convolution reads the filter's window rows beyond its stripes: refuse a
// radius that needs more of them than the halo the tracer renders
int dcrt_tracer::CheckHalo(float radius) const
{
    if (partition.world_size <= 1 && bands.empty()) return DCRT_OK;
    const uint32_t halo = partition.halo_rows ? partition.halo_rows : 2u;
    if (!(radius >= 0.0f) || FilterSupportRows(radius, filmH) > halo) {
        SetLastError("filter radius needs more halo rows than the film partition renders");
        return DCRT_E_INVALID_ARG;
    }
    return DCRT_OK;
}

int dcrt_tracer::SetFrame(const dcrt_frame_params& p)
{
    if (p.resolution[0] == 0 || p.resolution[1] == 0 || p.max_bounce_count > DCRT_MAX_RAY_BOUNCE) {
        SetLastError("invalid frame parameters");
        return DCRT_E_INVALID_ARG;
    }
    CHECKED(EnsureFilm(p.resolution[0], p.resolution[1]));
    if ((frame.features ^ p.features) & DCRT_FEATURE_ALLOW_ANYHIT) {   // captured graphs hold the other kernel variant
        HIPCHECK(hipStreamSynchronize(stream));
        InvalidateGraph();
    }
    frame = p;
    hasFrame = true;
    return DCRT_OK;
}

int dcrt_tracer::SetPartition(const dcrt_film_partition& p)
{
    if (p.world_size == 0 || p.rank >= p.world_size || (p.world_size > 1 && p.stripe_height == 0)) {
        SetLastError("invalid film partition");
        return DCRT_E_INVALID_ARG;
    }
    if (adaptive && p.world_size > 1) { SetLastError("adaptive sampling is on: the film cannot be partitioned"); return DCRT_E_INVALID_ARG; }
    if (firefly && p.world_size > 1) { SetLastError("firefly re-weighting is on: the film cannot be partitioned"); return DCRT_E_INVALID_ARG; }
    partition = p;
    bands.clear();
    if (filmW) {
        HIPCHECK(hipStreamSynchronize(stream));
        InvalidateGraph();
        CHECKED(BuildRows());
    }
    newImage = true;
    return DCRT_OK;
}

// Explicit film bands: this tracer owns rows [b[2i], b[2i+1]) (ascending, disjoint, non-empty),
// path-traces them plus `halo` rows beyond each band and convolves only its own rows. Any cut
// of the film into bands dealt to tracers sums to the one-tracer film bit for bit, as the
// stripes do; cost-balanced cuts come from the row-cost probe (partition.balanced_bands).
int dcrt_tracer::SetBands(const uint32_t* b, uint32_t count, uint32_t halo)
{
    if (count == 0 || !b) { SetLastError("no film bands"); return DCRT_E_INVALID_ARG; }
    if (adaptive) { SetLastError("adaptive sampling is on: the film cannot be cut into bands"); return DCRT_E_INVALID_ARG; }
    if (firefly) { SetLastError("firefly re-weighting is on: the film cannot be cut into bands"); return DCRT_E_INVALID_ARG; }
    for (uint32_t i = 0; i < count; ++i) {
        if (b[2 * i] >= b[2 * i + 1] || (i > 0 && b[2 * i] < b[2 * i - 1])) {
            SetLastError("film bands: ascending, disjoint, non-empty [y0, y1) ranges");
            return DCRT_E_INVALID_ARG;
        }
    }
    bands.assign(b, b + 2 * count);
    partition = dcrt_film_partition{1, 0, 64, halo};
    if (filmW) {
        HIPCHECK(hipStreamSynchronize(stream));
        InvalidateGraph();
        CHECKED(BuildRows());
    }
    newImage = true;
    return DCRT_OK;
}

// The camera and film fields of the frame constants, as generate_ray reads them (BeginImage for the path kernels,
// dcrt_device_camera_ray for the probe: one copy, so both see the same camera)
static void FillCameraConstants(const dcrt_frame_params& frame, FrameConstants* out)
{
    FrameConstants& fc = *out;
    std::memcpy(fc.camera, frame.camera_transform, sizeof(fc.camera));
    fc.resolution[0] = frame.resolution[0]; fc.resolution[1] = frame.resolution[1];
    fc.filmSize[0] = frame.film_size[0]; fc.filmSize[1] = frame.film_size[1];
    fc.apertureRadius = frame.aperture_radius;
    fc.focalDistance = frame.focal_distance;
    fc.filmDistance = frame.film_distance;
    fc.bladeCount = frame.blade_count;
    fc.bladeVertexPos[0] = frame.blade_vertex_pos[0]; fc.bladeVertexPos[1] = frame.blade_vertex_pos[1];
    fc.apertureBaseAngle = frame.aperture_base_angle;
}

// ResetImage + SET_IDLE + constant upload for one image (WavefrontPathTracer.cpp:441-468)
int dcrt_tracer::BeginImage()
{
    Annotation an("Reset", !capturing);
    FrameConstants fc;
    std::memset(&fc, 0, sizeof(fc));
    FillCameraConstants(frame, &fc);
    fc.frameSeed = frame.frame_seed;
    fc.seedStride = seedStride;
    fc.shadowInlineMask = material.fusedMask;
    fc.maxBounce = frame.max_bounce_count;
    fc.rouletteEnable = roulette.enable ? 1u : 0u;
    fc.rouletteStart = roulette.start_bounce;
    fc.rouletteMin = roulette.min_survival;
    fc.rouletteMax = roulette.max_survival;
    fc.lightCount = frame.light_count;
    fc.envLightIndex = frame.environment_light_index;
    fc.features = frame.features;
    fc.blocksX = (frame.resolution[0] + kBlockW - 1) / kBlockW;
    fc.bandCount = bandCount;
    // (adaptive sampling: an image of RenderImages is its listed blocks, film.blockList)
    fc.blocksPerImage = listFrame ? listCount : fc.blocksX * bandCount;
#ifndef DCRT_REFILL_GLOBAL
#define DCRT_REFILL_GLOBAL 28
#endif
    fc.refillLanes = knobs.tuneOverride || plan.allCached ? knobs.refillLanes : DCRT_REFILL_GLOBAL;
    fc.parkLanes = knobs.parkLanes;
    // virtual batch starts (control_kernel): the merged cast kernels carry the camera-ray fetch;
    // not with ALLOW_ANYHIT_SHADER (NEW_PATH's opacity draw)
    fc.virtualStart = knobs.virtualStart && knobs.mergedCasts && !(frame.features & DCRT_FEATURE_ALLOW_ANYHIT) ? 1u : 0u;
    // drain completion (drain_kernel): not with ALLOW_ANYHIT_SHADER, and not while the cast
    // kernels are instrumented (the roofline leg's counts and launch times are the wavefront's)
    fc.drainPaths = !(frame.features & DCRT_FEATURE_ALLOW_ANYHIT) && !instrCounters && !extTiming && !rowProbe ? knobs.drainPaths : 0u;
    hipLaunchKernelGGL(set_frame_kernel, dim3(1), dim3(1), 0, stream, dFrame, fc);
    const uint32_t total = fc.blocksPerImage;
    const uint32_t idleThreads = std::max<uint32_t>(poolSize, 2u * (uint32_t)(sizeof(Counters) / 4));
    hipLaunchKernelGGL(set_idle_kernel, dim3((idleThreads + 255) / 256), dim3(256), 0, stream, pool, dCounters, dGlobals, total);
    HIPCHECK(hipGetLastError());
    parity = 0;
    newImage = false;
    imageComplete = false;
    return DCRT_OK;
}

// RenderOneIteration (WavefrontPathTracer.cpp:622-1162): CONTROL(+NEW_PATH) ->
// MATERIAL -> EXTENSION_RAY_CAST -> SHADOW_RAY_CAST. Queue sizes are read on the
// device, so no indirect-argument pass and no host round trip is needed.
// `sequenced` appends the film pass and the image advance, both no-ops unless
// this iteration completed an image (RenderImages runs images back to back).
int dcrt_tracer::LaunchIteration(uint32_t par, bool timed, bool sequenced)
{
    Annotation an("Iteration", !capturing);
    Counters* cnt = dCounters + par;
    Counters* next = dCounters + (par ^ 1u);   // (the previous iteration's; the casts clear them for the next)
    PathPool pool = this->pool;
    pool.extRec = extRecs + (size_t)par * kShards * pool.recCap * 2;
    pool.extPrevRec = extRecs + (size_t)(par ^ 1u) * kShards * pool.recCap * 2;
    pool.stateA = stateRecsA + (size_t)par * kShards * pool.recCap;
    pool.stateB = stateRecsB + (size_t)par * kShards * pool.recCap;
    pool.stateAPrev = stateRecsA + (size_t)(par ^ 1u) * kShards * pool.recCap;
    pool.stateBPrev = stateRecsB + (size_t)(par ^ 1u) * kShards * pool.recCap;
    pool.shadowHit = shadowHits + (size_t)par * kShards * pool.recCap;
    pool.shadowHitPrev = shadowHits + (size_t)(par ^ 1u) * kShards * pool.recCap;
    pool.finRec = finRecs + (size_t)par * kFinShards * pool.finCap;
    pool.finPrevRec = finRecs + (size_t)(par ^ 1u) * kFinShards * pool.finCap;
    pool.finHit = finHits + (size_t)par * kFinShards * pool.finCap;
    pool.finHitPrev = finHits + (size_t)(par ^ 1u) * kFinShards * pool.finCap;
    const bool opacity = (frame.features & DCRT_FEATURE_ALLOW_ANYHIT) != 0;
    const CastLaunch cast = plan.Launch(instrCounters, opacity);
    const uint32_t castBlock = plan.block, castGrid = std::min<uint32_t>((poolSize + castBlock - 1) / castBlock, cast.resident);
    // Timed launches take their start/stop timestamps from the dispatch itself
    // (hipExtLaunchKernelGGL), so the duration is the kernel's, as rocprofv3 reports it.
    hipEvent_t c0 = nullptr, c1 = nullptr, m0 = nullptr, m1 = nullptr, e0 = nullptr, e1 = nullptr;
    if (timed) CHECKED(TimedPair(kTimedControl, &c0, &c1));
    {
        Annotation a("Control", !capturing);
        // (RenderImages' iterations claim from the block list while adaptive sampling is on)
        Film claims = film;
        claims.blockList = sequenced && adaptive ? dBlockList : nullptr;
        hipExtLaunchKernelGGL(control_kernel, dim3(controlGrid), dim3(kControlBlock), 0, stream, c0, c1, 0, pool, claims,
                              (const FrameConstants*)dFrame, cnt, (const Counters*)next, dGlobals, (uint32_t)(film.debugRng != nullptr));
    }
    // (the fused variant with the CELLS cast, and only with it: FusedShadow)
    const bool fused = FusedShadow();
    ShadowInline si{};
    if (fused) si = ShadowInline{ plan.sceneFlat.nodes, plan.sceneFlat.shadowCells, plan.sceneFlat.shadowLeaves, plan.sceneFlat.cachedNodes, plan.sceneFlat.shadowRes };
    if (timed) CHECKED(TimedPair(kTimedMaterial, &m0, &m1));
    {
        Annotation a("Material", !capturing);
        hipExtLaunchKernelGGL(material.Kernel(rowProbe, fused), dim3(materialGrid), dim3(kMaterialBlock), material.LdsBytes(rowProbe, fused), stream, m0, m1, 0, pool, plan.scene,
                              (const FrameConstants*)dFrame, cnt, (const Counters*)next, (const SampleOut*)dSampleOut, si);
    }
    if (timed) CHECKED(TimedPair(kTimedCast, &e0, &e1));
    Annotation castAnnotation(knobs.mergedCasts ? "Extension + shadow ray cast" : "Extension ray cast, shadow ray cast", !capturing);
    if (knobs.mergedCasts) {
        hipExtLaunchKernelGGL(cast.kernel, dim3(castGrid), dim3(castBlock), cast.lds, stream, e0, e1, 0, pool, cast.scene,
                              (const FrameConstants*)dFrame, cnt, next, dGlobals, dInstr);
    } else {
        auto ext = instrCounters ? (opacity ? extension_kernel<true, true> : extension_kernel<true, false>)
                                 : (opacity ? extension_kernel<false, true> : extension_kernel<false, false>);
        auto shadow = instrCounters ? (opacity ? shadow_kernel<true, true> : shadow_kernel<true, false>)
                                    : (opacity ? shadow_kernel<false, true> : shadow_kernel<false, false>);
        hipExtLaunchKernelGGL(ext, dim3(castGrid), dim3(castBlock), cast.lds, stream, e0, e1, 0, pool, cast.scene,
                              (const FrameConstants*)dFrame, (const Counters*)cnt, dGlobals, dInstr);
        hipLaunchKernelGGL(shadow, dim3(castGrid), dim3(castBlock), cast.lds, stream, pool, cast.scene, (const FrameConstants*)dFrame, cnt,
                           next, dGlobals, dInstr);
    }
    if (knobs.drainPaths) {
        // (returns at once unless the batch's last paths are few enough: fc.drainPaths)
        hipLaunchKernelGGL(material.DrainKernel(), dim3(material.drainGrid), dim3(castBlock), plan.ldsWholeStack, stream, pool, plan.scene, (const FrameConstants*)dFrame, cnt,
                           dGlobals, (const SampleOut*)dSampleOut);
    }
    if (sequenced) {
        CHECKED(LaunchFilm(1u, dGlobals, nullptr, nullptr, 0u));
        hipLaunchKernelGGL(advance_image_kernel, dim3(1), dim3(64), 0, stream, dFrame, dGlobals);
    }
    HIPCHECK(hipGetLastError());
    return DCRT_OK;
}

// Replay `iters` iterations (even, starting at parity 0) as one captured graph.
// RenderImages' graph of tail chunks (its final batch) holds kTailChunk iterations
static uint32_t GraphSlot(bool sequenced, uint32_t iters) { return !sequenced ? 0u : (iters == kTailChunk ? 2u : 1u); }
int dcrt_tracer::LaunchGraph(bool sequenced, uint32_t iters)
{
    Annotation an(sequenced ? "Iterations (graph, sequenced images)" : "Iterations (graph)");
    CHECKED(BuildGraph(sequenced, iters));
    HIPCHECK(hipGraphLaunch(graphs[GraphSlot(sequenced, iters)].exec, stream));
    return DCRT_OK;
}

// Capture (once) the graph of `iters` iterations; kernels take the buffers by value, so
// a reallocation (EnsureSamples) invalidates it.
int dcrt_tracer::BuildGraph(bool sequenced, uint32_t iters)
{
    GraphCache& gc = graphs[GraphSlot(sequenced, iters)];
    if (!gc.exec || gc.iters != iters) {
        if (gc.exec) (void)hipGraphExecDestroy(gc.exec);
        gc.exec = nullptr;
        hipGraph_t g = nullptr;
        HIPCHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
        int rc = DCRT_OK;
        capturing = true;
        for (uint32_t i = 0; i < iters && rc == DCRT_OK; ++i) rc = LaunchIteration(i & 1u, false, sequenced);
        capturing = false;
        hipError_t ec = hipStreamEndCapture(stream, &g);
        if (rc != DCRT_OK) return rc;
        HIPCHECK(ec);
        HIPCHECK(hipGraphInstantiate(&gc.exec, g, nullptr, nullptr, 0));
        (void)hipGraphDestroy(g);
        gc.iters = iters;
    }
    return DCRT_OK;
}

// What RenderImages(count) would allocate or capture on its first call: the batch's
// sample textures and the sequenced graph. Lets a caller keep both out of a timed region.
int dcrt_tracer::PrepareImages(uint32_t count)
{
    if (!hasScene) { SetLastError("no scene uploaded"); return DCRT_E_NO_SCENE; }
    if (!hasFrame) { SetLastError("no frame parameters"); return DCRT_E_INVALID_ARG; }
    if (count == 0 || mode == 1) return DCRT_OK;
    // (also the slots of a render without the film pass, which keeps every image: slot k = image k)
    const uint64_t keptCap = std::min<uint64_t>(kMaxImageBatch, ((uint64_t)1 << 31) / ((uint64_t)filmW * filmH));
    CHECKED(EnsureSamples(std::max<uint32_t>(AutoBatch(count), count <= keptCap ? count : 0u)));
    if (!extTiming) {
        const uint32_t chunk = std::max<uint32_t>(2, iterationsPerRender & ~1u);
        CHECKED(BuildGraph(true, chunk));
        if (chunk > kTailChunk) CHECKED(BuildGraph(true, kTailChunk));
    }
    HIPCHECK(hipStreamSynchronize(stream));
    return DCRT_OK;
}

// n plain iterations (Render); even chunks replay a captured graph.
int dcrt_tracer::RunIterations(uint32_t n)
{
    const uint32_t chunk = std::max<uint32_t>(2, iterationsPerRender & ~1u);
    while (n > 0) {
        if (!extTiming && parity == 0 && n >= chunk) {
            CHECKED(LaunchGraph(false, chunk));
            n -= chunk;
        } else {
            CHECKED(LaunchIteration(parity, extTiming, false));
            parity ^= 1u;
            --n;
        }
    }
    return DCRT_OK;
}

// IsImageComplete (WavefrontPathTracer.cpp:508-523): no path was live entering the last
// iteration and none was started (Globals::poolIdle). Here exact, not 2 frames late.
int dcrt_tracer::ReadCompletion(bool* complete)
{
    HIPCHECK(hipMemcpyAsync(hPoolIdle.get(), &dGlobals->poolIdle, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    *complete = hPoolIdle[0] != 0;
    return DCRT_OK;
}

// One first-hit view image (dcrt_tracer_set_output) of the frame constants BeginImage uploaded,
// into sample slot 0: one persistent launch, as the megakernel's
int dcrt_tracer::LaunchView() { return LaunchView(output.output_type, film); }

// ... of output `type` into the sample textures of `target` (RenderGuides: the tracer's own, by value)
int dcrt_tracer::LaunchView(uint32_t type, const Film& target)
{
    Annotation an("Output view", !capturing);
    const bool opacity = (frame.features & DCRT_FEATURE_ALLOW_ANYHIT) != 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (extTiming) CHECKED(TimedPair(kTimedCast, &e0, &e1));
    auto vk = opacity ? view_kernel<true> : view_kernel<false>;
    hipExtLaunchKernelGGL(vk, dim3(opacity ? viewResidentOpacity : viewResident), dim3(plan.block), plan.ldsWholeStack, stream, e0, e1, 0, plan.scene,
                          (const FrameConstants*)dFrame, target, dGlobals, (uint32_t)(target.debugRng != nullptr), type,
                          output.iteration_threshold);
    HIPCHECK(hipGetLastError());
    return DCRT_OK;
}

int dcrt_tracer::Render(uint32_t maxIterations)
{
    if (!hasScene) { SetLastError("no scene uploaded"); return DCRT_E_NO_SCENE; }
    if (!hasFrame) { SetLastError("no frame parameters"); return DCRT_E_INVALID_ARG; }
    CHECKED(CheckFrameLights());
    if (output.output_type != DCRT_OUTPUT_PATH_TRACING) {
        // a view image is one launch: the whole image of the current frame seed, complete on return
        SlotZeroOverwritten();
        CHECKED(BeginImage());
        CHECKED(LaunchView());
        HIPCHECK(hipStreamSynchronize(stream));
        ++imagesCompleted;
        imageComplete = true;
        newImage = true;
        return DCRT_OK;
    }
    // (a progressive image fills slot 0 in every block; what an earlier render_images kept stays on offer)
    inactiveFilled = false;
    lastSlot = 0;
    if (newImage) CHECKED(BeginImage());
    CHECKED(RunIterations(maxIterations ? maxIterations : iterationsPerRender));
    bool complete = false;
    CHECKED(ReadCompletion(&complete));
    if (complete) ++imagesCompleted;
    imageComplete = complete;
    newImage = complete;   // WavefrontPathTracer.cpp:500
    return DCRT_OK;
}

int dcrt_tracer::UploadFilter(const dcrt_filter_params& f)
{
    CHECKED(dcrt::CheckFilterParams(f));        // (refused before anything is enqueued or changed)
    HIPCHECK(hipStreamSynchronize(stream));     // the pinned staging buffer is reused
    *hFilter.get() = MakeFilter(f);
    lastFilter = f;
    hasFilter = true;
    HIPCHECK(hipMemcpyAsync(dFilter, hFilter.get(), sizeof(FilterConsts), hipMemcpyHostToDevice, stream));
    return DCRT_OK;
}

int dcrt_tracer::Accumulate(const dcrt_filter_params& f)
{
    Annotation an("SampleConvolution");
    if (!film.accum) { SetLastError("no film"); return DCRT_E_INVALID_ARG; }
    CHECKED(UploadFilter(f));
    CHECKED(LaunchFilm(1u, nullptr, nullptr, nullptr, filmImages));
    HIPCHECK(hipGetLastError());
    ++filmImages;
    return DCRT_OK;
}

// The guide films and the denoised image, W x H of the film; EnsureFilm drops them with it.
int dcrt_tracer::EnsureGuides()
{
    if (guideNormal) return DCRT_OK;
    if (!film.accum) { SetLastError("no film"); return DCRT_E_INVALID_ARG; }
    const size_t n = (size_t)filmW * filmH;
    CHECKED(filmAllocs.Alloc(&guideNormal, n));
    CHECKED(filmAllocs.Alloc(&guideAlbedo, n));
    CHECKED(filmAllocs.Alloc(&denoised, n));
    return DCRT_OK;
}

// The denoiser's guides: for each seed the first-hit shading-normal and albedo views (view_kernel,
// the sub-pixel positions of the path-traced image of that seed), convolved with the film's
// reconstruction filter into the two guide films. The film, the selected output, the frame seed
// and the counters stay; the sample textures (slot 0) and the path pool are overwritten.
int dcrt_tracer::RenderGuides(uint32_t firstSeed, uint32_t count)
{
    Annotation an("RenderGuides");
    if (!hasScene) { SetLastError("no scene uploaded"); return DCRT_E_NO_SCENE; }
    if (!hasFrame) { SetLastError("no frame parameters"); return DCRT_E_INVALID_ARG; }
    if (!hasFilter) { SetLastError("render_guides convolves with the film's filter: render or accumulate the film first"); return DCRT_E_INVALID_ARG; }
    CHECKED(CheckFrameLights());
    CHECKED(CheckHalo(lastFilter.radius));
    CHECKED(EnsureGuides());
    const size_t n = (size_t)filmW * filmH;
    HIPCHECK(hipMemsetAsync(guideNormal, 0, n * sizeof(float4), stream));
    HIPCHECK(hipMemsetAsync(guideAlbedo, 0, n * sizeof(float4), stream));
    guidesRendered = false;
    SlotZeroOverwritten();   // (slot 0 holds the last guide image now)
    const uint32_t seed = frame.frame_seed;
    int rc = DCRT_OK;
    for (uint32_t img = 0; img < count && rc == DCRT_OK; ++img) {
        for (int which = 0; which < 2 && rc == DCRT_OK; ++which) {
            Film target = film;
            target.accum = which == 0 ? guideNormal : guideAlbedo;
            frame.frame_seed = firstSeed + img;
            rc = BeginImage();
            if (rc == DCRT_OK) rc = LaunchView(which == 0 ? DCRT_OUTPUT_SHADING_NORMAL : DCRT_OUTPUT_ALBEDO, target);
            if (rc != DCRT_OK) break;
            (void)LaunchFilm(target, nullptr, false, 1u, nullptr, nullptr, nullptr, 0u);   // (a guide film: never timed, no half)
            if (hipGetLastError() != hipSuccess) { SetLastError("guide film pass failed to launch"); rc = DCRT_E_HIP; }
        }
    }
    frame.frame_seed = seed;
    newImage = true;   // (BeginImage reset the pool: a progressive image in flight starts over)
    if (rc != DCRT_OK) return rc;
    HIPCHECK(hipStreamSynchronize(stream));
    guidesRendered = true;
    return DCRT_OK;
}

// Images firstSeed .. firstSeed+count-1 back to back: the device detects each
// image's completion, convolves it into the film and starts the next one, so the
// host only enqueues graphs and polls a pinned "stopped" word two graphs behind.
int dcrt_tracer::RenderImages(uint32_t firstSeed, uint32_t count, const dcrt_filter_params& filter, uint32_t stride, bool convolve)
{
    CHECKED(dcrt::CheckFilterParams(filter));   // (before the seed stride, the kept slots and the sample textures change)
    seedStride = std::max<uint32_t>(1u, stride);
    keptSlots = false;
    Annotation an("RenderImages");
    if (!hasScene) { SetLastError("no scene uploaded"); return DCRT_E_NO_SCENE; }
    if (!hasFrame) { SetLastError("no frame parameters"); return DCRT_E_INVALID_ARG; }
    CHECKED(CheckFrameLights());
    if (count == 0) return DCRT_OK;
    CHECKED(CheckHalo(filter.radius));
    lastSlot = 0;
    // MegakernelPathTracer::Render: one persistent launch + SampleConvolution per image -- the
    // path-tracing megakernel, or the first-hit kernel of the selected output view
    const bool view = output.output_type != DCRT_OUTPUT_PATH_TRACING;
    // adaptive sampling: the path-traced images start paths in the listed blocks only (the views
    // run over every block)
    const bool listed = adaptive && !view;
    if (listed && listCount == 0) { SetLastError("adaptive sampling: nothing left to sample (the block list is empty)"); return DCRT_E_INVALID_ARG; }
    if (view || mode == 1) {
        if (!convolve) {
            SetLastError(view ? "an output view convolves every image" : "the megakernel mode convolves every image");
            return DCRT_E_INVALID_ARG;
        }
        CHECKED(UploadFilter(filter));
        if (listed) CHECKED(FillInactive());
        if (view) SlotZeroOverwritten();   // (slot 0 gets a whole view image)
        Film claims = film;
        claims.blockList = listed ? dBlockList : nullptr;
        for (uint32_t img = 0; img < count; ++img) {
            frame.frame_seed = firstSeed + img * seedStride;
            listFrame = listed;
            const int rc = BeginImage();
            listFrame = false;
            CHECKED(rc);
            if (view) {
                CHECKED(LaunchView());
            } else {
                hipEvent_t e0 = nullptr, e1 = nullptr;
                if (extTiming) CHECKED(TimedPair(kTimedCast, &e0, &e1));
                auto mk = material.Megakernel((frame.features & DCRT_FEATURE_ALLOW_ANYHIT) != 0);
                hipExtLaunchKernelGGL(mk, dim3(megaResident), dim3(plan.block), plan.ldsWholeStack, stream, e0, e1, 0, plan.scene,
                                      (const FrameConstants*)dFrame, claims, dGlobals, (uint32_t)(film.debugRng != nullptr));
            }
            CHECKED(LaunchFilm(1u, nullptr, nullptr, nullptr, filmImages));
            HIPCHECK(hipGetLastError());
            ++filmImages;
        }
        HIPCHECK(hipStreamSynchronize(stream));
        imageComplete = true;
        newImage = true;
        imagesCompleted += count;
        if (listed) pathsSkipped += (uint64_t)count * ((uint64_t)rowCount * filmW - listPixels);
        return DCRT_OK;
    }
    uint32_t batch = AutoBatch(count);
    if (!convolve) {
        // every image keeps its samples (slot k = image k) for the caller's film pass: one batch
        const uint64_t cap = std::min<uint64_t>(kMaxImageBatch, ((uint64_t)1 << 31) / ((uint64_t)filmW * filmH));
        if (count > cap) { SetLastError("render_images without the film pass: too many images for one batch"); return DCRT_E_LIMIT; }
        batch = count;
    }
    CHECKED(EnsureSamples(batch));
    frame.frame_seed = firstSeed;
    CHECKED(UploadFilter(filter));
    if (listed) CHECKED(FillInactive());   // (after EnsureSamples: the slots the film pass reads)
    listFrame = listed;
    const int began = BeginImage();
    listFrame = false;
    CHECKED(began);
    // static batch-start claims: one per wave of CONTROL's virtual workgroups
    const uint32_t staticGrid = poolSize / kControlBlock;
    hipLaunchKernelGGL(begin_images_kernel, dim3(1), dim3(64), 0, stream, dGlobals, (const FrameConstants*)dFrame, count, firstSeed, batch,
                       staticGrid, convolve ? 0u : 1u, filmImages);
    HIPCHECK(hipGetLastError());
    // a path needs maxBounce + 3 iterations; cap the total so a broken scene cannot spin forever
    const uint64_t maxIterations = ((uint64_t)count + 2) * (frame.max_bounce_count + 8) * (1 + (filmW * (uint64_t)filmH) / poolSize) + 64;
    uint64_t launched = 0;
    bool stopped = false;
    {
        // chunks of `chunk` iterations (a replayed graph, or plain timed launches when the
        // EXT kernel is being timed), the "stopped" word polled two chunks behind; once the
        // final batch is in flight (imagesDone + batch >= count, polled with it), chunks of
        // kTailChunk: the chunks launched after the last image completes find no work
        // (32 empty iterations after a one-batch call took 0.4 ms with 16-iteration chunks)
        const uint32_t bigChunk = std::max<uint32_t>(2, iterationsPerRender & ~1u);
        bool finalBatch = count <= batch;
        uint32_t inflight[4];
        uint32_t head = 0, size = 0, slot = 0;
        while (!stopped && launched < maxIterations) {
            const uint32_t chunk = finalBatch ? std::min(bigChunk, kTailChunk) : bigChunk;
            if (extTiming) {
                for (uint32_t i = 0; i < chunk; ++i) {
                    CHECKED(LaunchIteration(parity, true, true));
                    parity ^= 1u;
                }
            } else {
                CHECKED(LaunchGraph(true, chunk));
            }
            launched += chunk;
            static_assert(offsetof(Globals, imagesDone) == offsetof(Globals, stopped) + 4, "polled together");
            HIPCHECK(hipMemcpyAsync(&hStop[2 * slot], &dGlobals->stopped, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
            HIPCHECK(hipEventRecord(stopEvents[slot], stream));
            inflight[(head + size) % 4] = slot;
            ++size;
            slot = (slot + 1) % 4;
            if (size >= 2) {
                const uint32_t s0 = inflight[head];
                HIPCHECK(hipEventSynchronize(stopEvents[s0]));
                stopped = hStop[2 * s0] != 0;
                finalBatch = finalBatch || (uint64_t)hStop[2 * s0 + 1] + batch >= count;
                head = (head + 1) % 4;
                --size;
            }
        }
        // graphs still in flight after `stopped` find no work (CONTROL returns at once)
    }
    HIPCHECK(hipStreamSynchronize(stream));
    if (!stopped) {
        HIPCHECK(hipMemcpy(hStop.get(), &dGlobals->stopped, sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (!hStop[0]) { SetLastError("images did not complete"); return DCRT_E_LIMIT; }
    }
    imageComplete = true;
    newImage = true;
    imagesCompleted += count;
    if (listed) pathsSkipped += (uint64_t)count * ((uint64_t)rowCount * filmW - listPixels);
    if (convolve) filmImages += count;
    lastSlot = (count - 1) % batch;
    keptSlots = !convolve;
    keptImages = keptSlots ? count : 0u;
    return DCRT_OK;
}

// The film pass over `count` images whose sample textures (W*H each, this film's size) sit at
// the caller's device pointers -- e.g. the slots of several pipelines that rendered interleaved
// images (render_images without the film pass): image b of the list is convolved b-th, so the
// film is the one-pipeline film bit for bit when the list is in image order.
int dcrt_tracer::AccumulateImages(const void* const* pos, const void* const* val, uint32_t count, const dcrt_filter_params& f)
{
    Annotation an("SampleConvolution (image list)");
    if (!film.accum) { SetLastError("no film"); return DCRT_E_INVALID_ARG; }
    CHECKED(dcrt::CheckFilterParams(f));
    if (count == 0) return DCRT_OK;
    if (count > sourceCap) {
        HIPCHECK(hipStreamSynchronize(stream));
        sourceAllocs.Free();
        sourceCap = 0;
        CHECKED(sourceAllocs.Alloc(&dSourceLists, (size_t)count * 2));
        sourceCap = count;
    }
    std::vector<const void*> lists((size_t)count * 2);
    for (uint32_t i = 0; i < count; ++i) {
        if (!pos[i] || !val[i]) { SetLastError("null sample texture pointer"); return DCRT_E_INVALID_ARG; }
        lists[i] = pos[i];
        lists[count + i] = val[i];
    }
    CHECKED(UploadFilter(f));   // (synchronises: the list's staging below is reused safely)
    HIPCHECK(hipMemcpyAsync(dSourceLists, lists.data(), lists.size() * sizeof(void*), hipMemcpyHostToDevice, stream));
    CHECKED(LaunchFilm(count, nullptr, (const float2* const*)dSourceLists, (const float4* const*)(dSourceLists + count), filmImages));
    HIPCHECK(hipGetLastError());
    filmImages += count;
    HIPCHECK(hipStreamSynchronize(stream));   // (the host list is released on return)
    return DCRT_OK;
}

// ---- the film pass, the films and the film noise estimate -------------------------------------
// A film pass into `target` (of the film's size): film_kernel, or with `half` the kernel that also feeds that
// half film (firstIndex: the film image count of the pass's first image; under `guard` the kernel takes it from
// Globals instead). The tracer's own film takes the overload in the struct.
int dcrt_tracer::LaunchFilm(const Film& target, float4* half, bool timed, uint32_t images, const Globals* guard, const float2* const* posList,
                            const float4* const* valList, uint32_t firstIndex)
{
    if (timed) {
        // timed (ext_timing): the dispatch's own timestamps, as the cast / MATERIAL / CONTROL launches'
        hipEvent_t e0 = nullptr, e1 = nullptr;
        CHECKED(TimedPair(kTimedFilm, &e0, &e1));
        if (half) {
            hipExtLaunchKernelGGL(film_half_kernel, dim3(FilmGrid()), dim3(kFilmThreads), 0, stream, e0, e1, 0, target,
                                  (const FilterConsts*)dFilter, images, guard, posList, valList, half, firstIndex);
        } else {
            hipExtLaunchKernelGGL(film_kernel, dim3(FilmGrid()), dim3(kFilmThreads), 0, stream, e0, e1, 0, target,
                                  (const FilterConsts*)dFilter, images, guard, posList, valList);
        }
    } else if (half) {
        hipLaunchKernelGGL(film_half_kernel, dim3(FilmGrid()), dim3(kFilmThreads), 0, stream, target, (const FilterConsts*)dFilter, images,
                           guard, posList, valList, half, firstIndex);
    } else {
        hipLaunchKernelGGL(film_kernel, dim3(FilmGrid()), dim3(kFilmThreads), 0, stream, target, (const FilterConsts*)dFilter, images,
                           guard, posList, valList);
    }
    return DCRT_OK;
}

// dst += src, two W x H films on the device (the films of disjoint film partitions). Synchronous.
int dcrt_tracer::AddFilm(float4* dst, const void* src)
{
    const uint32_t n = filmW * filmH;
    hipLaunchKernelGGL(add_film_kernel, dim3(std::min<uint32_t>((n + 255) / 256, kMaxPersistentBlocks)), dim3(256), 0, stream, dst,
                       (const float4*)src, n);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(stream));
    return DCRT_OK;
}

// A W x H float4 image of the film's size to the host. Synchronous.
int dcrt_tracer::ReadImage(const float4* image, float* out)
{
    HIPCHECK(hipMemcpyAsync(out, image, (size_t)filmW * filmH * sizeof(float4), hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    return DCRT_OK;
}

int dcrt_tracer::NeedHalfFilm() const
{
    if (!halfFilm) { SetLastError("no half film: convergence is off (dcrt_tracer_set_convergence)"); return DCRT_E_INVALID_ARG; }
    return DCRT_OK;
}

int dcrt_tracer::ClearFilm()
{
    if (!film.accum) return DCRT_E_INVALID_ARG;
    const size_t bytes = (size_t)filmW * filmH * sizeof(float4);
    HIPCHECK(hipMemsetAsync(film.accum, 0, bytes, stream));
    if (halfFilm) HIPCHECK(hipMemsetAsync(halfFilm, 0, bytes, stream));
    for (uint32_t j = 0; firefly && j < fireflyParams.cascades; ++j) HIPCHECK(hipMemsetAsync(cascades.film[j], 0, bytes, stream));
    hasReweighted = false;
    filmImages = 0;
    if (adaptive) CHECKED(ResetBlockList());   // (an empty film is noisy everywhere)
    return DCRT_OK;
}

int dcrt_tracer::SetConvergence(bool on)
{
    if (!film.accum) { SetLastError("set_convergence: no film (set the frame parameters first)"); return DCRT_E_INVALID_ARG; }
    HIPCHECK(hipStreamSynchronize(stream));
    if (on != convergence) InvalidateGraph();   // (the in-graph film pass is another kernel)
    if (on && !halfFilm) CHECKED(halfAllocs.Alloc(&halfFilm, (size_t)filmW * filmH));
    if (!on) {
        halfAllocs.Free();
        halfFilm = nullptr;
    }
    convergence = on;
    return ClearFilm();
}

// The K cascade films and the re-weighted image, W x H of the film (EnsureFilm and SetFirefly drop them first)
int dcrt_tracer::AllocCascades()
{
    const size_t n = (size_t)filmW * filmH;
    for (uint32_t j = 0; j < fireflyParams.cascades; ++j) {
        CHECKED(cascadeAllocs.Alloc(&cascades.film[j], n));
        HIPCHECK(hipMemsetAsync(cascades.film[j], 0, n * sizeof(float4), stream));
    }
    return cascadeAllocs.Alloc(&reweighted, n);
}

// ... or, where that fails, none of them and the feature off: no film pass launches onto a missing cascade
int dcrt_tracer::AllocCascadesOrOff()
{
    const int rc = AllocCascades();
    firefly = rc == DCRT_OK;
    if (!firefly) {
        cascadeAllocs.Free();
        cascades = CascadeFilms{};
        reweighted = nullptr;
    }
    return rc;
}

// dcrt_tracer_set_firefly: on with `p`, off with null; either way the films are cleared
int dcrt_tracer::SetFirefly(const dcrt_firefly_params* p)
{
    if (!film.accum) { SetLastError("set_firefly: no film (set the frame parameters first)"); return DCRT_E_INVALID_ARG; }
    FireflyConsts k{};
    if (p) {
        CHECKED(FireflyFilter::MakeConsts(*p, &k));
        if (Partitioned()) {
            SetLastError("set_firefly: a banded or partitioned film; reduce the films and cascades and use dcrt_tracer_firefly_resolve_device");
            return DCRT_E_INVALID_ARG;
        }
    }
    HIPCHECK(hipStreamSynchronize(stream));
    const bool on = p != nullptr;
    // the in-graph cascade launch carries K and the scales as kernel arguments; min_support is the resolve's alone
    const bool same = on == firefly && (!on || (p->cascades == fireflyParams.cascades && p->start == fireflyParams.start &&
                                                p->base == fireflyParams.base));
    if (!same) {
        InvalidateGraph();
        CHECKED(ClearFilm());   // (with the cascades it had: nothing in flight writes them after the free below)
        HIPCHECK(hipStreamSynchronize(stream));
        cascadeAllocs.Free();
        cascades = CascadeFilms{};
        reweighted = nullptr;
        firefly = false;
        if (on) {
            fireflyParams = *p;
            CHECKED(AllocCascadesOrOff());
        }
    }
    if (on) {
        fireflyParams = *p;
        fireflyConsts = k;
    }
    return ClearFilm();
}

// ... of the tracer's own film, into its own maps
int dcrt_tracer::NoiseOwn(float threshold, dcrt_noise_stats* out)
{
    if (!out) return DCRT_E_INVALID_ARG;
    if (!convergence || !halfFilm) { SetLastError("noise: convergence is off (dcrt_tracer_set_convergence)"); return DCRT_E_INVALID_ARG; }
    if (filmImages < 2) { SetLastError("noise: the film holds fewer than 2 images"); return DCRT_E_INVALID_ARG; }
    if (!(threshold >= 0.0f)) { SetLastError("noise: the threshold is negative or NaN"); return DCRT_E_INVALID_ARG; }
    if (!noisePixelMap) {
        const uint32_t T = (uint32_t)kNoiseTile;
        CHECKED(noiseMapAllocs.Alloc(&noisePixelMap, (size_t)filmW * filmH));
        CHECKED(noiseMapAllocs.Alloc(&noiseTileMap, (size_t)((filmW + T - 1) / T) * ((filmH + T - 1) / T)));
    }
    hasNoiseMaps = false;
    CHECKED(noiseEstimator.Run(stream, filmW, filmH, film.accum, halfFilm, threshold, noisePixelMap, noiseTileMap, out));
    out->images = filmImages;
    hasNoiseMaps = true;
    return DCRT_OK;
}

// Render until the estimate meets the target: RenderImages between the check points (film image
// counts min, min + interval, ..., capped at max), the image with film image count i of seed
// firstSeed + i, so the film at count n is RenderImages(firstSeed, n)'s.
// adaptiveCall (render_adaptive): the same loop with the block list rebuilt at every check point that
// goes on -- the list is a function of the film, the half film, the threshold and the margin alone, so a
// block whose neighbourhood turns noisy again wakes up. The call starts on every block, and fills in
// `report` once it has.
int dcrt_tracer::RenderConverged(uint32_t firstSeed, const dcrt_converge_params& p, const dcrt_filter_params& filter, dcrt_noise_stats* outStats,
                                 int* outConverged, const AdaptiveCall* adaptiveCall)
{
    const char* const prefix = adaptiveCall ? "render_adaptive" : "render_converged";
    auto refuse = [&](const char* what, int code) { SetLastError(std::string(prefix) + what); return code; };
    if (adaptiveCall && !adaptive) return refuse(": adaptive sampling is off (dcrt_tracer_set_adaptive)", DCRT_E_INVALID_ARG);
    if (!convergence || !halfFilm) return refuse(": convergence is off (dcrt_tracer_set_convergence)", DCRT_E_INVALID_ARG);
    if (!(p.threshold >= 0.0f) || !(p.target_fraction > 0.0f && p.target_fraction <= 1.0f) || p.min_images < 2u ||
        p.max_images < p.min_images || p.check_interval < 1u)
        return refuse(": threshold >= 0, 0 < target_fraction <= 1, 2 <= min_images <= max_images, check_interval >= 1", DCRT_E_INVALID_ARG);
    CHECKED(dcrt::CheckFilterParams(filter));
    dcrt_adaptive_report rep{};
    uint32_t margin = 0;
    if (adaptiveCall) {
        margin = adaptiveCall->margin == 0xFFFFFFFFu ? FilterSupportRows(filter.radius, filmH) : adaptiveCall->margin;
        CHECKED(ResetBlockList());
        rep.total_blocks = blockTotal;
        rep.active_blocks = listCount;
    }
    *outConverged = 0;
    int rc = DCRT_OK;
    for (uint64_t point = p.min_images; rc == DCRT_OK; point += p.check_interval) {
        const uint32_t target = (uint32_t)std::min<uint64_t>(point, p.max_images);
        if (filmImages < target) {
            const uint32_t n = target - filmImages;
            rc = RenderImages(firstSeed + filmImages, n, filter);
            if (rc != DCRT_OK) break;
            rep.images += n;
            rep.pixel_samples += (uint64_t)n * listPixels;
        }
        if (filmImages < target) { rc = refuse(": the images did not reach the film", DCRT_E_LIMIT); break; }
        rc = NoiseOwn(p.threshold, outStats);
        if (rc != DCRT_OK) break;
        ++rep.check_points;
        if ((double)outStats->converged_pixels >= (double)p.target_fraction * (double)outStats->valid_pixels) { *outConverged = 1; break; }
        if (filmImages >= p.max_images) break;
        if (!adaptiveCall) continue;
        rc = UpdateSampleBlocks(p.threshold, margin, &rep.active_blocks);
        if (rc == DCRT_OK && rep.active_blocks == 0u) { *outConverged = 1; break; }
    }
    if (adaptiveCall && adaptiveCall->report) *adaptiveCall->report = rep;
    return rc;
}

// ---- adaptive sampling (dcrt.h "adaptive sampling") -----------------------------------------
// The flag and list buffers of the film's blocks (room for every block, so film.blockList is one
// pointer while the resolution stands), the list set to every block.
int dcrt_tracer::AllocBlockList()
{
    HIPCHECK(hipStreamSynchronize(stream));
    InvalidateGraph();   // (captured CONTROL launches hold the old list pointer)
    adaptiveAllocs.Free();
    dBlockFlags = dBlockList = nullptr;
    blockTotal = ((filmW + kBlockW - 1) / kBlockW) * ((filmH + kBlockH - 1) / kBlockH);
    CHECKED(adaptiveAllocs.Alloc(&dBlockFlags, blockTotal));
    CHECKED(adaptiveAllocs.Alloc(&dBlockList, blockTotal));
    return ResetBlockList();
}

int dcrt_tracer::ResetBlockList()
{
    hipLaunchKernelGGL(all_blocks_kernel, dim3(std::min<uint32_t>((blockTotal + 255) / 256, kMaxPersistentBlocks)), dim3(256), 0, stream,
                       dBlockFlags, dBlockList, blockTotal);
    HIPCHECK(hipGetLastError());
    listCount = blockTotal;
    listPixels = filmW * filmH;
    inactiveFilled = false;
    return DCRT_OK;
}

int dcrt_tracer::SetAdaptive(bool on)
{
    if (!film.accum) { SetLastError("set_adaptive: no film (set the frame parameters first)"); return DCRT_E_INVALID_ARG; }
    if (on && (partition.world_size > 1 || !bands.empty())) {
        SetLastError("set_adaptive: not on a partitioned or banded film");
        return DCRT_E_INVALID_ARG;
    }
    HIPCHECK(hipStreamSynchronize(stream));
    if (on == adaptive) return on ? ResetBlockList() : DCRT_OK;
    InvalidateGraph();   // (the in-graph CONTROL launches take another Film)
    adaptive = on;
    if (on) return AllocBlockList();
    adaptiveAllocs.Free();
    dBlockFlags = dBlockList = nullptr;
    blockTotal = listCount = listPixels = 0;
    return DCRT_OK;
}

int dcrt_tracer::SetSampleBlocks(const uint32_t* blocks, uint32_t count)
{
    if (!adaptive) { SetLastError("set_sample_blocks: adaptive sampling is off (dcrt_tracer_set_adaptive)"); return DCRT_E_INVALID_ARG; }
    if (count > blockTotal || (count && !blocks)) { SetLastError("set_sample_blocks: more blocks than the film has"); return DCRT_E_INVALID_ARG; }
    const uint32_t blocksX = (filmW + kBlockW - 1) / kBlockW;
    std::vector<uint32_t> flags(blockTotal, 0u);
    uint64_t pixels = 0;
    for (uint32_t i = 0; i < count; ++i) {
        if (blocks[i] >= blockTotal || (i > 0 && blocks[i] <= blocks[i - 1])) {
            SetLastError("set_sample_blocks: block indices are strictly ascending and below blocksX * ceil(H / 8)");
            return DCRT_E_INVALID_ARG;
        }
        flags[blocks[i]] = 1u;
        const uint32_t by = blocks[i] / blocksX, bx = blocks[i] - by * blocksX;
        pixels += (uint64_t)std::min(kBlockW, filmW - bx * kBlockW) * std::min(kBlockH, filmH - by * kBlockH);
    }
    HIPCHECK(hipStreamSynchronize(stream));
    HIPCHECK(hipMemcpy(dBlockFlags, flags.data(), (size_t)blockTotal * 4, hipMemcpyHostToDevice));
    if (count) HIPCHECK(hipMemcpy(dBlockList, blocks, (size_t)count * 4, hipMemcpyHostToDevice));
    listCount = count;
    listPixels = (uint32_t)pixels;
    inactiveFilled = false;
    return DCRT_OK;
}

int dcrt_tracer::GetSampleBlocks(uint32_t* out, uint32_t capacity, uint32_t* outCount)
{
    if (!adaptive) { SetLastError("get_sample_blocks: adaptive sampling is off (dcrt_tracer_set_adaptive)"); return DCRT_E_INVALID_ARG; }
    if (!outCount || (capacity && !out)) return DCRT_E_INVALID_ARG;
    *outCount = listCount;
    const uint32_t n = std::min(capacity, listCount);
    if (n) {
        HIPCHECK(hipMemcpyAsync(out, dBlockList, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
    }
    return DCRT_OK;
}

// ... of the tracer's own film and half film into its own list
int dcrt_tracer::UpdateSampleBlocks(float threshold, uint32_t margin, uint32_t* outActive)
{
    if (!adaptive) { SetLastError("update_sample_blocks: adaptive sampling is off (dcrt_tracer_set_adaptive)"); return DCRT_E_INVALID_ARG; }
    if (!convergence || !halfFilm) { SetLastError("update_sample_blocks: convergence is off (dcrt_tracer_set_convergence)"); return DCRT_E_INVALID_ARG; }
    if (filmImages < 2) { SetLastError("update_sample_blocks: the film holds fewer than 2 images"); return DCRT_E_INVALID_ARG; }
    if (!(threshold >= 0.0f)) { SetLastError("update_sample_blocks: the threshold is negative or NaN"); return DCRT_E_INVALID_ARG; }
    if (margin == 0xFFFFFFFFu) {
        if (!hasFilter) { SetLastError("update_sample_blocks: no film pass has set the filter the default margin follows"); return DCRT_E_INVALID_ARG; }
        margin = FilterSupportRows(lastFilter.radius, filmH);
    }
    uint32_t count = 0, pixels = 0;
    CHECKED(blockSampler.Run(stream, extTiming, filmW, filmH, film.accum, halfFilm, threshold, margin, dBlockFlags, dBlockList, &count, &pixels));
    listCount = count;
    listPixels = pixels;
    inactiveFilled = false;
    if (outActive) *outActive = count;
    return DCRT_OK;
}

// The sentinel sample into every slot's inactive pixels. It runs before a listed RenderImages
// whenever a slot's inactive pixels may hold older samples: the list changed, EnsureSamples
// allocated or grew the slots, or a progressive / view / guide image went through slot 0.
int dcrt_tracer::FillInactive()
{
    if (inactiveFilled) return DCRT_OK;
    if (listCount < blockTotal)
        CHECKED(blockSampler.Fill(stream, extTiming, film.samplePosition, film.sampleValue, dBlockFlags, filmW, filmH, sampleImages));
    inactiveFilled = true;
    return DCRT_OK;
}

// ============================ C ABI ========================================
#define TRACER_GUARD(t)                                         \
    if (!(t)) return DCRT_E_INVALID_ARG;                        \
    if (hipSetDevice((t)->device) != hipSuccess) {              \
        SetLastError("hipSetDevice failed");                    \
        return DCRT_E_HIP;                                      \
    }

// The one round trip of caller arrays, n items each: inputs up, one launch, outputs down, the stream synchronised.
// The device copies come from the caller's group, which may hold more (ProbeScene's rows) and frees them all when
// it goes. n == 0 copies and launches nothing; an array with neither side is left out (its device pointer stays null).
struct HostArray {
    const void* in;       // copied up, or null
    void* out;            // copied down, or null
    size_t bytesPerItem;
    void* device = nullptr;
};
// `launch` takes no arguments: the caller picks the geometry (ItemGrid: one thread per item). A status it returns is kept.
template <size_t N, typename Launch>
static int RoundTrip(dcrt_tracer* t, DeviceGroup& group, uint32_t n, HostArray (&arrays)[N], Launch launch)
{
    int rc = DCRT_OK;
    for (HostArray& a : arrays) {
        if (rc != DCRT_OK || (!a.in && !a.out)) continue;
        char* d = nullptr;
        rc = group.Alloc(&d, (size_t)n * a.bytesPerItem);
        a.device = d;
        if (rc == DCRT_OK && a.in && n && hipMemcpyAsync(d, a.in, (size_t)n * a.bytesPerItem, hipMemcpyHostToDevice, t->stream) != hipSuccess) rc = DCRT_E_HIP;
    }
    if (rc == DCRT_OK && n) {
        if constexpr (std::is_void_v<decltype(launch())>) launch();
        else rc = launch();
        if (rc == DCRT_OK && hipGetLastError() != hipSuccess) rc = DCRT_E_HIP;
    }
    for (HostArray& a : arrays) {
        if (rc == DCRT_OK && a.out && n && hipMemcpyAsync(a.out, a.device, (size_t)n * a.bytesPerItem, hipMemcpyDeviceToHost, t->stream) != hipSuccess) rc = DCRT_E_HIP;
    }
    if (hipStreamSynchronize(t->stream) != hipSuccess) rc = DCRT_E_HIP;
    return rc;
}
static dim3 ItemGrid(uint32_t n) { return dim3((n + 255) / 256); }   // (with dim3(256) threads)

extern "C" {

DCRT_API int dcrt_device_count(int* out)
{
    if (!out) return DCRT_E_INVALID_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *out = n;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_create(const dcrt_tracer_config* config, dcrt_tracer** out)
{
    if (!out) return DCRT_E_INVALID_ARG;
    *out = nullptr;
    dcrt_tracer_config cfg{};
    if (config) cfg = *config;
    dcrt_tracer* t = new (std::nothrow) dcrt_tracer();
    if (!t) return DCRT_E_LIMIT;
    const int rc = t->Create(cfg);
    if (rc != DCRT_OK) { delete t; return rc; }
    *out = t;
    return DCRT_OK;
}

DCRT_API void dcrt_tracer_destroy(dcrt_tracer* t) { delete t; }

DCRT_API int dcrt_tracer_upload_scene(dcrt_tracer* t, const dcrt_flat_scene* s)
{
    TRACER_GUARD(t);
    if (!s) return DCRT_E_INVALID_ARG;
    return t->UploadScene(*s);
}

DCRT_API int dcrt_tracer_update_materials(dcrt_tracer* t, const dcrt_material* materials, uint32_t material_count)
{
    if (!t || !materials) return DCRT_E_INVALID_ARG;   // (before any device call)
    TRACER_GUARD(t);
    return t->UpdateMaterials(materials, material_count);
}

DCRT_API int dcrt_tracer_update_lights(dcrt_tracer* t, const dcrt_light* lights, uint32_t light_count)
{
    if (!t || (!lights && light_count)) return DCRT_E_INVALID_ARG;   // (no lights: a null array is fine)
    TRACER_GUARD(t);
    return t->UpdateLights(lights, light_count);
}

DCRT_API int dcrt_tracer_update_instance_flags(dcrt_tracer* t, const uint32_t* flags, uint32_t instance_count)
{
    if (!t || !flags) return DCRT_E_INVALID_ARG;
    TRACER_GUARD(t);
    return t->UpdateInstanceFlags(flags, instance_count);
}

DCRT_API int dcrt_tracer_upload_stats(dcrt_tracer* t, dcrt_upload_stats* out)
{
    if (!t || !out) return DCRT_E_INVALID_ARG;
    *out = t->uploadStats;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_set_frame_params(dcrt_tracer* t, const dcrt_frame_params* p)
{
    TRACER_GUARD(t);
    if (!p) return DCRT_E_INVALID_ARG;
    return t->SetFrame(*p);
}

DCRT_API int dcrt_tracer_set_film_partition(dcrt_tracer* t, const dcrt_film_partition* p)
{
    TRACER_GUARD(t);
    if (!p) return DCRT_E_INVALID_ARG;
    return t->SetPartition(*p);
}

DCRT_API int dcrt_tracer_set_film_bands(dcrt_tracer* t, const uint32_t* bands, uint32_t band_count, uint32_t halo_rows)
{
    TRACER_GUARD(t);
    return t->SetBands(bands, band_count, halo_rows);
}

DCRT_API int dcrt_tracer_render(dcrt_tracer* t, uint32_t max_iterations)
{
    TRACER_GUARD(t);
    return t->Render(max_iterations);
}

DCRT_API int dcrt_tracer_render_images(dcrt_tracer* t, uint32_t first_seed, uint32_t count, const dcrt_filter_params* f)
{
    TRACER_GUARD(t);
    if (!f) return DCRT_E_INVALID_ARG;
    return t->RenderImages(first_seed, count, *f);
}

DCRT_API int dcrt_tracer_render_images_strided(dcrt_tracer* t, uint32_t first_seed, uint32_t seed_stride, uint32_t count,
                                               int convolve, const dcrt_filter_params* f)
{
    TRACER_GUARD(t);
    if (!f || seed_stride == 0) return DCRT_E_INVALID_ARG;
    return t->RenderImages(first_seed, count, *f, seed_stride, convolve != 0);
}

DCRT_API int dcrt_tracer_image_sample_ptrs(dcrt_tracer* t, uint32_t image, void** pos, void** val)
{
    TRACER_GUARD(t);
    if (!pos || !val) return DCRT_E_INVALID_ARG;
    if (!t->keptSlots || image >= t->keptImages) {
        SetLastError("no such image: its samples are kept only by render_images without the film pass");
        return DCRT_E_INVALID_ARG;
    }
    const size_t o = (size_t)t->filmW * t->filmH * image;
    *pos = (void*)(t->film.samplePosition + o);
    *val = (void*)(t->film.sampleValue + o);
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_accumulate_images(dcrt_tracer* t, const void* const* d_positions, const void* const* d_values,
                                           uint32_t image_count, const dcrt_filter_params* f)
{
    TRACER_GUARD(t);
    if (!f || (image_count && (!d_positions || !d_values))) return DCRT_E_INVALID_ARG;
    return t->AccumulateImages(d_positions, d_values, image_count, *f);
}

DCRT_API int dcrt_tracer_reset_image(dcrt_tracer* t)
{
    TRACER_GUARD(t);
    t->newImage = true;
    t->imageComplete = false;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_is_image_complete(dcrt_tracer* t, int* out)
{
    TRACER_GUARD(t);
    if (!out) return DCRT_E_INVALID_ARG;
    *out = t->imageComplete ? 1 : 0;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_acquire_film_clear_trigger(dcrt_tracer* t, int* out)
{
    TRACER_GUARD(t);
    if (!out) return DCRT_E_INVALID_ARG;
    *out = t->filmClearTrigger ? 1 : 0;
    t->filmClearTrigger = false;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_clear_film(dcrt_tracer* t)
{
    TRACER_GUARD(t);
    return t->ClearFilm();
}

DCRT_API int dcrt_tracer_accumulate_film(dcrt_tracer* t, const dcrt_filter_params* f)
{
    TRACER_GUARD(t);
    if (!f) return DCRT_E_INVALID_ARG;
    return t->Accumulate(*f);
}

DCRT_API int dcrt_tracer_read_film(dcrt_tracer* t, float* out)
{
    TRACER_GUARD(t);
    if (!out || !t->film.accum) return DCRT_E_INVALID_ARG;
    return t->ReadImage(t->film.accum, out);
}

DCRT_API int dcrt_tracer_read_samples(dcrt_tracer* t, float* pos, float* val)
{
    TRACER_GUARD(t);
    if (!t->film.sampleValue) return DCRT_E_INVALID_ARG;
    const size_t n = (size_t)t->filmW * t->filmH, o = n * t->lastSlot;   // the last image's samples
    if (pos) HIPCHECK(hipMemcpyAsync(pos, t->film.samplePosition + o, n * sizeof(float2), hipMemcpyDeviceToHost, t->stream));
    if (val) HIPCHECK(hipMemcpyAsync(val, t->film.sampleValue + o, n * sizeof(float4), hipMemcpyDeviceToHost, t->stream));
    HIPCHECK(hipStreamSynchronize(t->stream));
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_read_rng(dcrt_tracer* t, uint32_t* out)
{
    TRACER_GUARD(t);
    if (!out || !t->film.debugRng) { SetLastError("tracer was created without debug_rng"); return DCRT_E_INVALID_ARG; }
    const size_t n = (size_t)t->filmW * t->filmH;
    HIPCHECK(hipMemcpyAsync(out, t->film.debugRng + n * t->lastSlot, n * sizeof(uint4), hipMemcpyDeviceToHost, t->stream));
    HIPCHECK(hipStreamSynchronize(t->stream));
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_film_device_ptr(dcrt_tracer* t, void** out)
{
    TRACER_GUARD(t);
    if (!out) return DCRT_E_INVALID_ARG;
    *out = t->film.accum;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_sample_device_ptrs(dcrt_tracer* t, void** pos, void** val)
{
    TRACER_GUARD(t);
    if (!pos || !val) return DCRT_E_INVALID_ARG;
    if (!t->film.sampleValue) { SetLastError("no frame parameters: the sample textures are not allocated"); return DCRT_E_INVALID_ARG; }
    const size_t o = (size_t)t->filmW * t->filmH * t->lastSlot;   // the last image's slot
    *pos = (void*)(t->film.samplePosition + o);
    *val = (void*)(t->film.sampleValue + o);
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_set_row_cost_probe(dcrt_tracer* t, int enable)
{
    TRACER_GUARD(t);
    if (enable && t->mode != 0) { SetLastError("the row-cost probe counts the wavefront's MATERIAL passes"); return DCRT_E_INVALID_ARG; }
    return t->SetRowProbe(enable != 0);
}

DCRT_API int dcrt_tracer_read_row_cost(dcrt_tracer* t, uint32_t* out_rows)
{
    TRACER_GUARD(t);
    if (!out_rows) return DCRT_E_INVALID_ARG;
    if (!t->rowProbe || !t->dRowRays) { SetLastError("the row-cost probe is off"); return DCRT_E_INVALID_ARG; }
    HIPCHECK(hipMemcpyAsync(out_rows, t->dRowRays, (size_t)t->filmH * 4, hipMemcpyDeviceToHost, t->stream));
    HIPCHECK(hipStreamSynchronize(t->stream));
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_copy_film_device(dcrt_tracer* t, void* d_dst)
{
    TRACER_GUARD(t);
    if (!d_dst || !t->film.accum) return DCRT_E_INVALID_ARG;
    HIPCHECK(hipMemcpyAsync(d_dst, t->film.accum, (size_t)t->filmW * t->filmH * sizeof(float4), hipMemcpyDeviceToDevice,
                            t->stream));
    HIPCHECK(hipStreamSynchronize(t->stream));
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_add_film_device(dcrt_tracer* t, const void* d_src)
{
    TRACER_GUARD(t);
    if (!d_src || !t->film.accum) return DCRT_E_INVALID_ARG;
    if (t->firefly) { SetLastError("add_film_device: firefly re-weighting is on, and the film would hold more than the cascades"); return DCRT_E_INVALID_ARG; }
    return t->AddFilm(t->film.accum, d_src);
}

// ---- film noise estimate ----------------------------------------------------------------------
DCRT_API int dcrt_tracer_set_convergence(dcrt_tracer* t, int enable)
{
    TRACER_GUARD(t);
    return t->SetConvergence(enable != 0);
}

DCRT_API int dcrt_tracer_half_film_device_ptr(dcrt_tracer* t, void** out)
{
    TRACER_GUARD(t);
    if (!out) return DCRT_E_INVALID_ARG;
    CHECKED(t->NeedHalfFilm());
    *out = t->halfFilm;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_read_half_film(dcrt_tracer* t, float* out)
{
    TRACER_GUARD(t);
    if (!out) return DCRT_E_INVALID_ARG;
    CHECKED(t->NeedHalfFilm());
    return t->ReadImage(t->halfFilm, out);
}

DCRT_API int dcrt_tracer_add_half_film_device(dcrt_tracer* t, const void* d_src)
{
    TRACER_GUARD(t);
    if (!d_src) return DCRT_E_INVALID_ARG;
    CHECKED(t->NeedHalfFilm());
    return t->AddFilm(t->halfFilm, d_src);
}

DCRT_API int dcrt_tracer_film_image_count(dcrt_tracer* t, uint32_t* out)
{
    TRACER_GUARD(t);
    if (!out) return DCRT_E_INVALID_ARG;
    *out = t->filmImages;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_film_pass_timing(dcrt_tracer* t, uint64_t* out_launches, double* out_ms)
{
    TRACER_GUARD(t);
    if (!out_launches || !out_ms) return DCRT_E_INVALID_ARG;
    HIPCHECK(hipStreamSynchronize(t->stream));
    CHECKED(t->CollectTimes());
    *out_launches = t->kindLaunches[dcrt_tracer::kTimedFilm];
    *out_ms = t->kindMs[dcrt_tracer::kTimedFilm];
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_noise(dcrt_tracer* t, float threshold, dcrt_noise_stats* out)
{
    TRACER_GUARD(t);
    return t->NoiseOwn(threshold, out);
}

DCRT_API int dcrt_tracer_noise_device(dcrt_tracer* t, uint32_t width, uint32_t height, const void* d_film, const void* d_half,
                                      float threshold, void* d_pixel_map, void* d_tile_map, dcrt_noise_stats* out)
{
    TRACER_GUARD(t);
    return t->noiseEstimator.Run(t->stream, width, height, (const float4*)d_film, (const float4*)d_half, threshold, (float*)d_pixel_map, (float*)d_tile_map, out);
}

DCRT_API int dcrt_tracer_noise_map_device_ptrs(dcrt_tracer* t, void** out_pixel, void** out_tile)
{
    TRACER_GUARD(t);
    if (!out_pixel || !out_tile) return DCRT_E_INVALID_ARG;
    if (!t->hasNoiseMaps) { SetLastError("no noise maps at this resolution (dcrt_tracer_noise)"); return DCRT_E_INVALID_ARG; }
    *out_pixel = t->noisePixelMap;
    *out_tile = t->noiseTileMap;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_read_noise_maps(dcrt_tracer* t, float* out_pixel, float* out_tile)
{
    TRACER_GUARD(t);
    if (!out_pixel && !out_tile) return DCRT_E_INVALID_ARG;
    if (!t->hasNoiseMaps) { SetLastError("no noise maps at this resolution (dcrt_tracer_noise)"); return DCRT_E_INVALID_ARG; }
    const uint32_t T = (uint32_t)kNoiseTile;
    const size_t tiles = (size_t)((t->filmW + T - 1) / T) * ((t->filmH + T - 1) / T);
    if (out_pixel)
        HIPCHECK(hipMemcpyAsync(out_pixel, t->noisePixelMap, (size_t)t->filmW * t->filmH * sizeof(float), hipMemcpyDeviceToHost, t->stream));
    if (out_tile) HIPCHECK(hipMemcpyAsync(out_tile, t->noiseTileMap, tiles * sizeof(float), hipMemcpyDeviceToHost, t->stream));
    HIPCHECK(hipStreamSynchronize(t->stream));
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_render_converged(dcrt_tracer* t, uint32_t first_seed, const dcrt_converge_params* p,
                                          const dcrt_filter_params* f, dcrt_noise_stats* out_stats, int* out_converged)
{
    TRACER_GUARD(t);
    if (!p || !f || !out_stats || !out_converged) return DCRT_E_INVALID_ARG;
    return t->RenderConverged(first_seed, *p, *f, out_stats, out_converged);
}

// ---- adaptive sampling ------------------------------------------------------------------------
DCRT_API int dcrt_tracer_set_adaptive(dcrt_tracer* t, int enable)
{
    TRACER_GUARD(t);
    return t->SetAdaptive(enable != 0);
}

DCRT_API int dcrt_tracer_set_sample_blocks(dcrt_tracer* t, const uint32_t* blocks, uint32_t count)
{
    TRACER_GUARD(t);
    return t->SetSampleBlocks(blocks, count);
}

DCRT_API int dcrt_tracer_get_sample_blocks(dcrt_tracer* t, uint32_t* out, uint32_t capacity, uint32_t* out_count)
{
    TRACER_GUARD(t);
    return t->GetSampleBlocks(out, capacity, out_count);
}

DCRT_API int dcrt_tracer_update_sample_blocks(dcrt_tracer* t, float threshold, uint32_t margin, uint32_t* out_active)
{
    TRACER_GUARD(t);
    return t->UpdateSampleBlocks(threshold, margin, out_active);
}

DCRT_API int dcrt_tracer_sample_blocks_device(dcrt_tracer* t, uint32_t width, uint32_t height, const void* d_film, const void* d_half,
                                              float threshold, uint32_t margin, void* d_flags, void* d_list, uint32_t* out_count)
{
    TRACER_GUARD(t);
    return t->blockSampler.Run(t->stream, t->extTiming, width, height, (const float4*)d_film, (const float4*)d_half, threshold, margin, (uint32_t*)d_flags,
                           (uint32_t*)d_list, out_count, nullptr);
}

DCRT_API int dcrt_tracer_adaptive_timings(dcrt_tracer* t, float* out_mask_ms, float* out_compact_ms, float* out_fill_ms)
{
    TRACER_GUARD(t);
    if (!out_mask_ms || !out_compact_ms || !out_fill_ms) return DCRT_E_INVALID_ARG;
    HIPCHECK(hipStreamSynchronize(t->stream));
    return t->blockSampler.Timings(out_mask_ms, out_compact_ms, out_fill_ms);
}

DCRT_API int dcrt_tracer_render_adaptive(dcrt_tracer* t, uint32_t first_seed, const dcrt_converge_params* p, uint32_t margin,
                                         const dcrt_filter_params* f, dcrt_noise_stats* out_stats, int* out_converged,
                                         dcrt_adaptive_report* out_report)
{
    TRACER_GUARD(t);
    if (!p || !f || !out_stats || !out_converged) return DCRT_E_INVALID_ARG;
    const dcrt_tracer::AdaptiveCall call{ margin, out_report };
    return t->RenderConverged(first_seed, *p, *f, out_stats, out_converged, &call);
}

DCRT_API int dcrt_tracer_counters(dcrt_tracer* t, dcrt_ray_stats* out)
{
    TRACER_GUARD(t);
    if (!out) return DCRT_E_INVALID_ARG;
    Globals g;
    HIPCHECK(hipMemcpyAsync(&g, t->dGlobals, sizeof(Globals), hipMemcpyDeviceToHost, t->stream));
    HIPCHECK(hipStreamSynchronize(t->stream));
    out->extension_rays = g.extRays;
    out->shadow_rays = g.shadowRays;
    // every rendered pixel (film rows of this tracer, halo included) starts one path per image
    // (less the pixels of the blocks an adaptive block list left out)
    out->new_paths = t->imagesCompleted * (uint64_t)t->rowCount * t->filmW - t->pathsSkipped;
    out->iterations = g.iterations;
    out->images_completed = t->imagesCompleted;
    out->early_finished = g.earlyFinished;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_set_instrumentation(dcrt_tracer* t, int counters, int ext_timing)
{
    TRACER_GUARD(t);
    if ((counters != 0) != t->instrCounters) t->InvalidateGraph();
    t->instrCounters = counters != 0;
    t->extTiming = ext_timing != 0;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_get_info(dcrt_tracer* t, dcrt_tracer_info* out)
{
    TRACER_GUARD(t);
    if (!out) return DCRT_E_INVALID_ARG;
    const CastPlan& plan = t->plan;
    const CastLaunch shipped = plan.Launch(false, false);
    out->path_pool_size = t->poolSize;
    out->scene_in_lds = t->hasScene && plan.allCached ? 1u : 0u;
    out->cached_nodes = t->hasScene ? plan.scene.cachedNodes : 0u;
    out->cached_triangles = t->hasScene ? plan.scene.cachedTris : 0u;
    out->cast_block = plan.block;
    out->traversal_stack = t->hasScene ? plan.scene.stackSize : 0u;
    out->material_generic = caps_any_scene(t->material.caps) ? 1u : 0u;
    out->pair_traversal = t->hasScene && plan.pair ? 1u : 0u;
    out->control_grid = t->controlGrid;
    out->material_grid = t->materialGrid;
    out->cast_grid = shipped.resident;
    out->material_lds = t->material.lds.shading;
    out->cast_identity = plan.ident ? (plan.flat ? 2u : 1u) : 0u;
    out->stack_lds_rows = t->hasScene ? shipped.scene.stackRows : 0u;
    out->ring_rows = t->hasScene ? plan.ringRows : 0u;
    out->cast_waves_per_cu = plan.perCU * (plan.block / 64u);
    const bool cells = t->hasScene && shipped.scene.shadowRes != 0u;   // (the flat scene's, while a table stands)
    out->shadow_cells = cells ? shipped.scene.shadowRes : 0u;
    out->shadow_cell_max_leaves = cells ? t->cells.maxLeaves : 0u;
    out->shadow_cell_mean_leaves = cells ? t->cells.meanLeaves : 0.0f;
    out->shadow_inline = t->hasScene && t->FusedShadow() ? 1u : 0u;
    out->shading_tables = t->hasScene ? t->material.tables : 0u;
    out->dielectric_row_bytes = t->hasScene && (t->material.tables & kTableDielRows) ? diel_rows_bytes((uint32_t)t->hostMaterials.size()) : 0u;
    out->dielectric_row_lds = t->hasScene ? t->material.lds.rows : 0u;
    out->frame_table_bytes = t->hasScene ? t->material.lds.frames : 0u;
    out->early_finish = t->hasScene ? t->material.EarlyFinish(t->rowProbe, (t->frame.features & DCRT_FEATURE_ALLOW_ANYHIT) != 0) : 0u;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_debug_ring_spills(dcrt_tracer* t, uint64_t* out)
{
    TRACER_GUARD(t);
    if (!out) return DCRT_E_INVALID_ARG;
    *out = 0;
    const CastLaunch shipped = t->plan.Launch(false, false);
    if (!t->hasScene || !shipped.scene.spill) return DCRT_OK;   // (the ring cast's scene alone has spill columns)
    const size_t n = (size_t)shipped.resident * t->plan.block * shipped.scene.stackSize;
    std::vector<uint32_t> h(n);
    HIPCHECK(hipStreamSynchronize(t->stream));
    HIPCHECK(hipMemcpy(h.data(), shipped.scene.spill, n * 4, hipMemcpyDeviceToHost));
    for (const uint32_t w : h) *out += w != 0u;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_traversal_stats(dcrt_tracer* t, dcrt_traversal_stats* out)
{
    TRACER_GUARD(t);
    if (!out) return DCRT_E_INVALID_ARG;
    unsigned long long v[8];
    HIPCHECK(hipMemcpyAsync(v, t->dInstr, sizeof(v), hipMemcpyDeviceToHost, t->stream));
    HIPCHECK(hipStreamSynchronize(t->stream));
    CHECKED(t->CollectTimes());
    out->ext_node_visits = v[0]; out->ext_triangle_tests = v[1]; out->ext_blas_entries = v[2];
    out->shadow_node_visits = v[3]; out->shadow_triangle_tests = v[4]; out->shadow_blas_entries = v[5];
    out->ext_launches = t->kindLaunches[dcrt_tracer::kTimedCast];
    out->ext_kernel_ms = t->kindMs[dcrt_tracer::kTimedCast];
    out->ext_max_node_visits = v[6]; out->shadow_max_node_visits = v[7];
    out->material_launches = t->kindLaunches[dcrt_tracer::kTimedMaterial];
    out->material_kernel_ms = t->kindMs[dcrt_tracer::kTimedMaterial];
    out->control_launches = t->kindLaunches[dcrt_tracer::kTimedControl];
    out->control_kernel_ms = t->kindMs[dcrt_tracer::kTimedControl];
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_reset_stats(dcrt_tracer* t)
{
    TRACER_GUARD(t);
    HIPCHECK(hipStreamSynchronize(t->stream));
    HIPCHECK(hipMemsetAsync(t->dInstr, 0, 8 * sizeof(unsigned long long), t->stream));
    Globals g;
    HIPCHECK(hipMemcpyAsync(&g, t->dGlobals, sizeof(Globals), hipMemcpyDeviceToHost, t->stream));
    HIPCHECK(hipStreamSynchronize(t->stream));
    g.extRays = g.shadowRays = g.iterations = g.earlyFinished = 0;
    t->imagesCompleted = 0;
    t->pathsSkipped = 0;
    HIPCHECK(hipMemcpyAsync(t->dGlobals, &g, sizeof(Globals), hipMemcpyHostToDevice, t->stream));
    HIPCHECK(hipStreamSynchronize(t->stream));
    t->eventsUsed = 0;
    for (int k = 0; k < dcrt_tracer::kTimedKinds; ++k) {
        t->kindMs[k] = 0.0;
        t->kindLaunches[k] = 0;
    }
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_synchronize(dcrt_tracer* t)
{
    TRACER_GUARD(t);
    HIPCHECK(hipStreamSynchronize(t->stream));
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_get_luts(dcrt_tracer* t, dcrt_bxdf_luts* out)
{
    TRACER_GUARD(t);
    if (!out) return DCRT_E_INVALID_ARG;
    HIPCHECK(hipMemcpyAsync(out, t->dLuts, sizeof(dcrt_bxdf_luts), hipMemcpyDeviceToHost, t->stream));
    HIPCHECK(hipStreamSynchronize(t->stream));
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_set_luts(dcrt_tracer* t, const dcrt_bxdf_luts* luts)
{
    TRACER_GUARD(t);
    if (!luts) return DCRT_E_INVALID_ARG;
    HIPCHECK(hipMemcpyAsync(t->dLuts, luts, sizeof(dcrt_bxdf_luts), hipMemcpyHostToDevice, t->stream));
    HIPCHECK(hipStreamSynchronize(t->stream));
    // (the materials' rows of the dielectric LUT hold the old texels: the same buffer refilled, nothing re-derived)
    if (t->hasScene && (t->material.tables & kTableDielRows)) {
        CHECKED(t->BuildDielRows());
        HIPCHECK(hipStreamSynchronize(t->stream));
    }
    return DCRT_OK;
}

static int TraceBatch(dcrt_tracer* t, const dcrt_ray* d_rays, uint32_t n, dcrt_ray_hit* d_hits, uint32_t* d_occ, bool any, uint32_t features)
{
    if (!t->hasScene) { SetLastError("no scene uploaded"); return DCRT_E_NO_SCENE; }
    // (the plain scene with the whole stack, on the shipped kernel's grid)
    const CastPlan& plan = t->plan;
    const uint32_t grid = std::min<uint32_t>((n + plan.block - 1) / plan.block, plan.resident[0][0]);
    if (n == 0) return DCRT_OK;
    unsigned long long* instr = t->instrCounters ? t->dInstr : nullptr;
    auto kernel = any ? (instr ? batch_trace_kernel<true, true> : batch_trace_kernel<true, false>)
                      : (instr ? batch_trace_kernel<false, true> : batch_trace_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(plan.block), plan.ldsWholeStack, t->stream, plan.scene, d_rays, n, features, d_hits, d_occ, instr);
    HIPCHECK(hipGetLastError());
    return DCRT_OK;
}

// trace_rays / occluded: the caller's rays through TraceBatch, to its hit records or its occlusion words
static int TraceHostRays(dcrt_tracer* t, const dcrt_ray* rays, uint32_t n, void* out, bool any, uint32_t features)
{
    TRACER_GUARD(t);
    if ((!rays || !out) && n) return DCRT_E_INVALID_ARG;
    if (!t->hasScene) { SetLastError("no scene uploaded"); return DCRT_E_NO_SCENE; }
    DeviceGroup scratch;
    HostArray a[2] = {{rays, nullptr, sizeof(dcrt_ray)}, {nullptr, out, any ? sizeof(uint32_t) : sizeof(dcrt_ray_hit)}};
    return RoundTrip(t, scratch, n, a, [&] {
        return TraceBatch(t, (const dcrt_ray*)a[0].device, n, any ? nullptr : (dcrt_ray_hit*)a[1].device, any ? (uint32_t*)a[1].device : nullptr, any, features);
    });
}

DCRT_API int dcrt_tracer_trace_rays(dcrt_tracer* t, const dcrt_ray* rays, uint32_t n, dcrt_ray_hit* out, uint32_t features)
{
    return TraceHostRays(t, rays, n, out, false, features);
}

DCRT_API int dcrt_tracer_occluded(dcrt_tracer* t, const dcrt_ray* rays, uint32_t n, uint32_t* out, uint32_t features)
{
    return TraceHostRays(t, rays, n, out, true, features);
}

DCRT_API int dcrt_tracer_cast_rays(dcrt_tracer* t, const dcrt_ray* rays, const uint32_t* kinds, const float* opacity_samples, uint32_t n,
                                   uint32_t features, dcrt_ray_hit* out_hits, uint32_t* out_occluded, uint32_t* out_variant)
{
    TRACER_GUARD(t);
    const bool opacity = (features & DCRT_FEATURE_ALLOW_ANYHIT) != 0;
    if (!out_variant || ((!rays || !kinds || !out_hits || !out_occluded || (opacity && !opacity_samples)) && n)) return DCRT_E_INVALID_ARG;
    if (!t->hasScene) { SetLastError("no scene uploaded"); return DCRT_E_NO_SCENE; }
    // the launch a render of this scene with these features would make, and the ray-batch twin of its kernel
    // (the CELLS cast's shadow section has its own entry: its twin is the plain FLAT kernel's)
    const CastLaunch cast = t->plan.Launch(false, opacity);
    CastVariant want = cast.asked;
    want.cells = false;
    const CastRow* row = CastTableRow(want);
    if (!row || !row->rays) { SetLastError("no ray-batch kernel for the scene's cast variant"); return DCRT_E_INVALID_ARG; }
    const CastVariant& v = row->v;
    *out_variant = (v.opacity ? DCRT_CAST_VARIANT_OPACITY : 0u) | (v.allCached ? DCRT_CAST_VARIANT_ALL_CACHED : 0u) |
                   (v.pair ? DCRT_CAST_VARIANT_PAIR : 0u) | (v.ident ? DCRT_CAST_VARIANT_IDENT : 0u) |
                   (v.ring ? DCRT_CAST_VARIANT_RING : 0u) | (v.flat ? DCRT_CAST_VARIANT_FLAT : 0u);
    DeviceGroup scratch;
    HostArray a[5] = {{rays, nullptr, sizeof(dcrt_ray)}, {kinds, nullptr, 4}, {opacity ? opacity_samples : nullptr, nullptr, 4},
                      {nullptr, out_hits, sizeof(dcrt_ray_hit)}, {nullptr, out_occluded, 4}};
    return RoundTrip(t, scratch, n, a, [&] {
        // (the refill / park thresholds of a frame: BeginImage)
        const uint32_t refill = t->knobs.tuneOverride || t->plan.allCached ? t->knobs.refillLanes : DCRT_REFILL_GLOBAL;
        const uint32_t block = t->plan.block, grid = std::min<uint32_t>((n + block - 1) / block, cast.resident);
        hipLaunchKernelGGL(row->rays, dim3(grid), dim3(block), cast.lds, t->stream, cast.scene, (const dcrt_ray*)a[0].device, (const uint32_t*)a[1].device,
                           (const float*)a[2].device, n, features, refill, t->knobs.parkLanes, (dcrt_ray_hit*)a[3].device, (uint32_t*)a[4].device);
    });
}

DCRT_API int dcrt_tracer_trace_occlusion_cells(dcrt_tracer* t, const dcrt_ray* rays, uint32_t n, uint32_t* out, uint32_t features)
{
    TRACER_GUARD(t);
    if ((!rays || !out) && n) return DCRT_E_INVALID_ARG;
    const CastLaunch shipped = t->plan.Launch(false, false);
    if (!t->hasScene || shipped.scene.shadowRes == 0u) {
        SetLastError("the uploaded scene has no direction-cell table" + (t->cells.reason.empty() ? std::string() : ": " + t->cells.reason));
        return DCRT_E_NO_SCENE;
    }
    DeviceGroup scratch;
    HostArray a[2] = {{rays, nullptr, sizeof(dcrt_ray)}, {nullptr, out, 4}};
    return RoundTrip(t, scratch, n, a, [&] {
        const uint32_t block = t->plan.block, grid = std::min<uint32_t>((n + block - 1) / block, shipped.resident);
        hipLaunchKernelGGL(cells_occlusion_kernel, dim3(grid), dim3(block), shipped.lds, t->stream, shipped.scene, (const dcrt_ray*)a[0].device, n,
                           features, (uint32_t*)a[1].device);
    });
}

DCRT_API int dcrt_tracer_trace_rays_device(dcrt_tracer* t, const void* d_rays, uint32_t n, void* d_hits, uint32_t features)
{
    TRACER_GUARD(t);
    if ((!d_rays || !d_hits) && n) return DCRT_E_INVALID_ARG;
    return TraceBatch(t, (const dcrt_ray*)d_rays, n, (dcrt_ray_hit*)d_hits, nullptr, false, features);
}

DCRT_API int dcrt_tracer_prepare_images(dcrt_tracer* t, uint32_t image_count)
{
    TRACER_GUARD(t);
    return t->PrepareImages(image_count);
}

DCRT_API int dcrt_tracer_set_image_batch(dcrt_tracer* t, uint32_t images)
{
    TRACER_GUARD(t);
    if (images > kMaxImageBatch) { SetLastError("image batch too large (max 256)"); return DCRT_E_INVALID_ARG; }
    t->batchImages = images;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_set_mode(dcrt_tracer* t, int mode)
{
    TRACER_GUARD(t);
    if (mode != 0 && mode != 1) return DCRT_E_INVALID_ARG;
    t->mode = mode;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_set_output(dcrt_tracer* t, const dcrt_output_params* p)
{
    TRACER_GUARD(t);
    if (!p) return DCRT_E_INVALID_ARG;
    if (p->output_type > DCRT_OUTPUT_ITERATION_COUNT) { SetLastError("unknown output type"); return DCRT_E_INVALID_ARG; }
    if (p->output_type == DCRT_OUTPUT_ITERATION_COUNT && (p->iteration_threshold < 1u || p->iteration_threshold > 10000u)) {
        SetLastError("iteration threshold: 1..10000");
        return DCRT_E_INVALID_ARG;
    }
    if (p->output_type != t->output.output_type || p->iteration_threshold != t->output.iteration_threshold) {
        t->filmClearTrigger = true;
        t->newImage = true;
        t->imageComplete = false;
    }
    t->output = *p;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_get_output(dcrt_tracer* t, dcrt_output_params* out)
{
    TRACER_GUARD(t);
    if (!out) return DCRT_E_INVALID_ARG;
    *out = t->output;
    return DCRT_OK;
}

// SumLuminance + post-processing of `image` (the film, or the denoised image: W x H of the film)
static int ResolveFrom(dcrt_tracer* t, const float4* image, const dcrt_postfx_params* prm, uint8_t* out, float* outSumLogLum)
{
    const uint32_t W = t->filmW, H = t->filmH;
    float hth[255];
    dcrt_srgb_encode_thresholds(hth);
    DeviceGroup scratch;
    float* dth = nullptr;
    CHECKED(scratch.Alloc(&dth, 255));
    HIPCHECK(hipMemcpyAsync(dth, hth, sizeof(hth), hipMemcpyHostToDevice, t->stream));
    // SumLuminance: REDUCE_TO_1D then REDUCE_TO_SINGLE until one value (SceneLuminance.cpp:110-190)
    const uint32_t bx = (((W + 7) / 8) + 1) / 2, by = (((H + 7) / 8) + 1) / 2;
    float *la = nullptr, *lb = nullptr;
    CHECKED(scratch.Alloc(&la, (size_t)bx * by + 1));
    CHECKED(scratch.Alloc(&lb, (size_t)bx * by + 1));
    hipLaunchKernelGGL(luminance_1d_kernel, dim3(bx, by), dim3(64), 0, t->stream, image, W, H, bx, by, la);
    uint32_t count = bx * by;
    while (count != 1) {
        const uint32_t groups = (count + 127) / 128;
        hipLaunchKernelGGL(luminance_single_kernel, dim3(groups), dim3(128), 0, t->stream, (const float*)la, count, lb);
        std::swap(la, lb);
        count = groups;
    }
    uchar4* dout = nullptr;
    CHECKED(scratch.Alloc(&dout, (size_t)W * H));
    const uint32_t grid = std::max<uint32_t>(1u, std::min<uint32_t>((W * H + 255) / 256, kMaxPersistentBlocks));
    hipLaunchKernelGGL(postfx_kernel, dim3(grid), dim3(256), 0, t->stream, image, W, H, prm->enabled,
                       prm->auto_exposure, prm->ev100, prm->luminance_white * prm->luminance_white, (const float*)la,
                       (const float*)dth, dout);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(out, dout, (size_t)W * H * 4, hipMemcpyDeviceToHost, t->stream));
    if (outSumLogLum) HIPCHECK(hipMemcpyAsync(outSumLogLum, la, sizeof(float), hipMemcpyDeviceToHost, t->stream));
    HIPCHECK(hipStreamSynchronize(t->stream));
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_resolve_image(dcrt_tracer* t, const dcrt_postfx_params* prm, uint8_t* out, float* outSumLogLum)
{
    TRACER_GUARD(t);
    if (!prm || !out || !t->film.accum) return DCRT_E_INVALID_ARG;
    return ResolveFrom(t, (const float4*)t->film.accum, prm, out, outSumLogLum);
}

// ---- firefly re-weighting -----------------------------------------------------------------
DCRT_API int dcrt_firefly_default_params(dcrt_firefly_params* out)
{
    if (!out) return DCRT_E_INVALID_ARG;
    out->cascades = 6u;
    out->start = 1.0f;
    out->base = 8.0f;
    out->min_support = 3.0f;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_set_firefly(dcrt_tracer* t, const dcrt_firefly_params* p)
{
    TRACER_GUARD(t);
    return t->SetFirefly(p);
}

DCRT_API int dcrt_tracer_get_firefly(dcrt_tracer* t, int* out_enabled, dcrt_firefly_params* out)
{
    TRACER_GUARD(t);
    if (!out_enabled) return DCRT_E_INVALID_ARG;
    *out_enabled = t->firefly ? 1 : 0;
    if (out && t->firefly) *out = t->fireflyParams;
    return DCRT_OK;
}

static int NeedFirefly(const dcrt_tracer* t)
{
    if (!t->firefly) { SetLastError("firefly re-weighting is off (dcrt_tracer_set_firefly)"); return DCRT_E_INVALID_ARG; }
    return DCRT_OK;
}
static int NeedReweighted(const dcrt_tracer* t)
{
    if (!t->hasReweighted) { SetLastError("no re-weighted image (dcrt_tracer_firefly_resolve)"); return DCRT_E_INVALID_ARG; }
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_firefly_resolve(dcrt_tracer* t)
{
    TRACER_GUARD(t);
    CHECKED(NeedFirefly(t));
    t->hasReweighted = false;
    CHECKED(t->fireflyFilter.Resolve(t->stream, t->extTiming, t->fireflyConsts, t->filmW, t->filmH, t->filmImages, t->film.accum, t->cascades,
                                     t->reweighted));
    t->hasReweighted = true;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_read_firefly(dcrt_tracer* t, float* out)
{
    TRACER_GUARD(t);
    if (!out) return DCRT_E_INVALID_ARG;
    CHECKED(NeedReweighted(t));
    return t->ReadImage(t->reweighted, out);
}

DCRT_API int dcrt_tracer_firefly_device_ptr(dcrt_tracer* t, void** out)
{
    TRACER_GUARD(t);
    if (!out) return DCRT_E_INVALID_ARG;
    CHECKED(NeedReweighted(t));
    *out = t->reweighted;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_resolve_firefly(dcrt_tracer* t, const dcrt_postfx_params* prm, uint8_t* out, float* outSumLogLum)
{
    TRACER_GUARD(t);
    if (!prm || !out) return DCRT_E_INVALID_ARG;
    CHECKED(NeedReweighted(t));
    return ResolveFrom(t, (const float4*)t->reweighted, prm, out, outSumLogLum);
}

DCRT_API int dcrt_tracer_read_cascades(dcrt_tracer* t, float* out)
{
    TRACER_GUARD(t);
    if (!out) return DCRT_E_INVALID_ARG;
    CHECKED(NeedFirefly(t));
    const size_t n = (size_t)t->filmW * t->filmH;
    for (uint32_t j = 0; j < t->fireflyParams.cascades; ++j)
        HIPCHECK(hipMemcpyAsync(out + j * n * 4, t->cascades.film[j], n * sizeof(float4), hipMemcpyDeviceToHost, t->stream));
    HIPCHECK(hipStreamSynchronize(t->stream));
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_cascade_device_ptrs(dcrt_tracer* t, void** out, uint32_t capacity, uint32_t* out_count)
{
    TRACER_GUARD(t);
    if (!out || !out_count) return DCRT_E_INVALID_ARG;
    CHECKED(NeedFirefly(t));
    *out_count = t->fireflyParams.cascades;
    if (capacity < t->fireflyParams.cascades) { SetLastError("cascade_device_ptrs: room for fewer than K pointers"); return DCRT_E_INVALID_ARG; }
    for (uint32_t j = 0; j < t->fireflyParams.cascades; ++j) out[j] = t->cascades.film[j];
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_firefly_resolve_device(dcrt_tracer* t, const dcrt_firefly_params* p, uint32_t width, uint32_t height,
                                                uint32_t image_count, const void* d_film, const void* const* d_cascades, void* d_out)
{
    TRACER_GUARD(t);
    if (!p || !d_cascades) return DCRT_E_INVALID_ARG;
    FireflyConsts k{};
    CHECKED(FireflyFilter::MakeConsts(*p, &k));
    CascadeFilms cas{};
    for (uint32_t j = 0; j < p->cascades; ++j) cas.film[j] = (float4*)const_cast<void*>(d_cascades[j]);
    return t->fireflyFilter.Resolve(t->stream, t->extTiming, k, width, height, image_count, (const float4*)d_film, cas, (float4*)d_out);
}

DCRT_API int dcrt_tracer_firefly_timings(dcrt_tracer* t, float* out_cascade_ms, float* out_resolve_ms)
{
    TRACER_GUARD(t);
    if (!out_cascade_ms || !out_resolve_ms) return DCRT_E_INVALID_ARG;
    HIPCHECK(hipStreamSynchronize(t->stream));
    return t->fireflyFilter.Timings(out_cascade_ms, out_resolve_ms);
}

// ---- film denoiser ------------------------------------------------------------------------
DCRT_API int dcrt_denoise_default_params(dcrt_denoise_params* out)
{
    if (!out) return DCRT_E_INVALID_ARG;
    out->iterations = 5u;
    out->sigma_luminance = 4.0f;
    out->sigma_normal = 0.2f;
    out->sigma_albedo = 0.1f;
    out->demodulate = 1u;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_render_guides(dcrt_tracer* t, uint32_t first_seed, uint32_t image_count)
{
    TRACER_GUARD(t);
    return t->RenderGuides(first_seed, image_count);
}

DCRT_API int dcrt_tracer_guide_device_ptrs(dcrt_tracer* t, void** out_normal, void** out_albedo)
{
    TRACER_GUARD(t);
    if (!out_normal || !out_albedo) return DCRT_E_INVALID_ARG;
    if (!t->guidesRendered) { SetLastError("no guides rendered at this resolution"); return DCRT_E_INVALID_ARG; }
    *out_normal = t->guideNormal;
    *out_albedo = t->guideAlbedo;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_read_guides(dcrt_tracer* t, float* out_normal, float* out_albedo)
{
    TRACER_GUARD(t);
    if (!out_normal || !out_albedo) return DCRT_E_INVALID_ARG;
    if (!t->guidesRendered) { SetLastError("no guides rendered at this resolution"); return DCRT_E_INVALID_ARG; }
    const size_t bytes = (size_t)t->filmW * t->filmH * sizeof(float4);
    HIPCHECK(hipMemcpyAsync(out_normal, t->guideNormal, bytes, hipMemcpyDeviceToHost, t->stream));
    HIPCHECK(hipMemcpyAsync(out_albedo, t->guideAlbedo, bytes, hipMemcpyDeviceToHost, t->stream));
    HIPCHECK(hipStreamSynchronize(t->stream));
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_denoise(dcrt_tracer* t, const dcrt_denoise_params* p)
{
    TRACER_GUARD(t);
    if (!p) return DCRT_E_INVALID_ARG;
    if (t->partition.world_size > 1 || !t->bands.empty()) {
        SetLastError("denoise: a banded or partitioned film lacks its neighbours' rows; reduce the films and guides and "
                     "use dcrt_tracer_denoise_device on the sums");
        return DCRT_E_INVALID_ARG;
    }
    if (!t->guidesRendered || !t->film.accum) {
        SetLastError("denoise: no guides rendered at this resolution (dcrt_tracer_render_guides)");
        return DCRT_E_INVALID_ARG;
    }
    CHECKED(t->denoiser.Run(t->stream, t->extTiming, *p, t->filmW, t->filmH, t->film.accum, t->guideNormal, t->guideAlbedo, t->denoised));
    t->hasDenoised = true;
    return DCRT_OK;
}

// ... with the re-weighted image of the last dcrt_tracer_firefly_resolve as the colour input
DCRT_API int dcrt_tracer_denoise_firefly(dcrt_tracer* t, const dcrt_denoise_params* p)
{
    TRACER_GUARD(t);
    if (!p) return DCRT_E_INVALID_ARG;
    if (!t->hasReweighted) { SetLastError("denoise_firefly: no re-weighted image (dcrt_tracer_firefly_resolve)"); return DCRT_E_INVALID_ARG; }
    if (!t->guidesRendered || !t->guideNormal) {
        SetLastError("denoise: no guides rendered at this resolution (dcrt_tracer_render_guides)");
        return DCRT_E_INVALID_ARG;
    }
    t->hasDenoised = false;
    CHECKED(t->denoiser.Run(t->stream, t->extTiming, *p, t->filmW, t->filmH, t->reweighted, t->guideNormal, t->guideAlbedo, t->denoised));
    t->hasDenoised = true;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_denoise_device(dcrt_tracer* t, const dcrt_denoise_params* p, uint32_t width, uint32_t height,
                                        const void* d_color, const void* d_normal, const void* d_albedo, void* d_out)
{
    TRACER_GUARD(t);
    if (!p) return DCRT_E_INVALID_ARG;
    return t->denoiser.Run(t->stream, t->extTiming, *p, width, height, (const float4*)d_color, (const float4*)d_normal, (const float4*)d_albedo, (float4*)d_out);
}

DCRT_API int dcrt_tracer_denoise_images(dcrt_tracer* t, const dcrt_denoise_params* p, uint32_t width, uint32_t height,
                                        const float* color, const float* normal, const float* albedo, float* out)
{
    TRACER_GUARD(t);
    if (!p || !color || !normal || !albedo || !out || width == 0 || height == 0 || width > 65535u || height > 65535u)
        return DCRT_E_INVALID_ARG;
    CHECKED(CheckDenoiseParams(*p));
    const size_t n = (size_t)width * height, bytes = n * sizeof(float4);
    DeviceGroup scratch;
    float4* d[4] = {};
    for (float4*& q : d) CHECKED(scratch.Alloc(&q, n));
    const float* src[3] = { color, normal, albedo };
    for (int i = 0; i < 3; ++i) HIPCHECK(hipMemcpyAsync(d[i], src[i], bytes, hipMemcpyHostToDevice, t->stream));
    CHECKED(t->denoiser.Run(t->stream, t->extTiming, *p, width, height, d[0], d[1], d[2], d[3]));
    HIPCHECK(hipMemcpyAsync(out, d[3], bytes, hipMemcpyDeviceToHost, t->stream));
    HIPCHECK(hipStreamSynchronize(t->stream));
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_read_denoised(dcrt_tracer* t, float* out)
{
    TRACER_GUARD(t);
    if (!out) return DCRT_E_INVALID_ARG;
    if (!t->hasDenoised) { SetLastError("no denoised image (dcrt_tracer_denoise)"); return DCRT_E_INVALID_ARG; }
    return t->ReadImage(t->denoised, out);
}

DCRT_API int dcrt_tracer_denoised_device_ptr(dcrt_tracer* t, void** out)
{
    TRACER_GUARD(t);
    if (!out) return DCRT_E_INVALID_ARG;
    if (!t->hasDenoised) { SetLastError("no denoised image (dcrt_tracer_denoise)"); return DCRT_E_INVALID_ARG; }
    *out = t->denoised;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_resolve_denoised(dcrt_tracer* t, const dcrt_postfx_params* prm, uint8_t* out, float* outSumLogLum)
{
    TRACER_GUARD(t);
    if (!prm || !out) return DCRT_E_INVALID_ARG;
    if (!t->hasDenoised) { SetLastError("no denoised image (dcrt_tracer_denoise)"); return DCRT_E_INVALID_ARG; }
    return ResolveFrom(t, (const float4*)t->denoised, prm, out, outSumLogLum);
}

DCRT_API int dcrt_tracer_denoise_timings(dcrt_tracer* t, float* out_ms, uint32_t capacity, uint32_t* out_count)
{
    TRACER_GUARD(t);
    if (!out_count || (capacity && !out_ms)) return DCRT_E_INVALID_ARG;
    return t->denoiser.Timings(out_ms, capacity, out_count);
}

DCRT_API int dcrt_device_math_eval(dcrt_tracer* t, int function, const float* x, uint32_t n, float* y)
{
    TRACER_GUARD(t);
    if ((!x || !y) && n) return DCRT_E_INVALID_ARG;
    DeviceGroup scratch;
    HostArray a[2] = {{x, nullptr, 4}, {nullptr, y, 4}};
    return RoundTrip(t, scratch, n, a, [&] {
        hipLaunchKernelGGL(math_eval_kernel, ItemGrid(n), dim3(256), 0, t->stream, function, (float*)a[0].device, n, (float*)a[1].device);
    });
}

// A DeviceScene with nothing but the tracer's current LUTs (the BSDF probe kernels read no more).
static DeviceScene LutOnlyScene(const dcrt_tracer* t)
{
    DeviceScene d{};
    d.lutBrdf = t->dLuts->brdf;
    d.lutBrdfAvg = t->dLuts->brdf_avg;
    d.lutBrdfDielectric = t->dLuts->brdf_dielectric;
    d.lutBrdfDielectricAvg = t->dLuts->brdf_dielectric_avg;
    d.lutBsdf = t->dLuts->bsdf;
    d.lutBsdfAvg = t->dLuts->bsdf_avg;
    return d;
}
// ... and, under DCRT_SHADING_TABLES' rows bit, the probe material's rows of the dielectric LUT (in
// `scratch`), so the probe kernels run the path MATERIAL takes for a material with that alpha and ior.
static int ProbeScene(dcrt_tracer* t, const dcrt_bsdf_probe_material& m, DeviceGroup& scratch, DeviceScene* out)
{
    *out = LutOnlyScene(t);
    if (!(ReadShadingKnobs().shadingTables & kTableDielRows)) return DCRT_OK;
    float* rows = nullptr;
    CHECKED(scratch.Alloc(&rows, kDielRowFloats));
    hipLaunchKernelGGL(probe_diel_rows_kernel, dim3(1), dim3(256), 0, t->stream, out->lutBrdfDielectric, out->lutBrdfDielectricAvg, rows,
                       m.alpha, m.ior[0]);
    HIPCHECK(hipGetLastError());
    out->dielRows = rows;
    out->shadingTables = kTableDielRows;
    return DCRT_OK;
}

DCRT_API int dcrt_device_bsdf_eval(dcrt_tracer* t, const dcrt_bsdf_probe_material* m, uint32_t features, const float* wi,
                                   const float* wo, uint32_t n, float* f, float* pdf)
{
    TRACER_GUARD(t);
    if (!m || ((!wi || !wo || !f || !pdf) && n)) return DCRT_E_INVALID_ARG;
    DeviceGroup scratch;
    DeviceScene ps;
    CHECKED(ProbeScene(t, *m, scratch, &ps));
    HostArray a[4] = {{wi, nullptr, 12}, {wo, nullptr, 12}, {nullptr, f, 12}, {nullptr, pdf, 4}};
    return RoundTrip(t, scratch, n, a, [&] {
        hipLaunchKernelGGL(bsdf_eval_kernel, ItemGrid(n), dim3(256), 0, t->stream, ps, *m, features, (const float*)a[0].device,
                           (const float*)a[1].device, n, (float*)a[2].device, (float*)a[3].device);
    });
}

// The frame and intersection probes' scene: plan.scene's global-memory arrays with the frame table or without,
// once the hit records' triangle and instance indices lie inside it
static int HitProbeScene(dcrt_tracer* t, const uint32_t* records, uint32_t n, int use_table, const char* probe, DeviceScene* out)
{
    if (!t->hasScene || (use_table && !t->dTriFrames)) { SetLastError("no scene uploaded, or no frame table for it"); return DCRT_E_NO_SCENE; }
    *out = t->plan.scene;
    for (uint32_t i = 0; i < n; ++i) {
        if ((records[4 * (size_t)i + 2] & 0x7FFFFFFFu) >= out->triangleCount || records[4 * (size_t)i + 3] >= out->instanceCount) {
            SetLastError(std::string(probe) + ": triangle or instance index out of range");
            return DCRT_E_INVALID_ARG;
        }
    }
    out->triFrames = use_table ? t->dTriFrames : nullptr;
    return DCRT_OK;
}

DCRT_API int dcrt_device_frame_probe(dcrt_tracer* t, const uint32_t* records, uint32_t n, int use_table, float* out)
{
    TRACER_GUARD(t);
    if ((!records || !out) && n) return DCRT_E_INVALID_ARG;
    DeviceScene sc;
    CHECKED(HitProbeScene(t, records, n, use_table, "frame probe", &sc));
    DeviceGroup scratch;
    HostArray a[2] = {{records, nullptr, 16}, {nullptr, out, 36}};
    return RoundTrip(t, scratch, n, a, [&] {
        hipLaunchKernelGGL(frame_probe_kernel, ItemGrid(n), dim3(256), 0, t->stream, sc, (const uint4*)a[0].device, n, (float*)a[1].device);
    });
}

// A mesh light (MESH_LIGHT without POINT or DIRECTIONAL) and its range: first triangle, triangle count, instance
static bool MeshLightRange(const dcrt_light& L, uint32_t w[3])
{
    if (!(L.flags & DCRT_LIGHT_FLAGS_MESH_LIGHT) || (L.flags & (DCRT_LIGHT_FLAGS_POINT_LIGHT | DCRT_LIGHT_FLAGS_DIRECTIONAL_LIGHT))) return false;
    std::memcpy(w, L.position_or_triangle_range, 3 * sizeof(uint32_t));
    return true;
}
// A mesh light's triangle range and instance lie inside the uploaded scene (the probes read them)
static bool LightInScene(const dcrt_light& L, const DeviceScene& sc)
{
    uint32_t w[3];
    if (!MeshLightRange(L, w)) return true;
    return w[1] != 0u && w[0] < sc.triangleCount && w[1] <= sc.triangleCount - w[0] && w[2] < sc.instanceCount;
}
// The light probes' kernels for the scene's MATERIAL variant: the cube sampled by its table, or the any-scene stack
static auto LightSampleProbe(const dcrt_tracer* t)
{
    if (t->material.caps == kCapAllLightTable) return light_sample_probe_kernel<kCapAllLightTable>;
    return t->material.caps == kCapAllEnvImportance ? light_sample_probe_kernel<kCapAllEnvImportance> : light_sample_probe_kernel<kCapAll>;
}
static auto LightEvalProbe(const dcrt_tracer* t)
{
    if (t->material.caps == kCapAllLightTable) return light_eval_probe_kernel<kCapAllLightTable>;
    return t->material.caps == kCapAllEnvImportance ? light_eval_probe_kernel<kCapAllEnvImportance> : light_eval_probe_kernel<kCapAll>;
}

DCRT_API int dcrt_device_camera_ray(dcrt_tracer* t, const float* film, const float* aperture, uint32_t n, float* origins, float* directions)
{
    TRACER_GUARD(t);
    if ((!film || !aperture || !origins || !directions) && n) return DCRT_E_INVALID_ARG;
    if (!t->hasFrame) { SetLastError("no frame parameters"); return DCRT_E_INVALID_ARG; }
    FrameConstants fc;
    std::memset(&fc, 0, sizeof(fc));
    FillCameraConstants(t->frame, &fc);
    DeviceGroup scratch;
    HostArray b[4] = {{film, nullptr, 8}, {aperture, nullptr, 12}, {nullptr, origins, 12}, {nullptr, directions, 12}};
    return RoundTrip(t, scratch, n, b, [&] {
        hipLaunchKernelGGL(camera_ray_probe_kernel, ItemGrid(n), dim3(256), 0, t->stream, fc, (const float*)b[0].device, (const float*)b[1].device, n,
                           (float*)b[2].device, (float*)b[3].device);
    });
}

DCRT_API int dcrt_device_intersection_probe(dcrt_tracer* t, const uint32_t* records, uint32_t n, int use_table, float* out_floats,
                                            uint32_t* out_words)
{
    TRACER_GUARD(t);
    if ((!records || !out_floats || !out_words) && n) return DCRT_E_INVALID_ARG;
    DeviceScene sc;
    CHECKED(HitProbeScene(t, records, n, use_table, "intersection probe", &sc));
    DeviceGroup scratch;
    HostArray b[3] = {{records, nullptr, 16}, {nullptr, out_floats, 64}, {nullptr, out_words, 12}};
    return RoundTrip(t, scratch, n, b, [&] {
        if (use_table) hipLaunchKernelGGL(intersection_probe_kernel<true>, ItemGrid(n), dim3(256), 0, t->stream, sc, (const uint4*)b[0].device, n, (float*)b[1].device, (uint32_t*)b[2].device);
        else hipLaunchKernelGGL(intersection_probe_kernel<false>, ItemGrid(n), dim3(256), 0, t->stream, sc, (const uint4*)b[0].device, n, (float*)b[1].device, (uint32_t*)b[2].device);
    });
}

// The light probes read the frame's light_count lights (CheckFrameLights holds it to the uploaded array)
static int ProbeLights(dcrt_tracer* t, uint32_t* lightCount)
{
    if (!t->hasScene) { SetLastError("no scene uploaded"); return DCRT_E_NO_SCENE; }
    if (!t->hasFrame) { SetLastError("no frame parameters"); return DCRT_E_INVALID_ARG; }
    *lightCount = t->frame.light_count;
    CHECKED(t->CheckFrameLights());   // (under the light table: exactly the lights it was built for)
    if (*lightCount == 0u || *lightCount > t->hostLights.size()) { SetLastError("light probe: the frame has no lights"); return DCRT_E_INVALID_ARG; }
    for (uint32_t i = 0; i < *lightCount; ++i) {
        if (!LightInScene(t->hostLights[i], t->plan.scene)) { SetLastError("light probe: a mesh light's triangles or instance lie outside the scene"); return DCRT_E_INVALID_ARG; }
    }
    return DCRT_OK;
}

DCRT_API int dcrt_device_light_sample(dcrt_tracer* t, const float* points, const uint32_t* states, uint32_t n, float* out_floats,
                                      uint32_t* out_words)
{
    TRACER_GUARD(t);
    if ((!points || !states || !out_floats || !out_words) && n) return DCRT_E_INVALID_ARG;
    uint32_t lightCount = 0;
    CHECKED(ProbeLights(t, &lightCount));
    // the two selections a state leads to stay inside the arrays: float(draw) * count can round up to count
    // (xoshiro128**'s output and state step, as dmath.h has them)
    // Under the light table both searches are clamped to the arrays and every lamp lies inside the scene
    // (BuildLightTable); ProbeLights has held the frame to the table's light count.
    auto rotl = [](uint32_t x, int k) { return (x << k) | (x >> (32 - k)); };
    for (uint32_t i = 0; i < n && !t->LightTableActive(); ++i) {
        uint32_t s[4];
        std::memcpy(s, states + 4 * (size_t)i, sizeof(s));
        float draw[2];
        for (int k = 0; k < 2; ++k) {
            draw[k] = (float)((rotl(s[0] * 5u, 7) * 9u) >> 8) / 16777216.0f;
            const uint32_t x = s[1] << 9;
            s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= x; s[3] = rotl(s[3], 11);
        }
        const float li = floorf(draw[0] * (float)lightCount);
        bool ok = li < (float)lightCount;
        if (ok) {
            uint32_t w[3];
            if (MeshLightRange(t->hostLights[(uint32_t)li], w)) {
                const float tri = (float)w[0] + floorf(draw[1] * (float)w[1]);
                ok = tri < (float)t->plan.scene.triangleCount && (uint32_t)tri < t->plan.scene.triangleCount;
            }
        }
        if (!ok) { SetLastError("light sample probe: a state selects past the lights or the triangles"); return DCRT_E_INVALID_ARG; }
    }
    const DeviceScene sc = t->plan.scene;
    DeviceGroup scratch;
    HostArray b[4] = {{points, nullptr, 12}, {states, nullptr, 16}, {nullptr, out_floats, 32}, {nullptr, out_words, 20}};
    return RoundTrip(t, scratch, n, b, [&] {
        hipLaunchKernelGGL(LightSampleProbe(t), ItemGrid(n), dim3(256), 0, t->stream, sc, lightCount, (const float*)b[0].device, (const uint4*)b[1].device, n,
                           (float*)b[2].device, (uint32_t*)b[3].device);
    });
}

DCRT_API int dcrt_device_light_eval(dcrt_tracer* t, const uint32_t* light_triangle, const float* normal_wi_distance, uint32_t n, float* out)
{
    TRACER_GUARD(t);
    if ((!light_triangle || !normal_wi_distance || !out) && n) return DCRT_E_INVALID_ARG;
    uint32_t lightCount = 0;
    CHECKED(ProbeLights(t, &lightCount));
    for (uint32_t i = 0; i < n; ++i) {
        if (light_triangle[2 * (size_t)i] >= lightCount || light_triangle[2 * (size_t)i + 1] >= t->plan.scene.triangleCount) {
            SetLastError("light eval probe: light or triangle index out of range");
            return DCRT_E_INVALID_ARG;
        }
    }
    const DeviceScene sc = t->plan.scene;
    DeviceGroup scratch;
    HostArray b[3] = {{light_triangle, nullptr, 8}, {normal_wi_distance, nullptr, 28}, {nullptr, out, 16}};
    return RoundTrip(t, scratch, n, b, [&] {
        hipLaunchKernelGGL(LightEvalProbe(t), ItemGrid(n), dim3(256), 0, t->stream, sc, lightCount, (const uint32_t*)b[0].device, (const float*)b[1].device, n,
                           (float*)b[2].device);
    });
}

DCRT_API int dcrt_tracer_set_environment_sampling(dcrt_tracer* t, int mode)
{
    TRACER_GUARD(t);
    return t->SetEnvSampling(mode);
}

DCRT_API int dcrt_tracer_get_environment_sampling(dcrt_tracer* t, int* mode, int* active)
{
    if (!t || (!mode && !active)) return DCRT_E_INVALID_ARG;
    if (mode) *mode = t->envSampling;
    if (active) *active = t->EnvTableActive() ? 1 : 0;
    return DCRT_OK;
}

// ---- Russian roulette -----------------------------------------------------------------------
DCRT_API int dcrt_roulette_default_params(dcrt_roulette_params* out)
{
    if (!out) return DCRT_E_INVALID_ARG;
    *out = kRouletteDefaults;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_set_roulette(dcrt_tracer* t, const dcrt_roulette_params* params)
{
    if (!t || !params) return DCRT_E_INVALID_ARG;
    if (!RouletteParamsValid(*params)) {
        SetLastError("Russian roulette: 0 < min_survival <= max_survival <= 1 and start_bounce <= DCRT_MAX_RAY_BOUNCE");
        return DCRT_E_INVALID_ARG;
    }
    // (BeginImage writes it into the frame constants with the next image: no graph holds it)
    t->roulette = *params;
    t->roulette.enable = params->enable ? 1u : 0u;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_get_roulette(dcrt_tracer* t, dcrt_roulette_params* out)
{
    if (!t || !out) return DCRT_E_INVALID_ARG;
    *out = t->roulette;
    return DCRT_OK;
}

DCRT_API int dcrt_device_roulette(dcrt_tracer* t, const dcrt_roulette_params* params, const float* throughputs, const float* u, uint32_t n,
                                  float* out_q, uint32_t* out_survive, float* out_scaled)
{
    TRACER_GUARD(t);
    if (!params || ((!throughputs || !u || !out_q || !out_survive || !out_scaled) && n)) return DCRT_E_INVALID_ARG;
    if (!RouletteParamsValid(*params)) { SetLastError("Russian roulette probe: invalid parameters"); return DCRT_E_INVALID_ARG; }
    const float lo = params->min_survival, hi = params->max_survival;
    DeviceGroup scratch;
    HostArray a[5] = {{throughputs, nullptr, 12}, {u, nullptr, 4}, {nullptr, out_q, 4}, {nullptr, out_survive, 4}, {nullptr, out_scaled, 12}};
    return RoundTrip(t, scratch, n, a, [&] {
        hipLaunchKernelGGL(roulette_probe_kernel, ItemGrid(n), dim3(256), 0, t->stream, lo, hi, (const float*)a[0].device, (const float*)a[1].device, n,
                           (float*)a[2].device, (uint32_t*)a[3].device, (float*)a[4].device);
    });
}

DCRT_API int dcrt_tracer_read_environment_distribution(dcrt_tracer* t, float* prob, float* row_cdf, float* marginal_cdf)
{
    TRACER_GUARD(t);
    if (!prob && !row_cdf && !marginal_cdf) return DCRT_E_INVALID_ARG;
    if (!t->EnvTableActive()) { SetLastError("no environment sampling table: the mode is uniform, or no scene, no cube, or a cube without finite positive weight"); return DCRT_E_NO_SCENE; }
    const size_t rows = (size_t)6 * t->plan.scene.envCubeSize, texels = rows * t->plan.scene.envCubeSize;
    if (prob) HIPCHECK(hipMemcpyAsync(prob, t->dEnvProb, texels * sizeof(float), hipMemcpyDeviceToHost, t->stream));
    if (row_cdf) HIPCHECK(hipMemcpyAsync(row_cdf, t->dEnvRowCdf, texels * sizeof(float), hipMemcpyDeviceToHost, t->stream));
    if (marginal_cdf) HIPCHECK(hipMemcpyAsync(marginal_cdf, t->dEnvMarginal, rows * sizeof(float), hipMemcpyDeviceToHost, t->stream));
    HIPCHECK(hipStreamSynchronize(t->stream));
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_environment_build_timing(dcrt_tracer* t, float* out_ms)
{
    if (!t || !out_ms) return DCRT_E_INVALID_ARG;
    *out_ms = t->envBuildMs;
    return DCRT_OK;
}

// The light table of the lights as they stand (dcrt.h, "light selection"; the kernels: kernels_impl.h), on the
// tracer's stream between two events. Where the lights' count, kinds, triangle ranges and instances are those the
// standing table was built for, only the light-level kernel runs again, into the same buffers: A_l is kept on the
// device, and no captured graph notices. Otherwise the buffers are freed and the whole table is built. No table:
// see dcrt_tracer::lightTable.
int dcrt_tracer::BuildLightTable()
{
    const uint32_t n = (uint32_t)hostLights.size();
    auto lamp = [](const dcrt_light& a, uint32_t w[3]) { return MeshLightRange(a, w) && !(a.flags & DCRT_LIGHT_FLAGS_POINT_LIGHT); };
    auto sameLamps = [&]() {
        if (!lightTable.prob || lightTable.lights.size() != n) return false;
        for (uint32_t i = 0; i < n; ++i) {
            const dcrt_light &a = lightTable.lights[i], &b = hostLights[i];
            if (a.flags != b.flags) return false;
            uint32_t wa[3], wb[3];
            if (lamp(a, wa) && lamp(b, wb) && std::memcmp(wa, wb, sizeof(wa)) != 0) return false;
        }
        return true;
    };
    lightBuildMs = 0.0f;
    if (sameLamps()) {
        lightTable.lights = hostLights;
        CHECKED(LightWeights());
        if (!(lightTable.total > 0.0 && std::isfinite(lightTable.total))) {
            lightAllocs.Free();
            lightTable = LightTable{};
        }
        return DCRT_OK;
    }
    lightAllocs.Free();
    lightTable = LightTable{};
    if (n == 0u) return DCRT_OK;
    uint32_t w[3];
    if (n == 1u && !lamp(hostLights[0], w)) return DCRT_OK;   // (nothing to choose: the Cornell configs keep their variants)
    std::vector<uint32_t> base(n);
    uint64_t entries = 0;
    for (uint32_t i = 0; i < n; ++i) {
        base[i] = (uint32_t)entries;
        if (!lamp(hostLights[i], w)) continue;
        if (!LightInScene(hostLights[i], plan.scene)) return DCRT_OK;   // (a lamp the kernels could not read)
        entries += w[1];
        if (entries > 0x7FFFFFFFu) return DCRT_OK;
    }
    CHECKED(CubeMeanLuminance());
    LightTable t;
    t.entries = (uint32_t)entries;
    t.lights = hostLights;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto build = [&]() -> int {
        CHECKED(lightAllocs.Alloc(&t.prob, n));
        CHECKED(lightAllocs.Alloc(&t.cdf, n));
        CHECKED(lightAllocs.Alloc(&t.triBase, n));
        CHECKED(lightAllocs.Alloc(&t.triProb, t.entries));
        CHECKED(lightAllocs.Alloc(&t.triCdf, t.entries));
        CHECKED(lightAllocs.Alloc(&t.areas, t.entries));
        CHECKED(lightAllocs.Alloc(&t.triSums, t.entries));
        CHECKED(lightAllocs.Alloc(&t.lightAreas, n));
        CHECKED(lightAllocs.Alloc(&t.weightSums, (size_t)n + 1));
        HIPCHECK(hipMemcpyAsync(t.triBase, base.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        HIPCHECK(hipEventCreate(&e0));
        HIPCHECK(hipEventCreate(&e1));
        HIPCHECK(hipEventRecord(e0, stream));
        if (t.entries)
            hipLaunchKernelGGL(light_tri_area_kernel, dim3((t.entries + 255u) / 256u), dim3(256), 0, stream, plan.scene, (const uint32_t*)t.triBase, n, t.entries, t.areas);
        hipLaunchKernelGGL(light_tri_scan_kernel, dim3((n + 3u) / 4u), dim3(256), 0, stream, (const dcrt_light*)dLights, (const uint32_t*)t.triBase, n,
                           (const float*)t.areas, t.triSums, t.lightAreas);
        hipLaunchKernelGGL(light_weights_kernel, dim3(1), dim3(256), 0, stream, (const dcrt_light*)dLights, n, (const double*)t.lightAreas, sceneRadius, envMeanY,
                           t.weightSums, t.prob, t.cdf);
        if (t.entries)
            hipLaunchKernelGGL(light_tri_finish_kernel, dim3((t.entries + 255u) / 256u), dim3(256), 0, stream, (const dcrt_light*)dLights, (const uint32_t*)t.triBase, n,
                               t.entries, (const float*)t.areas, (const double*)t.triSums, (const double*)t.lightAreas, t.triProb, t.triCdf);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(e1, stream));
        HIPCHECK(hipMemcpyAsync(&t.total, t.weightSums + n, sizeof(double), hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));   // (base ends with this function)
        HIPCHECK(hipEventElapsedTime(&lightBuildMs, e0, e1));
        return DCRT_OK;
    };
    const int rc = build();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (rc != DCRT_OK || !(t.total > 0.0 && std::isfinite(t.total))) {
        lightAllocs.Free();
        return rc;
    }
    lightTable = std::move(t);
    return DCRT_OK;
}

// Ybar of the uploaded cube, once per upload and only when a table is built: the cube read back from the device (the
// caller's array is not kept) and summed on the host in float64 in index order, as the definition has it. Measured
// figures for a large cube: DESIGN.md, "Light selection".
int dcrt_tracer::CubeMeanLuminance()
{
    if (envMeanYKnown) return DCRT_OK;
    const uint32_t n = plan.scene.envCubeSize;
    std::vector<float> cube((size_t)6 * n * n * 3);
    HIPCHECK(hipMemcpyAsync(cube.data(), plan.scene.envCube, cube.size() * sizeof(float), hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    double sumY = 0.0, sumOmega = 0.0;
    for (size_t i = 0; i < (size_t)6 * n * n; ++i) {
        const float* t = cube.data() + i * 3;
        const float y = std::fmax(0.0f, t[0] * 0.299f + t[1] * 0.587f + t[2] * 0.114f);
        const uint32_t x = (uint32_t)(i % n), row = (uint32_t)((i / n) % n);
        const double sc = (double)(2 * x + 1) / (double)n - 1.0, tc = (double)(2 * row + 1) / (double)n - 1.0;
        const double r2 = 1.0 + sc * sc + tc * tc;
        const double omega = (4.0 / ((double)n * (double)n)) / (r2 * std::sqrt(r2));
        sumY += (double)y * omega;
        sumOmega += omega;
    }
    envMeanY = sumY / sumOmega;
    envMeanYKnown = true;
    return DCRT_OK;
}

// The light-level kernel alone, over the standing table's A_l: lightProb and lightCdf rewritten in place
int dcrt_tracer::LightWeights()
{
    const uint32_t n = (uint32_t)lightTable.lights.size();
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto run = [&]() -> int {
        HIPCHECK(hipEventCreate(&e0));
        HIPCHECK(hipEventCreate(&e1));
        HIPCHECK(hipEventRecord(e0, stream));
        hipLaunchKernelGGL(light_weights_kernel, dim3(1), dim3(256), 0, stream, (const dcrt_light*)dLights, n, (const double*)lightTable.lightAreas, sceneRadius,
                           envMeanY, lightTable.weightSums, lightTable.prob, lightTable.cdf);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(e1, stream));
        HIPCHECK(hipMemcpyAsync(&lightTable.total, lightTable.weightSums + n, sizeof(double), hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
        HIPCHECK(hipEventElapsedTime(&lightBuildMs, e0, e1));
        return DCRT_OK;
    };
    const int rc = run();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return rc;
}

// DCRT_LIGHT_SAMPLING_*: set on an uploaded scene, like the scene edits, and kept for it and every later scene. The
// table is built when the mode first asks for it and dropped when it no longer does; the plan is rederived, and the
// captured graphs go exactly when the variant or the table's pointers changed. Film and path state stay as they are.
int dcrt_tracer::SetLightSampling(int mode)
{
    if (mode != DCRT_LIGHT_SAMPLING_UNIFORM && mode != DCRT_LIGHT_SAMPLING_POWER) { SetLastError("unknown light sampling mode"); return DCRT_E_INVALID_ARG; }
    if (!hasScene) { SetLastError("no scene uploaded"); return DCRT_E_NO_SCENE; }
    if (mode == lightSampling) return DCRT_OK;
    lightSampling = mode;
    HIPCHECK(hipStreamSynchronize(stream));
    if (mode == DCRT_LIGHT_SAMPLING_POWER) CHECKED(BuildLightTable());
    CHECKED(RederiveShading());
    HIPCHECK(hipStreamSynchronize(stream));
    if (mode == DCRT_LIGHT_SAMPLING_UNIFORM) {   // (no launch reads it any more: the plan above named none)
        lightAllocs.Free();
        lightTable = LightTable{};
    }
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_set_light_sampling(dcrt_tracer* t, int mode)
{
    TRACER_GUARD(t);
    return t->SetLightSampling(mode);
}

DCRT_API int dcrt_tracer_get_light_sampling(dcrt_tracer* t, int* mode, int* active)
{
    if (!t || (!mode && !active)) return DCRT_E_INVALID_ARG;
    if (mode) *mode = t->lightSampling;
    if (active) *active = t->LightTableActive() ? 1 : 0;
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_read_light_distribution(dcrt_tracer* t, dcrt_light_table_info* out_info, float* light_prob, float* light_cdf,
                                                 uint32_t* tri_base, float* tri_prob, float* tri_cdf)
{
    TRACER_GUARD(t);
    if (!out_info && !light_prob && !light_cdf && !tri_base && !tri_prob && !tri_cdf) return DCRT_E_INVALID_ARG;
    if (!t->LightTableActive()) { SetLastError("no light table: the mode is uniform, or no scene, or lights without finite positive weight, or nothing to choose"); return DCRT_E_NO_SCENE; }
    const dcrt_tracer::LightTable& lt = t->lightTable;
    const size_t n = lt.lights.size(), e = lt.entries;
    if (out_info) *out_info = dcrt_light_table_info{ (uint32_t)n, lt.entries, t->sceneRadius, lt.total };
    if (light_prob) HIPCHECK(hipMemcpyAsync(light_prob, lt.prob, n * sizeof(float), hipMemcpyDeviceToHost, t->stream));
    if (light_cdf) HIPCHECK(hipMemcpyAsync(light_cdf, lt.cdf, n * sizeof(float), hipMemcpyDeviceToHost, t->stream));
    if (tri_base) HIPCHECK(hipMemcpyAsync(tri_base, lt.triBase, n * sizeof(uint32_t), hipMemcpyDeviceToHost, t->stream));
    if (tri_prob && e) HIPCHECK(hipMemcpyAsync(tri_prob, lt.triProb, e * sizeof(float), hipMemcpyDeviceToHost, t->stream));
    if (tri_cdf && e) HIPCHECK(hipMemcpyAsync(tri_cdf, lt.triCdf, e * sizeof(float), hipMemcpyDeviceToHost, t->stream));
    HIPCHECK(hipStreamSynchronize(t->stream));
    return DCRT_OK;
}

DCRT_API int dcrt_tracer_light_table_build_timing(dcrt_tracer* t, float* out_ms)
{
    if (!t || !out_ms) return DCRT_E_INVALID_ARG;
    *out_ms = t->lightBuildMs;
    return DCRT_OK;
}

DCRT_API int dcrt_device_env_lookup(dcrt_tracer* t, const float* directions, uint32_t n, float* out_rgb)
{
    TRACER_GUARD(t);
    if ((!directions || !out_rgb) && n) return DCRT_E_INVALID_ARG;
    if (!t->hasScene || !t->plan.scene.envCube || t->plan.scene.envCubeSize == 0u) { SetLastError("no scene uploaded, or no environment cube in it"); return DCRT_E_NO_SCENE; }
    const DeviceScene sc = t->plan.scene;
    DeviceGroup scratch;
    HostArray b[2] = {{directions, nullptr, 12}, {nullptr, out_rgb, 12}};
    return RoundTrip(t, scratch, n, b, [&] {
        hipLaunchKernelGGL(env_lookup_probe_kernel, ItemGrid(n), dim3(256), 0, t->stream, sc, (const float*)b[0].device, n, (float*)b[1].device);
    });
}

DCRT_API int dcrt_device_bsdf_sample(dcrt_tracer* t, const dcrt_bsdf_probe_material* m, uint32_t features, const float* wo,
                                     const float* u, uint32_t n, float* wi, float* f, float* pdf, uint32_t* delta)
{
    TRACER_GUARD(t);
    if (!m || ((!wo || !u || !wi || !f || !pdf || !delta) && n)) return DCRT_E_INVALID_ARG;
    DeviceGroup scratch;
    DeviceScene ps;
    CHECKED(ProbeScene(t, *m, scratch, &ps));
    HostArray a[6] = {{wo, nullptr, 12}, {u, nullptr, 12}, {nullptr, wi, 12}, {nullptr, f, 12}, {nullptr, pdf, 4}, {nullptr, delta, 4}};
    return RoundTrip(t, scratch, n, a, [&] {
        hipLaunchKernelGGL(bsdf_sample_kernel, ItemGrid(n), dim3(256), 0, t->stream, ps, *m, features, (const float*)a[0].device,
                           (const float*)a[1].device, n, (float*)a[2].device, (float*)a[3].device, (float*)a[4].device, (uint32_t*)a[5].device);
    });
}

}  // extern "C"

#ifdef DCRT_WAVE_TIMELINE
// Diagnostic build only: copy the per-wave cast timeline (see kernels_impl.h).
extern "C" DCRT_API int dcrt_debug_wave_timeline(dcrt_tracer* t, unsigned long long* stamps, uint32_t* items)
{
    TRACER_GUARD(t);
    HIPCHECK(hipStreamSynchronize(t->stream));
    HIPCHECK(hipMemcpyFromSymbol(stamps, HIP_SYMBOL(g_waveLog), sizeof(g_waveLog)));
    HIPCHECK(hipMemcpyFromSymbol(items, HIP_SYMBOL(g_waveItems), sizeof(g_waveItems)));
    return DCRT_OK;
}
#endif

#ifdef DCRT_PHASE_CLOCKS
// Diagnostic build only: read and clear the cast kernels' per-phase wave cycles.
extern "C" DCRT_API int dcrt_debug_phase_clocks(dcrt_tracer* t, unsigned long long* out)
{
    TRACER_GUARD(t);
    HIPCHECK(hipStreamSynchronize(t->stream));
    HIPCHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phaseClk), sizeof(g_phaseClk)));
    const unsigned long long zero[24] = {};
    HIPCHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_phaseClk), zero, sizeof(zero)));
    return DCRT_OK;
}
#endif
