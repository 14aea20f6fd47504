// kernels_impl.h -- MI355X (gfx950) kernels of the wavefront path tracer and the
// BxDF LUT integrator. Host orchestration lives in tracer.hip.
//
// Reference map (Shaders/WavefrontPathTracing.hlsl):
//   set_idle_kernel      SET_IDLE            :628-651
//   control_kernel       CONTROL + NEW_PATH  :483-607 + :176-255 (fused)
//   material_kernel      MATERIAL            :257-481
//   extension_kernel     EXTENSION_RAY_CAST  :66-122
//   shadow_kernel        SHADOW_RAY_CAST     :124-174
//   film_kernel          SampleConvolution.hlsl:67-106
//   lut_*_kernel         BxDFTexturesBuilding.hlsl:10-186
#include "kernels.h"
// (included once, by tracer.hip)

namespace dcrt {
namespace dev {

#ifdef DCRT_PHASE_CLOCKS
// Diagnostic build only (tools/phase_clocks.py): shader-clock cycles the cast kernels'
// waves spend per phase of the persistent loop, summed over all waves:
// [0] hand-over + result stores + ray set-up, [1] phase A (node visits), [2] phase B
// (leaf work), [3] loop trips, [4] phase-A checks, [5] phase-B entries.
// MATERIAL: [8] loads + Li update, [9] HitInfoToIntersection, [10] record / sample stores,
// [11] emission + NEE (BSDF frame, light sample, BSDF eval + pdf, shadow ray), [12] BSDF
// sample + new ray, [13] end-of-path loads, [14] queue appends (barriers + atomics), [15] items.
__device__ unsigned long long g_phaseClk[24];
#define DCRT_PHASE_INIT unsigned long long clk_[6] = {0, 0, 0, 0, 0, 0}; unsigned long long tP_ = __builtin_amdgcn_s_memtime()
#define DCRT_PHASE(i) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); clk_[i] += t_ - tP_; tP_ = t_; } while (0)
#define DCRT_PHASE_COUNT(i) (++clk_[i])
#define DCRT_PHASE_FLUSH() do { if ((threadIdx.x & 63u) == 0) for (int i_ = 0; i_ < 6; ++i_) atomicAdd(&g_phaseClk[i_], clk_[i_]); } while (0)
#define DCRT_MCLK_INIT unsigned long long mclk_[8] = {0, 0, 0, 0, 0, 0, 0, 0}; unsigned long long mT_ = __builtin_amdgcn_s_memtime()
#define DCRT_MCLK(i) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); mclk_[i] += t_ - mT_; mT_ = t_; } while (0)
#define DCRT_MCLK_FLUSH(items) do { mclk_[7] += (items); if ((threadIdx.x & 63u) == 0) for (int i_ = 0; i_ < 8; ++i_) atomicAdd(&g_phaseClk[8 + i_], mclk_[i_]); } while (0)
// (shade_path's sections clock into its caller's MATERIAL clocks)
#define DCRT_MCLK_PARAMS , unsigned long long (&mclk_)[8], unsigned long long& mT_
#define DCRT_MCLK_ARGS , mclk_, mT_
#else
#define DCRT_MCLK_PARAMS
#define DCRT_MCLK_ARGS
#define DCRT_MCLK_INIT do {} while (0)
#define DCRT_MCLK(i) do {} while (0)
#define DCRT_MCLK_FLUSH(items) do {} while (0)
#define DCRT_PHASE_INIT do {} while (0)
#define DCRT_PHASE(i) do {} while (0)
#define DCRT_PHASE_COUNT(i) do {} while (0)
#define DCRT_PHASE_FLUSH() do {} while (0)
#endif

// One atomic per workgroup: wave ballot + mbcnt prefix, LDS scan over waves.
// Every thread of the block must call it (it contains barriers).
__device__ __forceinline__ uint32_t block_append(bool pred, uint32_t* counter, uint32_t* sm)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(pred);
    const uint32_t prefix = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    if (lane == 0) sm[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        const uint32_t waves = blockDim.x >> 6;
        for (uint32_t w = 0; w < waves; ++w) { const uint32_t c = sm[w]; sm[w] = total; total += c; }
        sm[32] = total ? atomicAdd(counter, total) : 0u;
    }
    __syncthreads();
    const uint32_t r = sm[32] + sm[wave] + prefix;
    __syncthreads();
    return r;
}

// Two appends at once (one barrier round for both queues): returns the slots of `pa` in
// counter a and of `pb` in counter b. sm needs 2 * (waves + 1) words; two calls in a row
// must use different sm halves (callers alternate), so no third barrier guards reuse.
__device__ __forceinline__ void block_append2(bool pa, uint32_t* ca, bool pb, uint32_t* cb, uint32_t* sm, uint32_t* ra, uint32_t* rb)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t waves = blockDim.x >> 6;
    const unsigned long long ma = __ballot(pa), mb = __ballot(pb);
    const uint32_t xa = __builtin_amdgcn_mbcnt_hi((uint32_t)(ma >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ma, 0u));
    const uint32_t xb = __builtin_amdgcn_mbcnt_hi((uint32_t)(mb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mb, 0u));
    if (lane == 0) { sm[wave] = (uint32_t)__popcll(ma); sm[16 + wave] = (uint32_t)__popcll(mb); }
    __syncthreads();
    if (threadIdx.x < 2) {   // thread 0: queue a, thread 1: queue b (their atomics overlap)
        uint32_t* q = sm + threadIdx.x * 16;
        uint32_t total = 0;
        for (uint32_t w = 0; w < waves; ++w) { const uint32_t c = q[w]; q[w] = total; total += c; }
        q[15] = total ? atomicAdd(threadIdx.x ? cb : ca, total) : 0u;
    }
    __syncthreads();
    *ra = sm[15] + sm[wave] + xa;
    *rb = sm[31] + sm[16 + wave] + xb;
}

// Three appends at once (MATERIAL: extension, shadow and finish queues): as block_append2,
// threads 0 / 1 / 2 issue the three atomics together. sm needs 48 words per call (callers
// alternate two halves of 96).
__device__ __forceinline__ void block_append3(bool pa, uint32_t* ca, bool pb, uint32_t* cb, bool pc, uint32_t* cc, uint32_t* sm,
                                              uint32_t* ra, uint32_t* rb, uint32_t* rc)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t waves = blockDim.x >> 6;
    const unsigned long long ma = __ballot(pa), mb = __ballot(pb), mc = __ballot(pc);
    const uint32_t xa = __builtin_amdgcn_mbcnt_hi((uint32_t)(ma >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ma, 0u));
    const uint32_t xb = __builtin_amdgcn_mbcnt_hi((uint32_t)(mb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mb, 0u));
    const uint32_t xc = __builtin_amdgcn_mbcnt_hi((uint32_t)(mc >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mc, 0u));
    if (lane == 0) { sm[wave] = (uint32_t)__popcll(ma); sm[16 + wave] = (uint32_t)__popcll(mb); sm[32 + wave] = (uint32_t)__popcll(mc); }
    __syncthreads();
    if (threadIdx.x < 3) {
        uint32_t* q = sm + threadIdx.x * 16;
        uint32_t total = 0;
        for (uint32_t w = 0; w < waves; ++w) { const uint32_t c = q[w]; q[w] = total; total += c; }
        q[15] = total ? atomicAdd(threadIdx.x == 0 ? ca : (threadIdx.x == 1 ? cb : cc), total) : 0u;
    }
    __syncthreads();
    *ra = sm[15] + sm[wave] + xa;
    *rb = sm[31] + sm[16 + wave] + xb;
    *rc = sm[47] + sm[32 + wave] + xc;
}

__device__ __forceinline__ unsigned long long wave_sum(uint32_t v)
{
    unsigned long long s = v;
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

__global__ void set_frame_kernel(FrameConstants* dst, FrameConstants src) { *dst = src; }

__global__ void set_idle_kernel(PathPool pool, Counters* counters, Globals* g, uint32_t totalBlocks)
{
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid < pool.size) pool.flags[tid] = kFlagIdle;
    if (tid < 2 * (uint32_t)(sizeof(Counters) / 4)) ((uint32_t*)counters)[tid] = 0u;
    if (tid < kShards) g->nextBlock[tid * kShardStride] = 0u;
    if (tid == 0) {
        g->totalBlocks = totalBlocks;
        g->batchImages = 1u;
        g->batchCap = 1u;
        g->imageComplete = 0u;
        g->poolIdle = 0u;
        g->prevLive = 0u;
        g->stopped = 0u;
        g->imagesDone = 0u;
        g->imageTarget = 1u;
        g->staticFill = 0u;
        g->staticGrid = 0u;
        g->skipFilm = 0u;
    }
}

// Preset the shard cursors for a batch start (see Globals::staticFill): shard s's first
// min(waves of its CONTROL workgroups, its blocks) blocks are taken statically.
// Invariant the batch start relies on: every slot is idle when staticFill is set -- the two
// callers are begin_images_kernel (right after BeginImage's set_idle_kernel) and
// advance_image_kernel (only once the batch completed: no path was live entering the last
// iteration and none was started, end_iteration). The static claims (and the virtual start's
// pixel / flag writes, control_kernel) overwrite the slots without checking them.
__device__ __forceinline__ void begin_batch_claims(Globals* g)
{
    const uint32_t G = g->staticGrid, wavesPerGroup = kControlBlock >> 6;
    for (uint32_t s = 0; s < kShards; ++s) {
        const uint32_t blocks = g->totalBlocks > s ? (g->totalBlocks - s + kShards - 1) / kShards : 0u;
        const uint32_t waves = G > s ? ((G - s + kShards - 1) / kShards) * wavesPerGroup : 0u;
        g->nextBlock[s * kShardStride] = G ? min(blocks, waves) : 0u;
    }
    g->staticFill = G ? 1u : 0u;
}

// ---- the environment cube's sampling table (dcrt.h, "environment importance sampling") ----------
// Three plain 256-thread launches at upload. Sums are float64 throughout; a stored value is one
// rounding of a float64 quotient.
// An inclusive scan of one double per lane across the wave (Hillis-Steele over __shfl_up)
DEV double env_wave_scan(double v)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const double up = __shfl_up(v, d, 64);
        if (lane >= d) v += up;
    }
    return v;
}
// One wave per row r = face * n + y: the texel weights (env_texel_weight) scanned in chunks of 64 columns
// with a carry; the unnormalised row CDF and the row's total.
__global__ __launch_bounds__(256) void env_rows_kernel(const float* cube, uint32_t n, double* rowSums, double* rowTotals)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= 6u * n) return;   // (whole waves leave: r is wave-uniform)
    const uint32_t face = r / n, y = r - face * n;
    double carry = 0.0;
    for (uint32_t x0 = 0u; x0 < n; x0 += 64u) {
        const uint32_t x = x0 + lane;
        const double w = x < n ? env_texel_weight(cube, (int)n, (int)face, (int)y, (int)x) : 0.0;
        const double inc = carry + env_wave_scan(w);
        if (x < n) rowSums[(size_t)r * n + x] = inc;
        carry = __shfl(inc, 63, 64);
    }
    if (lane == 0u) rowTotals[r] = carry;
}
// One workgroup: the row totals scanned in chunks of its width with a carry; the unnormalised
// marginal CDF and, behind its last entry, the table's total.
__global__ __launch_bounds__(256) void env_marginal_kernel(const double* rowTotals, uint32_t rows, double* marginalSums)
{
    __shared__ double waveTotals[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    double carry = 0.0;
    for (uint32_t r0 = 0u; r0 < rows; r0 += 256u) {
        const uint32_t r = r0 + threadIdx.x;
        const double inc = env_wave_scan(r < rows ? rowTotals[r] : 0.0);
        if (lane == 63u) waveTotals[wave] = inc;
        __syncthreads();
        double before = carry;
        for (uint32_t w = 0u; w < wave; ++w) before += waveTotals[w];
        if (r < rows) marginalSums[r] = before + inc;
        carry = carry + waveTotals[0] + waveTotals[1] + waveTotals[2] + waveTotals[3];
        __syncthreads();
    }
    if (threadIdx.x == 0u) marginalSums[rows] = carry;
}
// Per texel: P = w / total, the row's CDF over its total (zeros for an empty row); per row: the
// marginal CDF over the total. The last entry of each stored CDF is exactly 1.
__global__ __launch_bounds__(256) void env_finish_kernel(const float* cube, uint32_t n, const double* rowSums, const double* rowTotals,
                                                         const double* marginalSums, float* prob, float* rowCdf, float* marginal)
{
    const uint32_t rows = 6u * n;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)rows * n) return;
    const uint32_t r = (uint32_t)(i / n), x = (uint32_t)(i - (size_t)r * n);
    const uint32_t face = r / n, y = r - face * n;
    const double total = marginalSums[rows], rowTotal = rowTotals[r];
    prob[i] = (float)(env_texel_weight(cube, (int)n, (int)face, (int)y, (int)x) / total);
    rowCdf[i] = rowTotal > 0.0 ? (x == n - 1u ? 1.0f : (float)(rowSums[i] / rowTotal)) : 0.0f;
    if (x == 0u) marginal[r] = r == rows - 1u ? 1.0f : (float)(marginalSums[r] / total);
}

// ---- the light table (dcrt.h, "light selection") ------------------------------------------------
// Four plain 256-thread launches at upload; a light edit that keeps the lamps reruns the third alone.
// Sums are float64 throughout; a stored value is one rounding of a float64 quotient. `triBase` comes
// from the host (dcrt_tracer::BuildLightTable), which also holds every mesh light's range to the scene.
// The kind light sampling takes a light for: its tests' order (point, directional, mesh, environment)
DEV uint32_t light_table_kind(uint32_t flags)
{
    if (flags & DCRT_LIGHT_FLAGS_POINT_LIGHT) return DCRT_LIGHT_FLAGS_POINT_LIGHT;
    if (flags & DCRT_LIGHT_FLAGS_DIRECTIONAL_LIGHT) return DCRT_LIGHT_FLAGS_DIRECTIONAL_LIGHT;
    if (flags & DCRT_LIGHT_FLAGS_MESH_LIGHT) return DCRT_LIGHT_FLAGS_MESH_LIGHT;
    return flags & DCRT_LIGHT_FLAGS_ENVIRONMENT_LIGHT;
}
DEV uint32_t light_table_tri_count(const dcrt_light& L)
{
    return light_table_kind(L.flags) == DCRT_LIGHT_FLAGS_MESH_LIGHT ? asu(L.position_or_triangle_range[1]) : 0u;
}
// The light of emissive entry e: the last l with triBase[l] <= e (triBase[0] = 0; lights without entries share
// their successor's base and come before it)
DEV uint32_t light_of_entry(const uint32_t* triBase, uint32_t n, uint32_t e)
{
    uint32_t lo = 0u, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (triBase[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}
// One thread per emissive entry: a_t as sample_light computes it, 0 where the sampler's threshold rejects it
__global__ __launch_bounds__(256) void light_tri_area_kernel(DeviceScene sc, const uint32_t* triBase, uint32_t n, uint32_t entries, float* areas)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= entries) return;
    const uint32_t l = light_of_entry(triBase, n, e);
    const dcrt_light& L = sc.lights[l];
    const uint32_t tri = asu(L.position_or_triangle_range[0]) + (e - triBase[l]);
    const float4* M = sc.transforms + (size_t)asu(L.position_or_triangle_range[2]) * 3;
    const V3 w0 = mul43(tri_pos(sc, tri, 0), 1.0f, M), w1 = mul43(tri_pos(sc, tri, 1), 1.0f, M), w2 = mul43(tri_pos(sc, tri, 2), 1.0f, M);
    areas[e] = light_table_area(length(cross(w2 - w0, w1 - w0)) * 0.5f);
}
// One wave per light: its triangles' areas scanned in chunks of 64 entries with a carry; the unnormalised
// triangle CDF and the lamp's area A_l (0 for a light that is no mesh light)
__global__ __launch_bounds__(256) void light_tri_scan_kernel(const dcrt_light* lights, const uint32_t* triBase, uint32_t n, const float* areas,
                                                             double* triSums, double* lightAreas)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t l = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (l >= n) return;   // (whole waves leave: l is wave-uniform)
    const uint32_t count = light_table_tri_count(lights[l]), base = triBase[l];
    double carry = 0.0;
    for (uint32_t k0 = 0u; k0 < count; k0 += 64u) {
        const uint32_t k = k0 + lane;
        const double inc = carry + env_wave_scan(k < count ? (double)areas[base + k] : 0.0);
        if (k < count) triSums[base + k] = inc;
        carry = __shfl(inc, 63, 64);
    }
    if (lane == 0u) lightAreas[l] = carry;
}
// A light's weight: its power up to the factors the definition keeps (radius: R, meanY: the cube's Ybar or 1)
DEV double light_table_weight(const dcrt_light& L, double area, double radius, double meanY)
{
    const double pi = 3.14159265358979323846;
    const double y = (double)fmaxf(0.0f, L.radiance[0] * 0.299f + L.radiance[1] * 0.587f + L.radiance[2] * 0.114f);
    switch (light_table_kind(L.flags)) {
    case DCRT_LIGHT_FLAGS_POINT_LIGHT: return 4.0 * pi * y;
    case DCRT_LIGHT_FLAGS_DIRECTIONAL_LIGHT: return pi * radius * radius * y;
    case DCRT_LIGHT_FLAGS_MESH_LIGHT: return pi * y * area;
    case DCRT_LIGHT_FLAGS_ENVIRONMENT_LIGHT: return 4.0 * pi * (pi * radius * radius) * y * meanY;
    default: return 0.0;
    }
}
// One workgroup over the lights: the weights scanned in chunks of its width with a carry, then P(l) with its
// uniform share and the CDF of P; the total behind the sums' last entry, for the host's "inactive" test.
__global__ __launch_bounds__(256) void light_weights_kernel(const dcrt_light* lights, uint32_t n, const double* lightAreas, double radius, double meanY,
                                                            double* weightSums, float* lightProb, float* lightCdf)
{
    __shared__ double waveTotals[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    double carry = 0.0;
    for (uint32_t l0 = 0u; l0 < n; l0 += 256u) {
        const uint32_t l = l0 + threadIdx.x;
        const double inc = env_wave_scan(l < n ? light_table_weight(lights[l], lightAreas[l], radius, meanY) : 0.0);
        if (lane == 63u) waveTotals[wave] = inc;
        __syncthreads();
        double before = carry;
        for (uint32_t w = 0u; w < wave; ++w) before += waveTotals[w];
        if (l < n) weightSums[l] = before + inc;
        carry = carry + waveTotals[0] + waveTotals[1] + waveTotals[2] + waveTotals[3];
        __syncthreads();
    }
    if (threadIdx.x == 0u) weightSums[n] = carry;
    // (every thread holds the same total, and reads back only the sums it wrote itself)
    const double total = carry, share = kLightUniformShare;
    for (uint32_t l = threadIdx.x; l < n; l += 256u) {
        const double w = light_table_weight(lights[l], lightAreas[l], radius, meanY);
        lightProb[l] = (float)((1.0 - share) * (w / total) + share / (double)n);
        lightCdf[l] = l == n - 1u ? 1.0f : (float)((1.0 - share) * (weightSums[l] / total) + share * (double)(l + 1u) / (double)n);
    }
}
// Per emissive entry: P(t | l) = a_t / A_l and the lamp's CDF, its last entry exactly 1; zeros for a lamp without area
__global__ __launch_bounds__(256) void light_tri_finish_kernel(const dcrt_light* lights, const uint32_t* triBase, uint32_t n, uint32_t entries,
                                                               const float* areas, const double* triSums, const double* lightAreas,
                                                               float* triProb, float* triCdf)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= entries) return;
    const uint32_t l = light_of_entry(triBase, n, e);
    const double A = lightAreas[l];
    const bool last = e - triBase[l] == light_table_tri_count(lights[l]) - 1u;
    triProb[e] = A > 0.0 ? (float)((double)areas[e] / A) : 0.0f;
    triCdf[e] = A > 0.0 ? (last ? 1.0f : (float)(triSums[e] / A)) : 0.0f;
}

// The per-material rows of the plastic dielectric LUT (DeviceScene::dielRows; a launch per upload of
// the materials or the LUTs): float k of material m at rows[m * kDielRowFloats + k], with alpha as
// hit_to_intersection forms it for a material without the roughness checkerboard.
__global__ void build_diel_rows_kernel(const dcrt_material* materials, uint32_t count, const uint16_t* lut, const uint16_t* lutAvg,
                                       float* rows)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count * kDielRowFloats) return;
    const uint32_t m = i / kDielRowFloats, k = i % kDielRowFloats;
    float roughness = materials[m].roughness;
    roughness = roughness * 1.0f;
    const float alpha = roughness * roughness;
    rows[i] = diel_row_value(lut, lutAvg, alpha, materials[m].ior[0], k);
}
// (tests) the rows of the BSDF probe kernels' one material, whose alpha is given as it stands
__global__ void probe_diel_rows_kernel(const uint16_t* lut, const uint16_t* lutAvg, float* rows, float alpha, float ior)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < kDielRowFloats) rows[k] = diel_row_value(lut, lutAvg, alpha, ior, k);
}

// The world-space frame of every triangle (DeviceScene::triFrames) of a scene whose triangles each
// belong to one instance (`triInstance`, UINT32_MAX: a triangle no instance reaches): the per-hit
// helpers at u = v = +0 with the instance's matrix, and the two flags that say for which hits the
// normal and the tangent stand (hit_to_intersection).
__global__ void build_tri_frames_kernel(const float4* triVerts, const float4* triShade, const float4* transforms, const uint32_t* triInstance,
                                        uint32_t count, float4* frames)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const uint32_t inst = triInstance[t];
    float4 f0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), f1 = f0, f2 = f0;
    if (inst != 0xFFFFFFFFu) {
        const float4* P = triVerts + (size_t)t * 3;
        const float4* Q = triShade + (size_t)t * 6;
        const float4 q0 = P[0], q1 = P[1], q2 = P[2];
        const float4 a0 = Q[0], b0 = Q[1], a1 = Q[2], b1 = Q[3], a2 = Q[4], b2 = Q[5];
        const float4* M = transforms + (size_t)inst * 3;
        const V3 n = frame_normal(a0, a1, a2, 0.0f, 0.0f);
        const V3 nw = normalize(mul43(n, 0.0f, M));
        const V3 tw = normalize(mul43(frame_tangent(a0, b0, a1, b1, a2, b2, 0.0f, 0.0f, n), 0.0f, M));
        const V3 gw = normalize(mul43(frame_geometry_normal(mk(q0.x, q0.y, q0.z), mk(q1.x, q1.y, q1.z), mk(q2.x, q2.y, q2.z)), 0.0f, M));
        auto same3 = [](float x0, float y0, float z0, float x1, float y1, float z1) {
            return asu(x0) == asu(x1) && asu(y0) == asu(y1) && asu(z0) == asu(z1);
        };
        uint32_t flags = 0u;
        if (same3(a0.x, a0.y, a0.z, a1.x, a1.y, a1.z) && same3(a0.x, a0.y, a0.z, a2.x, a2.y, a2.z)) flags |= kFrameFlatNormal;
        if (same3(a0.w, b0.x, b0.y, a1.w, b1.x, b1.y) && same3(a0.w, b0.x, b0.y, a2.w, b2.x, b2.y)) flags |= kFrameFlatTangent;
        f0 = make_float4(nw.x, nw.y, nw.z, asf(flags));
        f1 = make_float4(tw.x, tw.y, tw.z, 0.0f);
        f2 = make_float4(gw.x, gw.y, gw.z, 0.0f);
    }
    frames[(size_t)t * 3] = f0;
    frames[(size_t)t * 3 + 1] = f1;
    frames[(size_t)t * 3 + 2] = f2;
}

// Upload-time gathers of the triangles' vertices (one fetch level less for the traversal
// and for MATERIAL's HitInfoToIntersection): positions (+ the degenerate flag and the
// per-triangle material id in the w words) and the shading attributes.
__global__ void build_tri_verts_kernel(const dcrt_vertex* vertices, const uint32_t* triangles, const uint32_t* materialIds,
                                       uint32_t count, float4* out, float4* shade)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    V3 p[3];
    for (int k = 0; k < 3; ++k) {
        const dcrt_vertex& v = vertices[triangles[t * 3 + k]];
        p[k] = mk(v.position[0], v.position[1], v.position[2]);
        shade[(size_t)t * 6 + 2 * k] = make_float4(v.normal[0], v.normal[1], v.normal[2], v.tangent[0]);
        shade[(size_t)t * 6 + 2 * k + 1] = make_float4(v.tangent[1], v.tangent[2], v.texcoord[0], v.texcoord[1]);
    }
    // RayTriangleIntersect's degenerate test (RayPrimitiveIntersect.inc.hlsl), hoisted to upload time
    const V3 cp = cross(p[1] - p[0], p[2] - p[0]);
    const float degenerate = dot(cp, cp) == 0.0f ? 1.0f : 0.0f;
    out[(size_t)t * 3] = make_float4(p[0].x, p[0].y, p[0].z, degenerate);
    out[(size_t)t * 3 + 1] = make_float4(p[1].x, p[1].y, p[1].z, __uint_as_float(materialIds[t]));
    out[(size_t)t * 3 + 2] = make_float4(p[2].x, p[2].y, p[2].z, 0.0f);
}

// ---- CONTROL (+ NEW_PATH) -------------------------------------------------------
// Live paths never pass through CONTROL: MATERIAL takes them from the previous
// iteration's extension queue and ends the paths it can (no shadow ray pending) itself.
// CONTROL (1) completes the paths MATERIAL ended with a shadow ray pending (listed in
// the previous iteration's finish queue): Li += light sampling result unless the shadow
// ray hit (:520-528) and WriteSample; (2) while its shard has pixel blocks to hand out,
// scans the slots for fully idle waves, which claim the next 8x8 block and start its
// paths (NEW_PATH). With every block claimed (the batch's first pass claims all of
// them) a pass is the finish list only, not a read of every slot's flags.
__global__ __launch_bounds__(kControlBlock) void control_kernel(PathPool pool, Film film, const FrameConstants* __restrict__ fc, Counters* cnt,
                                                       const Counters* prev, Globals* g, uint32_t debugRng)
{
    __shared__ uint32_t sm[64];
    if (g->stopped) return;                    // RenderImages finished: nothing live, nothing to claim
    const uint32_t epoch = epoch_of(cnt);      // (this iteration's: the previous end_iteration wrote it)
    {
        QueueMapN<kFinShards> fm;
        qmap(prev, kQFinish, &fm);
        const uint32_t nFin = drained(prev) ? 0u : fm.prefix[kFinShards];   // (drain_kernel completed them)
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nFin; i += gridDim.x * blockDim.x) {
            // the path's finish record and its shadow ray's result, both at its finish-queue
            // position (dense); only the pixel is per slot
            const uint32_t f = qpos(pool.finCap, fm, i);
            const FinishRec fr = pool.finPrevRec[f];
            const bool shadowHit = pool.finHitPrev[f] != 0u;
            const uint32_t path = asu(fr.lsrSlot.z);
            F3 li{fr.liLsr.x, fr.liLsr.y, fr.liLsr.z};
            const F3 lsr{fr.liLsr.w, fr.lsrSlot.x, fr.lsrSlot.y};
            li.x = li.x + (!shadowHit ? lsr.x : 0.0f);
            li.y = li.y + (!shadowHit ? lsr.y : 0.0f);
            li.z = li.z + (!shadowHit ? lsr.z : 0.0f);
            const uint32_t p = slot(pool.pixel, path);
            sample_at(film.samplePosition, p) = pixel_sample(*fc, p);
            sample_at(film.sampleValue, p) = make_float4(li.x, li.y, li.z, 0.0f);
            // (debug RNG: MATERIAL stored it when it ended the path)
            // last, after stores that consumed the loads: another workgroup's scan may see the
            // slot idle from here on and start a new path in it
            // (a path finished at its last shaded bounce: idle from the next iteration's scan on,
            // where MATERIAL's idle flag would have shown -- kFlagIdleFrom)
            slot(pool.flags, path) = asu(fr.lsrSlot.w) == kFinishEarly ? idle_from(epoch + 1u) : kFlagIdle;
        }
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t shard = blockIdx.x % kShards;
    uint32_t* cursor = &g->nextBlock[shard * kShardStride];
    // pixel blocks of this shard: shard, shard + kShards, ...
    const uint32_t shardBlocks = g->totalBlocks > shard ? (g->totalBlocks - shard + kShards - 1) / kShards : 0u;
    const bool staticFill = g->staticFill != 0u;
    if (staticFill && fc->virtualStart) {
        // Virtual batch start: every slot is idle (the previous batch drained), wave j of the
        // shard takes the shard's block j, and NEW_PATH is deferred -- the cast generates slot
        // i's camera ray from its pixel (new_path<true>) and the path's first MATERIAL pass
        // recomputes its rng (new_path<false>), so the only per-slot writes are the pixel (or
        // kNoPixel: a hole in the virtual queue) and the busy flag. A 4K batch's start wrote
        // 72 B per path here and read 64 of them back.
        for (uint32_t base = blockIdx.x * blockDim.x; base < pool.size; base += gridDim.x * blockDim.x) {
            const uint32_t tid = base + threadIdx.x;
            const uint32_t vb = base / kControlBlock;
            const uint32_t claimed = (vb / kShards) * (kControlBlock >> 6) + (threadIdx.x >> 6);
            uint32_t pixel = kNoPixel, px = 0, py = 0, image = 0;
            if (claimed < shardBlocks && block_pixel(*fc, film, shard + claimed * kShards, lane, &px, &py, &image)) {
                pixel = image * (film.width * film.height) + py * film.width + px;
                pool.flags[tid] = 0u;   // busy
            }
            pool.pixel[tid] = pixel;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) cnt->w[kVirtualWord * kShardStride] = pool.size;
        return;
    }
    if (!staticFill) {
        // (one read for the workgroup: the scan below holds barriers, so the exit must be uniform)
        __shared__ uint32_t exhausted;
        if (threadIdx.x == 0) exhausted = __hip_atomic_load(cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= shardBlocks;
        __syncthreads();
        if (exhausted) return;
    }
    // (the grid is a multiple of kShards, or one round: every virtual workgroup vb of this
    // workgroup is in its shard)
    for (uint32_t base = blockIdx.x * blockDim.x; base < pool.size; base += gridDim.x * blockDim.x) {
    const uint32_t tid = base + threadIdx.x;
    const uint32_t vb = base / kControlBlock;
    const bool idle = slot_idle(pool.flags[tid], epoch);
    // A fully idle wave claims the next 8x8 block (one atomic per workgroup); at a batch
    // start (all slots idle, cursors preset) wave j of the shard takes block j outright.
    const bool waveIdle = __ballot(!idle) == 0ull;
    uint32_t claimed = 0;
    bool got = false;
    if (staticFill) {
        claimed = (vb / kShards) * (kControlBlock >> 6) + (threadIdx.x >> 6);
        got = waveIdle && claimed < shardBlocks;
    } else {
        bool want = false;
        if (waveIdle && lane == 0)
            want = __hip_atomic_load(cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < shardBlocks;
        uint32_t bslot, unused;
        block_append2(false, cursor, want, cursor, sm, &unused, &bslot);
        claimed = (uint32_t)__shfl((int)bslot, 0, 64);
        got = __shfl((int)want, 0, 64) != 0 && claimed < shardBlocks;
    }
    const uint32_t block = shard + claimed * kShards;
    bool newPath = false;
    V3 o = mk(0.0f, 0.0f, 0.0f), d = mk(0.0f, 0.0f, 0.0f);
    Rng rng;
    rng.s0 = rng.s1 = rng.s2 = rng.s3 = 0u;
    if (got) {
        uint32_t px = 0, py = 0, image = 0;
        if (block_pixel(*fc, film, block, lane, &px, &py, &image)) {
            // NEW_PATH :211-237 (image `image` of the batch has frame seed image_seed(fc, image))
            rng = rng_init(px, py, image_seed(*fc, image));
            const float psx = next1(rng), psy = next1(rng);
            const float fsx = (psx + (float)px) / (float)fc->resolution[0];
            const float fsy = (psy + (float)py) / (float)fc->resolution[1];
            const float a0 = next1(rng), a1 = next1(rng), a2 = next1(rng);
            generate_ray(*fc, fsx, fsy, a0, a1, a2, &o, &d);
            if (fc->features & DCRT_FEATURE_ALLOW_ANYHIT) pool.extOpacity[tid] = next1(rng);   // :223-226
            // (the sub-pixel position is recomputed from the pixel where WriteSample needs it:
            // pixel_sample)
            pool.pixel[tid] = image * (film.width * film.height) + py * film.width + px;
            pool.flags[tid] = 0u;   // busy
            newPath = true;
        }
    }
    // (the other half of sm: the next round's first append reuses the first half only
    // after every thread has passed this append's barriers)
    uint32_t eslot, unused;
    block_append2(newPath, qctr(cnt, kQExt, shard), false, qctr(cnt, kQExt, shard), sm + 32, &eslot, &unused);
    if (newPath) {
        const uint32_t q = shard * pool.recCap + eslot;
        float4* r = ext_rec(pool.extRec, q);
        r[0] = make_float4(o.x, o.y, o.z, 0.0f);
        r[1] = make_float4(d.x, d.y, d.z, asf(tid));
        // NEW_PATH's state (:227-237) beside the ray: the rng, isDelta = true, bounce 0, the
        // slot (32 B); Li = 0, light sampling result = 0, T = 1, bsdfPdf = 0 are implicit
        // (kFlagFirst: writing all 64 B cost the 4K batches' first passes 3 GB of writes)
        PathStateA& st = state_at(pool.stateA, q);
        st.rng = make_uint4(rng.s0, rng.s1, rng.s2, rng.s3);
        st.lsrMisc = make_float4(0.0f, 0.0f, asf(kFlagDelta | kFlagFirst), asf(tid));
    }
    }
}

// MATERIAL's shading of one path at its hit (WavefrontPathTracing.hlsl:302-441): emission with
// MIS, termination, next-event estimation (the shadow ray and its light sampling result), the
// BSDF sample (the next extension ray), the new throughput, bsdfPdf (thr.w) and flags. `li` is
// the path's Li after CONTROL's `Li += light sampling result`. Shared by material_kernel and
// the drain kernel (drain_kernel), so both run the same arithmetic in the same order.
template <uint32_t CAPS, bool FRAMES = false>
__device__ __forceinline__ void shade_path(const DeviceScene& sc, const FrameConstants& fc, const HitRecord& hit, V3 dir, Rng& rng,
                                           uint32_t& flags, float4& thr, const F3& li, V3& T, V3& L, V3& lsr, bool& terminate,
                                           bool& hasShadow, V3& nO, V3& nD, float4& sO, V3& sD, float& extOpacity,
                                           float& shadowOpacity DCRT_MCLK_PARAMS)
{
    const uint32_t bounce = flags & 0xFFu;
    const uint32_t features = fc.features;
    const bool vndf = (features & DCRT_FEATURE_GGX_SAMPLE_VNDF) != 0;
    const bool hasHit = hit.t != inf();
    Intersection it;
    it.lightIndex = DCRT_LIGHT_INDEX_INVALID; it.triangleIndex = 0;
    it.geometryNormal = mk(0.0f, 0.0f, 0.0f);
    if (hasHit) hit_to_intersection<CAPS, FRAMES>(sc, hit, it);
    DCRT_MCLK(1);
    T = mk(thr.x, thr.y, thr.z);
    L = mk(li.x, li.y, li.z);
    // Evaluate light :331-349
    {
        const uint32_t lightIndex = hasHit ? it.lightIndex : fc.envLightIndex;
        const bool visible = (features & DCRT_FEATURE_LIGHT_VISIBLE) != 0;
        if (visible ? lightIndex != DCRT_LIGHT_INDEX_INVALID : (bounce > 0 && lightIndex != DCRT_LIGHT_INDEX_INVALID)) {
            V3 radiance; float lightPdf;
            evaluate_light<CAPS>(sc, lightIndex, it.triangleIndex, it.geometryNormal, dir, hit.t, fc.lightCount, &radiance, &lightPdf);
            if (lightPdf > 0.0f) {
                const float weight = !(flags & kFlagDelta) ? power_heuristic(thr.w, lightPdf) : 1.0f;
                L = L + T * radiance * weight;
            }
        }
    }
    lsr = mk(0.0f, 0.0f, 0.0f);
    if (bounce > fc.maxBounce || !hasHit) {
        flags |= kFlagTerminate;
        terminate = true;
    } else {
        const V3 wo = -dir;
        const BsdfFrame bf = bsdf_frame(sc, wo, it);
        if (fc.lightCount != 0) {
            const LightSample ls = sample_light<CAPS>(sc, it.position, fc.lightCount, rng);
            if (any_pos(ls.radiance) && ls.pdf > 0.0f) {
                const V3 bsdf = evaluate_bsdf(sc, vndf, ls.wi, bf, it);
                const float NdotWI = fabsf(dot(it.normal, ls.wi));
                // The pdf enters the weight of an area light's sample alone (kTableDeltaPdf): a variant
                // without mesh and environment lights samples delta lights only, and one wave-uniform
                // test of the knob stands in front of the call. The other variants compute it for every
                // sample as before (a branch per sample diverges where delta and area lights mix).
                bool wantPdf = true;
                if constexpr ((CAPS & (kCapLightMesh | kCapLightEnv)) == 0u) wantPdf = (sc.shadingTables & kTableDeltaPdf) == 0u;
                float bsdfPdf = 0.0f;
                if (wantPdf) bsdfPdf = evaluate_bsdf_pdf(sc, vndf, ls.wi, bf, it);
                const float weight = ls.isDelta ? 1.0f : power_heuristic(ls.pdf, bsdfPdf);
                lsr = T * ls.radiance * bsdf * NdotWI * weight / ls.pdf;
                const V3 so = offset_ray_origin(it.position, it.geometryNormal, ls.wi);
                sO = make_float4(so.x, so.y, so.z, ls.distance);   // (written into the shadow
                sD = ls.wi;                                         //  queue after the append)
                hasShadow = true;
            }
        }
        DCRT_MCLK(3);
        float bsdfPdf = 0.0f;
        bool isDelta = false;
        {
            const float sel = next1(rng);
            const float sx = next1(rng), sy = next1(rng);
            V3 wi, bsdf;
            sample_bsdf(sc, vndf, bf, sx, sy, sel, it, &wi, &bsdf, &bsdfPdf, &isDelta);
            if ((bsdf.x != 0.0f || bsdf.y != 0.0f || bsdf.z != 0.0f) && bsdfPdf != 0.0f) {
                const float NdotWI = fabsf(dot(it.normal, wi));
                T = T * bsdf * NdotWI / bsdfPdf;
                nO = offset_ray_origin(it.position, it.geometryNormal, wi);
                nD = wi;   // (written into the extension queue after the append)
                flags = (flags & 0xFFFFFF00u) | ((bounce + 1) & 0xFFu);
                // Russian roulette (off: one scalar test, and the lines above are the code without it): its draw
                // follows the three above, ahead of the opacity draws. A path it ends is a path whose sample was
                // rejected: the bounce index as it was and kFlagTerminate (T and the ray are read of survivors only).
                if (fc.rouletteEnable != 0u && bounce >= fc.rouletteStart &&
                    !roulette(fc.rouletteMin, fc.rouletteMax, T, [&] { return next1(rng); })) {
                    flags = (flags & 0xFFFFFF00u) | bounce | kFlagTerminate;
                    terminate = true;
                }
            } else {
                flags |= kFlagTerminate;
                terminate = true;
            }
        }
        thr.w = bsdfPdf;
        flags = isDelta ? flags | kFlagDelta : flags & ~kFlagDelta;
        if (features & DCRT_FEATURE_ALLOW_ANYHIT) {   // :422-430 (the caller stores them)
            if (!terminate) extOpacity = next1(rng);
            if (hasShadow) shadowOpacity = next1(rng);
        }
    }
}

// ---- MATERIAL -----------------------------------------------------------------------
#ifndef DCRT_MATERIAL_BLOCK
#define DCRT_MATERIAL_BLOCK 256
#endif
static_assert(DCRT_MATERIAL_BLOCK % 64 == 0 && DCRT_MATERIAL_BLOCK <= 960, "MATERIAL workgroup: whole waves, at most 15 (block_append3)");
// The any-scene MATERIAL variant is held to 5 waves/SIMD (<= 96 VGPRs; 117 and 4 waves
// unbounded): it then spills 3 VGPRs and still gains, coffee 3.12 -> 3.02, lamp 7.78 ->
// 7.62 ms/spp (three / two A/B passes). The scene-specialised variants reach 5 waves by
// themselves (95 VGPRs); held to 5 the compiler schedules them into 91 and the Cornell
// bench loses 2 % (2.393 -> 2.447, four passes), so they are left unbounded. The FUSED
// variants are held to 5 as well: unbounded, the Cornell one takes 98 VGPRs (4 waves); held,
// 94 with no scratch (tools/vgprs.sh).
#ifndef DCRT_MATERIAL_WAVES_PER_EU
#define DCRT_MATERIAL_WAVES_PER_EU 5
#endif
#ifndef DCRT_MATERIAL_OD_WAVES_PER_EU
#define DCRT_MATERIAL_OD_WAVES_PER_EU 1   // (the opaque / delta-light variants: the compiler's choice)
#endif
#define DCRT_MATERIAL_OCCUPANCY __attribute__((amdgpu_waves_per_eu(caps_any_scene(CAPS) || FUSED ? DCRT_MATERIAL_WAVES_PER_EU : DCRT_MATERIAL_OD_WAVES_PER_EU, 8)))
// CAPS: the scene capabilities this variant is compiled for (kCapAll = any scene; see
// kCapOpaqueDelta in dscene.h and dcrt_tracer::UploadScene).
// SCENE_LDS: the scene arrays MATERIAL's shading reads per item are copied into LDS by each
// workgroup first, so HitInfoToIntersection's dependent fetches are LDS reads -- 1: all of them
// (pre-gathered triangles, the forward instance transforms and instance words, materials,
// lights: small scenes, material_lds_layout's shading bytes within the host's budget); 2: all but the triangles
// (larger scenes: the hit -> triangle fetch stays global, the triangle -> material one and the
// light sample's reads become LDS reads); 0: none.
// PROBE: counts the rays per film row (the row-cost probe); launched only while it is on.
// FUSED (with SCENE_LDS == 1; launched exactly when the cast is cast_kernel's CELLS variant): a shadow
// ray whose 1/d is finite is tested here, against the point light's direction cells
// (cells_occluded_cached, the function the cast calls, over this workgroup's own LDS copy of what it
// reads: `si`), instead of travelling through the shadow queue -- no 32-B record, no result word. Its
// answer goes into the path's flags (kFlagShadowResolved) or, for a path that ends here, straight to
// finHit at its finish-queue position. A ray with a non-finite 1/d component takes the queue as before.
// Early finish (variants without mesh and environment lights, not PROBE, sc.earlyFinish != 0, no
// ALLOW_ANYHIT_SHADER): a path that continues past the last shaded bounce is handed to CONTROL here, as a
// path that ends with its shadow ray pending is, and its extension ray goes to the last-ray queue
// (kLastRayWord) -- the pass that would only have completed it has no item.
template <uint32_t CAPS, int SCENE_LDS, bool PROBE = false, bool FUSED = false>
__global__ __launch_bounds__(DCRT_MATERIAL_BLOCK) DCRT_MATERIAL_OCCUPANCY void material_kernel(PathPool pool, DeviceScene sc, const FrameConstants* __restrict__ fcr, Counters* cnt,
                                                                             const Counters* prev, const SampleOut* __restrict__ sampleOut, ShadowInline si)
{
    static_assert(!FUSED || (SCENE_LDS == 1 && !PROBE), "FUSED: beside the whole LDS shading copy");
    // EARLY: this variant may finish a path at its last shaded bounce (sc.earlyFinish says whether it does)
    constexpr bool EARLY = caps_early_finish(CAPS) && !PROBE;
#if defined(DCRT_MATERIAL_PRIO) && DCRT_MATERIAL_PRIO > 0
    __builtin_amdgcn_s_setprio(DCRT_MATERIAL_PRIO);   // (A/B: issue priority over a co-resident cast)
#endif
    __shared__ uint32_t sm[96 + (FUSED ? 1 : 0)];
    // the work list: the previous iteration's extension queue (its rays have been cast) -- or
    // a batch start's virtual queue (item i = path slot i, kVirtualWord)
    QueueMap qm;
    qmap(prev, kQExt, &qm);
    const uint32_t virt = virtual_items(prev);
    // (a work list drain_kernel already completed holds nothing)
    const uint32_t count = drained(prev) ? 0u : (virt ? virt : qm.prefix[kShards]);
    const uint32_t shard = blockIdx.x % kShards;
    const uint32_t fshard = blockIdx.x % kFinShards;
    // The frame constants through a restrict-qualified pointer: nothing this kernel stores
    // aliases them, so their reads in the item loop are scalar loads (scalar cache) -- through
    // the plain pointer they were vector loads, each waited on at once, several dependent round
    // trips per round.
    const FrameConstants& fcv = *fcr;
    // (FUSED) the cells' LDS copy, and the shadow rays tested here: counted per wave, added per workgroup
    const float4* cellNodes = nullptr;
    const float4* cellTris = nullptr;
    const uint32_t* cellLeaves = nullptr;
    uint32_t& inlineTotal = sm[FUSED ? 96 : 0];
    uint32_t inlineRays = 0;
    if constexpr (SCENE_LDS != 0) {
        extern __shared__ float4 sceneLds[];
        if (blockIdx.x * blockDim.x >= count) return;   // (no item: no copy)
        const uint32_t T = SCENE_LDS == 1 ? sc.triangleCount : 0u, I = sc.instanceCount;
        float4* tv = sceneLds;
        float4* ts = tv + 3u * T;
        float4* tf = ts + 6u * T;
        uint32_t* w = (uint32_t*)(tf + 3u * I);
        uint32_t* li = w;
        uint32_t* ov = li + I;
        uint32_t* mt = ov + I;
        uint32_t* lt = mt + 13u * sc.ldsMaterials;
        float* rw = (float*)(lt + 7u * sc.ldsLights);   // (the dielectric LUT's rows of sc.ldsRows materials)
        for (uint32_t i = threadIdx.x; i < kDielRowFloats * sc.ldsRows; i += blockDim.x) rw[i] = sc.dielRows[i];
        // (the triangles' frames at the next 16-B boundary, in front of the fused variant's cells: material_lds_layout,
        // dscene.h, is the layout these pointers walk and the host sizes the launch by)
        const uint32_t frameOff = material_lds_layout(T, I, sc.ldsMaterials, sc.ldsLights, sc.ldsRows, false, 0u, false).framesAt;
        const uint32_t FT = sc.ldsFrames ? T : 0u;
        float4* fr = sceneLds + (frameOff >> 4);
        for (uint32_t i = threadIdx.x; i < 3u * FT; i += blockDim.x) fr[i] = sc.triFrames[i];
        for (uint32_t i = threadIdx.x; i < 3u * T; i += blockDim.x) tv[i] = sc.triVerts[i];
        for (uint32_t i = threadIdx.x; i < 6u * T; i += blockDim.x) ts[i] = sc.triShade[i];
        for (uint32_t i = threadIdx.x; i < 3u * I; i += blockDim.x) tf[i] = sc.transforms[i];
        for (uint32_t i = threadIdx.x; i < I; i += blockDim.x) { li[i] = sc.instanceLightIndices[i]; ov[i] = sc.overrides[i]; }
        for (uint32_t i = threadIdx.x; i < 13u * sc.ldsMaterials; i += blockDim.x) mt[i] = ((const uint32_t*)sc.materials)[i];
        for (uint32_t i = threadIdx.x; i < 7u * sc.ldsLights; i += blockDim.x) lt[i] = ((const uint32_t*)sc.lights)[i];
        if constexpr (FUSED) {
            // behind the shading copy (material_lds_layout's cellsAt): the cast's scene cache of the flat
            // scene, as scene_cache_load<true> fills it, then the leaf words
            float4* cn = fr + 3u * FT;
            float4* ct = cn + 2u * si.nodeCount;
            uint32_t* cl = (uint32_t*)(ct + kRotTriFloat4 * T);
            for (uint32_t i = threadIdx.x; i < 2u * si.nodeCount; i += blockDim.x) cn[i] = si.nodes[i];
            for (uint32_t i = threadIdx.x; i < kRotTriFloat4 * T; i += blockDim.x) ct[i] = rot_tri_float4(sc.triVerts, i);
            for (uint32_t i = threadIdx.x; i < kCellWords; i += blockDim.x) cl[i] = si.leaves[i];
            if (threadIdx.x == 0) inlineTotal = 0u;
            cellNodes = cn;
            cellTris = ct;
            cellLeaves = cl;
        }
        __syncthreads();
        if constexpr (SCENE_LDS == 1) {
            sc.triVerts = tv;
            sc.triShade = ts;
        }
        sc.transforms = tf;
        sc.instanceLightIndices = li;
        sc.overrides = ov;
        sc.materials = (const dcrt_material*)mt;
        sc.lights = (const dcrt_light*)lt;
        if (sc.ldsRows != 0u) sc.dielRows = rw;
        if (FT != 0u) sc.triFrames = fr;
    }
    DCRT_MCLK_INIT;
    uint32_t itemsDone = 0;
    uint32_t round = 0;   // grid-stride round: alternates block_append2's sm halves
    // (EARLY) the flags word of a slot whose path this pass completes at its last shaded bounce (one scalar)
    uint32_t doneFlag = kFlagIdle;
    if constexpr (EARLY) doneFlag = (uint32_t)__builtin_amdgcn_readfirstlane((int)idle_from(epoch_of(cnt) + 2u));
    for (uint32_t base = blockIdx.x * blockDim.x; base < count; base += gridDim.x * blockDim.x) {
    const uint32_t i = base + threadIdx.x;
    bool active = i < count;
    uint32_t newPixel = kNoPixel;   // a virtual item's pixel (a hole of the virtual queue has none)
    if (virt && active) {
        newPixel = slot(pool.pixel, i);
        active = newPixel != kNoPixel;
    }
    bool terminate = false, hasShadow = false, ends = false, last = false;
    uint32_t path = 0, pix = 0;
    float4 sample = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float2* outPos = nullptr;
    float4* outVal = nullptr;
    V3 nO = mk(0.0f, 0.0f, 0.0f), nD = mk(0.0f, 0.0f, 0.0f);   // the next extension ray
    float4 sO = make_float4(0.0f, 0.0f, 0.0f, 0.0f);            // the shadow ray (origin, tMax)
    V3 sD = mk(0.0f, 0.0f, 0.0f);
    // the path's state after this pass, stored at the positions the appends return
    uint32_t pathFlags = 0;
    float4 sThr = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    V3 sT = mk(0.0f, 0.0f, 0.0f), sL = mk(0.0f, 0.0f, 0.0f), sLsr = mk(0.0f, 0.0f, 0.0f);
    uint4 sRng = make_uint4(0u, 0u, 0u, 0u);
    if (active) {
        ++itemsDone;
        // Everything this pass reads is indexed by the item (no load waits for another):
        // the path's state record at its extension-queue position q, the cast's hit record
        // (with the ray's direction) at item i, the result of the path's last shadow ray at q
        // (only when it cast one: kFlagShadowPending)
        const float4 h4 = pool.hit[2 * i], hd = pool.hit[2 * i + 1];
        HitRecord hit;
        hit.t = h4.x; hit.u = h4.y; hit.v = h4.z; hit.tri = asu(h4.w); hit.inst = asu(hd.w);
        const V3 dir = mk(hd.x, hd.y, hd.z);
        Rng rng;
        uint32_t flags;
        float4 thr, l4, l2;
        bool shadowHit = false;
        if (virt) {
            // a virtual batch start's path (slot i): NEW_PATH's state (:227-237) recomputed from
            // its pixel -- the rng after the five camera draws, isDelta, bounce 0, T = 1,
            // bsdfPdf = 0, Li = 0, no light sampling result
            V3 unusedO, unusedD;
            rng = new_path<false>(fcv, newPixel, &unusedO, &unusedD);
            path = i;
            flags = kFlagDelta;
            thr = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
            l4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            l2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        } else {
            const uint32_t q = qpos(pool.recCap, qm, i);
            const PathStateA& ps = state_at(pool.stateAPrev, q);
            const PathStateB& psB = state_at(pool.stateBPrev, q);
            // All of the item's loads in one round trip: both state halves and the shadow result
            // are read unconditionally (position q is always allocated; what the flags say is not
            // there is stale and not used) -- conditioned on the flags, the compiler issued them
            // only after the first half arrived, a second and third dependent round trip.
            const uint4 r4 = ps.rng;
            l2 = ps.lsrMisc;
            const float4 bThr = psB.thr, bLi = psB.liLsr;
            uint32_t shRaw = 0u;
            if constexpr (FUSED) {
                // (the queue is the rare route here: the result is fetched only by a wave one of
                // whose paths took it, behind the flags -- one ballot, then the dependent load)
                if (__ballot((asu(l2.z) & kFlagShadowPending) != 0u) != 0ull) shRaw = pool.shadowHitPrev[q];
            } else {
                shRaw = pool.shadowHitPrev[q];
            }
            rng.s0 = r4.x; rng.s1 = r4.y; rng.s2 = r4.z; rng.s3 = r4.w;
            path = asu(l2.w);
            flags = asu(l2.z);
            // a new path's first pass: NEW_PATH's constants, not the record's unwritten half
            const bool first = (flags & kFlagFirst) != 0u;
            thr = first ? make_float4(1.0f, 1.0f, 1.0f, 0.0f) : bThr;
            l4 = first ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : bLi;
            // the last shadow ray's result exists only if the path cast one (a position nothing
            // wrote this batch holds a stale value; its lsr is 0 then, but it is not read)
            // (... or the last pass tested the ray itself: kFlagShadowResolved, set only if occluded)
            shadowHit = (flags & kFlagShadowResolved) != 0u || ((flags & kFlagShadowPending) != 0u && shRaw != 0u);
            flags &= ~(kFlagFirst | kFlagShadowPending | kFlagShadowResolved);
        }
        F3 li{l4.x, l4.y, l4.z};
        {
            // CONTROL's Li += light sampling result (:520-528), done here for live paths (a
            // path without a shadow ray carries lsr = 0: Li + 0 either way)
            const F3 lsr0{l4.w, l2.x, l2.y};
            li.x = li.x + (!shadowHit ? lsr0.x : 0.0f);
            li.y = li.y + (!shadowHit ? lsr0.y : 0.0f);
            li.z = li.z + (!shadowHit ? lsr0.z : 0.0f);
        }
        // the slot index as a fresh value for the stores below: their addresses are then
        // formed where they are used instead of being shared with the loads' and kept
        // live in VGPR pairs across the whole shading code
        uint32_t out = path;
        asm volatile("" : "+v"(out));
        float extOpacity = 0.0f, shadowOpacity = 0.0f;
        V3 T, L, lsr;
        DCRT_MCLK(0);
        shade_path<CAPS, SCENE_LDS == 1 && !caps_any_scene(CAPS)>(sc, fcv, hit, dir, rng, flags, thr, li, T, L, lsr, terminate, hasShadow, nO, nD, sO, sD,
                         extOpacity, shadowOpacity DCRT_MCLK_ARGS);
        DCRT_MCLK(4);
        if (fcv.features & DCRT_FEATURE_ALLOW_ANYHIT) {   // :422-430
            if (!terminate) slot(pool.extOpacity, out) = extOpacity;
            if (hasShadow) slot(pool.shadowOpacity, out) = shadowOpacity;
        }
        ends = terminate && !hasShadow;
        // EARLY: the path continues, but its next bounce is past the last one shaded. The pass after
        // that ray would add no radiance (this variant's scenes have no light a ray can reach) and
        // only complete the path, which CONTROL does from a finish record; so the path finishes here,
        // and its ray -- cast all the same -- takes the last-ray queue: no state, no hit record.
        // (sc.earlyFinish 2, a test value: odd path slots go the long way, so a wave holds both routes.)
        if constexpr (EARLY) {
            const uint32_t mode = sc.earlyFinish;
            last = !terminate && (flags & 0xFFu) > fcv.maxBounce && mode != 0u && (mode != 2u || (path & 1u) == 0u) &&
                   (fcv.features & DCRT_FEATURE_ALLOW_ANYHIT) == 0u;
        }
        // the row-cost probe (PROBE: the variant dcrt_tracer_set_row_cost_probe launches): the rays
        // of this pass per film row -- the extension ray this item shades and the shadow ray it
        // casts -- for cost-balanced film bands (partition.balanced_bands)
        if constexpr (PROBE) {
            uint32_t* rowRays = sampleOut->rowRays;
            const uint32_t p = virt ? newPixel : slot(pool.pixel, out);
            const uint32_t W = fcv.resolution[0], wh = W * fcv.resolution[1];
            atomicAdd(&rowRays[(p % wh) / W], hasShadow ? 2u : 1u);
        }
        // (the state written below goes to the queue positions the appends return)
        pathFlags = flags;
        sThr = thr;
        sT = T;
        sL = L;
        sLsr = lsr;
        sRng = make_uint4(rng.s0, rng.s1, rng.s2, rng.s3);
        if (ends || terminate || last) {
            // The path ends here with no shadow ray pending: all CONTROL would still do is
            // Li += light sampling result (0: the same bits as L + 0.0f) and WriteSample
            // (RayTracingCommon.inc.hlsl:118-122), so both happen in this pass and the slot
            // goes idle at once. (A path ending WITH a shadow ray pending goes to the finish
            // queue; CONTROL completes it. Its debug RNG state, final now, is stored here.)
            // The pixel is loaded here and the sample stored after the queue appends, whose
            // atomic round trip hides the load.
            const SampleOut so = *sampleOut;
            if (ends || last || so.debugRng) pix = slot(pool.pixel, out);
            if (ends || last) {
                // (a path finished at its last shaded bounce: the sample of the pass that would have ended
                // it, should this pass turn out to know its shadow ray's result -- `done` below)
                sample = make_float4(L.x + 0.0f, L.y + 0.0f, L.z + 0.0f, 0.0f);
                // the sample pointers are read here too, not after the appends: read there
                // (behind the barriers and the atomic) they were one more round trip
                outPos = so.samplePosition;
                outVal = so.sampleValue;
            }
            if (so.debugRng) sample_at(so.debugRng, pix) = make_uint4(rng.s0, rng.s1, rng.s2, rng.s3);
        }
    }
    // FUSED: the shadow ray's occlusion bit here, after the shading (its temporaries are dead), from
    // the ray still in registers; `queued`: the rays that take the shadow queue
    bool inlined = false, occluded = false;
    if constexpr (FUSED) {
        const V3 sInv = inv_dir(sD);
        inlined = active && hasShadow && cells_finite(sInv) && (path & fcv.shadowInlineMask) == 0u;
        if (inlined)
            occluded = cells_occluded_cached(si.cells, si.res, mk(sO.x, sO.y, sO.z), sD, sO.w, sInv,
                                             (fcv.features & DCRT_FEATURE_WATERTIGHT) != 0, cellNodes, cellTris, cellLeaves);
        inlineRays += (uint32_t)__popcll(__ballot(inlined));
    }
    const bool queued = active && hasShadow && !inlined;
    DCRT_MCLK(5);
    uint32_t es, ss;
    // (paths ended with a shadow ray pending: the next CONTROL pass completes them)
    // A path finished at its last shaded bounce whose shadow ray's result is known here (tested above, or
    // none cast) is complete: the pass that would have ended it computes (Li + lsr unless occluded) + 0 and
    // writes that sample, so this pass does, and no list holds the path. One whose shadow ray took the
    // queue goes to the finish queue, as a path that ends with its shadow ray pending does.
    const bool done = last && (!hasShadow || inlined);
    if (done) {
        sample.x = (sL.x + (!occluded ? sLsr.x : 0.0f)) + 0.0f;
        sample.y = (sL.y + (!occluded ? sLsr.y : 0.0f)) + 0.0f;
        sample.z = (sL.z + (!occluded ? sLsr.z : 0.0f)) + 0.0f;
    }
    const bool fin = active && ((terminate && hasShadow) || (last && !done));
    uint32_t fb;
    // The last rays' positions: one atomic per wave that has some (with the count of the paths completed
    // here in its upper half), issued ahead of the workgroup's three so that all four round trips overlap
    // (such waves come in one iteration of a batch's maxBounce + 2, and the append's LDS words stay as they are)
    uint32_t lastBase = 0u, lastRank = 0u;
    if constexpr (EARLY) {
        const unsigned long long lm = __ballot(last);
        if (lm != 0ull) {
            lastRank = __builtin_amdgcn_mbcnt_hi((uint32_t)(lm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)lm, 0u));
            const unsigned long long both = (unsigned long long)__popcll(lm) | ((unsigned long long)__popcll(__ballot(done)) << 32);
            if ((threadIdx.x & 63u) == 0u) lastBase = (uint32_t)atomicAdd(last_ctr(cnt, shard), both);
        }
    }
    block_append3(active && !terminate && !last, qctr(cnt, kQExt, shard), queued, qctr(cnt, kQShadow, shard),
                  fin, qctr(cnt, kQFinish, fshard), sm + (round & 1u) * 48u, &es, &ss, &fb);
    DCRT_MCLK(6);
    if constexpr (EARLY) lastBase = (uint32_t)__builtin_amdgcn_readfirstlane((int)lastBase);
    const uint32_t qNext = shard * pool.recCap + es;           // the continuing path's records
    const uint32_t fPos = fshard * pool.finCap + fb;           // a finishing path's record
    // An ended path's sample (and its slot's idle flag) is stored before the records: its
    // address needs the pixel load, and vmcnt counts loads and stores in issue order, so a
    // wait for the pixel issued after the record stores waited for all of them too. The empty
    // asm takes the pixel in every wave (whether or not one of its paths ended), so that wait
    // is placed here, ahead of every store, and not where the pixel's register is next reused.
    asm volatile("" ::"v"(pix));
    if (ends || done) {
        store_global(outPos, pix, pixel_sample(fcv, pix));
        store_global(outVal, pix, sample);
        // (done: idle for the scans from the iteration after next on, as after the pass that would have
        // ended the path -- kFlagIdleFrom)
        slot(pool.flags, path) = done ? doneFlag : kFlagIdle;
    }
    if (last) {
        // the last ray's record alone, from the end of the shard's records downwards
        float4* r = ext_rec(pool.extRec, shard * pool.recCap + (pool.recCap - 1u - (lastBase + lastRank)));
        r[0] = make_float4(nO.x, nO.y, nO.z, 0.0f);
        r[1] = make_float4(nD.x, nD.y, nD.z, asf(path));
    }
    if (active && !terminate && !last) {
        float4* r = ext_rec(pool.extRec, qNext);
        r[0] = make_float4(nO.x, nO.y, nO.z, 0.0f);
        r[1] = make_float4(nD.x, nD.y, nD.z, asf(path));
        PathStateA& st = state_at(pool.stateA, qNext);
        PathStateB& stB = state_at(pool.stateB, qNext);
        st.rng = sRng;
        stB.thr = make_float4(sT.x, sT.y, sT.z, sThr.w);
        stB.liLsr = make_float4(sL.x, sL.y, sL.z, sLsr.x);
        st.lsrMisc = make_float4(sLsr.y, sLsr.z, asf(pathFlags | (queued ? kFlagShadowPending : 0u) | (occluded ? kFlagShadowResolved : 0u)), asf(path));
    }
    if (fin) {
        FinishRec& fr = pool.finRec[fPos];
        fr.liLsr = make_float4(sL.x, sL.y, sL.z, sLsr.x);
        fr.lsrSlot = make_float4(sLsr.y, sLsr.z, asf(path), asf(last ? kFinishEarly : 0u));
        // (the result CONTROL reads beside it: the cast writes a queued ray's)
        if (inlined) pool.finHit[fPos] = occluded ? 1u : 0u;
    }
    if (queued) {
        const uint32_t sq = shard * pool.recCap + ss;
        float4* r = ext_rec(pool.shRec, sq);
        r[0] = sO;
        // where the shadow cast writes the result: the continuing path's next state, or its
        // finish record
        r[1] = make_float4(sD.x, sD.y, sD.z, asf(terminate || last ? (fPos | kDestFinish) : qNext));
        // the path slot beside it: only ALLOW_ANYHIT_SHADER's cast reads it (the shadow ray's
        // opacity sample is per slot)
        if (fcv.features & DCRT_FEATURE_ALLOW_ANYHIT) slot(pool.shadowQueue, sq) = path;
    }
    DCRT_MCLK(2);
    ++round;
    }
    if constexpr (FUSED) {
        // shadow_rays counts every shadow ray: the ones tested here, one add per workgroup
        if ((threadIdx.x & 63u) == 0u && inlineRays) atomicAdd(&inlineTotal, inlineRays);
        __syncthreads();
        if (threadIdx.x == 0 && inlineTotal) atomicAdd(&cnt->w[(kInlineShadowWord + shard) * kShardStride], inlineTotal);
    }
    DCRT_MCLK_FLUSH(itemsDone);
    (void)itemsDone;
}

// Cast-kernel occupancy: 5 waves per SIMD (<= 96 VGPRs; the compiler alone takes ~99,
// i.e. 4 waves). Measured on the 1080p Cornell bench, one pipeline: 4 waves 5.51,
// 5 waves 5.46, 6 waves 5.37, 7 waves 5.77 (spills), 8 waves 7.19 ms/spp; with the
// two concurrent pipelines of the default bench 5 waves leave the other pipeline's
// kernels room on the CU: 4.60 vs 4.66 ms/spp at 6 (3 repeats, tools/ab_libs.sh),
// although a lone launch is 3 % slower (106 vs 102.5 us).
#ifndef DCRT_CAST_WAVES_PER_EU
#define DCRT_CAST_WAVES_PER_EU 5
#endif
#if DCRT_CAST_WAVES_PER_EU > 0
#define DCRT_CAST_OCCUPANCY __attribute__((amdgpu_waves_per_eu(DCRT_CAST_WAVES_PER_EU, 8)))
#else
#define DCRT_CAST_OCCUPANCY
#endif
// The cache-only cast variant: 7 waves/SIMD (72 VGPRs, no spills; 6 waves at 74 VGPRs
// before the per-leaf shear: 2.96 vs 3.03 ms/spp, three A/B passes)
#ifndef DCRT_CACHED_CAST_WAVES_PER_EU
#define DCRT_CACHED_CAST_WAVES_PER_EU 7
#endif

// ---- EXTENSION_RAY_CAST / SHADOW_RAY_CAST ----------------------------------------------
// Persistent while-while loop with per-lane dynamic fetch: wave w owns items
// [w*chunk, (w+1)*chunk) of the queue; every step, lanes whose ray finished take
// the next items of the wave's range (ballot + mbcnt, no atomics), so all 64
// lanes keep traversing until the range is drained.

// log2(blockDim.x): traversal kernels run power-of-two workgroups (tracer.hip)
__device__ __forceinline__ uint32_t block_shift() { return 31u - (uint32_t)__clz((int)blockDim.x); }

#ifndef DCRT_VISITS_PER_CHECK
#define DCRT_VISITS_PER_CHECK 3
#endif
// node visits between two wave-level checks of the phase-A exit condition
constexpr int kVisitsPerCheck = DCRT_VISITS_PER_CHECK;
#ifndef DCRT_INTERLEAVE
#define DCRT_INTERLEAVE 64
#endif
// queue items per round-robin group of the cast kernels' static work split (power of two)
constexpr uint32_t kInterleave = DCRT_INTERLEAVE;
// PAIR (persistent_trace): phase A steps with trav_visit_pair instead of trav_visit. The
// tracer takes it for scenes whose nodes + triangles exceed an XCD's L2 (latency-bound
// fetches: spaceship 2.50 -> 2.46 ms/spp); on L2-resident scenes the second box test per
// step costs more than the shorter fetch chain saves (coffee 2.92 -> 3.02, lamp 7.21 ->
// 7.48). The test / megakernel paths always use it (the GPU parity tests cover it on every
// scene).

#ifdef DCRT_WAVE_TIMELINE
// Diagnostic build only (tools/wave_timeline.py): per-wave start/end realtime stamps
// and item counts of the cast kernels, 16 iteration slots x 8192 waves x 2 kernels.
__device__ unsigned long long g_waveLog[2][16][8192][2];
__device__ uint32_t g_waveItems[2][16][8192];
#define DCRT_WAVE_TAG(g) ((int)((g)->iterations & 15ull))
#else
#define DCRT_WAVE_TAG(g) (-1)
#endif


constexpr uint32_t kNoItem = 0xFFFFFFFFu;   // a fetch's "no ray for this item"
constexpr uint32_t kLastItem = 0xFFFFFFFEu;   // a closest-hit fetch's "a last ray: traced, no result wanted" (kLastRayWord)
#ifndef DCRT_INLINE_ENTRY
#define DCRT_INLINE_ENTRY 1   // identity-instance BLAS entries in phase A (trav_visit ENTER)
#endif

// RING stacks: the lane's LDS stack is a window of sc.ringRows entries (dscene.h stack_row) over
// a per-lane global column (sc.spill). Before every batch of kVisitsPerCheck node visits the wave
// checks that each lane's window can take the batch: a visit writes the row above its top (push or
// not), so the window must hold at most ringRows - 1 entries before each visit, i.e. at most
// ringRows - kVisitsPerCheck before the batch; and a visit (or the following leaf work) pops at most one entry,
// so with entries spilled below the window it must hold at least kVisitsPerCheck + 1. A lane
// outside those bounds moves entries between the window and its spill column until the window
// holds ringRows / 2 (or every entry); the host keeps ringRows >= 2 * (kVisitsPerCheck + 1), so
// that window passes both checks (kMinRingRows). The entries' values and order are untouched: traversal,
// hits and counts are those of the whole-stack kernels bit for bit.
constexpr uint32_t kMinRingRows = 2u * ((uint32_t)kVisitsPerCheck + 1u);
template <bool RING>
__device__ __forceinline__ void ring_maintain(const DeviceScene& sc, TravState& s, bool active, uint32_t* lds, uint32_t shift)
{
    if constexpr (RING) {
        const uint32_t stride = 4u << shift;
        const uint32_t live = s.sp - s.base;
        const bool spill = active && live > (sc.ringRows - (uint32_t)kVisitsPerCheck) * stride;
        const bool fill = active && s.base != 0u && live <= (uint32_t)kVisitsPerCheck * stride;
        if (__builtin_expect(__ballot(spill | fill) != 0ull, 0)) {
            const uint32_t lanes = gridDim.x * blockDim.x;
            uint32_t* col = sc.spill + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
            const uint32_t half = (sc.ringRows >> 1) * stride;
            const uint32_t target = s.sp > half ? s.sp - half : 0u;   // the new base
            if (spill) {
                // positions base + 1 .. target go to the column (entry e at col[(e - 1) * lanes])
                for (uint32_t p = s.base + stride; p <= target; p += stride)
                    col[(size_t)((p >> (shift + 2u)) - 1u) * lanes] = stack_at(lds, stack_row<true>(sc, p, shift));
                s.base = target;
            } else if (fill) {
                // positions target + 1 .. base come back into the window
                for (uint32_t p = target + stride; p <= s.base; p += stride)
                    stack_at(lds, stack_row<true>(sc, p, shift)) = col[(size_t)((p >> (shift + 2u)) - 1u) * lanes];
                s.base = target;
            }
        }
    }
}

template <bool ANY_HIT, bool INSTR, bool OPACITY, bool LANE_ANY = false, bool ALL_CACHED = false, bool PAIR = false,
          int LAYOUT = kLayoutScene, bool IDENT = false, bool RING = false, bool FLAT = false, typename Lookup, typename Fetch,
          typename Emit>
__device__ __forceinline__ void persistent_trace(const DeviceScene& sc, uint32_t n, uint32_t features, uint32_t kRefillLanes,
                                                 uint32_t kParkLanes, uint32_t* lds, uint32_t shift, Lookup lookup, Fetch fetch,
                                                 Emit emit, TraversalStats& st, int waveTag = -1)
{
    const bool watertight = (features & DCRT_FEATURE_WATERTIGHT) != 0;
    const bool f2b = (features & DCRT_FEATURE_NO_FRONT_TO_BACK) == 0;
    const uint32_t wavesPerBlock = blockDim.x >> 6;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves = gridDim.x * wavesPerBlock;
    const uint32_t waveId = blockIdx.x * wavesPerBlock + (threadIdx.x >> 6);
    // Work split: the queue is cut into groups of kInterleave consecutive items (one
    // region of the image / one producer workgroup each) dealt round-robin to the
    // waves, so every wave samples the whole queue and per-wave costs even out
    // (contiguous ranges follow the image's cost structure and leave the slowest
    // waves alone at the end). `cursor` and `end` count in the wave's own sequence.
    // A sparse queue (an image's drain: a few thousand long rays) is cut into smaller groups
    // -- the largest power of two <= n / (4 * waves), at least 1 -- so every wave gets some of
    // it: with 64-item groups the rays sat 64 to a wave on a few dozen waves (a handful of
    // CUs), and each of those waves took as long as its slowest lane plus every other lane's
    // leaf work. (At least 4 groups per wave keep the per-wave item counts within 5/4 of
    // each other.)
#ifndef DCRT_ADAPTIVE_GROUPS
#define DCRT_ADAPTIVE_GROUPS 1
#endif
    constexpr uint32_t kLgInterleave = 31u - __builtin_clz(kInterleave);
    const uint32_t perWave4 = n / (4u * waves);
    const uint32_t lg = !DCRT_ADAPTIVE_GROUPS || perWave4 >= kInterleave ? kLgInterleave : (perWave4 ? 31u - (uint32_t)__clz((int)perWave4) : 0u);
    const uint32_t gmask = (1u << lg) - 1u;
    const uint32_t groups = (n + gmask) >> lg;
    const uint32_t myGroups = groups > waveId ? (groups - waveId + waves - 1) / waves : 0u;
    uint32_t cursor = 0;
    const uint32_t end = myGroups << lg;
    const uint32_t chunk = end;   // (diagnostics)
    // (24-bit multiply: a 32-bit a * b + c becomes v_mad_u64_u32 with an arbitrary VGPR as
    // the unused high addend, which made the refill wait for the window's pending load)
    auto itemIndex = [&](uint32_t k) { return ((waveId + __umul24(k >> lg, waves)) << lg) + (k & gmask); };
    // lookup(i) is arithmetic only (a ray's record position in its queue): a refill waits for
    // the ray loads alone (the earlier 4-B queue entries needed a prefetch window of lookups
    // one refill ahead, a bpermute and a register)
    TravState s;
    // lane state, one integer (per-lane bools cost mask <-> register conversions per step):
    // kIdle no ray; kRun visiting nodes; kPark at a leaf (phase B work pending); kFin ray
    // finished, its result not yet written
    constexpr uint32_t kIdle = 0, kRun = 1, kPark = 2, kFin = 3;
    uint32_t ls = kIdle;
    uint32_t item = 0;
#ifdef DCRT_WAVE_TIMELINE
    const unsigned long long tStart = wall_clock64();
#endif
    DCRT_PHASE_INIT;
    for (;;) {
        DCRT_PHASE_COUNT(3);
        // refill only when at least kRefillLanes lanes are idle: the fetch (ray loads,
        // three IEEE divisions) is then shared by many lanes
        const bool free = ls == kIdle || ls == kFin;
        const unsigned long long need = __ballot(free);
        const uint32_t nNeed = (uint32_t)__popcll(need);
        const bool refill = nNeed >= kRefillLanes && cursor < end;
        const uint32_t k = cursor + __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
        // Finished rays are written here, just before the ray loads (stores count in vmcnt
        // too: the loads are then not queued behind older stores' acknowledgements twice).
        if (ls == kFin) {
            emit(item, s);
            ls = kIdle;
        }
        if (refill) {
            const uint32_t idx = itemIndex(k);
            if (free && k < end && idx < n) {
                item = fetch(idx, lookup(idx), s);
                if (!f2b) s.negMask = 0u;
                if constexpr (!INSTR && !PAIR && !RING && !OPACITY) {
                    if (sc.skipRoot && item != kNoItem) trav_skip_root<ALL_CACHED, LAYOUT, IDENT>(sc, s, lds, shift);
                } else if constexpr (!INSTR && PAIR && !ALL_CACHED && !OPACITY) {
                    if (sc.skipRoot && item != kNoItem) trav_skip_root_pair(sc, s, lds, shift);
                }
                // (kNoItem: the queue item has no ray -- a hole of a virtual batch start)
                ls = item != kNoItem ? kRun : kIdle;
            }
            cursor += min(nNeed, end - cursor);
        }
        DCRT_PHASE(0);
        if (__ballot(ls != kIdle) == 0ull) break;
        // phase A: node visits only, until enough lanes are parked at leaves (or
        // enough are idle to refill, or none can advance)
        // (a lane whose ray ends here only flags it: the result is written at the next
        // refill point, which keeps the stores out of the unrolled visit steps)
        for (;;) {
            ring_maintain<RING>(sc, s, ls == kRun || ls == kPark, lds, shift);
#pragma unroll
            for (int k = 0; k < kVisitsPerCheck; ++k) {
                if (ls == kRun) {
                    const bool fin = PAIR && !INSTR && !ALL_CACHED ? trav_visit_pair<false, LAYOUT, RING>(sc, s, lds, shift)
                                                                   : trav_visit<INSTR, ALL_CACHED, LAYOUT, !FLAT && (ALL_CACHED || IDENT) && !OPACITY && DCRT_INLINE_ENTRY, IDENT, RING>(sc, s, lds, shift, st);
                    if (fin) ls = kFin;
                    else if (s.parked) ls = kPark;
                }
            }
            const unsigned long long runnable = __ballot(ls == kRun);
            const uint32_t parked = (uint32_t)__popcll(__ballot(ls == kPark));
            const uint32_t idle = 64u - (uint32_t)__popcll(runnable) - parked;
            DCRT_PHASE_COUNT(4);
#ifndef DCRT_ADAPTIVE_PARK
#define DCRT_ADAPTIVE_PARK 1
#endif
#ifndef DCRT_PARK_EIGHTHS
#define DCRT_PARK_EIGHTHS 4
#endif
            // leaf work once kParkLanes lanes wait at leaves -- or half of the wave's rays, when
            // it holds few (a drain's sparse waves: a lane parked at a leaf would otherwise wait
            // for every other ray to reach one)
            const uint32_t parkAt = DCRT_ADAPTIVE_PARK ? min(kParkLanes, max(1u, ((64u - idle) * DCRT_PARK_EIGHTHS) >> 3)) : kParkLanes;
            if (runnable == 0ull || parked >= parkAt || (idle >= kRefillLanes && cursor < end)) break;
        }
        DCRT_PHASE(1);
        // phase B: the parked lanes' leaf work, shared by many lanes at once
        if (__ballot(ls == kPark) != 0ull) DCRT_PHASE_COUNT(5);
        if (ls == kPark)
            ls = trav_leaf<ANY_HIT, INSTR, OPACITY, LANE_ANY, ALL_CACHED, IDENT, RING, FLAT>(sc, s, watertight, lds, shift, st) ? kFin : kRun;
        DCRT_PHASE(2);
    }
    DCRT_PHASE_FLUSH();
#ifdef DCRT_WAVE_TIMELINE
    if (waveTag >= 0 && n > 0 && (threadIdx.x & 63u) == 0 && waveId < 8192) {
        g_waveLog[ANY_HIT ? 1 : 0][waveTag & 15][waveId][0] = tStart;
        g_waveLog[ANY_HIT ? 1 : 0][waveTag & 15][waveId][1] = wall_clock64();
        g_waveItems[ANY_HIT ? 1 : 0][waveTag & 15][waveId] = chunk;
    }
#endif
}

// Kernel arguments the cast kernels select between per lane (extension vs shadow ray):
// pinned in SGPRs, so the select is a v_cndmask of two values and not a per-lane load
// of the pointer from the kernel-argument segment in front of every ray fetch.
// (The asm takes the pointer in the global address space and the result is cast back,
// so the loads through it stay global_load, not FLAT; the host pass only parses it.)
template <typename T>
__device__ __forceinline__ T* sgpr_ptr(T* p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __attribute__((address_space(1))) T* g = (__attribute__((address_space(1))) T*)p;
    asm volatile("" : "+s"(g));
    return (T*)g;
#else
    return p;
#endif
}

__device__ __forceinline__ void flush_stats(const TraversalStats& st, unsigned long long* dst)
{
    const unsigned long long a = wave_sum(st.nodes), b = wave_sum(st.tris), c = wave_sum(st.blas);
    if ((threadIdx.x & 63u) == 0 && (a | b | c)) { atomicAdd(&dst[0], a); atomicAdd(&dst[1], b); atomicAdd(&dst[2], c); }
}

// the wave's largest value into *dst (the longest ray's node visits)
__device__ __forceinline__ void flush_max(uint32_t v, unsigned long long* dst)
{
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
    if ((threadIdx.x & 63u) == 0 && v) atomicMax(dst, (unsigned long long)v);
}

// The extension cast's result at the ray's queue item: the hit and, for MATERIAL, the
// ray's direction and instance (so MATERIAL reads nothing of the ray record)
__device__ __forceinline__ void emit_hit(const PathPool& pool, uint32_t item, const TravState& s)
{
    float4* h = pool.hit + 2 * (size_t)item;
    h[0] = s.found ? make_float4(s.hit.t, s.hit.u, s.hit.v, asf(s.hit.tri)) : make_float4(inf(), 0.0f, 0.0f, 0.0f);
    h[1] = make_float4(s.d.x, s.d.y, s.d.z, asf(s.found ? s.hit.inst : 0u));
}
// The shadow cast's result where MATERIAL asked for it: the continuing path's next
// extension-queue position, or its finish-queue position (kDestFinish)
__device__ __forceinline__ void emit_occlusion(const PathPool& pool, uint32_t dest, bool found)
{
    uint32_t* dst = (dest & kDestFinish) ? pool.finHit : pool.shadowHit;
    dst[dest & ~kDestFinish] = found ? 1u : 0u;
}
__device__ __forceinline__ void emit_occlusion(const PathPool& pool, uint32_t dest, const TravState& s) { emit_occlusion(pool, dest, s.found); }

// OPACITY: the ALLOW_ANYHIT_SHADER variant (a separate instantiation, so the default
// kernels carry none of its state).
template <bool INSTR, bool OPACITY>
__global__ __launch_bounds__(256) DCRT_CAST_OCCUPANCY void extension_kernel(PathPool pool, DeviceScene sc, const FrameConstants* __restrict__ fc, const Counters* cnt,
                                                         Globals* g, unsigned long long* instr)
{
    extern __shared__ uint32_t stackMem[];
    scene_cache_load(sc, stackMem, block_shift());
    QueueMap qm;
    qmap(cnt, kQExt, &qm);
    const uint32_t nExt = qm.prefix[kShards];
    TraversalStats st = {};
    // (the last rays behind the extension queue's: traced alike, nothing written for them)
    persistent_trace<false, INSTR, OPACITY>(
        sc, nExt + last_total(cnt), fc->features, fc->refillLanes, fc->parkLanes, stackMem + threadIdx.x, block_shift(),
        [&](uint32_t i) __attribute__((always_inline)) { return i >= nExt ? last_pos(cnt, pool.recCap, i - nExt) : qpos(pool.recCap, qm, i); },
        [&](uint32_t i, uint32_t q, TravState& s) __attribute__((always_inline)) {
            const float4* r = ext_rec((const float4*)pool.extRec, q);
            const float4 o = r[0], d = r[1];
            trav_init(s, mk(o.x, o.y, o.z), mk(d.x, d.y, d.z), 0.0f, inf());
            if (OPACITY) s.opacitySample = pool.extOpacity[asu(d.w) & ~kEntryFirst];
            return i >= nExt ? kLastItem : i;   // the result goes to the ray's queue item
        },
        [&](uint32_t item, const TravState& s) __attribute__((always_inline)) { if (item != kLastItem) emit_hit(pool, item, s); },
        st, DCRT_WAVE_TAG(g));
    if (INSTR) flush_stats(st, instr);
    (void)g;
}

// End of an iteration (after both casts): account it and clear the other parity's counters.
__device__ __forceinline__ void end_iteration(const Counters* cnt, Counters* nextCnt, Globals* g, uint32_t shadowRays)
{
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) {
#if defined(__HIP_DEVICE_COMPILE__)
            // (the counters through a pointer the compiler takes as new here: their scalar loads stay in this
            // block, not hoisted to the kernel's entry and held -- spilled -- across the whole traversal loop)
            asm volatile("" : "+s"(cnt));
#endif
            uint32_t fin = 0;
            for (uint32_t sh = 0; sh < kFinShards; ++sh) fin += qctr_load(cnt, kQFinish, sh);
            // (a virtual batch start's items: its cast counted the rays, holes excluded)
            const uint32_t virt = virtual_items(cnt);
            // (the last rays are extension rays like the queue's; their paths are in the finish list)
            // (`completed`: those whose paths MATERIAL completed itself -- in no list, live until the pass that
            // would have ended them)
            uint32_t lastRays, completed;
            last_totals(cnt, &lastRays, &completed);
            const uint32_t queued = virt ? virt : qtotal(cnt, kQExt);
            const uint32_t ext = queued + lastRays;
            if (!virt) g->extRays += ext;
            g->earlyFinished += lastRays;
            nextCnt->w[kEpochLine * kShardStride] = epoch_of(cnt) + 1u;
            // (with the rays MATERIAL's FUSED variant tested itself: they are in no queue)
            g->shadowRays += shadowRays + inline_shadow_rays(cnt);
            g->iterations += 1ull;
            g->staticFill = 0u;   // only a batch's first CONTROL pass claims statically
            // IsImageComplete (WavefrontPathTracer.cpp:508-523), exact and on the device: no
            // path was live entering this iteration (so CONTROL's scan saw every slot idle)
            // and none was started
            const bool idle = g->prevLive == 0u && ext == 0u;
            g->poolIdle = idle ? 1u : 0u;
            g->imageComplete = (idle && !g->stopped) ? 1u : 0u;
            g->prevLive = queued + fin + completed;   // (each live path once: the extension queue's, the finish list's, ...)
        }
        if (threadIdx.x < kCounterLines) nextCnt->w[threadIdx.x * kShardStride] = 0u;   // (with kVirtual/kDrainedWord, kInlineShadowWord, kLastRayWord)
        if (threadIdx.x < kShards) nextCnt->w[(kLastRayWord + threadIdx.x) * kShardStride + 1u] = 0u;   // (the last-ray lines' second words)
    }
}

template <bool INSTR, bool OPACITY>
__global__ __launch_bounds__(256) DCRT_CAST_OCCUPANCY void shadow_kernel(PathPool pool, DeviceScene sc, const FrameConstants* __restrict__ fc, Counters* cnt,
                                                      Counters* nextCnt, Globals* g, unsigned long long* instr)
{
    extern __shared__ uint32_t stackMem[];
    scene_cache_load(sc, stackMem, block_shift());
    QueueMap qm;
    qmap(cnt, kQShadow, &qm);
    const uint32_t n = qm.prefix[kShards];
    TraversalStats st = {};
    persistent_trace<true, INSTR, OPACITY>(
        sc, n, fc->features, fc->refillLanes, fc->parkLanes, stackMem + threadIdx.x, block_shift(),
        [&](uint32_t i) __attribute__((always_inline)) { return qpos(pool.recCap, qm, i); },
        [&](uint32_t i, uint32_t q, TravState& s) __attribute__((always_inline)) {
            const float4* r = ext_rec((const float4*)pool.shRec, q);
            const float4 o = r[0], d = r[1];
            trav_init(s, mk(o.x, o.y, o.z), mk(d.x, d.y, d.z), 0.0f, o.w);
            if (OPACITY) s.opacitySample = pool.shadowOpacity[slot(pool.shadowQueue, q)];
            return asu(d.w);   // the result's destination (MATERIAL's kDestFinish code)
        },
        [&](uint32_t dest, const TravState& s) __attribute__((always_inline)) { emit_occlusion(pool, dest, s); },
        st, DCRT_WAVE_TAG(g));
    if (INSTR) flush_stats(st, instr + 3);
    end_iteration(cnt, nextCnt, g, n);
}

// EXTENSION_RAY_CAST + SHADOW_RAY_CAST in one persistent launch. The two queues are
// independent (MATERIAL filled both), so their items form one sequence (extension
// rays first) dealt to the waves like a single queue: one ramp and one drain per
// iteration instead of two, and a shadow ray can fill a lane an extension ray left
// idle. Per lane the ray keeps its own semantics (closest hit vs first hit), so the
// results are those of the two separate kernels.
// IDENT: the cache-only kernel of a scene whose instances all have the identity inverse
// (trav_visit): no instance-space ray, 8 waves/SIMD.
#ifndef DCRT_IDENT_CAST_WAVES_PER_EU
#define DCRT_IDENT_CAST_WAVES_PER_EU 8
#endif
// RING: the traversal stack as an LDS window over a per-lane global column (ring_maintain), for
// scenes whose whole stack would cost LDS occupancy (tracer.hip UploadScene).
// FLAT: the cache-only IDENT kernel over the entry-free node order (bvh_layout.h EntryFreeLayout)
// CELLS (with FLAT, a scene with a direction-cell table, shadow_cells.h): every wave first streams
// through its share of the shadow queue, one ray per lane, testing only the leaves of the ray's
// cell (cells_occluded: the reference's occlusion bit), then traces the extension queue alone
template <bool INSTR, bool OPACITY, bool ALL_CACHED, bool PAIR, bool IDENT = false, bool RING = false, bool FLAT = false,
          bool CELLS = false>
__global__ __launch_bounds__(256)
#ifndef DCRT_GLOBAL_CAST_WAVES_PER_EU
#define DCRT_GLOBAL_CAST_WAVES_PER_EU DCRT_CAST_WAVES_PER_EU   // (the global-memory, non-pair kernel; A/B)
#endif
__attribute__((amdgpu_waves_per_eu(ALL_CACHED && !OPACITY && !INSTR ? (IDENT ? DCRT_IDENT_CAST_WAVES_PER_EU : DCRT_CACHED_CAST_WAVES_PER_EU)
                                   : (!ALL_CACHED && !PAIR && !OPACITY && !INSTR ? DCRT_GLOBAL_CAST_WAVES_PER_EU : DCRT_CAST_WAVES_PER_EU), 8))) void cast_kernel(PathPool pool, DeviceScene sc, const FrameConstants* __restrict__ fc, Counters* cnt,
                                                                     Counters* nextCnt, Globals* g, unsigned long long* instr)
{
    extern __shared__ uint32_t stackMem[];
    static_assert(!CELLS || (FLAT && ALL_CACHED && IDENT && !INSTR && !OPACITY && !PAIR && !RING), "CELLS: the entry-free cache-only kernel");
    // (CELLS: the table's leaf words behind the scene cache, stored before its barrier)
    uint32_t* leafWords = (uint32_t*)(scene_cache(sc, stackMem, block_shift()) + sc.cachedNodes * 2u + sc.cachedTris * kRotTriFloat4);
    if (CELLS && threadIdx.x < kCellWords) leafWords[threadIdx.x] = sc.shadowLeaves[threadIdx.x];
    scene_cache_load<ALL_CACHED>(sc, stackMem, block_shift());
    QueueMap qe, qs;
    qmap(cnt, kQExt, &qe);
    qmap(cnt, kQShadow, &qs);
    // (the last rays, kLastRayWord: closest-hit items between the two queues' that emit nothing; nClosest: both)
    const uint32_t nExt = qe.prefix[kShards], nShadow = qs.prefix[kShards], nClosest = nExt + last_total(cnt);
    const uint32_t* shQueue = sgpr_ptr(pool.shadowQueue);
    const float4* extRec = sgpr_ptr((const float4*)pool.extRec);
    const float4* shRec = sgpr_ptr((const float4*)pool.shRec);
    TraversalStats st = {};
    TraversalStats stExt = {}, stShadow = {};
    constexpr int kLayout = PAIR ? kLayoutPairs : (!INSTR || ALL_CACHED ? kLayoutFlat : kLayoutScene);
    const uint32_t virt = !OPACITY ? virtual_items(cnt) : 0u;
    if (!OPACITY && virt) {
        // A virtual batch start (control_kernel): item i is path slot i; its camera ray is
        // (the branch costs no registers: 74 / 72 / 77 VGPRs as without it, tools/vgprs.sh)
        // NEW_PATH's (new_path<true>) from the slot's pixel, its hit goes to item i. (The
        // shadow queue is empty: the previous batch drained.) The rays traced are counted
        // here -- the queue's holes are not rays.
        const FrameConstants& f = *fc;
        const uint32_t* pixels = sgpr_ptr((const uint32_t*)pool.pixel);
        uint32_t rays = 0;
        persistent_trace<false, INSTR, OPACITY, true, ALL_CACHED, PAIR, kLayout, IDENT, RING, FLAT>(
            sc, virt, f.features, f.refillLanes, f.parkLanes, stackMem + threadIdx.x, block_shift(),
            [&](uint32_t i) __attribute__((always_inline)) { return i; },
            [&](uint32_t i, uint32_t v, TravState& s) __attribute__((always_inline)) {
                const uint32_t p = slot(pixels, v);
                if (p == kNoPixel) return kNoItem;
                V3 o, d;
                (void)new_path<true>(f, p, &o, &d);
                trav_init(s, o, d, 0.0f, inf());
                s.anyHit = false;
                if (INSTR) st = TraversalStats{};
                ++rays;
                return i;
            },
            [&](uint32_t item, const TravState& s) __attribute__((always_inline)) {
                emit_hit(pool, item, s);
                if (INSTR) {
                    stExt.nodes += st.nodes; stExt.tris += st.tris; stExt.blas += st.blas;
                    stExt.maxNodes = max(stExt.maxNodes, st.nodes);
                }
            },
            st, DCRT_WAVE_TAG(g));
        const unsigned long long r = wave_sum(rays);
        if ((threadIdx.x & 63u) == 0 && r) atomicAdd(&g->extRays, r);
    } else if constexpr (CELLS) {
        // The shadow queue, in the groups of 64 items the round-robin deal below hands out: a
        // plain loop, every lane busy (no stack, no refill hand-over, no parking)
        const uint32_t wavesPerBlock = blockDim.x >> 6, waves = gridDim.x * wavesPerBlock;
        const uint32_t waveId = blockIdx.x * wavesPerBlock + (threadIdx.x >> 6);
        const bool watertight = (fc->features & DCRT_FEATURE_WATERTIGHT) != 0;
        auto shadowSection = [&]() __attribute__((always_inline)) {
            for (uint32_t i = (waveId << 6) + (threadIdx.x & 63u); i < nShadow; i += waves << 6) {
                const float4* r = ext_rec(shRec, qpos(pool.recCap, qs, i));
                const float4 o = r[0], d = r[1];
                emit_occlusion(pool, asu(d.w), cells_occluded(sc, o, d, watertight, stackMem + threadIdx.x, block_shift(), leafWords));
            }
        };
#ifndef DCRT_CELLS_LAST
#define DCRT_CELLS_LAST 0   // (A/B: the shadow section after the extension rays)
#endif
        if (!DCRT_CELLS_LAST) shadowSection();
        persistent_trace<false, INSTR, OPACITY, false, ALL_CACHED, PAIR, kLayout, IDENT, RING, FLAT>(
            sc, nClosest, fc->features, fc->refillLanes, fc->parkLanes, stackMem + threadIdx.x, block_shift(),
            [&](uint32_t i) __attribute__((always_inline)) { return i >= nExt ? last_pos(cnt, pool.recCap, i - nExt) : qpos(pool.recCap, qe, i); },
            [&](uint32_t i, uint32_t v, TravState& s) __attribute__((always_inline)) {
                const float4* r = ext_rec(extRec, v);
                const float4 o = r[0], d = r[1];
                trav_init(s, mk(o.x, o.y, o.z), mk(d.x, d.y, d.z), 0.0f, inf());
                return i >= nExt ? kLastItem : i;   // the result goes to the ray's queue item; a last ray's nowhere
            },
            [&](uint32_t item, const TravState& s) __attribute__((always_inline)) { if (item != kLastItem) emit_hit(pool, item, s); },
            st, DCRT_WAVE_TAG(g));
        if (DCRT_CELLS_LAST) shadowSection();
    } else {
    // (node order: the pair kernels run on pair-ordered scenes, the other non-counting ones on
    // PackBVH-ordered ones -- tracer.hip's cast plan takes both from `pair` -- the counting ones on either)
    persistent_trace<false, INSTR, OPACITY, true, ALL_CACHED, PAIR, kLayout, IDENT, RING, FLAT>(
        sc, nClosest + nShadow, fc->features, fc->refillLanes, fc->parkLanes, stackMem + threadIdx.x, block_shift(),
        [&](uint32_t i) __attribute__((always_inline)) {
            // any kind: its record's position in its queue (no load)
            if (i >= nClosest) return qpos(pool.recCap, qs, i - nClosest);
            return i >= nExt ? last_pos(cnt, pool.recCap, i - nExt) : qpos(pool.recCap, qe, i);
        },
        [&](uint32_t i, uint32_t v, TravState& s) __attribute__((always_inline)) {
            const bool shadow = i >= nClosest;
            // the ray's 32-B record at its queue position v (32-bit byte offsets: the records
            // stay below 4 GiB, dcrt_tracer::Create); a shadow ray's path slot beside it
            const float4* r = ext_rec(shadow ? shRec : extRec, v);
            const float4 o = r[0], d = r[1];
            trav_init(s, mk(o.x, o.y, o.z), mk(d.x, d.y, d.z), 0.0f, shadow ? o.w : inf());
            s.anyHit = shadow;
            if (OPACITY) {
                const uint32_t path = shadow ? slot(shQueue, v) : asu(d.w);
                s.opacitySample = shadow ? pool.shadowOpacity[path] : pool.extOpacity[path];
            }
            if (INSTR) st = TraversalStats{};
            // an extension ray's result goes to its queue item, a shadow ray's to the
            // destination MATERIAL put in its record, a last ray's nowhere
            return shadow ? asu(d.w) : (i >= nExt ? kLastItem : i);
        },
        [&](uint32_t item, const TravState& s) __attribute__((always_inline)) {
            if (s.anyHit) emit_occlusion(pool, item, s);
            else if (item != kLastItem) emit_hit(pool, item, s);
            if (INSTR) {
                TraversalStats& dst = s.anyHit ? stShadow : stExt;
                dst.nodes += st.nodes; dst.tris += st.tris; dst.blas += st.blas;
                dst.maxNodes = max(dst.maxNodes, st.nodes);
#ifdef DCRT_PHASE_CLOCKS
                dst.cached += st.cached; dst.deep4 += st.deep4; dst.deep8 += st.deep8; dst.deep12 += st.deep12;
#endif
            }
        },
        st, DCRT_WAVE_TAG(g));
    }
    if (INSTR) {
        flush_stats(stExt, instr);
        flush_stats(stShadow, instr + 3);
        flush_max(stExt.maxNodes, instr + 6);
        flush_max(stShadow.maxNodes, instr + 7);
    }
#ifdef DCRT_PHASE_CLOCKS
    if (INSTR) {
        const unsigned long long c = wave_sum(stExt.cached + stShadow.cached), d4 = wave_sum(stExt.deep4 + stShadow.deep4),
                                 d8 = wave_sum(stExt.deep8 + stShadow.deep8), d12 = wave_sum(stExt.deep12 + stShadow.deep12);
        if ((threadIdx.x & 63u) == 0) {
            atomicAdd(&g_phaseClk[16], c); atomicAdd(&g_phaseClk[17], d4); atomicAdd(&g_phaseClk[18], d8); atomicAdd(&g_phaseClk[19], d12);
        }
    }
#endif
    end_iteration(cnt, nextCnt, g, nShadow);
}

// ---- GPU megakernel (MegakernelPathTracing.hlsl:65-208) -------------------------------------
// One lane traces one pixel's whole path; a fully finished wave claims the next 8x8
// pixel block (same per-shard cursors as CONTROL). Shares every device function with
// the wavefront kernels; differs from them only in the bounce-0 triangle-light
// emission, exactly like the reference's two tracers.
template <bool ANY_HIT, bool OPACITY>
__device__ __forceinline__ bool trace_full(const DeviceScene& sc, V3 o, V3 d, float tMax, bool watertight, bool f2b,
                                           float opacitySample, uint32_t* lds, uint32_t shift, HitRecord* hit)
{
    TravState s;
    trav_init(s, o, d, 0.0f, tMax, f2b);
    s.opacitySample = opacitySample;
    TraversalStats st = {};
    for (;;) {
        if (trav_visit_pair(sc, s, lds, shift)) break;
        if (s.parked && trav_leaf<ANY_HIT, false, OPACITY>(sc, s, watertight, lds, shift, st)) break;
    }
    *hit = s.hit;
    return s.found;
}

// CAPS: kCapAll, kCapAllEnvImportance where the environment cube is sampled by its table, or kCapAllLightTable
// where lights are picked by the light table (and the cube by its table, if one stands)
template <bool OPACITY, uint32_t CAPS = kCapAll>
__global__ __launch_bounds__(256) void megakernel(DeviceScene sc, const FrameConstants* __restrict__ fcp, Film film, Globals* g, uint32_t debugRng)
{
    extern __shared__ uint32_t stackMem[];
    scene_cache_load(sc, stackMem, block_shift());
    __shared__ uint32_t sm[64];
    const FrameConstants& fc = *fcp;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t shard = blockIdx.x % kShards;
    uint32_t* cursor = &g->nextBlock[shard * kShardStride];
    const uint32_t shardBlocks = g->totalBlocks > shard ? (g->totalBlocks - shard + kShards - 1) / kShards : 0u;
    const bool watertight = (fc.features & DCRT_FEATURE_WATERTIGHT) != 0;
    const bool f2b = (fc.features & DCRT_FEATURE_NO_FRONT_TO_BACK) == 0;
    const bool vndf = (fc.features & DCRT_FEATURE_GGX_SAMPLE_VNDF) != 0;
    const bool lightVisible = (fc.features & DCRT_FEATURE_LIGHT_VISIBLE) != 0;
    uint32_t* lds = stackMem + threadIdx.x;
    const uint32_t shift = block_shift();
    unsigned long long extRays = 0, shadowRays = 0;
    for (;;) {
        // every wave of the block claims one block per round (one atomic per workgroup)
        bool want = false;
        if (lane == 0) want = __hip_atomic_load(cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < shardBlocks;
        const uint32_t bslot = block_append(want, cursor, sm);
        const uint32_t claimed = (uint32_t)__shfl((int)bslot, 0, 64);
        const bool got = __shfl((int)want, 0, 64) != 0 && claimed < shardBlocks;
        if (__syncthreads_or(got ? 1 : 0) == 0) break;
        if (!got) continue;
        const uint32_t block = shard + claimed * kShards;
        uint32_t px = 0, py = 0, image = 0;
        if (!block_pixel(fc, film, block, lane, &px, &py, &image)) continue;
        Rng rng = rng_init(px, py, image_seed(fc, image));
        const float psx = next1(rng), psy = next1(rng);
        const float fsx = (psx + (float)px) / (float)fc.resolution[0];
        const float fsy = (psy + (float)py) / (float)fc.resolution[1];
        const float a0 = next1(rng), a1 = next1(rng), a2 = next1(rng);
        V3 ro, rd;
        generate_ray(fc, fsx, fsy, a0, a1, a2, &ro, &rd);
        V3 T = mk(1.0f, 1.0f, 1.0f), L = mk(0.0f, 0.0f, 0.0f);
        float bsdfPdfPrev = 0.0f;
        bool isDeltaPrev = true;
        uint32_t bounce = 0;
        for (;;) {
            HitRecord hit;
            ++extRays;
            // IntersectScene draws the ray's opacity sample (MegakernelPathTracing.hlsl:27-28)
            const float extOpacity = OPACITY ? next1(rng) : 0.0f;
            const bool hasHit = trace_full<false, OPACITY>(sc, ro, rd, inf(), watertight, f2b, extOpacity, lds, shift, &hit);
            const float hitT = hasHit ? hit.t : inf();
            Intersection it;
            it.lightIndex = DCRT_LIGHT_INDEX_INVALID; it.triangleIndex = 0;
            it.geometryNormal = mk(0.0f, 0.0f, 0.0f);
            if (hasHit) hit_to_intersection(sc, hit, it);
            {
                const uint32_t lightIndex = hasHit ? it.lightIndex : fc.envLightIndex;
                const bool doEval = lightVisible ? lightIndex != DCRT_LIGHT_INDEX_INVALID : (bounce > 0 && lightIndex != DCRT_LIGHT_INDEX_INVALID);
                if (doEval) {
                    if (bounce == 0) {
                        // MegakernelPathTracing.hlsl:135-140, 200-205
                        const dcrt_light& Lt = sc.lights[lightIndex];
                        const V3 rad = mk(Lt.radiance[0], Lt.radiance[1], Lt.radiance[2]);
                        if (hasHit) L = dot(-rd, it.geometryNormal) > 0.0f ? rad : mk(0.0f, 0.0f, 0.0f);
                        else L = sc.envCube ? sample_env(sc, rd) * rad : rad;
                    } else {
                        V3 radiance; float lightPdf;
                        evaluate_light<CAPS>(sc, lightIndex, it.triangleIndex, it.geometryNormal, rd, hitT, fc.lightCount, &radiance, &lightPdf);
                        if (lightPdf > 0.0f) {
                            const float weight = !isDeltaPrev ? power_heuristic(bsdfPdfPrev, lightPdf) : 1.0f;
                            L = L + T * radiance * weight;
                        }
                    }
                }
            }
            if (bounce > fc.maxBounce || !hasHit) break;
            const V3 wo = -rd;
            const BsdfFrame bf = bsdf_frame(sc, wo, it);
            V3 lsr = mk(0.0f, 0.0f, 0.0f);
            bool hasShadow = false;
            V3 so = mk(0.0f, 0.0f, 0.0f), sd = so;
            float sdist = 0.0f;
            if (fc.lightCount != 0) {
                const LightSample ls = sample_light<CAPS>(sc, it.position, fc.lightCount, rng);
                if (any_pos(ls.radiance) && ls.pdf > 0.0f) {
                    const V3 bsdf = evaluate_bsdf(sc, vndf, ls.wi, bf, it);
                    const float NdotWI = fabsf(dot(it.normal, ls.wi));
                    const float bsdfPdf = evaluate_bsdf_pdf(sc, vndf, ls.wi, bf, it);
                    const float weight = ls.isDelta ? 1.0f : power_heuristic(ls.pdf, bsdfPdf);
                    lsr = T * ls.radiance * bsdf * NdotWI * weight / ls.pdf;
                    so = offset_ray_origin(it.position, it.geometryNormal, ls.wi);
                    sd = ls.wi;
                    sdist = ls.distance;
                    hasShadow = true;
                }
            }
            // IsOcculuded draws its opacity sample before the BSDF sample (:57-58)
            const float shadowOpacity = OPACITY && hasShadow ? next1(rng) : 0.0f;
            bool terminate = false;
            {
                const float sel = next1(rng);
                const float sx = next1(rng), sy = next1(rng);
                V3 wi, bsdf;
                float bsdfPdf = 0.0f;
                bool isDelta = false;
                sample_bsdf(sc, vndf, bf, sx, sy, sel, it, &wi, &bsdf, &bsdfPdf, &isDelta);
                if ((bsdf.x != 0.0f || bsdf.y != 0.0f || bsdf.z != 0.0f) && bsdfPdf != 0.0f) {
                    const float NdotWI = fabsf(dot(it.normal, wi));
                    T = T * bsdf * NdotWI / bsdfPdf;
                    ro = offset_ray_origin(it.position, it.geometryNormal, wi);
                    rd = wi;
                    ++bounce;
                    // Russian roulette, as in shade_path (the vertex's bounce index is bounce - 1): the draw follows
                    // the three above, ahead of the next turn's; a path it ends leaves the loop below
                    if (fc.rouletteEnable != 0u && bounce > fc.rouletteStart &&
                        !roulette(fc.rouletteMin, fc.rouletteMax, T, [&] { return next1(rng); }))
                        terminate = true;
                } else {
                    terminate = true;
                }
                bsdfPdfPrev = bsdfPdf;
                isDeltaPrev = isDelta;
            }
            if (hasShadow) {
                ++shadowRays;
                HitRecord sh;
                const bool occluded = trace_full<true, OPACITY>(sc, so, sd, sdist, watertight, f2b, shadowOpacity, lds, shift, &sh);
                if (!occluded) L = L + lsr;
            }
            if (terminate) break;
        }
        const size_t p = (size_t)image * film.width * film.height + (size_t)py * film.width + px;
        film.samplePosition[p] = make_float2(psx, psy);
        film.sampleValue[p] = make_float4(L.x, L.y, L.z, 0.0f);
        if (debugRng) film.debugRng[p] = make_uint4(rng.s0, rng.s1, rng.s2, rng.s3);
    }
    const unsigned long long e = wave_sum((uint32_t)extRays), sh = wave_sum((uint32_t)shadowRays);
    if (lane == 0) { atomicAdd(&g->extRays, e); atomicAdd(&g->shadowRays, sh); }
}

// ---- first-hit debug views (MegakernelPathTracing.hlsl:212-291, the OUTPUT_* variants) ------
// The megakernel's launch shape (persistent grid, one claimed 8x8 block per wave, the LDS scene
// cache and stack columns), but a pixel's work ends at its camera ray's closest hit: the view's
// colour is a function of that hit (hit_to_intersection, as MATERIAL and the megakernel call
// it) or, for the iteration-count heat map, of the ray's node visits. The traversal is the
// counting one (trav_visit<INSTR>: one call per visited node in the reference's order, in
// either device node order), so `nodes` is BVHAccel.inc.hlsl:121's iterationCounter. The view
// and the threshold are kernel arguments: the traversal dominates a pixel's time.
template <bool OPACITY>
__global__ __launch_bounds__(256) void view_kernel(DeviceScene sc, const FrameConstants* __restrict__ fcp, Film film, Globals* g, uint32_t debugRng,
                                                   uint32_t outputType, uint32_t iterationThreshold)
{
    extern __shared__ uint32_t stackMem[];
    scene_cache_load(sc, stackMem, block_shift());
    __shared__ uint32_t sm[64];
    const FrameConstants& fc = *fcp;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t shard = blockIdx.x % kShards;
    uint32_t* cursor = &g->nextBlock[shard * kShardStride];
    const uint32_t shardBlocks = g->totalBlocks > shard ? (g->totalBlocks - shard + kShards - 1) / kShards : 0u;
    const bool watertight = (fc.features & DCRT_FEATURE_WATERTIGHT) != 0;
    const bool f2b = (fc.features & DCRT_FEATURE_NO_FRONT_TO_BACK) == 0;
    uint32_t* lds = stackMem + threadIdx.x;
    const uint32_t shift = block_shift();
    uint32_t extRays = 0;
    for (;;) {
        // every wave of the block claims one block per round (one atomic per workgroup)
        bool want = false;
        if (lane == 0) want = __hip_atomic_load(cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < shardBlocks;
        const uint32_t bslot = block_append(want, cursor, sm);
        const uint32_t claimed = (uint32_t)__shfl((int)bslot, 0, 64);
        const bool got = __shfl((int)want, 0, 64) != 0 && claimed < shardBlocks;
        if (__syncthreads_or(got ? 1 : 0) == 0) break;
        if (!got) continue;
        const uint32_t block = shard + claimed * kShards;
        uint32_t px = 0, py = 0, image = 0;
        if (!block_pixel(fc, film, block, lane, &px, &py, &image)) continue;
        Rng rng = rng_init(px, py, image_seed(fc, image));
        const float psx = next1(rng), psy = next1(rng);
        const float fsx = (psx + (float)px) / (float)fc.resolution[0];
        const float fsy = (psy + (float)py) / (float)fc.resolution[1];
        const float a0 = next1(rng), a1 = next1(rng), a2 = next1(rng);
        V3 ro, rd;
        generate_ray(fc, fsx, fsy, a0, a1, a2, &ro, &rd);
        ++extRays;
        TravState s;
        trav_init(s, ro, rd, 0.0f, inf(), f2b);
        // IntersectScene draws the ray's opacity sample (MegakernelPathTracing.hlsl:27-28)
        s.opacitySample = OPACITY ? next1(rng) : 0.0f;
        TraversalStats st = {};
        for (;;) {
            if (trav_visit<true>(sc, s, lds, shift, st)) break;
            if (s.parked && trav_leaf<false, true, OPACITY>(sc, s, watertight, lds, shift, st)) break;
        }
        V3 l = mk(0.0f, 0.0f, 0.0f);
        if (outputType == DCRT_OUTPUT_ITERATION_COUNT) {
            // (hits and misses alike, :286-288; an IEEE division as the HLSL's)
            const float f = (float)st.nodes / (float)iterationThreshold;
            l = st.nodes <= iterationThreshold ? mk(f, f, f) : mk(1.0f, 0.0f, 0.0f);
        } else if (s.found) {
            Intersection it;
            hit_to_intersection(sc, s.hit, it);
            const V3 green = mk(0.0f, 1.0f, 0.0f), red = mk(1.0f, 0.0f, 0.0f);
            switch (outputType) {
            case DCRT_OUTPUT_SHADING_NORMAL: l = it.normal * 0.5f + mk(0.5f, 0.5f, 0.5f); break;
            case DCRT_OUTPUT_SHADING_TANGENT: l = it.tangent * 0.5f + mk(0.5f, 0.5f, 0.5f); break;
            case DCRT_OUTPUT_ALBEDO: l = it.albedo; break;
            case DCRT_OUTPUT_NEGATIVE_NDOTV: l = dot(-rd, it.normal) < 0.0f ? green : red; break;
            case DCRT_OUTPUT_BACKFACE: l = it.backface ? green : red; break;
            default: break;
            }
        }
        const size_t p = (size_t)image * film.width * film.height + (size_t)py * film.width + px;
        film.samplePosition[p] = make_float2(psx, psy);
        film.sampleValue[p] = make_float4(l.x, l.y, l.z, 0.0f);
        if (debugRng) film.debugRng[p] = make_uint4(rng.s0, rng.s1, rng.s2, rng.s3);
    }
    const unsigned long long e = wave_sum(extRays);
    if (lane == 0) atomicAdd(&g->extRays, e);
}

// ---- drain completion ----------------------------------------------------------------------
// Launched after every iteration's cast. Once a batch has no pixel block left to claim and
// at most fc.drainPaths paths are live, it runs each of them to its end in one lane, as the
// megakernel does, with the wavefront's arithmetic: the MATERIAL pass (shade_path) at the hit
// the cast just wrote, then the shadow ray, then the next extension ray, and so on, and the
// finish list's completion (CONTROL :520-528 + WriteSample) -- the same operations in the same
// order per path, so the same bits as the remaining iterations. A batch's drain iterations
// each took as long as their longest ray (a few thousand rays with 100-500 dependent node
// visits on the spaceship scene, 3 launches each); here a path's remaining rays follow each
// other in its lane and different paths overlap. The next iteration then finds the queues
// empty (kDrainedWord) and the batch complete.
template <uint32_t CAPS>
__global__ __launch_bounds__(256) void drain_kernel(PathPool pool, DeviceScene sc, const FrameConstants* __restrict__ fcp, Counters* cnt,
                                                    Globals* g, const SampleOut* __restrict__ sampleOut)
{
    const FrameConstants& fc = *fcp;
    if (!fc.drainPaths || g->stopped || virtual_items(cnt)) return;
    QueueMap qe;
    qmap(cnt, kQExt, &qe);
    QueueMapN<kFinShards> fm;
    qmap(cnt, kQFinish, &fm);
    const uint32_t nExt = qe.prefix[kShards], nFin = fm.prefix[kFinShards];
    // (live all the same: the paths MATERIAL completed at their last shaded bounce, whose last rays this
    // iteration's cast traced -- nothing is left to do for them)
    uint32_t lastRays, completed;
    last_totals(cnt, &lastRays, &completed);
    if (nExt + nFin + completed == 0u || nExt + nFin + completed > fc.drainPaths) return;
    for (uint32_t sh = 0; sh < kShards; ++sh) {   // a block still to claim: new paths will follow
        const uint32_t blocks = g->totalBlocks > sh ? (g->totalBlocks - sh + kShards - 1) / kShards : 0u;
        if (__hip_atomic_load(&g->nextBlock[sh * kShardStride], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < blocks) return;
    }
    extern __shared__ uint32_t stackMem[];
    scene_cache_load(sc, stackMem, block_shift());
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        cnt->w[kDrainedWord * kShardStride] = 1u;   // the next MATERIAL / CONTROL pass: nothing to take
        g->prevLive = 0u;                           // (so the next iteration completes the batch)
    }
    const bool watertight = (fc.features & DCRT_FEATURE_WATERTIGHT) != 0;
    const bool f2b = (fc.features & DCRT_FEATURE_NO_FRONT_TO_BACK) == 0;
    uint32_t* lds = stackMem + threadIdx.x;
    const uint32_t shift = block_shift();
    const SampleOut so = *sampleOut;
    uint32_t extRays = 0, shadowRays = 0;
    // paths dealt to the waves first, lanes second (path w -> wave w mod waves, lane w / waves):
    // a wave runs a lane's path until that path ends, and its traversal and shading loops
    // last as long as their slowest lane, so few paths per wave let each path run at its own
    // chain's latency (the paths dealt to consecutive lanes had made every wave wait, bounce
    // by bounce, for its slowest path -- the wavefront's drain iterations again)
    const uint32_t waves = gridDim.x * (blockDim.x >> 6);
    const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    for (uint32_t w = (threadIdx.x & 63u) * waves + wave; w < nExt + nFin; w += 64u * waves) {
        if (w >= nExt) {
            // a path MATERIAL ended with its shadow ray pending (cast this iteration): CONTROL's
            // completion, as control_kernel does it
            const uint32_t f = qpos(pool.finCap, fm, w - nExt);
            const FinishRec fr = pool.finRec[f];
            const bool shadowHit = pool.finHit[f] != 0u;
            const uint32_t path = asu(fr.lsrSlot.z);
            F3 li{fr.liLsr.x, fr.liLsr.y, fr.liLsr.z};
            const F3 lsr{fr.liLsr.w, fr.lsrSlot.x, fr.lsrSlot.y};
            li.x = li.x + (!shadowHit ? lsr.x : 0.0f);
            li.y = li.y + (!shadowHit ? lsr.y : 0.0f);
            li.z = li.z + (!shadowHit ? lsr.z : 0.0f);
            const uint32_t p = slot(pool.pixel, path);
            sample_at(so.samplePosition, p) = pixel_sample(fc, p);
            sample_at(so.sampleValue, p) = make_float4(li.x, li.y, li.z, 0.0f);
            slot(pool.flags, path) = kFlagIdle;
            continue;
        }
        // a continuing path: its state at its extension-queue position, the hit at its item
        const uint32_t q = qpos(pool.recCap, qe, w);
        const PathStateA ps = state_at(pool.stateA, q);
        const float4 h4 = pool.hit[2 * w], hd = pool.hit[2 * w + 1];
        HitRecord hit;
        hit.t = h4.x; hit.u = h4.y; hit.v = h4.z; hit.tri = asu(h4.w); hit.inst = asu(hd.w);
        V3 dir = mk(hd.x, hd.y, hd.z);
        Rng rng;
        rng.s0 = ps.rng.x; rng.s1 = ps.rng.y; rng.s2 = ps.rng.z; rng.s3 = ps.rng.w;
        const uint32_t path = asu(ps.lsrMisc.w);
        uint32_t flags = asu(ps.lsrMisc.z);
        const bool first = (flags & kFlagFirst) != 0u;
        float4 thr = make_float4(1.0f, 1.0f, 1.0f, 0.0f), l4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (!first) {
            const PathStateB psB = state_at(pool.stateB, q);
            thr = psB.thr;
            l4 = psB.liLsr;
        }
        bool shadowHit = (flags & kFlagShadowResolved) != 0u || ((flags & kFlagShadowPending) ? pool.shadowHit[q] != 0u : false);
        flags &= ~(kFlagFirst | kFlagShadowPending | kFlagShadowResolved);
        F3 li{l4.x, l4.y, l4.z};
        V3 lsr0 = mk(l4.w, ps.lsrMisc.x, ps.lsrMisc.y);
        for (;;) {
            li.x = li.x + (!shadowHit ? lsr0.x : 0.0f);
            li.y = li.y + (!shadowHit ? lsr0.y : 0.0f);
            li.z = li.z + (!shadowHit ? lsr0.z : 0.0f);
            bool terminate = false, hasShadow = false;
            V3 T, L, lsr, nO = mk(0.0f, 0.0f, 0.0f), nD = nO, sD = nO;
            float4 sO = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float extOpacity = 0.0f, shadowOpacity = 0.0f;
            DCRT_MCLK_INIT;   // (the drain's sections are not reported)
            shade_path<CAPS>(sc, fc, hit, dir, rng, flags, thr, li, T, L, lsr, terminate, hasShadow, nO, nD, sO, sD,
                             extOpacity, shadowOpacity DCRT_MCLK_ARGS);
            shadowHit = false;
            if (hasShadow) {   // SHADOW_RAY_CAST
                HitRecord sh;
                shadowHit = trace_full<true, false>(sc, mk(sO.x, sO.y, sO.z), sD, sO.w, watertight, f2b, 0.0f, lds, shift, &sh);
                ++shadowRays;
            }
            if (terminate) {
                // MATERIAL's WriteSample (no shadow ray: L + 0) or CONTROL's (Li += lsr unless
                // the shadow ray hit)
                const uint32_t p = slot(pool.pixel, path);
                sample_at(so.samplePosition, p) = pixel_sample(fc, p);
                sample_at(so.sampleValue, p) = make_float4(L.x + (!shadowHit ? lsr.x : 0.0f), L.y + (!shadowHit ? lsr.y : 0.0f),
                                                           L.z + (!shadowHit ? lsr.z : 0.0f), 0.0f);
                if (so.debugRng) sample_at(so.debugRng, p) = make_uint4(rng.s0, rng.s1, rng.s2, rng.s3);
                slot(pool.flags, path) = kFlagIdle;
                break;
            }
            // EXTENSION_RAY_CAST of the next ray; the next MATERIAL pass's inputs
            if (!trace_full<false, false>(sc, nO, nD, inf(), watertight, f2b, 0.0f, lds, shift, &hit)) {
                hit.t = inf(); hit.u = 0.0f; hit.v = 0.0f; hit.tri = 0u; hit.inst = 0u;
            }
            ++extRays;
            dir = nD;
            thr = make_float4(T.x, T.y, T.z, thr.w);
            li = F3{L.x, L.y, L.z};
            lsr0 = lsr;
        }
    }
    const unsigned long long e = wave_sum(extRays), sr = wave_sum(shadowRays);
    if ((threadIdx.x & 63u) == 0) {
        if (e) atomicAdd(&g->extRays, e);
        if (sr) atomicAdd(&g->shadowRays, sr);
    }
}

// ---- kernel-level batch entry points (tests / roofline) -----------------------------------
// INSTR: count the reference's traversal (trav_visit); otherwise the kernels' trav_visit_pair
template <bool ANY, bool INSTR>
__global__ __launch_bounds__(256) void batch_trace_kernel(DeviceScene sc, const dcrt_ray* rays, uint32_t n, uint32_t features,
                                                           dcrt_ray_hit* hits, uint32_t* occluded, unsigned long long* instr)
{
    extern __shared__ uint32_t stackMem[];
    scene_cache_load(sc, stackMem, block_shift());
    TraversalStats st = {};
    persistent_trace<ANY, INSTR, false, false, false, !INSTR>(
        sc, n, features, 16u, 32u, stackMem + threadIdx.x, block_shift(),
        [&](uint32_t i) __attribute__((always_inline)) { return i; },
        [&](uint32_t i, uint32_t, TravState& s) __attribute__((always_inline)) {
            const dcrt_ray r = rays[i];
            trav_init(s, ld3(r.origin), ld3(r.direction), 0.0f, ANY ? r.t_max : inf());
            return i;
        },
        [&](uint32_t i, const TravState& s) __attribute__((always_inline)) {
            if (ANY) {
                occluded[i] = s.found ? 1u : 0u;
            } else {
                dcrt_ray_hit o;
                o.t = s.found ? s.hit.t : inf(); o.u = s.found ? s.hit.u : 0.0f; o.v = s.found ? s.hit.v : 0.0f;
                o.triangle_id = s.found ? s.hit.tri : 0u; o.instance_index = s.found ? s.hit.inst : 0u;
                hits[i] = o;
            }
        },
        st);
    if (INSTR) flush_stats(st, instr);
}

// cast_kernel's merged section over a caller's ray batch (tests: dcrt_tracer_cast_rays): the same persistent_trace
// instantiation (LANE_ANY, the variant's template arguments, its kLayout, its occupancy target), launched on the
// scene copy, LDS bytes and block of the cast plan's launch. kinds[i] != 0: a shadow ray (first hit below its
// t_max); else an extension ray (closest hit, infinite t_max). OPACITY: ray i carries opacity[i].
template <bool OPACITY, bool ALL_CACHED, bool PAIR, bool IDENT, bool RING, bool FLAT>
__global__ __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(ALL_CACHED && !OPACITY ? (IDENT ? DCRT_IDENT_CAST_WAVES_PER_EU : DCRT_CACHED_CAST_WAVES_PER_EU)
                                   : (!ALL_CACHED && !PAIR && !OPACITY ? DCRT_GLOBAL_CAST_WAVES_PER_EU : DCRT_CAST_WAVES_PER_EU), 8)))
void cast_rays_kernel(DeviceScene sc, const dcrt_ray* rays, const uint32_t* kinds, const float* opacity, uint32_t n, uint32_t features,
                      uint32_t refillLanes, uint32_t parkLanes, dcrt_ray_hit* hits, uint32_t* occluded)
{
    extern __shared__ uint32_t stackMem[];
    scene_cache_load<ALL_CACHED>(sc, stackMem, block_shift());
    constexpr int kLayout = PAIR ? kLayoutPairs : kLayoutFlat;   // (cast_kernel's rule for its non-counting variants)
    TraversalStats st = {};
    persistent_trace<false, false, OPACITY, true, ALL_CACHED, PAIR, kLayout, IDENT, RING, FLAT>(
        sc, n, features, refillLanes, parkLanes, stackMem + threadIdx.x, block_shift(),
        [&](uint32_t i) __attribute__((always_inline)) { return i; },
        [&](uint32_t i, uint32_t, TravState& s) __attribute__((always_inline)) {
            const dcrt_ray r = rays[i];
            const bool shadow = kinds[i] != 0u;
            trav_init(s, ld3(r.origin), ld3(r.direction), 0.0f, shadow ? r.t_max : inf());
            s.anyHit = shadow;
            if (OPACITY) s.opacitySample = opacity[i];
            return i;
        },
        [&](uint32_t i, const TravState& s) __attribute__((always_inline)) {
            const bool rec = s.found && !s.anyHit;
            dcrt_ray_hit o;
            o.t = rec ? s.hit.t : inf(); o.u = rec ? s.hit.u : 0.0f; o.v = rec ? s.hit.v : 0.0f;
            o.triangle_id = rec ? s.hit.tri : 0u; o.instance_index = rec ? s.hit.inst : 0u;
            hits[i] = o;
            occluded[i] = s.anyHit && s.found ? 1u : 0u;
        },
        st);
}

// The merged cast's streaming shadow section over a caller's ray batch (tests): cast_kernel<..., CELLS>'s
// LDS layout and device function, one ray per lane
__global__ __launch_bounds__(256) void cells_occlusion_kernel(DeviceScene sc, const dcrt_ray* rays, uint32_t n, uint32_t features,
                                                               uint32_t* occluded)
{
    extern __shared__ uint32_t stackMem[];
    uint32_t* leafWords = (uint32_t*)(scene_cache(sc, stackMem, block_shift()) + sc.cachedNodes * 2u + sc.cachedTris * kRotTriFloat4);
    if (threadIdx.x < kCellWords) leafWords[threadIdx.x] = sc.shadowLeaves[threadIdx.x];
    scene_cache_load<true>(sc, stackMem, block_shift());
    const bool watertight = (features & DCRT_FEATURE_WATERTIGHT) != 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const dcrt_ray r = rays[i];
        const bool occ = cells_occluded(sc, make_float4(r.origin[0], r.origin[1], r.origin[2], r.t_max),
                                        make_float4(r.direction[0], r.direction[1], r.direction[2], 0.0f), watertight,
                                        stackMem + threadIdx.x, block_shift(), leafWords);
        occluded[i] = occ ? 1u : 0u;
    }
}

__global__ void math_eval_kernel(int function, const float* x, uint32_t n, float* y)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    switch (function) {
    case 0: y[i] = det_sin(x[i]); break;
    case 1: y[i] = det_cos(x[i]); break;
    case 2: y[i] = det_exp(x[i]); break;
    case 4: y[i] = det_log(x[i]); break;
    case 5: y[i] = rcp_ieee(x[i]); break;    // (the fast reciprocal against ...)
    case 6: y[i] = 1.0f / x[i]; break;       // (... the compiler's IEEE division)
    default: y[i] = det_atan(x[i]); break;
    }
}

// One material's BSDF at a caller's directions (tests): MATERIAL's bsdf_frame / evaluate_bsdf /
// evaluate_bsdf_pdf / sample_bsdf in the frame n = (0,0,1), t = (1,0,0). Of `sc` only the LUTs are read.
__device__ __forceinline__ Intersection bsdf_probe_intersection(const dcrt_bsdf_probe_material& m, const float* dielRows)
{
    Intersection it;
    it.albedo = mk(m.albedo[0], m.albedo[1], m.albedo[2]);
    it.alpha = m.alpha;
    it.position = mk(0.0f, 0.0f, 0.0f);
    it.normal = mk(0.0f, 0.0f, 1.0f);
    it.tangent = mk(1.0f, 0.0f, 0.0f);
    it.geometryNormal = mk(0.0f, 0.0f, 1.0f);
    it.ior = mk(m.ior[0], m.ior[1], m.ior[2]);
    it.isTwoSided = m.two_sided != 0;
    it.backface = false;
    it.multiscattering = m.multiscattering != 0;
    it.internalScatteringMode = m.internal_scattering_mode;
    it.materialType = m.type;
    it.lightIndex = DCRT_LIGHT_INDEX_INVALID;
    it.triangleIndex = 0;
    it.dielRows = dielRows;   // (the probe material's own rows, or null)
    return it;
}
// The frame of caller-supplied hit records (tests): hit_to_intersection in the form that takes the
// frame table (sc.triFrames, or null), as MATERIAL's delta-only whole-scene variants call it.
__global__ void frame_probe_kernel(DeviceScene sc, const uint4* records, uint32_t n, float* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 r = records[i];
    HitRecord h;
    h.t = 1.0f; h.u = asf(r.x); h.v = asf(r.y); h.tri = r.z; h.inst = r.w;
    Intersection it;
    hit_to_intersection<kCapAll, true>(sc, h, it);
    float* o = out + (size_t)i * 9;
    o[0] = it.normal.x; o[1] = it.normal.y; o[2] = it.normal.z;
    o[3] = it.tangent.x; o[4] = it.tangent.y; o[5] = it.tangent.z;
    o[6] = it.geometryNormal.x; o[7] = it.geometryNormal.y; o[8] = it.geometryNormal.z;
}
// The stages between the casts and the BSDF at a caller's inputs (tests; layouts in dcrt.h): generate_ray,
// hit_to_intersection (TABLE: the form that takes the frame table, else the per-hit form of the any-scene
// MATERIAL variants), sample_light, evaluate_light and sample_env as the path kernels call them.
__global__ void camera_ray_probe_kernel(FrameConstants fc, const float* film, const float* aperture, uint32_t n, float* origins, float* directions)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    V3 o, d;
    generate_ray(fc, film[2 * i], film[2 * i + 1], aperture[3 * i], aperture[3 * i + 1], aperture[3 * i + 2], &o, &d);
    origins[3 * i] = o.x; origins[3 * i + 1] = o.y; origins[3 * i + 2] = o.z;
    directions[3 * i] = d.x; directions[3 * i + 1] = d.y; directions[3 * i + 2] = d.z;
}
// dcrt_device_roulette: the path kernels' roulette on given throughputs, u standing in for the path's draw. q, whether
// the path goes on (1 / 0), and the throughput it goes on with (as given where it ends or q >= 1).
__global__ void roulette_probe_kernel(float lo, float hi, const float* throughputs, const float* u, uint32_t n, float* outQ, uint32_t* outSurvive,
                                      float* outScaled)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    V3 T = mk(throughputs[3 * i], throughputs[3 * i + 1], throughputs[3 * i + 2]);
    float q;
    const bool survives = roulette(lo, hi, T, [&] { return u[i]; }, &q);
    outQ[i] = q;
    outSurvive[i] = survives ? 1u : 0u;
    outScaled[3 * i] = T.x; outScaled[3 * i + 1] = T.y; outScaled[3 * i + 2] = T.z;
}
template <bool TABLE>
__global__ void intersection_probe_kernel(DeviceScene sc, const uint4* records, uint32_t n, float* outFloats, uint32_t* outWords)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 r = records[i];
    HitRecord h;
    h.t = 1.0f; h.u = asf(r.x); h.v = asf(r.y); h.tri = r.z; h.inst = r.w;
    Intersection it;
    hit_to_intersection<kCapAll, TABLE>(sc, h, it);
    float* o = outFloats + (size_t)i * 16;
    const V3 v[5] = {it.position, it.normal, it.tangent, it.geometryNormal, it.albedo};
    for (int k = 0; k < 5; ++k) { o[3 * k] = v[k].x; o[3 * k + 1] = v[k].y; o[3 * k + 2] = v[k].z; }
    o[15] = it.alpha;
    uint32_t* w = outWords + (size_t)i * 3;
    w[0] = it.materialType;
    w[1] = (it.isTwoSided ? 1u : 0u) | (it.backface ? 2u : 0u) | (it.multiscattering ? 4u : 0u) | (it.internalScatteringMode << 4);
    w[2] = it.lightIndex;
}
template <uint32_t CAPS>
__global__ void light_sample_probe_kernel(DeviceScene sc, uint32_t lightCount, const float* points, const uint4* states, uint32_t n,
                                          float* outFloats, uint32_t* outWords)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 s = states[i];
    Rng rng;
    rng.s0 = s.x; rng.s1 = s.y; rng.s2 = s.z; rng.s3 = s.w;
    const LightSample r = sample_light<CAPS>(sc, mk(points[3 * i], points[3 * i + 1], points[3 * i + 2]), lightCount, rng);
    float* o = outFloats + (size_t)i * 8;
    o[0] = r.radiance.x; o[1] = r.radiance.y; o[2] = r.radiance.z;
    o[3] = r.wi.x; o[4] = r.wi.y; o[5] = r.wi.z;
    o[6] = r.pdf; o[7] = r.distance;
    uint32_t* w = outWords + (size_t)i * 5;
    w[0] = r.isDelta ? 1u : 0u;
    w[1] = rng.s0; w[2] = rng.s1; w[3] = rng.s2; w[4] = rng.s3;
}
template <uint32_t CAPS>
__global__ void light_eval_probe_kernel(DeviceScene sc, uint32_t lightCount, const uint32_t* lightTriangle, const float* in, uint32_t n, float* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* a = in + (size_t)i * 7;
    V3 radiance; float pdf;
    evaluate_light<CAPS>(sc, lightTriangle[2 * i], lightTriangle[2 * i + 1], mk(a[0], a[1], a[2]), mk(a[3], a[4], a[5]), a[6], lightCount, &radiance, &pdf);
    out[4 * i] = radiance.x; out[4 * i + 1] = radiance.y; out[4 * i + 2] = radiance.z; out[4 * i + 3] = pdf;
}
__global__ void env_lookup_probe_kernel(DeviceScene sc, const float* directions, uint32_t n, float* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3 c = sample_env(sc, mk(directions[3 * i], directions[3 * i + 1], directions[3 * i + 2]));
    out[3 * i] = c.x; out[3 * i + 1] = c.y; out[3 * i + 2] = c.z;
}
__global__ void bsdf_eval_kernel(DeviceScene sc, dcrt_bsdf_probe_material m, uint32_t features, const float* wi, const float* wo,
                                 uint32_t n, float* f, float* pdf)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool vndf = (features & DCRT_FEATURE_GGX_SAMPLE_VNDF) != 0;
    const Intersection it = bsdf_probe_intersection(m, sc.dielRows);
    const V3 a = mk(wi[3 * i], wi[3 * i + 1], wi[3 * i + 2]), b = mk(wo[3 * i], wo[3 * i + 1], wo[3 * i + 2]);
    const BsdfFrame bf = bsdf_frame(sc, b, it);
    const V3 v = evaluate_bsdf(sc, vndf, a, bf, it);
    f[3 * i] = v.x; f[3 * i + 1] = v.y; f[3 * i + 2] = v.z;
    pdf[i] = evaluate_bsdf_pdf(sc, vndf, a, bf, it);
}
__global__ void bsdf_sample_kernel(DeviceScene sc, dcrt_bsdf_probe_material m, uint32_t features, const float* wo, const float* u,
                                   uint32_t n, float* wi, float* f, float* pdf, uint32_t* delta)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool vndf = (features & DCRT_FEATURE_GGX_SAMPLE_VNDF) != 0;
    const Intersection it = bsdf_probe_intersection(m, sc.dielRows);
    const V3 b = mk(wo[3 * i], wo[3 * i + 1], wo[3 * i + 2]);
    const BsdfFrame bf = bsdf_frame(sc, b, it);
    V3 w, v; float p; bool d;
    sample_bsdf(sc, vndf, bf, u[3 * i], u[3 * i + 1], u[3 * i + 2], it, &w, &v, &p, &d);
    wi[3 * i] = w.x; wi[3 * i + 1] = w.y; wi[3 * i + 2] = w.z;
    f[3 * i] = v.x; f[3 * i + 1] = v.y; f[3 * i + 2] = v.z;
    pdf[i] = p;
    delta[i] = d ? 1u : 0u;
}

// ---- SampleConvolution ----------------------------------------------------------------
struct FilterConsts { float radius, gaussianAlpha, gaussianExp, mf[7]; uint32_t tau, kind; };

__device__ __forceinline__ float filter_1d_sinc(float x) { x = fabsf(x); return x >= 1e-5f ? det_sin(3.1415926535f * x) / (3.1415926535f * x) : 1.0f; }
__device__ __forceinline__ float evaluate_filter(const FilterConsts& c, float px, float py)
{
    const float r = c.radius;
    switch (c.kind) {
    case DCRT_FILTER_TRIANGLE: return fmaxf(0.0f, r - fabsf(px)) * fmaxf(0.0f, r - fabsf(py));
    case DCRT_FILTER_GAUSSIAN: {
        const float gx = fmaxf(0.0f, det_exp(-c.gaussianAlpha * px * px) - c.gaussianExp);
        const float gy = fmaxf(0.0f, det_exp(-c.gaussianAlpha * py * py) - c.gaussianExp);
        return gx * gy;
    }
    case DCRT_FILTER_MITCHELL: {
        float v[2] = { px / c.radius, py / c.radius }, o[2];
        for (int k = 0; k < 2; ++k) {
            const float x = fabsf(2.0f * v[k]);
            float m = x < 1.0f ? c.mf[4] * x * x * x + c.mf[5] * x * x + c.mf[6]
                               : (x < 2.0f ? c.mf[0] * x * x * x + c.mf[1] * x * x + c.mf[2] * x + c.mf[3] : 0.0f);
            o[k] = m * (1.0f / 6.0f);
        }
        return o[0] * o[1];
    }
    case DCRT_FILTER_LANCZOS: {
        float o[2], v[2] = { px, py };
        for (int k = 0; k < 2; ++k) {
            const float x = fabsf(v[k]);
            const float lanczos = filter_1d_sinc(x / (float)c.tau);
            o[k] = x > r ? 0.0f : filter_1d_sinc(x) * lanczos;
        }
        return o[0] * o[1];
    }
    default: return (fabsf(px) <= r && fabsf(py) <= r) ? 1.0f : 0.0f;
    }
}

// SampleConvolution (SampleConvolution.hlsl:67-106), grid-stride over pixels. With
// `guard` set it runs only in the iteration that completed an image (RenderImages).
// One 16x16 pixel tile per workgroup: each image's samples of the tile plus the filter's
// halo are staged in LDS once (instead of every pixel fetching its (2r+1)^2 window from
// memory), then every pixel gathers its window from LDS. Per pixel the arithmetic and its
// order are those of the direct gather (images in order, window rows then columns).
#ifndef DCRT_FILM_TILE
#define DCRT_FILM_TILE 16
#endif
constexpr int kFilmTile = DCRT_FILM_TILE;   // (a workgroup per kFilmTile^2-pixel tile, one thread per pixel)
constexpr int kFilmThreads = kFilmTile * kFilmTile;
constexpr int kFilmMaxHalo = 4;
constexpr int kFilmSpan = kFilmTile + 2 * kFilmMaxHalo;
constexpr int kFilmStage = (kFilmSpan * kFilmSpan + kFilmThreads - 1) / kFilmThreads;   // staging elements per thread

__device__ __forceinline__ void film_pixel_window(const FilterConsts& c, uint32_t px, uint32_t py, uint32_t W, uint32_t H,
                                                  int* xs, int* xe, int* ys, int* ye)
{
    const float r = c.radius;
    const float cx = (float)px + 0.5f, cy = (float)py + 0.5f;
    *xs = (int)floorf(cx - r); *xs = *xs < 0 ? 0 : *xs;
    *xe = (int)floorf(cx + r); *xe = *xe > (int)W - 1 ? (int)W - 1 : *xe;
    *ys = (int)floorf(cy - r); *ys = *ys < 0 ? 0 : *ys;
    *ye = (int)floorf(cy + r); *ye = *ye > (int)H - 1 ? (int)H - 1 : *ye;
}

// posList / valList (accumulate_images): image b's sample textures sit at posList[b] / valList[b]
// (W*H each, e.g. other pipelines' slots) instead of at slot b of this film's.
// HALF (the convergence estimate's half film, dcrt.h "film noise estimate"): a second accumulator
// `half` takes the same additions, in the same order, for the images whose film image index
// (firstIndex + b; under `guard` the call's base plus the images done, both from device memory:
// the launch sits in a replayed graph) is even.
template <bool HALF>
__device__ __forceinline__ void film_pass(Film film, const FilterConsts* fcon, uint32_t images, const Globals* guard,
                                          const float2* const* __restrict__ posList, const float4* const* __restrict__ valList,
                                          float4* half, uint32_t firstIndex)
{
    if (guard && (!guard->imageComplete || guard->skipFilm)) return;
    const uint32_t first = HALF ? (guard ? guard->filmImageBase + guard->imagesDone : firstIndex) : 0u;
    // the images of a completed batch, in order: per pixel the same additions as one
    // film pass per image
    const uint32_t count = guard ? guard->batchImages : images;
    const FilterConsts c = *fcon;
    const uint32_t W = film.width, H = film.height;
    const uint32_t total = W * H;
    const uint32_t tilesX = (W + kFilmTile - 1) / kFilmTile, tiles = tilesX * ((H + kFilmTile - 1) / kFilmTile);
    // two tile buffers: image b is convolved from buffer b & 1 while image b + 1's loads are in flight
    __shared__ float2 tPos[2][kFilmSpan * kFilmSpan];
    __shared__ float4 tVal[2][kFilmSpan * kFilmSpan];
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int x0 = (int)(tile % tilesX) * kFilmTile, y0 = (int)(tile / tilesX) * kFilmTile;
        const uint32_t px = (uint32_t)x0 + (threadIdx.x % kFilmTile), py = (uint32_t)y0 + (threadIdx.x / kFilmTile);
        const bool mine = px < W && py < H && !(film.rowOwned && !film.rowOwned[py]);
        // a partitioned film's tiles without an owned pixel stage and convolve nothing
        // (at N ranks that is (N-1)/N of the tiles)
        if (film.rowOwned && !__syncthreads_or(mine)) continue;
        int xs = 0, xe = -1, ys = 0, ye = -1;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float4 hv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (mine) {
            film_pixel_window(c, px, py, W, H, &xs, &xe, &ys, &ye);
            v = film.accum[(size_t)py * W + px];
            if (HALF) hv = half[(size_t)py * W + px];
        }
        // The tile's staged span is the union of its pixels' windows, taken from the
        // windows of its first and last pixel: floorf(p + 0.5 -/+ r) is monotone in p, so
        // every window of the tile lies inside, whatever the rounding of p + 0.5 + r does
        // (for r just below k + 0.5 a window can reach floor(r + 0.5) + 1 pixels out).
        int txs, txe, tys, tye, unused0, unused1;
        film_pixel_window(c, (uint32_t)x0, (uint32_t)y0, W, H, &txs, &unused0, &tys, &unused1);
        film_pixel_window(c, min((uint32_t)x0 + kFilmTile - 1u, W - 1u), min((uint32_t)y0 + kFilmTile - 1u, H - 1u), W, H,
                          &unused0, &txe, &unused1, &tye);
        const int spanX = txe - txs + 1, spanY = tye - tys + 1;
        if (spanX > kFilmSpan || spanY > kFilmSpan) {
            // wide filters: the direct gather from memory
            for (uint32_t b = 0; b < count && mine; ++b) {
                const float2* sPos = posList ? posList[b] : film.samplePosition + (size_t)b * total;
                const float4* sVal = valList ? valList[b] : film.sampleValue + (size_t)b * total;
                const float cx = (float)px + 0.5f, cy = (float)py + 0.5f;
                float wsum = 0.0f;
                V3 sum = mk(0.0f, 0.0f, 0.0f);
                for (int y = ys; y <= ye; ++y)
                    for (int x = xs; x <= xe; ++x) {
                        const size_t q = (size_t)y * W + x;
                        const float2 sp = sPos[q];
                        const float4 sv = sVal[q];
                        const float w = evaluate_filter(c, cx - (sp.x + (float)x), cy - (sp.y + (float)y));
                        sum = sum + mk(sv.x, sv.y, sv.z) * w;
                        wsum = wsum + w;
                    }
                v.x = v.x + sum.x; v.y = v.y + sum.y; v.z = v.z + sum.z; v.w = v.w + wsum;
                if (HALF && !((first + b) & 1u)) { hv.x = hv.x + sum.x; hv.y = hv.y + sum.y; hv.z = hv.z + sum.z; hv.w = hv.w + wsum; }
            }
        } else {
            // staged span [txs, txe] x [tys, tye]: inside the film by construction
            const int span = spanX, ox = txs, oy = tys;
            // Software-pipelined over the images of a batch: image b + 1's tile is loaded into
            // registers while image b is convolved from its LDS buffer, and one barrier per image
            // separates the two buffers' writes from their reads. The barrier is s_barrier after
            // the LDS stores drain (lgkmcnt), not __syncthreads: that one's fence would also wait
            // for the next image's loads. (A buffer written at image b + 1 was last read at image
            // b - 1, which every thread finished before passing image b's barrier.)
            // (kFilmStage staging elements per thread, in registers: the loops below unroll)
            const int nStage = spanX * spanY;
            const size_t oFirst = (size_t)oy * W + (size_t)ox;
            size_t off[kFilmStage];
            float2 nP[kFilmStage];
            float4 nV[kFilmStage];
#pragma unroll
            for (int k = 0; k < kFilmStage; ++k) {
                const int i = (int)threadIdx.x + k * kFilmThreads;
                off[k] = i < nStage ? (size_t)(oy + i / spanX) * W + (size_t)(ox + i % spanX) : oFirst;
                nP[k] = make_float2(0.0f, 0.0f);
                nV[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
            // image b's sample textures: this film's slot b, or a list entry (accumulate_images),
            // read one image ahead with a vector load (the index made opaque to the uniformity
            // analysis: a scalar load would share lgkmcnt with the LDS traffic, whose waits would
            // then drain it too). The two sources run as two instances of the loop, so neither
            // carries the other's selects and register hazards.
            uint32_t lane0 = 0u;
            asm volatile("" : "+v"(lane0));
            auto run = [&](auto srcPos, auto srcVal) __attribute__((always_inline)) {
                // (unconditional loads: a thread without a third element loads the span's first
                // one again, so no branch splits the loads and their waits stay exact)
                auto stage_load = [&](const float2* lp, const float4* lv) __attribute__((always_inline)) {
#pragma unroll
                    for (int k = 0; k < kFilmStage; ++k) {
                        nP[k] = global_load2(lp, off[k]);
                        nV[k] = global_load4(lv, off[k]);
                    }
                };
                if (count > 0) stage_load(srcPos(0u), srcVal(0u));
                const float2* nextPos = count > 1 ? srcPos(1u) : nullptr;
                const float4* nextVal = count > 1 ? srcVal(1u) : nullptr;
                for (uint32_t b = 0; b < count; ++b) {
                    const uint32_t buf = b & 1u;
#pragma unroll
                    for (int k = 0; k < kFilmStage; ++k) {
                        const int i = (int)threadIdx.x + k * kFilmThreads;
                        if (i < nStage) {
                            tPos[buf][i] = nP[k];
                            tVal[buf][i] = nV[k];
                        }
                    }
                    if (b + 1 < count) {
                        stage_load(nextPos, nextVal);
                        if (b + 2 < count) { nextPos = srcPos(b + 2u); nextVal = srcVal(b + 2u); }
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                    if (mine) {
                        const float cx = (float)px + 0.5f, cy = (float)py + 0.5f;
                        float wsum = 0.0f;
                        V3 sum = mk(0.0f, 0.0f, 0.0f);
                        for (int y = ys; y <= ye; ++y)
                            for (int x = xs; x <= xe; ++x) {
                                const int i = (y - oy) * span + (x - ox);
                                const float2 sp = tPos[buf][i];
                                const float4 sv = tVal[buf][i];
                                const float w = evaluate_filter(c, cx - (sp.x + (float)x), cy - (sp.y + (float)y));
                                sum = sum + mk(sv.x, sv.y, sv.z) * w;
                                wsum = wsum + w;
                            }
                        v.x = v.x + sum.x; v.y = v.y + sum.y; v.z = v.z + sum.z; v.w = v.w + wsum;
                        if (HALF && !((first + b) & 1u)) { hv.x = hv.x + sum.x; hv.y = hv.y + sum.y; hv.z = hv.z + sum.z; hv.w = hv.w + wsum; }
                    }
                }
            };
            if (posList) {
                run([&](uint32_t b) __attribute__((always_inline)) { return (const float2*)global_load_u64((const uint64_t*)posList, b + lane0); },
                    [&](uint32_t b) __attribute__((always_inline)) { return (const float4*)global_load_u64((const uint64_t*)valList, b + lane0); });
            } else {
                run([&](uint32_t b) __attribute__((always_inline)) { return film.samplePosition + (size_t)b * total; },
                    [&](uint32_t b) __attribute__((always_inline)) { return film.sampleValue + (size_t)b * total; });
            }
        }
        if (mine) film.accum[(size_t)py * W + px] = v;
        if (HALF && mine) half[(size_t)py * W + px] = hv;
        __syncthreads();   // the tile buffers are reused by the next tile
    }
}

__global__ __launch_bounds__(kFilmThreads) void film_kernel(Film film, const FilterConsts* fcon, uint32_t images, const Globals* guard,
                                                   const float2* const* __restrict__ posList,
                                                   const float4* const* __restrict__ valList)
{
    film_pass<false>(film, fcon, images, guard, posList, valList, nullptr, 0u);
}
// ... with the half film (convergence on: dcrt_tracer_set_convergence)
__global__ __launch_bounds__(kFilmThreads) void film_half_kernel(Film film, const FilterConsts* fcon, uint32_t images, const Globals* guard,
                                                        const float2* const* __restrict__ posList,
                                                        const float4* const* __restrict__ valList, float4* half, uint32_t firstIndex)
{
    film_pass<true>(film, fcon, images, guard, posList, valList, half, firstIndex);
}

// ---- firefly re-weighting (dcrt.h "firefly re-weighting"; tests/firefly_ref.py restates it) ----
// Zirr, Hanika, Dachsbacher 2018: K cascade films beside the film take each sample's share by its
// brightness band, and a resolve pass keeps a band at a pixel to the extent its neighbourhood
// supports it.
constexpr int kFireflyMaxCascades = 8;
// scale[j] = s_j for j < cascades (the host's float32 products), top = s_{K-1}, invBase = 1 / b,
// invSpan = 1 - invBase: all float32, from the host
struct FireflyConsts { float scale[kFireflyMaxCascades]; float top, invBase, invSpan, minSupport; uint32_t cascades; };
struct CascadeFilms { float4* film[kFireflyMaxCascades]; };

__device__ __forceinline__ float firefly_luminance(float r, float g, float b) { return fmaxf(0.0f, r * 0.299f + g * 0.587f + b * 0.114f); }

// The split of a sample (dcrt.h): its lower cascade `band` and that cascade's share alpha; cascade
// band + 1 takes 1 - alpha (no cascade where band + 1 == K: alpha is 1 there).
__device__ __forceinline__ void firefly_split(const FireflyConsts& k, float Y, uint32_t* band, float* alpha)
{
    uint32_t j = 0u;
    float a = 1.0f;
    if (Y > k.top) {
        j = k.cascades - 1u;
    } else if (Y > k.scale[0]) {
        float sj = k.scale[0];
#pragma unroll
        for (int i = 1; i < kFireflyMaxCascades - 1; ++i)
            if ((uint32_t)i + 1u < k.cascades && Y > k.scale[i]) { j = (uint32_t)i; sj = k.scale[i]; }
        a = fminf(fmaxf((sj / Y - k.invBase) / k.invSpan, 0.0f), 1.0f);
    }
    *band = j;
    *alpha = a;
}

// One tap of a pixel's gather into its per-image cascade sums: the sample's two shares times the
// filter weight, (alpha v) w, each added to its own cascade's sum. The selects unroll, so the sums
// stay in registers whatever the band.
__device__ __forceinline__ void firefly_tap(V3 (&sum)[kFireflyMaxCascades], V3 v, float alpha, uint32_t band, float w)
{
    const float beta = 1.0f - alpha;
    const V3 lo = mk(v.x * alpha, v.y * alpha, v.z * alpha) * w;
    const V3 hi = mk(v.x * beta, v.y * beta, v.z * beta) * w;
#pragma unroll
    for (int j = 0; j < kFireflyMaxCascades; ++j) {
        const bool isLo = band == (uint32_t)j, isHi = band + 1u == (uint32_t)j;
        if (isLo || isHi) sum[j] = sum[j] + (isLo ? lo : hi);
    }
}

// The cascade pass: film_pass's gather (same tiles, same windows, same filter weight, images in
// order, window rows then columns, a per-image sum added to the accumulator) into the K cascade
// films. A sample's band and alpha are computed once, when it is staged; wide filters take the
// direct gather and split per tap. Cascade .w is left as it is (0 from the clear): the film's .w is
// the weight sum of every cascade.
__global__ __launch_bounds__(kFilmThreads) void film_cascade_kernel(Film film, CascadeFilms cas, FireflyConsts ff, const FilterConsts* fcon,
                                                                    uint32_t images, const Globals* guard,
                                                                    const float2* const* __restrict__ posList,
                                                                    const float4* const* __restrict__ valList)
{
    if (guard && (!guard->imageComplete || guard->skipFilm)) return;
    const uint32_t count = guard ? guard->batchImages : images;
    const FilterConsts c = *fcon;
    const uint32_t W = film.width, H = film.height;
    const uint32_t total = W * H;
    const uint32_t tilesX = (W + kFilmTile - 1) / kFilmTile, tiles = tilesX * ((H + kFilmTile - 1) / kFilmTile);
    // two tile buffers, so one barrier per image separates a buffer's writes from its reads
    __shared__ float2 tPos[2][kFilmSpan * kFilmSpan];
    __shared__ float4 tVal[2][kFilmSpan * kFilmSpan];    // (v.rgb, alpha)
    __shared__ uint32_t tBand[2][kFilmSpan * kFilmSpan];
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int x0 = (int)(tile % tilesX) * kFilmTile, y0 = (int)(tile / tilesX) * kFilmTile;
        const uint32_t px = (uint32_t)x0 + (threadIdx.x % kFilmTile), py = (uint32_t)y0 + (threadIdx.x / kFilmTile);
        const bool mine = px < W && py < H && !(film.rowOwned && !film.rowOwned[py]);
        const size_t p = (size_t)py * W + px;
        int xs = 0, xe = -1, ys = 0, ye = -1;
        V3 acc[kFireflyMaxCascades];
#pragma unroll
        for (int j = 0; j < kFireflyMaxCascades; ++j) acc[j] = mk(0.0f, 0.0f, 0.0f);
        if (mine) {
            film_pixel_window(c, px, py, W, H, &xs, &xe, &ys, &ye);
#pragma unroll
            for (int j = 0; j < kFireflyMaxCascades; ++j)
                if ((uint32_t)j < ff.cascades) {
                    const float4 a = cas.film[j][p];
                    acc[j] = mk(a.x, a.y, a.z);
                }
        }
        const float cx = (float)px + 0.5f, cy = (float)py + 0.5f;
        // the tile's staged span, as film_pass takes it
        int txs, txe, tys, tye, unused0, unused1;
        film_pixel_window(c, (uint32_t)x0, (uint32_t)y0, W, H, &txs, &unused0, &tys, &unused1);
        film_pixel_window(c, min((uint32_t)x0 + kFilmTile - 1u, W - 1u), min((uint32_t)y0 + kFilmTile - 1u, H - 1u), W, H,
                          &unused0, &txe, &unused1, &tye);
        const int spanX = txe - txs + 1, spanY = tye - tys + 1;
        const bool staged = spanX <= kFilmSpan && spanY <= kFilmSpan;
        const int nStage = spanX * spanY;
        for (uint32_t b = 0; b < count; ++b) {
            const float2* sPos = posList ? posList[b] : film.samplePosition + (size_t)b * total;
            const float4* sVal = valList ? valList[b] : film.sampleValue + (size_t)b * total;
            V3 sum[kFireflyMaxCascades];
#pragma unroll
            for (int j = 0; j < kFireflyMaxCascades; ++j) sum[j] = mk(0.0f, 0.0f, 0.0f);
            if (staged) {
                const uint32_t buf = b & 1u;
                for (int i = (int)threadIdx.x; i < nStage; i += kFilmThreads) {
                    const size_t q = (size_t)(tys + i / spanX) * W + (size_t)(txs + i % spanX);   // inside the film by construction
                    const float4 sv = sVal[q];
                    uint32_t band;
                    float alpha;
                    firefly_split(ff, firefly_luminance(sv.x, sv.y, sv.z), &band, &alpha);
                    tPos[buf][i] = sPos[q];
                    tVal[buf][i] = make_float4(sv.x, sv.y, sv.z, alpha);
                    tBand[buf][i] = band;
                }
                __syncthreads();   // (buffer `buf` was last read at image b - 2, before image b - 1's barrier)
                for (int y = ys; y <= ye; ++y)
                    for (int x = xs; x <= xe; ++x) {
                        const int i = (y - tys) * spanX + (x - txs);
                        const float2 sp = tPos[buf][i];
                        const float4 sv = tVal[buf][i];
                        const float w = evaluate_filter(c, cx - (sp.x + (float)x), cy - (sp.y + (float)y));
                        firefly_tap(sum, mk(sv.x, sv.y, sv.z), sv.w, tBand[buf][i], w);
                    }
            } else {
                // wide filters: the direct gather from memory
                for (int y = ys; y <= ye; ++y)
                    for (int x = xs; x <= xe; ++x) {
                        const size_t q = (size_t)y * W + x;
                        const float2 sp = sPos[q];
                        const float4 sv = sVal[q];
                        uint32_t band;
                        float alpha;
                        firefly_split(ff, firefly_luminance(sv.x, sv.y, sv.z), &band, &alpha);
                        const float w = evaluate_filter(c, cx - (sp.x + (float)x), cy - (sp.y + (float)y));
                        firefly_tap(sum, mk(sv.x, sv.y, sv.z), alpha, band, w);
                    }
            }
#pragma unroll
            for (int j = 0; j < kFireflyMaxCascades; ++j) acc[j] = acc[j] + sum[j];
        }
        if (mine) {
#pragma unroll
            for (int j = 0; j < kFireflyMaxCascades; ++j)
                if ((uint32_t)j < ff.cascades) {
                    float4* dst = cas.film[j] + p;
                    dst->x = acc[j].x; dst->y = acc[j].y; dst->z = acc[j].z;
                }
        }
        __syncthreads();   // the tile buffers are reused by the next tile
    }
}

// The resolve (dcrt.h): one thread per pixel of a 16 x 16 tile. The counts count_i(q) of the tile
// plus a one-pixel ring are staged in LDS -- each costs a division and is read by up to nine
// pixels -- and every pixel then sums its 3 x 3 from there.
constexpr int kFireflyTile = 16;
constexpr int kFireflySpan = kFireflyTile + 2;
__global__ __launch_bounds__(kFireflyTile * kFireflyTile) void firefly_resolve_kernel(const float4* __restrict__ film, CascadeFilms cas,
                                                                                      FireflyConsts ff, float imageCount, uint32_t W, uint32_t H,
                                                                                      float4* __restrict__ out)
{
    __shared__ float cnt[kFireflyMaxCascades][kFireflySpan * kFireflySpan];
    const int x0 = (int)blockIdx.x * kFireflyTile, y0 = (int)blockIdx.y * kFireflyTile;
    for (int i = (int)threadIdx.x; i < kFireflySpan * kFireflySpan; i += kFireflyTile * kFireflyTile) {
        const int qx = x0 - 1 + i % kFireflySpan, qy = y0 - 1 + i / kFireflySpan;
        const bool inside = qx >= 0 && qy >= 0 && qx < (int)W && qy < (int)H;
        const size_t q = inside ? (size_t)qy * W + (size_t)qx : 0;
        const float wq = inside ? film[q].w : 0.0f;
        const bool valid = wq > 0.0f;
#pragma unroll
        for (int j = 0; j < kFireflyMaxCascades; ++j) {
            float n = 0.0f;
            if (valid && (uint32_t)j < ff.cascades) {
                const float4 cq = cas.film[j][q];
                n = (imageCount * firefly_luminance(cq.x, cq.y, cq.z)) / (wq * ff.scale[j]);
            }
            if ((uint32_t)j < ff.cascades) cnt[j][i] = n;   // (the rows past K are never read)
        }
    }
    __syncthreads();
    const int tx = (int)threadIdx.x % kFireflyTile, ty = (int)threadIdx.x / kFireflyTile;
    const uint32_t px = (uint32_t)(x0 + tx), py = (uint32_t)(y0 + ty);
    if (px >= W || py >= H) return;
    const size_t p = (size_t)py * W + px;
    const float wp = film[p].w;
    if (!(wp > 0.0f)) { out[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); return; }
    // T_i = the 3 x 3 sum of count_i, rows then columns
    float T[kFireflyMaxCascades];
#pragma unroll
    for (int j = 0; j < kFireflyMaxCascades; ++j) {
        float s = 0.0f;
        if ((uint32_t)j < ff.cascades)
            for (int dy = 0; dy < 3; ++dy)
                for (int dx = 0; dx < 3; ++dx) s = s + cnt[j][(ty + dy) * kFireflySpan + (tx + dx)];
        T[j] = s;
    }
    V3 sum = mk(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int j = 0; j < kFireflyMaxCascades; ++j) {
        if ((uint32_t)j < ff.cascades) {
            const float4 cj = cas.film[j][p];
            if (j == 0) {
                sum = mk(cj.x, cj.y, cj.z);   // omega_0 = 1
            } else {
                // S_j = T_{j-1} + T_j + T_{j+1}, in that order (no T_K: the last cascade has two terms)
                float S = T[j - 1] + T[j];
                if ((uint32_t)j + 1u < ff.cascades) S = S + T[j + 1 < kFireflyMaxCascades ? j + 1 : j];
                const float omega = fminf(fmaxf((S - 1.0f) / ff.minSupport, 0.0f), 1.0f);
                sum = sum + mk(cj.x, cj.y, cj.z) * omega;
            }
        }
    }
    out[p] = make_float4(sum.x / wp, sum.y / wp, sum.z / wp, 1.0f);
}

// film += src (dcrt_tracer_add_film_device): the films of disjoint film partitions
__global__ void add_film_kernel(float4* film, const float4* src, uint32_t n)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 a = film[i], b = src[i];
        film[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
}

// After the film pass of a completed batch: the next batch's first frame seed and
// size, rewind the block cursors.
__global__ void advance_image_kernel(FrameConstants* fc, Globals* g)
{
    if (threadIdx.x != 0 || !g->imageComplete) return;
    g->imageComplete = 0u;
    g->imagesDone += g->batchImages;
    if (g->imagesDone < g->imageTarget) {
        fc->frameSeed = g->seedBase + g->imagesDone * fc->seedStride;
        g->batchImages = min(g->batchCap, g->imageTarget - g->imagesDone);
        g->totalBlocks = fc->blocksPerImage * g->batchImages;
        begin_batch_claims(g);
    } else {
        g->stopped = 1u;
    }
}

__global__ void begin_images_kernel(Globals* g, const FrameConstants* fc, uint32_t count, uint32_t firstSeed, uint32_t batchCap,
                                    uint32_t staticGrid, uint32_t skipFilm, uint32_t filmImageBase)
{
    if (threadIdx.x != 0) return;
    g->skipFilm = skipFilm;
    g->filmImageBase = filmImageBase;
    g->imagesDone = 0u;
    g->imageTarget = count;
    g->seedBase = firstSeed;
    g->batchCap = batchCap;
    g->batchImages = min(batchCap, count);
    g->totalBlocks = fc->blocksPerImage * g->batchImages;
    g->stopped = count == 0u ? 1u : 0u;
    g->imageComplete = 0u;
    g->staticGrid = staticGrid;
    begin_batch_claims(g);
}

// ---- post-processing: SumLuminance.hlsl + PostProcessings.hlsl ---------------------------
__device__ __forceinline__ float4 film_load(const float4* film, uint32_t W, uint32_t H, uint32_t x, uint32_t y)
{
    return (x < W && y < H) ? film[(size_t)y * W + x] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // OOB Load -> 0
}
__device__ __forceinline__ float lum_log(float4 s)            // SumLuminance.hlsl:29-44
{
    V3 c = mk(0.0f, 0.0f, 0.0f);
    if (s.w > 0.0f) c = mk(s.x / s.w, s.y / s.w, s.z / s.w);
    c = mk(fminf(fmaxf(c.x, 0.0f), 65000.0f), fminf(fmaxf(c.y, 0.0f), 65000.0f), fminf(fmaxf(c.z, 0.0f), 65000.0f));
    const float lum = c.x * 0.299f + c.y * 0.587f + c.z * 0.114f;
    return det_log(0.0001f + lum);
}
// REDUCE_TO_1D: 8x8 groups, each thread four film texels, LDS tree 64 -> 1 (same order as the shader)
__global__ __launch_bounds__(64) void luminance_1d_kernel(const float4* film, uint32_t W, uint32_t H, uint32_t bx, uint32_t by, float* out)
{
    __shared__ float acc[64];
    const uint32_t tx = threadIdx.x & 7u, ty = threadIdx.x >> 3;
    const uint32_t x = blockIdx.x * 8 + tx, y = blockIdx.y * 8 + ty;
    float v = lum_log(film_load(film, W, H, x, y));
    v = v + lum_log(film_load(film, W, H, x + 8 * bx, y));
    v = v + lum_log(film_load(film, W, H, x, y + 8 * by));
    v = v + lum_log(film_load(film, W, H, x + 8 * bx, y + 8 * by));
    acc[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t k = 32; k >= 1; k >>= 1) {
        if (threadIdx.x < k) acc[threadIdx.x] = acc[threadIdx.x] + acc[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.y * bx + blockIdx.x] = acc[0];
}
// REDUCE_TO_SINGLE: 128-thread groups, LDS tree 128 -> 1
__global__ __launch_bounds__(128) void luminance_single_kernel(const float* in, uint32_t count, float* out)
{
    __shared__ float acc[128];
    const uint32_t i = blockIdx.x * 128 + threadIdx.x;
    acc[threadIdx.x] = i < count ? in[i] : 0.0f;
    __syncthreads();
    for (uint32_t k = 64; k >= 1; k >>= 1) {
        if (threadIdx.x < k) acc[threadIdx.x] = acc[threadIdx.x] + acc[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = acc[0];
}

// ---- film noise estimate (dcrt.h "film noise estimate"; tests/noise_ref.py restates it) -------
constexpr int kNoiseTile = 16;
struct NoiseTotals { uint32_t valid, converged; float total, maxError, maxTileError; };
// A pixel's error e of the film value f against the half film's h (dcrt.h): false, and e left
// alone, for an invalid pixel (either weight not positive).
__device__ __forceinline__ bool noise_pixel_error(float4 f, float4 h, float* e)
{
    if (!(f.w > 0.0f && h.w > 0.0f)) return false;
    const float cr = f.x / f.w, cg = f.y / f.w, cb = f.z / f.w;
    const float ar = h.x / h.w, ag = h.y / h.w, ab = h.z / h.w;
    const float d = (fabsf(cr - ar) + fabsf(cg - ag)) + fabsf(cb - ab);
    const float s = (cr + cg) + cb;
    const float n = sqrtf(fmaxf(s, 0.0f));
    *e = d / (n + 1e-4f);
    return true;
}
// One 16x16 pixel tile per workgroup: the per-pixel error e of the film against its half film,
// the tile's sum of e (LDS tree 128 -> 1), valid / converged counts and fmaxf maximum.
__global__ __launch_bounds__(kNoiseTile * kNoiseTile) void noise_tile_kernel(const float4* film, const float4* half, uint32_t W, uint32_t H,
                                                                          float threshold, float* pixelMap, float* tileMap,
                                                                          float* tileSum, float* tileMax, float* tileErr,
                                                                          uint32_t* tileCounts)
{
    __shared__ float acc[kNoiseTile * kNoiseTile];
    __shared__ float top[kNoiseTile * kNoiseTile];
    __shared__ uint32_t cnt[2][kNoiseTile * kNoiseTile];
    const uint32_t t = threadIdx.x;
    const uint32_t x = blockIdx.x * kNoiseTile + (t % kNoiseTile), y = blockIdx.y * kNoiseTile + (t / kNoiseTile);
    float e = 0.0f;
    uint32_t valid = 0u, converged = 0u;
    if (x < W && y < H) {
        const size_t p = (size_t)y * W + x;
        if (noise_pixel_error(film[p], half[p], &e)) {
            valid = 1u;
            converged = e <= threshold ? 1u : 0u;
        }
        if (pixelMap) pixelMap[p] = e;
    }
    acc[t] = e;
    top[t] = fmaxf(0.0f, e);
    cnt[0][t] = valid;
    cnt[1][t] = converged;
    __syncthreads();
    for (uint32_t k = kNoiseTile * kNoiseTile / 2; k >= 1; k >>= 1) {
        if (t < k) {
            acc[t] = acc[t] + acc[t + k];
            top[t] = fmaxf(top[t], top[t + k]);
            cnt[0][t] += cnt[0][t + k];
            cnt[1][t] += cnt[1][t + k];
        }
        __syncthreads();
    }
    if (t == 0) {
        const uint32_t tile = blockIdx.y * gridDim.x + blockIdx.x;
        const float err = cnt[0][0] ? acc[0] / (float)cnt[0][0] : 0.0f;
        tileSum[tile] = acc[0];
        tileMax[tile] = top[0];
        tileErr[tile] = err;
        tileCounts[2 * tile] = cnt[0][0];
        tileCounts[2 * tile + 1] = cnt[1][0];
        if (tileMap) tileMap[tile] = err;
    }
}
// The whole image: integer sums of the tiles' counts, fmaxf maxima (both independent of the
// order), and the total that luminance_single_kernel's passes left in *total. One workgroup.
__global__ __launch_bounds__(256) void noise_finish_kernel(const float* tileMax, const float* tileErr, const uint32_t* tileCounts,
                                                           uint32_t tiles, const float* total, NoiseTotals* out)
{
    __shared__ float top[2][256];
    __shared__ uint32_t cnt[2][256];
    const uint32_t t = threadIdx.x;
    float m0 = 0.0f, m1 = 0.0f;
    uint32_t v = 0u, c = 0u;
    for (uint32_t i = t; i < tiles; i += 256u) {
        m0 = fmaxf(m0, tileMax[i]);
        m1 = fmaxf(m1, tileErr[i]);
        v += tileCounts[2 * i];
        c += tileCounts[2 * i + 1];
    }
    top[0][t] = m0; top[1][t] = m1; cnt[0][t] = v; cnt[1][t] = c;
    __syncthreads();
    for (uint32_t k = 128; k >= 1; k >>= 1) {
        if (t < k) {
            top[0][t] = fmaxf(top[0][t], top[0][t + k]);
            top[1][t] = fmaxf(top[1][t], top[1][t + k]);
            cnt[0][t] += cnt[0][t + k];
            cnt[1][t] += cnt[1][t + k];
        }
        __syncthreads();
    }
    if (t == 0) {
        out->valid = cnt[0][0];
        out->converged = cnt[1][0];
        out->total = total[0];
        out->maxError = top[0][0];
        out->maxTileError = top[1][0];
    }
}

// ---- adaptive sampling (dcrt.h "adaptive sampling"; tests/adaptive_ref.py restates it) --------
// One flag per 8x8 pixel block of a W x H film: 1 while some film pixel within `margin` pixels of
// the block is not converged -- invalid, or !(e <= threshold), so a NaN e counts -- else 0. One
// wave per block, its lanes striding over the block's window (clamped to the film), leaving at
// the first chunk that holds such a pixel. No barrier: a wave past the last block just returns.
__global__ __launch_bounds__(256) void sample_mask_kernel(const float4* film, const float4* half, uint32_t W, uint32_t H, float threshold,
                                                          uint32_t margin, uint32_t blocksX, uint32_t blocks, uint32_t* flags)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t b = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (b >= blocks) return;
    const uint32_t by = b / blocksX, bx = b - by * blocksX;
    const uint32_t bx0 = bx * kBlockW, by0 = by * kBlockH;
    const uint32_t x0 = bx0 > margin ? bx0 - margin : 0u, y0 = by0 > margin ? by0 - margin : 0u;
    const uint32_t x1 = (uint32_t)min((unsigned long long)bx0 + (kBlockW - 1u) + margin, (unsigned long long)W - 1u);
    const uint32_t y1 = (uint32_t)min((unsigned long long)by0 + (kBlockH - 1u) + margin, (unsigned long long)H - 1u);
    const uint32_t ww = x1 - x0 + 1u, n = ww * (y1 - y0 + 1u);   // (<= W * H <= 65535^2: base + 64 cannot wrap)
    uint32_t active = 0u;
    for (uint32_t base = 0; base < n; base += 64u) {
        const uint32_t i = base + lane;
        bool noisy = false;
        if (i < n) {
            const uint32_t wy = i / ww, wx = i - wy * ww;
            const size_t p = (size_t)(y0 + wy) * W + (x0 + wx);
            float e = 0.0f;
            noisy = !noise_pixel_error(film[p], half[p], &e) || !(e <= threshold);
        }
        if (__ballot(noisy) != 0ull) { active = 1u; break; }
    }
    if (lane == 0) flags[b] = active;
}

// The flags' ascending list of active blocks: one workgroup walks the flags 256 at a time, a
// wave ballot + mbcnt gives each active block its place in its wave, an LDS scan of the four wave
// counts its place in the chunk. out[0] = the count, out[1] = the in-film pixels of the listed
// blocks (the paths an image starts; partial edge blocks count their pixels inside the film).
__global__ __launch_bounds__(256) void compact_blocks_kernel(const uint32_t* flags, uint32_t blocks, uint32_t blocksX, uint32_t W, uint32_t H,
                                                             uint32_t* list, uint32_t* out)
{
    __shared__ uint32_t ws[4];
    __shared__ uint32_t pix[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t base = 0u, pixels = 0u;
    for (uint32_t start = 0; start < blocks; start += 256u) {
        const uint32_t i = start + threadIdx.x;
        const bool a = i < blocks && flags[i] != 0u;
        const unsigned long long m = __ballot(a);
        const uint32_t x = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (lane == 0) ws[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t off = 0u, total = 0u;
        for (uint32_t w = 0; w < 4u; ++w) {
            const uint32_t c = ws[w];
            off += w < wave ? c : 0u;
            total += c;
        }
        if (a) {
            list[base + off + x] = i;
            const uint32_t by = i / blocksX, bx = i - by * blocksX;
            pixels += min(kBlockW, W - bx * kBlockW) * min(kBlockH, H - by * kBlockH);
        }
        base += total;
        __syncthreads();   // (ws is rewritten by the next chunk)
    }
    const uint32_t s = (uint32_t)wave_sum(pixels);   // (<= W * H < 2^32)
    if (lane == 0) pix[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = base;
        out[1] = (pix[0] + pix[1]) + (pix[2] + pix[3]);
    }
}

// Every block active: flags 1, list 0 .. blocks-1 (the list before any mask, and after a clear)
__global__ void all_blocks_kernel(uint32_t* flags, uint32_t* list, uint32_t blocks)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < blocks; i += gridDim.x * blockDim.x) {
        flags[i] = 1u;
        list[i] = i;
    }
}

// The sentinel sample -- position (+inf, +inf), value 0, which every reconstruction filter weighs
// with exactly +0 -- into the pixels of the inactive blocks of `slots` sample images, so that a
// film pass over the slots adds nothing for the pixels no path was started in.
__global__ __launch_bounds__(256) void fill_inactive_samples_kernel(float2* pos, float4* val, const uint32_t* flags, uint32_t W, uint32_t H,
                                                                    uint32_t blocksX, uint32_t slots)
{
    const uint32_t total = W * H;
    const float2 sp = make_float2(inf(), inf());
    const float4 sv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (unsigned long long pp = blockIdx.x * blockDim.x + threadIdx.x; pp < total; pp += gridDim.x * blockDim.x) {
        const uint32_t p = (uint32_t)pp;
        const uint32_t y = p / W, x = p - y * W;
        if (flags[(y / kBlockH) * blocksX + x / kBlockW] != 0u) continue;
        for (uint32_t s = 0; s < slots; ++s) {
            const size_t q = (size_t)s * total + p;
            pos[q] = sp;
            val[q] = sv;
        }
    }
}

// MainPS: rgb / w -> exposure -> Reinhard -> R8G8B8A8_UNORM_SRGB (encode by host-made thresholds)
__global__ __launch_bounds__(256) void postfx_kernel(const float4* film, uint32_t W, uint32_t H, int enabled, int autoExposure,
                                                     float ev100, float maxWhiteSqr, const float* sumLogLum,
                                                     const float* thresholds, uchar4* out)
{
    __shared__ float th[255];
    for (uint32_t t = threadIdx.x; t < 255; t += blockDim.x) th[t] = thresholds[t];
    __syncthreads();
    float exposure = 1.0f;
    if (enabled) {
        float e = ev100;
        if (autoExposure) {
            const float recip = 1.0f / (float)(W * H);
            const float avgLum = det_exp(sumLogLum[0] * recip);
            e = det_log(avgLum * 100.0f / 12.5f) * 1.44269504088896341f;
        }
        const float maxLuminance = 1.2f * det_exp(e * 0.693147180559945309f);
        exposure = 1.0f / maxLuminance;
    }
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < W * H; p += gridDim.x * blockDim.x) {
        const float4 f = film[p];
        float c[3] = { f.x / f.w, f.y / f.w, f.z / f.w };
        uint32_t code[3];
        for (int k = 0; k < 3; ++k) {
            float v = c[k];
            if (enabled) {
                v = v * exposure;
                v = v * (1.0f + v / maxWhiteSqr) / (1.0f + v);
            }
            v = v != v ? 0.0f : fminf(fmaxf(v, 0.0f), 1.0f);
            uint32_t n = 0;
            for (int t = 0; t < 255; ++t) n += v >= th[t] ? 1u : 0u;
            code[k] = n;
        }
        out[p] = make_uchar4((unsigned char)code[0], (unsigned char)code[1], (unsigned char)code[2], 255);
    }
}

// ---- BxDF LUT integration (BxDFTexturesBuilding.hlsl, "%f" defines) -------------------------
__global__ void lut_integrate_kernel(int which, uint32_t texels, float* out)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= texels) return;
    const float ix = 0.032258f;
    const float iy = which == 0 ? 0.032258f : 0.066667f;
    const float iz = which == 0 ? 1.0f : 0.133333f;
    const float sz = which == 0 ? 0.0f : 1.0f;
    const double weight = which == 2 ? 0.000010 : 0.000049;
    const uint32_t batches = which == 2 ? 24u : 5u;
    const uint32_t w = 32, h = which == 0 ? 32u : 16u;
    const uint32_t slice = t / (w * h), rem = t % (w * h);
    const uint32_t ty = rem / w, tx = rem % w;
    const bool entering = slice >= 16;
    const uint32_t tz = slice & 15u;
    const float cosThetaO = fmaxf((float)tx * ix, 0.0001f);
    const float alpha = (float)ty * iy;
    const float ior = (float)tz * iz + sz;
    const bool smooth = alpha < 0.00052441f;
    float acc = 0.0f;
    for (uint32_t batch = 0; batch < batches; ++batch) {
        Rng rng = rng_init(0, 0, batch);
        double result = batch == 0 ? 0.0 : (double)acc;
        for (uint32_t i = 0; i < 4096; ++i) {
            const V3 wo = mk(sqrtf(1.0f - cosThetaO * cosThetaO), 0.0f, cosThetaO);
            V3 wi = mk(0.0f, 0.0f, 0.0f);
            LCtx c; c.H = mk(0.0f, 0.0f, 0.0f); c.WOdotH = 0.0f;
            float value = 0.0f, pdf = 0.0f;
            if (which != 2) {
                if (smooth) {
                    wi = specular_brdf_sample(wo, &value, &pdf, c);
                } else {
                    const float sx = next1(rng), sy = next1(rng);
                    const V3 m = sample_vndf(wo, sx, sy, alpha);
                    wi = -reflect(wo, m);
                    c.H = m; c.WOdotH = dot(m, wo);
                    value = ct_brdf(wi, wo, alpha, c);
                    pdf = ct_brdf_pdf(true, wi, wo, alpha, c);
                }
                if (pdf > 0.0f) {
                    if (which == 1) {
                        const float etaO = entering ? ior : 1.0f, etaI = entering ? 1.0f : ior;
                        value = value * fresnel_dielectric(c.WOdotH, etaO, etaI);
                    }
                    result += weight * (double)value * (double)fabsf(wi.z) / (double)pdf;
                }
            } else {
                const float etaO = entering ? ior : 1.0f, etaI = entering ? 1.0f : ior;
                const float sel = next1(rng);
                if (smooth) {
                    wi = specular_bsdf_sample<true>(wo, sel, etaO, etaI, false, &value, &pdf, c);
                } else {
                    const float sx = next1(rng), sy = next1(rng);
                    wi = ct_bsdf_sample(true, wo, sel, sx, sy, alpha, etaO, etaI, c);
                    value = ct_bsdf<true>(wi, wo, alpha, etaO, etaI);
                    pdf = ct_bsdf_pdf(true, wi, wo, alpha, etaO, etaI);
                }
                if (pdf > 0.0f) result += weight * (double)value * (double)fabsf(wi.z) / (double)pdf;
            }
        }
        acc = (float)result;
    }
    out[t] = acc;
}

__device__ __forceinline__ uint16_t to_unorm16(float f) { return (uint16_t)rintf(saturate(f) * 65535.0f); }
__device__ __forceinline__ float average_row(const float* row)
{
    const uint32_t n = 31;
    const double fa = (double)(row[0] * 0.0001f);
    double sum = 0.0;
    for (uint32_t i = 1; i < n; ++i) {
        const double cosTheta = (double)((float)i * 0.032258f);
        sum += (double)saturate(row[i]) * cosTheta;
    }
    const double fb = (double)row[n];
    const double result = (sum + (fa + fb) * 0.5) * (double)(1.0f / (float)n);
    return (float)(result * 2.0);
}
__global__ void lut_finalize_kernel(const float* brdf, const float* brdfd, const float* bsdf, dcrt_bxdf_luts* L)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < DCRT_LUT_BRDF_COUNT) L->brdf[t] = to_unorm16(brdf[t]);
    if (t < DCRT_LUT_BRDF_DIELECTRIC_COUNT) { L->brdf_dielectric[t] = to_unorm16(brdfd[t]); L->bsdf[t] = to_unorm16(bsdf[t]); }
    if (t < 32) L->brdf_avg[t] = to_unorm16(average_row(brdf + t * 32));
    if (t < 512) {
        const uint32_t z = t / 16, y = t % 16;
        const uint32_t dest = (z / 16) * 256 + (z % 16) * 16 + y;
        L->brdf_dielectric_avg[dest] = to_unorm16(average_row(brdfd + (size_t)z * 512 + y * 32));
        L->bsdf_avg[dest] = to_unorm16(average_row(bsdf + (size_t)z * 512 + y * 32));
    }
}

// ---- film denoiser: variance-guided, edge-avoiding a-trous wavelet filter ------------------
// (Dammertz et al. 2010 with the spatial variance guidance of SVGF, Schied et al. 2017; no
// temporal part.) dcrt.h states the arithmetic; tests/denoise_ref.py restates it in numpy
// float32, and every kernel below computes a pixel with the same operations in the same order
// -- each thread sums its own pixel's taps sequentially (rows outer, columns inner, ascending),
// whatever the staging, so all variants give the same bits. Taps outside the image are skipped.
// Working image: (c.rgb, var) per pixel plus the decoded guides (n.xyz, 0), (a.xyz, 0).
struct DenoiseConsts { float sigmaL, kn, ka; uint32_t demodulate; };

constexpr int kDnTile = 16;                       // a workgroup: 16 x 16 pixels (or lattice points), one per thread
constexpr int kDnThreads = kDnTile * kDnTile;
constexpr int kDnVarHalo = 3;                     // the variance estimate's 7 x 7 window

DEV float dn_lum(float4 c) { return c.x * 0.299f + c.y * 0.587f + c.z * 0.114f; }
DEV float dn_dist2(float4 q, float4 p)
{
    const float x = q.x - p.x, y = q.y - p.y, z = q.z - p.z;
    return x * x + y * y + z * z;
}
DEV V3 dn_resolve(float4 f) { return f.w > 0.0f ? mk(f.x / f.w, f.y / f.w, f.z / f.w) : mk(0.0f, 0.0f, 0.0f); }
DEV V3 dn_demodulation(float4 a, uint32_t demodulate)
{
    return demodulate ? mk(fmaxf(a.x, 1e-3f), fmaxf(a.y, 1e-3f), fmaxf(a.z, 1e-3f)) : mk(1.0f, 1.0f, 1.0f);
}

// Resolve the three films and pack the working image: c0 = c / d, var = 0 (the variance kernel fills it in)
__global__ __launch_bounds__(256) void denoise_prologue_kernel(const float4* __restrict__ color, const float4* __restrict__ normal,
                                                               const float4* __restrict__ albedo, uint32_t n, uint32_t demodulate,
                                                               float4* __restrict__ cv, float4* __restrict__ gn, float4* __restrict__ ga)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const V3 c = dn_resolve(color[i]), nr = dn_resolve(normal[i]), a = dn_resolve(albedo[i]);
        const float4 a4 = make_float4(a.x, a.y, a.z, 0.0f);
        const V3 d = dn_demodulation(a4, demodulate);
        cv[i] = make_float4(c.x / d.x, c.y / d.y, c.z / d.z, 0.0f);
        gn[i] = make_float4(2.0f * nr.x - 1.0f, 2.0f * nr.y - 1.0f, 2.0f * nr.z - 1.0f, 0.0f);
        ga[i] = a4;
    }
}

// Where a pixel's taps come from. tap(): the tap at pixel (qx, qy) = p + step * (dx, dy), inside
// the image; var(): var of the pixel at p + (dx, dy), inside the image (the 3 x 3 prefilter).
struct DnGlobalSrc {
    const float4 *cv, *gn, *ga;
    int W;
    DEV void tap(int qx, int qy, int, int, float4* c, float4* n, float4* a) const
    {
        const size_t q = (size_t)qy * W + qx;
        *c = cv[q]; *n = gn[q]; *a = ga[q];
    }
    DEV float var(int qx, int qy, int, int) const { return cv[(size_t)qy * W + qx].w; }
};
// The staged span of a workgroup: span x span lattice points around its 16 x 16, `base` this
// thread's own, a tap `t` points apart. With varStaged the lattice is the pixel grid itself
// (stride 1) and the prefilter's neighbours are staged too; otherwise they come from memory.
struct DnLdsSrc {
    const float4 *sC, *sN, *sA, *cv;
    int base, span, t, W;
    bool varStaged;
    DEV void tap(int, int, int dx, int dy, float4* c, float4* n, float4* a) const
    {
        const int i = base + dy * t * span + dx * t;
        *c = sC[i]; *n = sN[i]; *a = sA[i];
    }
    DEV float var(int qx, int qy, int dx, int dy) const
    {
        return varStaged ? sC[base + dy * span + dx].w : cv[(size_t)qy * W + qx].w;
    }
};

// Stage the lattice points {(ox, oy) + L * (i - halo, j - halo)}, 0 <= i, j < span, that lie in the image
DEV void dn_stage(float4* sC, float4* sN, float4* sA, const float4* __restrict__ cv, const float4* __restrict__ gn,
                  const float4* __restrict__ ga, int ox, int oy, int L, int halo, int span, int W, int H)
{
    for (int e = (int)threadIdx.x; e < span * span; e += kDnThreads) {
        const int j = e / span, i = e - j * span;
        const int qx = ox + (i - halo) * L, qy = oy + (j - halo) * L;
        if (qx >= 0 && qx < W && qy >= 0 && qy < H) {
            const size_t q = (size_t)qy * W + qx;
            sC[e] = cv[q]; sN[e] = gn[q]; sA[e] = ga[q];
        }
    }
    __syncthreads();
}

// var0 of pixel (px, py): the guide-weighted second moment of the luminance over 7 x 7
template <class Src>
DEV float dn_variance_pixel(const DenoiseConsts& k, int px, int py, int W, int H, const Src& src)
{
    float4 cp, np, ap;
    src.tap(px, py, 0, 0, &cp, &np, &ap);
    float m1 = 0.0f, m2 = 0.0f, ws = 0.0f;
    for (int dy = -kDnVarHalo; dy <= kDnVarHalo; ++dy) {
        const int qy = py + dy;
        if (qy < 0 || qy >= H) continue;
        for (int dx = -kDnVarHalo; dx <= kDnVarHalo; ++dx) {
            const int qx = px + dx;
            if (qx < 0 || qx >= W) continue;
            float4 cq, nq, aq;
            src.tap(qx, qy, dx, dy, &cq, &nq, &aq);
            const float wg = det_exp(-(dn_dist2(nq, np) * k.kn + dn_dist2(aq, ap) * k.ka));
            const float l = dn_lum(cq);
            m1 = m1 + l * wg;
            m2 = m2 + l * l * wg;
            ws = ws + wg;
        }
    }
    const float mean = m1 / ws;
    return fmaxf(m2 / ws - mean * mean, 0.0f);
}

// One a-trous pass at pixel (px, py), taps `step` pixels apart: (c_{i+1}.rgb, var_{i+1})
template <class Src>
DEV float4 dn_pass_pixel(const DenoiseConsts& k, int px, int py, int W, int H, int step, const Src& src)
{
    constexpr float h[5] = { 1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f };
    constexpr float g[3] = { 1.0f / 4.0f, 1.0f / 2.0f, 1.0f / 4.0f };
    float gs = 0.0f, gw = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = py + dy;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = px + dx;
            if (qx < 0 || qx >= W) continue;
            const float w = g[dy + 1] * g[dx + 1];
            gs = gs + src.var(qx, qy, dx, dy) * w;
            gw = gw + w;
        }
    }
    const float gv = gs / gw;
    const float kl = k.sigmaL > 0.0f ? 1.0f / (k.sigmaL * sqrtf(gv) + 1e-6f) : 0.0f;
    float4 cp, np, ap;
    src.tap(px, py, 0, 0, &cp, &np, &ap);
    const float lp = dn_lum(cp);
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f, ws = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = py + dy * step;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = px + dx * step;
            if (qx < 0 || qx >= W) continue;
            float4 cq, nq, aq;
            src.tap(qx, qy, dx, dy, &cq, &nq, &aq);
            const float e = fabsf(dn_lum(cq) - lp) * kl + dn_dist2(nq, np) * k.kn + dn_dist2(aq, ap) * k.ka;
            const float w = (h[dy + 2] * h[dx + 2]) * det_exp(-e);
            sx = sx + cq.x * w; sy = sy + cq.y * w; sz = sz + cq.z * w;
            sv = sv + cq.w * (w * w);
            ws = ws + w;
        }
    }
    return make_float4(sx / ws, sy / ws, sz / ws, sv / (ws * ws));
}

// The last pass remodulates: (c_N * d, 1) into the caller's image instead of the working one
DEV void dn_store(float4 r, float4 a, const DenoiseConsts& k, size_t p, float4* __restrict__ dst, float4* __restrict__ finalOut)
{
    if (finalOut) {
        const V3 d = dn_demodulation(a, k.demodulate);
        finalOut[p] = make_float4(r.x * d.x, r.y * d.y, r.z * d.z, 1.0f);
    } else {
        dst[p] = r;
    }
}

// Variance estimate, a 16 x 16 tile plus its 3-pixel halo staged in LDS (22 x 22 x 48 B): dst = (c0, var0)
__global__ __launch_bounds__(kDnThreads) void denoise_variance_kernel(DenoiseConsts k, const float4* __restrict__ cv,
                                                                      const float4* __restrict__ gn, const float4* __restrict__ ga,
                                                                      int W, int H, float4* __restrict__ dst)
{
    constexpr int span = kDnTile + 2 * kDnVarHalo;
    __shared__ float4 sC[span * span], sN[span * span], sA[span * span];
    const int tilesX = (W + kDnTile - 1) / kDnTile;
    const int x0 = (int)(blockIdx.x % (uint32_t)tilesX) * kDnTile, y0 = (int)(blockIdx.x / (uint32_t)tilesX) * kDnTile;
    dn_stage(sC, sN, sA, cv, gn, ga, x0, y0, 1, kDnVarHalo, span, W, H);
    const int li = (int)threadIdx.x % kDnTile, lj = (int)threadIdx.x / kDnTile;
    const int px = x0 + li, py = y0 + lj;
    if (px >= W || py >= H) return;
    const DnLdsSrc src{ sC, sN, sA, cv, (lj + kDnVarHalo) * span + li + kDnVarHalo, span, 1, W, true };
    const float4 c = sC[src.base];
    dst[(size_t)py * W + px] = make_float4(c.x, c.y, c.z, dn_variance_pixel(k, px, py, W, H, src));
}

// A-trous pass, every tap from memory: one thread per pixel of a 16 x 16 tile
__global__ __launch_bounds__(kDnThreads) void denoise_pass_global_kernel(DenoiseConsts k, const float4* __restrict__ cv,
                                                                         const float4* __restrict__ gn, const float4* __restrict__ ga,
                                                                         int W, int H, int step, float4* __restrict__ dst,
                                                                         float4* __restrict__ finalOut)
{
    const int tilesX = (W + kDnTile - 1) / kDnTile;
    const int px = (int)(blockIdx.x % (uint32_t)tilesX) * kDnTile + (int)threadIdx.x % kDnTile;
    const int py = (int)(blockIdx.x / (uint32_t)tilesX) * kDnTile + (int)threadIdx.x / kDnTile;
    if (px >= W || py >= H) return;
    const DnGlobalSrc src{ cv, gn, ga, W };
    const size_t p = (size_t)py * W + px;
    dn_store(dn_pass_pixel(k, px, py, W, H, step, src), ga[p], k, p, dst, finalOut);
}

// A-trous pass from an LDS-staged span (dynamic LDS: 3 x span^2 float4). The workgroup owns
// 16 x 16 points of the lattice {r + L * (i, j)} of residue class r = (rx, ry), 0 <= rx, ry < L:
//   L = 1:    a pixel tile; the taps are step pixels apart, the halo 2 * step (small steps);
//   L = step: the decimated lattice, whose taps are neighbours again: halo 2 at any step.
// blockIdx.x = class * tiles + tile, tiles = tilesX * tilesY over the largest class's lattice.
__global__ __launch_bounds__(kDnThreads) void denoise_pass_staged_kernel(DenoiseConsts k, const float4* __restrict__ cv,
                                                                         const float4* __restrict__ gn, const float4* __restrict__ ga,
                                                                         int W, int H, int step, int L, float4* __restrict__ dst,
                                                                         float4* __restrict__ finalOut)
{
    extern __shared__ float4 dnSpan[];
    const int t = step / L, halo = 2 * t, span = kDnTile + 2 * halo;
    float4 *sC = dnSpan, *sN = sC + span * span, *sA = sN + span * span;
    const int tilesX = ((W + L - 1) / L + kDnTile - 1) / kDnTile, tilesY = ((H + L - 1) / L + kDnTile - 1) / kDnTile;
    const uint32_t tiles = (uint32_t)(tilesX * tilesY);
    const int cls = (int)(blockIdx.x / tiles), tile = (int)(blockIdx.x % tiles);
    const int rx = cls % L, ry = cls / L;
    const int i0 = (tile % tilesX) * kDnTile, j0 = (tile / tilesX) * kDnTile;   // lattice coordinates of the tile
    const int x0 = rx + i0 * L, y0 = ry + j0 * L;
    if (x0 >= W || y0 >= H) return;   // (the whole workgroup: a class or tile without a pixel)
    dn_stage(sC, sN, sA, cv, gn, ga, x0, y0, L, halo, span, W, H);
    const int li = (int)threadIdx.x % kDnTile, lj = (int)threadIdx.x / kDnTile;
    const int px = x0 + li * L, py = y0 + lj * L;
    if (px >= W || py >= H) return;
    const DnLdsSrc src{ sC, sN, sA, cv, (lj + halo) * span + li + halo, span, t, W, L == 1 };
    const size_t p = (size_t)py * W + px;
    dn_store(dn_pass_pixel(k, px, py, W, H, step, src), sA[src.base], k, p, dst, finalOut);
}

// ---- explicit instantiations used by tracer.hip ---------------------------------------
template __global__ void extension_kernel<false, false>(PathPool, DeviceScene, const FrameConstants*, const Counters*, Globals*, unsigned long long*);
template __global__ void extension_kernel<false, true>(PathPool, DeviceScene, const FrameConstants*, const Counters*, Globals*, unsigned long long*);
template __global__ void extension_kernel<true, false>(PathPool, DeviceScene, const FrameConstants*, const Counters*, Globals*, unsigned long long*);
template __global__ void extension_kernel<true, true>(PathPool, DeviceScene, const FrameConstants*, const Counters*, Globals*, unsigned long long*);
template __global__ void shadow_kernel<false, false>(PathPool, DeviceScene, const FrameConstants*, Counters*, Counters*, Globals*, unsigned long long*);
template __global__ void shadow_kernel<false, true>(PathPool, DeviceScene, const FrameConstants*, Counters*, Counters*, Globals*, unsigned long long*);
template __global__ void shadow_kernel<true, false>(PathPool, DeviceScene, const FrameConstants*, Counters*, Counters*, Globals*, unsigned long long*);
template __global__ void shadow_kernel<true, true>(PathPool, DeviceScene, const FrameConstants*, Counters*, Counters*, Globals*, unsigned long long*);
// The compiled cast_kernel variants (INSTR, OPACITY, ALL_CACHED, PAIR, IDENT, RING, FLAT, CELLS): this one list
// instantiates them and is the table that tracer.hip's CastKernel() picks from, in this order.
#define DCRT_CAST_VARIANTS(X)                                   \
    X(false, false, false, false, false, false, false, false)   \
    X(false, false, true, false, false, false, false, false)    \
    X(false, true, false, false, false, false, false, false)    \
    X(false, true, true, false, false, false, false, false)     \
    X(true, false, false, false, false, false, false, false)    \
    X(true, false, true, false, false, false, false, false)     \
    X(true, true, false, false, false, false, false, false)     \
    X(true, true, true, false, false, false, false, false)      \
    X(false, false, false, true, false, false, false, false)    \
    X(false, true, false, true, false, false, false, false)     \
    X(false, false, true, false, true, false, false, false)     \
    X(false, false, true, false, true, false, true, false)      \
    X(false, false, true, false, true, false, true, true)       \
    X(true, false, true, false, true, false, false, false)      \
    X(false, false, false, false, true, false, false, false)    \
    X(true, false, false, false, true, false, false, false)     \
    X(false, false, false, false, false, true, false, false)    \
    X(false, false, false, false, true, true, false, false)     \
    X(false, false, false, true, false, true, false, false)
#define DCRT_INSTANTIATE_CAST(...) \
    template __global__ void cast_kernel<__VA_ARGS__>(PathPool, DeviceScene, const FrameConstants*, Counters*, Counters*, Globals*, unsigned long long*);
DCRT_CAST_VARIANTS(DCRT_INSTANTIATE_CAST)
#undef DCRT_INSTANTIATE_CAST
template __global__ void megakernel<false>(DeviceScene, const FrameConstants*, Film, Globals*, uint32_t);
template __global__ void megakernel<true>(DeviceScene, const FrameConstants*, Film, Globals*, uint32_t);
template __global__ void megakernel<false, kCapAllEnvImportance>(DeviceScene, const FrameConstants*, Film, Globals*, uint32_t);
template __global__ void megakernel<true, kCapAllEnvImportance>(DeviceScene, const FrameConstants*, Film, Globals*, uint32_t);
template __global__ void megakernel<false, kCapAllLightTable>(DeviceScene, const FrameConstants*, Film, Globals*, uint32_t);
template __global__ void megakernel<true, kCapAllLightTable>(DeviceScene, const FrameConstants*, Film, Globals*, uint32_t);
template __global__ void view_kernel<false>(DeviceScene, const FrameConstants*, Film, Globals*, uint32_t, uint32_t, uint32_t);
template __global__ void view_kernel<true>(DeviceScene, const FrameConstants*, Film, Globals*, uint32_t, uint32_t, uint32_t);
template __global__ void batch_trace_kernel<false, false>(DeviceScene, const dcrt_ray*, uint32_t, uint32_t, dcrt_ray_hit*, uint32_t*, unsigned long long*);
template __global__ void batch_trace_kernel<true, false>(DeviceScene, const dcrt_ray*, uint32_t, uint32_t, dcrt_ray_hit*, uint32_t*, unsigned long long*);
template __global__ void batch_trace_kernel<false, true>(DeviceScene, const dcrt_ray*, uint32_t, uint32_t, dcrt_ray_hit*, uint32_t*, unsigned long long*);
template __global__ void batch_trace_kernel<true, true>(DeviceScene, const dcrt_ray*, uint32_t, uint32_t, dcrt_ray_hit*, uint32_t*, unsigned long long*);

}  // namespace dev
}  // namespace dcrt
