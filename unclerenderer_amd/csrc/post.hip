// AutoExposure and CAS for gfx950 — the post chain after Tonemap's input (DeferredRenderer.cpp:1363-1573), and Tonemap+CAS
// fused into one launch.
//
// AutoExposure (Shaders/AutoExposure.hlsl:24-93): ONE workgroup of 16 x 16 lanes, one bilinear tap each, a log2-luminance
// sum in a fixed order (wave64 butterfly, then the four wave sums in LDS in index order) and one float written by lane 0.
// A latency-bound launch of a few microseconds; there is nothing to stream.
//
// CAS (Shaders/Cas.hlsl:67-99): the pixel and its 4-neighbours of the R8G8B8A8_UNORM image, the reference's own amp / w
// formula (not FidelityFX RCAS). The taps are exact texels: the pass samples at pixel centres with TexelDelta = (1/W, 1/H)
// through a clamp sampler, so a tap is the neighbour texel, clamped at the image edges.
//
// Both CAS forms run one kernel, cas_strip_kernel below: a wave owns a 64 * PX-column strip of kRows output rows. It loads
// the kRows + 2 input rows its taps need (rows clamped to the frame) and the texel left and right of the strip in each of
// them in ONE load phase, converts each input row once to fp32 (R, G, B, luminance) and takes the horizontal neighbours
// from the adjacent lanes (DPP wave shifts), the vertical ones from the rows kept in registers. No LDS, no barrier. In the
// fused form an input row is HDR and is converted by the same tonemap_pixel as ur_tonemap (csrc/post_common.h) before
// anything else: the bytes CAS sees are exactly ur_tonemap's, and the intermediate image is never written.
// Bytes per output pixel: CAS 4 read + 4 written (8), fused 8 read + 4 written (12, against 8 + 4 + 4 + 4 = 20 for the two
// launches); the two halo rows of a strip (2 / kRows more rows) are read again by the neighbouring strip's waves and,
// in the fused form, tonemapped twice.
// Built with -ffp-contract=off. The quotients go through v_rcp_f32 and the reciprocal square root through v_rsq_f32 (1 ulp
// each); each output byte stays within one LSB of a scalar fp32 evaluation of the HLSL (tests/post_ref.py).

#include "ur_internal.h"
#include "ur_device.h"
#include "post_common.h"

namespace {

using ur_post::half4_t;
using ur_post::TonemapParams;
using ur_post::tonemap_pixel;
using ur_post::final_exposure;
using ur_post::unorm8;

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

constexpr float kLumR = 0.2126f, kLumG = 0.7152f, kLumB = 0.0722f; // LuminanceWeights / LumCoeff of both shaders

// ---- AutoExposure ---------------------------------------------------------------------------------------------------
struct AeParams {
    const half4_t* hdr;
    const float* prev; // PrevLogAverageLuminance texel, read only with use_history
    float* out;
    uint32_t W, H;
    float size_x, size_y; // InputSize (== W, H)
    float delta_time, speed_up, speed_down;
    uint32_t use_history;
    float key, ev_min, ev_max;
};

__global__ __launch_bounds__(256) void auto_exposure_kernel(AeParams p)
{
    const uint32_t index = threadIdx.x, gx = index & 15u, gy = index >> 4; // GroupThreadId.xy of [numthreads(16,16,1)]
    // AutoExposure.hlsl:27-29
    const float samplePosX = ((float)gx + 0.5f) * (p.size_x / 16.0f), samplePosY = ((float)gy + 0.5f) * (p.size_y / 16.0f);
    const float u = samplePosX / fmaxf(p.size_x, 1.0f), v = samplePosY / fmaxf(p.size_y, 1.0f);
    // SampleLevel(linear, clamp) of mip 0 (the Lighting SRV has one mip, DeferredRenderer.cpp:3006-3007): the 2x2 footprint
    // around t = uv * size - 0.5, indices clamped, weights the fractions of t, blended as two lerps along x then one along y
    const float tx = u * (float)p.W - 0.5f, ty = v * (float)p.H - 0.5f;
    const float fx = floorf(tx), fy = floorf(ty), ax = tx - fx, ay = ty - fy;
    const int ix = (int)fx, iy = (int)fy, mx = (int)p.W - 1, my = (int)p.H - 1;
    const size_t x0 = (size_t)min(max(ix, 0), mx), x1 = (size_t)min(max(ix + 1, 0), mx);
    const size_t y0 = (size_t)min(max(iy, 0), my) * p.W, y1 = (size_t)min(max(iy + 1, 0), my) * p.W;
    const half4_t t00 = p.hdr[y0 + x0], t10 = p.hdr[y0 + x1], t01 = p.hdr[y1 + x0], t11 = p.hdr[y1 + x1];
    float c[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float a = (float)t00[ch], b = (float)t10[ch], d = (float)t01[ch], e = (float)t11[ch];
        const float top = a + ax * (b - a), bottom = d + ax * (e - d);
        c[ch] = top + ay * (bottom - top);
    }
    // :33-34, :38: fmaxf, so a NaN channel counts as 0
    const float luminance = fmaxf(c[0], 0.0f) * kLumR + fmaxf(c[1], 0.0f) * kLumG + fmaxf(c[2], 0.0f) * kLumB;
    float s = log2f(fmaxf(luminance, 1e-4f));
    // WaveActiveSum in a fixed order: lane l adds lane l ^ m for m = 32, 16, ..., 1
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s = s + __shfl_xor(s, m, 64);
    __shared__ float waveSums[4];
    if ((index & 63u) == 0u) waveSums[index >> 6] = s;
    __syncthreads();
    if (index != 0u) return;
    // :65-92
    const float logAverageEv = (((waveSums[0] + waveSums[1]) + waveSums[2]) + waveSums[3]) / 256.0f;
    const float keyEv = log2f(fmaxf(p.key, 1e-4f));
    const float minEv = log2f(fmaxf(p.ev_min, 1e-4f)), maxEv = log2f(fmaxf(p.ev_max, 1e-4f));
    const float targetExposureEv = fminf(fmaxf(keyEv - logAverageEv, minEv), maxEv); // clamp
    float adapted = targetExposureEv;
    if (p.use_history != 0u) {
        const float previousLog = p.prev[0];
        const float speed = targetExposureEv > previousLog ? p.speed_up : p.speed_down;
        const float alpha = 1.0f - expf(-p.delta_time * speed);
        adapted = previousLog + fminf(fmaxf(alpha, 0.0f), 1.0f) * (targetExposureEv - previousLog); // lerp(prev, target, saturate(alpha))
    }
    p.out[0] = adapted;
}

// ---- CAS ------------------------------------------------------------------------------------------------------------
struct Px { float r, g, b, l; }; // a texel (byte / 255) and its luminance dot(rgb, LumCoeff)

__device__ __forceinline__ Px unpack(uint32_t c)
{
    constexpr float k = 1.0f / 255.0f;
    Px p;
    p.r = (float)(c & 255u) * k; p.g = (float)((c >> 8) & 255u) * k; p.b = (float)((c >> 16) & 255u) * k;
    p.l = p.r * kLumR + p.g * kLumG + p.b * kLumB;
    return p;
}

// Cas.hlsl:67-99 for one pixel
__device__ __forceinline__ uint32_t cas_pixel(const Px& C, const Px& N, const Px& W, const Px& E, const Px& S, float sharpness)
{
    constexpr float RcasInvPeak = 1.0f / (8.0f - 3.0f), FsrEps = 0.0001f;
    const float mnR = fminf(fminf(fminf(N.r, W.r), fminf(E.r, S.r)), C.r), mxR = fmaxf(fmaxf(fmaxf(N.r, W.r), fmaxf(E.r, S.r)), C.r);
    const float mnG = fminf(fminf(fminf(N.g, W.g), fminf(E.g, S.g)), C.g), mxG = fmaxf(fmaxf(fmaxf(N.g, W.g), fmaxf(E.g, S.g)), C.g);
    const float mnB = fminf(fminf(fminf(N.b, W.b), fminf(E.b, S.b)), C.b), mxB = fmaxf(fmaxf(fmaxf(N.b, W.b), fmaxf(E.b, S.b)), C.b);
    // amp = rsqrt(saturate(min(minRGB, 2 - maxRGB) * (1 / (maxRGB + eps))) + eps)
    auto amp = [](float mn, float mx) {
        const float a = fminf(fmaxf(fminf(mn, 2.0f - mx) * __builtin_amdgcn_rcpf(mx + FsrEps), 0.0f), 1.0f);
        return __builtin_amdgcn_rsqf(a + FsrEps);
    };
    const float ampR = amp(mnR, mxR), ampG = amp(mnG, mxG), ampB = amp(mnB, mxB);
    const float w = -RcasInvPeak * __builtin_amdgcn_rcpf(ampR * kLumR + ampG * kLumG + ampB * kLumB);
    const float sumL = ((N.l + W.l) + E.l) + S.l;
    const float invDen = __builtin_amdgcn_rcpf(4.0f * w + 1.0f);
    const float sharpL = fminf(fmaxf((sumL * w + C.l) * invDen, 0.0f), 1.0f);
    // outColor = lerp(C, (C - CL) + sharpL, Sharpness)
    const float r = C.r + sharpness * (((C.r - C.l) + sharpL) - C.r);
    const float g = C.g + sharpness * (((C.g - C.l) + sharpL) - C.g);
    const float b = C.b + sharpness * (((C.b - C.l) + sharpL) - C.b);
    return unorm8(r) | (unorm8(g) << 8) | (unorm8(b) << 16) | 0xFF000000u;
}

struct CasParams {
    const void* src;   // FUSED: the full RGBA16F frame; else the full R8G8B8A8 image
    uint32_t* out;     // band rows [row0, row0 + rows)
    uint32_t W, H, row0, rows;
    float sharpness;
    TonemapParams tm;  // FUSED: the Tonemap constants (hdr / out / count unused)
};

constexpr int kRows = 8; // output rows per wave: kRows + 2 input rows in one load phase

// DPP wave shifts (as in csrc/taa.hip): wave_shr:1 - lane l reads lane l - 1, lane 0 keeps `old`; wave_shl:1 - lane l reads
// lane l + 1, lane 63 keeps `old`
__device__ __forceinline__ float shr1(float old, float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v), 0x138, 0xF, 0xF, false));
}
__device__ __forceinline__ float shl1(float old, float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v), 0x130, 0xF, 0xF, false));
}
__device__ __forceinline__ Px shr1(const Px& old, const Px& v) { return Px{shr1(old.r, v.r), shr1(old.g, v.g), shr1(old.b, v.b), shr1(old.l, v.l)}; }
__device__ __forceinline__ Px shl1(const Px& old, const Px& v) { return Px{shl1(old.r, v.r), shl1(old.g, v.g), shl1(old.b, v.b), shl1(old.l, v.l)}; }
__device__ __forceinline__ Px readlane(const Px& v, int lane)
{
    auto rl = [lane](float x) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), lane)); };
    return Px{rl(v.r), rl(v.g), rl(v.b), rl(v.l)};
}

// FUSED: tonemap HDR rows on the way in. PX: pixels per lane - 2 (even width; 16-B aligned HDR / 8-B aligned RGBA8 rows: one
// 16- or 8-byte load and one 8-byte store per lane and row) or 1 (any width and alignment).
template <bool FUSED, int PX>
__global__ __launch_bounds__(256) void cas_strip_kernel(CasParams p)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t x0 = (blockIdx.x * 4u + wave) * (64u * PX); // the wave's first column; the four waves side by side
    if (x0 >= p.W) return;                                     // uniform per wave (no barrier in this kernel)
    const uint32_t rb0 = blockIdx.y * (uint32_t)kRows;          // first output row of the strip, band-local
    const uint32_t nrows = min((uint32_t)kRows, p.rows - rb0);
    const int maxy = (int)p.H - 1;
    const uint32_t maxx = p.W - 1u, px0 = x0 + lane * PX;       // the lane's first column
    const bool beyond = px0 > maxx;                             // lanes right of the frame repeat the last column
    const float finalExposure = FUSED ? final_exposure(p.tm) : 0.0f;
    // input row k (0 .. kRows + 1) = frame row row0 + rb0 - 1 + k, clamped (the taps' clamp at the top and bottom edges)
    auto row_offset = [&](int k) -> size_t { return (size_t)(uint32_t)min(max((int)(p.row0 + rb0) - 1 + k, 0), maxy) * p.W; };
    auto interior = [&](int k) { return k >= 1 && k <= kRows; }; // the strip's own rows (nontemporal; its halo rows are other strips' own)

    // ---- the load phase: kRows + 2 rows, and the texels left / right of the strip (lane j < kRows + 2: row j's left one,
    // lane 32 + j: its right one), all in flight before the first is used
    const uint32_t hx = lane < 32u ? (x0 == 0u ? 0u : x0 - 1u) : min(x0 + 64u * PX, maxx);
    const size_t hoff = row_offset((int)min(lane & 31u, (uint32_t)kRows + 1u)) + hx;
    uint32_t halo;
    Px rowA[kRows + 2], rowB[kRows + 2]; // the lane's pixel(s) of each input row (rowB: PX == 2 only)
    if constexpr (FUSED) {
        const half4_t* hdr = static_cast<const half4_t*>(p.src);
        const half4_t hh = hdr[hoff];
        if constexpr (PX == 2) {
            const u32x4_t* src = static_cast<const u32x4_t*>(p.src);
            const size_t pair = (size_t)(min(px0, maxx - 1u) >> 1);
            u32x4_t v[kRows + 2];
#pragma unroll
            for (int k = 0; k < kRows + 2; ++k) {
                const u32x4_t* a = src + (row_offset(k) >> 1) + pair;
                v[k] = interior(k) ? __builtin_nontemporal_load(a) : *a;
            }
            halo = tonemap_pixel(p.tm, finalExposure, hh);
#pragma unroll
            for (int k = 0; k < kRows + 2; ++k) {
                union { u32x2_t u; half4_t h; } a, b;
                a.u = u32x2_t{v[k].x, v[k].y}; b.u = u32x2_t{v[k].z, v[k].w};
                const uint32_t tb = tonemap_pixel(p.tm, finalExposure, b.h);
                const uint32_t ta = beyond ? tb : tonemap_pixel(p.tm, finalExposure, a.h);
                rowA[k] = unpack(ta); rowB[k] = unpack(tb);
            }
        } else {
            const size_t x = min(px0, maxx);
            half4_t v[kRows + 2];
#pragma unroll
            for (int k = 0; k < kRows + 2; ++k) v[k] = interior(k) ? __builtin_nontemporal_load(hdr + row_offset(k) + x) : hdr[row_offset(k) + x];
            halo = tonemap_pixel(p.tm, finalExposure, hh);
#pragma unroll
            for (int k = 0; k < kRows + 2; ++k) rowA[k] = unpack(tonemap_pixel(p.tm, finalExposure, v[k]));
        }
    } else {
        const uint32_t* ldr = static_cast<const uint32_t*>(p.src);
        halo = ldr[hoff];
        if constexpr (PX == 2) {
            const u32x2_t* src = static_cast<const u32x2_t*>(p.src);
            const size_t pair = (size_t)(min(px0, maxx - 1u) >> 1);
            u32x2_t v[kRows + 2];
#pragma unroll
            for (int k = 0; k < kRows + 2; ++k) {
                const u32x2_t* a = src + (row_offset(k) >> 1) + pair;
                v[k] = interior(k) ? __builtin_nontemporal_load(a) : *a;
            }
#pragma unroll
            for (int k = 0; k < kRows + 2; ++k) { rowA[k] = unpack(beyond ? v[k].y : v[k].x); rowB[k] = unpack(v[k].y); }
        } else {
            const size_t x = min(px0, maxx);
            uint32_t v[kRows + 2];
#pragma unroll
            for (int k = 0; k < kRows + 2; ++k) v[k] = interior(k) ? __builtin_nontemporal_load(ldr + row_offset(k) + x) : ldr[row_offset(k) + x];
#pragma unroll
            for (int k = 0; k < kRows + 2; ++k) rowA[k] = unpack(v[k]);
        }
    }
    const Px haloPx = unpack(halo);

    // ---- the output rows: centre row k + 1, N = row k, S = row k + 2
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
        const Px hl = readlane(haloPx, k + 1), hr = readlane(haloPx, 32 + k + 1);
        const Px& cA = rowA[k + 1];
        if constexpr (PX == 2) {
            const Px& cB = rowB[k + 1];
            const Px wA = shr1(hl, cB), eB = shl1(hr, cA); // W of the first pixel = the second pixel of lane - 1, E of the second = the first of lane + 1
            const uint32_t oA = cas_pixel(cA, rowA[k], wA, cB, rowA[k + 2], p.sharpness);
            const uint32_t oB = cas_pixel(cB, rowB[k], cA, eB, rowB[k + 2], p.sharpness);
            if ((uint32_t)k < nrows && !beyond) ur::store_once_b64(p.out + (size_t)(rb0 + (uint32_t)k) * p.W + px0, ur::once_u32x2_t{oA, oB});
        } else {
            const Px w = shr1(hl, cA), e = shl1(hr, cA);
            const uint32_t o = cas_pixel(cA, rowA[k], w, e, rowA[k + 2], p.sharpness);
            if ((uint32_t)k < nrows && !beyond) p.out[(size_t)(rb0 + (uint32_t)k) * p.W + px0] = o;
        }
    }
}

bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + b_bytes && y < x + a_bytes;
}

// shared checks and launch of both CAS forms
int launch_cas(ur_ctx* ctx, const char* who, const ur_cas_constants* cas, bool fused, const void* src, const TonemapParams* tm, uint32_t* out,
               uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    if (w == 0 || h == 0 || rows == 0 || (uint64_t)row0 + rows > h) { ur::set_error("%s: empty or out-of-frame band", who); return UR_EINVAL; }
    const size_t src_bytes = (size_t)w * h * (fused ? 8u : 4u), out_bytes = (size_t)w * rows * 4u;
    if (overlaps(src, src_bytes, out, out_bytes)) { ur::set_error("%s: the output band overlaps the input frame", who); return UR_EINVAL; }
    // the taps are the 4-neighbour texels: TexelDelta must be one texel (relative tolerance for a delta computed in double)
    const float dx = 1.0f / (float)w, dy = 1.0f / (float)h;
    if (!(fabsf(cas->TexelDelta[0] - dx) <= 1e-6f * dx) || !(fabsf(cas->TexelDelta[1] - dy) <= 1e-6f * dy)) {
        ur::set_error("%s: TexelDelta must be (1/w, 1/h) (neighbour texels)", who);
        return UR_EUNSUPPORTED;
    }
    const uint32_t grid_y = (rows + (uint32_t)kRows - 1u) / (uint32_t)kRows;
    if (grid_y > 65535u) { ur::set_error("%s: band too tall", who); return UR_EUNSUPPORTED; }
    CasParams p{};
    p.src = src; p.out = out;
    p.W = w; p.H = h; p.row0 = row0; p.rows = rows;
    p.sharpness = cas->Sharpness;
    if (tm) p.tm = *tm;
    const bool pairs = (w % 2u) == 0u && (reinterpret_cast<uintptr_t>(src) & (fused ? 15u : 7u)) == 0u && (reinterpret_cast<uintptr_t>(out) & 7u) == 0u;
    const uint32_t px = pairs ? 2u : 1u;
    const dim3 grid((w + 256u * px - 1u) / (256u * px), grid_y);
    if (fused) {
        if (pairs) hipLaunchKernelGGL((cas_strip_kernel<true, 2>), grid, dim3(256), 0, ctx->stream, p);
        else hipLaunchKernelGGL((cas_strip_kernel<true, 1>), grid, dim3(256), 0, ctx->stream, p);
    } else {
        if (pairs) hipLaunchKernelGGL((cas_strip_kernel<false, 2>), grid, dim3(256), 0, ctx->stream, p);
        else hipLaunchKernelGGL((cas_strip_kernel<false, 1>), grid, dim3(256), 0, ctx->stream, p);
    }
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

} // namespace

extern "C" int ur_auto_exposure(ur_ctx* ctx, const ur_auto_exposure_constants* constants, const ur_half4* hdr_full, uint32_t w, uint32_t h,
                                const float* prev_ev, float* out_ev)
{
    if (!ctx || !constants || !hdr_full || !out_ev || (constants->UseHistory != 0u && !prev_ev)) {
        ur::set_error("ur_auto_exposure: null argument");
        return UR_EINVAL;
    }
    if (w == 0 || h == 0 || constants->InputSize[0] != (float)w || constants->InputSize[1] != (float)h) {
        ur::set_error("ur_auto_exposure: InputSize must be (w, h) of a non-empty frame");
        return UR_EINVAL;
    }
    AeParams p{};
    p.hdr = reinterpret_cast<const half4_t*>(hdr_full);
    p.prev = prev_ev; p.out = out_ev;
    p.W = w; p.H = h;
    p.size_x = constants->InputSize[0]; p.size_y = constants->InputSize[1];
    p.delta_time = constants->DeltaTime; p.speed_up = constants->AdaptationSpeedUp; p.speed_down = constants->AdaptationSpeedDown;
    p.use_history = constants->UseHistory;
    p.key = constants->AutoExposureKey; p.ev_min = constants->AutoExposureMin; p.ev_max = constants->AutoExposureMax;
    hipLaunchKernelGGL(auto_exposure_kernel, dim3(1), dim3(256), 0, ctx->stream, p);
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

extern "C" int ur_cas(ur_ctx* ctx, const ur_cas_constants* constants, const uint32_t* ldr_full, uint32_t* out_band,
                      uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    if (!ctx || !constants || !ldr_full || !out_band) { ur::set_error("ur_cas: null argument"); return UR_EINVAL; }
    return launch_cas(ctx, "ur_cas", constants, false, ldr_full, nullptr, out_band, w, h, row0, rows);
}

extern "C" int ur_tonemap_cas(ur_ctx* ctx, const ur_tonemap_constants* tonemap, const ur_cas_constants* cas, const ur_half4* hdr_full,
                              const float* exposure_ev, uint32_t* out_band, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    if (!ctx || !tonemap || !cas || !hdr_full || !out_band) { ur::set_error("ur_tonemap_cas: null argument"); return UR_EINVAL; }
    TonemapParams tm{}; // exactly ur_tonemap's (csrc/tonemap.hip)
    tm.exposure_ev = exposure_ev;
    tm.enable_tonemap = tonemap->EnableTonemap;
    tm.enable_auto_exposure = tonemap->EnableAutoExposure;
    tm.exposure = tonemap->Exposure;
    tm.inv_gamma = 1.0f / (tonemap->Gamma > 1e-3f ? tonemap->Gamma : 1e-3f);
    return launch_cas(ctx, "ur_tonemap_cas", cas, true, hdr_full, &tm, out_band, w, h, row0, rows);
}
