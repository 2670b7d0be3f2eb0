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
// Every CAS form runs one body, cas_strip below (cas_strip_kernel on the full image, cas_halo_kernel on a row band with the two
// rows around it): a wave owns a 64 * PX-column strip of kRows output rows. It loads the kRows + 2 input rows its taps need
// (rows clamped to the frame) and the texel left and right of the strip in each of them in ONE load phase, written once for
// every input kind and width (load_texels), converts each input row once to fp32 (R, G, B, luminance) and takes the horizontal
// neighbours from the adjacent lanes (DPP wave shifts, csrc/ur_device.h), the vertical ones from the rows kept in registers.
// No LDS, no barrier. Where an input row is HDR (every row of the fused form, the rows around the band of ur_cas_halo) it is
// converted by the same tonemap_pixel as ur_tonemap (csrc/post_common.h) before anything else: the bytes CAS sees are exactly
// ur_tonemap's, and the intermediate image is never written.
// Bytes per output pixel: CAS 4 read + 4 written (8), fused 8 read + 4 written (12, against 8 + 4 + 4 + 4 = 20 for the two
// launches); the two halo rows of a strip (2 / kRows more rows) are read again by the neighbouring strip's waves and,
// in the fused form, tonemapped twice.
// Built with -ffp-contract=off. The quotients go through v_rcp_f32 and the reciprocal square root through v_rsq_f32 (1 ulp
// each); each output byte stays within one LSB of a scalar fp32 evaluation of the HLSL (tests/post_ref.py).

#include "ur_internal.h"
#include "ur_device.h"
#include "post_common.h"
#include "post_records.h"

#include <type_traits>

namespace {

using ur_post::half4_t;
using ur_post::u32x2_t;
using ur_post::u32x4_t;
using ur_post::as_half4;
using ur_post::TonemapParams;
using ur_post::tonemap_pixel;
using ur_post::final_exposure;
using ur_post::unorm8;
using namespace ur_records;
using ur::overlaps;

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

// Tap (gx, gy) of AutoExposure.hlsl:27-29 and the 2x2 footprint SampleLevel(linear, clamp) of mip 0 reads around it (the
// Lighting SRV has one mip, DeferredRenderer.cpp:3006-3007): t = uv * size - 0.5, indices clamped, weights the fractions of t.
// The one definition of which texels a tap reads: auto_exposure_kernel samples them, post_record_kernel packs them.
struct AeTap {
    uint32_t x0, x1, y0, y1; // clamped texel indices of t00 = (x0, y0), t10 = (x1, y0), t01 = (x0, y1), t11 = (x1, y1)
    float ax, ay;
};

__device__ __forceinline__ AeTap ae_tap(uint32_t gx, uint32_t gy, uint32_t W, uint32_t H, float size_x, float size_y)
{
    const float samplePosX = ((float)gx + 0.5f) * (size_x / 16.0f), samplePosY = ((float)gy + 0.5f) * (size_y / 16.0f);
    const float u = samplePosX / fmaxf(size_x, 1.0f), v = samplePosY / fmaxf(size_y, 1.0f);
    const float tx = u * (float)W - 0.5f, ty = v * (float)H - 0.5f;
    const float fx = floorf(tx), fy = floorf(ty);
    const int ix = (int)fx, iy = (int)fy, mx = (int)W - 1, my = (int)H - 1;
    return AeTap{(uint32_t)min(max(ix, 0), mx), (uint32_t)min(max(ix + 1, 0), mx), (uint32_t)min(max(iy, 0), my), (uint32_t)min(max(iy + 1, 0), my),
                 tx - fx, ty - fy};
}

// The whole AutoExposure pass for one 256-lane workgroup; fetch(corner, x, y) returns texel (x, y) of the lane's tap, corner 0..3 =
// t00, t10, t01, t11. Both kernels below share every operation after the fetch, so the same texels give the same bits.
template <class Fetch>
__device__ __forceinline__ void ae_body(const AeParams& p, Fetch fetch)
{
    const uint32_t index = threadIdx.x, gx = index & 15u, gy = index >> 4; // GroupThreadId.xy of [numthreads(16,16,1)]
    const AeTap t = ae_tap(gx, gy, p.W, p.H, p.size_x, p.size_y);
    const float ax = t.ax, ay = t.ay;
    const half4_t t00 = fetch(0u, t.x0, t.y0), t10 = fetch(1u, t.x1, t.y0), t01 = fetch(2u, t.x0, t.y1), t11 = fetch(3u, t.x1, t.y1);
    // the blend: two lerps along x then one along y
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

__global__ __launch_bounds__(256) void auto_exposure_kernel(AeParams p)
{
    ae_body(p, [&](uint32_t, uint32_t x, uint32_t y) { return p.hdr[(size_t)y * p.W + x]; });
}

// ---- the post record of a row band (include/ur_hotpath.h, ur_post_record_bytes; its layout: csrc/post_records.h) ----------
// A tap texel (ae_tap) is written by the band that holds its row, zero by every other band: equal bands, owner = y / (H / N).

struct PackParams {
    const half4_t* band; // rows [row0, row0 + rows) of the W x H frame
    half4_t* record;
    uint32_t W, H, row0, rows;
};

__global__ __launch_bounds__(256) void post_record_kernel(PackParams p)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x, W = p.W;
    if (j < kPostRows * W) { // the record's two rows
        static_assert(kPostFirstRow == 0u && kPostLastRow == 1u && kPostRows == 2u, "the first row, then the last row");
        const uint32_t last = kPostLastRow * W; // where the last row starts in the record
        p.record[j] = j < last ? p.band[j] : p.band[(size_t)(p.rows - 1u) * W + (j - last)];
        return;
    }
    const uint32_t s = j - kPostRows * W;
    if (s >= kTapTexels) return;
    const uint32_t i = s >> 2, corner = s & 3u;
    const AeTap t = ae_tap(i & 15u, i >> 4, W, p.H, (float)W, (float)p.H); // InputSize == (W, H), as ur_auto_exposure requires
    const uint32_t x = (corner & 1u) ? t.x1 : t.x0, y = (corner & 2u) ? t.y1 : t.y0;
    half4_t v = {0, 0, 0, 0};
    if (y >= p.row0 && y - p.row0 < p.rows) v = p.band[(size_t)(y - p.row0) * W + x];
    p.record[j] = v;
}

struct AeRecordsParams {
    AeParams ae;             // hdr unused
    const half4_t* records;  // n_ranks records of record_texels half4 each, in rank order
    uint32_t record_texels, band_rows;
};

// auto_exposure_kernel with every texel read from its owner's record
__global__ __launch_bounds__(256) void ae_records_kernel(AeRecordsParams q)
{
    const uint32_t slot = kPostRows * q.ae.W + threadIdx.x * 4u;
    ae_body(q.ae, [&](uint32_t corner, uint32_t, uint32_t y) { return q.records[(size_t)(y / q.band_rows) * q.record_texels + slot + corner]; });
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

// a texel from the neighbouring lane (ur::wave_shr1 / wave_shl1: lane 0 / lane 63 keeps `old`, the texel beside the strip)
__device__ __forceinline__ Px shr1(const Px& old, const Px& v)
{
    auto s = [](float o, float x) { return __builtin_bit_cast(float, ur::wave_shr1(__builtin_bit_cast(uint32_t, o), __builtin_bit_cast(uint32_t, x))); };
    return Px{s(old.r, v.r), s(old.g, v.g), s(old.b, v.b), s(old.l, v.l)};
}
__device__ __forceinline__ Px shl1(const Px& old, const Px& v)
{
    auto s = [](float o, float x) { return __builtin_bit_cast(float, ur::wave_shl1(__builtin_bit_cast(uint32_t, o), __builtin_bit_cast(uint32_t, x))); };
    return Px{s(old.r, v.r), s(old.g, v.g), s(old.b, v.b), s(old.l, v.l)};
}
__device__ __forceinline__ Px readlane(const Px& v, int lane)
{
    auto rl = [lane](float x) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), lane)); };
    return Px{rl(v.r), rl(v.g), rl(v.b), rl(v.l)};
}

// What the input rows of a strip are: Ldr - R8G8B8A8; Hdr - RGBA16F, tonemapped on the way in (the fused form); LdrHdrHalo - the
// band's rows R8G8B8A8 (ur_tonemap's output), the two rows around the band RGBA16F, tonemapped here (ur_cas_halo).
enum class In { Ldr, Hdr, LdrHdrHalo };

// Where input row y (a frame row, already clamped to the frame) is. FrameRows: the full image (cas_strip_kernel). BandRows: a
// band-local image and one row above and one below it (cas_halo_kernel), each its own pointer; a strip's rows are uniform per wave,
// so the choice is scalar. Rows further out than the halo rows only feed output rows that are not stored: they read the halo row.
// units<U, N>(y): the row as units U of N texels each (N = 2: W is even, so a row starts on a unit).
struct FrameRows {
    const void* src;
    uint32_t W;
    __device__ __forceinline__ bool halo(uint32_t) const { return false; }
    template <class U, int N> __device__ __forceinline__ const U* units(uint32_t y) const { return static_cast<const U*>(src) + ((size_t)y * W) / N; }
};

struct BandRows {
    const void* band;
    const void* above; // row row0 - 1 (null iff row0 == 0: never selected then)
    const void* below; // row row0 + rows (null iff row0 + rows == H)
    uint32_t W, row0, rows;
    __device__ __forceinline__ bool halo(uint32_t y) const { return y < row0 || y - row0 >= rows; }
    template <class U, int N> __device__ __forceinline__ const U* units(uint32_t y) const
    {
        return y < row0 ? static_cast<const U*>(above) : y - row0 >= rows ? static_cast<const U*>(below) : static_cast<const U*>(band) + ((size_t)(y - row0) * W) / N;
    }
};

// ---- the one loader of every CAS form. N texels of an input row as loaded: N dwords of an RGBA8 row, 2N of an RGBA16F one.
template <int DWORDS> using dwords_t = std::conditional_t<DWORDS == 1, uint32_t, std::conditional_t<DWORDS == 2, u32x2_t, u32x4_t>>;
// ... kept as the wider of the kinds MODE can meet, RGBA8 texels in the low dwords
template <In MODE, int N> using raw_t = dwords_t<MODE == In::Ldr ? N : 2 * N>;
__device__ __forceinline__ u32x2_t widen(uint32_t l) { return u32x2_t{l, 0u}; }
__device__ __forceinline__ u32x4_t widen(u32x2_t l) { return u32x4_t{l.x, l.y, 0u, 0u}; }
__device__ __forceinline__ uint32_t dword(uint32_t v, int) { return v; }
template <class V> __device__ __forceinline__ uint32_t dword(V v, int i) { return v[i]; }

// Is input row y RGBA16F, to be tonemapped on the way in? Uniform per wave where y is.
template <In MODE, class Rows>
__device__ __forceinline__ bool hdr_row(const Rows& src, uint32_t y) { return MODE == In::Hdr || (MODE == In::LdrHdrHalo && src.halo(y)); }

// Unit i of row y. own: a row only this strip reads, for which the source asks for a nontemporal load; a row around the band
// (LdrHdrHalo) is a plain load whatever k. Written as a select of two loads, the request does not reach the gfx950 instructions: no
// load of a CAS kernel carries `nt`, before this loader or with it (an open item in EXPERIMENTS.md; the form is kept as it was).
template <In MODE, int N, class Rows>
__device__ __forceinline__ raw_t<MODE, N> load_texels(const Rows& src, uint32_t y, size_t i, bool own)
{
    auto load = [](const auto* a, bool once) { return once ? __builtin_nontemporal_load(a) : *a; };
    if constexpr (MODE == In::Ldr) return load(src.template units<dwords_t<N>, N>(y) + i, own);
    else if (hdr_row<MODE>(src, y)) return load(src.template units<dwords_t<2 * N>, N>(y) + i, own && MODE == In::Hdr);
    else return widen(load(src.template units<dwords_t<N>, N>(y) + i, own));
}

// Texel t of a loaded unit as the R8G8B8A8 CAS reads: an RGBA16F one through ur_tonemap's pixel
template <In MODE, class Raw>
__device__ __forceinline__ uint32_t rgba8(const TonemapParams& tm, float finalExposure, Raw v, bool hdr, int t)
{
    if constexpr (MODE != In::Ldr) {
        if (hdr) return tonemap_pixel(tm, finalExposure, as_half4(u32x2_t{dword(v, 2 * t), dword(v, 2 * t + 1)}));
    }
    return dword(v, t);
}

// One strip of CAS output (see the file comment). PX: pixels per lane - 2 (even width; 16-B aligned HDR / 8-B aligned RGBA8 rows:
// one 16- or 8-byte load and one 8-byte store per lane and row) or 1 (any width and alignment).
template <In MODE, int PX, class Rows>
__device__ __forceinline__ void cas_strip(const CasParams& p, const Rows& src)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t x0 = (blockIdx.x * 4u + wave) * (64u * PX); // the wave's first column; the four waves side by side
    if (x0 >= p.W) return;                                     // uniform per wave (no barrier in this kernel)
    const uint32_t rb0 = blockIdx.y * (uint32_t)kRows;          // first output row of the strip, band-local
    const uint32_t nrows = min((uint32_t)kRows, p.rows - rb0);
    const int maxy = (int)p.H - 1;
    const uint32_t maxx = p.W - 1u, px0 = x0 + lane * PX;       // the lane's first column
    const bool beyond = px0 > maxx;                             // lanes right of the frame repeat the last column
    const float finalExposure = MODE != In::Ldr ? final_exposure(p.tm) : 0.0f;
    // input row k (0 .. kRows + 1) = frame row row0 + rb0 - 1 + k, clamped (the taps' clamp at the top and bottom edges)
    auto frame_row = [&](int k) -> uint32_t { return (uint32_t)min(max((int)(p.row0 + rb0) - 1 + k, 0), maxy); };
    auto interior = [&](int k) { return k >= 1 && k <= kRows; }; // the strip's own rows (its halo rows are other strips' own): `own` of load_texels

    // ---- the load phase: kRows + 2 rows, and the texels left / right of the strip (lane j < kRows + 2: row j's left one,
    // lane 32 + j: its right one), all in flight before the first is used
    const uint32_t hx = lane < 32u ? (x0 == 0u ? 0u : x0 - 1u) : min(x0 + 64u * PX, maxx);
    const uint32_t hy = frame_row((int)min(lane & 31u, (uint32_t)kRows + 1u));
    const size_t unit = min(px0, maxx - (PX - 1u)) / PX; // the lane's PX texels of a row, clamped into the frame
    const raw_t<MODE, 1> side = load_texels<MODE, 1>(src, hy, hx, false);
    raw_t<MODE, PX> v[kRows + 2];
#pragma unroll
    for (int k = 0; k < kRows + 2; ++k) v[k] = load_texels<MODE, PX>(src, frame_row(k), unit, interior(k));
    // ---- the convert phase: each texel once to RGBA8 (ur_tonemap's bytes) and on to fp32
    const uint32_t halo = rgba8<MODE>(p.tm, finalExposure, side, hdr_row<MODE>(src, hy), 0);
    Px rowA[kRows + 2], rowB[kRows + 2]; // the lane's pixel(s) of each input row (rowB: PX == 2 only)
#pragma unroll
    for (int k = 0; k < kRows + 2; ++k) {
        const bool hdr = hdr_row<MODE>(src, frame_row(k));
        // tb: the unit's last texel (index PX - 1); ta: its first - for PX == 1 the same texel, and a lane beyond the frame repeats tb
        const uint32_t tb = rgba8<MODE>(p.tm, finalExposure, v[k], hdr, PX - 1);
        const uint32_t ta = (PX == 2 && beyond) ? tb : rgba8<MODE>(p.tm, finalExposure, v[k], hdr, 0);
        rowA[k] = unpack(ta);
        if constexpr (PX == 2) rowB[k] = unpack(tb);
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

// FUSED: tonemap HDR rows on the way in; the input is the full image
template <bool FUSED, int PX>
__global__ __launch_bounds__(256) void cas_strip_kernel(CasParams p)
{
    cas_strip<FUSED ? In::Hdr : In::Ldr, PX>(p, FrameRows{p.src, p.W});
}

struct CasHaloParams {
    CasParams c;         // src: the band-local input rows
    const void* above;   // RGBA16F row row0 - 1, nullable iff row0 == 0
    const void* below;   // RGBA16F row row0 + rows, nullable iff row0 + rows == H
};

// MODE Hdr: ur_tonemap_cas_halo; LdrHdrHalo: ur_cas_halo
template <In MODE, int PX>
__global__ __launch_bounds__(256) void cas_halo_kernel(CasHaloParams p)
{
    cas_strip<MODE, PX>(p.c, BandRows{p.c.src, p.above, p.below, p.c.W, p.c.row0, p.c.rows});
}

// shared checks and launch of every CAS form. halo: src holds the band's rows only, above / below the RGBA16F rows around it.
int launch_cas(ur_ctx* ctx, const char* who, const ur_cas_constants* cas, In mode, bool halo, const void* src, const void* above, const void* below,
               const TonemapParams* tm, uint32_t* out, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    if (rows == 0 || !ur::band_in_frame(w, h, row0, rows)) { ur::set_error("%s: empty or out-of-frame band", who); return UR_EINVAL; }
    if (halo && ((row0 > 0 && !above) || (row0 + rows < h && !below))) {
        ur::set_error("%s: hdr_above may be null only when row0 == 0, hdr_below only when row0 + rows == h", who);
        return UR_EINVAL;
    }
    const size_t src_bytes = (size_t)w * (halo ? rows : h) * (mode == In::Hdr ? 8u : 4u), out_bytes = (size_t)w * rows * 4u, halo_bytes = (size_t)w * 8u;
    if (overlaps(src, src_bytes, out, out_bytes) || (above && overlaps(above, halo_bytes, out, out_bytes)) || (below && overlaps(below, halo_bytes, out, out_bytes))) {
        ur::set_error("%s: the output band overlaps the input frame", who);
        return UR_EINVAL;
    }
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
    auto aligned = [](const void* q, uintptr_t m) { return (reinterpret_cast<uintptr_t>(q) & m) == 0u; };
    const bool pairs = (w % 2u) == 0u && aligned(src, mode == In::Hdr ? 15u : 7u) && aligned(out, 7u) && aligned(above, 15u) && aligned(below, 15u);
    const uint32_t px = pairs ? 2u : 1u;
    const dim3 grid((w + 256u * px - 1u) / (256u * px), grid_y);
    auto launch = [&](auto* one, auto* two, const auto& q) { // the kernel of one pixel per lane, or of two
        auto* kernel = pairs ? two : one;
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, q);
    };
    if (halo && mode == In::Hdr) launch(cas_halo_kernel<In::Hdr, 1>, cas_halo_kernel<In::Hdr, 2>, CasHaloParams{p, above, below});
    else if (halo) launch(cas_halo_kernel<In::LdrHdrHalo, 1>, cas_halo_kernel<In::LdrHdrHalo, 2>, CasHaloParams{p, above, below});
    else if (mode == In::Hdr) launch(cas_strip_kernel<true, 1>, cas_strip_kernel<true, 2>, p);
    else launch(cas_strip_kernel<false, 1>, cas_strip_kernel<false, 2>, p);
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

AeParams ae_params(const ur_auto_exposure_constants* constants, uint32_t w, uint32_t h, const float* prev_ev, float* out_ev)
{
    AeParams p{};
    p.prev = prev_ev; p.out = out_ev;
    p.W = w; p.H = h;
    p.size_x = constants->InputSize[0]; p.size_y = constants->InputSize[1];
    p.delta_time = constants->DeltaTime; p.speed_up = constants->AdaptationSpeedUp; p.speed_down = constants->AdaptationSpeedDown;
    p.use_history = constants->UseHistory;
    p.key = constants->AutoExposureKey; p.ev_min = constants->AutoExposureMin; p.ev_max = constants->AutoExposureMax;
    return p;
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
    AeParams p = ae_params(constants, w, h, prev_ev, out_ev);
    p.hdr = reinterpret_cast<const half4_t*>(hdr_full);
    hipLaunchKernelGGL(auto_exposure_kernel, dim3(1), dim3(256), 0, ctx->stream, p);
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

extern "C" int ur_cas(ur_ctx* ctx, const ur_cas_constants* constants, const uint32_t* ldr_full, uint32_t* out_band,
                      uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    if (!ctx || !constants || !ldr_full || !out_band) { ur::set_error("ur_cas: null argument"); return UR_EINVAL; }
    return launch_cas(ctx, "ur_cas", constants, In::Ldr, false, ldr_full, nullptr, nullptr, nullptr, out_band, w, h, row0, rows);
}

extern "C" int ur_tonemap_cas(ur_ctx* ctx, const ur_tonemap_constants* tonemap, const ur_cas_constants* cas, const ur_half4* hdr_full,
                              const float* exposure_ev, uint32_t* out_band, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    if (!ctx || !tonemap || !cas || !hdr_full || !out_band) { ur::set_error("ur_tonemap_cas: null argument"); return UR_EINVAL; }
    const TonemapParams tm = ur_post::tonemap_params(tonemap, exposure_ev, nullptr);
    return launch_cas(ctx, "ur_tonemap_cas", cas, In::Hdr, false, hdr_full, nullptr, nullptr, &tm, out_band, w, h, row0, rows);
}

// ---- the post exchange of row bands ---------------------------------------------------------------------------------------

extern "C" uint64_t ur_post_record_bytes(uint32_t w) { return post_texels(w) * kTexelBytes; }

extern "C" int ur_pack_post_record(ur_ctx* ctx, const ur_half4* hdr_band, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows, void* record)
{
    if (!ctx || !hdr_band || !record) { ur::set_error("ur_pack_post_record: null argument"); return UR_EINVAL; }
    if (rows == 0 || !ur::band_in_frame(w, h, row0, rows)) { ur::set_error("ur_pack_post_record: empty or out-of-frame band"); return UR_EINVAL; }
    if (overlaps(hdr_band, (size_t)w * rows * 8u, record, ur_post_record_bytes(w))) { ur::set_error("ur_pack_post_record: the record overlaps the band"); return UR_EINVAL; }
    PackParams p{reinterpret_cast<const half4_t*>(hdr_band), static_cast<half4_t*>(record), w, h, row0, rows};
    const uint32_t n = (uint32_t)post_texels(w);
    hipLaunchKernelGGL(post_record_kernel, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, p);
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

extern "C" int ur_auto_exposure_records(ur_ctx* ctx, const ur_auto_exposure_constants* constants, const void* records, uint32_t n_ranks, uint32_t w,
                                        uint32_t h, const float* prev_ev, float* out_ev)
{
    if (!ctx || !constants || !records || !out_ev || (constants->UseHistory != 0u && !prev_ev)) {
        ur::set_error("ur_auto_exposure_records: null argument");
        return UR_EINVAL;
    }
    if (w == 0 || h == 0 || constants->InputSize[0] != (float)w || constants->InputSize[1] != (float)h) {
        ur::set_error("ur_auto_exposure_records: InputSize must be (w, h) of a non-empty frame");
        return UR_EINVAL;
    }
    if (n_ranks == 0 || h % n_ranks != 0) { ur::set_error("ur_auto_exposure_records: n_ranks must divide h (equal bands)"); return UR_EINVAL; }
    AeRecordsParams q{};
    q.ae = ae_params(constants, w, h, prev_ev, out_ev);
    q.records = static_cast<const half4_t*>(records);
    q.record_texels = (uint32_t)post_texels(w);
    q.band_rows = h / n_ranks;
    hipLaunchKernelGGL(ae_records_kernel, dim3(1), dim3(256), 0, ctx->stream, q);
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

extern "C" int ur_tonemap_cas_halo(ur_ctx* ctx, const ur_tonemap_constants* tonemap, const ur_cas_constants* cas, const ur_half4* hdr_band,
                                   const ur_half4* hdr_above, const ur_half4* hdr_below, const float* exposure_ev, uint32_t* out_band,
                                   uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    if (!ctx || !tonemap || !cas || !hdr_band || !out_band) { ur::set_error("ur_tonemap_cas_halo: null argument"); return UR_EINVAL; }
    const TonemapParams tm = ur_post::tonemap_params(tonemap, exposure_ev, nullptr);
    return launch_cas(ctx, "ur_tonemap_cas_halo", cas, In::Hdr, true, hdr_band, hdr_above, hdr_below, &tm, out_band, w, h, row0, rows);
}

extern "C" int ur_cas_halo(ur_ctx* ctx, const ur_tonemap_constants* tonemap, const ur_cas_constants* cas, const uint32_t* ldr_band,
                           const ur_half4* hdr_above, const ur_half4* hdr_below, const float* exposure_ev, uint32_t* out_band,
                           uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    if (!ctx || !tonemap || !cas || !ldr_band || !out_band) { ur::set_error("ur_cas_halo: null argument"); return UR_EINVAL; }
    const TonemapParams tm = ur_post::tonemap_params(tonemap, exposure_ev, nullptr);
    return launch_cas(ctx, "ur_cas_halo", cas, In::LdrHdrHalo, true, ldr_band, hdr_above, hdr_below, &tm, out_band, w, h, row0, rows);
}
