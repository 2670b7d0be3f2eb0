// TemporalAA resolve for gfx950: 3x3 neighbourhood min/max of the current HDR frame, history clamped
// into that box, blended by HistoryWeight.
//
// Reference: Shaders/TemporalAA.hlsl:12-50 ([numthreads(8,8,1)], nine Texture2D.Load per pixel, neighbour coordinates
// clamped to the frame), pass Source/Render/DeferredRenderer.cpp:1308-1361. Here a wave owns a 64-column x 8-row strip
// and keeps it in registers (see taa_strip_kernel below): no LDS, every row access 512 contiguous aligned bytes per wave,
// 2 KB per workgroup. HBM: 8 B current + 8 B history read, 8 B written per pixel (24 B/pixel; the two halo rows of a
// strip are L2 hits while the neighbouring strip is in flight).
// Built with -ffp-contract=off: min/max/clamp are exact and lerp is a + t*(b-a) in fp32 with one RTE to fp16, so the
// output is bit-identical to the oracle.
// History of the shape (4K, 199 MB per launch; a plain 2-reads-1-write streaming kernel of that size takes 35.3 us,
// tools/microbench/stream_ceiling.hip): 64x8 tiles through LDS 43.8 us; 16-row strips walked four rows at a time 43.8 us
// (a chain of five dependent memory round trips per wave: 8 us of fixed cost); 8-row strips loaded in one phase 42.5 us
// (68 VGPRs: 7 waves/SIMD, the grid took 2.3 rounds = 3); the halo texels of a strip in ONE load, 56 VGPRs, 8 waves/SIMD,
// two rounds: 37.0 us = 5.4 TB/s.
//
// ur_temporal_aa_tonemap is the same strip body with a Tonemap epilogue (the Post policy of taa_strip_kernel): each blended
// texel, after its rounding to fp16, also goes through tonemap_pixel (csrc/post_common.h, the one ur_tonemap runs) while it is
// in registers, so the history image is not read back by a Tonemap launch: 8 + 8 read, 8 + 4 written = 28 B/pixel in one
// launch instead of 24 + 12 in two. The history bytes are ur_temporal_aa's and the LDR bytes ur_tonemap's of that image.
//
// Row bands (the TAA record and ur_temporal_aa_halo / ur_temporal_aa_tonemap_halo, include/ur_hotpath.h): taa_band_kernel runs the
// same strip body (taa_strip below) with only the band in memory. Where a row is comes from a rows policy: FrameRows - the full
// frame, one base pointer (taa_strip_kernel); BandRows - the band, the current row above and below it, the second row out on either
// side, and the neighbours' history rows, each its own pointer. A strip's rows are uniform per wave, so the choice of the base
// pointer is scalar. The same launch resolves the rows row0 - 1 and row0 + rows (two more one-row strips at the end of the grid):
// the HDR halo rows of the CAS launch behind it, the very texels the neighbour rank writes into its own history image.

#include "ur_internal.h"
#include "ur_device.h"
#include "post_common.h"
#include "post_records.h"

namespace {

using ur_post::half4_t;
using ur_post::u32x2_t;
using namespace ur_records;

struct TaaParams {
    const half4_t* current; // full frame
    const half4_t* history; // band
    half4_t* output;        // band
    uint32_t W, H, row0, rows;
    float weight;           // saturate(HistoryWeight)
    uint32_t use_history;
};

// ---- a wave owns a 64-column x kStripRows strip ------------------------------------------------------------------------
// The 3x3 box is separable: per row the horizontal min/max of (left, centre, right), then the vertical min/max of three
// consecutive rows. Left/right come from the neighbouring lanes (DPP wave shifts, no LDS); the texels left of lane 0 and
// right of lane 63 are fetched for all rows of the strip by one load and broadcast with v_readlane. min/max run on the
// packed fp16 pairs (exact: no rounding, the same ordering as the fp32 compares of the reference), the clamp and the
// lerp in fp32 as in TemporalAA.hlsl:41-49.
constexpr int kStripRows = 8;
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));

struct RowMinMax { half2_t mn0, mn1, mx0, mx1; }; // (R,G) and (B,A) pairs

__device__ __forceinline__ half2_t as_h2(uint32_t u) { union { uint32_t u; half2_t h; } c; c.u = u; return c.h; }
__device__ __forceinline__ uint32_t as_u(half2_t h) { union { uint32_t u; half2_t h; } c; c.h = h; return c.u; }
// HLSL's min / max ignore a NaN operand. v_pk_min/max_f16 do so for a quiet NaN, but return NaN when an operand is a
// signalling NaN (IEEE mode), so min(-Inf, sNaN) would drop the -Inf. The texels of a row are quieted (v_pk_max_f16 x, x)
// before the row's min / max; the compiler did so on its own for most of them, but not for the halo texel a lane at the
// strip's edge takes from v_readlane through the DPP shift. The centre texel itself stays as loaded: its alpha is copied.
__device__ __forceinline__ half2_t quiet(uint32_t u) { return __builtin_elementwise_canonicalize(as_h2(u)); }
__device__ __forceinline__ half2_t pk_min(half2_t a, half2_t b) { return __builtin_elementwise_min(a, b); }
__device__ __forceinline__ half2_t pk_max(half2_t a, half2_t b) { return __builtin_elementwise_max(a, b); }

// horizontal (left, centre, right) min/max of one row; (hl0, hl1) / (hr0, hr1) = the texel left of lane 0 / right of lane 63
__device__ __forceinline__ RowMinMax row_minmax(u32x2_t c, uint32_t hl0, uint32_t hl1, uint32_t hr0, uint32_t hr1)
{
    const uint32_t l0 = ur::wave_shr1(hl0, c.x), l1 = ur::wave_shr1(hl1, c.y); // the left texel: lane l - 1's, lane 0 takes hl
    const uint32_t r0 = ur::wave_shl1(hr0, c.x), r1 = ur::wave_shl1(hr1, c.y); // the right texel: lane l + 1's, lane 63 takes hr
    RowMinMax m;
    const half2_t ql0 = quiet(l0), ql1 = quiet(l1), qr0 = quiet(r0), qr1 = quiet(r1), qc0 = quiet(c.x), qc1 = quiet(c.y);
    m.mn0 = pk_min(pk_min(ql0, qr0), qc0); m.mn1 = pk_min(pk_min(ql1, qr1), qc1);
    m.mx0 = pk_max(pk_max(ql0, qr0), qc0); m.mx1 = pk_max(pk_max(ql1, qr1), qc1);
    return m;
}

// What happens to a resolved texel besides the history store. NoPost: nothing (ur_temporal_aa). TonemapPost: the Tonemap pixel
// of the stored fp16 value into the LDR band (ur_temporal_aa_tonemap); ONCE = the history store keeps its write-through +
// nontemporal hint (nothing reads the image again in this frame), else it is a plain store (UR_OPT_TAA_TONEMAP_HISTORY_STORE).
struct NoPost {
    static constexpr bool kHistoryOnce = true;
    __device__ __forceinline__ float prepare() const { return 0.0f; }
    __device__ __forceinline__ void texel(float, size_t, uint32_t, uint32_t) const {}
};
template <bool ONCE>
struct TonemapPost {
    static constexpr bool kHistoryOnce = ONCE;
    ur_post::TonemapParams tm; // hdr / count unused: the texel comes from the strip; out = the LDR band
    __device__ __forceinline__ float prepare() const { return ur_post::final_exposure(tm); } // uniform: one scalar load of the EV per wave
    __device__ __forceinline__ void texel(float finalExposure, size_t i, uint32_t lo, uint32_t hi) const
    {
        ur::store_once_b32(tm.out + i, ur_post::tonemap_pixel(tm, finalExposure, ur_post::as_half4(u32x2_t{lo, hi})));
    }
};

// Where the rows of a strip are. cur(y): y is a frame row already clamped to the frame (the taps' clamp, TemporalAA.hlsl:38);
// hist(r) / out(r) / in_band(r): r is a row relative to the band's first (an output row of the strip).
// FrameRows: current = the full frame, history / output = band-local images of rows [row0, row0 + rows).
struct FrameRows {
    const u32x2_t* current;
    const u32x2_t* history;
    u32x2_t* output;
    uint32_t W;
    __device__ __forceinline__ const u32x2_t* cur(uint32_t y) const { return current + (size_t)y * W; }
    __device__ __forceinline__ const u32x2_t* hist(int r) const { return history + (size_t)(uint32_t)r * W; }
    __device__ __forceinline__ u32x2_t* out(int r) const { return output + (size_t)(uint32_t)r * W; }
    __device__ __forceinline__ bool in_band(int) const { return true; }
};

// BandRows: only the band's rows of the three images are in memory; the rows around it are the neighbours' record rows.
// Current rows: above2 | above | band | below | below2 = frame rows max(row0 - 2, 0), row0 - 1, the band, row0 + rows, min(row0 + rows
// + 1, H - 1). [ylo, yhi] are the outermost rows that have a pointer: a row further out only feeds output rows that are not stored, and
// reads the outermost row instead (never a null pointer). History / output rows outside the band are the resolved rows' own.
struct BandRows {
    const u32x2_t *band, *above, *below, *above2, *below2;
    const u32x2_t *history, *hist_above, *hist_below;
    u32x2_t *output, *res_above, *res_below;
    uint32_t W, row0, rows, ylo, yhi;
    __device__ __forceinline__ const u32x2_t* cur(uint32_t y) const
    {
        y = min(max(y, ylo), yhi);
        return y < row0 ? (y + 1u == row0 ? above : above2) : y - row0 < rows ? band + (size_t)(y - row0) * W : (y - row0 == rows ? below : below2);
    }
    __device__ __forceinline__ const u32x2_t* hist(int r) const
    {
        return r < 0 ? hist_above : (uint32_t)r < rows ? history + (size_t)(uint32_t)r * W : hist_below;
    }
    __device__ __forceinline__ u32x2_t* out(int r) const
    {
        return r < 0 ? res_above : (uint32_t)r < rows ? output + (size_t)(uint32_t)r * W : res_below;
    }
    __device__ __forceinline__ bool in_band(int r) const { return r >= 0 && (uint32_t)r < rows; }
};

// One strip: output rows [r0, r0 + nrows) (relative to the band's first row row0; nrows <= kStripRows) of the wave's 64 columns. The one body of every TemporalAA
// launch: the same texels give the same bits wherever the rows come from. Post::texel runs for rows of the band only (its index is
// band-local); a resolved row outside the band is stored and nothing else.
template <class Post, class Rows>
__device__ __forceinline__ void taa_strip(const Rows& R, const Post& post, uint32_t W, uint32_t H, float weight, uint32_t use_history, uint32_t row0,
                                          int r0, uint32_t nrows)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // the four waves of a workgroup sit side by side: a workgroup touches 2 KB of contiguous bytes per row and buffer
    // (with the waves stacked vertically - 512-byte segments - the kernel ran at 4.5 TB/s, as did the LDS-tiled one with
    // its 64x8 tiles; a plain streaming kernel of the same byte mix reaches 5.6: tools/microbench/stream_ceiling.hip)
    const uint32_t x0 = (blockIdx.x * 4u + wave) * 64u;
    if (x0 >= W) return;                                 // uniform per wave (no barrier in this kernel)
    const uint32_t maxx = W - 1u, maxy = H - 1u;
    const uint32_t px = x0 + lane, cx = min(px, maxx);                    // lanes right of the frame re-read the last column
    // halo texels: ONE load for the whole strip - lane k holds the texel left of the strip in row k, lane 32 + k the one
    // right of it (k < kStripRows + 2); row k's pair is broadcast from there when the row is reduced
    const uint32_t hx = lane < 32u ? (x0 == 0u ? 0u : x0 - 1u) : min(x0 + 64u, maxx); // clamped to the frame (:38)

    auto frame_row = [&](int band_row) -> uint32_t { return (uint32_t)min(max((int)row0 + band_row, 0), (int)maxy); }; // band row (may be outside the band) -> clamped frame row
    const float finalExposure = post.prepare();
    if (use_history == 0) { // UseHistory == 0: the resolve is a copy of the current frame (TemporalAA.hlsl:23-27)
        for (uint32_t k = 0; k < nrows; ++k)
            if (px <= maxx) {
                const int r = r0 + (int)k;
                const u32x2_t v = R.cur(frame_row(r))[px];
                R.out(r)[px] = v;
                if (R.in_band(r)) post.texel(finalExposure, (size_t)(uint32_t)r * W + px, v.x, v.y);
            }
        return;
    }
    // One load phase per wave: the strip's kStripRows + 2 current rows (with their halo texels) and kStripRows history
    // rows are all in flight before the first is used - a wave's life is one memory round trip, the arithmetic, the
    // stores. (Walking a taller strip group by group made every wave a chain of five dependent round trips: 8 us of
    // fixed cost per launch at any frame size.) Later workgroups of the grid load while earlier ones compute and store.
    u32x2_t c[kStripRows + 2], hist[kStripRows];
    const u32x2_t halo = R.cur(frame_row(r0 - 1 + (int)min(lane & 31u, (uint32_t)kStripRows + 1u)))[hx];
#pragma unroll
    for (int k = 0; k < kStripRows + 2; ++k) c[k] = R.cur(frame_row(r0 + k - 1))[cx];
    const int rlast = r0 + (int)nrows - 1;
#pragma unroll
    for (int k = 0; k < kStripRows; ++k) hist[k] = __builtin_nontemporal_load(R.hist(min(r0 + k, rlast)) + cx); // read once
    auto reduce_row = [&](int k) {
        return row_minmax(c[k], __builtin_amdgcn_readlane(halo.x, k), __builtin_amdgcn_readlane(halo.y, k),
                          __builtin_amdgcn_readlane(halo.x, 32 + k), __builtin_amdgcn_readlane(halo.y, 32 + k));
    };
    RowMinMax mPrev = reduce_row(0), mCur = reduce_row(1);
#pragma unroll
    for (int k = 0; k < kStripRows; ++k) {
        const int r = r0 + k;
        const RowMinMax mNext = reduce_row(k + 2);
        if ((uint32_t)k < nrows && px <= maxx) {
            const half2_t mn0 = pk_min(pk_min(mPrev.mn0, mNext.mn0), mCur.mn0), mn1 = pk_min(pk_min(mPrev.mn1, mNext.mn1), mCur.mn1);
            const half2_t mx0 = pk_max(pk_max(mPrev.mx0, mNext.mx0), mCur.mx0), mx1 = pk_max(pk_max(mPrev.mx1, mNext.mx1), mCur.mx1);
            const half2_t c0 = as_h2(c[k + 1].x), c1 = as_h2(c[k + 1].y), h0 = as_h2(hist[k].x), h1 = as_h2(hist[k].y);
            const float cf[3] = {(float)c0.x, (float)c0.y, (float)c1.x};
            const float hv[3] = {(float)h0.x, (float)h0.y, (float)h1.x};
            const float mn[3] = {(float)mn0.x, (float)mn0.y, (float)mn1.x}, mx[3] = {(float)mx0.x, (float)mx0.y, (float)mx1.x};
            float b[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float hc = fminf(fmaxf(hv[ch], mn[ch]), mx[ch]); // clamp(History, Min, Max)
                b[ch] = cf[ch] + weight * (hc - cf[ch]);              // lerp(Current, History, w)
            }
            half2_t o0, o1;
            o0.x = (_Float16)b[0]; o0.y = (_Float16)b[1]; o1.x = (_Float16)b[2]; o1.y = c1.y; // alpha of the current texel
            u32x2_t* o = R.out(r) + px;
            if constexpr (Post::kHistoryOnce) ur::store_once_b64(o, ur::once_u32x2_t{as_u(o0), as_u(o1)});
            else *o = u32x2_t{as_u(o0), as_u(o1)};
            // the row is tonemapped right before its store: no row stays live for it
            if (R.in_band(r)) post.texel(finalExposure, (size_t)(uint32_t)r * W + px, as_u(o0), as_u(o1));
        }
        mPrev = mCur; mCur = mNext;
    }
}

template <class Post>
__global__ __launch_bounds__(256) void taa_strip_kernel(TaaParams p, Post post)
{
    const uint32_t r0 = blockIdx.y * (uint32_t)kStripRows; // first row of the strip inside the band
    const FrameRows R{reinterpret_cast<const u32x2_t*>(p.current), reinterpret_cast<const u32x2_t*>(p.history), reinterpret_cast<u32x2_t*>(p.output), p.W};
    taa_strip(R, post, p.W, p.H, p.weight, p.use_history, p.row0, (int)r0, min((uint32_t)kStripRows, p.rows - r0));
}

struct TaaBandParams {
    BandRows R;
    uint32_t H;
    float weight; // saturate(HistoryWeight)
    uint32_t use_history;
    uint32_t strips; // strips of the band; behind them in the grid: the resolved row above (if any), then the one below (if any)
};

// The band alone (ur_temporal_aa_halo / ur_temporal_aa_tonemap_halo): blockIdx.y < strips - a strip of the band, whose outer rows come
// from the rows around the band; then one one-row strip per resolved row.
template <class Post>
__global__ __launch_bounds__(256) void taa_band_kernel(TaaBandParams p, Post post)
{
    const uint32_t s = blockIdx.y; // uniform: the choice of a row's base pointer in BandRows is scalar
    int r0; // relative to the band's first row
    uint32_t nrows;
    if (s < p.strips) {
        r0 = (int)(s * (uint32_t)kStripRows);
        nrows = min((uint32_t)kStripRows, p.R.rows - s * (uint32_t)kStripRows);
    } else {
        const bool above = s == p.strips && p.R.res_above != nullptr;
        r0 = above ? -1 : (int)p.R.rows;
        nrows = 1u;
    }
    taa_strip(p.R, post, p.R.W, p.H, p.weight, p.use_history, p.R.row0, r0, nrows);
}

// ---- the TAA record of a row band (include/ur_hotpath.h, ur_taa_record_bytes; its layout: csrc/post_records.h) ----------------
struct TaaRecordParams {
    const u32x2_t* band;    // current rows [row0, row0 + rows)
    const u32x2_t* history; // the same rows of the history image read; null without history
    u32x2_t* record;
    uint32_t W, rows;
};

__global__ __launch_bounds__(256) void taa_record_kernel(TaaRecordParams p)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x, W = p.W;
    if (j >= kTaaRows * W) return;
    const uint32_t part = j / W, x = j - part * W; // the record's row; uniform per wave except across a row's edge
    const uint32_t second = min(1u, p.rows - 1u), second_last = p.rows >= 2u ? p.rows - 2u : 0u;
    u32x2_t v = {0u, 0u};
    if (part < kTaaHistFirstRow) v = p.band[(size_t)(part == kTaaSecondRow ? second : second_last) * W + x];
    else if (p.history != nullptr) v = p.history[(size_t)(part == kTaaHistFirstRow ? 0u : p.rows - 1u) * W + x];
    p.record[j] = v;
}

} // namespace

static int fill_params(const char* who, TaaParams& p, ur_ctx* ctx, const ur_half4* current_frame, const ur_half4* history_band, ur_half4* output_band,
                       float history_weight, uint32_t use_history, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    if (!ctx || !current_frame || !output_band || (use_history && !history_band)) { ur::set_error("%s: null argument", who); return UR_EINVAL; }
    if (!ur::band_in_frame(w, h, row0, rows)) { ur::set_error("%s: bad frame/band", who); return UR_EINVAL; } // (an empty band: nothing to do)
    p.current = reinterpret_cast<const half4_t*>(current_frame);
    p.history = reinterpret_cast<const half4_t*>(history_band);
    p.output = reinterpret_cast<half4_t*>(output_band);
    p.W = w; p.H = h; p.row0 = row0; p.rows = rows;
    p.weight = history_weight < 0.0f ? 0.0f : (history_weight > 1.0f ? 1.0f : history_weight);
    if (!(history_weight == history_weight)) p.weight = 0.0f; // saturate(NaN) = 0
    p.use_history = use_history ? 1u : 0u;
    return UR_OK;
}

// history_band may BE output_band (a ring of one image): a history texel is read only by the lane that writes it, and every load
// of a wave is issued before its first store; current_frame is a different buffer.
extern "C" int ur_temporal_aa(ur_ctx* ctx, const ur_half4* current_frame, const ur_half4* history_band, ur_half4* output_band, float history_weight,
                              uint32_t use_history, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    TaaParams p{};
    const int rc = fill_params("ur_temporal_aa", p, ctx, current_frame, history_band, output_band, history_weight, use_history, w, h, row0, rows);
    if (rc != UR_OK) return rc;
    if (rows == 0) return UR_OK;
    hipLaunchKernelGGL(taa_strip_kernel<NoPost>, dim3((w + 255u) / 256u, (rows + kStripRows - 1u) / kStripRows), dim3(256), 0, ctx->stream, p, NoPost{});
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

extern "C" int ur_temporal_aa_tonemap(ur_ctx* ctx, const ur_tonemap_constants* tonemap, const ur_half4* current_frame, const ur_half4* history_band,
                                      ur_half4* history_out_band, const float* exposure_ev, uint32_t* ldr_out_band, float history_weight,
                                      uint32_t use_history, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    if (!tonemap || !ldr_out_band) { ur::set_error("ur_temporal_aa_tonemap: null argument"); return UR_EINVAL; }
    TaaParams p{};
    const int rc = fill_params("ur_temporal_aa_tonemap", p, ctx, current_frame, history_band, history_out_band, history_weight, use_history, w, h, row0, rows);
    if (rc != UR_OK) return rc;
    if (rows == 0) return UR_OK;
    const ur_post::TonemapParams tm = ur_post::tonemap_params(tonemap, exposure_ev, ldr_out_band);
    const dim3 grid((w + 255u) / 256u, (rows + kStripRows - 1u) / kStripRows);
    if (ctx->opt.taa_tonemap_history_store == 0) hipLaunchKernelGGL(taa_strip_kernel<TonemapPost<true>>, grid, dim3(256), 0, ctx->stream, p, TonemapPost<true>{tm});
    else hipLaunchKernelGGL(taa_strip_kernel<TonemapPost<false>>, grid, dim3(256), 0, ctx->stream, p, TonemapPost<false>{tm});
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

// ---- row bands: the TAA record and the halo forms ---------------------------------------------------------------------------

using ur::overlaps;

extern "C" uint64_t ur_taa_record_bytes(uint32_t w) { return taa_texels(w) * kTexelBytes; }

extern "C" int ur_pack_taa_record(ur_ctx* ctx, const ur_half4* hdr_band, const ur_half4* history_read_band, uint32_t use_history, uint32_t w, uint32_t h,
                                  uint32_t row0, uint32_t rows, void* record)
{
    if (!ctx || !hdr_band || !record || (use_history && !history_read_band)) { ur::set_error("ur_pack_taa_record: null argument"); return UR_EINVAL; }
    if (rows == 0 || !ur::band_in_frame(w, h, row0, rows)) { ur::set_error("ur_pack_taa_record: empty or out-of-frame band"); return UR_EINVAL; }
    if (rows < 2u && rows != h) { ur::set_error("ur_pack_taa_record: a band that is not the whole frame needs at least 2 rows"); return UR_EUNSUPPORTED; }
    const size_t band_bytes = (size_t)w * rows * 8u;
    if (overlaps(hdr_band, band_bytes, record, ur_taa_record_bytes(w)) || (use_history && overlaps(history_read_band, band_bytes, record, ur_taa_record_bytes(w)))) {
        ur::set_error("ur_pack_taa_record: the record overlaps a band");
        return UR_EINVAL;
    }
    const TaaRecordParams p{reinterpret_cast<const u32x2_t*>(hdr_band), use_history ? reinterpret_cast<const u32x2_t*>(history_read_band) : nullptr,
                            static_cast<u32x2_t*>(record), w, rows};
    hipLaunchKernelGGL(taa_record_kernel, dim3((uint32_t)((taa_texels(w) + 255u) / 256u)), dim3(256), 0, ctx->stream, p);
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

// shared checks of the two halo forms; fills the launch parameters and the grid's row count
static int fill_band_params(const char* who, TaaBandParams& q, uint32_t& grid_y, ur_ctx* ctx, const ur_half4* current_band, const ur_half4* cur_above,
                            const ur_half4* cur_below, const ur_half4* history_band, ur_half4* output_band, const ur_half4* above2, const ur_half4* hist_above,
                            const ur_half4* below2, const ur_half4* hist_below, ur_half4* resolved_above, ur_half4* resolved_below, float history_weight,
                            uint32_t use_history, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    TaaParams p{};
    const int rc = fill_params(who, p, ctx, current_band, history_band, output_band, history_weight, use_history, w, h, row0, rows);
    if (rc != UR_OK) return rc;
    if (rows == 0) { ur::set_error("%s: empty band", who); return UR_EINVAL; }
    const bool top = row0 == 0, bottom = row0 + rows == h;
    if ((!top && !cur_above) || (!bottom && !cur_below)) {
        ur::set_error("%s: cur_above may be null only when row0 == 0, cur_below only when row0 + rows == h", who);
        return UR_EINVAL;
    }
    if ((top && (cur_above || above2 || hist_above || resolved_above)) || (bottom && (cur_below || below2 || hist_below || resolved_below))) {
        ur::set_error("%s: there is no row beyond the frame's edge: the pointers of that side must be null", who);
        return UR_EINVAL;
    }
    // a resolved row needs the second current row out and, with history, the neighbour's history row; they come together or not at all
    if ((resolved_above != nullptr) != (above2 != nullptr) || (resolved_below != nullptr) != (below2 != nullptr) ||
        (hist_above && !resolved_above) || (hist_below && !resolved_below) ||
        (use_history && ((resolved_above && !hist_above) || (resolved_below && !hist_below)))) {
        ur::set_error("%s: resolved_above goes with above2 (and hist_above when use_history), resolved_below with below2 (and hist_below)", who);
        return UR_EINVAL;
    }
    const size_t band_bytes = (size_t)w * rows * 8u, row_bytes = (size_t)w * 8u;
    const void* ins[] = {cur_above, cur_below, above2, below2, hist_above, hist_below};
    void* outs[] = {resolved_above, resolved_below};
    for (void* o : outs) {
        if (!o) continue;
        bool bad = overlaps(o, row_bytes, current_band, band_bytes) || overlaps(o, row_bytes, output_band, band_bytes) ||
                   (use_history && overlaps(o, row_bytes, history_band, band_bytes));
        for (const void* i : ins) bad = bad || (i && overlaps(o, row_bytes, i, row_bytes));
        if (bad) { ur::set_error("%s: a resolved row overlaps another buffer", who); return UR_EINVAL; }
    }
    if (resolved_above && resolved_below && overlaps(resolved_above, row_bytes, resolved_below, row_bytes)) { ur::set_error("%s: the resolved rows overlap", who); return UR_EINVAL; }
    bool bad = overlaps(current_band, band_bytes, output_band, band_bytes);
    for (const void* i : ins) bad = bad || (i && overlaps(i, row_bytes, output_band, band_bytes));
    if (bad) { ur::set_error("%s: the output band overlaps a current or neighbour row", who); return UR_EINVAL; }
    const uint32_t strips = (rows + (uint32_t)kStripRows - 1u) / (uint32_t)kStripRows;
    grid_y = strips + (resolved_above ? 1u : 0u) + (resolved_below ? 1u : 0u);
    if (grid_y > 65535u) { ur::set_error("%s: band too tall", who); return UR_EUNSUPPORTED; }
    auto in = [](const ur_half4* x) { return reinterpret_cast<const u32x2_t*>(x); };
    BandRows& R = q.R;
    R.band = in(current_band); R.above = in(cur_above); R.below = in(cur_below); R.above2 = in(above2); R.below2 = in(below2);
    R.history = in(history_band); R.hist_above = in(hist_above); R.hist_below = in(hist_below);
    R.output = reinterpret_cast<u32x2_t*>(output_band); R.res_above = reinterpret_cast<u32x2_t*>(resolved_above); R.res_below = reinterpret_cast<u32x2_t*>(resolved_below);
    R.W = w; R.row0 = row0; R.rows = rows;
    R.ylo = top ? 0u : (above2 ? (row0 >= 2u ? row0 - 2u : 0u) : row0 - 1u);
    R.yhi = bottom ? h - 1u : (below2 ? min(row0 + rows + 1u, h - 1u) : row0 + rows);
    q.H = h; q.weight = p.weight; q.use_history = p.use_history; q.strips = strips;
    return UR_OK;
}

// history_band may BE output_band, as for ur_temporal_aa; the rows around the band and the resolved rows are buffers of their own.
extern "C" int ur_temporal_aa_halo(ur_ctx* ctx, const ur_half4* current_band, const ur_half4* cur_above, const ur_half4* cur_below, const ur_half4* history_band,
                                   ur_half4* output_band, const ur_half4* above2, const ur_half4* hist_above, const ur_half4* below2, const ur_half4* hist_below,
                                   ur_half4* resolved_above, ur_half4* resolved_below, float history_weight, uint32_t use_history, uint32_t w, uint32_t h,
                                   uint32_t row0, uint32_t rows)
{
    TaaBandParams q{};
    uint32_t grid_y = 0;
    const int rc = fill_band_params("ur_temporal_aa_halo", q, grid_y, ctx, current_band, cur_above, cur_below, history_band, output_band, above2, hist_above, below2,
                                    hist_below, resolved_above, resolved_below, history_weight, use_history, w, h, row0, rows);
    if (rc != UR_OK) return rc;
    hipLaunchKernelGGL(taa_band_kernel<NoPost>, dim3((w + 255u) / 256u, grid_y), dim3(256), 0, ctx->stream, q, NoPost{});
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

// The history store keeps its write-once hint under either value of UR_OPT_TAA_TONEMAP_HISTORY_STORE: one form of the band launch.
extern "C" int ur_temporal_aa_tonemap_halo(ur_ctx* ctx, const ur_tonemap_constants* tonemap, const ur_half4* current_band, const ur_half4* cur_above,
                                           const ur_half4* cur_below, const ur_half4* history_band, ur_half4* history_out_band, const float* exposure_ev,
                                           uint32_t* ldr_out_band, const ur_half4* above2, const ur_half4* hist_above, const ur_half4* below2,
                                           const ur_half4* hist_below, ur_half4* resolved_above, ur_half4* resolved_below, float history_weight,
                                           uint32_t use_history, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    if (!tonemap || !ldr_out_band) { ur::set_error("ur_temporal_aa_tonemap_halo: null argument"); return UR_EINVAL; }
    TaaBandParams q{};
    uint32_t grid_y = 0;
    const int rc = fill_band_params("ur_temporal_aa_tonemap_halo", q, grid_y, ctx, current_band, cur_above, cur_below, history_band, history_out_band, above2,
                                    hist_above, below2, hist_below, resolved_above, resolved_below, history_weight, use_history, w, h, row0, rows);
    if (rc != UR_OK) return rc;
    const ur_post::TonemapParams tm = ur_post::tonemap_params(tonemap, exposure_ev, ldr_out_band);
    hipLaunchKernelGGL(taa_band_kernel<TonemapPost<true>>, dim3((w + 255u) / 256u, grid_y), dim3(256), 0, ctx->stream, q, TonemapPost<true>{tm});
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}
