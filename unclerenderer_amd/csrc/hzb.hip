// BuildHZB for gfx950 — min-depth mip chain (reverse-Z: min == farthest).
//
// Reference: Shaders/BuildHZB.hlsl:34-126 (8x8 groups, <=4 mips per dispatch through groupshared tiles) and the
// dispatch loop Source/Render/DeferredRenderer.cpp:1046-1207. The values produced here are bit-identical to that
// chain, including its out-of-range fills (1.0 below the first mip of a dispatch, 0.0 below the second and third —
// BuildHZB.hlsl:47,81,104). What is NOT kept is the reference's launch shape: one workgroup here is
// four wave64s covering a 128x32 source tile; each lane owns a 4x4 source block in registers (four 16-byte loads,
// 512 contiguous bytes per wave row), so mips k and k+1 never touch LDS, mip k+2 is two DPP/shuffle steps inside the
// wave (lane^1, lane^32) and only mip k+3 crosses waves through a 64-float LDS tile. One barrier per workgroup instead
// of three; HBM traffic == algorithmic bytes (every source texel read once, every mip texel written once).
//
// Built with -ffp-contract=off; the only arithmetic is fminf, on quieted operands (hzb_min4, hzb_tail.h: HLSL min ignores a
// NaN operand, a signalling one included).
//
// The host half executes a plan: which levels a launch takes, on which grid, and whether it goes out now or is held for the next
// streaming Lighting launch is decided in csrc/hzb_plan.cpp (plain C++, tested without a GPU); here a step is bound to its buffers
// and launched, or handed to the context's ur::HeldHzb. The Build HZB entry points of include/ur_hotpath.h are at the end.

#include "ur_internal.h"
#include "ur_device.h"
#include "hzb_tail.h"
#include "hzb_wide.h"

namespace {

using ur::HzbDispatch;

using ur::hzb_min4;

__global__ __launch_bounds__(256) void hzb_reduce4_kernel(HzbDispatch p)
{
    __shared__ float sh2[4][16];
    __shared__ float sh3[2][8];

    const uint32_t tx = threadIdx.x & 31u, ty = threadIdx.x >> 5;
    const uint32_t by = blockIdx.y + p.by0; // (a band-sharded launch starts at its rank's first piece row)
    const uint32_t x1 = blockIdx.x * 32u + tx, y1 = by * 8u + ty; // coords in mip k+1 (== 4x4 source block index)
    const uint32_t sx = x1 * 4u, sy = y1 * 4u;

    // ---- mip k: four texels (2x1+i, 2y1+j) from the 4x4 source block, clamped reads (SampleDepth, :34-39)
    float v0[2][2] = {{1.0f, 1.0f}, {1.0f, 1.0f}}; // out-of-range lanes hold 1.0 (:47)
    const bool any0 = (x1 * 2u < p.W[0]) && (y1 * 2u < p.H[0]);
    if (any0) {
        float s[4][4];
        if (p.vec4_ok && sx + 3u < p.SW && sy + 3u < p.SH) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                typedef float f32x4_t __attribute__((ext_vector_type(4)));
                const f32x4_t q = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(p.src + (size_t)(sy + r) * p.SW + sx)); // read once
                s[r][0] = q.x; s[r][1] = q.y; s[r][2] = q.z; s[r][3] = q.w;
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t yy = min(sy + r, p.SH - 1u);
#pragma unroll
                for (int c = 0; c < 4; ++c) s[r][c] = p.src[(size_t)yy * p.SW + min(sx + c, p.SW - 1u)];
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const uint32_t x0 = x1 * 2u + i, y0 = y1 * 2u + j;
                if (x0 < p.W[0] && y0 < p.H[0]) v0[j][i] = hzb_min4(s[2 * j][2 * i], s[2 * j][2 * i + 1], s[2 * j + 1][2 * i], s[2 * j + 1][2 * i + 1]);
            }
        float* d0 = p.dst[0];
        const uint32_t x0 = x1 * 2u, y0 = y1 * 2u;
        if (p.pair_ok && x0 + 1u < p.W[0]) { // 8-byte aligned pair
            ur::store_once_b64(d0 + (size_t)y0 * p.W[0] + x0, ur::once_u32x2_t{__float_as_uint(v0[0][0]), __float_as_uint(v0[0][1])}); // written once, read by a later launch
            if (y0 + 1u < p.H[0]) ur::store_once_b64(d0 + (size_t)(y0 + 1u) * p.W[0] + x0, ur::once_u32x2_t{__float_as_uint(v0[1][0]), __float_as_uint(v0[1][1])});
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    if (x0 + i < p.W[0] && y0 + j < p.H[0]) d0[(size_t)(y0 + j) * p.W[0] + x0 + i] = v0[j][i];
        }
    }
    if (p.mips < 2u) return;

    // ---- mip k+1: this lane's texel; out-of-range lanes hold 0.0 (:81)
    float v1 = 0.0f;
    if (x1 < p.W[1] && y1 < p.H[1]) {
        v1 = hzb_min4(v0[0][0], v0[0][1], v0[1][0], v0[1][1]);
        p.dst[1][(size_t)y1 * p.W[1] + x1] = v1;
    }
    if (p.mips < 3u) return; // uniform

    // ---- mip k+2: 2x2 of v1 lives in lanes {l, l^1, l^32, l^33} of this wave (wave = rows 2w, 2w+1 of the tile)
    float m = fminf(v1, __shfl_xor(v1, 1));
    m = fminf(m, __shfl_xor(m, 32));
    const uint32_t x2 = x1 >> 1, y2 = y1 >> 1;
    float v2 = 0.0f; // out-of-range holds 0.0 (:104)
    if (x2 < p.W[2] && y2 < p.H[2]) v2 = m;
    if (((tx | ty) & 1u) == 0u) {
        if (x2 < p.W[2] && y2 < p.H[2]) p.dst[2][(size_t)y2 * p.W[2] + x2] = v2;
        sh2[ty >> 1][tx >> 1] = v2;
    }
    if (p.mips < 4u) return; // uniform
    __syncthreads();

    // ---- mip k+3: 2x2 of v2 through LDS
    if (((tx | ty) & 3u) == 0u) {
        const uint32_t x3 = x1 >> 2, y3 = y1 >> 2;
        if (x3 < p.W[3] && y3 < p.H[3]) {
            const uint32_t cx = tx >> 1, cy = ty >> 1;
            const float v3 = hzb_min4(sh2[cy][cx], sh2[cy][cx + 1], sh2[cy + 1][cx], sh2[cy + 1][cx + 1]);
            p.dst[3][(size_t)y3 * p.W[3] + x3] = v3;
            sh3[ty >> 2][tx >> 2] = v3;
        }
    }
    if (p.mips < 5u) return; // uniform
    __syncthreads();

    // ---- mip k+4 = the FIRST level of the reference's next dispatch, produced here so that the single-workgroup tail
    //      launch starts from a mip a quarter the size: clamped 2x2 footprints of mip k+3 (SampleDepth, :34-39). The
    //      workgroup's 8x2 texels of mip k+3 hold every tap: a clamped coordinate of an in-range texel stays in its pair.
    if (threadIdx.x < 4u) {
        const uint32_t x4 = blockIdx.x * 4u + threadIdx.x, y4 = by;
        if (x4 < p.W[4] && y4 < p.H[4]) {
            const uint32_t c0 = min(2u * x4, p.W[3] - 1u) & 7u, c1 = min(2u * x4 + 1u, p.W[3] - 1u) & 7u;
            const uint32_t r0 = min(2u * y4, p.H[3] - 1u) & 1u, r1 = min(2u * y4 + 1u, p.H[3] - 1u) & 1u;
            p.dst[4][(size_t)y4 * p.W[4] + x4] = hzb_min4(sh3[r0][c0], sh3[r0][c1], sh3[r1][c0], sh3[r1][c1]);
        }
    }
}

__global__ __launch_bounds__(1024) void hzb_tail_kernel(ur::HzbTail p)
{
    __shared__ float bufA[ur::kTailTexels], bufB[ur::kTailTexels / 2];
    ur::hzb_tail_run(p, bufA, bufB);
}

} // namespace

namespace ur {

// One wide step of a plan bound to its buffers: the kernel's arguments
static HzbDispatch bind_wide(const HzbStep& s, const float* depth, uint32_t src_w, uint32_t src_h, float* hzb, const ur_mip_desc* mips)
{
    HzbDispatch d{};
    if (s.from_depth) {
        d.src = depth;
        d.SW = src_w;
        d.SH = src_h;
    } else {
        d.src = hzb + mips[s.first - 1].offset;
        d.SW = mips[s.first - 1].width;
        d.SH = mips[s.first - 1].height;
    }
    for (uint32_t k = 0; k < 5; ++k) {
        if (k < s.levels) {
            d.dst[k] = hzb + mips[s.first + k].offset;
            d.W[k] = mips[s.first + k].width;
            d.H[k] = mips[s.first + k].height;
        } else {
            d.dst[k] = nullptr;
            d.W[k] = 0;
            d.H[k] = 0;
        }
    }
    d.mips = s.levels;
    d.vec4_ok = ((d.SW & 3u) == 0u && (reinterpret_cast<uintptr_t>(d.src) & 15u) == 0u) ? 1u : 0u;
    d.pair_ok = ((d.W[0] & 1u) == 0u && (reinterpret_cast<uintptr_t>(d.dst[0]) & 7u) == 0u) ? 1u : 0u;
    d.by0 = s.by0;
    return d;
}

// The tail step of a plan bound to its buffers
static HzbTail bind_tail(const HzbStep& s, float* hzb, const ur_mip_desc* mips)
{
    HzbTail t{};
    t.src = hzb + mips[s.first - 1].offset;
    t.SW = mips[s.first - 1].width;
    t.SH = mips[s.first - 1].height;
    t.first_mip = s.first;
    t.levels = s.levels;
    for (uint32_t k = 0; k < t.levels; ++k) {
        t.dst[k] = hzb + mips[s.first + k].offset;
        t.W[k] = mips[s.first + k].width;
        t.H[k] = mips[s.first + k].height;
        t.magic[k] = t.W[k] > 1u ? (uint32_t)((1ull << 32) / t.W[k] + 1ull) : 0u; // W == 1: y = i (handled in the kernel)
    }
    return t;
}

static int launch_wide(ur_ctx* ctx, const HzbDispatch& d, uint32_t grid_x, uint32_t grid_y)
{
    hipLaunchKernelGGL(hzb_reduce4_kernel, dim3(grid_x, grid_y), dim3(256), 0, ctx->stream, d);
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

static int launch_tail(ur_ctx* ctx, const HzbTail& t)
{
    hipLaunchKernelGGL(hzb_tail_kernel, dim3(1), dim3(1024), 0, ctx->stream, t);
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

// Every step of a plan in order: launched, or held on the context for the next streaming Lighting launch (ur_flush otherwise)
static int run_plan(ur_ctx* ctx, const HzbPlan& plan, const float* depth, uint32_t src_w, uint32_t src_h, float* hzb, const ur_mip_desc* mips)
{
    for (uint32_t i = 0; i < plan.count; ++i) {
        const HzbStep& s = plan.steps[i];
        int rc = UR_OK;
        if (s.kind == HzbStep::wide) {
            const HzbDispatch d = bind_wide(s, depth, src_w, src_h, hzb, mips);
            if (s.hold) ctx->held_hzb.hold_wide(d, s.grid_x, s.grid_y);
            else rc = launch_wide(ctx, d, s.grid_x, s.grid_y);
        } else {
            const HzbTail t = bind_tail(s, hzb, mips);
            if (s.hold) ctx->held_hzb.hold_tail(t);
            else rc = launch_tail(ctx, t);
        }
        if (rc != UR_OK) return rc;
    }
    return UR_OK;
}

// The three forms below: flush what is held (an earlier chain's tail must not run after this chain's levels), plan (csrc/hzb_plan.cpp),
// then launch or hold each step.
int launch_build_hzb(ur_ctx* ctx, const float* depth, uint32_t src_w, uint32_t src_h, float* hzb, const ur_mip_desc* mips,
                     uint32_t mip_count)
{
    const int rc = flush_hzb_tail(ctx);
    if (rc != UR_OK) return rc;
    const HzbPlan plan = plan_hzb_chain(src_w, src_h, mips, mip_count, ctx->held_hzb.mode(), ctx->hzb_done != nullptr);
    if (plan.status != HzbPlan::ok) { set_error("ur_build_hzb: mip chain does not match CreateHZBResources sizing"); return UR_EINVAL; }
    return run_plan(ctx, plan, depth, src_w, src_h, hzb, mips);
}

int launch_build_hzb_band(ur_ctx* ctx, const float* depth, uint32_t src_w, uint32_t src_h, float* hzb, const ur_mip_desc* mips, uint32_t mip_count,
                          uint32_t piece_row0, uint32_t piece_rows)
{
    const int rc = flush_hzb_tail(ctx);
    if (rc != UR_OK) return rc;
    const HzbPlan plan = plan_hzb_band(src_w, src_h, mips, mip_count, ctx->held_hzb.mode(), piece_row0, piece_rows);
    if (plan.status == HzbPlan::not_wide_plus_tail) {
        set_error("ur_build_hzb_band: a %u x %u frame's chain is not one five-level launch plus the tail (build it whole: ur_build_hzb)", src_w, src_h);
        return UR_EUNSUPPORTED;
    }
    if (plan.status != HzbPlan::ok) { set_error("ur_build_hzb_band: mip chain does not match CreateHZBResources sizing"); return UR_EINVAL; }
    return run_plan(ctx, plan, depth, src_w, src_h, hzb, mips);
}

int launch_build_hzb_tail(ur_ctx* ctx, float* hzb, const ur_mip_desc* mips, uint32_t mip_count)
{
    const int rc = flush_hzb_tail(ctx);
    if (rc != UR_OK) return rc;
    const HzbPlan plan = plan_hzb_tail(mips, mip_count);
    if (plan.status == HzbPlan::not_wide_plus_tail) {
        set_error("ur_build_hzb_tail: the chain is not one five-level launch plus the tail");
        return UR_EUNSUPPORTED;
    }
    if (plan.status != HzbPlan::ok) { set_error("ur_build_hzb_tail: bad argument"); return UR_EINVAL; }
    return run_plan(ctx, plan, nullptr, 0u, 0u, hzb, mips);
}

int flush_hzb_tail(ur_ctx* ctx)
{
    if (ctx->held_hzb.has_wide()) { // the held-back wide launch goes first (the tail reads what it writes)
        const HeldHzb::Wide& w = ctx->held_hzb.take_wide();
        const int rc = launch_wide(ctx, w.d, w.grid_x, w.grid_y);
        if (rc != UR_OK) return rc;
    }
    if (!ctx->held_hzb.has_tail()) return UR_OK;
    return launch_tail(ctx, ctx->held_hzb.take_tail());
}

int check_hzb_timeout(ur_ctx* ctx, const char* who)
{
    if (ctx && ctx->claim_timed_out && *ctx->claim_timed_out != 0u) {
        *ctx->claim_timed_out = 0u;
        (void)hipMemsetAsync(ctx->claim_words, 0, (kClaimWords + 1u) * kClaimWordStride * sizeof(uint32_t), ctx->stream);
        set_error("%s: a wave of a balanced Lighting launch gave up waiting for a tile claim of its workgroup: tiles of that launch were not shaded — "
                  "shade the frame again (reported once; the context is usable)", who);
        return UR_ETIMEOUT;
    }
    if (!ctx || !ctx->hzb_timed_out || *ctx->hzb_timed_out == 0u) return UR_OK;
    *ctx->hzb_timed_out = 0u;
    (void)hipMemsetAsync(ctx->hzb_done, 0, 64, ctx->stream); // stragglers may have left any count behind
    set_error("%s: the tail of a Build HZB chain that rode a Lighting launch gave up waiting for its producers: the HZB's small levels are stale — "
              "build it again (reported once; the context is usable)", who);
    return UR_ETIMEOUT;
}

} // namespace ur

// ---- the entry points (include/ur_hotpath.h): argument checks and error texts; the arithmetic is csrc/hzb_plan.cpp's ----

using ur::set_error;

extern "C" {

int ur_defer_hzb_tail(ur_ctx* ctx, int enable)
{
    if (!ctx) { set_error("ur_defer_hzb_tail: null context"); return UR_EINVAL; }
    if (enable < 0 || enable > 2) { set_error("ur_defer_hzb_tail: mode %d (0 off, 1 tail, 2 whole chain)", enable); return UR_EINVAL; }
    return ctx->held_hzb.set_mode(enable) ? ur::flush_hzb_tail(ctx) : UR_OK; // (a narrower mode flushes)
}

int ur_flush(ur_ctx* ctx)
{
    if (!ctx) { set_error("ur_flush: null context"); return UR_EINVAL; }
    const int trc = ur::check_hzb_timeout(ctx, "ur_flush");
    if (trc != UR_OK) return trc;
    return ur::flush_hzb_tail(ctx);
}

uint32_t ur_hzb_layout(uint32_t src_w, uint32_t src_h, ur_mip_desc* mips, uint32_t* mip_count)
{
    if (!mips || !mip_count || src_w == 0 || src_h == 0) return 0;
    return ur::hzb_layout(src_w, src_h, mips, mip_count);
}

int ur_build_hzb(ur_ctx* ctx, const float* depth, uint32_t src_w, uint32_t src_h, float* hzb_base, const ur_mip_desc* mips,
                 uint32_t mip_count)
{
    if (!ctx || !depth || !hzb_base || src_w == 0 || src_h == 0) { set_error("ur_build_hzb: null/zero argument"); return UR_EINVAL; }
    if (!ur::valid_hzb_chain(src_w, src_h, mips, mip_count)) { set_error("ur_build_hzb: mip chain does not match CreateHZBResources sizing"); return UR_EINVAL; }
    const int trc = ur::check_hzb_timeout(ctx, "ur_build_hzb");
    if (trc != UR_OK) return trc;
    return ur::launch_build_hzb(ctx, depth, src_w, src_h, hzb_base, mips, mip_count);
}

int ur_hzb_band_pieces(uint32_t src_h, uint32_t n_ranks, uint32_t rank, uint32_t* piece_row0, uint32_t* piece_rows)
{
    if (src_h == 0 || n_ranks == 0 || rank >= n_ranks || src_h % n_ranks != 0 || !piece_row0 || !piece_rows) { set_error("ur_hzb_band_pieces: bad argument"); return UR_EINVAL; }
    ur::hzb_band_pieces(src_h, n_ranks, rank, piece_row0, piece_rows);
    return UR_OK;
}

int ur_hzb_band_slices(const ur_mip_desc* mips, uint32_t mip_count, uint32_t piece_row0, uint32_t piece_rows, ur_hzb_slice* out5)
{
    if (!mips || mip_count < 5 || !out5) { set_error("ur_hzb_band_slices: bad argument"); return UR_EINVAL; }
    ur::hzb_band_slices(mips, piece_row0, piece_rows, out5);
    return UR_OK;
}

int ur_build_hzb_band(ur_ctx* ctx, const float* depth, uint32_t src_w, uint32_t src_h, float* hzb_base, const ur_mip_desc* mips, uint32_t mip_count,
                      uint32_t piece_row0, uint32_t piece_rows)
{
    if (!ctx || !depth || !hzb_base || src_w == 0 || src_h == 0) { set_error("ur_build_hzb_band: null/zero argument"); return UR_EINVAL; }
    if (!ur::valid_hzb_chain(src_w, src_h, mips, mip_count)) { set_error("ur_build_hzb_band: mip chain does not match CreateHZBResources sizing"); return UR_EINVAL; }
    if ((uint64_t)piece_row0 + piece_rows > (src_h + 31u) / 32u) { set_error("ur_build_hzb_band: piece rows [%u, %u) of %u", piece_row0, piece_row0 + piece_rows, (src_h + 31u) / 32u); return UR_EINVAL; }
    const int trc = ur::check_hzb_timeout(ctx, "ur_build_hzb_band");
    if (trc != UR_OK) return trc;
    return ur::launch_build_hzb_band(ctx, depth, src_w, src_h, hzb_base, mips, mip_count, piece_row0, piece_rows);
}

int ur_build_hzb_tail(ur_ctx* ctx, float* hzb_base, const ur_mip_desc* mips, uint32_t mip_count)
{
    if (!ctx || !hzb_base || !ur::valid_hzb_chain_below_mip0(mips, mip_count)) { set_error("ur_build_hzb_tail: bad argument"); return UR_EINVAL; }
    const int trc = ur::check_hzb_timeout(ctx, "ur_build_hzb_tail");
    if (trc != UR_OK) return trc;
    return ur::launch_build_hzb_tail(ctx, hzb_base, mips, mip_count);
}

} // extern "C"
