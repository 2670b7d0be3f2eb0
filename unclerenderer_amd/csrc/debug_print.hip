// GpuDebugPrint for gfx950 — the reference's GPU-side text facility and its last frame pass.
//
// Reference: Shaders/DebugPrintCommon.hlsl (the buffer: a 4-byte entry count, then up to 4096 entries {x, y, code, color} of 16 bytes;
// PrintChar takes a slot with one atomic add and drops the entry when the slot is >= 4096, the count keeps growing),
// Shaders/GpuDebugPrintStats.hlsl (one thread prints "FRUSTUM n" / "OCCLUDE n" from the cull's two counters),
// Shaders/GpuDebugPrint.hlsl + Renderer.cpp:626-724, 824-884 (6 x 4096 vertices, one axis-aligned glyph quad per entry, alpha-blended
// SRC_ALPHA / INV_SRC_ALPHA onto the back buffer, alpha ONE / ZERO, no depth), pass DeferredRenderer.cpp:1575-1598.
//
// The draw has an exact compute form: a pixel is covered by an entry iff its centre lies in the half-open quad
// [min, max) evaluated on the fp32 pixel-space corners; entries blend in entry order; the target is 8-bit between blends. One workgroup
// owns a 64 x 64 tile, walks the min(count, 4096) entries in chunks of 256 and keeps, with a wave64 ballot + popcount, the ASCENDING list
// of the entries whose quad touches the tile in LDS (the idiom of the cull's compaction: the order, hence the image, is deterministic).
// A tile with an empty list returns without touching the image: the cost follows the text, not the frame.
// Built with -ffp-contract=off: the arithmetic below is the operation count the test's error bound is derived from.

#include "ur_internal.h"

namespace {

constexpr uint32_t kHeaderDwords = 1u;   // kDebugPrintHeaderSize = 4 bytes
constexpr uint32_t kEntryDwords = 4u;    // kDebugPrintEntryStride = 16 bytes
constexpr uint32_t kMaxEntries = UR_DEBUG_PRINT_MAX_ENTRIES;
constexpr uint32_t kAdvance = 8u;        // kDebugPrintDefaultAdvance
constexpr uint32_t kTextChunk = 256u;    // characters per ur_debug_print_text launch

// DebugPrintCommon.hlsl:20-34
__device__ __forceinline__ void print_char(uint32_t* buf, uint32_t x, uint32_t y, uint32_t code, uint32_t color)
{
    const uint32_t index = atomicAdd(buf, 1u);
    if (index >= kMaxEntries) return;
    uint32_t* e = buf + kHeaderDwords + index * kEntryDwords;
    e[0] = x; e[1] = y; e[2] = code; e[3] = color;
}

// PrintLabel / PrintString (GpuDebugPrintStats.hlsl:6-11, DebugPrintCommon.hlsl:36-51): eight characters, stops at a zero code
__device__ void print_label(uint32_t* buf, uint32_t x, uint32_t y, uint32_t color, const char (&c)[9])
{
    for (uint32_t i = 0; i < 8u; ++i) {
        const uint32_t code = (uint32_t)(uint8_t)c[i];
        if (code == 0u) return;
        print_char(buf, x, y, code, color);
        x += kAdvance;
    }
}

// GpuDebugPrintStats.hlsl:13-31, as written: a value >= 100000 makes the first "digit" exceed 9
__device__ void print_uint(uint32_t* buf, uint32_t x, uint32_t y, uint32_t value, uint32_t color)
{
    uint32_t divisor = 10000u;
    bool started = false;
    for (uint32_t i = 0; i < 5u; ++i) {
        const uint32_t digit = value / divisor;
        value -= digit * divisor;
        divisor = max(1u, divisor / 10u);
        if (digit != 0u || started || i == 4u) {
            started = true;
            print_char(buf, x, y, 48u + digit, color);
            x += kAdvance;
        }
    }
}

// GpuDebugPrintStats.hlsl:33-47, [numthreads(1, 1, 1)]
__global__ __launch_bounds__(64) void debug_print_stats_kernel(const uint32_t* __restrict__ stats, uint32_t* __restrict__ buf)
{
    if (threadIdx.x != 0u || blockIdx.x != 0u) return;
    const uint32_t frustum = stats[0], occlusion = stats[1];
    const uint32_t textColor = 0xffffffffu;
    print_label(buf, 8u, 20u, textColor, "FRUSTUM ");
    print_uint(buf, 8u + 8u * 8u, 20u, frustum, textColor);
    print_label(buf, 8u, 36u, textColor, "OCCLUDE ");
    print_uint(buf, 8u + 8u * 8u, 36u, occlusion, textColor);
}

// PrepareGpuDebugPrint (Renderer.cpp:474-527): the count word and, when given, the two stats words
__global__ __launch_bounds__(64) void debug_print_reset_kernel(uint32_t* __restrict__ buf, uint32_t* __restrict__ stats)
{
    if (blockIdx.x != 0u) return;
    if (threadIdx.x == 0u) buf[0] = 0u;
    if (stats != nullptr && threadIdx.x >= 1u && threadIdx.x <= 2u) stats[threadIdx.x - 1u] = 0u;
}

// PrintString for a caller's string: `count` characters (the host has cut the string at its first zero code), character i at
// x + 8 i. The slots are taken with ONE add of `count`: the string's entries are consecutive whatever else prints, and with no
// other printer the buffer is what `count` PrintChar calls leave, entries past 4096 dropped and the count still counting.
struct TextChunk { uint8_t c[kTextChunk]; };
__global__ __launch_bounds__(kTextChunk) void debug_print_text_kernel(uint32_t* __restrict__ buf, uint32_t x, uint32_t y, uint32_t color, uint32_t count,
                                                                      TextChunk text)
{
    __shared__ uint32_t base;
    if (threadIdx.x == 0u) base = atomicAdd(buf, count);
    __syncthreads();
    const uint32_t i = threadIdx.x;
    if (i >= count) return;
    const uint32_t index = base + i;
    if (index < base || index >= kMaxEntries) return; // (a count word that wrapped: dropped like any slot past the end)
    uint32_t* e = buf + kHeaderDwords + index * kEntryDwords;
    e[0] = x + kAdvance * i; e[1] = y; e[2] = text.c[i]; e[3] = color;
}

// ---- the composite ----------------------------------------------------------------------------------------------------------------

constexpr uint32_t kTileW = 64u, kTileH = 64u, kThreads = 256u, kRowsPerThread = kTileW * kTileH / kThreads; // 16 rows, 4 apart
constexpr uint32_t kRowStep = kThreads / kTileW;

struct DrawParams {
    const ur_debug_glyph* glyphs;
    const uint8_t* atlas;
    const uint32_t* buf;
    uint32_t* ldr;          // band-local: rows [row0, row0 + rows)
    uint32_t glyph_count, atlas_w, atlas_h;
    uint32_t first_char, char_count;
    uint32_t w, row0, rows;
};

// The quad of an entry in pixels, fp32: [pos + Offset, pos + Offset + Size). false: the entry draws nothing (GpuDebugPrint.hlsl:51-66
// sends it off-screen; a glyph index past the table reads zeros in D3D, an empty quad).
struct Quad { float minx, miny, maxx, maxy; };
__device__ __forceinline__ bool entry_quad(const DrawParams& p, uint32_t posx, uint32_t posy, uint32_t code, Quad& q)
{
    if (code < p.first_char || code >= p.first_char + p.char_count) return false;
    if (code >= p.glyph_count) return false;
    const ur_debug_glyph& g = p.glyphs[code];
    q.minx = (float)posx + g.Offset[0];
    q.miny = (float)posy + g.Offset[1];
    q.maxx = q.minx + g.Size[0];
    q.maxy = q.miny + g.Size[1];
    return q.minx < q.maxx && q.miny < q.maxy; // empty, negative and NaN quads cover nothing
}

// R8_UNORM texel, clamp addressing
__device__ __forceinline__ float atlas_texel(const DrawParams& p, int x, int y)
{
    x = min(max(x, 0), (int)p.atlas_w - 1);
    y = min(max(y, 0), (int)p.atlas_h - 1);
    return (float)p.atlas[(size_t)y * p.atlas_w + (uint32_t)x] / 255.0f;
}

__device__ __forceinline__ uint32_t unorm8(float x) { return (uint32_t)(fminf(fmaxf(x, 0.0f), 1.0f) * 255.0f + 0.5f); } // (NaN -> 0)

__global__ __launch_bounds__(kThreads) void debug_print_draw_kernel(DrawParams p)
{
    __shared__ uint16_t list[kMaxEntries];
    __shared__ uint32_t wave_counts[kThreads / 64u];
    __shared__ uint32_t list_count;

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t total = min(p.buf[0], kMaxEntries);
    const uint32_t tx0 = blockIdx.x * kTileW, ty0 = p.row0 + blockIdx.y * kTileH; // frame coordinates
    // the tile's pixel centres span [tx0 + 0.5, tx1 - 0.5], [ty0 + 0.5, ty1 - 0.5]
    const float cx0 = (float)tx0 + 0.5f, cx1 = (float)min(tx0 + kTileW, p.w) - 0.5f;
    const float cy0 = (float)ty0 + 0.5f, cy1 = (float)min(ty0 + kTileH, p.row0 + p.rows) - 0.5f;

    if (tid == 0u) list_count = 0u;
    __syncthreads();
    for (uint32_t chunk = 0; chunk < total; chunk += kThreads) {
        const uint32_t i = chunk + tid;
        bool touches = false;
        if (i < total) {
            const uint32_t* e = p.buf + kHeaderDwords + i * kEntryDwords;
            Quad q;
            // some pixel centre c of the tile has min <= c < max
            if (entry_quad(p, e[0], e[1], e[2], q)) touches = q.minx <= cx1 && cx0 < q.maxx && q.miny <= cy1 && cy0 < q.maxy;
        }
        const unsigned long long mask = __ballot(touches);
        if (lane == 0u) wave_counts[wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t before = list_count;
        for (uint32_t v = 0; v < wave; ++v) before += wave_counts[v];
        if (touches) list[before + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = (uint16_t)i;
        __syncthreads();
        if (tid == 0u) list_count += wave_counts[0] + wave_counts[1] + wave_counts[2] + wave_counts[3];
        __syncthreads();
    }
    const uint32_t n = list_count;
    if (n == 0u) return; // nothing of the text in this tile: the image is neither read nor written

    const uint32_t px = tx0 + (tid & (kTileW - 1u));
    const uint32_t ly0 = blockIdx.y * kTileH + tid / kTileW; // band-local row of this thread's first pixel
    const bool in_x = px < p.w;
    const float cx = (float)px + 0.5f;
    uint32_t pix[kRowsPerThread];
    uint32_t dirty = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kRowsPerThread; ++k) {
        const uint32_t ly = ly0 + k * kRowStep;
        pix[k] = (in_x && ly < p.rows) ? p.ldr[(size_t)ly * p.w + px] : 0u;
    }
    const float aw = (float)p.atlas_w, ah = (float)p.atlas_h;
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t i = __builtin_amdgcn_readfirstlane((uint32_t)list[j]); // uniform: the entry and its glyph are scalar loads
        const uint32_t* e = p.buf + kHeaderDwords + i * kEntryDwords;
        const uint32_t code = e[2], color = e[3];
        Quad q;
        if (!entry_quad(p, e[0], e[1], code, q)) continue; // (listed entries have a quad; keeps the glyph index in range for the compiler too)
        if (!(in_x && q.minx <= cx && cx < q.maxx)) continue;
        const ur_debug_glyph& g = p.glyphs[code];
        // UnpackColor (GpuDebugPrint.hlsl:33-40)
        const float cr = (float)(color & 255u) / 255.0f, cg = (float)((color >> 8) & 255u) / 255.0f, cb = (float)((color >> 16) & 255u) / 255.0f,
                    ca = (float)(color >> 24) / 255.0f;
        // UV = UvMin + (centre - min) / Size * (UvMax - UvMin); the tap position t = uv * size - 0.5
        const float u = g.UvMin[0] + (cx - q.minx) / g.Size[0] * (g.UvMax[0] - g.UvMin[0]);
        const float tu = u * aw - 0.5f, fu = floorf(tu), wu = tu - fu;
        const int iu = (int)fu;
        const float dv = g.UvMax[1] - g.UvMin[1];
#pragma unroll
        for (uint32_t k = 0; k < kRowsPerThread; ++k) {
            const uint32_t ly = ly0 + k * kRowStep;
            const float cy = (float)(p.row0 + ly) + 0.5f;
            if (!(ly < p.rows && q.miny <= cy && cy < q.maxy)) continue;
            const float v = g.UvMin[1] + (cy - q.miny) / g.Size[1] * dv;
            const float tv = v * ah - 0.5f, fv = floorf(tv), wv = tv - fv;
            const int iv = (int)fv;
            const float t00 = atlas_texel(p, iu, iv), t10 = atlas_texel(p, iu + 1, iv), t01 = atlas_texel(p, iu, iv + 1), t11 = atlas_texel(p, iu + 1, iv + 1);
            const float top = t00 + (t10 - t00) * wu, bot = t01 + (t11 - t01) * wu;
            const float a = ca * (top + (bot - top) * wv); // PSMain: Color.a * alpha
            // SRC_ALPHA / INV_SRC_ALPHA on the UNORM values, alpha ONE / ZERO; one rounding to 8 bits per channel per entry
            const uint32_t d = pix[k];
            const float ia = 1.0f - a;
            const float dr = (float)(d & 255u) / 255.0f, dg = (float)((d >> 8) & 255u) / 255.0f, db = (float)((d >> 16) & 255u) / 255.0f;
            pix[k] = unorm8(cr * a + dr * ia) | (unorm8(cg * a + dg * ia) << 8) | (unorm8(cb * a + db * ia) << 16) | (unorm8(a) << 24);
            dirty |= 1u << k;
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < kRowsPerThread; ++k) {
        const uint32_t ly = ly0 + k * kRowStep;
        if (dirty & (1u << k)) p.ldr[(size_t)ly * p.w + px] = pix[k];
    }
}

} // namespace

namespace ur {

int launch_debug_print_reset(ur_ctx* ctx, void* buffer, uint32_t* stats)
{
    hipLaunchKernelGGL(debug_print_reset_kernel, dim3(1), dim3(64), 0, ctx->stream, static_cast<uint32_t*>(buffer), stats);
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

int launch_debug_print_stats(ur_ctx* ctx, const uint32_t* stats, void* buffer)
{
    hipLaunchKernelGGL(debug_print_stats_kernel, dim3(1), dim3(64), 0, ctx->stream, stats, static_cast<uint32_t*>(buffer));
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

int launch_debug_print_text(ur_ctx* ctx, void* buffer, uint32_t x, uint32_t y, uint32_t color, const char* text, uint32_t length)
{
    // PrintString stops at a zero code
    uint32_t n = 0;
    while (n < length && text[n] != 0) ++n;
    for (uint32_t at = 0; at < n; at += kTextChunk) {
        TextChunk chunk = {};
        const uint32_t count = n - at < kTextChunk ? n - at : kTextChunk;
        for (uint32_t i = 0; i < count; ++i) chunk.c[i] = (uint8_t)text[at + i];
        hipLaunchKernelGGL(debug_print_text_kernel, dim3(1), dim3(kTextChunk), 0, ctx->stream, static_cast<uint32_t*>(buffer), x + kAdvance * at, y, color,
                           count, chunk);
        UR_HIP_TRY(hipGetLastError());
    }
    return UR_OK;
}

int launch_debug_print_draw(ur_ctx* ctx, const ur_debug_print_constants* constants, const ur_debug_glyph* glyphs, uint32_t glyph_count,
                            const uint8_t* atlas_r8, uint32_t atlas_w, uint32_t atlas_h, const void* buffer, uint32_t* ldr_inout, uint32_t w,
                            uint32_t row0, uint32_t rows)
{
    if (rows == 0) return UR_OK;
    DrawParams p{};
    p.glyphs = glyphs; p.atlas = atlas_r8; p.buf = static_cast<const uint32_t*>(buffer); p.ldr = ldr_inout;
    p.glyph_count = glyph_count; p.atlas_w = atlas_w; p.atlas_h = atlas_h;
    p.first_char = constants->FirstChar; p.char_count = constants->CharCount;
    p.w = w; p.row0 = row0; p.rows = rows;
    const dim3 grid((w + kTileW - 1u) / kTileW, (rows + kTileH - 1u) / kTileH);
    if (grid.y > 65535u) { set_error("ur_debug_print_draw: band too tall"); return UR_EUNSUPPORTED; }
    hipLaunchKernelGGL(debug_print_draw_kernel, grid, dim3(kThreads), 0, ctx->stream, p);
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

} // namespace ur

// ---- the entry points (include/ur_hotpath.h) ----

using ur::set_error;

extern "C" {

uint64_t ur_debug_print_buffer_bytes(void) { return 4u + (uint64_t)UR_DEBUG_PRINT_MAX_ENTRIES * 16u; }

int ur_debug_print_reset(ur_ctx* ctx, void* buffer, uint32_t* stats)
{
    if (!ctx || !buffer) { set_error("ur_debug_print_reset: null argument"); return UR_EINVAL; }
    return ur::launch_debug_print_reset(ctx, buffer, stats);
}

int ur_debug_print_stats(ur_ctx* ctx, const uint32_t* stats, void* buffer)
{
    if (!ctx || !stats || !buffer) { set_error("ur_debug_print_stats: null argument"); return UR_EINVAL; }
    return ur::launch_debug_print_stats(ctx, stats, buffer);
}

int ur_debug_print_text(ur_ctx* ctx, void* buffer, uint32_t x, uint32_t y, uint32_t color, const char* text, uint32_t length)
{
    if (!ctx || !buffer || (!text && length != 0)) { set_error("ur_debug_print_text: null argument"); return UR_EINVAL; }
    return ur::launch_debug_print_text(ctx, buffer, x, y, color, text, length);
}

int ur_debug_print_draw(ur_ctx* ctx, const ur_debug_print_constants* constants, const ur_debug_glyph* glyphs, uint32_t glyph_count,
                        const uint8_t* atlas_r8, uint32_t atlas_w, uint32_t atlas_h, const void* buffer, uint32_t* ldr_inout, uint32_t w,
                        uint32_t h, uint32_t row0, uint32_t rows)
{
    const int rc = ur::check_band("ur_debug_print_draw", ctx, w, h, row0, rows);
    if (rc != UR_OK) return rc;
    if (!constants || !glyphs || !atlas_r8 || !buffer || !ldr_inout) { set_error("ur_debug_print_draw: null argument"); return UR_EINVAL; }
    if (glyph_count == 0 || atlas_w == 0 || atlas_h == 0 || atlas_w > 16384u || atlas_h > 16384u) {
        set_error("ur_debug_print_draw: glyph table of %u entries, atlas %u x %u (1..16384)", glyph_count, atlas_w, atlas_h);
        return UR_EINVAL;
    }
    if (constants->ScreenSize[0] != (float)w || constants->ScreenSize[1] != (float)h) {
        set_error("ur_debug_print_draw: ScreenSize (%g, %g) is not the frame's (%u, %u)", constants->ScreenSize[0], constants->ScreenSize[1], w, h);
        return UR_EINVAL;
    }
    return ur::launch_debug_print_draw(ctx, constants, glyphs, glyph_count, atlas_r8, atlas_w, atlas_h, buffer, ldr_inout, w, row0, rows);
}

} // extern "C"
