// The raster of ShadowMap, DepthPrepass and GBuffer for gfx950 — what turns draws of indexed triangle lists (include/ur_raster.h) into
// depth or visibility keys: one set of kernels, a policy per pass, their launches, the checks of an ur_raster_draws (ur_internal.h) and
// ur_shadow_map / ur_depth_prepass / ur_raster_reserve. ShadowMap first; what the other passes change is at the policies below.
//
// Reference: the "ShadowMap" pass (DeferredRenderer.cpp:551-633), Shaders/ShadowMap.hlsl (position * World * LightViewProjection, no
// pixel shader), its pipeline (Renderer.cpp:240-300: CULL_MODE_FRONT, FrontCounterClockwise, LESS_EQUAL, zero bias, depth clip) and
// target (D32_FLOAT, cleared to 1.0). The result is a per-texel minimum, so it is specified to the bit: DESIGN.md section 3.7 is the
// rule, tests/shadow_ref.py restates it in numpy, and this file computes the same bytes. Built with -ffp-contract=off.
//
// Three launches, nothing read back:
//   clear   every texel = 1.0f (16-byte nontemporal stores), the large queue's count = 0;
//   raster  a wave per (draw candidate, segment): it walks the 64-triangle chunks c = segment, segment + S, ... of its command, a lane
//           per triangle (rules 1-3 and the bounding box), then serves the survivors: a triangle of at most 4 centres by its own lane,
//           the others by the whole wave as an 8 x 8 pixel stamp, the triangle broadcast by readlane. Triangles of more than 64 stamps
//           go to the queue, one (triangle, 64 x 64 tile) entry per tile under the bounding box, one atomic reservation per triangle;
//           without room the wave rasterises the triangle itself (stats[3]);
//   large   a fixed grid whose waves stride over the entries: a tile the triangle cannot touch is rejected at its corners, the rest
//           is stamped.
// A fragment is one device-scope atomic unsigned minimum of the depth's bit pattern (depths lie in [0, 1]); a plain load in front
// skips it when the texel is already nearer (texels only decrease, so a stale value only costs an atomic, never a fragment).
//
// DepthPrepass (DeferredRenderer.cpp:635-718, pipeline :1894-1961, Shaders/DeferredBasePass.hlsl:58-70): position * World * View *
// Projection under a perspective camera, reverse-Z (GREATER_EQUAL, cleared to 0.0: a per-texel maximum, the atomic mirrored),
// CULL_MODE_BACK, and a D24 target. DESIGN.md section 3.8 is its rule and tests/depth_ref.py the restatement. A lane clips its triangle
// against the near plane with selects on registers (no per-lane arrays): up to four vertices S0..S3 in target space, emitted triangle
// e = (S0, S[1 + e], S[2 + e]). The wave serves emitted triangle 0 of every lane, then, when a ballot finds a lane that was cut into
// two, runs the same code once more over emitted triangle 1.
//
// GBuffer's alpha-masked draws (restated in tests/gbuffer_mask_ref.py) are a third keyed policy: a fragment that
// passes the depth test competes for a 64-bit word per texel, (depth bits << 32) | key, and runs the base pass' alpha test (alpha_discards
// below, with the resolves' front end: visibility_key.h, gbuffer_interp.h, texture_sample.h) only when its word is above the texel's; a
// merge launch then folds the words into the opaque draws' key image and raises the depth where a masked fragment won.
//
// The ObjectId pick (restated in tests/object_id_ref.py) is the keyed raster at up to 64 given texels: pick_kernel
// runs raster_kernel's front half and tests the points against each surviving triangle instead of serving its fragments; a word per point
// takes (key << 32) | depth bits, and a one-wave finish turns the words into records.

#include "raster_rule.h"
#include "ur_internal.h"
#include "visibility_key.h"

namespace {

using namespace ur_raster;

typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr uint32_t kQueueHeaderDwords = 16u; // the count on a line of its own
constexpr uint32_t kEntryDwords = 12u;       // x0 y0 x1 y1 | x2 y2 z0 k1 | k2 tile box_min box_max
constexpr uint32_t kKeyedEntryDwords = 16u;  // GBuffer: | key - - - behind them; the queue is allocated for entries of this size
constexpr uint32_t kLargeStamps = 64u;       // a bounding box of more 8 x 8 stamps than this is a large triangle
constexpr uint32_t kOwnPixels = 4u;          // a bounding box of at most this many centres is rasterised by the triangle's own lane
constexpr uint32_t kNoTile = 0xFFFFFFFFu;

struct RasterParams {
    const uint8_t* commands;
    uint32_t command_count;
    uint32_t mode; // 0 every slot, 1 list, 2 ranges
    const uint32_t* visible_idx;
    const uint32_t* visible_count;
    uint32_t index_base;
    uint32_t range_count;
    const uint32_t* offsets;
    const uint32_t* counts;
    float L[16];  // ShadowMap: LightViewProjection; DepthPrepass: View
    float Pr[16]; // DepthPrepass: Projection
    uint32_t* map;
    uint32_t w, h;
    float half_w, half_h; // 0.5f * w, 0.5f * h
    uint32_t* stats;
    uint32_t* queue; // 64-bit count at [0..1], entries from kQueueHeaderDwords; null without room
    uint32_t queue_cap;
    uint32_t segments, items; // items = candidates * segments
    // GBuffer: `map` is the key image of the band [row0, row0 + rows); depth is the whole target, read only
    const float* depth;
    uint32_t row0, rows, key_bits;
};

// What the masked policy's kernels take behind a RasterParams: `map` is then the band's 64-bit words
struct MaskArgs {
    const ur_material* materials; // null: no slot has a material (nothing is discarded)
    uint32_t material_count;
    const float* lod; // 127 thresholds of the level of detail
};
struct MaskedParams : RasterParams {
    MaskArgs mask;
};

// What the pick kernels take behind a RasterParams: `map`, the band and the queue are not used. The points ride in the
// kernel arguments, 256 bytes for the most there can be
struct PickParams : RasterParams {
    uint32_t point_count;
    uint32_t points[UR_PICK_MAX_POINTS]; // x | y << 16, clamped to the target
    unsigned long long* results;         // 16-byte records: the first 8 bytes of record i take (key << 32) | depth bits
};

// What a fragment's alpha test reads: nothing in the passes without one
struct NoAlpha {};
struct AlphaCtx {
    const MaskedParams* p;
    const float* lds; // the sampler's tables (texture_sample.h): code / 255 and the level thresholds; the decode part is not filled
};
template <class P>
__device__ __forceinline__ bool alpha_discards(const AlphaCtx& a, uint32_t key, int px, int py);

struct Tri {
    int x0, y0, x1, y1, x2, y2; // 24.8 target space, y down
    float z0, k1, k2;
};

// Rules 4-6 for one pixel
template <class P>
__device__ __forceinline__ void shade(const Tri& t, int b01, int b12, int b20, uint32_t* __restrict__ map, uint32_t w, int px, int py,
                                      const float* __restrict__ depth, uint32_t row0, uint32_t key, const typename P::Alpha& alpha)
{
    const int sx = 256 * px + 128, sy = 256 * py + 128;
    const long long e01 = (long long)(t.x1 - t.x0) * (sy - t.y0) - (long long)(t.y1 - t.y0) * (sx - t.x0);
    const long long e12 = (long long)(t.x2 - t.x1) * (sy - t.y1) - (long long)(t.y2 - t.y1) * (sx - t.x1);
    const long long e20 = (long long)(t.x0 - t.x2) * (sy - t.y2) - (long long)(t.y0 - t.y2) * (sx - t.x2);
    if (((e01 - b01) | (e12 - b12) | (e20 - b20)) < 0) return;
    float z = t.z0 + ((float)e20 * t.k1 + (float)e01 * t.k2);
    if constexpr (P::kKeyed) {
        if (!(z >= 0.0f)) return; // the value ur_depth_prepass stores ...
        if (z > 1.0f) z = 1.0f;
        if constexpr (P::kD24) z = (float)(__builtin_rint((double)z * 16777215.0) / 16777215.0);
        if (!(z >= depth[(size_t)py * w + (uint32_t)px])) return; // ... under GREATER_EQUAL against the prepass' maximum
        if constexpr (P::kMasked) {
            // section 3.11: the word's order is (depth, key); the alpha test runs only for a fragment that would raise the texel
            unsigned long long* k64 = reinterpret_cast<unsigned long long*>(map) + (size_t)((uint32_t)py - row0) * w + (uint32_t)px;
            const unsigned long long word = ((unsigned long long)(__float_as_uint(z) & 0x7FFFFFFFu) << 32) | key; // z += 0.0f
            if (word <= __hip_atomic_load(k64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return; // (words only increase)
            if (alpha_discards<P>(alpha, key, px, py)) return;
            (void)__hip_atomic_fetch_max(k64, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        uint32_t* k = map + (size_t)((uint32_t)py - row0) * w + (uint32_t)px;
        if (key <= __hip_atomic_load(k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return; // (keys only increase)
        (void)__hip_atomic_fetch_max(k, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    uint32_t* p = map + (size_t)py * w + (uint32_t)px;
    if constexpr (P::kNearest) {
        if (!(z >= 0.0f && z <= 1.0f)) return; // depth clip (a NaN goes too)
        uint32_t bits = __float_as_uint(z);
        if (bits == 0x80000000u) bits = 0u; // z += 0.0f
        if (bits >= __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return;
        (void)__hip_atomic_fetch_min(p, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        if (!(z >= 0.0f)) return; // (a NaN goes too)
        if (z > 1.0f) z = 1.0f;   // the geometry lies inside z <= w: only rounding goes above
        if constexpr (P::kD24) z = (float)(__builtin_rint((double)z * 16777215.0) / 16777215.0);
        const uint32_t bits = __float_as_uint(z) & 0x7FFFFFFFu; // z += 0.0f
        if (bits <= __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return; // (texels only increase)
        (void)__hip_atomic_fetch_max(p, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The whole wave stamps the pixels [px0, px1] x [py0, py1] (inside the target) of one triangle, uniform arguments
template <class P>
__device__ __forceinline__ void stamp_rect(const Tri& t, uint32_t* __restrict__ map, uint32_t w, int px0, int py0, int px1, int py1, uint32_t lane,
                                           const float* __restrict__ depth, uint32_t row0, uint32_t key, const typename P::Alpha& alpha)
{
    const int b01 = edge_bias(t.x0, t.y0, t.x1, t.y1), b12 = edge_bias(t.x1, t.y1, t.x2, t.y2), b20 = edge_bias(t.x2, t.y2, t.x0, t.y0);
    const int lx = (int)(lane & 7u), ly = (int)(lane >> 3);
    for (int sy = py0 & ~7; sy <= py1; sy += 8) {
        const int py = sy + ly;
        for (int sx = px0 & ~7; sx <= px1; sx += 8) {
            const int px = sx + lx;
            if (px >= px0 && px <= px1 && py >= py0 && py <= py1) shade<P>(t, b01, b12, b20, map, w, px, py, depth, row0, key, alpha);
        }
    }
}

__device__ __forceinline__ int rl(int v, uint32_t s) { return __builtin_amdgcn_readlane(v, (int)s); }
__device__ __forceinline__ float rlf(float v, uint32_t s) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int)s)); }

__device__ __forceinline__ Tri broadcast(const Tri& t, uint32_t s)
{
    Tri r;
    r.x0 = rl(t.x0, s); r.y0 = rl(t.y0, s); r.x1 = rl(t.x1, s); r.y1 = rl(t.y1, s); r.x2 = rl(t.x2, s); r.y2 = rl(t.y2, s);
    r.z0 = rlf(t.z0, s); r.k1 = rlf(t.k1, s); r.k2 = rlf(t.k2, s);
    return r;
}

// ---- the policies: what a pass does with a vertex and a triangle -------------------------------------------------------------------
// project():  rule 1 for one vertex.
// assemble(): from the three clip-space vertices to the target-space vertices S0..S3 (rule 2; DepthPrepass: the near clip in front of it);
//             returns how many triangles (S0, S[1 + e], S[2 + e]) the lane emits.

// ShadowMap: orthographic, drawn iff A > 0, a per-texel minimum over a map cleared to 1.0
struct ShadowPolicy {
    using Params = RasterParams;
    using Alpha = NoAlpha;
    static constexpr bool kNearest = true, kSwap12 = false, kKeyed = false, kMasked = false;
    static constexpr uint32_t kEmit = 1u, kVertexBytes = 12u, kEntryDwords = ::kEntryDwords;
    static constexpr float kGuardBand = (float)UR_RASTER_MAX_TARGET;

    // position * World * LightViewProjection, each a left-to-right sum of four products
    static __device__ __forceinline__ void project(const float* __restrict__ pos, const float (&W)[16], const RasterParams& p, float (&clip)[4])
    {
        const float x = pos[0], y = pos[1], z = pos[2];
        float wv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) wv[k] = ((x * W[k] + y * W[4 + k]) + z * W[8 + k]) + W[12 + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) clip[k] = ((wv[0] * p.L[k] + wv[1] * p.L[4 + k]) + wv[2] * p.L[8 + k]) + wv[3] * p.L[12 + k];
    }

    static __device__ __forceinline__ uint32_t assemble(const float (&c)[3][4], const RasterParams& p, float (&SX)[4], float (&SY)[4], float (&SZ)[4],
                                                        bool& unsupported, bool& cut, bool& behind)
    {
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            if (c[v][3] != 1.0f) unsupported = true;
            SX[v] = (c[v][0] + 1.0f) * p.half_w; // rule 2
            SY[v] = (1.0f - c[v][1]) * p.half_h;
            SZ[v] = c[v][2];
        }
        return unsupported ? 0u : 1u;
    }
};

// DepthPrepass: perspective with a near clip, drawn iff A < 0 (every emitted triangle is taken as (u0, u2, u1), then
// drawn iff A > 0 as above), a per-texel maximum over a target cleared to 0.0, optionally quantised to D24
template <bool D24>
struct DepthPolicy {
    using Params = RasterParams;
    using Alpha = NoAlpha;
    static constexpr bool kNearest = false, kD24 = D24, kSwap12 = true, kKeyed = false, kMasked = false;
    static constexpr uint32_t kEmit = 2u, kVertexBytes = 12u, kEntryDwords = ::kEntryDwords;
    static constexpr float kGuardBand = kDepthGuardBand;

    // position * World * View * Projection, in the order the vertex shader multiplies
    static __device__ __forceinline__ void project(const float* __restrict__ pos, const float (&W)[16], const RasterParams& p, float (&clip)[4])
    {
        const float x = pos[0], y = pos[1], z = pos[2];
        float wv[4], vv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) wv[k] = ((x * W[k] + y * W[4 + k]) + z * W[8 + k]) + W[12 + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) vv[k] = ((wv[0] * p.L[k] + wv[1] * p.L[4 + k]) + wv[2] * p.L[8 + k]) + wv[3] * p.L[12 + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) clip[k] = ((vv[0] * p.Pr[k] + vv[1] * p.Pr[4 + k]) + vv[2] * p.Pr[8 + k]) + vv[3] * p.Pr[12 + k];
    }

    static __device__ __forceinline__ uint32_t assemble(const float (&c)[3][4], const RasterParams& p, float (&SX)[4], float (&SY)[4], float (&SZ)[4],
                                                        bool& unsupported, bool& cut, bool& behind)
    {
        bool ok = true;
#pragma unroll
        for (int v = 0; v < 3; ++v) {
#pragma unroll
            for (int k = 0; k < 4; ++k) ok = ok && fabsf(c[v][k]) <= kFloatMax; // (false for NaN)
            ok = ok && c[v][2] > 0.0f;
        }
        if (!ok) { unsupported = true; return 0u; }
        // the near plane: inside iff d = w - z >= 0
        const float d0 = c[0][3] - c[0][2], d1 = c[1][3] - c[1][2], d2 = c[2][3] - c[2][2];
        const bool o0 = d0 < 0.0f, o1 = d1 < 0.0f, o2 = d2 < 0.0f;
        const uint32_t n_out = (o0 ? 1u : 0u) + (o1 ? 1u : 0u) + (o2 ? 1u : 0u);
        if (n_out == 3u) { behind = true; return 0u; }
        cut = n_out != 0u;
        // (a, b, c) = the triangle rotated (its winding kept) so that c is the one vertex outside, or a the one vertex inside
        const uint32_t rot = n_out == 1u ? (o0 ? 1u : (o1 ? 2u : 0u)) : (n_out == 2u ? (!o0 ? 0u : (!o1 ? 1u : 2u)) : 0u);
        const float ax = sel3(rot, c[0][0], c[1][0], c[2][0]), ay = sel3(rot, c[0][1], c[1][1], c[2][1]), az = sel3(rot, c[0][2], c[1][2], c[2][2]);
        const float aw = sel3(rot, c[0][3], c[1][3], c[2][3]), ad = sel3(rot, d0, d1, d2);
        const float bx = sel3(rot, c[1][0], c[2][0], c[0][0]), by = sel3(rot, c[1][1], c[2][1], c[0][1]), bz = sel3(rot, c[1][2], c[2][2], c[0][2]);
        const float bw = sel3(rot, c[1][3], c[2][3], c[0][3]), bd = sel3(rot, d1, d2, d0);
        const float cx = sel3(rot, c[2][0], c[0][0], c[1][0]), cy = sel3(rot, c[2][1], c[0][1], c[1][1]), cz = sel3(rot, c[2][2], c[0][2], c[1][2]);
        const float cw = sel3(rot, c[2][3], c[0][3], c[1][3]), cd = sel3(rot, d2, d0, d1);
        // new vertices, always from the inside vertex towards the outside one: p on b -> c (one out) or a -> b (two out), q on a -> c
        const bool one = n_out == 1u;
        const float ix = one ? bx : ax, iy = one ? by : ay, iw = one ? bw : aw, id = one ? bd : ad;
        const float ox = one ? cx : bx, oy = one ? cy : by, ow = one ? cw : bw, od = one ? cd : bd;
        const float tp = id / (id - od), tq = ad / (ad - cd);
        const float px = ix + tp * (ox - ix), py = iy + tp * (oy - iy), pw = iw + tp * (ow - iw);
        const float qx = ax + tq * (cx - ax), qy = ay + tq * (cy - ay), qw = aw + tq * (cw - aw);
        // the polygon: (a, b, c) whole, (a, b, p, q) with one vertex out - diagonal a-p -, (a, p, q) with two; a new vertex has z := w
        const bool two = n_out == 2u, whole = n_out == 0u;
        float vx[4], vy[4], vz[4], vw[4];
        vx[0] = ax; vy[0] = ay; vz[0] = az; vw[0] = aw;
        vx[1] = two ? px : bx; vy[1] = two ? py : by; vz[1] = two ? pw : bz; vw[1] = two ? pw : bw;
        vx[2] = whole ? cx : (one ? px : qx); vy[2] = whole ? cy : (one ? py : qy); vz[2] = whole ? cz : (one ? pw : qw); vw[2] = whole ? cw : (one ? pw : qw);
        vx[3] = qx; vy[3] = qy; vz[3] = qw; vw[3] = qw;
#pragma unroll
        for (int k = 0; k < 4; ++k) { // rule 2 (S3 is read only when two triangles are emitted)
            SX[k] = (vx[k] / vw[k] + 1.0f) * p.half_w;
            SY[k] = (1.0f - vy[k] / vw[k]) * p.half_h;
            SZ[k] = vz[k] / vw[k];
        }
        return one ? 2u : 1u;
    }
};

// GBuffer's raster: DepthPrepass' vertex, near clip, facing, coverage and depth plane; a fragment whose depth passes
// GREATER_EQUAL against the prepass' result raises the texel of the key image to the triangle's key ((ordinal + 1) << T) | t. The key
// rides with the triangle: the lane's own in the own-lane path, a readlane in the stamp paths, a dword of the queue's record.
template <bool D24>
struct VisPolicy : DepthPolicy<D24> {
    static constexpr bool kKeyed = true;
    static constexpr uint32_t kVertexBytes = 64u, kEntryDwords = kKeyedEntryDwords;
};

// GBuffer's alpha-masked draws: VisPolicy's fragment in front of a 64-bit word per texel and the alpha test
template <bool D24>
struct MaskPolicy : VisPolicy<D24> {
    using Params = MaskedParams;
    using Alpha = AlphaCtx;
    static constexpr bool kMasked = true;
};

// Rule 3 of section 3.11 for the fragment of the triangle `key` names at the texel (px, py): the triangle is fetched again from the key as
// the resolve fetches it, COLOR.a and TEXCOORD interpolated with the resolve's weights, channel A of the base-colour map sampled with the
// resolve's sampler. True iff alpha < AlphaCutoff (false for a NaN on either side).
template <class P>
__device__ __forceinline__ bool alpha_discards(const AlphaCtx& a, uint32_t key, int px, int py)
{
    const MaskedParams& p = *a.p;
    uint32_t t;
    const uint32_t slot = key_slot<false>(p, key, 0u, t); // (the masked draws' own selection: no detour)
    uint32_t bits = 0u;
    if (p.mask.materials != nullptr && slot < p.mask.material_count) bits = reinterpret_cast<const uint32_t*>(p.mask.materials + slot)[16];
    if ((bits & UR_MATERIAL_ALPHA_MASK) == 0u) return false;
    const KeyDraw d = key_draw(p.commands, slot, t);
    const float* cb = d.cb;
    const float (&W)[16] = d.W;
    float c[3][4], uv[3][2], va[3]; // clip position, TEXCOORD, COLOR.a
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const uint64_t vi = (uint64_t)(d.base_vertex + (long long)d.indices[d.first + (uint32_t)v]);
        const float* vp = reinterpret_cast<const float*>(d.vertices + vi * d.stride);
        P::project(vp, W, p, c[v]);
        uv[v][0] = vp[6]; uv[v][1] = vp[7];
        va[v] = vp[15];
    }
    float SX[4], SY[4], vw[4], B[4][3];
    bool one;
    clip_polygon(c, p.half_w, p.half_h, SX, SY, vw, B, one);
    Piece pc;
    covering_piece(SX, SY, vw, one, 256 * px + 128, 256 * py + 128, pc);
    float b[3];
    piece_weights(pc, pc.l0, pc.l1, pc.l2, B, b);
    float alpha = cb[106] * ((b[0] * va[0] + b[1] * va[1]) + b[2] * va[2]); // BaseColorAlpha * COLOR.a
    if (bits & UR_MATERIAL_BASE_COLOR_MAP) {
        const u32x4_t desc = reinterpret_cast<const u32x4_t*>(p.mask.materials + slot)[0];
        if (valid_texture(desc)) {
            const bool odd_column = ((uint32_t)px & 1u) != 0u, odd_row = ((uint32_t)py & 1u) != 0u;
            float pu[3], pv[3], tu[3], tv[3];
            quad_texcoords(pc, B, uv, odd_column, odd_row, pu, pv);
#pragma unroll
            for (int point = 0; point < 3; ++point) texture_transform(cb, 112u, pu[point], pv[point], tu[point], tv[point]);
            float dxu, dxv, dyu, dyv, sa[1];
            quad_differences(tu, tv, odd_column, odd_row, dxu, dxv, dyu, dyv);
            sample_map<3, 1>(desc, tu[0], tv[0], dxu, dxv, dyu, dyv, a.lds, sa);
            alpha = alpha * sa[0];
        }
    }
    return alpha < cb[107]; // AlphaCutoff
}

__global__ __launch_bounds__(kThreads) void shadow_clear_kernel(float* __restrict__ map, uint32_t n, uint32_t head, uint32_t* __restrict__ queue, float value)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i == 0u && queue != nullptr) queue[0] = queue[1] = 0u; // (a 64-bit count: it never wraps)
    // `head` floats up to the first 16-byte boundary, then whole 16-byte groups, then what is left
    const uint32_t groups = (n - head) / 4u, tail = head + groups * 4u;
    if (i < head) map[i] = value;
    if (i < n - tail) map[tail + i] = value;
    f32x4_t* body = reinterpret_cast<f32x4_t*>(map + head);
    const f32x4_t fill = {value, value, value, value};
    for (uint32_t g = i; g < groups; g += gridDim.x * kThreads) __builtin_nontemporal_store(fill, body + g);
}

template <class P>
__global__ __launch_bounds__(kThreads) void raster_kernel(typename P::Params p)
{
    typename P::Alpha alpha{};
    if constexpr (P::kMasked) {
        __shared__ float sampler_tables[kLdsFloats];
        fill_sampler_tables<false>(sampler_tables, nullptr, p.mask.lod);
        __syncthreads();
        alpha.p = &p; alpha.lds = sampler_tables;
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
    const uint32_t wave_count = gridDim.x * kWaves;
    uint32_t n_drawn = 0, n_unsupported = 0, n_dropped = 0, n_unqueued = 0, n_cut = 0, n_behind = 0; // uniform; added to stats once per wave

    for (uint32_t item = wave; item < p.items; item += wave_count) {
        const uint32_t cand = item / p.segments, seg = item - cand * p.segments;
        // ---- selection: the candidate's slot, or none
        uint32_t slot = cand;
        if (p.mode == 1u) {
            if (cand >= *p.visible_count) continue;
            slot = p.visible_idx[cand] - p.index_base;
        } else if (p.mode == 2u) {
            uint32_t lo = 0u, hi = p.range_count + 1u; // first k with offsets[k] > cand
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (p.offsets[mid] > cand) hi = mid; else lo = mid + 1u;
            }
            if (lo == 0u || lo > p.range_count) continue;
            const uint32_t r = lo - 1u;
            if (cand - p.offsets[r] >= p.counts[r]) continue;
        }
        slot = __builtin_amdgcn_readfirstlane(slot);
        if (slot >= p.command_count) continue;
        // ---- the command (uniform)
        const u32x4_t* cmd = reinterpret_cast<const u32x4_t*>(p.commands + (size_t)slot * UR_INDIRECT_COMMAND_STRIDE);
        const u32x4_t c0 = cmd[0], c1 = cmd[1], c2 = cmd[2], c3 = cmd[3];
        if (c2.w == 0u) continue; // InstanceCount
        const uint64_t vb = (uint64_t)c0.x | ((uint64_t)c0.y << 32), ib = (uint64_t)c1.x | ((uint64_t)c1.y << 32), cb = (uint64_t)c2.x | ((uint64_t)c2.y << 32);
        const uint32_t vb_size = c0.z, stride = c0.w, ib_size = c1.z, format = c1.w;
        const uint32_t tri_count = c2.z / 3u, start_index = c3.x;
        const long long base_vertex = (int)c3.y;
        bool too_many = false;
        if constexpr (P::kKeyed) too_many = tri_count > (1u << p.key_bits);
        if (too_many || format != UR_RASTER_INDEX_FORMAT_R32_UINT || stride < P::kVertexBytes || (stride & 3u) != 0u || vb == 0u || (vb & 3u) != 0u || ib == 0u || (ib & 3u) != 0u ||
            cb == 0u || (cb & 3u) != 0u) {
            if (seg == 0u) n_unsupported += tri_count;
            continue;
        }
        const uint32_t chunks = (tri_count + 63u) / 64u;
        if (seg >= chunks) continue;
        float W[16];
        {
            const float* wp = reinterpret_cast<const float*>(cb);
#pragma unroll
            for (int k = 0; k < 16; ++k) W[k] = wp[k];
        }
        const uint32_t* indices = reinterpret_cast<const uint32_t*>(ib);
        const uint8_t* vertices = reinterpret_cast<const uint8_t*>(vb);
        const uint64_t index_slots = ib_size / 4u;

        for (uint32_t chunk = seg; chunk < chunks; chunk += p.segments) {
            const uint32_t t = chunk * 64u + lane;
            const uint32_t key = P::kKeyed ? (((cand + 1u) << p.key_bits) | t) : 0u; // (cand is the ordinal under every selection)
            // ---- a lane per triangle: rules 1-2 (and the near clip), up to four target-space vertices
            float SX[4] = {}, SY[4] = {}, SZ[4] = {};
            uint32_t emit = 0u;
            bool unsupported = false, cut = false, behind = false;
            if (t < tri_count) {
                const uint64_t first = (uint64_t)start_index + 3ull * t;
                float clip[3][4] = {};
                if (first + 2u >= index_slots) unsupported = true;
                if (!unsupported) {
#pragma unroll
                    for (int v = 0; v < 3; ++v) {
                        const long long vi = base_vertex + (long long)indices[first + (uint32_t)v];
                        if (vi < 0 || (uint64_t)vi * stride + P::kVertexBytes > (uint64_t)vb_size) { unsupported = true; continue; }
                        P::project(reinterpret_cast<const float*>(vertices + (uint64_t)vi * stride), W, p, clip[v]);
                    }
                }
                if (!unsupported) emit = P::assemble(clip, p, SX, SY, SZ, unsupported, cut, behind);
            }
            n_unsupported += (uint32_t)__popcll(__ballot(unsupported));
            uint32_t passes = 1u;
            if constexpr (P::kEmit > 1u) {
                n_cut += (uint32_t)__popcll(__ballot(cut));
                n_behind += (uint32_t)__popcll(__ballot(behind));
                if (__ballot(emit > 1u) != 0ull) passes = 2u;
            }

            for (uint32_t e = 0u; e < passes; ++e) {
                // ---- emitted triangle e of the lane: the guard band, rule 3 and the bounding box
                Tri tri = {};
                int bx0 = 0, by0 = 0, bx1 = -1, by1 = -1;
                uint32_t kind = 0u; // 0 nothing to draw, 1 own lane, 2 wave, 3 large
                bool dropped = false;
                if (e < emit) {
                    float X[3], Y[3], Z[3];
                    const bool second = P::kEmit > 1u && e != 0u;
                    const int i1 = P::kSwap12 ? 2 : 1, i2 = P::kSwap12 ? 1 : 2; // (DepthPrepass: (u0, u2, u1))
                    X[0] = SX[0]; Y[0] = SY[0]; Z[0] = SZ[0];
                    X[i1] = second ? SX[2] : SX[1]; Y[i1] = second ? SY[2] : SY[1]; Z[i1] = second ? SZ[2] : SZ[1];
                    X[i2] = second ? SX[3] : SX[2]; Y[i2] = second ? SY[3] : SY[2]; Z[i2] = second ? SZ[3] : SZ[2];
#pragma unroll
                    for (int v = 0; v < 3; ++v) {
                        const bool finite = fabsf(X[v]) <= kFloatMax && fabsf(Y[v]) <= kFloatMax && fabsf(Z[v]) <= kFloatMax; // (false for NaN)
                        if (!finite || fabsf(X[v]) > P::kGuardBand || fabsf(Y[v]) > P::kGuardBand) dropped = true;
                    }
                    if (!dropped) {
                        tri.x0 = (int)rintf(X[0] * 256.0f); tri.y0 = (int)rintf(Y[0] * 256.0f);
                        tri.x1 = (int)rintf(X[1] * 256.0f); tri.y1 = (int)rintf(Y[1] * 256.0f);
                        tri.x2 = (int)rintf(X[2] * 256.0f); tri.y2 = (int)rintf(Y[2] * 256.0f);
                        const long long A = (long long)(tri.x1 - tri.x0) * (tri.y2 - tri.y0) - (long long)(tri.x2 - tri.x0) * (tri.y1 - tri.y0); // rule 3
                        if (A > 0) {
                            kind = 1u;
                            const float inv = 1.0f / (float)A; // rule 5
                            tri.z0 = Z[0];
                            tri.k1 = (Z[1] - Z[0]) * inv;
                            tri.k2 = (Z[2] - Z[0]) * inv;
                            // centres 256 p + 128 inside [min, max], clamped to the target
                            const int minx = min(tri.x0, min(tri.x1, tri.x2)), maxx = max(tri.x0, max(tri.x1, tri.x2));
                            const int miny = min(tri.y0, min(tri.y1, tri.y2)), maxy = max(tri.y0, max(tri.y1, tri.y2));
                            bx0 = max((minx + 127) >> 8, 0); bx1 = min((maxx - 128) >> 8, (int)p.w - 1);
                            by0 = max((miny + 127) >> 8, 0); by1 = min((maxy - 128) >> 8, (int)p.h - 1);
                            if constexpr (P::kKeyed) { by0 = max(by0, (int)p.row0); by1 = min(by1, (int)(p.row0 + p.rows) - 1); } // the band scissor
                        }
                    }
                }
                const uint32_t drawn = kind;
                if (kind != 0u) {
                    if (bx0 > bx1 || by0 > by1) kind = 0u; // no centre under the box
                    else {
                        const uint32_t pixels = (uint32_t)(bx1 - bx0 + 1) * (uint32_t)(by1 - by0 + 1);
                        const uint32_t stamps = (uint32_t)((bx1 >> 3) - (bx0 >> 3) + 1) * (uint32_t)((by1 >> 3) - (by0 >> 3) + 1);
                        kind = pixels <= kOwnPixels ? 1u : (stamps <= kLargeStamps ? 2u : 3u);
                    }
                }
                n_drawn += (uint32_t)__popcll(__ballot(drawn != 0u));
                n_dropped += (uint32_t)__popcll(__ballot(dropped));

                // ---- the smallest by their own lanes
                if (kind == 1u) {
                    const int b01 = edge_bias(tri.x0, tri.y0, tri.x1, tri.y1), b12 = edge_bias(tri.x1, tri.y1, tri.x2, tri.y2), b20 = edge_bias(tri.x2, tri.y2, tri.x0, tri.y0);
                    for (int py = by0; py <= by1; ++py)
                        for (int px = bx0; px <= bx1; ++px) shade<P>(tri, b01, b12, b20, p.map, p.w, px, py, p.depth, p.row0, key, alpha);
                }
                // ---- the middle ones by the wave
                unsigned long long todo = __ballot(kind == 2u);
                while (todo != 0ull) {
                    const uint32_t s = (uint32_t)__ffsll((long long)todo) - 1u;
                    todo &= todo - 1ull;
                    const Tri u = broadcast(tri, s);
                    stamp_rect<P>(u, p.map, p.w, rl(bx0, s), rl(by0, s), rl(bx1, s), rl(by1, s), lane, p.depth, p.row0, (uint32_t)rl((int)key, s), alpha);
                }
                // ---- the large ones to the queue, or by the wave when there is no room
                todo = __ballot(kind == 3u);
                while (todo != 0ull) {
                    const uint32_t s = (uint32_t)__ffsll((long long)todo) - 1u;
                    todo &= todo - 1ull;
                    const Tri u = broadcast(tri, s);
                    const int x0 = rl(bx0, s), y0 = rl(by0, s), x1 = rl(bx1, s), y1 = rl(by1, s);
                    const uint32_t ukey = (uint32_t)rl((int)key, s);
                    const uint32_t tx0 = (uint32_t)x0 >> 6, ty0 = (uint32_t)y0 >> 6, tnx = ((uint32_t)x1 >> 6) - tx0 + 1u, tny = ((uint32_t)y1 >> 6) - ty0 + 1u;
                    const uint32_t tiles = tnx * tny;
                    bool queued = false;
                    if (p.queue_cap != 0u) {
                        unsigned long long at = 0ull;
                        if (lane == 0u) at = __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(p.queue), (unsigned long long)tiles, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        at = ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(at >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)at);
                        queued = at + tiles <= p.queue_cap;
                        // the slots this reservation took and cannot use are marked empty
                        const uint32_t base = (uint32_t)min(at, (unsigned long long)p.queue_cap), end = (uint32_t)min(at + tiles, (unsigned long long)p.queue_cap);
                        for (uint32_t q_at = base + lane; q_at < end; q_at += 64u) {
                            const uint32_t k = q_at - base, tx = tx0 + k % tnx, ty = ty0 + k / tnx;
                            u32x4_t* q = reinterpret_cast<u32x4_t*>(p.queue + kQueueHeaderDwords + (size_t)q_at * P::kEntryDwords);
                            const u32x4_t q0 = {(uint32_t)u.x0, (uint32_t)u.y0, (uint32_t)u.x1, (uint32_t)u.y1};
                            const u32x4_t q1 = {(uint32_t)u.x2, (uint32_t)u.y2, __float_as_uint(u.z0), __float_as_uint(u.k1)};
                            const u32x4_t q2 = {__float_as_uint(u.k2), queued ? (tx | (ty << 16)) : kNoTile, (uint32_t)x0 | ((uint32_t)y0 << 16), (uint32_t)x1 | ((uint32_t)y1 << 16)};
                            q[0] = q0; q[1] = q1; q[2] = q2;
                            if constexpr (P::kKeyed) q[3] = u32x4_t{ukey, 0u, 0u, 0u};
                        }
                    }
                    if (!queued) {
                        ++n_unqueued;
                        stamp_rect<P>(u, p.map, p.w, x0, y0, x1, y1, lane, p.depth, p.row0, ukey, alpha);
                    }
                }
            }
        }
    }
    if (p.stats != nullptr && lane == 0u) {
        if (n_drawn) (void)__hip_atomic_fetch_add(p.stats + 0, n_drawn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n_unsupported) (void)__hip_atomic_fetch_add(p.stats + 1, n_unsupported, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n_dropped) (void)__hip_atomic_fetch_add(p.stats + 2, n_dropped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n_unqueued) (void)__hip_atomic_fetch_add(p.stats + 3, n_unqueued, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (P::kEmit > 1u) {
            if (n_cut) (void)__hip_atomic_fetch_add(p.stats + 4, n_cut, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (n_behind) (void)__hip_atomic_fetch_add(p.stats + 5, n_behind, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---- the pick: the key raster's answer at up to 64 texels, from the triangles alone ---------------------------------

// Rules 4-5 and the depth test of `shade` for one triangle at one point, whose depth rides in `point_depth`: a passing fragment raises
// the point's word to (key << 32) | depth bits, so the greatest key wins and carries its own depth
template <class P>
__device__ __forceinline__ void pick_fragment(const Tri& t, int b01, int b12, int b20, int px, int py, float point_depth, uint32_t key,
                                              unsigned long long* __restrict__ word_at)
{
    const int sx = 256 * px + 128, sy = 256 * py + 128;
    const long long e01 = (long long)(t.x1 - t.x0) * (sy - t.y0) - (long long)(t.y1 - t.y0) * (sx - t.x0);
    const long long e12 = (long long)(t.x2 - t.x1) * (sy - t.y1) - (long long)(t.y2 - t.y1) * (sx - t.x1);
    const long long e20 = (long long)(t.x0 - t.x2) * (sy - t.y2) - (long long)(t.y0 - t.y2) * (sx - t.x2);
    if (((e01 - b01) | (e12 - b12) | (e20 - b20)) < 0) return;
    float z = t.z0 + ((float)e20 * t.k1 + (float)e01 * t.k2);
    if (!(z >= 0.0f)) return;
    if (z > 1.0f) z = 1.0f;
    if constexpr (P::kD24) z = (float)(__builtin_rint((double)z * 16777215.0) / 16777215.0);
    if (!(z >= point_depth)) return;
    const unsigned long long word = ((unsigned long long)key << 32) | (__float_as_uint(z) & 0x7FFFFFFFu); // z += 0.0f
    if (word <= __hip_atomic_load(word_at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return; // (words only increase)
    (void)__hip_atomic_fetch_max(word_at, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// raster_kernel's work distribution and per-triangle front half (selection, command, rules 1-3, the near clip, the guard band, the
// snap), written out again and not shared as a function, so that raster_kernel's registers stay what they were; behind it a surviving
// lane tests the points against its triangle's box instead of serving fragments. Lane j of every wave holds point j's depth
template <class P>
__global__ __launch_bounds__(kThreads) void pick_kernel(PickParams p)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
    const uint32_t wave_count = gridDim.x * kWaves;
    uint32_t n_drawn = 0, n_unsupported = 0, n_dropped = 0, n_cut = 0, n_behind = 0; // uniform; added to stats once per wave
    float point_depth = 0.0f;
    if (lane < p.point_count) {
        const uint32_t xy = p.points[lane];
        point_depth = p.depth[(size_t)(xy >> 16) * p.w + (xy & 0xFFFFu)];
    }

    for (uint32_t item = wave; item < p.items; item += wave_count) {
        const uint32_t cand = item / p.segments, seg = item - cand * p.segments;
        // ---- selection: the candidate's slot, or none
        uint32_t slot = cand;
        if (p.mode == 1u) {
            if (cand >= *p.visible_count) continue;
            slot = p.visible_idx[cand] - p.index_base;
        } else if (p.mode == 2u) {
            uint32_t lo = 0u, hi = p.range_count + 1u; // first k with offsets[k] > cand
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (p.offsets[mid] > cand) hi = mid; else lo = mid + 1u;
            }
            if (lo == 0u || lo > p.range_count) continue;
            const uint32_t r = lo - 1u;
            if (cand - p.offsets[r] >= p.counts[r]) continue;
        }
        slot = __builtin_amdgcn_readfirstlane(slot);
        if (slot >= p.command_count) continue;
        // ---- the command (uniform)
        const u32x4_t* cmd = reinterpret_cast<const u32x4_t*>(p.commands + (size_t)slot * UR_INDIRECT_COMMAND_STRIDE);
        const u32x4_t c0 = cmd[0], c1 = cmd[1], c2 = cmd[2], c3 = cmd[3];
        if (c2.w == 0u) continue; // InstanceCount
        const uint64_t vb = (uint64_t)c0.x | ((uint64_t)c0.y << 32), ib = (uint64_t)c1.x | ((uint64_t)c1.y << 32), cb = (uint64_t)c2.x | ((uint64_t)c2.y << 32);
        const uint32_t vb_size = c0.z, stride = c0.w, ib_size = c1.z, format = c1.w;
        const uint32_t tri_count = c2.z / 3u, start_index = c3.x;
        const long long base_vertex = (int)c3.y;
        if (tri_count > (1u << p.key_bits) || format != UR_RASTER_INDEX_FORMAT_R32_UINT || stride < P::kVertexBytes || (stride & 3u) != 0u || vb == 0u || (vb & 3u) != 0u ||
            ib == 0u || (ib & 3u) != 0u || cb == 0u || (cb & 3u) != 0u) {
            if (seg == 0u) n_unsupported += tri_count;
            continue;
        }
        const uint32_t chunks = (tri_count + 63u) / 64u;
        if (seg >= chunks) continue;
        float W[16];
        {
            const float* wp = reinterpret_cast<const float*>(cb);
#pragma unroll
            for (int k = 0; k < 16; ++k) W[k] = wp[k];
        }
        const uint32_t* indices = reinterpret_cast<const uint32_t*>(ib);
        const uint8_t* vertices = reinterpret_cast<const uint8_t*>(vb);
        const uint64_t index_slots = ib_size / 4u;

        for (uint32_t chunk = seg; chunk < chunks; chunk += p.segments) {
            const uint32_t t = chunk * 64u + lane;
            const uint32_t key = ((cand + 1u) << p.key_bits) | t;
            // ---- a lane per triangle: rules 1-2 and the near clip, up to four target-space vertices
            float SX[4] = {}, SY[4] = {}, SZ[4] = {};
            uint32_t emit = 0u;
            bool unsupported = false, cut = false, behind = false;
            if (t < tri_count) {
                const uint64_t first = (uint64_t)start_index + 3ull * t;
                float clip[3][4] = {};
                if (first + 2u >= index_slots) unsupported = true;
                if (!unsupported) {
#pragma unroll
                    for (int v = 0; v < 3; ++v) {
                        const long long vi = base_vertex + (long long)indices[first + (uint32_t)v];
                        if (vi < 0 || (uint64_t)vi * stride + P::kVertexBytes > (uint64_t)vb_size) { unsupported = true; continue; }
                        P::project(reinterpret_cast<const float*>(vertices + (uint64_t)vi * stride), W, p, clip[v]);
                    }
                }
                if (!unsupported) emit = P::assemble(clip, p, SX, SY, SZ, unsupported, cut, behind);
            }
            n_unsupported += (uint32_t)__popcll(__ballot(unsupported));
            n_cut += (uint32_t)__popcll(__ballot(cut));
            n_behind += (uint32_t)__popcll(__ballot(behind));
            const uint32_t passes = __ballot(emit > 1u) != 0ull ? 2u : 1u;

            for (uint32_t e = 0u; e < passes; ++e) {
                // ---- emitted triangle e of the lane: the guard band, rule 3 and the box of the centres it can cover
                Tri tri = {};
                int bx0 = 0, by0 = 0, bx1 = -1, by1 = -1;
                bool drawn = false, dropped = false;
                if (e < emit) {
                    float X[3], Y[3], Z[3];
                    const bool second = e != 0u;
                    X[0] = SX[0]; Y[0] = SY[0]; Z[0] = SZ[0]; // (u0, u2, u1)
                    X[2] = second ? SX[2] : SX[1]; Y[2] = second ? SY[2] : SY[1]; Z[2] = second ? SZ[2] : SZ[1];
                    X[1] = second ? SX[3] : SX[2]; Y[1] = second ? SY[3] : SY[2]; Z[1] = second ? SZ[3] : SZ[2];
#pragma unroll
                    for (int v = 0; v < 3; ++v) {
                        const bool finite = fabsf(X[v]) <= kFloatMax && fabsf(Y[v]) <= kFloatMax && fabsf(Z[v]) <= kFloatMax; // (false for NaN)
                        if (!finite || fabsf(X[v]) > P::kGuardBand || fabsf(Y[v]) > P::kGuardBand) dropped = true;
                    }
                    if (!dropped) {
                        tri.x0 = (int)rintf(X[0] * 256.0f); tri.y0 = (int)rintf(Y[0] * 256.0f);
                        tri.x1 = (int)rintf(X[1] * 256.0f); tri.y1 = (int)rintf(Y[1] * 256.0f);
                        tri.x2 = (int)rintf(X[2] * 256.0f); tri.y2 = (int)rintf(Y[2] * 256.0f);
                        const long long A = (long long)(tri.x1 - tri.x0) * (tri.y2 - tri.y0) - (long long)(tri.x2 - tri.x0) * (tri.y1 - tri.y0); // rule 3
                        if (A > 0) {
                            drawn = true;
                            const float inv = 1.0f / (float)A; // rule 5
                            tri.z0 = Z[0];
                            tri.k1 = (Z[1] - Z[0]) * inv;
                            tri.k2 = (Z[2] - Z[0]) * inv;
                            const int minx = min(tri.x0, min(tri.x1, tri.x2)), maxx = max(tri.x0, max(tri.x1, tri.x2));
                            const int miny = min(tri.y0, min(tri.y1, tri.y2)), maxy = max(tri.y0, max(tri.y1, tri.y2));
                            bx0 = (minx + 127) >> 8; bx1 = (maxx - 128) >> 8; // (a point lies inside the target: no clamp)
                            by0 = (miny + 127) >> 8; by1 = (maxy - 128) >> 8;
                        }
                    }
                }
                n_drawn += (uint32_t)__popcll(__ballot(drawn));
                n_dropped += (uint32_t)__popcll(__ballot(dropped));
                if (__ballot(drawn && bx0 <= bx1 && by0 <= by1) == 0ull) continue;
                // ---- the points against the lane's triangle: a uniform loop, the point and its depth in scalar registers
                const int b01 = edge_bias(tri.x0, tri.y0, tri.x1, tri.y1), b12 = edge_bias(tri.x1, tri.y1, tri.x2, tri.y2), b20 = edge_bias(tri.x2, tri.y2, tri.x0, tri.y0);
                for (uint32_t j = 0u; j < p.point_count; ++j) {
                    const uint32_t xy = p.points[j];
                    const int px = (int)(xy & 0xFFFFu), py = (int)(xy >> 16);
                    const float d = rlf(point_depth, j);
                    if (drawn && px >= bx0 && px <= bx1 && py >= by0 && py <= by1) pick_fragment<P>(tri, b01, b12, b20, px, py, d, key, p.results + 2u * j);
                }
            }
        }
    }
    if (p.stats != nullptr && lane == 0u) {
        if (n_drawn) (void)__hip_atomic_fetch_add(p.stats + 0, n_drawn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n_unsupported) (void)__hip_atomic_fetch_add(p.stats + 1, n_unsupported, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n_dropped) (void)__hip_atomic_fetch_add(p.stats + 2, n_dropped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n_cut) (void)__hip_atomic_fetch_add(p.stats + 4, n_cut, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n_behind) (void)__hip_atomic_fetch_add(p.stats + 5, n_behind, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// One wave behind pick_kernel: lane i turns record i's word into {ObjectId, key, slot, depth bits}; a word of 0 is {0, 0, ~0, 0}
__global__ __launch_bounds__(64) void pick_finish_kernel(PickParams p)
{
    const uint32_t i = threadIdx.x;
    if (i >= p.point_count) return;
    const unsigned long long word = p.results[2u * i];
    const uint32_t key = (uint32_t)(word >> 32), zbits = (uint32_t)word;
    u32x4_t record = {0u, 0u, 0xFFFFFFFFu, 0u};
    if (key != 0u) {
        uint32_t t;
        const uint32_t slot = key_slot<false>(p, key, 0u, t);
        const u32x4_t c2 = reinterpret_cast<const u32x4_t*>(p.commands + (size_t)slot * UR_INDIRECT_COMMAND_STRIDE)[2];
        const uint32_t* cb = reinterpret_cast<const uint32_t*>((uint64_t)c2.x | ((uint64_t)c2.y << 32));
        record = u32x4_t{cb[148], key, slot, zbits};
    }
    reinterpret_cast<u32x4_t*>(p.results)[i] = record;
}

// The largest value of the edge function a->b over the centres of the pixels [px0, px1] x [py0, py1]: below zero, no centre passes
__device__ __forceinline__ long long edge_max(int ax, int ay, int bx, int by, int px0, int py0, int px1, int py1)
{
    const int dx = bx - ax, dy = by - ay;
    const int sy = 256 * (dx > 0 ? py1 : py0) + 128, sx = 256 * (dy > 0 ? px0 : px1) + 128;
    return (long long)dx * (sy - ay) - (long long)dy * (sx - ax);
}

template <class P>
__device__ __forceinline__ void large_body(const uint32_t* __restrict__ queue, uint32_t queue_cap, uint32_t* __restrict__ map, uint32_t w,
                                           const float* __restrict__ depth, uint32_t row0, const typename P::Alpha& alpha)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
    const uint32_t wave_count = gridDim.x * kWaves;
    const uint32_t count = (uint32_t)min(*reinterpret_cast<const unsigned long long*>(queue), (unsigned long long)queue_cap);
    for (uint32_t e = wave; e < count; e += wave_count) {
        const u32x4_t* q = reinterpret_cast<const u32x4_t*>(queue + kQueueHeaderDwords + (size_t)e * P::kEntryDwords);
        const u32x4_t q0 = q[0], q1 = q[1], q2 = q[2];
        uint32_t key = 0u;
        if constexpr (P::kKeyed) key = q[3].x;
        if (q2.y == kNoTile) continue;
        Tri t;
        t.x0 = (int)q0.x; t.y0 = (int)q0.y; t.x1 = (int)q0.z; t.y1 = (int)q0.w; t.x2 = (int)q1.x; t.y2 = (int)q1.y;
        t.z0 = __uint_as_float(q1.z); t.k1 = __uint_as_float(q1.w); t.k2 = __uint_as_float(q2.x);
        const int tx = (int)(q2.y & 0xFFFFu) * 64, ty = (int)(q2.y >> 16) * 64;
        const int px0 = max((int)(q2.z & 0xFFFFu), tx), py0 = max((int)(q2.z >> 16), ty);
        const int px1 = min((int)(q2.w & 0xFFFFu), tx + 63), py1 = min((int)(q2.w >> 16), ty + 63);
        if (edge_max(t.x0, t.y0, t.x1, t.y1, px0, py0, px1, py1) < 0 || edge_max(t.x1, t.y1, t.x2, t.y2, px0, py0, px1, py1) < 0 ||
            edge_max(t.x2, t.y2, t.x0, t.y0, px0, py0, px1, py1) < 0)
            continue;
        stamp_rect<P>(t, map, w, px0, py0, px1, py1, lane, depth, row0, key, alpha);
    }
}

template <class P>
__global__ __launch_bounds__(kThreads) void large_kernel(const uint32_t* __restrict__ queue, uint32_t queue_cap, uint32_t* __restrict__ map, uint32_t w,
                                                         const float* __restrict__ depth, uint32_t row0)
{
    large_body<P>(queue, queue_cap, map, w, depth, row0, NoAlpha{});
}

// The masked policy's: what the alpha test reads rides in the parameters, its tables in LDS
template <class P>
__global__ __launch_bounds__(kThreads) void large_masked_kernel(MaskedParams p)
{
    __shared__ float sampler_tables[kLdsFloats];
    fill_sampler_tables<false>(sampler_tables, nullptr, p.mask.lod);
    __syncthreads();
    large_body<P>(p.queue, p.queue_cap, p.map, p.w, p.depth, p.row0, AlphaCtx{&p, sampler_tables});
}

// Rule 5 of section 3.11, a lane per texel of the band: the masked word against the opaque key and the depth; where the masked fragment
// wins, the key image takes its key and the depth its depth, where it loses its word is set to 0 (a word that is left says which selection
// the texel's key belongs to). `depth` points at the band's first row. `won` is added to once per wave.
__global__ __launch_bounds__(kThreads) void mask_merge_kernel(unsigned long long* __restrict__ keys64, uint32_t* __restrict__ keys, uint32_t* __restrict__ depth,
                                                              uint32_t n, uint32_t* __restrict__ won)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    bool wins = false;
    if (i < n) {
        const unsigned long long km = keys64[i];
        const uint32_t hi = (uint32_t)(km >> 32), lo = (uint32_t)km;
        wins = km != 0ull && (hi > depth[i] || lo > keys[i]);
        if (wins) { keys[i] = lo; depth[i] = hi; }
        else if (km != 0ull) keys64[i] = 0ull;
    }
    const uint32_t count = (uint32_t)__popcll(__ballot(wins));
    if (won != nullptr && count != 0u && (threadIdx.x & 63u) == 0u) (void)__hip_atomic_fetch_add(won, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// What GBuffer's raster has beside a depth pass': the depth it tests against, its band and the key's triangle bits
struct VisArgs {
    const float* depth;
    uint32_t row0, rows, key_bits;
};

// What the raster and the pick launch alike: the selection, the matrices, the target's size, the counters, GBuffer's depth, band and key
// bits, and the split of the work into (candidate, segment) items - enough waves to fill the device whatever the command count, since
// index counts live on the device. Returns the blocks of the launch. command_count is not 0.
uint32_t fill_raster_params(RasterParams& p, const ur_ctx* ctx, const float* m0, const float* m1, const ur_raster_draws* draws, uint32_t w, uint32_t h, uint32_t* stats,
                            const VisArgs* vis)
{
    const ur_draw_ranges* rg = draws->ranges;
    p.commands = static_cast<const uint8_t*>(ur::raster_commands(*draws));
    p.command_count = draws->command_count;
    p.mode = draws->visible_idx != nullptr ? 1u : (rg ? 2u : 0u);
    p.visible_idx = draws->visible_idx; p.visible_count = draws->visible_count; p.index_base = draws->index_base;
    if (rg) { p.range_count = rg->range_count; p.offsets = rg->offsets; p.counts = rg->counts; }
    for (int k = 0; k < 16; ++k) { p.L[k] = m0[k]; p.Pr[k] = m1 ? m1[k] : 0.0f; }
    p.w = w; p.h = h;
    p.half_w = 0.5f * (float)w; p.half_h = 0.5f * (float)h;
    p.stats = stats;
    if (vis) { p.depth = vis->depth; p.row0 = vis->row0; p.rows = vis->rows; p.key_bits = vis->key_bits; }
    const uint32_t want_waves = (uint32_t)ctx->cu_count * 16u;
    p.segments = max(1u, min(1024u, want_waves / p.command_count));
    const uint64_t items = (uint64_t)p.command_count * p.segments;
    p.items = (uint32_t)items;
    if (items > 0xFFFFFFFFull) { p.segments = 1u; p.items = p.command_count; }
    return min((p.items + kWaves - 1u) / kWaves, (uint32_t)ctx->cu_count * 32u);
}

// clear, raster, large: the launches every pass shares. `map` holds n = w * (rows of the map) dwords: the whole target of a depth pass
// (vis null), GBuffer's key image of its band. m1 is null for ShadowMap.
template <class P>
int launch_raster(ur_ctx* ctx, const float* m0, const float* m1, const ur_raster_draws* draws, uint32_t* map, uint32_t n, uint32_t w, uint32_t h, float clear,
                  uint32_t* stats, const VisArgs* vis, const MaskArgs* mask = nullptr)
{
    const uint32_t head = min((uint32_t)((16u - (reinterpret_cast<uintptr_t>(map) & 15u)) & 15u) / 4u, n);
    uint32_t* queue = ctx->raster_queue_cap != 0u ? ctx->raster_queue : nullptr;
    const uint32_t clear_blocks = min((n / 4u + kThreads - 1u) / kThreads + 1u, (uint32_t)ctx->cu_count * 16u);
    hipLaunchKernelGGL(shadow_clear_kernel, dim3(clear_blocks), dim3(kThreads), 0, ctx->stream, reinterpret_cast<float*>(map), n, head, queue, clear);
    UR_HIP_TRY(hipGetLastError());
    if (draws->command_count == 0u) return UR_OK;

    typename P::Params p{};
    if constexpr (P::kMasked) p.mask = *mask;
    p.map = map;
    p.queue = queue; p.queue_cap = queue ? ctx->raster_queue_cap : 0u;
    const uint32_t blocks = fill_raster_params(p, ctx, m0, m1, draws, w, h, stats, vis);
    hipLaunchKernelGGL(raster_kernel<P>, dim3(blocks), dim3(kThreads), 0, ctx->stream, p);
    UR_HIP_TRY(hipGetLastError());
    if (queue) {
        if constexpr (P::kMasked) hipLaunchKernelGGL(large_masked_kernel<P>, dim3((uint32_t)ctx->cu_count * 8u), dim3(kThreads), 0, ctx->stream, p);
        else hipLaunchKernelGGL(large_kernel<P>, dim3((uint32_t)ctx->cu_count * 8u), dim3(kThreads), 0, ctx->stream, queue, p.queue_cap, p.map, w, p.depth, p.row0);
        UR_HIP_TRY(hipGetLastError());
    }
    return UR_OK;
}

} // namespace

// ---- what the direct calls and the frame's setters (frame/FrameApi.cpp) share (ur_checks.h); `who` goes into the error text ----
int ur::check_raster_draws(const char* who, const ur_raster_draws& draws, const void* target, const char* target_name, const void* stats)
{
    if (!target) { set_error("%s: null %s", who, target_name); return UR_EINVAL; }
    const bool list = draws.visible_idx != nullptr || draws.visible_count != nullptr;
    if (list && (!draws.visible_idx || !draws.visible_count)) { set_error("%s: a list needs visible_idx and visible_count", who); return UR_EINVAL; }
    if (list && draws.ranges) { set_error("%s: a list and ranges at once", who); return UR_EINVAL; }
    const ur_draw_ranges* rg = draws.ranges;
    if (rg && (!rg->offsets || !rg->commands || !rg->counts || rg->range_count == 0u)) { set_error("%s: a null member of ranges / no range", who); return UR_EINVAL; }
    const void* commands = raster_commands(draws);
    if (!commands && draws.command_count != 0u) { set_error("%s: null commands", who); return UR_EINVAL; }
    if (!aligned(commands, 16) || !aligned(target, 4) || !aligned(stats, 4) || !aligned(draws.visible_idx, 4) || !aligned(draws.visible_count, 4) ||
        (rg && (!aligned(rg->offsets, 4) || !aligned(rg->counts, 4)))) {
        set_error("%s: a misaligned buffer (commands 16 bytes, the others 4)", who);
        return UR_EINVAL;
    }
    return UR_OK;
}

int ur::check_raster_call(const char* who, const ur_ctx* ctx, const float* m0, const float* m1, const ur_raster_draws* draws, const void* target, const char* target_name,
                          uint32_t w, uint32_t h, const void* stats)
{
    if (!ctx || !m0 || !m1 || !draws) { set_error("%s: null context, matrix or draws", who); return UR_EINVAL; }
    if (w == 0u || h == 0u || w > UR_RASTER_MAX_TARGET || h > UR_RASTER_MAX_TARGET) { set_error("%s: a %u x %u target (1..%u)", who, w, h, UR_RASTER_MAX_TARGET); return UR_EINVAL; }
    return check_raster_draws(who, *draws, target, target_name, stats);
}

int ur::launch_visibility_raster(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, const float* depth, uint32_t* keys, uint32_t w,
                                 uint32_t h, uint32_t row0, uint32_t rows, uint32_t key_bits, bool d24, uint32_t* stats)
{
    const VisArgs vis{depth, row0, rows, key_bits};
    if (d24) return launch_raster<VisPolicy<true>>(ctx, view, projection, draws, keys, w * rows, w, h, 0.0f, stats, &vis);
    return launch_raster<VisPolicy<false>>(ctx, view, projection, draws, keys, w * rows, w, h, 0.0f, stats, &vis);
}

int ur::launch_masked_raster(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, float* depth, uint64_t* keys64, uint32_t* keys,
                             uint32_t w, uint32_t h, uint32_t row0, uint32_t rows, uint32_t key_bits, bool d24, uint32_t* stats, const ur_material* materials,
                             uint32_t material_count, uint32_t* won)
{
    const VisArgs vis{depth, row0, rows, key_bits};
    const MaskArgs mask{materials, material_count, ctx->lod_table};
    uint32_t* words = reinterpret_cast<uint32_t*>(keys64);
    const uint32_t n = w * rows;
    const int rc = d24 ? launch_raster<MaskPolicy<true>>(ctx, view, projection, draws, words, 2u * n, w, h, 0.0f, stats, &vis, &mask)
                       : launch_raster<MaskPolicy<false>>(ctx, view, projection, draws, words, 2u * n, w, h, 0.0f, stats, &vis, &mask);
    if (rc != UR_OK) return rc;
    hipLaunchKernelGGL(mask_merge_kernel, dim3((n + kThreads - 1u) / kThreads), dim3(kThreads), 0, ctx->stream, reinterpret_cast<unsigned long long*>(keys64), keys,
                       reinterpret_cast<uint32_t*>(depth) + (size_t)row0 * w, n, won);
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

int ur::launch_object_id_pick(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, const float* depth, uint32_t w, uint32_t h,
                              uint32_t key_bits, bool d24, const uint32_t* points, uint32_t point_count, ur_pick_result* results, uint32_t* stats)
{
    static_assert(sizeof(ur_pick_result) == 16, "a pick record is 16 bytes");
    UR_HIP_TRY(hipMemsetAsync(results, 0, (size_t)point_count * sizeof(ur_pick_result), ctx->stream));
    PickParams p{};
    p.point_count = point_count;
    for (uint32_t i = 0; i < point_count; ++i) p.points[i] = points[i];
    p.results = reinterpret_cast<unsigned long long*>(results);
    if (draws->command_count != 0u) {
        const VisArgs vis{depth, 0u, h, key_bits};
        const uint32_t blocks = fill_raster_params(p, ctx, view, projection, draws, w, h, stats, &vis);
        if (d24) hipLaunchKernelGGL(pick_kernel<VisPolicy<true>>, dim3(blocks), dim3(kThreads), 0, ctx->stream, p);
        else hipLaunchKernelGGL(pick_kernel<VisPolicy<false>>, dim3(blocks), dim3(kThreads), 0, ctx->stream, p);
        UR_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(pick_finish_kernel, dim3(1), dim3(64), 0, ctx->stream, p); // (every word is 0 without commands)
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

extern "C" {

int ur_raster_reserve(ur_ctx* ctx, uint32_t max_large_work_items)
{
    if (!ctx) { ur::set_error("ur_raster_reserve: null context"); return UR_EINVAL; }
    if (max_large_work_items == ctx->raster_queue_cap) return UR_OK;
    UR_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->raster_queue) (void)hipFree(ctx->raster_queue);
    ctx->raster_queue = nullptr;
    ctx->raster_queue_cap = 0;
    if (max_large_work_items == 0u) return UR_OK;
    const size_t bytes = ((size_t)kQueueHeaderDwords + (size_t)max_large_work_items * kKeyedEntryDwords) * sizeof(uint32_t);
    if (hipMalloc(&ctx->raster_queue, bytes) != hipSuccess) {
        ctx->raster_queue = nullptr;
        ur::set_error("ur_raster_reserve: allocation of %u large work items failed", max_large_work_items);
        return UR_ENOMEM;
    }
    ctx->raster_queue_cap = max_large_work_items;
    return UR_OK;
}

int ur_shadow_map(ur_ctx* ctx, const float* lvp, const ur_raster_draws* draws, float* shadow_map, uint32_t w, uint32_t h, uint32_t* stats4)
{
    const int rc = ur::check_raster_call("ur_shadow_map", ctx, lvp, lvp, draws, shadow_map, "shadow_map", w, h, stats4);
    if (rc != UR_OK) return rc;
    if (!(lvp[3] == 0.0f && lvp[7] == 0.0f && lvp[11] == 0.0f && lvp[15] == 1.0f)) {
        ur::set_error("ur_shadow_map: the light's fourth column is (%g, %g, %g, %g), not (0, 0, 0, 1): only orthographic lights are rasterised", lvp[3], lvp[7], lvp[11], lvp[15]);
        return UR_EUNSUPPORTED;
    }
    return launch_raster<ShadowPolicy>(ctx, lvp, nullptr, draws, reinterpret_cast<uint32_t*>(shadow_map), w * h, w, h, 1.0f, stats4, nullptr);
}

int ur_depth_prepass(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, float* depth, uint32_t w, uint32_t h, uint32_t flags,
                     uint32_t* stats6)
{
    int rc = ur::check_raster_call("ur_depth_prepass", ctx, view, projection, draws, depth, "depth", w, h, stats6);
    if (rc == UR_OK) rc = ur::check_depth_flags("ur_depth_prepass", flags);
    if (rc != UR_OK) return rc;
    if (flags & UR_DEPTH_QUANTIZE_D24) return launch_raster<DepthPolicy<true>>(ctx, view, projection, draws, reinterpret_cast<uint32_t*>(depth), w * h, w, h, 0.0f, stats6, nullptr);
    return launch_raster<DepthPolicy<false>>(ctx, view, projection, draws, reinterpret_cast<uint32_t*>(depth), w * h, w, h, 0.0f, stats6, nullptr);
}

} // extern "C"
