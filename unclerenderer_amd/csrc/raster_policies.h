// The policies of the raster kernels: what a pass does with a vertex and a triangle. ShadowMap first; the others say what they change.
// project():  rule 1 for one vertex.
// assemble(): from the three clip-space vertices to the target-space vertices S0..S3 (rule 2; DepthPrepass: the near clip in front of it);
//             returns how many triangles (S0, S[1 + e], S[2 + e]) the lane emits.
//
// Reference: the "ShadowMap" pass (DeferredRenderer.cpp:551-633), Shaders/ShadowMap.hlsl (position * World * LightViewProjection, no
// pixel shader), its pipeline (Renderer.cpp:240-300: CULL_MODE_FRONT, FrontCounterClockwise, LESS_EQUAL, zero bias, depth clip) and
// target (D32_FLOAT, cleared to 1.0). The result is a per-texel minimum, so it is specified to the bit: DESIGN.md section 3.7 is the
// rule, tests/shadow_ref.py restates it in numpy, and the kernels compute the same bytes. Built with -ffp-contract=off.
//
// DepthPrepass (DeferredRenderer.cpp:635-718, pipeline :1894-1961, Shaders/DeferredBasePass.hlsl:58-70): position * World * View *
// Projection under a perspective camera, reverse-Z (GREATER_EQUAL, cleared to 0.0: a per-texel maximum, the atomic mirrored),
// CULL_MODE_BACK, and a D24 target. DESIGN.md section 3.8 is its rule and tests/depth_ref.py the restatement. A lane clips its triangle
// against the near plane with selects on registers (no per-lane arrays): up to four vertices S0..S3 in target space, emitted triangle
// e = (S0, S[1 + e], S[2 + e]). The wave serves emitted triangle 0 of every lane, then, when a ballot finds a lane that was cut into
// two, runs the same code once more over emitted triangle 1.
#pragma once

#include "raster_params.h"

namespace {

// What a fragment's alpha test reads: nothing in the passes without one
struct NoAlpha {};
struct AlphaCtx {
    const MaskedParams* p;
    const float* lds; // the sampler's tables (texture_sample.h): code / 255 and the level thresholds; the decode part is not filled
};

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
// (csrc/raster_mask.hip)
template <bool D24>
struct MaskPolicy : VisPolicy<D24> {
    using Params = MaskedParams;
    using Alpha = AlphaCtx;
    static constexpr bool kMasked = true;
};

} // namespace
