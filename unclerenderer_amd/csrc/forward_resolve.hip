// The Forward pass' resolve for gfx950 — a lane per texel of the band turns the winning visibility key (csrc/raster.hip) into the HDR
// colour: it fetches the key's triangle again as GBuffer's resolve does (csrc/gbuffer_resolve.hip), forms the attributes
// Shaders/ForwardVS.hlsl forms, and runs Shaders/ForwardPS.hlsl:73-143 in two phases: the material (the maps through csrc/texture_sample.h,
// the world normal), then the shading (PCF shadow, EvaluatePBR, the prefiltered cube, the BRDF LUT, irradiance). DESIGN.md section 3.12
// is its rule, tests/forward_ref.py the restatement. Built with -ffp-contract=off; every divide and square root is IEEE.

#include "forward_resolve.h"
#include "resolve_pack.h"
#include "ur_device.h"
#include "visibility_key.h"

namespace {

using namespace ur_raster;
using ur::ForwardParams;

typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

constexpr uint32_t kLdsMips = 16u; // the cube's mip offsets in LDS: a lane indexes them by its own level

__device__ __forceinline__ float sat(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); } // a NaN stays
__device__ __forceinline__ float at_least(float x, float c) { return x < c ? c : x; }              // a NaN stays
__device__ __forceinline__ float mix2(float a, float b, float t) { return a + t * (b - a); }
__device__ __forceinline__ float dot3(const float (&a)[3], const float (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ float half_value(uint32_t bits) { return (float)__builtin_bit_cast(_Float16, (unsigned short)bits); }
__device__ __forceinline__ bool finite(float x) { return fabsf(x) <= kFloatMax; }

// D3D cube addressing (+X, -X, +Y, -Y, +Z, -Z; ties z > y > x): u = (sc / |ma| + 1) / 2
__device__ __forceinline__ void cube_face(const float (&d)[3], uint32_t& face, float& u, float& v)
{
    const float ax = fabsf(d[0]), ay = fabsf(d[1]), az = fabsf(d[2]);
    const bool zmaj = az >= ax && az >= ay, ymaj = !zmaj && ay >= ax;
    const float comp = zmaj ? d[2] : (ymaj ? d[1] : d[0]);
    face = (zmaj ? 4u : (ymaj ? 2u : 0u)) + (comp < 0.0f ? 1u : 0u);
    const float ma = fabsf(comp);
    const float sc = face == 0u ? -d[2] : (face == 1u ? d[2] : (face == 5u ? -d[0] : d[0]));
    const float tc = face == 2u ? d[2] : (face == 3u ? -d[2] : -d[1]);
    u = (sc / ma + 1.0f) * 0.5f;
    v = (tc / ma + 1.0f) * 0.5f;
}

// The 2 x 2 taps of one bilinear cube sample: 8-byte texels of the bordered face (no edge logic), and the weights
struct CubeTaps { u32x2_t t00, t10, t01, t11; float fx, fy; bool ok; };

__device__ __forceinline__ CubeTaps cube_taps(const uint2* __restrict__ env, uint32_t offset, uint32_t N, uint32_t face, float u, float v)
{
    CubeTaps t;
    t.ok = finite(u) && finite(v);
    const float x = (t.ok ? u : 0.5f) * (float)N - 0.5f, y = (t.ok ? v : 0.5f) * (float)N - 0.5f;
    const float x0 = floorf(x), y0 = floorf(y);
    t.fx = x - x0;
    t.fy = y - y0;
    const uint32_t i0 = (uint32_t)min(max((int)x0 + 1, 0), (int)N), j0 = (uint32_t)min(max((int)y0 + 1, 0), (int)N), E = N + 2u;
    const u32x2_t* at = reinterpret_cast<const u32x2_t*>(env) + offset + (size_t)((face * E + j0) * E + i0);
    t.t00 = at[0]; t.t10 = at[1]; t.t01 = at[E]; t.t11 = at[E + 1u];
    return t;
}

__device__ __forceinline__ void cube_filter(const CubeTaps& t, float (&out)[3])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t sh = c == 1 ? 16u : 0u;
        const float a = half_value((c == 2 ? t.t00.y : t.t00.x) >> sh), b = half_value((c == 2 ? t.t10.y : t.t10.x) >> sh);
        const float d = half_value((c == 2 ? t.t01.y : t.t01.x) >> sh), e = half_value((c == 2 ? t.t11.y : t.t11.x) >> sh);
        const float value = mix2(mix2(a, b, t.fx), mix2(d, e, t.fx), t.fy);
        out[c] = t.ok ? value : __builtin_nanf("");
    }
}

// TextureCube.SampleLevel's two mips: the level clamped to [0, mips - 1]; the upper mip's taps are loaded whatever the fraction is
struct CubeLevel { CubeTaps lo, hi; float fl; };

__device__ __forceinline__ CubeLevel cube_level_taps(const ForwardParams& p, const uint32_t* mip_offset, const float (&d)[3], float level)
{
    uint32_t face;
    float u, v;
    cube_face(d, face, u, v);
    const float top = (float)(p.env_mips - 1u);
    const float lv = level < 0.0f ? 0.0f : (level > top ? top : level);
    const uint32_t m0 = lv != lv ? 0u : (uint32_t)lv, m1 = min(m0 + 1u, p.env_mips - 1u);
    CubeLevel r;
    r.fl = lv - (float)m0;
    r.lo = cube_taps(p.env, mip_offset[m0], max(1u, p.env_base >> m0), face, u, v);
    r.hi = cube_taps(p.env, mip_offset[m1], max(1u, p.env_base >> m1), face, u, v);
    return r;
}

__device__ __forceinline__ void cube_level_filter(const CubeLevel& t, float (&out)[3])
{
    float lo[3], hi[3];
    cube_filter(t.lo, lo);
    cube_filter(t.hi, hi);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = t.fl != 0.0f ? mix2(lo[c], hi[c], t.fl) : lo[c];
}

// The BRDF LUT: bilinear at uv * size - 0.5, clamped, texel = code / 65535 (R in the low half)
struct LutTaps { uint32_t t00, t10, t01, t11; float fx, fy; bool ok; };

__device__ __forceinline__ LutTaps lut_taps(const ForwardParams& p, float u, float v)
{
    LutTaps t;
    t.ok = finite(u) && finite(v);
    const float x = (t.ok ? u : 0.0f) * (float)p.lut_w - 0.5f, y = (t.ok ? v : 0.0f) * (float)p.lut_h - 0.5f;
    const float x0 = floorf(x), y0 = floorf(y);
    t.fx = x - x0;
    t.fy = y - y0;
    const int W = (int)p.lut_w, H = (int)p.lut_h;
    const int i = (int)fminf(fmaxf(x0, -1.0f), (float)W), j = (int)fminf(fmaxf(y0, -1.0f), (float)H);
    const uint32_t i0 = (uint32_t)min(max(i, 0), W - 1), i1 = (uint32_t)min(max(i + 1, 0), W - 1);
    const uint32_t j0 = (uint32_t)min(max(j, 0), H - 1), j1 = (uint32_t)min(max(j + 1, 0), H - 1);
    t.t00 = p.lut[j0 * p.lut_w + i0]; t.t10 = p.lut[j0 * p.lut_w + i1];
    t.t01 = p.lut[j1 * p.lut_w + i0]; t.t11 = p.lut[j1 * p.lut_w + i1];
    return t;
}

__device__ __forceinline__ void lut_filter(const LutTaps& t, float& a, float& b)
{
    float out[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const uint32_t sh = 16u * (uint32_t)c;
        const float v00 = (float)((t.t00 >> sh) & 0xFFFFu) / 65535.0f, v10 = (float)((t.t10 >> sh) & 0xFFFFu) / 65535.0f;
        const float v01 = (float)((t.t01 >> sh) & 0xFFFFu) / 65535.0f, v11 = (float)((t.t11 >> sh) & 0xFFFFu) / 65535.0f;
        const float value = mix2(mix2(v00, v10, t.fx), mix2(v01, v11, t.fx), t.fy);
        out[c] = t.ok ? value : __builtin_nanf("");
    }
    a = out[0];
    b = out[1];
}

// SampleCmpLevelZero: four LESS_EQUAL compares around uv * size - 0.5, a tap outside the map reads the border 1.0, blended bilinearly
__device__ __forceinline__ float sample_cmp(const float* __restrict__ map, int W, int H, float u, float v, float cmp)
{
    const float x = u * (float)W - 0.5f, y = v * (float)H - 0.5f;
    const float x0 = floorf(x), y0 = floorf(y);
    const float fx = x - x0, fy = y - y0;
    const int i0 = (int)fminf(fmaxf(x0, -2.0f), (float)W), j0 = (int)fminf(fmaxf(y0, -2.0f), (float)H);
    float r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = i0 + (k & 1), j = j0 + (k >> 1);
        const bool inside = i >= 0 && j >= 0 && i < W && j < H;
        const float t = map[(size_t)min(max(j, 0), H - 1) * (size_t)W + (size_t)min(max(i, 0), W - 1)];
        r[k] = cmp <= (inside ? t : 1.0f) ? 1.0f : 0.0f;
    }
    return mix2(mix2(r[0], r[1], fx), mix2(r[2], r[3], fx), fy);
}

// What phase 1 hands to phase 2
struct Surface { float albedo[3], emissive[3], n[3], wpos[3], metallic, roughness; };

// ForwardPS.hlsl:97-142 on the material's values
__device__ __forceinline__ void shade(const ForwardParams& p, const uint32_t* mip_offset, const Surface& s, float (&color)[3])
{
    // ---- the vectors, and every gather: the cube's two lookups, the LUT, the shadow taps
    const float toeye[3] = {p.camera[0] - s.wpos[0], p.camera[1] - s.wpos[1], p.camera[2] - s.wpos[2]};
    const float vl = sqrtf(dot3(toeye, toeye));
    const float V[3] = {toeye[0] / vl, toeye[1] / vl, toeye[2] / vl};
    const float ll = sqrtf((p.light_direction[0] * p.light_direction[0] + p.light_direction[1] * p.light_direction[1]) + p.light_direction[2] * p.light_direction[2]);
    const float L[3] = {p.light_direction[0] / ll, p.light_direction[1] / ll, p.light_direction[2] / ll};
    const float inc[3] = {-V[0], -V[1], -V[2]};
    const float twice = 2.0f * dot3(inc, s.n);
    const float refl[3] = {inc[0] - twice * s.n[0], inc[1] - twice * s.n[1], inc[2] - twice * s.n[2]};
    const float NdotV = sat(dot3(s.n, V));
    const CubeLevel pre_taps = cube_level_taps(p, mip_offset, refl, s.roughness * p.max_mip);
    const CubeLevel irr_taps = cube_level_taps(p, mip_offset, s.n, p.max_mip);
    const LutTaps brdf_taps = lut_taps(p, NdotV, s.roughness);
    float shadow = 1.0f;
    {
        float sp[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) sp[k] = ((s.wpos[0] * p.lvp[k] + s.wpos[1] * p.lvp[4 + k]) + s.wpos[2] * p.lvp[8 + k]) + p.lvp[12 + k];
        const float su = (sp[0] / sp[3]) * 0.5f + 0.5f, sv = (sp[1] / sp[3]) * -0.5f + 0.5f;
        if (p.shadow_strength > 0.0f && su >= 0.0f && sv >= 0.0f && su <= 1.0f && sv <= 1.0f) {
            const float hx = 0.5f / p.shadow_size[0], hy = 0.5f / p.shadow_size[1];
            const float cmp = sp[2] / sp[3] - p.shadow_bias;
            const float s0 = sample_cmp(p.shadow, p.shadow_w, p.shadow_h, su + hx, sv + hy, cmp);
            const float s1 = sample_cmp(p.shadow, p.shadow_w, p.shadow_h, su - hx, sv + hy, cmp);
            const float s2 = sample_cmp(p.shadow, p.shadow_w, p.shadow_h, su + hx, sv - hy, cmp);
            const float s3 = sample_cmp(p.shadow, p.shadow_w, p.shadow_h, su - hx, sv - hy, cmp);
            const float pcf = 0.25f * (((s0 + s1) + s2) + s3);
            shadow = 1.0f + p.shadow_strength * (pcf - 1.0f);
        }
    }
    // ---- EvaluatePBR (PBRCommon.hlsl)
    const float hv[3] = {V[0] + L[0], V[1] + L[1], V[2] + L[2]};
    const float hl = sqrtf(dot3(hv, hv));
    const float H[3] = {hv[0] / hl, hv[1] / hl, hv[2] / hl};
    const float NdotL = sat(dot3(s.n, L)), NdotH = sat(dot3(s.n, H)), VdotH = sat(dot3(V, H));
    const float alpha = s.roughness * s.roughness, alpha2 = alpha * alpha;
    const float denom = (NdotH * NdotH) * (alpha2 - 1.0f) + 1.0f;
    const float D = alpha2 / at_least((3.14159265f * denom) * denom, 1e-4f);
    const float k1 = s.roughness + 1.0f, k = (k1 * k1) / 8.0f;
    const float G = (NdotV / (NdotV * (1.0f - k) + k)) * (NdotL / (NdotL * (1.0f - k) + k));
    const float x1 = 1.0f - VdotH, x2 = x1 * x1, p5 = (x2 * x2) * x1; // pow(x, 5) as a fixed product
    const float spec_denominator = at_least((4.0f * NdotL) * NdotV, 1e-4f);
    float F0[3], lighting[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        F0[c] = 0.04f + s.metallic * (s.albedo[c] - 0.04f);
        const float F = F0[c] + (1.0f - F0[c]) * p5;
        const float specular = ((D * G) * F) / spec_denominator;
        const float kd = (1.0f - F) * (1.0f - s.metallic);
        const float pbr = (kd * s.albedo[c] + specular) * NdotL;
        lighting[c] = ((pbr * p.light_intensity) * p.light_color[c]) * shadow;
    }
    // ---- the image-based terms
    float pre[3], irr[3], bx, by;
    cube_level_filter(pre_taps, pre);
    cube_level_filter(irr_taps, irr);
    lut_filter(brdf_taps, bx, by);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float spec_ibl = pre[c] * (F0[c] * bx + by);
        const float diff_ibl = (irr[c] * s.albedo[c]) * (1.0f - s.metallic);
        color[c] = (lighting[c] + (diff_ibl + spec_ibl)) + s.emissive[c];
    }
}

// Three waves per SIMD are asked for by name (168 of the 512 registers): with the BC taps of the sampler the allocator otherwise settles at
// 178 and two waves; under the bound it finds 167 without scratch
template <bool MAPS, bool MASKED>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(3))) void forward_resolve_kernel(ForwardParams p)
{
    __shared__ uint32_t mip_offset[kLdsMips];
    __shared__ float sampler_tables[MAPS ? kLdsFloats : 1u];
    if (threadIdx.x < kLdsMips) mip_offset[threadIdx.x] = p.env_offset[threadIdx.x];
    if constexpr (MAPS) fill_sampler_tables<true>(sampler_tables, p.decode, p.lod);
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t key = i < p.n ? p.keys[i] : 0u;
    __syncthreads();
    if (__ballot(key != 0u) == 0ull) return; // nothing of this wave's 64 texels is covered
    if (key == 0u) return;                   // hdr keeps what the caller drew before (the sky)
    uint32_t t;
    const uint32_t slot = key_slot<MASKED>(p, key, i, t);
    const KeyDraw d = key_draw(p.commands, slot, t);
    const float* cb = d.cb;
    const float (&W)[16] = d.W;

    // ---- ForwardVS.hlsl on the three vertices: clip position (rule 1), WorldPos, Normal * (float3x3)World, the normalised tangent, Color.
    // (One text with the vertex stage of GBuffer's resolve, csrc/gbuffer_resolve.hip, and not one function: in every form tried the
    // textured kernel here spills two or three registers to scratch at its three-wave bound. DESIGN.md 3.14 has the table)
    float c[3][4], wp[3][3], wn[3][3], col[3][3];
    [[maybe_unused]] float uv[3][2], tg[3][4];
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const uint64_t vi = (uint64_t)(d.base_vertex + (long long)d.indices[d.first + (uint32_t)v]);
        const f32x4u_t* vp = reinterpret_cast<const f32x4u_t*>(d.vertices + vi * d.stride);
        const f32x4u_t v0 = vp[0], v1 = vp[1], v3 = vp[3];
        const float x = v0.x, y = v0.y, z = v0.z, nx = v0.w, ny = v1.x, nz = v1.y;
        float wv[4], vv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) wv[k] = ((x * W[k] + y * W[4 + k]) + z * W[8 + k]) + W[12 + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) vv[k] = ((wv[0] * p.V[k] + wv[1] * p.V[4 + k]) + wv[2] * p.V[8 + k]) + wv[3] * p.V[12 + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) c[v][k] = ((vv[0] * p.Pr[k] + vv[1] * p.Pr[4 + k]) + vv[2] * p.Pr[8 + k]) + vv[3] * p.Pr[12 + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            wp[v][k] = wv[k];
            wn[v][k] = (nx * W[k] + ny * W[4 + k]) + nz * W[8 + k];
        }
        col[v][0] = v3.x; col[v][1] = v3.y; col[v][2] = v3.z;
        if constexpr (MAPS) {
            const f32x4u_t v2 = vp[2];
            uv[v][0] = v1.z; uv[v][1] = v1.w;
            float wt[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) wt[k] = (v2.x * W[k] + v2.y * W[4 + k]) + v2.z * W[8 + k];
            const float tl = sqrtf((wt[0] * wt[0] + wt[1] * wt[1]) + wt[2] * wt[2]);
            tg[v][0] = wt[0] / tl; tg[v][1] = wt[1] / tl; tg[v][2] = wt[2] / tl; tg[v][3] = v2.w;
        }
    }

    // ---- the piece that covers this centre and its weights (gbuffer_interp.h)
    float SX[4], SY[4], vw[4], B[4][3];
    bool one;
    clip_polygon(c, p.half_w, p.half_h, SX, SY, vw, B, one);
    const uint32_t row = i / p.w, column = i - row * p.w;
    Piece pc;
    covering_piece(SX, SY, vw, one, 256 * (int)column + 128, 256 * (int)(p.row0 + row) + 128, pc);
    float b[3];
    piece_weights(pc, pc.l0, pc.l1, pc.l2, B, b);
    float n[3], colour[3];
    Surface s;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        n[k] = (b[0] * wn[0][k] + b[1] * wn[1][k]) + b[2] * wn[2][k];
        s.wpos[k] = (b[0] * wp[0][k] + b[1] * wp[1][k]) + b[2] * wp[2][k];
        colour[k] = (b[0] * col[0][k] + b[1] * col[1][k]) + b[2] * col[2][k];
    }

    // ---- phase 1: the material (ForwardPS.hlsl:75-106, ComputeWorldNormal)
    const float nl = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    const float vn[3] = {n[0] / nl, n[1] / nl, n[2] / nl};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s.n[k] = vn[k];
        s.albedo[k] = cb[64 + k] * colour[k];
        s.emissive[k] = cb[80 + k];
    }
    s.metallic = cb[104];
    s.roughness = cb[105];
    if constexpr (MAPS) {
        uint32_t bits = 0u;
        if (slot < p.material_count) bits = reinterpret_cast<const uint32_t*>(p.materials + slot)[16] & 15u;
        float base[3] = {1.0f, 1.0f, 1.0f}, mr[3] = {1.0f, 1.0f, 1.0f}, nm[3] = {0.5f, 0.5f, 1.0f}, em[3] = {1.0f, 1.0f, 1.0f};
        if (__ballot(bits != 0u) != 0ull) {
            const bool odd_column = (column & 1u) != 0u, odd_row = ((p.row0 + row) & 1u) != 0u;
            float pu[3], pv[3]; // TEXCOORD at the centre, the horizontal and the vertical partner
            quad_texcoords(pc, B, uv, odd_column, odd_row, pu, pv);
            // (no SPLIT: 168 registers do not hold both forms of the gather)
            sample_maps<false, true>(p.materials + slot, bits, cb, pu, pv, odd_column, odd_row, sampler_tables, base, mr, nm, em);
        }
        if (bits & UR_MATERIAL_NORMAL_MAP) {
            float tn[3], bt[3];
            tangent_frame(vn, b, tg, tn, bt);
            // the tangent-space vector: the map's three channels (ForwardPS.hlsl takes the blue as it is; GBuffer's shader reconstructs it)
            const float nr = nm[0] * 2.0f - 1.0f, ng = nm[1] * 2.0f - 1.0f, nb = nm[2] * 2.0f - 1.0f;
            const bool flat = sqrtf((nr * nr + ng * ng) + nb * nb) < 1e-5f;
            const float e[3] = {flat ? 0.0f : nr, flat ? 0.0f : ng, flat ? 1.0f : nb};
            tangent_to_world(e, tn, bt, vn, s.n);
        }
        apply_map_factors(bits, base, mr, em, s.albedo, s.metallic, s.roughness, s.emissive);
    }

    // ---- phase 2: the shading, and the store
    float color[3];
    shade(p, mip_offset, s, color);
    ur::store_once_b64(p.hdr + i, pack_half4(color[0], color[1], color[2], 1.0f));
}

} // namespace

int ur::launch_forward_resolve(ur_ctx* ctx, const ForwardParams& p, bool maps, bool masked)
{
    const uint32_t blocks = (p.n + kThreads - 1u) / kThreads;
    if (maps && masked) hipLaunchKernelGGL((forward_resolve_kernel<true, true>), dim3(blocks), dim3(kThreads), 0, ctx->stream, p);
    else if (maps) hipLaunchKernelGGL((forward_resolve_kernel<true, false>), dim3(blocks), dim3(kThreads), 0, ctx->stream, p);
    else if (masked) hipLaunchKernelGGL((forward_resolve_kernel<false, true>), dim3(blocks), dim3(kThreads), 0, ctx->stream, p);
    else hipLaunchKernelGGL((forward_resolve_kernel<false, false>), dim3(blocks), dim3(kThreads), 0, ctx->stream, p);
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}
