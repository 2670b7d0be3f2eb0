// DeferredLighting (GGX + IBL) and SkyAtmosphere for gfx950, the per-tile kernel: one workgroup per 64 x 4 pixels, plain loads.
// It takes sky-only launches and every configuration the streaming kernel (lighting.hip, whose top comment describes the pass and
// its references) declines: launch_lighting() in lighting_host.hip decides per launch, never per row. One lane shades one pixel; a
// wave64 covers a 16 x 4 pixel tile. The PCF, the trilinear cube lookups and the BRDF LUT are filtered in ALU.

#include "lighting_device.h"

namespace {

using namespace ur;

// HDR out of the per-tile kernel: written once, write-through + nontemporal like the streaming kernel's store (store_hdr, lighting.hip)
__device__ __forceinline__ void st_hdr_once(void* base, uint32_t byte_offset, half4_t v)
{
    typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
    u32x2_t u;
    __builtin_memcpy(&u, &v, 8);
    asm volatile("global_store_dwordx2 %0, %1, %2 sc1 nt" ::"v"(byte_offset), "v"(u), "s"(base) : "memory");
}

// ---- bordered cube: face f of mip m is (N+2)^2 texels, border = seamless neighbours (ur_stage_env_cube) -----------
struct CubeUV { uint32_t face; float u, v; };
// D3D cube addressing (+X,-X,+Y,-Y,+Z,-Z; ties z > y > x; uc/vc table of the oracle's SelectCubeFace) is exactly what
// gfx950's v_cubeid/v_cubesc/v_cubetc/v_cubema compute (cubema = 2 * signed major axis), four instructions instead of a
// compare/select ladder.
__device__ __forceinline__ CubeUV cube_face(F3 d)
{
    CubeUV r;
    r.face = (uint32_t)__builtin_amdgcn_cubeid(d.x, d.y, d.z);
    const float inv = rcp(fabsf(__builtin_amdgcn_cubema(d.x, d.y, d.z))); // 1 / (2 |major|)
    r.u = fmaf(__builtin_amdgcn_cubesc(d.x, d.y, d.z), inv, 0.5f);
    r.v = fmaf(__builtin_amdgcn_cubetc(d.x, d.y, d.z), inv, 0.5f);
    return r;
}

// u,v in [0,1] (a NaN direction gives index 0 and NaN weights, i.e. a NaN result, like the reference).
__device__ __forceinline__ CubeTaps cube_taps_load(const void* __restrict__ env, uint32_t mipOffset, uint32_t N, const CubeUV& c)
{
    const uint32_t E = N + 2u;
    const float fN = (float)N;
    const float x = fmaf(c.u, fN, 0.5f), y = fmaf(c.v, fN, 0.5f); // bordered coordinates, in [0.5, N + 0.5]
    const uint32_t i0 = (uint32_t)x, j0 = (uint32_t)y;            // truncation == floor for x >= 0; NaN -> 0
    CubeTaps t;
    t.fx = x - (float)i0;
    t.fy = y - (float)j0;
    const uint32_t off = (mipOffset + (c.face * E + j0) * E + i0) * 8u, row = E * 8u;
    // the two taps of a row are adjacent in memory: one 16-byte load per row (8-byte aligned; gfx950 loads may be unaligned)
    t.r0 = ld<uint4u>(env, off);
    t.r1 = ld<uint4u>(env, off + row);
    return t;
}

struct LutTaps { uint32_t t00, t10, t01, t11; float fx, fy; };
__device__ __forceinline__ LutTaps lut_taps_load(const LightingParams& p, float u, float v)
{
    const float x = fmaf(u, (float)p.lutW, -0.5f), y = fmaf(v, (float)p.lutH, -0.5f);
    const float x0 = floorf(x), y0 = floorf(y);
    LutTaps t;
    t.fx = x - x0;
    t.fy = y - y0;
    const int W1 = (int)p.lutW - 1, H1 = (int)p.lutH - 1;
    const int i0 = min(max((int)x0, 0), W1), i1 = min(max((int)x0 + 1, 0), W1); // clamp addressing
    const int j0 = min(max((int)y0, 0), H1), j1 = min(max((int)y0 + 1, 0), H1);
    const uint32_t r0 = (uint32_t)j0 * p.lutW, r1 = (uint32_t)j1 * p.lutW;
    t.t00 = ld<uint32_t>(p.lut, (r0 + i0) * 4u);
    t.t10 = ld<uint32_t>(p.lut, (r0 + i1) * 4u);
    t.t01 = ld<uint32_t>(p.lut, (r1 + i0) * 4u);
    t.t11 = ld<uint32_t>(p.lut, (r1 + i1) * 4u);
    return t;
}
__device__ __forceinline__ void lut_taps_filter(const LutTaps& t, float& a, float& b)
{
    const float s = 1.0f / 65535.0f;
    const float wy1 = t.fy * s, wy0 = s - wy1;
    const float w10 = wy0 * t.fx, w00 = wy0 - w10, w11 = wy1 * t.fx, w01 = wy1 - w11;
    a = fmaf(w11, (float)(t.t11 & 0xFFFFu), fmaf(w01, (float)(t.t01 & 0xFFFFu), fmaf(w10, (float)(t.t10 & 0xFFFFu), w00 * (float)(t.t00 & 0xFFFFu))));
    b = fmaf(w11, (float)(t.t11 >> 16), fmaf(w01, (float)(t.t01 >> 16), fmaf(w10, (float)(t.t10 >> 16), w00 * (float)(t.t00 >> 16))));
}

// step(t) = (cmp <= t), LESS_EQUAL as the shader states it (a NaN on either side fails). A compare, not
// saturate((t - cmp) * 2^126 + 1): that form returns a fraction when 0 < |t - cmp| < 2^-126 (cmp = 0, t = -2^-149).
__device__ __forceinline__ float step_le(float cmp, float t)
{
    return cmp <= t ? 1.0f : 0.0f;
}

// The four PCF samples of DeferredLighting.hlsl:62-70: SampleCmpLevelZero (bilinear blend of four LESS_EQUAL results,
// border = 1.0) at (u, u + 1 texel) x (v, v + 1 texel). The second sample's footprint is the first's shifted by exactly
// one texel, so the union is a 3x3 block and the sum of the four bilinear blends factors into separable weights
// (1-f, 1, f) per axis: 9 loads, 9 compares. (The oracle evaluates the shifted coordinate (u + 1/W) * W - 0.5 in fp32;
// its fraction differs from f by O(1e-4), i.e. O(1e-5) in the result — far inside the HDR tolerance.)
struct ShadowTaps { float3u ra, rb, rc; float fx, fy; int ia, ja; };
__device__ __forceinline__ ShadowTaps shadow_taps_load(const LightingParams& p, float su, float sv)
{
    const float xa = fmaf(su, p.shadowW, -0.5f), ya = fmaf(sv, p.shadowH, -0.5f);
    const float xa0 = floorf(xa), ya0 = floorf(ya);
    ShadowTaps t;
    t.fx = xa - xa0;
    t.fy = ya - ya0;
    t.ia = (int)xa0;
    t.ja = (int)ya0;
    // clamped block origin: always a valid address (the host rejects shadow maps smaller than 3x3)
    const uint32_t ic = (uint32_t)min(max(t.ia, 0), p.shadowWi - 3), jc = (uint32_t)min(max(t.ja, 0), p.shadowHi - 3);
    const uint32_t W = (uint32_t)p.shadowWi;
    const uint32_t o0 = (jc * W + ic) * 4u, o1 = o0 + W * 4u, o2 = o1 + W * 4u;
    t.ra = ld<float3u>(p.shadow, o0); // one 12-byte load per row
    t.rb = ld<float3u>(p.shadow, o1);
    t.rc = ld<float3u>(p.shadow, o2);
    return t;
}
__device__ __forceinline__ float shadow_taps_filter(const ShadowTaps& t, float cmp)
{
    const float wx0 = 1.0f - t.fx, wy0 = 1.0f - t.fy;
    const float r0 = fmaf(step_le(cmp, t.ra.z), t.fx, fmaf(step_le(cmp, t.ra.x), wx0, step_le(cmp, t.ra.y)));
    const float r1 = fmaf(step_le(cmp, t.rb.z), t.fx, fmaf(step_le(cmp, t.rb.x), wx0, step_le(cmp, t.rb.y)));
    const float r2 = fmaf(step_le(cmp, t.rc.z), t.fx, fmaf(step_le(cmp, t.rc.x), wx0, step_le(cmp, t.rc.y)));
    return 0.25f * fmaf(t.fy, r2, fmaf(wy0, r0, r1));
}
// footprint touches the border (or the map is tiny): out-of-range taps read the border colour 1.0
__device__ __noinline__ float shadow_pcf_border(const float* __restrict__ map, int W, int H, int ia, int ja, float fx, float fy, float cmp)
{
    float acc = 0.0f;
    for (int r = 0; r < 3; ++r) {
        float s = 0.0f;
        for (int c = 0; c < 3; ++c) {
            const int xi = ia + c, yj = ja + r;
            const bool in = xi >= 0 && yj >= 0 && xi < W && yj < H;
            const float t = in ? map[(uint32_t)yj * (uint32_t)W + (uint32_t)xi] : 1.0f;
            s += cmp <= t ? (c == 0 ? 1.0f - fx : (c == 1 ? 1.0f : fx)) : 0.0f;
        }
        acc = fmaf(r == 0 ? 1.0f - fy : (r == 1 ? 1.0f : fy), s, acc);
    }
    return 0.25f * acc;
}

// DeferredLighting.hlsl:35-94 for one pixel. (a,b) = camera ray (ndc.x/P11, -ndc.y/P22); viewPos = viewZ * (a, b, 1).
template <bool SHADOWS>
__device__ __forceinline__ F3 shade_pixel(const LightingParams& p, const float* srgb, const uint32_t* mipOffset, float ra, float rb, half4_t ga, half4_t gb,
                                          uint32_t gc)
{
    // ---- decode, view vectors ------------------------------------------------------------------------------------------
    const float nx = (float)ga.x, ny = (float)ga.y, nz = (float)ga.z;
    const float nr = rsq(fmaf(nz, nz, fmaf(ny, ny, nx * nx))); // normalize(0) = NaN, as in the reference
    const F3 N = f3(nx * nr, ny * nr, nz * nr);
    const float viewZ = -(float)ga.w;
    const float spec0 = (float)gb.x, metallic = (float)gb.y, roughness = (float)gb.z;
    // V = normalize(-viewPos) = -sign(viewZ) * (a,b,1)/|(a,b,1)|
    const float rl = rsq(fmaf(ra, ra, fmaf(rb, rb, 1.0f)));
    const float vs = viewZ > 0.0f ? -rl : (viewZ < 0.0f ? rl : __builtin_nanf("")); // normalize(0) = NaN
    const F3 V = f3(ra * vs, rb * vs, vs);
    const F3 L = f3(p.L[0], p.L[1], p.L[2]);
    const float NdotVraw = dot(N, V);
    const float NdotV = sat(NdotVraw);

    // ---- issue every gather ------------------------------------------------------------------------------------------
    // IBL: world vectors are the view-space ones rotated by (float3x3)ViewInverse; reflect(-V, N) = 2 N (N.V) - V
    // With a rigid view matrix whose origin is CameraPosition (every camera the reference builds) that rotation keeps lengths and
    // angles, worldView is the rotated V and dot(worldNormal, worldView) = N.V. Otherwise (uniform, p.general) the vectors are formed
    // as the shader writes them: worldPos = viewPos * ViewInverse, worldView = normalize(CameraPosition - worldPos),
    // worldNormal = normalize(normal * (float3x3)ViewInverse) (DeferredLighting.hlsl:55,76-78,84).
    F3 wR = f3(0.0f, 0.0f, 0.0f), wN = f3(0.0f, 0.0f, 0.0f);
    float NdotVibl = NdotV;
    if (p.general == 0u) {
        const float t2 = 2.0f * NdotVraw;
        wR = rot(f3(fmaf(t2, N.x, -V.x), fmaf(t2, N.y, -V.y), fmaf(t2, N.z, -V.z)), p.R);
        wN = rot(N, p.R);
    } else {
        const F3 wp = rot(f3(ra * viewZ, rb * viewZ, viewZ), p.R);
        F3 wv = f3(p.camPos[0] - (wp.x + p.VIt[0]), p.camPos[1] - (wp.y + p.VIt[1]), p.camPos[2] - (wp.z + p.VIt[2]));
        const float wvr = rsq(dot(wv, wv));
        wv = f3(wv.x * wvr, wv.y * wvr, wv.z * wvr);
        wN = rot(N, p.R);
        const float wnr = rsq(dot(wN, wN));
        wN = f3(wN.x * wnr, wN.y * wnr, wN.z * wnr);
        const float nv = dot(wN, wv);
        wR = f3(fmaf(2.0f * nv, wN.x, -wv.x), fmaf(2.0f * nv, wN.y, -wv.y), fmaf(2.0f * nv, wN.z, -wv.z)); // reflect(-worldView, worldNormal)
        NdotVibl = sat(nv);
    }
    const CubeUV cr = cube_face(wR);
    const CubeUV cn = cube_face(wN);
    const float lvl = fminf(fmaxf(roughness * p.maxMip, 0.0f), (float)(p.envMips - 1u));
    const uint32_t m0 = (uint32_t)lvl, m1 = min(m0 + 1u, p.envMips - 1u);
    const float fl = lvl - (float)m0; // m1 == m0 only when fl == 0: the second mip then carries weight 0
    const CubeTaps pre0 = cube_taps_load(p.env, mipOffset[m0], max(1u, p.envBase >> m0), cr);
    const CubeTaps pre1 = cube_taps_load(p.env, mipOffset[m1], max(1u, p.envBase >> m1), cr);
    const CubeTaps irr0 = cube_taps_load(p.env, p.irrOffset0, p.irrN0, cn);
    const LutTaps lut = lut_taps_load(p, NdotVibl, roughness);
    // The shadow term multiplies NdotL: a wave whose every pixel faces away from the light skips the PCF altogether
    // (same result: direct = 0). Coherent G-buffers make this common (ceilings, walls turned from the sun).
    const float NdotL = sat(dot(N, L));
    const bool wave_lit = SHADOWS && __any(NdotL > 0.0f);
    float su = 0.0f, sv = 0.0f, cmp = 0.0f;
    bool lit = false;
    ShadowTaps sh;
    if (wave_lit) {
        // shadow clip = viewZ * ((a,b,1) * M3) + M[3]
        const float qx = fmaf(rb, p.SQ[4], fmaf(ra, p.SQ[0], p.SQ[8]));
        const float qy = fmaf(rb, p.SQ[5], fmaf(ra, p.SQ[1], p.SQ[9]));
        const float qz = fmaf(rb, p.SQ[6], fmaf(ra, p.SQ[2], p.SQ[10]));
        const float qw = fmaf(rb, p.SQ[7], fmaf(ra, p.SQ[3], p.SQ[11]));
        const float iw = rcp(fmaf(viewZ, qw, p.ST[3]));
        su = fmaf(fmaf(viewZ, qx, p.ST[0]) * iw, 0.5f, 0.5f);
        sv = fmaf(fmaf(viewZ, qy, p.ST[1]) * iw, -0.5f, 0.5f);
        cmp = fmaf(viewZ, qz, p.ST[2]) * iw - p.shadowBias;
        lit = su >= 0.0f && sv >= 0.0f && su <= 1.0f && sv <= 1.0f;
        if (p.shadowSmall == 0u) sh = shadow_taps_load(p, su, sv); // (uniform; the 3x3 block needs a map of at least 3x3 texels)
        else sh = ShadowTaps{};
    }
    const F3 albedo = f3(srgb[gc & 0xFFu], srgb[(gc >> 8) & 0xFFu], srgb[(gc >> 16) & 0xFFu]);

    // ---- EvaluatePBR, PBRCommon.hlsl:24-48 (runs while the gathers are in flight) --------------------------------------------
    const F3 F0 = mix(f3(spec0, spec0, spec0), albedo, metallic);
    F3 Hv = f3(V.x + L.x, V.y + L.y, V.z + L.z);
    const float hr = rsq(dot(Hv, Hv));
    const float NdotH = sat(dot(N, Hv) * hr);
    const float VdotH = dot(V, Hv) * hr; // = (1 + V.L)/|V + L| in [0,1]: saturate is the identity up to rounding
    const float alpha = roughness * roughness;
    const float alpha2 = alpha * alpha;
    const float denom = fmaf(NdotH * NdotH, alpha2 - 1.0f, 1.0f);
    const float D = alpha2 * rcp(fmaxf(3.14159265f * denom * denom, 1e-4f));
    float k = roughness + 1.0f;
    k = (k * k) * 0.125f;
    const float omk = 1.0f - k;
    // G / max(4 NdotL NdotV, 1e-4) * D, one reciprocal for the three denominators
    const float gv = fmaf(NdotV, omk, k), gl = fmaf(NdotL, omk, k);
    const float sc = (D * NdotV * NdotL) * rcp(gv * gl * fmaxf(4.0f * NdotL * NdotV, 1e-4f));
    const float om = 1.0f - VdotH;
    const float om2 = om * om;
    const float p5 = om2 * om2 * om;
    const float kdm = 1.0f - metallic;

    // ---- filter ---------------------------------------------------------------------------------------------------------------
    float shadow = 1.0f;
    if (wave_lit) {
        const bool fast = p.shadowSmall == 0u && sh.ia >= 0 && sh.ja >= 0 && sh.ia + 2 < p.shadowWi && sh.ja + 2 < p.shadowHi;
        float s = shadow_taps_filter(sh, cmp);
        if (__builtin_expect(lit && !fast, 0)) {
            const float xa = fmaf(su, p.shadowW, -0.5f), ya = fmaf(sv, p.shadowH, -0.5f);
            const float xa0 = floorf(xa), ya0 = floorf(ya);
            s = shadow_pcf_border(p.shadow, p.shadowWi, p.shadowHi, (int)xa0, (int)ya0, xa - xa0, ya - ya0, cmp);
        }
        shadow = lit ? mix(1.0f, s, p.shadowStrength) : 1.0f;
    }
    const float sh_l = shadow * NdotL;
    F3 prefiltered, irradiance;
    cube_taps_filter<false>(prefiltered, pre0, 1.0f - fl);
    cube_taps_filter<true>(prefiltered, pre1, fl);
    cube_taps_filter<false>(irradiance, irr0, 1.0f - p.irrFrac);
    if (p.irrFrac != 0.0f) cube_taps_filter<true>(irradiance, cube_taps_load(p.env, p.irrOffset1, p.irrN1, cn), p.irrFrac); // uniform
    float ba, bb;
    lut_taps_filter(lut, ba, bb);

    F3 color;
#define UR_CHANNEL(ch, i)                                                                                     \
    {                                                                                                         \
        const float A = kdm * albedo.ch;                     /* (1 - metallic) * albedo: diffuse weight, also irradiance's */ \
        const float F = fmaf(1.0f - F0.ch, p5, F0.ch);                                                        \
        const float direct = fmaf(F, sc - A, A);             /* (1-F) A + F sc */                            \
        const float ambient = fmaf(irradiance.ch, A, prefiltered.ch * fmaf(F0.ch, ba, bb));                   \
        color.ch = fmaf(direct, p.lightRGB[i] * sh_l, ambient);                                               \
    }
    UR_CHANNEL(x, 0)
    UR_CHANNEL(y, 1)
    UR_CHANNEL(z, 2)
#undef UR_CHANNEL
    return color;
}

// A workgroup is 4 waves; a wave covers TW x TH pixels; the four waves sit side by side in x.
template <int MODE, bool SHADOWS, int TW, int WAVES>
__global__ __launch_bounds__(256, WAVES) void lighting_kernel(LightingParams p)
{
    constexpr int TH = 64 / TW;
    __shared__ float srgb[256];
    if (MODE != ur::UR_MODE_SKY) {
        srgb[threadIdx.x] = p.srgb[threadIdx.x];
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t px = (blockIdx.x * 4u + wave) * TW + (lane % TW);
    const uint32_t r = blockIdx.y * TH + (lane / TW); // row inside the band
    if (px >= p.W || r >= p.rows) return;
    const uint32_t py = p.row0 + r;
    const uint32_t i = r * p.W + px; // pixel index inside the band (< 2^29: byte offsets below stay 32-bit)
    // ndc.x in the streaming kernel's two-step form (16-pixel tile origin, then the column inside the tile): the same bits
    // in both kernels, so a fused streaming launch equals Lighting followed by this kernel's Sky launch bit for bit
    const float ndcx = fmaf((float)(px & ~15u), p.invW2, fmaf((float)(px & 15u), p.invW2, 0.5f * p.invW2 - 1.0f));
    const float ndcy = fmaf((float)py + 0.5f, p.invH2, -1.0f);

    if (MODE != ur::UR_MODE_LIGHTING) {
        const float vx = ndcx * p.skyInvP11, vy = -ndcy * p.skyInvP22;
        const float len = __builtin_amdgcn_sqrtf(fmaf(vx, vx, fmaf(vy, vy, 1.0f)));
        const float skyDepth = p.skyNearOverR * len; // Near / (R * unit_dir.z), unit_dir.z = 1/len
        if (skyDepth >= ld<float>(p.depth, i * 4u)) {
            F3 sky = sky_pixel(&p, vx, vy);
            // the colour is an fp32 value rounded to fp16 in a second step, as in the oracle and in the streaming kernel: kept
            // apart from the conversion, or hipcc fuses the last FMA with it (v_fma_mixlo_f16: ONE rounding, a different bit in
            // about one sky pixel in seven thousand)
            asm volatile("" : "+v"(sky.x), "+v"(sky.y), "+v"(sky.z));
            half4_t o;
            o.x = (_Float16)sky.x; o.y = (_Float16)sky.y; o.z = (_Float16)sky.z; o.w = (_Float16)1.0f;
            st_hdr_once(p.hdr, i * 8u, o);
            return;
        }
        if (MODE == ur::UR_MODE_SKY) return;
    }
    const half4_t ga = ld<half4_t>(p.A, i * 8u), gb = ld<half4_t>(p.B, i * 8u);
    const uint32_t gc = ld<uint32_t>(p.C, i * 4u);
    const half4_t d = ld<half4_t>(p.hdr, i * 8u);
    const F3 col = shade_pixel<SHADOWS>(p, srgb, p.envMipOffset, ndcx * p.invP11, -ndcy * p.invP22, ga, gb, gc);
    // blend in fp32, then ONE conversion to fp16 (not a fused mixed-precision add: see the sky branch above)
    float bx = (float)d.x + col.x, by = (float)d.y + col.y, bz = (float)d.z + col.z, bw = (float)d.w + 1.0f;
    asm volatile("" : "+v"(bx), "+v"(by), "+v"(bz), "+v"(bw));
    half4_t o;
    o.x = (_Float16)bx;
    o.y = (_Float16)by;
    o.z = (_Float16)bz;
    o.w = (_Float16)bw;
    st_hdr_once(p.hdr, i * 8u, o);
}

// register budget: waves/SIMD the kernel is compiled for (6 -> 80 VGPRs, the most that does not spill; 4 -> no cap)
template <int MODE, bool SHADOWS>
void launch_tiled(ur_ctx* ctx, const LightingParams& p)
{
    constexpr int TW = 16; // pixels per wave = 16 x 4: 128-byte G-buffer row segments and compact gather footprints
    const uint32_t tilesX = (p.W + 4 * TW - 1) / (4 * TW), tilesY = (p.rows + (64 / TW) - 1) / (64 / TW);
    if (ctx->opt.tiled_waves >= 6) /* UR_OPT_LIGHTING_TILED_WAVES */ launch_timed(ctx, lighting_kernel<MODE, SHADOWS, TW, 6>, dim3(tilesX, tilesY), dim3(256), 0u, p);
    else launch_timed(ctx, lighting_kernel<MODE, SHADOWS, TW, 4>, dim3(tilesX, tilesY), dim3(256), 0u, p);
}

} // namespace

namespace ur {

void launch_lighting_tiled(ur_ctx* ctx, const LightingParams& p, int mode, bool shadows)
{
    switch (mode) {
    case UR_MODE_LIGHTING:
        if (shadows) launch_tiled<UR_MODE_LIGHTING, true>(ctx, p); else launch_tiled<UR_MODE_LIGHTING, false>(ctx, p);
        break;
    case UR_MODE_SKY: launch_tiled<UR_MODE_SKY, false>(ctx, p); break;
    default:
        if (shadows) launch_tiled<UR_MODE_FUSED, true>(ctx, p); else launch_tiled<UR_MODE_FUSED, false>(ctx, p);
        break;
    }
}

} // namespace ur
