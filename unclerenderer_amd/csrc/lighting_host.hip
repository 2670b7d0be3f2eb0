// The host side of a Lighting launch: every launch uniform derived from the scene and sky constants (LightingParams, StreamHot), the
// choice between the streaming kernel (lighting.hip) and the per-tile kernel (lighting_tiled.hip). Host code only; it is compiled with
// the kernels' flags because the kernels' bits depend on the order of its fp32 and double arithmetic.

#include "lighting_params.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

void mat4_mul(const float* a, const float* b, float* o)
{
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            float s = 0.0f;
            for (int k = 0; k < 4; ++k) s += a[i * 4 + k] * b[k * 4 + j];
            o[i * 4 + j] = s;
        }
}

} // namespace

namespace ur {

int launch_lighting(ur_ctx* ctx, const ur_scene_constants* S, const ur_sky_constants* K, const ur_half4* A, const ur_half4* B,
                    const uint32_t* C, const float* depth, const ur_lighting_tables* T, ur_half4* hdr, uint32_t w, uint32_t h,
                    uint32_t row0, uint32_t rows, int mode)
{
    LightingParams p{};
    p.W = w; p.H = h; p.row0 = row0; p.rows = rows;
    p.invW2 = 2.0f / (float)w; p.invH2 = 2.0f / (float)h;
    p.A = reinterpret_cast<const half4_t*>(A);
    p.B = reinterpret_cast<const half4_t*>(B);
    p.C = C; p.depth = depth;
    p.hdr = reinterpret_cast<half4_t*>(hdr);
    p.srgb = ctx->srgb_table;
    bool shadows = false;
    float ortho_err = 0.0f; // departure of (float3x3)ViewInverse from an orthonormal matrix
    CubeLayout cube{};      // the staged cube (lighting_plan.h); no mips in a sky-only launch
    if (mode != UR_MODE_SKY) {
        // the view matrix must be rigid: rows of (float3x3)ViewInverse orthonormal
        const float* VI = S->ViewInverse;
        for (int i = 0; i < 3; ++i)
            for (int j = i; j < 3; ++j) {
                const float d = VI[i * 4] * VI[j * 4] + VI[i * 4 + 1] * VI[j * 4 + 1] + VI[i * 4 + 2] * VI[j * 4 + 2];
                ortho_err = std::fmax(ortho_err, std::fabs(d - (i == j ? 1.0f : 0.0f)));
            }
        // Every camera the reference builds is rigid with CameraPosition as its origin (RendererUtils.cpp: View from LookTo, its
        // inverse, the same position). Anything else takes the per-tile kernel's literal world-space vectors.
        float cam_err = 0.0f;
        for (int j = 0; j < 3; ++j) {
            p.VIt[j] = VI[12 + j]; p.camPos[j] = S->CameraPosition[j];
            cam_err = std::fmax(cam_err, std::fabs(VI[12 + j] - S->CameraPosition[j]) / std::fmax(1.0f, std::fabs(VI[12 + j])));
        }
        p.general = (!(ortho_err <= 1e-3f) || !(cam_err <= 1e-5f)) ? 1u : 0u;
        p.invP11 = 1.0f / S->Projection[0];
        p.invP22 = 1.0f / S->Projection[5];
        const float* V = S->View;
        const float* LD = S->LightDirection;
        float l[3];
        for (int j = 0; j < 3; ++j) l[j] = (LD[0] * V[j] + LD[1] * V[4 + j]) + LD[2] * V[8 + j];
        const float lr = 1.0f / std::sqrt((l[0] * l[0] + l[1] * l[1]) + l[2] * l[2]);
        for (int j = 0; j < 3; ++j) p.L[j] = l[j] * lr;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) p.R[i * 3 + j] = VI[i * 4 + j];
        float SM[16];
        mat4_mul(S->ViewInverse, S->LightViewProjection, SM);
        std::memcpy(p.SQ, SM, sizeof(p.SQ));
        std::memcpy(p.ST, SM + 12, sizeof(p.ST));
        for (int j = 0; j < 3; ++j) p.lightRGB[j] = S->LightIntensity * S->LightColor[j];
        p.shadowStrength = S->ShadowStrength;
        p.shadowBias = S->ShadowBias;
        p.shadowW = S->ShadowMapSize[0]; p.shadowH = S->ShadowMapSize[1];
        p.shadowWi = (int32_t)S->ShadowMapSize[0]; p.shadowHi = (int32_t)S->ShadowMapSize[1];
        p.shadowTexelX = 1.0f / S->ShadowMapSize[0]; p.shadowTexelY = 1.0f / S->ShadowMapSize[1];
        p.shadow = T->shadow_map;
        shadows = p.shadowStrength > 0.0f;
        p.shadowSmall = (shadows && (p.shadowWi < 3 || p.shadowHi < 3)) ? 1u : 0u; // per-tile kernel, every tap through the bordered PCF
        if (shadows && (p.shadow == nullptr || p.shadowWi <= 0 || p.shadowHi <= 0)) {
            set_error("ShadowStrength > 0 but no shadow map / ShadowMapSize");
            return UR_EINVAL;
        }
        p.maxMip = std::fmax(0.0f, S->EnvMapMipCount - 1.0f);
        p.envBase = T->env_base_size; p.envMips = T->env_mip_count;
        if (p.envMips == 0 || p.envMips > 16 || p.envBase == 0 || T->env_cube == nullptr || T->brdf_lut_rg16 == nullptr ||
            T->lut_width == 0 || T->lut_height == 0) {
            set_error("bad lighting tables");
            return UR_EINVAL;
        }
        cube = cube_layout(p.envBase, p.envMips);
        if (T->env_cube_texels != cube.texels) {
            set_error("ur_lighting_tables.env_cube_texels = %llu, but this version's ur_stage_env_cube writes %llu texels for a %u^2 cube of %u mips: "
                      "the buffer was sized or staged for another layout", (unsigned long long)T->env_cube_texels,
                      (unsigned long long)cube.texels, p.envBase, p.envMips);
            return UR_EINVAL;
        }
        for (uint32_t m = 0; m < p.envMips; ++m) p.envMipOffset[m] = (uint32_t)cube.bordered[m];
        {
            const float l = std::fmin(std::fmax(p.maxMip, 0.0f), (float)(p.envMips - 1u));
            const uint32_t m0 = (uint32_t)l, m1 = m0 + 1u < p.envMips ? m0 + 1u : p.envMips - 1u;
            p.irrFrac = l - (float)m0;
            p.irrOffset0 = p.envMipOffset[m0]; p.irrOffset1 = p.envMipOffset[m1];
            p.irrN0 = cube.size(m0);
            p.irrN1 = cube.size(m1);
        }
        p.env = reinterpret_cast<const half4_t*>(T->env_cube);
        p.lut = reinterpret_cast<const uint32_t*>(T->brdf_lut_rg16);
        p.lutW = T->lut_width; p.lutH = T->lut_height;
    }
    if (mode != UR_MODE_LIGHTING) {
        for (int j = 0; j < 3; ++j)
            for (int i = 0; i < 3; ++i) p.skyRot[j * 3 + i] = K->View[j * 4 + i];
        p.skyInvP11 = 1.0f / K->Projection[0];
        p.skyInvP22 = 1.0f / K->Projection[5];
        p.skyNearOverR = K->Projection[14] / K->World[0];
        const float* LD = K->LightDirection;
        const float lr = 1.0f / std::sqrt((LD[0] * LD[0] + LD[1] * LD[1]) + LD[2] * LD[2]);
        for (int j = 0; j < 3; ++j) p.sunDir[j] = LD[j] * lr;
        const float viewHeight = std::fmax(0.0f, K->CameraPosition[1]);
        const float rayleighDensity = std::exp(-viewHeight / 8000.0f), mieDensity = std::exp(-viewHeight / 1200.0f);
        const float rayleighColor[3] = {0.650f, 0.570f, 0.475f};
        const float g2 = 0.76f * 0.76f;
        for (int j = 0; j < 3; ++j) {
            p.skyScatterR[j] = rayleighColor[j] * rayleighDensity * (3.0f / (16.0f * 3.14159265f));
            p.skyMie[j] = K->LightColor[j] * mieDensity * 0.8f * ((1.0f - g2) / (4.0f * 3.14159265f));
        }
        const float cosSunUp = p.sunDir[1];
        p.sunAttenuation = std::fmin(std::fmax(std::exp(-std::fmax(0.0f, 1.0f - cosSunUp) * 2.0f), 0.0f), 1.0f);
    }
    if ((uint64_t)w * rows == 0) return UR_OK;
    if ((uint64_t)w * rows >= (1ull << 29)) {
        set_error("band of %u x %u pixels exceeds the 2^29-pixel limit of one launch", w, rows);
        return UR_EUNSUPPORTED;
    }
    // ---- streaming kernel when the band is a whole number of 16-pixel tile columns; the per-tile kernel otherwise -----------
    const int use_stream = ctx->opt.lighting_stream; // UR_OPT_LIGHTING_STREAM
    bool streamed = false;
    // (the streaming kernel addresses the staged cube's RGB row-pair section in fp32 BYTE offsets, which must stay below 2^24: base
    // sizes up to 256; bigger cubes take the per-tile kernel)
    const uint64_t n_tiles = (uint64_t)(w / 16u) * ((rows + 3u) / 4u);
    const uint64_t magic_err = w >= 16u ? ((1ull << 32) / (w / 16u) + 1ull) * (w / 16u) - (1ull << 32) : 0;
    // (the streaming kernel takes its dot products in world space: the rotation must be orthonormal to rounding; its tile DMA
    // moves 16 bytes per lane: 16-byte-aligned band buffers)
    const uintptr_t align_bits = reinterpret_cast<uintptr_t>(p.A) | reinterpret_cast<uintptr_t>(p.B) | reinterpret_cast<uintptr_t>(p.C) |
                                 reinterpret_cast<uintptr_t>(p.depth) | reinterpret_cast<uintptr_t>(p.hdr);
    if (use_stream && mode != UR_MODE_SKY && (align_bits & 15u) == 0 && ortho_err <= 1e-5f && p.general == 0u && p.shadowSmall == 0u && w % 16u == 0 && w >= 32u /* the magic of one tile per row does not fit 32 bits */ && magic_err * n_tiles < (1ull << 32) && p.lutW == kLutW && p.lutH == kLutH && p.irrFrac == 0.0f && cube.bytes < (1ull << 24)) {
        bool ok = true;
        StreamHot& h = p.hot;
        if (shadows) {
            // orthographic light (BuildDirectionalLightViewProjection, RendererUtils.cpp:1117-1137): clip.w == 1, so
            // su * W - 0.5, sv * H - 0.5 and depth - bias are affine in viewZ * (ra, rb, 1)
            ok = p.SQ[3] == 0.0f && p.SQ[7] == 0.0f && p.SQ[11] == 0.0f && p.ST[3] == 1.0f;
            const double hw = 0.5 * p.shadowW, hh = 0.5 * p.shadowH;
            const double sc[3] = {hw, -hh, 1.0}; // clip -> (texel x, texel y, depth)
            for (int k = 0; k < 3; ++k) {
                // clip[k] = viewZ * (ra * SQ[k] + rb * SQ[4 + k] + SQ[8 + k]) + ST[k], ra = ndc.x / P11, rb = -ndc.y / P22
                h.shA[k] = (float)(p.SQ[k] * sc[k] * p.invP11);
                h.shB[k] = (float)(p.SQ[4 + k] * sc[k] * -(double)p.invP22);
                h.shC[k] = (float)(p.SQ[8 + k] * sc[k]);
            }
            h.shT[0] = (float)(p.ST[0] * hw + hw - 0.5);
            h.shT[1] = (float)(p.ST[1] * -hh + hh - 0.5);
            h.shT[2] = p.ST[2] - p.shadowBias;
            h.shadowXmax = p.shadowW - 0.5f;
            h.shadowYmax = p.shadowH - 0.5f;
            h.shadowWi = p.shadowWi; h.shadowHi = p.shadowHi;
            h.shadowWm3 = (float)(p.shadowWi - 3); h.shadowHm3 = (float)(p.shadowHi - 3); h.shadowWf = (float)p.shadowWi;
            h.shadowRowBytes = (uint32_t)p.shadowWi * 4u;
            h.shadowStrength = p.shadowStrength;
            h.shadowQuarterStrength = 0.25f * p.shadowStrength;
            h.shadowOneMinusStrength = 1.0f - p.shadowStrength;
            h.shadow = p.shadow;
            ok = ok && (uint64_t)p.shadowWi * (uint64_t)p.shadowHi < (1ull << 24); // texel indices are computed in fp32 (exact below 2^24)
        }
        if (ok) {
            h.W = p.W; h.rows = p.rows; h.row0 = p.row0;
            h.invW2 = p.invW2; h.invH2 = p.invH2;
            h.invP11 = p.invP11; h.nInvP22 = -p.invP22;
            h.skyInvP11 = p.skyInvP11; h.nSkyInvP22 = -p.skyInvP22;
            h.skyNearOverR2 = p.skyNearOverR * p.skyNearOverR;
            h.maxMip = p.maxMip;
            h.envMaxLevel = (float)(p.envMips - 1u);
            const uint32_t iE = p.irrN0 + 2u;
            h.irrN0 = p.irrN0; h.irrNf = (float)p.irrN0; h.irrEf = (float)iE; h.irrEEf = (float)(iE * iE);
            if (p.irrN0 <= 2u) { h.irrEf = (float)(p.irrN0 + 1u); h.irrEEf = (float)((p.irrN0 + 1u) * (p.irrN0 + 1u)); } // LDS table of cells
            h.irrOfff = (float)p.irrOffset0; h.irrRowBytes = iE * 8u;
            h.env = p.env; h.hdr = p.hdr;
            for (int k = 0; k < 9; ++k) h.R[k] = p.R[k];
            for (int k = 0; k < 3; ++k) {
                h.Lw[k] = (p.L[0] * p.R[k] + p.L[1] * p.R[3 + k]) + p.L[2] * p.R[6 + k]; // view-space L rotated like every other vector
                h.WA[k] = p.invP11 * p.R[k];
                h.WB[k] = -p.invP22 * p.R[3 + k];
                h.WC[k] = p.R[6 + k];
                h.lightRGB[k] = p.lightRGB[k];
            }
            {   // largest sphere depth of the frame: (Near/R) * |(vx, vy, 1)| at the ndc corner, with a margin of a few ulp
                const double vx = p.skyInvP11, vy = p.skyInvP22;
                h.skyDepthMax = (float)(p.skyNearOverR * std::sqrt(vx * vx + vy * vy + 1.0) * (1.0 + 1e-5));
            }
            {   // the cube's smallest mips whose RGB row-pair entries fit the workgroup's LDS copy (the shipped cube: mips 4..8)
                const uint32_t first = cube_first_mip_within(cube, kLdsCubeBytes);
                h.cubeLdsLevel = first < p.envMips ? (float)first : 16.0f;
                h.cubeLdsBase = (uint32_t)cube.pairs[first];
                h.cubeLdsBytes = (uint32_t)(cube.bytes - cube.pairs[first]);
            }
            streamed = true;
            const int rc = launch_lighting_stream(ctx, p, mode, shadows, p.irrN0 <= 2u);
            if (rc != UR_OK) return rc;
        }
    }
    if (!streamed) {
        // the per-tile kernel cannot carry a held-back HZB tail: it goes out on its own, in front (ur_defer_hzb_tail's contract:
        // every Lighting launch on the context completes the chain)
        const int frc = flush_hzb_tail(ctx);
        if (frc != UR_OK) return frc;
        launch_lighting_tiled(ctx, p, mode, shadows);
    }
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

} // namespace ur
