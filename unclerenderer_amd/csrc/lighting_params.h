// The records a Lighting launch hands to its kernels, filled in on the host (lighting_host.hip, lighting.hip) and read by both
// kernels (lighting.hip, lighting_tiled.hip), and what the three units export to one another. Not installed.
#pragma once

#include "ur_internal.h"
#include "lighting_plan.h"

#include <hip/hip_ext.h>

namespace ur {

typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));

// The launch-uniform values of the streaming kernel's loop. The hot ones stay in SGPRs across the loop; cold paths (sky
// constants, shadow slow path, partial tiles) re-read theirs from the kernarg segment when they run (fresh_params()).
struct StreamHot {
    uint32_t groups; // lighting workgroups of the launch (a workgroup with this index, if any, runs the deferred HZB tail)
    uint32_t tilesX, numTiles, tilesXMagic, W, rows, row0, irrN0, irrRowBytes; // tilesXMagic: tile / tilesX = (tile * magic) >> 32
    uint32_t staticClaims; // a workgroup's claims c < staticClaims are dealt statically (above); from there on they index the chunks the
                           // workgroup claims at run time (Balance). 0xFFFFFFFF: every tile is dealt statically
    float invW2, invH2, invP11, nInvP22;      // ray: ra = ndc.x * invP11, rb = ndc.y * nInvP22 (= -1/P22)
    float skyInvP11, nSkyInvP22, skyNearOverR2, maxMip;
    float envMaxLevel, irrNf, irrEf, irrEEf, irrOfff; // irradiance mip: N, N+2, (N+2)^2, texel offset — as floats (exact)
    float shadowWm3, shadowHm3, shadowWf;     // W-3, H-3, W as floats
    float shadowXmax, shadowYmax, shadowStrength, shadowQuarterStrength, shadowOneMinusStrength; // W - 0.5, H - 0.5, s, s/4, 1 - s
    uint32_t shadowRowBytes;
    int32_t shadowWi, shadowHi;
    const void* env;
    const float* shadow;
    void* hdr;
    float skyDepthMax;   // no sphere depth of the frame exceeds it
    // the cube's small mips in LDS: a pixel whose prefiltered level is >= cubeLdsLevel takes both footprints from the workgroup's
    // copy of the RGB row-pair entries of mips [cubeLdsLevel, last] (byte address = global byte offset - cubeLdsAdj)
    float cubeLdsLevel;  // (16.0: nothing is in LDS)
    uint32_t cubeLdsBase, cubeLdsBytes; // where those mips' entries start in the staged buffer (bytes), and how many bytes they are
    // read once per wave into VGPRs
    float R[9];          // (float3x3)ViewInverse, row-major
    float Lw[3];         // light direction, world space
    float WA[3], WB[3], WC[3]; // world-space camera ray through the pixel = ndc.x * WA + ndc.y * WB + WC
    float lightRGB[3];
    float shA[3], shB[3], shC[3], shT[3]; // (su * W - 0.5, sv * H - 0.5, depth - bias)[k] = viewZ * (ndc.x * shA[k] + ndc.y * shB[k] + shC[k]) + shT[k]
};

// Inter-workgroup balancing of a streaming launch (UR_OPT_LIGHTING_BALANCE). Equal static shares leave the mean wave idle for the
// last ~5 us of a 4K launch: XCDs differ by up to 8 % in speed on the same work (profiles/r03_wave_exit_stamps.txt). So only the tiles
// [0, staticTiles) are dealt statically; the rest is a pool of chunks of 2^dynShift consecutive tiles that workgroups claim at run
// time, one returning device-scope atomic per chunk, `lookahead` chunks ahead of use (the first `lookahead` of a workgroup are
// pre-assigned). The pool is cut into kClaimWords sub-pools, word q serving workgroups 8q .. 8q+7 - one per XCD under round-robin
// placement, which is what evens out the XCDs; any placement is correct. Per workgroup the claims are strictly sequential (the chunk
// of slot k is claimed only after slot k - 1 has been published in LDS), so its slots are valid up to the first failed claim and
// END from there on: exactly one failed claim per workgroup, after which it adds one to words[kClaimWords * stride]; the
// workgroup whose add comes last puts every word back to zero for the next launch (also under hipGraph replay).
struct Balance {
    uint32_t poolChunks;   // 0: off
    uint32_t staticTiles, dynShift, lookahead;
    unsigned long long poolMagic; // first chunk of the share of workgroups [0, x) = (x * poolMagic) >> 32 (= x * poolChunks / groups, rounded up)
    uint32_t* words;
    uint32_t* timedOut;    // host-visible (mapped, coherent): a wave gave up waiting for a slot of its workgroup (ur_ctx::claim_timed_out)
};

struct LightingParams {
    // frame
    uint32_t W, H, row0, rows;
    float invW2, invH2;  // 2/W, 2/H
    // lighting
    float invP11, invP22;
    float L[3];          // normalize(mul(float4(LightDirection,0), View).xyz)
    float R[9];          // (float3x3)ViewInverse, row-major
    float SQ[12];        // rows 0..2 of (ViewInverse * LightViewProjection), columns x,y,z,w : applied to the camera ray (a,b,1)
    float VIt[3], camPos[3]; // row 3 of ViewInverse, CameraPosition: the general path below (general != 0)
    uint32_t general;    // ViewInverse is not a rigid transform, or CameraPosition is not its origin: world vectors are formed literally
    uint32_t shadowSmall; // a shadow map below 3x3 texels: every pixel takes the bordered PCF
    float ST[4];         // row 3 of the same matrix
    float lightRGB[3];   // LightIntensity * LightColor
    float shadowStrength, shadowBias;
    float shadowW, shadowH, shadowTexelX, shadowTexelY;
    int32_t shadowWi, shadowHi;
    float maxMip;        // max(0, EnvMapMipCount-1)
    uint32_t envBase, envMips;
    uint32_t envMipOffset[16]; // in half4 texels
    uint32_t irrOffset0, irrOffset1, irrN0, irrN1; // mip pair of the irradiance lookup (level == maxMip, launch-uniform)
    float irrFrac;
    uint32_t lutW, lutH;
    // sky
    float skyRot[9];     // rows of View's 3x3: world_j = dot(skyRot[3j..3j+2], v)
    float skyInvP11, skyInvP22;
    float skyNearOverR;  // Projection[14] / World[0]
    float sunDir[3];     // normalize(LightDirection)
    float skyScatterR[3];// rayleighColor * rayleighDensity * 3/(16 pi)
    float skyMie[3];     // LightColor * mieDensity * 0.8 * (1-g^2)/(4 pi)
    float sunAttenuation;
    StreamHot hot;       // streaming kernel: everything one loop iteration reads
    Balance bal;         // ... and what its run-time tile claims read (cold)
    unsigned long long* timeline; // debug: {first entry, last exit} of this launch (ur_debug_timeline), else null
    // buffers
    const half4_t* A;
    const half4_t* B;
    const uint32_t* C;
    const float* depth;
    const float* shadow;
    const half4_t* env;
    const uint32_t* lut; // RG16 texel = one dword
    const float* srgb;
    half4_t* hdr;
};

constexpr uint32_t kLutW = 128, kLutH = 32; // streaming kernel: LUT dimensions are compile-time

// One Lighting launch. With a pair of events waiting on the context (ur_time_next_lighting) the dispatch itself carries
// them (hipExtLaunchKernelGGL): their distance is the kernel's own begin -> end interval, no event record in the queue.
template <class K, class... Args>
void launch_timed(ur_ctx* ctx, K kern, dim3 grid, dim3 block, uint32_t lds, Args... args)
{
    if (ctx->time_stop != nullptr) {
        hipExtLaunchKernelGGL(kern, grid, block, lds, ctx->stream, ctx->time_start, ctx->time_stop, 0, args...);
        ctx->time_start = ctx->time_stop = nullptr;
    } else {
        hipLaunchKernelGGL(kern, grid, block, lds, ctx->stream, args...);
    }
}

// lighting.hip: the streaming kernel on a band it accepts (launch_lighting decides); fills in the tile walk. UR_OK, or what flushing
// a chain that cannot ride returned
int launch_lighting_stream(ur_ctx* ctx, const LightingParams& p, int mode, bool shadows, bool irr_lds);
// lighting_tiled.hip: the per-tile kernel, any band and every mode
void launch_lighting_tiled(ur_ctx* ctx, const LightingParams& p, int mode, bool shadows);

} // namespace ur
