// FramePlan — what a frame does, decided once. MakeFramePlan is a pure function of the options and of the few facts the decisions rest on
// (which resources are there, world size, ring size, whether the last frame built an HZB); RenderFrame, AddPostPasses, FinishPost and
// ur_frame_render read the plan and derive nothing from the options themselves. Plain C++17, no HIP, allocates nothing:
// tests/cpp/frame_trace.cpp runs every combination of the flags through it on the CPU.
#pragma once

#include <cstdint>

struct FHotPathOptions
{
    bool bEnableIndirectDraw = true;  // RendererConfig IndirectDraw
    bool bHZBEnabled = true;
    bool bShardHZB = false;           // several ranks: build only this rank's pieces of mips 0..4 (the caller gathers and runs the tail)
    bool bDoDepthPrepass = true;      // HZB is only built when the depth prepass ran (:996)
    bool bRenderShadows = true;
    bool bSkyEnabled = true;
    bool bFuseLightingAndSky = false; // MI355X fast path: one pass, same result as Lighting followed by Sky
    bool bTonemap = false;            // next row: Tonemap pass after Sky (TAA off)
    bool bAutoExposure = false;       // with bTonemap: AutoExposure pass before Tonemap (bAutoExposureEnabled)
    bool bCas = false;                // with bTonemap: CAS pass after Tonemap (bEnableCas)
    bool bFuseTonemapCas = false;     // MI355X fast path: Tonemap + CAS in one launch (ur_tonemap_cas), CAS pass culled
    bool bTaa = false;                // with bTonemap and a history ring: TemporalAA pass after Sky (bEnableTAA); Tonemap reads its output
    bool bFuseTaaTonemap = false;     // with bTaa: TemporalAA + Tonemap in one launch (ur_temporal_aa_tonemap), TemporalAA pass culled
    bool bPostExchange = false;       // row bands: with AutoExposure / CAS, end the frame with the "Post Record" pass; FinishPost runs the post passes
    bool bTaaBand = false;            // with bTaa and bPostExchange: TemporalAA on the band too (the TAA record beside the post record); the exchange is then active without AutoExposure / CAS as well
    bool bDebugPrint = false;         // with bTonemap, CullStats and a text buffer: reset ahead of the cull, DebugPrintEnabled, and the last pass "GpuDebugPrint" (bEnableGpuDebugPrint)
    bool bAsyncCompute = false;       // MI355X: GPU Culling + Build HZB on the async-compute stream, overlapping Lighting
    bool bTimeLighting = false;       // HIP event pair around the Lighting pass only (bench roofline leg), see SetLightingTimer
    bool bGpuTiming = false;
    bool bGraphDump = false;
    bool bBarrierLogs = false;
};

// What the decisions rest on besides the options
struct FFrameFacts
{
    bool bCullInputs = false;      // IndirectArgs, ModelBounds and at least one command
    bool bHZB = false;             // an HZB with at least one mip
    bool bHZBReady = false;        // the last frame built it (FDeferredRenderer::bHZBReady)
    bool bDepthBand = false;       // Sky's depth
    bool bTonemapBand = false;     // the back buffer
    bool bDebugPrintInputs = false; // CullStats and the text buffer
    bool bShadowDraws = false, bDepthDraws = false, bGBufferDraws = false; // the raster passes' draws and targets (ur_frame_set_*_pass)
    uint32_t WorldSize = 1;
    uint32_t TaaSlotCount = 0;     // images in the TemporalAA history ring
};

struct FPassPlan
{
    bool bExists = false;  // listed in the graph (and the report)
    bool bEnabled = false; // declares usages and launches; a listed pass that is not enabled is culled
};

enum class ETaaMode : uint8_t { Off, Whole, Band };                 // Band: on the rank's band, through the post exchange
enum class ETonemapLaunch : uint8_t { Tonemap, TonemapCas, TonemapCasHalo, TaaTonemap, TaaTonemapHalo }; // ur_tonemap, ur_tonemap_cas, ur_tonemap_cas_halo, ur_temporal_aa_tonemap, ur_temporal_aa_tonemap_halo
enum class ECasLaunch : uint8_t { None, Cas, CasHalo };             // ur_cas, ur_cas_halo (None: no pass, or fused into Tonemap's launch)
enum class ECasHaloRows : uint8_t { None, Records, Resolved };      // the HDR rows around the band that CAS reads: the neighbours' post records, or the rows TemporalAA resolved

struct FFramePlan
{
    // ---- the scene passes, in order ----
    FPassPlan Cull;                 // "GPU Culling": always listed
    bool bCullUsesHZB = false;      // ConfigureHZBOcclusion: the last frame's HZB
    bool bHZBAvailable = false;     // the option and the resource (else the renderer forgets bHZBReady, :514-517)
    FPassPlan Shadow, DepthPrepass, GBuffer, BuildHZB;
    bool bShardHZB = false;
    bool bAsyncCompute = false;     // the lane of "GPU Culling" and "Build HZB"
    bool bUseShadows = false;       // Lighting reads the shadow map
    bool bFusedSky = false;         // Lighting's launch shades the sky too
    FPassPlan Sky;                  // always listed; not enabled when fused or off
    bool bTimeLighting = false;
    // ---- the post chain ----
    bool bEndsAtPostRecord = false; // the frame stops at "Post Record"; FinishPost runs the passes below from RecordRanks gathered records
    uint32_t RecordRanks = 0;
    ETaaMode Taa = ETaaMode::Off;
    bool bFuseTaaTonemap = false;
    FPassPlan TemporalAA;           // listed with any TemporalAA; not enabled when Tonemap's launch resolves
    FPassPlan AutoExposure, Tonemap, Cas;
    ETonemapLaunch TonemapLaunch = ETonemapLaunch::Tonemap;
    bool bTonemapToScratch = false; // Tonemap writes "TonemapOutput" for a CAS pass of its own, else the back buffer
    ECasLaunch CasLaunch = ECasLaunch::None;
    ECasHaloRows CasHaloRows = ECasHaloRows::None; // of whichever launch sharpens the band (ur_cas_halo, ur_tonemap_cas_halo)
    bool bTaaHaloRows = false;      // the TemporalAA launch on the band also resolves the rows around it, for CAS
    bool bDebugPrint = false;       // reset at the head of "GPU Culling", DebugPrintEnabled, and the last pass "GpuDebugPrint"
    // ---- the graph ----
    bool bGpuTiming = false, bGraphDump = false, bBarrierLogs = false;

    bool TaaOnBand() const { return Taa == ETaaMode::Band; }
};

FFramePlan MakeFramePlan(const FHotPathOptions& Options, const FFrameFacts& Facts);
