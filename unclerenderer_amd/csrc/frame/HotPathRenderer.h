// HotPathRenderer — the four hot passes of FDeferredRenderer::RenderFrame, and its post chain, wired onto the render graph.
//
// Reference wiring (Source/Render/DeferredRenderer.cpp): "GPU Culling" :508-542 (+ FRenderer::ConfigureHZBOcclusion /
// DispatchGpuCulling, Renderer.cpp:384-472), "Build HZB" :982-1212, "Lighting" :1214-1255, "Sky" :1257-1296, and optionally the
// post chain "TemporalAA" :1308-1361, "AutoExposure" :1363-1438, "Tonemap" :1440-1513, "CAS" :1515-1573, "GpuDebugPrint" :1575-1598
// (with PrepareGpuDebugPrint, :390 / Renderer.cpp:474-527, at the head of the "GPU Culling" pass). TemporalAA keeps the
// reference's history ring: FDeferredRenderer::OnFrameFenceSignaled (:2787-2799, called by FApplication::RenderFrame after every
// submission) marks the slot a frame wrote as valid, so from the second frame on the pass runs with UseHistory = 1 and Tonemap reads
// its output instead of Lighting (:1454-1459).
// Pass names, PassData structs, declared usages/states and pass order are the reference's; the execute lambdas call
// the C-ABI (include/ur_hotpath.h) instead of recording D3D12 commands. The passes between them (shadow map, depth
// prepass, G-buffer raster, post FX) are out of scope: their outputs arrive as imported textures.
#pragma once

#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "../../../include/ur_hotpath.h"
#include "../../../include/ur_raster.h"
#include "../rg/RenderGraph.h"
#include "FramePlan.h"

// Device buffers owned by the caller (the renderer that rasterised the G-buffer). States mirror the variables the
// reference keeps next to each resource (DepthBufferState, GBufferStates[], HZBState, LightingBufferState, ...).
// What a raster pass of the frame works on (ur_frame_set_*_pass + UR_FRAME_*_PASS): the draws, the target, the optional counters and the entry point's own arguments
struct FShadowPassResources { const ur_raster_draws* Draws = nullptr; float* Map = nullptr; uint32* Stats = nullptr; };                    // Map == Tables.shadow_map
struct FDepthPassResources { const ur_raster_draws* Draws = nullptr; float* Depth = nullptr; uint32* Stats = nullptr; uint32 Flags = 0; }; // Depth == DepthFull
struct FGBufferPassResources { const ur_raster_draws* Draws = nullptr; ur_gbuffer_targets Targets = {}; uint32* Stats = nullptr; uint32 Flags = 0, KeyBits = 0; }; // Targets == GBufferA/B/C, LightingBand

struct FHotPathResources
{
    uint32 Width = 0, Height = 0;      // full frame
    uint32 Row0 = 0, Rows = 0;         // screen band shaded by this rank (whole frame: 0, Height)
    // band-local images
    ur_half4* GBufferA = nullptr;
    ur_half4* GBufferB = nullptr;
    uint32* GBufferC = nullptr;
    float* DepthBand = nullptr;
    ur_half4* LightingBand = nullptr;
    uint32* TonemapBand = nullptr;    // optional: R8G8B8A8_UNORM output of the Tonemap pass for this band (the back buffer)
    uint32* TonemapScratch = nullptr; // "TonemapOutput": Tonemap's output when CAS runs as its own pass
    float* Luminance[2] = {};         // LuminanceA / B: 1x1 R32_FLOAT (CreateLuminanceResources, DeferredRenderer.cpp:2692-2712)
    std::vector<ur_half4*> TaaHistory; // TaaHistory_<i>: max(1, FrameCount) Width x Height images in Lighting's format (CreateTaaResources, :2740-2785)
    void* PostRecord = nullptr;        // post exchange (new): this band's record (ur_pack_post_record) ...
    const void* PostRecords = nullptr; // ... and every rank's, gathered in rank order (may contain PostRecord)
    void* TaaRecord = nullptr;         // TemporalAA on a band (new): this band's TAA record (ur_pack_taa_record) ...
    const void* TaaRecords = nullptr;  // ... and every rank's, gathered in rank order (may contain TaaRecord)
    ur_half4* TaaHaloRows = nullptr;   // ... and the resolved rows above / below the band (2 x Width texels; only with CAS), CAS's HDR halo rows
    // full-frame depth for the replicated HZB build, and the HZB itself
    float* DepthFull = nullptr;
    float* HZB = nullptr;
    ur_mip_desc HZBMips[UR_MAX_HZB_MIPS] = {};
    uint32 HZBMipCount = 0;
    // lighting side tables
    ur_lighting_tables Tables = {};
    // GPU-driven draw data
    ur_float4* ModelBounds = nullptr;
    void* IndirectArgs = nullptr;
    uint32 IndirectCommandCount = 0;
    uint32 InstanceIndexBase = 0;
    uint32* VisibleIndices = nullptr; // optional (new): compacted ascending list
    uint32* VisibleCount = nullptr;
    uint32* CullStats = nullptr;      // optional: [frustum-culled, occluded]
    const ur_draw_ranges* DrawRanges = nullptr; // optional (ur_frame_set_draw_ranges): compacted commands + a count per range
    const ur_cull_view* CullViews = nullptr;     // optional (ur_frame_set_cull_views + UR_FRAME_CULL_VIEWS): extra frustum-only views
    uint32 CullViewCount = 0;
    // GpuDebugPrint (ur_frame_set_debug_print + UR_FRAME_DEBUG_PRINT): the text buffer, and the font the caller supplies
    void* DebugPrintBuffer = nullptr;
    const ur_debug_glyph* DebugGlyphs = nullptr;
    uint32 DebugGlyphCount = 0;
    const uint8_t* DebugAtlas = nullptr;
    uint32 DebugAtlasWidth = 0, DebugAtlasHeight = 0;
    uint32 DebugFirstChar = 0, DebugCharCount = 0;
    // The raster passes, each there iff its Draws are: "ShadowMap" behind "GPU Culling", "DepthPrepass" in front of "Build HZB", with it "GBuffer" behind it
    FShadowPassResources ShadowPass;
    FDepthPassResources DepthPass;
    FGBufferPassResources GBufferPass;
    const ur_material* GBufferMaterials = nullptr; // ur_frame_set_gbuffer_materials: null = the untextured resolve
    uint32 GBufferMaterialCount = 0;

    uint32 DepthState = RG_STATE_DEPTH_WRITE;
    uint32 GBufferStates[3] = {RG_STATE_RENDER_TARGET, RG_STATE_RENDER_TARGET, RG_STATE_RENDER_TARGET};
    uint32 ShadowState = RG_STATE_DEPTH_WRITE;
    uint32 HZBState = RG_STATE_UNORDERED_ACCESS;
    uint32 LightingState = RG_STATE_RENDER_TARGET;
    uint32 TonemapState = RG_STATE_RENDER_TARGET;
    uint32 TonemapScratchState = RG_STATE_RENDER_TARGET;
    uint32 LuminanceStates[2] = {RG_STATE_UNORDERED_ACCESS, RG_STATE_UNORDERED_ACCESS};
    std::vector<uint32> TaaHistoryStates; // one per image, RG_STATE_UNORDERED_ACCESS at creation
    uint32 PostRecordState = RG_STATE_UNORDERED_ACCESS;
    uint32 PostRecordsState = RG_STATE_UNORDERED_ACCESS;
    uint32 TaaRecordState = RG_STATE_UNORDERED_ACCESS;
    uint32 TaaRecordsState = RG_STATE_UNORDERED_ACCESS;
    uint32 TaaHaloRowsState = RG_STATE_UNORDERED_ACCESS;
    uint32 DebugPrintState = RG_STATE_UNORDERED_ACCESS;      // GpuDebugPrintState / GpuDebugPrintStatsState (Renderer.cpp:474-527)
    uint32 DebugPrintStatsState = RG_STATE_UNORDERED_ACCESS;
    uint32 ShadowDrawsState = RG_STATE_UNORDERED_ACCESS;     // the list / ranges the cull writes and the ShadowMap pass draws from
    uint32 DepthDrawsState = RG_STATE_UNORDERED_ACCESS;      // the same of the DepthPrepass pass
};

struct FHotPathFrameConstants
{
    uint32 CullingConstants[UR_CULL_CONSTANT_DWORDS] = {}; // packed like DispatchGpuCulling; dw 40-44 are filled per frame here
    ur_scene_constants Scene = {};
    ur_sky_constants Sky = {};
    ur_tonemap_constants Tonemap = {1u, 0u, 0.9f, 2.2f}; // bTonemapEnabled, auto exposure off, TonemapExposure, TonemapGamma (DeferredRenderer.h:193-196)
    float DeltaTime = 0.0f;                               // RenderFrame's DeltaTime (AutoExposure adaptation)
    float AutoExposureKey = 0.3f, AutoExposureMin = 0.1f, AutoExposureMax = 5.0f; // RendererConfig.h:28-30
    float AutoExposureSpeedUp = 3.0f, AutoExposureSpeedDown = 1.0f;              // RendererConfig.h:31-32
    float CasSharpness = 0.5f;                                                   // RendererConfig.h:26
    float TaaHistoryWeight = 0.9f;                                               // RendererConfig.h:34
};

class FHotPathRenderer
{
public:
    FHotPathRenderer(FHIPDevice* InDevice) : Device(InDevice) {}

    // What a frame of these resources and options does (FramePlan.h), given what the renderer carries over from the last one.
    FFramePlan PlanFrame(const FHotPathResources& Res, const FHotPathOptions& Options, int WorldSize) const;
    // Builds a fresh graph, adds the passes in the reference's order and executes it. Returns UR_OK or the first
    // error a pass reported. bHZBReady carries over between frames exactly like FDeferredRenderer::bHZBReady.
    int RenderFrame(FHIPCommandContext& Cmd, FHotPathResources& Res, const FHotPathFrameConstants& Constants, const FFramePlan& FramePlan);
    int RenderFrame(FHIPCommandContext& Cmd, FHotPathResources& Res, const FHotPathFrameConstants& Constants, const FHotPathOptions& Options)
    {
        return RenderFrame(Cmd, Res, Constants, PlanFrame(Res, Options, Cmd.GetWorldSize()));
    }
    // The second half of a frame whose plan ends at "Post Record" (bPostExchange with AutoExposure, CAS or bTaaBand): [TemporalAA,] AutoExposure,
    // Tonemap and CAS on the band, from the gathered records (Res.PostRecords, Res.TaaRecords), with the frame's constants and plan. UR_EINVAL if
    // nothing is pending. A TemporalAA frame's history bookkeeping (EndTaaHistory) happens here, when the image has been written.
    int FinishPost(FHIPCommandContext& Cmd, FHotPathResources& Res);
    bool IsPostPending() const { return bPostPending; }

    // Optional hook: called right before / after the Lighting pass launches, on the pass's stream (used by the frame
    // object to bracket the dominant kernel with a HIP event pair without timing every pass).
    void SetLightingTimer(std::function<void(hipStream_t, bool /*begin*/)> Fn) { LightingTimer = std::move(Fn); }
    bool IsHZBReady() const { return bHZBReady; }
    void ResetHZB() { bHZBReady = false; }
    // luminance ping-pong of the AutoExposure pass (LuminanceWriteIndex / bLuminanceHistoryValid, DeferredRenderer.cpp:1612-1620)
    void ResetLuminanceHistory() { bLuminanceHistoryValid = false; }
    // TemporalAA history (TaaHistoryValid / TaaSampleIndex, DeferredRenderer.cpp:1602-1610): all slots invalid, sample index 0
    void ResetTaa() { std::fill(TaaHistoryValid.begin(), TaaHistoryValid.end(), false); TaaSampleIndex = 0; }
    // What a frame with TemporalAA and a ring of SlotCount images does at frame slot FrameIndex (:394-403)
    struct FTaaSlots { uint32 Read = 0, Write = 0; bool bUseHistory = false; uint32 SampleIndex = 0; };
    FTaaSlots GetTaaSlots(uint32 FrameIndex, uint32 SlotCount) const;
    const std::vector<FRenderGraph::FPassReport>& GetLastReport() const { return LastReport; }

private:
    struct FDebugPrintHandles { FRGResourceHandle Stats, Buffer; }; // null without GpuDebugPrint
    // PostPasses.cpp: the post chain of the frame's plan, on the whole frame (RenderFrame) or on the band from the records (FinishPost)
    void AddPostRecordPass(FRenderGraph& Graph, FRGResourceHandle LightingHandle, FHotPathResources& Res);
    void AddPostPasses(FRenderGraph& Graph, FRGResourceHandle LightingHandle, FHotPathResources& Res, const FHotPathFrameConstants& Constants, FDebugPrintHandles DebugPrint);
    void EndPostHistory();
    void EndTaaHistory(bool bTaaWritten, uint32 SlotCount);
    // what both halves of a frame set up alike
    void ConfigureGraph(FRenderGraph& Graph) const;
    FDebugPrintHandles ImportDebugPrint(FRenderGraph& Graph, FHotPathResources& Res) const;
    FRGResourceHandle ImportTaaHistory(FRenderGraph& Graph, FHotPathResources& Res, uint32 Index) const;
    // The frame returns the first error a pass reported; the passes behind it still run.
    void RecordPassError(int rc) { if (rc != UR_OK && PassError == UR_OK) PassError = rc; }

    FHIPDevice* Device = nullptr;
    bool bHZBReady = false;
    bool bLuminanceHistoryValid = false;
    uint32 LuminanceWriteIndex = 0;
    std::vector<bool> TaaHistoryValid; // one per ring image
    uint32 TaaSampleIndex = 0;
    FFramePlan Plan;                   // of the frame being rendered; kept for FinishPost while its post passes are pending
    FTaaSlots TaaSlots;                // that frame's TemporalAA slots (Plan.Taa != Off)
    bool bPostPending = false;         // RenderFrame stopped at "Post Record"; FinishPost runs the rest with the plan and these
    FHotPathFrameConstants PendingConstants;
    int PassError = 0;
    std::vector<FRenderGraph::FPassReport> LastReport;
    std::function<void(hipStream_t, bool)> LightingTimer;
};
