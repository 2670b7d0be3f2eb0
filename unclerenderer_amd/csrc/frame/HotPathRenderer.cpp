// HotPathRenderer.cpp — RenderFrame: the scene passes of the hot path wired onto FRenderGraph (see HotPathRenderer.h for reference citations).
// The post chain behind them is PostPasses.cpp, the C face FrameApi.cpp; what a frame does is decided in FramePlan.cpp.

#include "HotPathRenderer.h"

#include <cstring>

#include "../ur_checks.h"

FFramePlan FHotPathRenderer::PlanFrame(const FHotPathResources& Res, const FHotPathOptions& Options, int WorldSize) const
{
    FFrameFacts F;
    F.bCullInputs = Res.IndirectArgs && Res.ModelBounds && Res.IndirectCommandCount != 0;
    F.bHZB = Res.HZB != nullptr && Res.HZBMipCount != 0;
    F.bHZBReady = bHZBReady;
    F.bDepthBand = Res.DepthBand != nullptr;
    F.bTonemapBand = Res.TonemapBand != nullptr;
    F.bDebugPrintInputs = Res.CullStats && Res.DebugPrintBuffer;
    F.bShadowDraws = Res.ShadowPass.Draws != nullptr && Res.ShadowPass.Map != nullptr;
    F.bDepthDraws = Res.DepthPass.Draws != nullptr && Res.DepthPass.Depth != nullptr;
    F.bGBufferDraws = Res.GBufferPass.Draws != nullptr;
    F.WorldSize = static_cast<uint32>(WorldSize);
    F.TaaSlotCount = static_cast<uint32>(Res.TaaHistory.size());
    return MakeFramePlan(Options, F);
}

void FHotPathRenderer::ConfigureGraph(FRenderGraph& Graph) const
{
    Graph.SetDevice(Device);
    Graph.SetGpuTimingEnabled(Plan.bGpuTiming);
    Graph.SetGraphDumpEnabled(Plan.bGraphDump);
    Graph.SetResourceLifetimeLogging(Plan.bGraphDump);
    Graph.SetBarrierLoggingEnabled(Plan.bBarrierLogs);
}

// GpuDebugPrint: the cull's two counters and the text buffer, written by "GPU Culling" (reset, then counted) and read by the last pass.
// Behind the exchange the counters are the ones the caller has summed over the ranks meanwhile (dist.allreduce_cull_stats).
FHotPathRenderer::FDebugPrintHandles FHotPathRenderer::ImportDebugPrint(FRenderGraph& Graph, FHotPathResources& Res) const
{
    if (!Plan.bDebugPrint) return {};
    return {Graph.ImportTexture("DebugPrintStats", Res.CullStats, &Res.DebugPrintStatsState, {2, 1, RG_FORMAT_UNKNOWN}),
            Graph.ImportTexture("DebugPrintBuffer", Res.DebugPrintBuffer, &Res.DebugPrintState, {static_cast<uint32>(ur_debug_print_buffer_bytes() / 4u), 1, RG_FORMAT_UNKNOWN})};
}

int FHotPathRenderer::RenderFrame(FHIPCommandContext& Cmd, FHotPathResources& Res, const FHotPathFrameConstants& Constants, const FFramePlan& FramePlan)
{
    // Every call must reach the bookkeeping after Graph.Execute at the end: it hands the luminance history to the next frame
    // (valid and flipped after an AutoExposure pass that ran, invalid after any other frame, :1612-1620). Errors of passes are
    // collected in PassError rather than returned early; an early return added above Execute must do that bookkeeping too.
    PassError = UR_OK;
    if (bPostPending) { // the last frame's post passes never ran: neither its AutoExposure nor its TemporalAA did
        bPostPending = false;
        bLuminanceHistoryValid = false;
        ResetTaa();
    }
    Plan = FramePlan;
    FRenderGraph Graph;
    ConfigureGraph(Graph);

    const uint32 HZBWidth = Res.HZBMipCount ? Res.HZBMips[0].width : 0, HZBHeight = Res.HZBMipCount ? Res.HZBMips[0].height : 0;

    // External resources, imported with a pointer to the owner's state variable (DeferredRenderer.cpp:437-506).
    const FRGResourceHandle DepthHandle = Graph.ImportTexture("Depth", Res.DepthFull, &Res.DepthState, {Res.Width, Res.Height, RG_FORMAT_R32_FLOAT});
    FRGResourceHandle GBufferHandles[3];
    GBufferHandles[0] = Graph.ImportTexture("GBufferA", Res.GBufferA, &Res.GBufferStates[0], {Res.Width, Res.Rows, RG_FORMAT_R16G16B16A16_FLOAT});
    GBufferHandles[1] = Graph.ImportTexture("GBufferB", Res.GBufferB, &Res.GBufferStates[1], {Res.Width, Res.Rows, RG_FORMAT_R16G16B16A16_FLOAT});
    GBufferHandles[2] = Graph.ImportTexture("GBufferC", Res.GBufferC, &Res.GBufferStates[2], {Res.Width, Res.Rows, RG_FORMAT_R8G8B8A8_UNORM_SRGB});
    const FRGResourceHandle ShadowHandle = Graph.ImportTexture("ShadowMap", const_cast<float*>(Res.Tables.shadow_map), &Res.ShadowState,
                                                               {static_cast<uint32>(Constants.Scene.ShadowMapSize[0]), static_cast<uint32>(Constants.Scene.ShadowMapSize[1]), RG_FORMAT_R32_FLOAT});
    const FRGResourceHandle LightingHandle = Graph.ImportTexture("Lighting", Res.LightingBand, &Res.LightingState, {Res.Width, Res.Rows, RG_FORMAT_R16G16B16A16_FLOAT});
    const FRGResourceHandle HZBHandle = Graph.ImportTexture("HZB", Res.HZB, &Res.HZBState, {HZBWidth, HZBHeight, RG_FORMAT_R32_FLOAT});

    // TemporalAA (:394-403): the slots of this frame slot and whether the image read was written by a frame that completed
    const uint32 TaaSlotCount = static_cast<uint32>(Res.TaaHistory.size());
    if (Res.TaaHistoryStates.size() != Res.TaaHistory.size()) Res.TaaHistoryStates.assign(Res.TaaHistory.size(), RG_STATE_UNORDERED_ACCESS);
    TaaSlots = Plan.Taa != ETaaMode::Off ? GetTaaSlots(Cmd.GetCurrentFrameIndex(), TaaSlotCount) : FTaaSlots{};

    const FDebugPrintHandles DebugPrint = ImportDebugPrint(Graph, Res);

    // What a raster pass draws from, written by this frame's cull when it runs: its list, else the commands of its ranges or its own
    const auto ImportDraws = [&Graph](const char* Name, const ur_raster_draws& D, uint32* State) {
        const void* Draws = D.visible_idx ? static_cast<const void*>(D.visible_idx) : ur::raster_commands(D);
        return Graph.ImportTexture(Name, const_cast<void*>(Draws), State, {D.command_count, 1, RG_FORMAT_UNKNOWN});
    };
    // ShadowMap: the light view's draws; DepthPrepass: the camera's
    const FRGResourceHandle ShadowDrawsHandle = Plan.Shadow.bExists ? ImportDraws("ShadowDraws", *Res.ShadowPass.Draws, &Res.ShadowDrawsState) : FRGResourceHandle{};
    const FRGResourceHandle DepthDrawsHandle = Plan.DepthPrepass.bExists ? ImportDraws("DepthDraws", *Res.DepthPass.Draws, &Res.DepthDrawsState) : FRGResourceHandle{};

    if (!Plan.bHZBAvailable) bHZBReady = false; // :514-517

    // ---- GPU Culling (first pass of the frame; uses LAST frame's HZB with the current camera) --------------------
    struct FGpuCullingPassData
    {
        uint32 Constants[UR_CULL_CONSTANT_DWORDS] = {};
    };
    Graph.AddPass<FGpuCullingPassData>("GPU Culling", [&](FGpuCullingPassData& Data, FRGPassBuilder& Builder)
    {
        std::memcpy(Data.Constants, Constants.CullingConstants, sizeof(Data.Constants));
        Data.Constants[40] = Res.IndirectCommandCount;
        Data.Constants[41] = Plan.bCullUsesHZB ? 1u : 0u;
        Data.Constants[42] = Res.HZBMipCount;
        Data.Constants[43] = HZBWidth;
        Data.Constants[44] = HZBHeight;
        if (Plan.bDebugPrint) { // PrepareGpuDebugPrint (:390) and DebugPrintEnabled: the counters are zeroed, then counted, on this pass's stream
            Data.Constants[45] = 1u;
            Builder.WriteTexture(DebugPrint.Stats, RG_STATE_UNORDERED_ACCESS);
            Builder.WriteTexture(DebugPrint.Buffer, RG_STATE_UNORDERED_ACCESS);
        }
        if (Plan.Cull.bEnabled) {
            if (Plan.bCullUsesHZB) Builder.ReadTexture(HZBHandle, RG_STATE_NON_PIXEL_SHADER_RESOURCE);
            if (Plan.Shadow.bEnabled) Builder.WriteTexture(ShadowDrawsHandle, RG_STATE_UNORDERED_ACCESS);     // the light view's list / ranges
            if (Plan.DepthPrepass.bEnabled) Builder.WriteTexture(DepthDrawsHandle, RG_STATE_UNORDERED_ACCESS); // the camera's list / ranges
            Builder.KeepAlive();
            // Neither visibility pass shares a resource with Lighting/Sky inside a frame (the cull reads LAST frame's
            // HZB), so both can run beside the VALU-bound lighting kernel on the second stream.
            if (Plan.bAsyncCompute) Builder.AsyncCompute();
        }
    }, [this, &Res](const FGpuCullingPassData& Data, FHIPCommandContext& Cmd)
    {
        if (Plan.bDebugPrint) RecordPassError(ur_debug_print_reset(Cmd.GetContext(), Res.DebugPrintBuffer, Res.CullStats));
        if (!Plan.Cull.bEnabled) return;
        // DispatchGpuCulling (Renderer.cpp:394-472): the UAV / INDIRECT_ARGUMENT transitions are stream order here.
        // With draw ranges the same call also places the visible commands of each range and writes its count (ur_cull_indirect_args_draws).
        // With extra views (UR_FRAME_CULL_VIEWS) the same launch also tests them (ur_cull_indirect_args_views): the DepthPrepass / ShadowMap
        // visibility of UpdateCullingVisibility (DeferredRenderer.cpp:3803-3812) and the shadow pass (:583-591).
        // (No views: views = NULL, exactly ur_cull_indirect_args_draws.)
        RecordPassError(ur_cull_indirect_args_views(Cmd.GetContext(), Data.Constants, Res.ModelBounds, Res.HZB, Res.HZBMips, Res.IndirectArgs, Res.CullStats,
                                                    Res.VisibleIndices, Res.VisibleCount, Res.InstanceIndexBase, Res.DrawRanges,
                                                    Res.CullViewCount != 0 ? Res.CullViews : nullptr, Res.CullViewCount));
    });

    // ---- ShadowMap (:551-633): the light view's draws, depth only, into the map Lighting samples -----------------------
    struct FShadowPassData
    {
        float LightViewProjection[16] = {};
        uint32 Width = 0, Height = 0;
    };
    if (Plan.Shadow.bExists) {
        Graph.AddPass<FShadowPassData>("ShadowMap", [&](FShadowPassData& Data, FRGPassBuilder& Builder)
        {
            std::memcpy(Data.LightViewProjection, Constants.Scene.LightViewProjection, sizeof(Data.LightViewProjection));
            Data.Width = static_cast<uint32>(Constants.Scene.ShadowMapSize[0]);
            Data.Height = static_cast<uint32>(Constants.Scene.ShadowMapSize[1]);
            if (Plan.Shadow.bEnabled) {
                if (Plan.Cull.bEnabled) Builder.ReadTexture(ShadowDrawsHandle, RG_STATE_INDIRECT_ARGUMENT); // (on the async lane: the wait on the cull)
                Builder.WriteTexture(ShadowHandle, RG_STATE_DEPTH_WRITE);
            }
        }, [this, &Res](const FShadowPassData& Data, FHIPCommandContext& Cmd)
        {
            if (!Plan.Shadow.bEnabled) return;
            // ClearDepth(1.0) and the draws of :571-631, on the stream the pass runs on (the main one: it is not an async-compute pass)
            RecordPassError(ur_shadow_map(Cmd.GetContext(), Data.LightViewProjection, Res.ShadowPass.Draws, Res.ShadowPass.Map, Data.Width, Data.Height, Res.ShadowPass.Stats));
        });
    }

    // ---- DepthPrepass (:635-718): the camera's draws, depth only, into the buffer Build HZB reads ---------------------------------
    struct FDepthPrepassData
    {
        float View[16] = {}, Projection[16] = {};
        uint32 Width = 0, Height = 0, Flags = 0;
    };
    if (Plan.DepthPrepass.bExists) {
        Graph.AddPass<FDepthPrepassData>("DepthPrepass", [&](FDepthPrepassData& Data, FRGPassBuilder& Builder)
        {
            std::memcpy(Data.View, Constants.Scene.View, sizeof(Data.View));
            std::memcpy(Data.Projection, Constants.Scene.Projection, sizeof(Data.Projection));
            Data.Width = Res.Width;
            Data.Height = Res.Height;
            Data.Flags = Res.DepthPass.Flags;
            if (Plan.DepthPrepass.bEnabled) {
                if (Plan.Cull.bEnabled) Builder.ReadTexture(DepthDrawsHandle, RG_STATE_INDIRECT_ARGUMENT); // (on the async lane: the wait on the cull)
                Builder.WriteTexture(DepthHandle, RG_STATE_DEPTH_WRITE);
            }
        }, [this, &Res](const FDepthPrepassData& Data, FHIPCommandContext& Cmd)
        {
            if (!Plan.DepthPrepass.bEnabled) return;
            // ClearDepth(0.0) and the draws of :655-716, on the main stream: Build HZB (on the async lane: behind a wait) reads what it wrote
            RecordPassError(ur_depth_prepass(Cmd.GetContext(), Data.View, Data.Projection, Res.DepthPass.Draws, Res.DepthPass.Depth, Data.Width, Data.Height, Data.Flags, Res.DepthPass.Stats));
        });
    }

    // ---- GBuffer (:720-865, with ObjectId :867-980 as its optional fifth output): the base pass against the prepass' depth ------------
    struct FGBufferPassData
    {
        float View[16] = {}, Projection[16] = {};
    };
    if (Plan.GBuffer.bExists) {
        Graph.AddPass<FGBufferPassData>("GBuffer", [&](FGBufferPassData& Data, FRGPassBuilder& Builder)
        {
            std::memcpy(Data.View, Constants.Scene.View, sizeof(Data.View));
            std::memcpy(Data.Projection, Constants.Scene.Projection, sizeof(Data.Projection));
            if (Plan.GBuffer.bEnabled) { // (the base pass tests against the prepass' depth: without it the pass is listed and culled)
                Builder.ReadTexture(DepthHandle, RG_STATE_DEPTH_READ); // (main stream, behind DepthPrepass: the cull's lists and ranges are complete)
                Builder.WriteTexture(GBufferHandles[0], RG_STATE_RENDER_TARGET);
                Builder.WriteTexture(GBufferHandles[1], RG_STATE_RENDER_TARGET);
                Builder.WriteTexture(GBufferHandles[2], RG_STATE_RENDER_TARGET);
                Builder.WriteTexture(LightingHandle, RG_STATE_RENDER_TARGET); // SceneColor: (emissive, 1), what Lighting adds to
            }
        }, [this, &Res](const FGBufferPassData& Data, FHIPCommandContext& Cmd)
        {
            if (!Plan.GBuffer.bEnabled) return;
            // (a null table is ur_gbuffer_pass)
            RecordPassError(ur_gbuffer_pass_materials(Cmd.GetContext(), Data.View, Data.Projection, Res.GBufferPass.Draws, Res.DepthPass.Depth, &Res.GBufferPass.Targets,
                                                      Res.Width, Res.Height, Res.Row0, Res.Rows, Res.DepthPass.Flags, Res.GBufferPass.KeyBits, Res.GBufferPass.Stats,
                                                      Res.GBufferMaterials, Res.GBufferMaterialCount));
        });
    }

    // ---- Build HZB (after the G-buffer pass; only with HZB and depth prepass enabled, :996) ------------------------
    struct FHZBPassData
    {
        uint32 Width = 0, Height = 0, MipCount = 0, SourceWidth = 0, SourceHeight = 0;
    };
    if (Plan.BuildHZB.bExists) {
        Graph.AddPass<FHZBPassData>("Build HZB", [&](FHZBPassData& Data, FRGPassBuilder& Builder)
        {
            Data.Width = HZBWidth;
            Data.Height = HZBHeight;
            Data.MipCount = Res.HZBMipCount;
            Data.SourceWidth = Res.Width;
            Data.SourceHeight = Res.Height;
            Builder.ReadTexture(DepthHandle, RG_STATE_NON_PIXEL_SHADER_RESOURCE);
            Builder.WriteTexture(HZBHandle, RG_STATE_UNORDERED_ACCESS);
            if (Plan.bAsyncCompute) Builder.AsyncCompute();
        }, [this, &Res](const FHZBPassData& Data, FHIPCommandContext& Cmd)
        {
            if (Data.MipCount == 0) return;
            int rc;
            if (Plan.bShardHZB) { // this rank's piece rows of the wide launch; the ranks' exchange and the tail are the caller's (it holds the communicator)
                uint32_t Row0 = 0, Rows = 0;
                rc = ur_hzb_band_pieces(Data.SourceHeight, static_cast<uint32_t>(Cmd.GetWorldSize()), static_cast<uint32_t>(Cmd.GetRank()), &Row0, &Rows);
                if (rc == UR_OK) rc = ur_build_hzb_band(Cmd.GetContext(), Res.DepthFull, Data.SourceWidth, Data.SourceHeight, Res.HZB, Res.HZBMips, Data.MipCount, Row0, Rows);
            } else {
                rc = ur_build_hzb(Cmd.GetContext(), Res.DepthFull, Data.SourceWidth, Data.SourceHeight, Res.HZB, Res.HZBMips, Data.MipCount);
            }
            RecordPassError(rc);
            Res.HZBState = RG_STATE_NON_PIXEL_SHADER_RESOURCE; // :1209
            if (rc == UR_OK) bHZBReady = true;                  // :1210
        });
    }

    // ---- Lighting (fullscreen, additive) --------------------------------------------------------------------------
    struct FLightingPassData
    {
        ur_scene_constants Scene;
        ur_sky_constants Sky;
    };
    Graph.AddPass<FLightingPassData>("Lighting", [&](FLightingPassData& Data, FRGPassBuilder& Builder)
    {
        Data.Scene = Constants.Scene;
        Data.Sky = Constants.Sky;
        if (!Plan.bUseShadows) Data.Scene.ShadowStrength = 0.0f; // bShadowsEnabled ? ShadowStrength : 0 (:3777)
        Builder.ReadTexture(GBufferHandles[0], RG_STATE_PIXEL_SHADER_RESOURCE);
        Builder.ReadTexture(GBufferHandles[1], RG_STATE_PIXEL_SHADER_RESOURCE);
        Builder.ReadTexture(GBufferHandles[2], RG_STATE_PIXEL_SHADER_RESOURCE);
        if (Plan.bUseShadows) Builder.ReadTexture(ShadowHandle, RG_STATE_PIXEL_SHADER_RESOURCE);
        if (Plan.bFusedSky) Builder.ReadTexture(DepthHandle, RG_STATE_DEPTH_READ);
        Builder.WriteTexture(LightingHandle, RG_STATE_RENDER_TARGET);
    }, [this, &Res](const FLightingPassData& Data, FHIPCommandContext& Cmd)
    {
        const bool bTimed = Plan.bTimeLighting && LightingTimer;
        if (bTimed) LightingTimer(Cmd.GetStream(), true);
        int rc;
        if (Plan.bFusedSky)
            rc = ur_deferred_lighting_sky(Cmd.GetContext(), &Data.Scene, &Data.Sky, Res.GBufferA, Res.GBufferB, Res.GBufferC, Res.DepthBand, &Res.Tables,
                                          Res.LightingBand, Res.Width, Res.Height, Res.Row0, Res.Rows);
        else
            rc = ur_deferred_lighting(Cmd.GetContext(), &Data.Scene, Res.GBufferA, Res.GBufferB, Res.GBufferC, &Res.Tables, Res.LightingBand, Res.Width,
                                      Res.Height, Res.Row0, Res.Rows);
        if (bTimed) LightingTimer(Cmd.GetStream(), false);
        RecordPassError(rc);
    });

    // ---- Sky --------------------------------------------------------------------------------------------------------
    struct FSkyPassData
    {
        ur_sky_constants Sky;
    };
    Graph.AddPass<FSkyPassData>("Sky", [&](FSkyPassData& Data, FRGPassBuilder& Builder)
    {
        Data.Sky = Constants.Sky;
        if (Plan.Sky.bEnabled) {
            Builder.ReadTexture(DepthHandle, RG_STATE_DEPTH_READ);
            Builder.WriteTexture(LightingHandle, RG_STATE_RENDER_TARGET);
        }
    }, [this, &Res](const FSkyPassData& Data, FHIPCommandContext& Cmd)
    {
        if (!Plan.Sky.bEnabled) return;
        RecordPassError(ur_sky_atmosphere(Cmd.GetContext(), &Data.Sky, Res.DepthBand, Res.LightingBand, Res.Width, Res.Height, Res.Row0, Res.Rows));
    });

    if (Plan.bEndsAtPostRecord) {
        AddPostRecordPass(Graph, LightingHandle, Res);
        Graph.Execute(Cmd);
        LastReport = Graph.GetLastExecutionReport();
        bPostPending = PassError == UR_OK;
        if (bPostPending) PendingConstants = Constants;
        else bLuminanceHistoryValid = false;
        // a TemporalAA frame on the band has not written its image yet: FinishPost does the ring's bookkeeping
        if (!(bPostPending && Plan.TaaOnBand())) EndTaaHistory(false, TaaSlotCount);
        return PassError;
    }

    AddPostPasses(Graph, LightingHandle, Res, Constants, DebugPrint);
    Graph.Execute(Cmd);
    LastReport = Graph.GetLastExecutionReport();
    EndPostHistory();
    EndTaaHistory(Plan.Taa != ETaaMode::Off, TaaSlotCount);
    return PassError;
}
