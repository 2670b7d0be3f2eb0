// HotPathRenderer.cpp — pass wiring of the hot path on FRenderGraph (see HotPathRenderer.h for reference citations).

#include "HotPathRenderer.h"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <sstream>

#include "../../../include/ur_frame.h"
#include "../../../include/ur_host.h"
#include "../ur_internal.h"

int FHotPathRenderer::RenderFrame(FHIPCommandContext& Cmd, FHotPathResources& Res, const FHotPathFrameConstants& Constants,
                                  const FHotPathOptions& Options)
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
    FRenderGraph Graph;
    Graph.SetDevice(Device);
    Graph.SetGpuTimingEnabled(Options.bGpuTiming);
    Graph.SetGraphDumpEnabled(Options.bGraphDump);
    Graph.SetResourceLifetimeLogging(Options.bGraphDump);
    Graph.SetBarrierLoggingEnabled(Options.bBarrierLogs);

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
    const bool bTaaBand = Options.bTaaBand && Options.bTaa && Options.bPostExchange; // TemporalAA on the band, through the exchange
    const bool bPostExchangeFrame = Options.bPostExchange && Options.bTonemap && Res.TonemapBand && (Options.bAutoExposure || Options.bCas || bTaaBand);
    const bool bTaaActive = Options.bTaa && Options.bTonemap && Res.TonemapBand && TaaSlotCount != 0 && (!bPostExchangeFrame || bTaaBand);
    TaaFrame = FTaaFrame{};
    if (bTaaActive) {
        TaaFrame.bActive = true;
        TaaFrame.bFuseTonemap = Options.bFuseTaaTonemap;
        TaaFrame.Slots = GetTaaSlots(Cmd.GetCurrentFrameIndex(), TaaSlotCount);
    }

    // GpuDebugPrint: the cull's two counters and the text buffer, written by "GPU Culling" (reset, then counted) and read by the last pass
    const bool bDebugPrint = IsDebugPrintActive(Res, Options);
    const FRGResourceHandle DebugStatsHandle = bDebugPrint ? Graph.ImportTexture("DebugPrintStats", Res.CullStats, &Res.DebugPrintStatsState, {2, 1, RG_FORMAT_UNKNOWN}) : FRGResourceHandle{};
    const FRGResourceHandle DebugBufferHandle = bDebugPrint ? Graph.ImportTexture("DebugPrintBuffer", Res.DebugPrintBuffer, &Res.DebugPrintState, {static_cast<uint32>(ur_debug_print_buffer_bytes() / 4u), 1, RG_FORMAT_UNKNOWN}) : FRGResourceHandle{};

    // What a raster pass draws from, written by this frame's cull when it runs: its list, else the commands of its ranges or its own
    const auto ImportDraws = [&Graph](const char* Name, const ur_raster_draws& D, uint32* State) {
        const void* Draws = D.visible_idx ? static_cast<const void*>(D.visible_idx) : ur::raster_commands(D);
        return Graph.ImportTexture(Name, const_cast<void*>(Draws), State, {D.command_count, 1, RG_FORMAT_UNKNOWN});
    };
    // ShadowMap: the light view's draws; DepthPrepass: the camera's
    const bool bShadowPass = Res.ShadowPass.Draws != nullptr && Res.ShadowPass.Map != nullptr;
    const bool bDepthPass = Res.DepthPass.Draws != nullptr && Res.DepthPass.Depth != nullptr;
    const bool bCullEnabled = Options.bEnableIndirectDraw && Res.IndirectArgs && Res.ModelBounds && Res.IndirectCommandCount != 0;
    const FRGResourceHandle ShadowDrawsHandle = bShadowPass ? ImportDraws("ShadowDraws", *Res.ShadowPass.Draws, &Res.ShadowDrawsState) : FRGResourceHandle{};
    const FRGResourceHandle DepthDrawsHandle = bDepthPass ? ImportDraws("DepthDraws", *Res.DepthPass.Draws, &Res.DepthDrawsState) : FRGResourceHandle{};

    const bool bHZBEnabled = Options.bHZBEnabled && Res.HZB != nullptr && Res.HZBMipCount != 0;
    if (!bHZBEnabled) bHZBReady = false; // :514-517
    const bool bUseHZBOcclusion = bHZBEnabled && bHZBReady; // ConfigureHZBOcclusion, :519-520

    // ---- GPU Culling (first pass of the frame; uses LAST frame's HZB with the current camera) --------------------
    struct FGpuCullingPassData
    {
        bool bEnabled = false;
        bool bResetDebugPrint = false;
        uint32 Constants[UR_CULL_CONSTANT_DWORDS] = {};
    };
    Graph.AddPass<FGpuCullingPassData>("GPU Culling", [&](FGpuCullingPassData& Data, FRGPassBuilder& Builder)
    {
        Data.bEnabled = Options.bEnableIndirectDraw && Res.IndirectArgs && Res.ModelBounds && Res.IndirectCommandCount != 0;
        std::memcpy(Data.Constants, Constants.CullingConstants, sizeof(Data.Constants));
        Data.Constants[40] = Res.IndirectCommandCount;
        Data.Constants[41] = bUseHZBOcclusion ? 1u : 0u;
        Data.Constants[42] = Res.HZBMipCount;
        Data.Constants[43] = HZBWidth;
        Data.Constants[44] = HZBHeight;
        if (bDebugPrint) { // PrepareGpuDebugPrint (:390) and DebugPrintEnabled: the counters are zeroed, then counted, on this pass's stream
            Data.bResetDebugPrint = true;
            Data.Constants[45] = 1u;
            Builder.WriteTexture(DebugStatsHandle, RG_STATE_UNORDERED_ACCESS);
            Builder.WriteTexture(DebugBufferHandle, RG_STATE_UNORDERED_ACCESS);
        }
        if (Data.bEnabled) {
            if (bUseHZBOcclusion) Builder.ReadTexture(HZBHandle, RG_STATE_NON_PIXEL_SHADER_RESOURCE);
            if (bShadowPass && Options.bRenderShadows) Builder.WriteTexture(ShadowDrawsHandle, RG_STATE_UNORDERED_ACCESS); // the light view's list / ranges
            if (bDepthPass && Options.bDoDepthPrepass) Builder.WriteTexture(DepthDrawsHandle, RG_STATE_UNORDERED_ACCESS);   // the camera's list / ranges
            Builder.KeepAlive();
            // Neither visibility pass shares a resource with Lighting/Sky inside a frame (the cull reads LAST frame's
            // HZB), so both can run beside the VALU-bound lighting kernel on the second stream.
            if (Options.bAsyncCompute) Builder.AsyncCompute();
        }
    }, [this, &Res](const FGpuCullingPassData& Data, FHIPCommandContext& Cmd)
    {
        if (Data.bResetDebugPrint) {
            const int rc = ur_debug_print_reset(Cmd.GetContext(), Res.DebugPrintBuffer, Res.CullStats);
            if (rc != UR_OK && PassError == UR_OK) PassError = rc;
        }
        if (!Data.bEnabled) return;
        // DispatchGpuCulling (Renderer.cpp:394-472): the UAV / INDIRECT_ARGUMENT transitions are stream order here.
        // With draw ranges the same call also places the visible commands of each range and writes its count (ur_cull_indirect_args_draws).
        // With extra views (UR_FRAME_CULL_VIEWS) the same launch also tests them (ur_cull_indirect_args_views): the DepthPrepass / ShadowMap
        // visibility of UpdateCullingVisibility (DeferredRenderer.cpp:3803-3812) and the shadow pass (:583-591).
        // (No views: views = NULL, exactly ur_cull_indirect_args_draws.)
        const int rc = ur_cull_indirect_args_views(Cmd.GetContext(), Data.Constants, Res.ModelBounds, Res.HZB, Res.HZBMips, Res.IndirectArgs, Res.CullStats,
                                                   Res.VisibleIndices, Res.VisibleCount, Res.InstanceIndexBase, Res.DrawRanges,
                                                   Res.CullViewCount != 0 ? Res.CullViews : nullptr, Res.CullViewCount);
        if (rc != UR_OK && PassError == UR_OK) PassError = rc;
    });

    // ---- ShadowMap (:551-633): the light view's draws, depth only, into the map Lighting samples -----------------------
    struct FShadowPassData
    {
        bool bEnabled = false;
        float LightViewProjection[16] = {};
        uint32 Width = 0, Height = 0;
    };
    if (bShadowPass) {
        Graph.AddPass<FShadowPassData>("ShadowMap", [&](FShadowPassData& Data, FRGPassBuilder& Builder)
        {
            Data.bEnabled = Options.bRenderShadows;
            std::memcpy(Data.LightViewProjection, Constants.Scene.LightViewProjection, sizeof(Data.LightViewProjection));
            Data.Width = static_cast<uint32>(Constants.Scene.ShadowMapSize[0]);
            Data.Height = static_cast<uint32>(Constants.Scene.ShadowMapSize[1]);
            if (Data.bEnabled) {
                if (bCullEnabled) Builder.ReadTexture(ShadowDrawsHandle, RG_STATE_INDIRECT_ARGUMENT); // (on the async lane: the wait on the cull)
                Builder.WriteTexture(ShadowHandle, RG_STATE_DEPTH_WRITE);
            }
        }, [this, &Res](const FShadowPassData& Data, FHIPCommandContext& Cmd)
        {
            if (!Data.bEnabled) return;
            // ClearDepth(1.0) and the draws of :571-631, on the stream the pass runs on (the main one: it is not an async-compute pass)
            const int rc = ur_shadow_map(Cmd.GetContext(), Data.LightViewProjection, Res.ShadowPass.Draws, Res.ShadowPass.Map, Data.Width, Data.Height, Res.ShadowPass.Stats);
            if (rc != UR_OK && PassError == UR_OK) PassError = rc;
        });
    }

    // ---- DepthPrepass (:635-718): the camera's draws, depth only, into the buffer Build HZB reads ---------------------------------
    struct FDepthPrepassData
    {
        bool bEnabled = false;
        float View[16] = {}, Projection[16] = {};
        uint32 Width = 0, Height = 0, Flags = 0;
    };
    if (bDepthPass) {
        Graph.AddPass<FDepthPrepassData>("DepthPrepass", [&](FDepthPrepassData& Data, FRGPassBuilder& Builder)
        {
            Data.bEnabled = Options.bDoDepthPrepass;
            std::memcpy(Data.View, Constants.Scene.View, sizeof(Data.View));
            std::memcpy(Data.Projection, Constants.Scene.Projection, sizeof(Data.Projection));
            Data.Width = Res.Width;
            Data.Height = Res.Height;
            Data.Flags = Res.DepthPass.Flags;
            if (Data.bEnabled) {
                if (bCullEnabled) Builder.ReadTexture(DepthDrawsHandle, RG_STATE_INDIRECT_ARGUMENT); // (on the async lane: the wait on the cull)
                Builder.WriteTexture(DepthHandle, RG_STATE_DEPTH_WRITE);
            }
        }, [this, &Res](const FDepthPrepassData& Data, FHIPCommandContext& Cmd)
        {
            if (!Data.bEnabled) return;
            // ClearDepth(0.0) and the draws of :655-716, on the main stream: Build HZB (on the async lane: behind a wait) reads what it wrote
            const int rc = ur_depth_prepass(Cmd.GetContext(), Data.View, Data.Projection, Res.DepthPass.Draws, Res.DepthPass.Depth, Data.Width, Data.Height, Data.Flags, Res.DepthPass.Stats);
            if (rc != UR_OK && PassError == UR_OK) PassError = rc;
        });
    }

    // ---- GBuffer (:720-865, with ObjectId :867-980 as its optional fifth output): the base pass against the prepass' depth ------------
    struct FGBufferPassData
    {
        bool bEnabled = false;
        float View[16] = {}, Projection[16] = {};
    };
    if (bDepthPass && Res.GBufferPass.Draws != nullptr) {
        Graph.AddPass<FGBufferPassData>("GBuffer", [&](FGBufferPassData& Data, FRGPassBuilder& Builder)
        {
            Data.bEnabled = Options.bDoDepthPrepass; // (the base pass tests against the prepass' depth: without it the pass is listed and culled)
            std::memcpy(Data.View, Constants.Scene.View, sizeof(Data.View));
            std::memcpy(Data.Projection, Constants.Scene.Projection, sizeof(Data.Projection));
            if (Data.bEnabled) {
                Builder.ReadTexture(DepthHandle, RG_STATE_DEPTH_READ); // (main stream, behind DepthPrepass: the cull's lists and ranges are complete)
                Builder.WriteTexture(GBufferHandles[0], RG_STATE_RENDER_TARGET);
                Builder.WriteTexture(GBufferHandles[1], RG_STATE_RENDER_TARGET);
                Builder.WriteTexture(GBufferHandles[2], RG_STATE_RENDER_TARGET);
                Builder.WriteTexture(LightingHandle, RG_STATE_RENDER_TARGET); // SceneColor: (emissive, 1), what Lighting adds to
            }
        }, [this, &Res](const FGBufferPassData& Data, FHIPCommandContext& Cmd)
        {
            if (!Data.bEnabled) return;
            // (a null table is ur_gbuffer_pass)
            const int rc = ur_gbuffer_pass_materials(Cmd.GetContext(), Data.View, Data.Projection, Res.GBufferPass.Draws, Res.DepthPass.Depth, &Res.GBufferPass.Targets,
                                                     Res.Width, Res.Height, Res.Row0, Res.Rows, Res.DepthPass.Flags, Res.GBufferPass.KeyBits, Res.GBufferPass.Stats,
                                                     Res.GBufferMaterials, Res.GBufferMaterialCount);
            if (rc != UR_OK && PassError == UR_OK) PassError = rc;
        });
    }

    // ---- Build HZB (after the G-buffer pass; only with HZB and depth prepass enabled, :996) ------------------------
    struct FHZBPassData
    {
        uint32 Width = 0, Height = 0, MipCount = 0, SourceWidth = 0, SourceHeight = 0;
        bool bShard = false;
    };
    if (bHZBEnabled && Options.bDoDepthPrepass) {
        Graph.AddPass<FHZBPassData>("Build HZB", [&](FHZBPassData& Data, FRGPassBuilder& Builder)
        {
            Data.Width = HZBWidth;
            Data.Height = HZBHeight;
            Data.MipCount = Res.HZBMipCount;
            Data.SourceWidth = Res.Width;
            Data.SourceHeight = Res.Height;
            Data.bShard = Options.bShardHZB;
            Builder.ReadTexture(DepthHandle, RG_STATE_NON_PIXEL_SHADER_RESOURCE);
            Builder.WriteTexture(HZBHandle, RG_STATE_UNORDERED_ACCESS);
            if (Options.bAsyncCompute) Builder.AsyncCompute();
        }, [this, &Res](const FHZBPassData& Data, FHIPCommandContext& Cmd)
        {
            if (Data.MipCount == 0) return;
            int rc;
            if (Data.bShard) { // this rank's piece rows of the wide launch; the ranks' exchange and the tail are the caller's (it holds the communicator)
                uint32_t Row0 = 0, Rows = 0;
                rc = ur_hzb_band_pieces(Data.SourceHeight, static_cast<uint32_t>(Cmd.GetWorldSize()), static_cast<uint32_t>(Cmd.GetRank()), &Row0, &Rows);
                if (rc == UR_OK) rc = ur_build_hzb_band(Cmd.GetContext(), Res.DepthFull, Data.SourceWidth, Data.SourceHeight, Res.HZB, Res.HZBMips, Data.MipCount, Row0, Rows);
            } else {
                rc = ur_build_hzb(Cmd.GetContext(), Res.DepthFull, Data.SourceWidth, Data.SourceHeight, Res.HZB, Res.HZBMips, Data.MipCount);
            }
            if (rc != UR_OK && PassError == UR_OK) PassError = rc;
            Res.HZBState = RG_STATE_NON_PIXEL_SHADER_RESOURCE; // :1209
            if (rc == UR_OK) bHZBReady = true;                  // :1210
        });
    }

    const bool bSky = Options.bSkyEnabled && Res.DepthBand != nullptr;
    const bool bFused = Options.bFuseLightingAndSky && bSky;

    // ---- Lighting (fullscreen, additive) --------------------------------------------------------------------------
    struct FLightingPassData
    {
        bool bUseShadows = false;
        bool bFusedSky = false;
        ur_scene_constants Scene;
        ur_sky_constants Sky;
    };
    Graph.AddPass<FLightingPassData>("Lighting", [&](FLightingPassData& Data, FRGPassBuilder& Builder)
    {
        Data.bUseShadows = Options.bRenderShadows;
        Data.bFusedSky = bFused;
        Data.Scene = Constants.Scene;
        Data.Sky = Constants.Sky;
        if (!Data.bUseShadows) Data.Scene.ShadowStrength = 0.0f; // bShadowsEnabled ? ShadowStrength : 0 (:3777)
        Builder.ReadTexture(GBufferHandles[0], RG_STATE_PIXEL_SHADER_RESOURCE);
        Builder.ReadTexture(GBufferHandles[1], RG_STATE_PIXEL_SHADER_RESOURCE);
        Builder.ReadTexture(GBufferHandles[2], RG_STATE_PIXEL_SHADER_RESOURCE);
        if (Data.bUseShadows) Builder.ReadTexture(ShadowHandle, RG_STATE_PIXEL_SHADER_RESOURCE);
        if (Data.bFusedSky) Builder.ReadTexture(DepthHandle, RG_STATE_DEPTH_READ);
        Builder.WriteTexture(LightingHandle, RG_STATE_RENDER_TARGET);
    }, [this, &Res, &Options](const FLightingPassData& Data, FHIPCommandContext& Cmd)
    {
        const bool bTimed = Options.bTimeLighting && LightingTimer;
        if (bTimed) LightingTimer(Cmd.GetStream(), true);
        int rc;
        if (Data.bFusedSky)
            rc = ur_deferred_lighting_sky(Cmd.GetContext(), &Data.Scene, &Data.Sky, Res.GBufferA, Res.GBufferB, Res.GBufferC, Res.DepthBand, &Res.Tables,
                                          Res.LightingBand, Res.Width, Res.Height, Res.Row0, Res.Rows);
        else
            rc = ur_deferred_lighting(Cmd.GetContext(), &Data.Scene, Res.GBufferA, Res.GBufferB, Res.GBufferC, &Res.Tables, Res.LightingBand, Res.Width,
                                      Res.Height, Res.Row0, Res.Rows);
        if (bTimed) LightingTimer(Cmd.GetStream(), false);
        if (rc != UR_OK && PassError == UR_OK) PassError = rc;
    });

    // ---- Sky --------------------------------------------------------------------------------------------------------
    struct FSkyPassData
    {
        bool bEnabled = false;
        ur_sky_constants Sky;
    };
    Graph.AddPass<FSkyPassData>("Sky", [&](FSkyPassData& Data, FRGPassBuilder& Builder)
    {
        Data.bEnabled = bSky && !bFused;
        Data.Sky = Constants.Sky;
        if (Data.bEnabled) {
            Builder.ReadTexture(DepthHandle, RG_STATE_DEPTH_READ);
            Builder.WriteTexture(LightingHandle, RG_STATE_RENDER_TARGET);
        }
    }, [this, &Res](const FSkyPassData& Data, FHIPCommandContext& Cmd)
    {
        if (!Data.bEnabled) return;
        const int rc = ur_sky_atmosphere(Cmd.GetContext(), &Data.Sky, Res.DepthBand, Res.LightingBand, Res.Width, Res.Height, Res.Row0, Res.Rows);
        if (rc != UR_OK && PassError == UR_OK) PassError = rc;
    });

    const bool bPostPasses = Options.bTonemap && Res.TonemapBand && (Options.bAutoExposure || Options.bCas);
    const bool bTaaBandFrame = bTaaBand && bTaaActive;
    if (Options.bPostExchange && (bPostPasses || bTaaBandFrame)) {
        // ---- Post Record: the band's part of the post exchange; the post passes wait for FinishPost --------------------------
        // With TemporalAA on the band the pass packs the TAA record too, from the history image the frame reads: before the resolve,
        // which with a ring of one image overwrites it.
        struct FPostRecordPassData
        {
            bool bTaa = false;
            uint32 TaaUseHistory = 0, TaaReadIndex = 0;
        };
        const FHotPathRenderer::FTaaSlots Taa = TaaFrame.Slots;
        FRGResourceHandle TaaRecordHandle, TaaReadHandle;
        if (bTaaBandFrame) {
            TaaRecordHandle = Graph.ImportTexture("TaaRecord", Res.TaaRecord, &Res.TaaRecordState,
                                                  {static_cast<uint32>(ur_taa_record_bytes(Res.Width) / 8u), 1, RG_FORMAT_R16G16B16A16_FLOAT});
            if (Taa.bUseHistory)
                TaaReadHandle = Graph.ImportTexture("TaaHistory_" + std::to_string(Taa.Read), Res.TaaHistory[Taa.Read], &Res.TaaHistoryStates[Taa.Read],
                                                    {Res.Width, Res.Rows, RG_FORMAT_R16G16B16A16_FLOAT});
        }
        const FRGResourceHandle RecordHandle = Graph.ImportTexture("PostRecord", Res.PostRecord, &Res.PostRecordState,
                                                                   {static_cast<uint32>(ur_post_record_bytes(Res.Width) / 8u), 1, RG_FORMAT_R16G16B16A16_FLOAT});
        Graph.AddPass<FPostRecordPassData>("Post Record", [&](FPostRecordPassData& Data, FRGPassBuilder& Builder)
        {
            Data.bTaa = bTaaBandFrame;
            Data.TaaUseHistory = Taa.bUseHistory ? 1u : 0u;
            Data.TaaReadIndex = Taa.Read;
            Builder.ReadTexture(LightingHandle, RG_STATE_NON_PIXEL_SHADER_RESOURCE);
            Builder.WriteTexture(RecordHandle, RG_STATE_UNORDERED_ACCESS);
            if (Data.bTaa) {
                if (Taa.bUseHistory) Builder.ReadTexture(TaaReadHandle, RG_STATE_NON_PIXEL_SHADER_RESOURCE);
                Builder.WriteTexture(TaaRecordHandle, RG_STATE_UNORDERED_ACCESS);
            }
        }, [this, &Res](const FPostRecordPassData& Data, FHIPCommandContext& Cmd)
        {
            int rc = ur_pack_post_record(Cmd.GetContext(), Res.LightingBand, Res.Width, Res.Height, Res.Row0, Res.Rows, Res.PostRecord);
            if (rc == UR_OK && Data.bTaa)
                rc = ur_pack_taa_record(Cmd.GetContext(), Res.LightingBand, Data.TaaUseHistory ? Res.TaaHistory[Data.TaaReadIndex] : nullptr, Data.TaaUseHistory,
                                        Res.Width, Res.Height, Res.Row0, Res.Rows, Res.TaaRecord);
            if (rc != UR_OK && PassError == UR_OK) PassError = rc;
        });
        Graph.Execute(Cmd);
        LastReport = Graph.GetLastExecutionReport();
        bPostPending = PassError == UR_OK;
        if (bPostPending) {
            PendingConstants = Constants;
            PendingOptions = Options;
        } else {
            bLuminanceHistoryValid = false;
        }
        // a TemporalAA frame on the band has not written its image yet: FinishPost does the ring's bookkeeping
        if (!(bPostPending && bTaaBandFrame)) EndTaaHistory(false, 0, TaaSlotCount);
        return PassError;
    }

    AddPostPasses(Graph, LightingHandle, Res, Constants, Options, 0, DebugStatsHandle, DebugBufferHandle);
    Graph.Execute(Cmd);
    LastReport = Graph.GetLastExecutionReport();
    EndPostHistory(Options.bTonemap && Res.TonemapBand && Options.bAutoExposure);
    EndTaaHistory(bTaaActive, TaaFrame.Slots.Write, TaaSlotCount);
    return PassError;
}

int FHotPathRenderer::FinishPost(FHIPCommandContext& Cmd, FHotPathResources& Res)
{
    if (!bPostPending) { ur::set_error("ur_frame_finish_post: no post passes are pending (render with UR_FRAME_POST_EXCHANGE and AUTO_EXPOSURE / CAS / TAA_BAND first)"); return UR_EINVAL; }
    bPostPending = false;
    PassError = UR_OK;
    const bool bTaaBandFrame = TaaFrame.bActive && PendingOptions.bTaaBand; // RenderFrame's slots, kept while the passes were pending
    if (!bTaaBandFrame) TaaFrame = FTaaFrame{}; // (without bTaaBand a frame of the post exchange runs without TemporalAA)
    FRenderGraph Graph;
    Graph.SetDevice(Device);
    Graph.SetGpuTimingEnabled(PendingOptions.bGpuTiming);
    Graph.SetGraphDumpEnabled(PendingOptions.bGraphDump);
    Graph.SetResourceLifetimeLogging(PendingOptions.bGraphDump);
    Graph.SetBarrierLoggingEnabled(PendingOptions.bBarrierLogs);
    const FRGResourceHandle LightingHandle = Graph.ImportTexture("Lighting", Res.LightingBand, &Res.LightingState, {Res.Width, Res.Rows, RG_FORMAT_R16G16B16A16_FLOAT});
    // GpuDebugPrint behind the exchange: the counters are the ones the caller has summed over the ranks meanwhile (dist.allreduce_cull_stats)
    const bool bDebugPrint = IsDebugPrintActive(Res, PendingOptions);
    const FRGResourceHandle DebugStatsHandle = bDebugPrint ? Graph.ImportTexture("DebugPrintStats", Res.CullStats, &Res.DebugPrintStatsState, {2, 1, RG_FORMAT_UNKNOWN}) : FRGResourceHandle{};
    const FRGResourceHandle DebugBufferHandle = bDebugPrint ? Graph.ImportTexture("DebugPrintBuffer", Res.DebugPrintBuffer, &Res.DebugPrintState, {static_cast<uint32>(ur_debug_print_buffer_bytes() / 4u), 1, RG_FORMAT_UNKNOWN}) : FRGResourceHandle{};
    AddPostPasses(Graph, LightingHandle, Res, PendingConstants, PendingOptions, static_cast<uint32>(Cmd.GetWorldSize()), DebugStatsHandle, DebugBufferHandle);
    Graph.Execute(Cmd);
    const std::vector<FRenderGraph::FPassReport>& Tail = Graph.GetLastExecutionReport();
    LastReport.insert(LastReport.end(), Tail.begin(), Tail.end());
    EndPostHistory(PendingOptions.bAutoExposure);
    if (bTaaBandFrame) EndTaaHistory(true, TaaFrame.Slots.Write, static_cast<uint32>(Res.TaaHistory.size())); // (else RenderFrame dropped the ring)
    return PassError;
}

void FHotPathRenderer::EndPostHistory(bool bAutoExposure)
{
    // :1612-1620: the luminance written this frame is next frame's history
    if (bAutoExposure && PassError == UR_OK) {
        bLuminanceHistoryValid = true;
        LuminanceWriteIndex = 1u - LuminanceWriteIndex;
    } else {
        bLuminanceHistoryValid = false;
    }
}

FHotPathRenderer::FTaaSlots FHotPathRenderer::GetTaaSlots(uint32 FrameIndex, uint32 SlotCount) const
{
    FTaaSlots S;
    if (SlotCount == 0) return S;
    S.Read = (FrameIndex + SlotCount - 1u) % SlotCount; // :396-397
    S.Write = FrameIndex % SlotCount;
    S.bUseHistory = S.Read < TaaHistoryValid.size() && TaaHistoryValid[S.Read];
    S.SampleIndex = TaaSampleIndex;
    return S;
}

void FHotPathRenderer::EndTaaHistory(bool bTaaActive, uint32 WriteIndex, uint32 SlotCount)
{
    // :1602-1610, and OnFrameFenceSignaled (:2787-2799): the slot a TemporalAA frame wrote is next frame's history. The reference marks
    // it when the frame's fence is signalled and does not wait for the GPU either; here stream order makes the image complete before
    // the next frame's pass reads it. A frame whose pass failed hands on nothing.
    if (TaaHistoryValid.size() != SlotCount) TaaHistoryValid.assign(SlotCount, false);
    if (bTaaActive && PassError == UR_OK) {
        TaaHistoryValid[WriteIndex] = true;
        TaaSampleIndex = (TaaSampleIndex + 1u) % 8u;
    } else {
        ResetTaa();
    }
}

// [TemporalAA ->] AutoExposure -> Tonemap -> CAS. RecordRanks != 0: on the band alone, from the RecordRanks gathered post records (FinishPost; the
// band is this rank's equal band): AutoExposure reads every rank's tap texels, Tonemap / CAS read the rows around the band from the
// neighbours' records in place. TemporalAA on the band (TaaFrame active in FinishPost) resolves from the neighbours' current rows in the
// post records and, for CAS, also resolves the row on either side of the band from their TAA records into Res.TaaHaloRows: CAS's halo rows.
void FHotPathRenderer::AddPostPasses(FRenderGraph& Graph, FRGResourceHandle LightingHandle, FHotPathResources& Res, const FHotPathFrameConstants& Constants,
                                     const FHotPathOptions& Options, uint32 RecordRanks, FRGResourceHandle DebugStatsHandle, FRGResourceHandle DebugBufferHandle)
{
    // (DeferredRenderer.cpp:1308-1573)
    // Without TemporalAA, AutoExposure and CAS this is the Tonemap pass alone, Lighting -> LDR band, as before they existed.
    const bool bAutoExposure = Options.bTonemap && Res.TonemapBand && Options.bAutoExposure;
    const bool bCas = Options.bTonemap && Res.TonemapBand && Options.bCas;
    const bool bFuseCas = bCas && Options.bFuseTonemapCas;
    const uint32 WriteIndex = LuminanceWriteIndex;
    const bool bFromRecords = RecordRanks != 0;
    const uint64 RecordBytes = ur_post_record_bytes(Res.Width);
    const uint8_t* Records = static_cast<const uint8_t*>(Res.PostRecords);
    const uint32 Rank = bFromRecords ? Res.Row0 / Res.Rows : 0;
    // the neighbours' last / first HDR rows: the halo rows of CAS (none at the frame's top / bottom edge), and of TemporalAA on the band
    const ur_half4* CurAbove = bFromRecords && Rank > 0 ? reinterpret_cast<const ur_half4*>(Records + (Rank - 1) * RecordBytes + 8ull * Res.Width) : nullptr;
    const ur_half4* CurBelow = bFromRecords && Rank + 1 < RecordRanks ? reinterpret_cast<const ur_half4*>(Records + (Rank + 1) * RecordBytes) : nullptr;
    // TemporalAA on the band: behind it CAS's halo rows are the RESOLVED rows around the band, which the TemporalAA launch writes
    // from the neighbours' TAA records: above second_last_row / history_last_row, below second_row / history_first_row
    const bool bTaaRecords = TaaFrame.bActive && bFromRecords;
    const bool bTaaHalo = bTaaRecords && bCas;
    const uint64 TaaRecordBytes = ur_taa_record_bytes(Res.Width);
    const uint8_t* TaaRecs = static_cast<const uint8_t*>(Res.TaaRecords);
    struct FTaaBandRows
    {
        const ur_half4 *CurAbove = nullptr, *CurBelow = nullptr, *Above2 = nullptr, *HistAbove = nullptr, *Below2 = nullptr, *HistBelow = nullptr;
        ur_half4 *ResolvedAbove = nullptr, *ResolvedBelow = nullptr;
    } TaaRows;
    if (bTaaRecords) {
        TaaRows.CurAbove = CurAbove;
        TaaRows.CurBelow = CurBelow;
        if (bTaaHalo && CurAbove) {
            const uint8_t* N = TaaRecs + (Rank - 1) * TaaRecordBytes;
            TaaRows.Above2 = reinterpret_cast<const ur_half4*>(N + 8ull * Res.Width);
            if (TaaFrame.Slots.bUseHistory) TaaRows.HistAbove = reinterpret_cast<const ur_half4*>(N + 24ull * Res.Width);
            TaaRows.ResolvedAbove = Res.TaaHaloRows;
        }
        if (bTaaHalo && CurBelow) {
            const uint8_t* N = TaaRecs + (Rank + 1) * TaaRecordBytes;
            TaaRows.Below2 = reinterpret_cast<const ur_half4*>(N);
            if (TaaFrame.Slots.bUseHistory) TaaRows.HistBelow = reinterpret_cast<const ur_half4*>(N + 16ull * Res.Width);
            TaaRows.ResolvedBelow = Res.TaaHaloRows + Res.Width;
        }
    }
    const ur_half4* HaloAbove = bTaaRecords ? TaaRows.ResolvedAbove : CurAbove;
    const ur_half4* HaloBelow = bTaaRecords ? TaaRows.ResolvedBelow : CurBelow;
    const FRGResourceHandle TaaRecordsHandle = bTaaHalo
        ? Graph.ImportTexture("TaaRecords", const_cast<void*>(Res.TaaRecords), &Res.TaaRecordsState, {static_cast<uint32>(TaaRecordBytes / 8u), RecordRanks, RG_FORMAT_R16G16B16A16_FLOAT})
        : FRGResourceHandle{};
    const FRGResourceHandle TaaHaloHandle = bTaaHalo
        ? Graph.ImportTexture("TaaHaloRows", Res.TaaHaloRows, &Res.TaaHaloRowsState, {Res.Width, 2, RG_FORMAT_R16G16B16A16_FLOAT})
        : FRGResourceHandle{};
    const FRGResourceHandle RecordsHandle = bFromRecords
        ? Graph.ImportTexture("PostRecords", const_cast<void*>(Res.PostRecords), &Res.PostRecordsState, {static_cast<uint32>(RecordBytes / 8u), RecordRanks, RG_FORMAT_R16G16B16A16_FLOAT})
        : FRGResourceHandle{};
    FRGResourceHandle LuminanceHandles[2];
    if (bAutoExposure) {
        LuminanceHandles[0] = Graph.ImportTexture("LuminanceA", Res.Luminance[0], &Res.LuminanceStates[0], {1, 1, RG_FORMAT_R32_FLOAT});
        LuminanceHandles[1] = Graph.ImportTexture("LuminanceB", Res.Luminance[1], &Res.LuminanceStates[1], {1, 1, RG_FORMAT_R32_FLOAT});
    }

    // ---- TemporalAA (:1308-1361): Lighting + TaaHistory_<Read> -> TaaHistory_<Write>; AutoExposure keeps reading Lighting (:1387),
    // Tonemap reads TaaHistory_<Write> (:1454-1459). With bFuseTaaTonemap the pass stays in the graph, disabled and culled, and the
    // Tonemap pass makes the one launch (ur_temporal_aa_tonemap).
    struct FTemporalAAPassData
    {
        bool bEnabled = false;
        float HistoryWeight = 0.9f;
        uint32 UseHistory = 0, ReadIndex = 0, WriteIndex = 0;
        bool bHalo = false; // the band alone (FinishPost): ur_temporal_aa_halo
    };
    // the rows around the band that a TemporalAA launch on the band reads, declared by the pass that makes the launch
    auto DeclareTaaBandRows = [&](FRGPassBuilder& Builder) {
        if (!bTaaRecords) return;
        Builder.ReadTexture(RecordsHandle, RG_STATE_NON_PIXEL_SHADER_RESOURCE);
        if (bTaaHalo) {
            Builder.ReadTexture(TaaRecordsHandle, RG_STATE_NON_PIXEL_SHADER_RESOURCE);
            Builder.WriteTexture(TaaHaloHandle, RG_STATE_UNORDERED_ACCESS);
        }
    };
    const bool bTaa = TaaFrame.bActive;
    const bool bFuseTaa = bTaa && TaaFrame.bFuseTonemap;
    const FHotPathRenderer::FTaaSlots Taa = TaaFrame.Slots;
    FRGResourceHandle TaaReadHandle, TaaWriteHandle;
    if (bTaa) {
        auto Import = [&](uint32 I) {
            return Graph.ImportTexture("TaaHistory_" + std::to_string(I), Res.TaaHistory[I], &Res.TaaHistoryStates[I], {Res.Width, Res.Rows, RG_FORMAT_R16G16B16A16_FLOAT});
        };
        TaaWriteHandle = Import(Taa.Write);
        TaaReadHandle = Taa.Read == Taa.Write ? TaaWriteHandle : Import(Taa.Read); // a ring of one image: read and written in place
        Graph.AddPass<FTemporalAAPassData>("TemporalAA", [&](FTemporalAAPassData& Data, FRGPassBuilder& Builder)
        {
            Data.bEnabled = !bFuseTaa;
            if (!Data.bEnabled) return;
            Data.ReadIndex = Taa.Read;
            Data.WriteIndex = Taa.Write;
            Data.HistoryWeight = Constants.TaaHistoryWeight;
            Data.UseHistory = Taa.bUseHistory ? 1u : 0u;
            Data.bHalo = bTaaRecords;
            Builder.ReadTexture(LightingHandle, RG_STATE_NON_PIXEL_SHADER_RESOURCE);
            if (Taa.Read != Taa.Write) Builder.ReadTexture(TaaReadHandle, RG_STATE_NON_PIXEL_SHADER_RESOURCE);
            DeclareTaaBandRows(Builder);
            Builder.WriteTexture(TaaWriteHandle, RG_STATE_UNORDERED_ACCESS);
        }, [this, &Res, TaaRows](const FTemporalAAPassData& Data, FHIPCommandContext& Cmd)
        {
            if (!Data.bEnabled) return;
            const int rc = Data.bHalo
                ? ur_temporal_aa_halo(Cmd.GetContext(), Res.LightingBand, TaaRows.CurAbove, TaaRows.CurBelow, Res.TaaHistory[Data.ReadIndex],
                                      Res.TaaHistory[Data.WriteIndex], TaaRows.Above2, TaaRows.HistAbove, TaaRows.Below2, TaaRows.HistBelow, TaaRows.ResolvedAbove,
                                      TaaRows.ResolvedBelow, Data.HistoryWeight, Data.UseHistory, Res.Width, Res.Height, Res.Row0, Res.Rows)
                : ur_temporal_aa(Cmd.GetContext(), Res.LightingBand, Res.TaaHistory[Data.ReadIndex], Res.TaaHistory[Data.WriteIndex], Data.HistoryWeight,
                                          Data.UseHistory, Res.Width, Res.Height, 0, Res.Height);
            if (rc != UR_OK && PassError == UR_OK) PassError = rc;
        });
    }

    struct FAutoExposurePassData
    {
        bool bEnabled = false;
        ur_auto_exposure_constants K = {};
        uint32 ReadIndex = 0, WriteIndex = 0;
        uint32 RecordRanks = 0;
    };
    if (bAutoExposure) {
        Graph.AddPass<FAutoExposurePassData>("AutoExposure", [&](FAutoExposurePassData& Data, FRGPassBuilder& Builder)
        {
            Data.bEnabled = true;
            Data.ReadIndex = 1u - WriteIndex;
            Data.WriteIndex = WriteIndex;
            Data.K.InputSize[0] = static_cast<float>(Res.Width);
            Data.K.InputSize[1] = static_cast<float>(Res.Height);
            Data.K.DeltaTime = Constants.DeltaTime;
            Data.K.AdaptationSpeedUp = Constants.AutoExposureSpeedUp;
            Data.K.AdaptationSpeedDown = Constants.AutoExposureSpeedDown;
            Data.K.UseHistory = bLuminanceHistoryValid ? 1u : 0u;
            Data.K.AutoExposureKey = Constants.AutoExposureKey;
            Data.K.AutoExposureMin = Constants.AutoExposureMin;
            Data.K.AutoExposureMax = Constants.AutoExposureMax;
            Data.RecordRanks = RecordRanks;
            Builder.ReadTexture(bFromRecords ? RecordsHandle : LightingHandle, RG_STATE_NON_PIXEL_SHADER_RESOURCE);
            Builder.ReadTexture(LuminanceHandles[Data.ReadIndex], RG_STATE_NON_PIXEL_SHADER_RESOURCE);
            Builder.WriteTexture(LuminanceHandles[Data.WriteIndex], RG_STATE_UNORDERED_ACCESS);
        }, [this, &Res](const FAutoExposurePassData& Data, FHIPCommandContext& Cmd)
        {
            const float* Prev = Data.K.UseHistory ? Res.Luminance[Data.ReadIndex] : nullptr;
            const int rc = Data.RecordRanks
                ? ur_auto_exposure_records(Cmd.GetContext(), &Data.K, Res.PostRecords, Data.RecordRanks, Res.Width, Res.Height, Prev, Res.Luminance[Data.WriteIndex])
                : ur_auto_exposure(Cmd.GetContext(), &Data.K, Res.LightingBand, Res.Width, Res.Height, Prev, Res.Luminance[Data.WriteIndex]);
            if (rc != UR_OK && PassError == UR_OK) PassError = rc;
        });
    }

    struct FTonemapPassData
    {
        bool bEnabled = false;
        bool bFuseCas = false;
        ur_tonemap_constants K;
        ur_cas_constants Cas;
        const float* ExposureEv = nullptr;
        uint32* Output = nullptr;
        bool bHalo = false;
        const ur_half4* HaloAbove = nullptr;
        const ur_half4* HaloBelow = nullptr;
        const ur_half4* Input = nullptr; // Lighting, or TaaHistory_<Write> behind a TemporalAA pass
        bool bFuseTaa = false;           // TemporalAA + Tonemap in this pass's launch
        bool bTaaHalo = false;           // ... on the band alone (ur_temporal_aa_tonemap_halo)
        float TaaHistoryWeight = 0.9f;
        uint32 TaaUseHistory = 0, TaaReadIndex = 0, TaaWriteIndex = 0;
    };
    struct FCasPassData
    {
        bool bEnabled = false;
        ur_cas_constants K;
        bool bHalo = false; // the band alone: the rows around it are Tonemap's input rows from the records, tonemapped by the CAS launch
        ur_tonemap_constants Tonemap;
        const float* ExposureEv = nullptr;
        const ur_half4* HaloAbove = nullptr;
        const ur_half4* HaloBelow = nullptr;
    };
    if (Options.bTonemap && Res.TonemapBand) {
        // the back buffer: "TonemapOutput" itself when nothing follows Tonemap
        const FRGResourceHandle TonemapHandle = bCas ? Graph.ImportTexture("BackBuffer", Res.TonemapBand, &Res.TonemapState, {Res.Width, Res.Rows, RG_FORMAT_R8G8B8A8_UNORM})
                                                     : Graph.ImportTexture("TonemapOutput", Res.TonemapBand, &Res.TonemapState, {Res.Width, Res.Rows, RG_FORMAT_R8G8B8A8_UNORM_SRGB});
        const FRGResourceHandle ScratchHandle = bCas && !bFuseCas
            ? Graph.ImportTexture("TonemapOutput", Res.TonemapScratch, &Res.TonemapScratchState, {Res.Width, Res.Rows, RG_FORMAT_R8G8B8A8_UNORM})
            : FRGResourceHandle{};
        const ur_cas_constants CasK = {{1.0f / static_cast<float>(Res.Width), 1.0f / static_cast<float>(Res.Height)}, Constants.CasSharpness, 0.0f}; // :1533
        Graph.AddPass<FTonemapPassData>("Tonemap", [&](FTonemapPassData& Data, FRGPassBuilder& Builder)
        {
            Data.bEnabled = true;
            Data.bFuseCas = bFuseCas;
            Data.K = Constants.Tonemap;
            Data.K.EnableAutoExposure = bAutoExposure ? 1u : 0u;
            Data.Cas = CasK;
            Data.ExposureEv = bAutoExposure ? Res.Luminance[WriteIndex] : nullptr;
            Data.Output = bCas && !bFuseCas ? Res.TonemapScratch : Res.TonemapBand;
            Data.bHalo = bFromRecords && bFuseCas;
            Data.HaloAbove = HaloAbove;
            Data.HaloBelow = HaloBelow;
            Data.Input = bTaa ? Res.TaaHistory[Taa.Write] : Res.LightingBand;
            Data.bFuseTaa = bFuseTaa;
            Data.bTaaHalo = bFuseTaa && bTaaRecords;
            Data.TaaHistoryWeight = Constants.TaaHistoryWeight;
            Data.TaaUseHistory = Taa.bUseHistory ? 1u : 0u;
            Data.TaaReadIndex = Taa.Read;
            Data.TaaWriteIndex = Taa.Write;
            if (bFuseTaa) { // the TemporalAA pass's usages move here
                Builder.ReadTexture(LightingHandle, RG_STATE_NON_PIXEL_SHADER_RESOURCE);
                if (Taa.Read != Taa.Write) Builder.ReadTexture(TaaReadHandle, RG_STATE_NON_PIXEL_SHADER_RESOURCE);
                DeclareTaaBandRows(Builder);
                Builder.WriteTexture(TaaWriteHandle, RG_STATE_UNORDERED_ACCESS);
            } else {
                Builder.ReadTexture(bTaa ? TaaWriteHandle : LightingHandle, RG_STATE_PIXEL_SHADER_RESOURCE);
            }
            if (Data.bHalo) Builder.ReadTexture(bTaaRecords ? TaaHaloHandle : RecordsHandle, RG_STATE_PIXEL_SHADER_RESOURCE);
            if (bAutoExposure) Builder.ReadTexture(LuminanceHandles[WriteIndex], RG_STATE_PIXEL_SHADER_RESOURCE);
            Builder.WriteTexture(bCas && !bFuseCas ? ScratchHandle : TonemapHandle, RG_STATE_RENDER_TARGET);
        }, [this, &Res, TaaRows](const FTonemapPassData& Data, FHIPCommandContext& Cmd)
        {
            const int rc = Data.bTaaHalo
                ? ur_temporal_aa_tonemap_halo(Cmd.GetContext(), &Data.K, Res.LightingBand, TaaRows.CurAbove, TaaRows.CurBelow, Res.TaaHistory[Data.TaaReadIndex],
                                              Res.TaaHistory[Data.TaaWriteIndex], Data.ExposureEv, Data.Output, TaaRows.Above2, TaaRows.HistAbove, TaaRows.Below2,
                                              TaaRows.HistBelow, TaaRows.ResolvedAbove, TaaRows.ResolvedBelow, Data.TaaHistoryWeight, Data.TaaUseHistory, Res.Width,
                                              Res.Height, Res.Row0, Res.Rows)
                : Data.bFuseTaa
                ? ur_temporal_aa_tonemap(Cmd.GetContext(), &Data.K, Res.LightingBand, Res.TaaHistory[Data.TaaReadIndex], Res.TaaHistory[Data.TaaWriteIndex],
                                         Data.ExposureEv, Data.Output, Data.TaaHistoryWeight, Data.TaaUseHistory, Res.Width, Res.Height, 0, Res.Height)
                : Data.bHalo
                ? ur_tonemap_cas_halo(Cmd.GetContext(), &Data.K, &Data.Cas, Data.Input, Data.HaloAbove, Data.HaloBelow, Data.ExposureEv, Data.Output, Res.Width,
                                      Res.Height, Res.Row0, Res.Rows)
                : Data.bFuseCas
                ? ur_tonemap_cas(Cmd.GetContext(), &Data.K, &Data.Cas, Data.Input, Data.ExposureEv, Data.Output, Res.Width, Res.Height, Res.Row0, Res.Rows)
                : ur_tonemap(Cmd.GetContext(), &Data.K, Data.Input, Data.ExposureEv, Data.Output, Res.Width, Res.Rows);
            if (rc != UR_OK && PassError == UR_OK) PassError = rc;
            Res.LightingState = RG_STATE_RENDER_TARGET; // the reference transitions the lighting buffer back (:1511-1512)
        });
        if (bCas) {
            // fused: still in the graph, disabled and culled, like Sky under bFuseLightingAndSky
            Graph.AddPass<FCasPassData>("CAS", [&](FCasPassData& Data, FRGPassBuilder& Builder)
            {
                Data.bEnabled = !bFuseCas;
                Data.K = CasK;
                if (!Data.bEnabled) return;
                Data.bHalo = bFromRecords;
                Data.Tonemap = Constants.Tonemap;
                Data.Tonemap.EnableAutoExposure = bAutoExposure ? 1u : 0u;
                Data.ExposureEv = bAutoExposure ? Res.Luminance[WriteIndex] : nullptr;
                Data.HaloAbove = HaloAbove;
                Data.HaloBelow = HaloBelow;
                Builder.ReadTexture(ScratchHandle, RG_STATE_PIXEL_SHADER_RESOURCE);
                if (Data.bHalo) {
                    Builder.ReadTexture(bTaaRecords ? TaaHaloHandle : RecordsHandle, RG_STATE_PIXEL_SHADER_RESOURCE);
                    if (bAutoExposure) Builder.ReadTexture(LuminanceHandles[WriteIndex], RG_STATE_PIXEL_SHADER_RESOURCE);
                }
                Builder.WriteTexture(TonemapHandle, RG_STATE_RENDER_TARGET);
            }, [this, &Res](const FCasPassData& Data, FHIPCommandContext& Cmd)
            {
                if (!Data.bEnabled) return;
                const int rc = Data.bHalo
                    ? ur_cas_halo(Cmd.GetContext(), &Data.Tonemap, &Data.K, Res.TonemapScratch, Data.HaloAbove, Data.HaloBelow, Data.ExposureEv, Res.TonemapBand,
                                  Res.Width, Res.Height, Res.Row0, Res.Rows)
                    : ur_cas(Cmd.GetContext(), &Data.K, Res.TonemapScratch, Res.TonemapBand, Res.Width, Res.Height, Res.Row0, Res.Rows);
                if (rc != UR_OK && PassError == UR_OK) PassError = rc;
            });
        }
        // ---- GpuDebugPrint (:1575-1598): last in the frame, DispatchGpuDebugPrintStats then RenderGpuDebugPrint onto the back buffer.
        // On a band the draw composites the part of the text inside it.
        struct FDebugPrintPassData
        {
            bool bEnabled = false;
            ur_debug_print_constants K = {};
        };
        if (DebugBufferHandle) {
            Graph.AddPass<FDebugPrintPassData>("GpuDebugPrint", [&](FDebugPrintPassData& Data, FRGPassBuilder& Builder)
            {
                Data.bEnabled = true;
                Data.K.ScreenSize[0] = static_cast<float>(Res.Width);
                Data.K.ScreenSize[1] = static_cast<float>(Res.Height);
                Data.K.FirstChar = Res.DebugFirstChar;
                Data.K.CharCount = Res.DebugCharCount;
                Builder.ReadTexture(DebugStatsHandle, RG_STATE_NON_PIXEL_SHADER_RESOURCE);
                Builder.WriteTexture(DebugBufferHandle, RG_STATE_UNORDERED_ACCESS);
                Builder.WriteTexture(TonemapHandle, RG_STATE_RENDER_TARGET);
            }, [this, &Res](const FDebugPrintPassData& Data, FHIPCommandContext& Cmd)
            {
                int rc = ur_debug_print_stats(Cmd.GetContext(), Res.CullStats, Res.DebugPrintBuffer);
                if (rc == UR_OK)
                    rc = ur_debug_print_draw(Cmd.GetContext(), &Data.K, Res.DebugGlyphs, Res.DebugGlyphCount, Res.DebugAtlas, Res.DebugAtlasWidth, Res.DebugAtlasHeight,
                                             Res.DebugPrintBuffer, Res.TonemapBand, Res.Width, Res.Height, Res.Row0, Res.Rows);
                if (rc != UR_OK && PassError == UR_OK) PassError = rc;
            });
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// C face
// ---------------------------------------------------------------------------------------------------------------------
// The draws of a raster pass as the frame keeps them: the caller's struct and a copy of its ranges, which Draws.ranges refers to. It points
// into itself: it lives in ur_frame, which is never copied.
struct FRasterPassBinding
{
    ur_raster_draws Draws = {};
    ur_draw_ranges Ranges = {};
    bool bSet = false;
    void Set(const ur_raster_draws& In) { Draws = In; Ranges = In.ranges ? *In.ranges : ur_draw_ranges{}; Draws.ranges = In.ranges ? &Ranges : nullptr; bSet = true; }
    void Clear() { Draws = ur_raster_draws{}; Ranges = ur_draw_ranges{}; bSet = false; }
    bool IsSet() const { return bSet; }
};

struct ur_frame
{
    FHIPDevice Device;
    FHIPCommandContext Cmd;
    FHotPathRenderer Renderer;
    FHotPathResources Res;
    hipStream_t AsyncStream = nullptr;
    ur_ctx* AsyncCtx = nullptr;
    int DeviceIndex = 0;
    struct FLightEvents { hipEvent_t first, second, after; bool has_after; bool on_dispatch; };
    std::vector<FLightEvents> LightEvents; // ring: an event pair around the Lighting pass + one more right behind it (what a record costs)
    size_t LightHead = 0, LightCount = 0;
    bool bRecordAfter = false; // this frame's bracket gets the third event (UR_FRAME_TIME_LIGHTING_RECORD_COST)
    bool bKernelEvents = false; // UR_FRAME_TIME_LIGHTING_KERNEL: the pair rides on the Lighting dispatch itself, nothing is recorded around it
    bool bStartOnCull = false;  // ... and this frame's START event was handed to the cull launch directly in front of the Lighting launch
    ur_frame_post Post = {{nullptr, nullptr}, nullptr, 0.0f, 0.9f, 2.2f, 0.3f, 0.1f, 5.0f, 3.0f, 1.0f, 0.5f}; // ur_frame_set_post
    ur_draw_ranges DrawRanges = {};    // ur_frame_set_draw_ranges
    bool bDrawRanges = false;
    ur_cull_view CullViews[UR_MAX_CULL_VIEWS] = {};  // ur_frame_set_cull_views (draws point into ViewDraws)
    ur_draw_ranges ViewDraws[UR_MAX_CULL_VIEWS] = {};
    uint32_t CullViewCount = 0;
    std::vector<ur_half4*> TaaHistory; // ur_frame_set_taa
    float TaaHistoryWeight = 0.9f;
    void* PostRecord = nullptr;        // ur_frame_set_post_records
    const void* PostRecords = nullptr;
    void* TaaRecord = nullptr;         // ur_frame_set_taa_records
    const void* TaaRecords = nullptr;
    ur_frame_debug_print DebugPrint = {}; // ur_frame_set_debug_print
    FRasterPassBinding ShadowDraws, DepthDraws, GBufferDraws; // ur_frame_set_shadow_pass / _depth_pass / _gbuffer_pass: the draws ...
    FShadowPassResources ShadowPass;                          // ... and the rest of each pass (Draws points at its binding's)
    FDepthPassResources DepthPass;
    FGBufferPassResources GBufferPass;
    const ur_material* GBufferMaterials = nullptr; // ur_frame_set_gbuffer_materials: the "GBuffer" pass resolves with them
    uint32_t GBufferMaterialCount = 0;
    ur_half4* TaaHaloRows = nullptr;   // the frame's own: 2 x TaaHaloWidth texels, the resolved rows around the band (UR_FRAME_TAA_BAND with CAS)
    uint32_t TaaHaloWidth = 0;
    ur_frame(ur_ctx* Ctx, hipStream_t Stream, uint32 Frames, int Rank, int World) : Cmd(Ctx, Stream, Frames, Rank, World), Renderer(&Device) {}
    ur_frame(const ur_frame&) = delete; // (CullViews and the bindings point into the frame)
    ur_frame& operator=(const ur_frame&) = delete;
};

extern "C" {

// rows [row0, row0 + rows) are rank's band of `world_size` equal bands of a frame of `height` rows (dist.plan_bands)
static bool equal_band(const ur_frame* f, uint32_t height, uint32_t row0, uint32_t rows)
{
    const int world = f->Cmd.GetWorldSize(), rank = f->Cmd.GetRank();
    if (world < 1 || rank < 0 || rank >= world || height % static_cast<uint32_t>(world) != 0) return false;
    const uint32_t band = height / static_cast<uint32_t>(world);
    return rows == band && row0 == static_cast<uint32_t>(rank) * band;
}

ur_frame* ur_frame_create(ur_ctx* ctx, void* stream, uint32_t frames_in_flight, int rank, int world_size)
{
    if (!ctx) return nullptr;
    ur_frame* f = new ur_frame(ctx, static_cast<hipStream_t>(stream), frames_in_flight, rank, world_size);
    f->Renderer.SetLightingTimer([f](hipStream_t s, bool begin) {
        constexpr size_t kRing = 1024;
        if (f->LightEvents.size() < kRing && begin && f->LightCount == f->LightEvents.size()) {
            hipEvent_t a = nullptr, b = nullptr, c = nullptr;
            if (hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess && hipEventCreate(&c) == hipSuccess) f->LightEvents.push_back({a, b, c, false, false});
        }
        if (f->LightEvents.empty()) return;
        if (f->bKernelEvents) {
            if (begin) {
                f->LightHead = f->LightCount % f->LightEvents.size();
                // stop = bound to the Lighting kernel's own dispatch (its completion signal's end stamp). start = the end stamp of the
                // dispatch directly in front of it when that is this frame's cull launch (ur_frame_render handed it the event: NOTHING
                // enters the queue for the measurement), else a marker the runtime puts in front of the kernel (~8 us of queue time).
                // (One event alone measures nothing on this runtime: hipEventElapsedTime(e, e) is 0.)
                // (a cull call that launched nothing took no event: the marker form then, never a stamp left over from an earlier use of the slot)
                if (f->bStartOnCull && !ur_time_cull_carried(f->Cmd.GetContext())) f->bStartOnCull = false;
                (void)ur_time_next_lighting(f->Cmd.GetContext(), f->bStartOnCull ? nullptr : f->LightEvents[f->LightHead].first, f->LightEvents[f->LightHead].second);
            } else {
                (void)ur_time_next_lighting(f->Cmd.GetContext(), nullptr, nullptr); // (a launch that failed validation consumed nothing)
                f->LightEvents[f->LightHead].has_after = false;
                f->LightEvents[f->LightHead].on_dispatch = true;
                ++f->LightCount;
            }
            return;
        }
        if (begin) {
            f->LightHead = f->LightCount % f->LightEvents.size();
            (void)hipEventRecord(f->LightEvents[f->LightHead].first, s);
        } else {
            (void)hipEventRecord(f->LightEvents[f->LightHead].second, s);
            // a third record with nothing in front of it: second -> after is what one event record adds to the bracket
            f->LightEvents[f->LightHead].has_after = f->bRecordAfter;
            f->LightEvents[f->LightHead].on_dispatch = false;
            if (f->bRecordAfter) (void)hipEventRecord(f->LightEvents[f->LightHead].after, s);
            ++f->LightCount;
        }
    });
    return f;
}

uint32_t ur_frame_lighting_times_ex(ur_frame* f, float* out_ms, float* out_record_ms, uint32_t cap)
{
    if (!f) return 0;
    const size_t n = f->LightCount < f->LightEvents.size() ? f->LightCount : f->LightEvents.size();
    uint32_t k = 0;
    for (size_t i = 0; i < n && k < cap; ++i) {
        float ms = 0.0f, rec = 0.0f;
        if (hipEventElapsedTime(&ms, f->LightEvents[i].first, f->LightEvents[i].second) != hipSuccess) continue;
        if (out_record_ms) {
            rec = -1.0f; // no third event on this sample
            if (f->LightEvents[i].has_after && hipEventElapsedTime(&rec, f->LightEvents[i].second, f->LightEvents[i].after) != hipSuccess) rec = -1.0f;
            out_record_ms[k] = rec;
        }
        out_ms[k++] = ms;
    }
    f->LightCount = 0;
    return k;
}

uint32_t ur_frame_lighting_times(ur_frame* f, float* out_ms, uint32_t cap) { return ur_frame_lighting_times_ex(f, out_ms, nullptr, cap); }

void ur_frame_destroy(ur_frame* f)
{
    if (!f) return;
    if (f->AsyncStream) (void)hipStreamSynchronize(f->AsyncStream);
    if (f->AsyncCtx) ur_destroy(f->AsyncCtx);
    if (f->AsyncStream) (void)hipStreamDestroy(f->AsyncStream);
    for (auto& e : f->LightEvents) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); (void)hipEventDestroy(e.after); }
    if (f->TaaHaloRows) (void)hipFree(f->TaaHaloRows);
    delete f;
}

int ur_frame_render(ur_frame* f, const ur_frame_resources* r, const uint32_t* culling_constants, const ur_scene_constants* scene,
                    const ur_sky_constants* sky, uint32_t flags)
{
    if (!f || !r || !culling_constants || !scene || !sky) return UR_EINVAL;
    const uint32_t post_flags = UR_FRAME_AUTO_EXPOSURE | UR_FRAME_CAS | UR_FRAME_FUSE_TONEMAP_CAS;
    if (flags & post_flags) {
        const bool cas_pass = (flags & UR_FRAME_CAS) && !(flags & UR_FRAME_FUSE_TONEMAP_CAS);
        if (!(flags & UR_FRAME_TONEMAP) || !r->tonemap_band) { ur::set_error("ur_frame_render: AUTO_EXPOSURE / CAS need UR_FRAME_TONEMAP and a tonemap_band"); return UR_EINVAL; }
        if ((flags & UR_FRAME_AUTO_EXPOSURE) && (!f->Post.luminance[0] || !f->Post.luminance[1])) { ur::set_error("ur_frame_render: AUTO_EXPOSURE needs ur_frame_set_post's luminance[2]"); return UR_EINVAL; }
        if (cas_pass && !f->Post.tonemap_scratch) { ur::set_error("ur_frame_render: a CAS pass of its own needs ur_frame_set_post's tonemap_scratch"); return UR_EINVAL; }
        const bool exchange = (flags & UR_FRAME_POST_EXCHANGE) && (flags & (UR_FRAME_AUTO_EXPOSURE | UR_FRAME_CAS));
        if ((flags & (UR_FRAME_AUTO_EXPOSURE | UR_FRAME_CAS)) && !exchange && (r->row0 != 0 || r->rows != r->height)) {
            ur::set_error("ur_frame_render: AutoExposure and CAS need the whole frame (rows == height), or UR_FRAME_POST_EXCHANGE on a band");
            return UR_EUNSUPPORTED;
        }
        if (exchange) {
            if (!f->PostRecord || !f->PostRecords) { ur::set_error("ur_frame_render: POST_EXCHANGE needs ur_frame_set_post_records"); return UR_EINVAL; }
            if (!equal_band(f, r->height, r->row0, r->rows)) {
                ur::set_error("ur_frame_render: POST_EXCHANGE needs rank's equal band (world_size | height)");
                return UR_EINVAL;
            }
        }
    }
    if (flags & (UR_FRAME_TAA | UR_FRAME_FUSE_TAA_TONEMAP)) {
        if (!(flags & UR_FRAME_TAA)) { ur::set_error("ur_frame_render: FUSE_TAA_TONEMAP needs UR_FRAME_TAA"); return UR_EINVAL; }
        if (!(flags & UR_FRAME_TONEMAP) || !r->tonemap_band) { ur::set_error("ur_frame_render: TAA needs UR_FRAME_TONEMAP and a tonemap_band"); return UR_EINVAL; }
        if (f->TaaHistory.empty()) { ur::set_error("ur_frame_render: TAA needs ur_frame_set_taa's history ring"); return UR_EINVAL; }
        if ((flags & UR_FRAME_FUSE_TAA_TONEMAP) && (flags & UR_FRAME_FUSE_TONEMAP_CAS)) {
            ur::set_error("ur_frame_render: FUSE_TAA_TONEMAP and FUSE_TONEMAP_CAS exclude each other (TAA + Tonemap + CAS in one launch is not built)");
            return UR_EINVAL;
        }
        if (!(flags & UR_FRAME_TAA_BAND) && ((flags & UR_FRAME_POST_EXCHANGE) || r->row0 != 0 || r->rows != r->height)) {
            ur::set_error("ur_frame_render: TAA needs the whole frame (rows == height, no UR_FRAME_POST_EXCHANGE), or UR_FRAME_TAA_BAND");
            return UR_EUNSUPPORTED;
        }
    }
    if (flags & UR_FRAME_TAA_BAND) {
        if (!(flags & UR_FRAME_TAA) || !(flags & UR_FRAME_POST_EXCHANGE)) { ur::set_error("ur_frame_render: TAA_BAND needs UR_FRAME_TAA and UR_FRAME_POST_EXCHANGE"); return UR_EINVAL; }
        if (!f->PostRecord || !f->PostRecords) { ur::set_error("ur_frame_render: TAA_BAND needs ur_frame_set_post_records"); return UR_EINVAL; }
        if (!f->TaaRecord || !f->TaaRecords) { ur::set_error("ur_frame_render: TAA_BAND needs ur_frame_set_taa_records"); return UR_EINVAL; }
        if (!equal_band(f, r->height, r->row0, r->rows)) {
            ur::set_error("ur_frame_render: TAA_BAND needs rank's equal band (world_size | height)");
            return UR_EINVAL;
        }
        if (r->rows < 2u && f->Cmd.GetWorldSize() > 1) { ur::set_error("ur_frame_render: TAA_BAND needs bands of at least 2 rows"); return UR_EUNSUPPORTED; }
        if ((flags & UR_FRAME_CAS) && (!f->TaaHaloRows || f->TaaHaloWidth < r->width)) { // the resolved rows around the band: the frame's own
            if (f->TaaHaloRows) { (void)hipStreamSynchronize(f->Cmd.GetStream()); (void)hipFree(f->TaaHaloRows); f->TaaHaloRows = nullptr; f->TaaHaloWidth = 0; }
            void* rows2 = nullptr;
            if (hipMalloc(&rows2, static_cast<size_t>(r->width) * 2u * sizeof(ur_half4)) != hipSuccess) { ur::set_error("ur_frame_render: no memory for the resolved rows of TAA_BAND"); return UR_ENOMEM; }
            f->TaaHaloRows = static_cast<ur_half4*>(rows2);
            f->TaaHaloWidth = r->width;
        }
    }
    if (flags & UR_FRAME_DEBUG_PRINT) {
        if (!(flags & UR_FRAME_TONEMAP) || !r->tonemap_band) { ur::set_error("ur_frame_render: DEBUG_PRINT needs UR_FRAME_TONEMAP and a tonemap_band"); return UR_EINVAL; }
        if (!r->cull_stats) { ur::set_error("ur_frame_render: DEBUG_PRINT needs cull_stats"); return UR_EINVAL; }
        if (!f->DebugPrint.buffer) { ur::set_error("ur_frame_render: DEBUG_PRINT needs ur_frame_set_debug_print's buffer and font"); return UR_EINVAL; }
    }
    if (flags & UR_FRAME_SHADOW_PASS) {
        if (!f->ShadowDraws.IsSet()) { ur::set_error("ur_frame_render: SHADOW_PASS needs ur_frame_set_shadow_pass"); return UR_EINVAL; }
        if ((flags & UR_FRAME_SHADOWS) && r->tables.shadow_map != f->ShadowPass.Map) {
            ur::set_error("ur_frame_render: SHADOW_PASS renders into ur_frame_set_shadow_pass' shadow_map, Lighting reads tables.shadow_map: they must be the same buffer");
            return UR_EINVAL;
        }
    }
    if (flags & UR_FRAME_DEPTH_PASS) {
        if (!f->DepthDraws.IsSet()) { ur::set_error("ur_frame_render: DEPTH_PASS needs ur_frame_set_depth_pass"); return UR_EINVAL; }
        if (r->depth_full != f->DepthPass.Depth) {
            ur::set_error("ur_frame_render: DEPTH_PASS renders into ur_frame_set_depth_pass' depth, Build HZB reads depth_full: they must be the same buffer");
            return UR_EINVAL;
        }
    }
    if (flags & UR_FRAME_GBUFFER_PASS) {
        if (!(flags & UR_FRAME_DEPTH_PASS)) { ur::set_error("ur_frame_render: GBUFFER_PASS needs UR_FRAME_DEPTH_PASS: the base pass tests against the prepass' depth"); return UR_EINVAL; }
        if (!f->GBufferDraws.IsSet()) { ur::set_error("ur_frame_render: GBUFFER_PASS needs ur_frame_set_gbuffer_pass"); return UR_EINVAL; }
        if (f->GBufferPass.Flags != f->DepthPass.Flags) {
            ur::set_error("ur_frame_render: GBUFFER_PASS and DEPTH_PASS must quantise alike (flags 0x%x and 0x%x)", f->GBufferPass.Flags, f->DepthPass.Flags);
            return UR_EINVAL;
        }
        const ur_gbuffer_targets& T = f->GBufferPass.Targets;
        if (T.gbuf_a != r->gbuffer_a || T.gbuf_b != r->gbuffer_b || T.gbuf_c != r->gbuffer_c || T.hdr != r->lighting_band) {
            ur::set_error("ur_frame_render: GBUFFER_PASS renders into ur_frame_set_gbuffer_pass' targets, Lighting reads gbuffer_a/b/c and adds to lighting_band: they must be the same buffers");
            return UR_EINVAL;
        }
    }
    FHotPathResources& R = f->Res; // resource states persist across frames, like the renderer's member variables
    R.Width = r->width; R.Height = r->height; R.Row0 = r->row0; R.Rows = r->rows;
    R.GBufferA = const_cast<ur_half4*>(r->gbuffer_a);
    R.GBufferB = const_cast<ur_half4*>(r->gbuffer_b);
    R.GBufferC = const_cast<uint32*>(r->gbuffer_c);
    R.DepthBand = const_cast<float*>(r->depth_band);
    R.LightingBand = r->lighting_band;
    R.TonemapBand = r->tonemap_band;
    R.TonemapScratch = f->Post.tonemap_scratch;
    R.Luminance[0] = f->Post.luminance[0];
    R.Luminance[1] = f->Post.luminance[1];
    R.PostRecord = f->PostRecord;
    R.PostRecords = f->PostRecords;
    R.TaaRecord = f->TaaRecord;
    R.TaaRecords = f->TaaRecords;
    R.TaaHaloRows = f->TaaHaloRows;
    R.TaaHistory = f->TaaHistory; // (RenderFrame sizes TaaHistoryStates)
    R.DepthFull = const_cast<float*>(r->depth_full);
    R.HZB = r->hzb;
    std::memcpy(R.HZBMips, r->hzb_mips, sizeof(R.HZBMips));
    R.HZBMipCount = r->hzb_mip_count;
    R.Tables = r->tables;
    R.ModelBounds = const_cast<ur_float4*>(r->model_bounds);
    R.IndirectArgs = r->indirect_args;
    R.IndirectCommandCount = r->indirect_command_count;
    R.InstanceIndexBase = r->instance_index_base;
    R.VisibleIndices = r->visible_indices;
    R.VisibleCount = r->visible_count;
    R.CullStats = r->cull_stats;
    R.DrawRanges = f->bDrawRanges ? &f->DrawRanges : nullptr;
    R.CullViews = f->CullViews;
    R.CullViewCount = (flags & UR_FRAME_CULL_VIEWS) ? f->CullViewCount : 0u;
    R.DebugPrintBuffer = f->DebugPrint.buffer;
    R.DebugGlyphs = f->DebugPrint.glyphs;
    R.DebugGlyphCount = f->DebugPrint.glyph_count;
    R.DebugAtlas = f->DebugPrint.atlas;
    R.DebugAtlasWidth = f->DebugPrint.atlas_w;
    R.DebugAtlasHeight = f->DebugPrint.atlas_h;
    R.DebugFirstChar = f->DebugPrint.first_char;
    R.DebugCharCount = f->DebugPrint.char_count;
    R.ShadowPass = (flags & UR_FRAME_SHADOW_PASS) ? f->ShadowPass : FShadowPassResources{}; // (a flag without its pass, or GBUFFER_PASS without DEPTH_PASS, was refused above)
    R.DepthPass = (flags & UR_FRAME_DEPTH_PASS) ? f->DepthPass : FDepthPassResources{};
    R.GBufferPass = (flags & UR_FRAME_GBUFFER_PASS) ? f->GBufferPass : FGBufferPassResources{};
    R.GBufferMaterials = f->GBufferMaterials; // (read by the "GBuffer" pass alone)
    R.GBufferMaterialCount = f->GBufferMaterialCount;

    FHotPathFrameConstants K;
    std::memcpy(K.CullingConstants, culling_constants, sizeof(K.CullingConstants));
    K.Scene = *scene;
    K.Sky = *sky;
    K.Tonemap.Exposure = f->Post.tonemap_exposure;
    K.Tonemap.Gamma = f->Post.tonemap_gamma;
    K.DeltaTime = f->Post.delta_time;
    K.AutoExposureKey = f->Post.ae_key;
    K.AutoExposureMin = f->Post.ae_min;
    K.AutoExposureMax = f->Post.ae_max;
    K.AutoExposureSpeedUp = f->Post.ae_speed_up;
    K.AutoExposureSpeedDown = f->Post.ae_speed_down;
    K.CasSharpness = f->Post.cas_sharpness;
    K.TaaHistoryWeight = f->TaaHistoryWeight;
    FHotPathOptions O;
    O.bEnableIndirectDraw = (flags & UR_FRAME_INDIRECT_DRAW) != 0;
    O.bHZBEnabled = (flags & UR_FRAME_HZB) != 0;
    O.bDoDepthPrepass = (flags & UR_FRAME_DEPTH_PREPASS) != 0;
    O.bRenderShadows = (flags & UR_FRAME_SHADOWS) != 0;
    O.bSkyEnabled = (flags & UR_FRAME_SKY) != 0;
    O.bFuseLightingAndSky = (flags & UR_FRAME_FUSE_LIGHTING_SKY) != 0;
    O.bTonemap = (flags & UR_FRAME_TONEMAP) != 0;
    O.bAutoExposure = (flags & UR_FRAME_AUTO_EXPOSURE) != 0;
    O.bCas = (flags & UR_FRAME_CAS) != 0;
    O.bFuseTonemapCas = (flags & UR_FRAME_FUSE_TONEMAP_CAS) != 0;
    O.bPostExchange = (flags & UR_FRAME_POST_EXCHANGE) != 0;
    O.bTaa = (flags & UR_FRAME_TAA) != 0;
    O.bFuseTaaTonemap = (flags & UR_FRAME_FUSE_TAA_TONEMAP) != 0;
    O.bTaaBand = (flags & UR_FRAME_TAA_BAND) != 0;
    O.bDebugPrint = (flags & UR_FRAME_DEBUG_PRINT) != 0;
    O.bShardHZB = (flags & UR_FRAME_HZB_SHARD) != 0 && f->Cmd.GetWorldSize() > 1;
    O.bAsyncCompute = (flags & UR_FRAME_ASYNC_COMPUTE) != 0;
    if (O.bAsyncCompute && !f->AsyncCtx) { // second stream + a context bound to it, created on first use
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipStreamCreateWithPriority(&f->AsyncStream, hipStreamNonBlocking, -1) != hipSuccess) return UR_EHIP; // high priority: its short kernels slot in beside the lighting kernel
        f->AsyncCtx = ur_create(dev, f->AsyncStream);
        if (!f->AsyncCtx) return UR_EHIP;
        f->Cmd.SetAsyncCompute(f->AsyncCtx, f->AsyncStream);
    }
    O.bTimeLighting = (flags & (UR_FRAME_TIME_LIGHTING | UR_FRAME_TIME_LIGHTING_RECORD_COST | UR_FRAME_TIME_LIGHTING_KERNEL)) != 0;
    f->bKernelEvents = (flags & UR_FRAME_TIME_LIGHTING_KERNEL) != 0;
    f->bRecordAfter = (flags & UR_FRAME_TIME_LIGHTING_RECORD_COST) != 0;
    O.bGpuTiming = (flags & UR_FRAME_GPU_TIMING) != 0;
    O.bGraphDump = (flags & UR_FRAME_GRAPH_DUMP) != 0;
    O.bBarrierLogs = (flags & UR_FRAME_BARRIER_LOGS) != 0;
    f->Cmd.SetJoinAsyncAtEnd((flags & UR_FRAME_ASYNC_NO_JOIN) == 0);
    f->Cmd.BeginFrame();
    // Launch scheduling across two passes (include/ur_hotpath.h, ur_defer_hzb_tail): only when both run on the main stream
    const bool chain_with_lighting = (flags & UR_FRAME_HZB_WITH_LIGHTING) != 0 && !O.bAsyncCompute;
    const bool tail_with_lighting = (chain_with_lighting || (flags & UR_FRAME_HZB_TAIL_WITH_LIGHTING) != 0) && !O.bAsyncCompute;
    if (tail_with_lighting) (void)ur_defer_hzb_tail(f->Cmd.GetContext(), chain_with_lighting ? 2 : 1);
    f->bStartOnCull = false;
    if (f->bKernelEvents && chain_with_lighting && O.bEnableIndirectDraw && O.bHZBEnabled && O.bDoDepthPrepass && R.IndirectArgs && R.ModelBounds &&
        R.IndirectCommandCount != 0) {
        // Two launches in this frame, the cull and the Lighting launch that carries Build HZB: the cull's own completion stamp is the
        // start of the Lighting measurement. (Events of the ring are created here if this is its first use.)
        constexpr size_t kRing = 1024;
        if (f->LightEvents.size() < kRing && f->LightCount == f->LightEvents.size()) {
            hipEvent_t a = nullptr, b = nullptr, c = nullptr;
            if (hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess && hipEventCreate(&c) == hipSuccess) f->LightEvents.push_back({a, b, c, false, false});
        }
        if (!f->LightEvents.empty() && ur_time_next_cull(f->Cmd.GetContext(), f->LightEvents[f->LightCount % f->LightEvents.size()].first) == UR_OK)
            f->bStartOnCull = true;
    }
    const int rc = f->Renderer.RenderFrame(f->Cmd, R, K, O);
    (void)ur_time_next_cull(f->Cmd.GetContext(), nullptr); // (a frame whose cull pass did not run consumed nothing)
    if (tail_with_lighting) {
        const int rc2 = ur_defer_hzb_tail(f->Cmd.GetContext(), 0); // launches the tail on its own if no Lighting launch took it
        // a riding tail that gave up waiting (a bounded wait inside an earlier Lighting launch) is reported here, once: UR_ETIMEOUT
        const int rc3 = ur_flush(f->Cmd.GetContext());
        return rc != UR_OK ? rc : (rc2 != UR_OK ? rc2 : rc3);
    }
    return rc;
}

void ur_frame_join_async(ur_frame* f) { if (f) f->Cmd.JoinAsyncCompute(); }
int ur_frame_hzb_ready(const ur_frame* f) { return f && f->Renderer.IsHZBReady() ? 1 : 0; }
void ur_frame_reset_hzb(ur_frame* f) { if (f) f->Renderer.ResetHZB(); }

int ur_frame_set_post(ur_frame* f, const ur_frame_post* post)
{
    if (!f || !post) { ur::set_error("ur_frame_set_post: null argument"); return UR_EINVAL; }
    f->Post = *post;
    return UR_OK;
}

int ur_frame_set_draw_ranges(ur_frame* f, const ur_draw_ranges* draws)
{
    if (!f) { ur::set_error("ur_frame_set_draw_ranges: null frame"); return UR_EINVAL; }
    if (draws && (!draws->offsets || !draws->commands || !draws->counts || draws->range_count == 0)) {
        ur::set_error("ur_frame_set_draw_ranges: null member / no range");
        return UR_EINVAL;
    }
    f->bDrawRanges = draws != nullptr;
    f->DrawRanges = draws ? *draws : ur_draw_ranges{};
    return UR_OK;
}

int ur_frame_set_cull_views(ur_frame* f, const ur_cull_view* views, uint32_t count)
{
    if (!f) { ur::set_error("ur_frame_set_cull_views: null frame"); return UR_EINVAL; }
    if (count > UR_MAX_CULL_VIEWS) { ur::set_error("ur_frame_set_cull_views: %u views (at most %u)", count, (uint32_t)UR_MAX_CULL_VIEWS); return UR_EINVAL; }
    if (count != 0 && !views) { ur::set_error("ur_frame_set_cull_views: null views"); return UR_EINVAL; }
    const int rc = ur::check_cull_views(views, count);
    if (rc != UR_OK) return rc;
    for (uint32_t v = 0; v < count; ++v) {
        f->CullViews[v] = views[v];
        f->ViewDraws[v] = views[v].draws ? *views[v].draws : ur_draw_ranges{};
        f->CullViews[v].draws = views[v].draws ? &f->ViewDraws[v] : nullptr;
    }
    f->CullViewCount = count;
    return UR_OK;
}

int ur_frame_set_debug_print(ur_frame* f, const ur_frame_debug_print* dp)
{
    if (!f) { ur::set_error("ur_frame_set_debug_print: null frame"); return UR_EINVAL; }
    if (dp && (!dp->buffer || !dp->glyphs || dp->glyph_count == 0 || !dp->atlas || dp->atlas_w == 0 || dp->atlas_h == 0)) {
        ur::set_error("ur_frame_set_debug_print: null buffer / glyphs / atlas, or an empty table or atlas");
        return UR_EINVAL;
    }
    f->DebugPrint = dp ? *dp : ur_frame_debug_print{};
    return UR_OK;
}

int ur_frame_set_depth_pass(ur_frame* f, const ur_frame_depth_pass* pass)
{
    if (!f) { ur::set_error("ur_frame_set_depth_pass: null frame"); return UR_EINVAL; }
    if (!pass) { f->DepthDraws.Clear(); f->DepthPass = {}; return UR_OK; }
    int rc = ur::check_raster_draws("ur_frame_set_depth_pass", pass->draws, pass->depth, "depth", pass->stats6);
    if (rc == UR_OK) rc = ur::check_depth_flags("ur_frame_set_depth_pass", pass->flags);
    if (rc != UR_OK) return rc;
    f->DepthDraws.Set(pass->draws);
    f->DepthPass = {&f->DepthDraws.Draws, pass->depth, pass->stats6, pass->flags};
    return UR_OK;
}

int ur_frame_set_gbuffer_materials(ur_frame* f, const ur_material* materials, uint32_t material_count)
{
    if (!f) { ur::set_error("ur_frame_set_gbuffer_materials: null frame"); return UR_EINVAL; }
    if ((reinterpret_cast<uintptr_t>(materials) & 15u) != 0u) { ur::set_error("ur_frame_set_gbuffer_materials: a misaligned material table (16 bytes)"); return UR_EINVAL; }
    f->GBufferMaterials = materials;
    f->GBufferMaterialCount = materials ? material_count : 0u;
    return UR_OK;
}

int ur_frame_set_gbuffer_pass(ur_frame* f, const ur_frame_gbuffer_pass* pass)
{
    if (!f) { ur::set_error("ur_frame_set_gbuffer_pass: null frame"); return UR_EINVAL; }
    if (!pass) { f->GBufferDraws.Clear(); f->GBufferPass = {}; return UR_OK; }
    int rc = ur::check_gbuffer_targets("ur_frame_set_gbuffer_pass", &pass->targets); // (the keys are the target the raster writes: never null from here on)
    if (rc == UR_OK) rc = ur::check_raster_draws("ur_frame_set_gbuffer_pass", pass->draws, pass->targets.keys, "keys", pass->stats6);
    if (rc == UR_OK) rc = ur::check_depth_flags("ur_frame_set_gbuffer_pass", pass->flags);
    if (rc == UR_OK) rc = ur::check_key_triangle_bits("ur_frame_set_gbuffer_pass", pass->key_triangle_bits);
    if (rc != UR_OK) return rc;
    f->GBufferDraws.Set(pass->draws);
    f->GBufferPass = {&f->GBufferDraws.Draws, pass->targets, pass->stats6, pass->flags, pass->key_triangle_bits};
    return UR_OK;
}

int ur_frame_set_shadow_pass(ur_frame* f, const ur_frame_shadow_pass* pass)
{
    if (!f) { ur::set_error("ur_frame_set_shadow_pass: null frame"); return UR_EINVAL; }
    if (!pass) { f->ShadowDraws.Clear(); f->ShadowPass = {}; return UR_OK; }
    const int rc = ur::check_raster_draws("ur_frame_set_shadow_pass", pass->draws, pass->shadow_map, "shadow_map", pass->stats4);
    if (rc != UR_OK) return rc;
    f->ShadowDraws.Set(pass->draws);
    f->ShadowPass = {&f->ShadowDraws.Draws, pass->shadow_map, pass->stats4};
    return UR_OK;
}

void ur_frame_reset_post(ur_frame* f) { if (f) f->Renderer.ResetLuminanceHistory(); }

int ur_frame_set_taa(ur_frame* f, const ur_frame_taa* taa)
{
    if (!f) { ur::set_error("ur_frame_set_taa: null frame"); return UR_EINVAL; }
    if (taa) {
        if (!taa->history || taa->history_count != f->Cmd.GetFrameCount()) {
            ur::set_error("ur_frame_set_taa: %u history images, the frame has %u frames in flight", taa->history ? taa->history_count : 0u, f->Cmd.GetFrameCount());
            return UR_EINVAL;
        }
        for (uint32_t i = 0; i < taa->history_count; ++i)
            if (!taa->history[i]) { ur::set_error("ur_frame_set_taa: history[%u] is null", i); return UR_EINVAL; }
        f->TaaHistory.assign(taa->history, taa->history + taa->history_count);
        f->TaaHistoryWeight = taa->history_weight;
    } else {
        f->TaaHistory.clear();
        f->TaaHistoryWeight = 0.9f;
    }
    f->Renderer.ResetTaa(); // new images: all invalid at creation (CreateTaaResources)
    return UR_OK;
}

void ur_frame_reset_taa(ur_frame* f) { if (f) f->Renderer.ResetTaa(); }

int ur_frame_taa_next(const ur_frame* f, ur_frame_taa_info* info)
{
    if (!f || !info) { ur::set_error("ur_frame_taa_next: null argument"); return UR_EINVAL; }
    if (f->TaaHistory.empty()) { ur::set_error("ur_frame_taa_next: no history ring (ur_frame_set_taa)"); return UR_EINVAL; }
    // ur_frame_render begins the frame (BeginFrame: the next frame slot) before it reads the slot index
    const uint32_t next = (f->Cmd.GetCurrentFrameIndex() + 1u) % f->Cmd.GetFrameCount();
    const FHotPathRenderer::FTaaSlots s = f->Renderer.GetTaaSlots(next, static_cast<uint32_t>(f->TaaHistory.size()));
    info->read_slot = s.Read;
    info->write_slot = s.Write;
    info->use_history = s.bUseHistory ? 1u : 0u;
    info->jitter[0] = info->jitter[1] = 0.0f; // bUseTaaJitter = bTaaActive && bTaaHistoryReady (:403-411)
    if (s.bUseHistory) ur_host_taa_jitter(s.SampleIndex, info->jitter);
    return UR_OK;
}

int ur_frame_set_post_records(ur_frame* f, void* own_record, const void* all_records)
{
    if (!f || !own_record || !all_records) { ur::set_error("ur_frame_set_post_records: null argument"); return UR_EINVAL; }
    f->PostRecord = own_record;
    f->PostRecords = all_records;
    return UR_OK;
}

int ur_frame_set_taa_records(ur_frame* f, void* own_record, const void* all_records)
{
    if (!f || !own_record || !all_records) { ur::set_error("ur_frame_set_taa_records: null argument"); return UR_EINVAL; }
    f->TaaRecord = own_record;
    f->TaaRecords = all_records;
    return UR_OK;
}

int ur_frame_finish_post(ur_frame* f)
{
    if (!f) { ur::set_error("ur_frame_finish_post: null argument"); return UR_EINVAL; }
    if (!f->Renderer.IsPostPending()) { ur::set_error("ur_frame_finish_post: no post passes are pending"); return UR_EINVAL; }
    FHotPathResources& R = f->Res;
    if (!equal_band(f, R.Height, R.Row0, R.Rows)) { ur::set_error("ur_frame_finish_post: the band is not rank's equal band (world_size | height)"); return UR_EINVAL; }
    R.PostRecords = f->PostRecords;
    R.TaaRecords = f->TaaRecords;
    return f->Renderer.FinishPost(f->Cmd, R);
}

static uint32_t copy_out(const std::string& s, char* buf, uint32_t cap)
{
    if (buf && cap) {
        const size_t n = s.size() < cap - 1 ? s.size() : cap - 1;
        std::memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return static_cast<uint32_t>(s.size() + 1);
}

uint32_t ur_frame_report(const ur_frame* f, char* buf, uint32_t cap)
{
    std::ostringstream s;
    if (f)
        for (const auto& p : f->Renderer.GetLastReport())
            s << p.Name << '|' << (p.bCulled ? 1 : 0) << '|' << p.Transitions << '|' << (p.bAsync ? 1 : 0) << '|' << p.CrossStreamWaits << '\n';
    return copy_out(s.str(), buf, cap);
}

uint32_t ur_rg_timing_stats(char* buf, uint32_t cap)
{
    std::ostringstream s;
    for (const auto& t : FRenderGraph::GetGpuTimingStats()) s << t.Name << '|' << t.AvgMs << '|' << t.MinMs << '|' << t.MaxMs << '|' << t.SampleCount << '\n';
    return copy_out(s.str(), buf, cap);
}

} // extern "C"
