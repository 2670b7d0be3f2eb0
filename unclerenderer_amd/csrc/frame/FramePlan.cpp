// FramePlan.cpp — every decision of a frame, stated once (FramePlan.h).

#include "FramePlan.h"

FFramePlan MakeFramePlan(const FHotPathOptions& O, const FFrameFacts& F)
{
    FFramePlan P;
    // ---- the scene passes ----
    P.Cull = {true, O.bEnableIndirectDraw && F.bCullInputs};
    P.bHZBAvailable = O.bHZBEnabled && F.bHZB;
    P.bCullUsesHZB = P.bHZBAvailable && F.bHZBReady; // ConfigureHZBOcclusion, :519-520
    // a raster pass is listed iff its draws are set; without its option it is culled, as in the reference
    P.Shadow = {F.bShadowDraws, F.bShadowDraws && O.bRenderShadows};
    P.DepthPrepass = {F.bDepthDraws, F.bDepthDraws && O.bDoDepthPrepass};
    P.GBuffer = {F.bDepthDraws && F.bGBufferDraws, F.bDepthDraws && F.bGBufferDraws && O.bDoDepthPrepass}; // (the base pass tests against the prepass' depth)
    P.BuildHZB.bExists = P.BuildHZB.bEnabled = P.bHZBAvailable && O.bDoDepthPrepass; // only with HZB and depth prepass enabled, :996
    P.bShardHZB = O.bShardHZB;
    P.bAsyncCompute = O.bAsyncCompute;
    P.bUseShadows = O.bRenderShadows;
    const bool bSky = O.bSkyEnabled && F.bDepthBand;
    P.bFusedSky = O.bFuseLightingAndSky && bSky;
    P.Sky = {true, bSky && !P.bFusedSky};
    P.bTimeLighting = O.bTimeLighting;

    // ---- the post chain: [TemporalAA ->] AutoExposure -> Tonemap -> CAS [-> GpuDebugPrint], all of it behind a back buffer ----
    const bool bTonemap = O.bTonemap && F.bTonemapBand;
    const bool bAutoExposure = bTonemap && O.bAutoExposure;
    const bool bCas = bTonemap && O.bCas;
    const bool bFuseCas = bCas && O.bFuseTonemapCas;
    // The exchange is active with AutoExposure or CAS, and with TemporalAA on the band. TemporalAA itself runs on the whole frame, or,
    // asked for on the band, through the exchange; a frame of the exchange without bTaaBand runs without it.
    const bool bTaaBandAsked = O.bTaaBand && O.bTaa && O.bPostExchange;
    const bool bExchangePost = O.bPostExchange && (bAutoExposure || bCas);
    const bool bTaa = O.bTaa && bTonemap && F.TaaSlotCount != 0 && (bTaaBandAsked || !bExchangePost);
    P.bEndsAtPostRecord = bExchangePost || (bTaaBandAsked && bTaa);
    P.RecordRanks = P.bEndsAtPostRecord ? F.WorldSize : 0;
    P.Taa = !bTaa ? ETaaMode::Off : P.bEndsAtPostRecord ? ETaaMode::Band : ETaaMode::Whole;
    P.bFuseTaaTonemap = bTaa && O.bFuseTaaTonemap;
    P.TemporalAA = {bTaa, bTaa && !P.bFuseTaaTonemap};
    P.AutoExposure = {bAutoExposure, bAutoExposure};
    P.Tonemap = {bTonemap, bTonemap};
    P.Cas = {bCas, bCas && !bFuseCas}; // fused: still in the graph, disabled and culled, like Sky under bFuseLightingAndSky
    // Tonemap's launch. (Both fuses together are refused by ur_frame_render: TAA + Tonemap + CAS in one launch is not built. Here TemporalAA's wins.)
    P.TonemapLaunch = P.bFuseTaaTonemap ? (P.TaaOnBand() ? ETonemapLaunch::TaaTonemapHalo : ETonemapLaunch::TaaTonemap)
                      : bFuseCas        ? (P.bEndsAtPostRecord ? ETonemapLaunch::TonemapCasHalo : ETonemapLaunch::TonemapCas)
                                        : ETonemapLaunch::Tonemap;
    P.bTonemapToScratch = P.Cas.bEnabled;
    P.CasLaunch = !P.Cas.bEnabled ? ECasLaunch::None : P.bEndsAtPostRecord ? ECasLaunch::CasHalo : ECasLaunch::Cas;
    // On the band alone CAS's rows around it are the neighbours': their post records' rows, or, behind TemporalAA on the band, the rows its launch resolved
    P.bTaaHaloRows = P.TaaOnBand() && bCas;
    P.CasHaloRows = !(P.bEndsAtPostRecord && bCas) ? ECasHaloRows::None : P.TaaOnBand() ? ECasHaloRows::Resolved : ECasHaloRows::Records;
    P.bDebugPrint = O.bDebugPrint && bTonemap && F.bDebugPrintInputs;

    P.bGpuTiming = O.bGpuTiming;
    P.bGraphDump = O.bGraphDump;
    P.bBarrierLogs = O.bBarrierLogs;
    return P;
}
