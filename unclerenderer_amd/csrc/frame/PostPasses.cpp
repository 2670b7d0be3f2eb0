// PostPasses.cpp — the post chain of FHotPathRenderer: [TemporalAA ->] AutoExposure -> Tonemap -> CAS [-> GpuDebugPrint] (DeferredRenderer.cpp:1308-1598),
// its two-call form on a row band ("Post Record" at the end of RenderFrame, the passes in FinishPost), and the luminance and TemporalAA histories.

#include "HotPathRenderer.h"

#include "../post_records.h"
#include "../ur_checks.h"

FRGResourceHandle FHotPathRenderer::ImportTaaHistory(FRenderGraph& Graph, FHotPathResources& Res, uint32 Index) const
{
    return Graph.ImportTexture("TaaHistory_" + std::to_string(Index), Res.TaaHistory[Index], &Res.TaaHistoryStates[Index], {Res.Width, Res.Rows, RG_FORMAT_R16G16B16A16_FLOAT});
}

// ---- Post Record: the band's part of the post exchange; the post passes wait for FinishPost --------------------------
// With TemporalAA on the band the pass packs the TAA record too, from the history image the frame reads: before the resolve,
// which with a ring of one image overwrites it.
void FHotPathRenderer::AddPostRecordPass(FRenderGraph& Graph, FRGResourceHandle LightingHandle, FHotPathResources& Res)
{
    struct FPostRecordPassData
    {
        uint32 TaaUseHistory = 0, TaaReadIndex = 0;
    };
    const FTaaSlots Taa = TaaSlots;
    FRGResourceHandle TaaRecordHandle, TaaReadHandle;
    if (Plan.TaaOnBand()) {
        TaaRecordHandle = Graph.ImportTexture("TaaRecord", Res.TaaRecord, &Res.TaaRecordState,
                                              {static_cast<uint32>(ur_records::taa_texels(Res.Width)), 1, RG_FORMAT_R16G16B16A16_FLOAT});
        if (Taa.bUseHistory) TaaReadHandle = ImportTaaHistory(Graph, Res, Taa.Read);
    }
    const FRGResourceHandle RecordHandle = Graph.ImportTexture("PostRecord", Res.PostRecord, &Res.PostRecordState,
                                                               {static_cast<uint32>(ur_records::post_texels(Res.Width)), 1, RG_FORMAT_R16G16B16A16_FLOAT});
    Graph.AddPass<FPostRecordPassData>("Post Record", [&](FPostRecordPassData& Data, FRGPassBuilder& Builder)
    {
        Data.TaaUseHistory = Taa.bUseHistory ? 1u : 0u;
        Data.TaaReadIndex = Taa.Read;
        Builder.ReadTexture(LightingHandle, RG_STATE_NON_PIXEL_SHADER_RESOURCE);
        Builder.WriteTexture(RecordHandle, RG_STATE_UNORDERED_ACCESS);
        if (Plan.TaaOnBand()) {
            if (Taa.bUseHistory) Builder.ReadTexture(TaaReadHandle, RG_STATE_NON_PIXEL_SHADER_RESOURCE);
            Builder.WriteTexture(TaaRecordHandle, RG_STATE_UNORDERED_ACCESS);
        }
    }, [this, &Res](const FPostRecordPassData& Data, FHIPCommandContext& Cmd)
    {
        int rc = ur_pack_post_record(Cmd.GetContext(), Res.LightingBand, Res.Width, Res.Height, Res.Row0, Res.Rows, Res.PostRecord);
        if (rc == UR_OK && Plan.TaaOnBand())
            rc = ur_pack_taa_record(Cmd.GetContext(), Res.LightingBand, Data.TaaUseHistory ? Res.TaaHistory[Data.TaaReadIndex] : nullptr, Data.TaaUseHistory,
                                    Res.Width, Res.Height, Res.Row0, Res.Rows, Res.TaaRecord);
        RecordPassError(rc);
    });
}

int FHotPathRenderer::FinishPost(FHIPCommandContext& Cmd, FHotPathResources& Res)
{
    if (!bPostPending) { ur::set_error("ur_frame_finish_post: no post passes are pending (render with UR_FRAME_POST_EXCHANGE and AUTO_EXPOSURE / CAS / TAA_BAND first)"); return UR_EINVAL; }
    bPostPending = false;
    PassError = UR_OK;
    FRenderGraph Graph;
    ConfigureGraph(Graph);
    const FRGResourceHandle LightingHandle = Graph.ImportTexture("Lighting", Res.LightingBand, &Res.LightingState, {Res.Width, Res.Rows, RG_FORMAT_R16G16B16A16_FLOAT});
    AddPostPasses(Graph, LightingHandle, Res, PendingConstants, ImportDebugPrint(Graph, Res));
    Graph.Execute(Cmd);
    const std::vector<FRenderGraph::FPassReport>& Tail = Graph.GetLastExecutionReport();
    LastReport.insert(LastReport.end(), Tail.begin(), Tail.end());
    EndPostHistory();
    if (Plan.TaaOnBand()) EndTaaHistory(true, static_cast<uint32>(Res.TaaHistory.size())); // (else RenderFrame dropped the ring)
    return PassError;
}

void FHotPathRenderer::EndPostHistory()
{
    // :1612-1620: the luminance written this frame is next frame's history
    if (Plan.AutoExposure.bEnabled && PassError == UR_OK) {
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

void FHotPathRenderer::EndTaaHistory(bool bTaaWritten, uint32 SlotCount)
{
    // :1602-1610, and OnFrameFenceSignaled (:2787-2799): the slot a TemporalAA frame wrote is next frame's history. The reference marks
    // it when the frame's fence is signalled and does not wait for the GPU either; here stream order makes the image complete before
    // the next frame's pass reads it. A frame whose pass failed hands on nothing.
    if (TaaHistoryValid.size() != SlotCount) TaaHistoryValid.assign(SlotCount, false);
    if (bTaaWritten && PassError == UR_OK) {
        TaaHistoryValid[TaaSlots.Write] = true;
        TaaSampleIndex = (TaaSampleIndex + 1u) % 8u;
    } else {
        ResetTaa();
    }
}

// The passes of the frame's plan. On the band alone (Plan.bEndsAtPostRecord, from FinishPost; the band is this rank's equal band) they work
// from the Plan.RecordRanks gathered post records: AutoExposure reads every rank's tap texels, Tonemap / CAS read the rows around the band
// from the neighbours' records in place. TemporalAA on the band resolves from the neighbours' current rows in the post records and, for CAS,
// also resolves the row on either side of the band from their TAA records into Res.TaaHaloRows: CAS's halo rows.
void FHotPathRenderer::AddPostPasses(FRenderGraph& Graph, FRGResourceHandle LightingHandle, FHotPathResources& Res, const FHotPathFrameConstants& Constants,
                                     FDebugPrintHandles DebugPrint)
{
    // (DeferredRenderer.cpp:1308-1573)
    // Without TemporalAA, AutoExposure and CAS this is the Tonemap pass alone, Lighting -> LDR band, as before they existed.
    const uint32 WriteIndex = LuminanceWriteIndex;
    const bool bFromRecords = Plan.bEndsAtPostRecord;
    const uint32 RecordRanks = Plan.RecordRanks;
    const uint64 RecordBytes = ur_post_record_bytes(Res.Width);
    const uint8_t* Records = static_cast<const uint8_t*>(Res.PostRecords);
    // row Row (a name of csrc/post_records.h: the layout ur_pack_post_record / ur_pack_taa_record wrote) of rank R's record, in place
    namespace Rec = ur_records;
    auto RecordRow = [&Res](const uint8_t* Recs, uint64 Bytes, uint32 R, uint32 Row) {
        return reinterpret_cast<const ur_half4*>(Recs + R * Bytes + Rec::row_offset(Row, Res.Width));
    };
    const uint32 Rank = bFromRecords ? Res.Row0 / Res.Rows : 0;
    // the neighbours' last / first HDR rows: the halo rows of CAS (none at the frame's top / bottom edge), and of TemporalAA on the band
    const ur_half4* CurAbove = bFromRecords && Rank > 0 ? RecordRow(Records, RecordBytes, Rank - 1, Rec::kPostLastRow) : nullptr;
    const ur_half4* CurBelow = bFromRecords && Rank + 1 < RecordRanks ? RecordRow(Records, RecordBytes, Rank + 1, Rec::kPostFirstRow) : nullptr;
    // TemporalAA on the band: behind it CAS's halo rows are the RESOLVED rows around the band, which the TemporalAA launch writes
    // from the neighbours' TAA records: above second_last_row / history_last_row, below second_row / history_first_row
    const uint64 TaaRecordBytes = ur_taa_record_bytes(Res.Width);
    const uint8_t* TaaRecs = static_cast<const uint8_t*>(Res.TaaRecords);
    struct FTaaBandRows
    {
        const ur_half4 *CurAbove = nullptr, *CurBelow = nullptr, *Above2 = nullptr, *HistAbove = nullptr, *Below2 = nullptr, *HistBelow = nullptr;
        ur_half4 *ResolvedAbove = nullptr, *ResolvedBelow = nullptr;
    } TaaRows;
    if (Plan.TaaOnBand()) {
        TaaRows.CurAbove = CurAbove;
        TaaRows.CurBelow = CurBelow;
        if (Plan.bTaaHaloRows && CurAbove) {
            TaaRows.Above2 = RecordRow(TaaRecs, TaaRecordBytes, Rank - 1, Rec::kTaaSecondLastRow);
            if (TaaSlots.bUseHistory) TaaRows.HistAbove = RecordRow(TaaRecs, TaaRecordBytes, Rank - 1, Rec::kTaaHistLastRow);
            TaaRows.ResolvedAbove = Res.TaaHaloRows;
        }
        if (Plan.bTaaHaloRows && CurBelow) {
            TaaRows.Below2 = RecordRow(TaaRecs, TaaRecordBytes, Rank + 1, Rec::kTaaSecondRow);
            if (TaaSlots.bUseHistory) TaaRows.HistBelow = RecordRow(TaaRecs, TaaRecordBytes, Rank + 1, Rec::kTaaHistFirstRow);
            TaaRows.ResolvedBelow = Res.TaaHaloRows + Res.Width;
        }
    }
    const ur_half4* HaloAbove = Plan.CasHaloRows == ECasHaloRows::Resolved ? TaaRows.ResolvedAbove : CurAbove;
    const ur_half4* HaloBelow = Plan.CasHaloRows == ECasHaloRows::Resolved ? TaaRows.ResolvedBelow : CurBelow;
    const FRGResourceHandle TaaRecordsHandle = Plan.bTaaHaloRows
        ? Graph.ImportTexture("TaaRecords", const_cast<void*>(Res.TaaRecords), &Res.TaaRecordsState,
                              {static_cast<uint32>(Rec::taa_texels(Res.Width)), RecordRanks, RG_FORMAT_R16G16B16A16_FLOAT})
        : FRGResourceHandle{};
    const FRGResourceHandle TaaHaloHandle = Plan.bTaaHaloRows
        ? Graph.ImportTexture("TaaHaloRows", Res.TaaHaloRows, &Res.TaaHaloRowsState, {Res.Width, 2, RG_FORMAT_R16G16B16A16_FLOAT})
        : FRGResourceHandle{};
    const FRGResourceHandle RecordsHandle = bFromRecords
        ? Graph.ImportTexture("PostRecords", const_cast<void*>(Res.PostRecords), &Res.PostRecordsState,
                              {static_cast<uint32>(Rec::post_texels(Res.Width)), RecordRanks, RG_FORMAT_R16G16B16A16_FLOAT})
        : FRGResourceHandle{};
    FRGResourceHandle LuminanceHandles[2];
    if (Plan.AutoExposure.bExists) {
        LuminanceHandles[0] = Graph.ImportTexture("LuminanceA", Res.Luminance[0], &Res.LuminanceStates[0], {1, 1, RG_FORMAT_R32_FLOAT});
        LuminanceHandles[1] = Graph.ImportTexture("LuminanceB", Res.Luminance[1], &Res.LuminanceStates[1], {1, 1, RG_FORMAT_R32_FLOAT});
    }

    // ---- TemporalAA (:1308-1361): Lighting + TaaHistory_<Read> -> TaaHistory_<Write>; AutoExposure keeps reading Lighting (:1387),
    // Tonemap reads TaaHistory_<Write> (:1454-1459). With bFuseTaaTonemap the pass stays in the graph, disabled and culled, and the
    // Tonemap pass makes the one launch (ur_temporal_aa_tonemap).
    struct FTemporalAAPassData
    {
        float HistoryWeight = 0.9f;
        uint32 UseHistory = 0, ReadIndex = 0, WriteIndex = 0;
    };
    // the rows around the band that a TemporalAA launch on the band reads, declared by the pass that makes the launch
    auto DeclareTaaBandRows = [&](FRGPassBuilder& Builder) {
        if (!Plan.TaaOnBand()) return;
        Builder.ReadTexture(RecordsHandle, RG_STATE_NON_PIXEL_SHADER_RESOURCE);
        if (Plan.bTaaHaloRows) {
            Builder.ReadTexture(TaaRecordsHandle, RG_STATE_NON_PIXEL_SHADER_RESOURCE);
            Builder.WriteTexture(TaaHaloHandle, RG_STATE_UNORDERED_ACCESS);
        }
    };
    const FTaaSlots Taa = TaaSlots;
    FRGResourceHandle TaaReadHandle, TaaWriteHandle;
    if (Plan.TemporalAA.bExists) {
        TaaWriteHandle = ImportTaaHistory(Graph, Res, Taa.Write);
        TaaReadHandle = Taa.Read == Taa.Write ? TaaWriteHandle : ImportTaaHistory(Graph, Res, Taa.Read); // a ring of one image: read and written in place
        Graph.AddPass<FTemporalAAPassData>("TemporalAA", [&](FTemporalAAPassData& Data, FRGPassBuilder& Builder)
        {
            if (!Plan.TemporalAA.bEnabled) return;
            Data.ReadIndex = Taa.Read;
            Data.WriteIndex = Taa.Write;
            Data.HistoryWeight = Constants.TaaHistoryWeight;
            Data.UseHistory = Taa.bUseHistory ? 1u : 0u;
            Builder.ReadTexture(LightingHandle, RG_STATE_NON_PIXEL_SHADER_RESOURCE);
            if (Taa.Read != Taa.Write) Builder.ReadTexture(TaaReadHandle, RG_STATE_NON_PIXEL_SHADER_RESOURCE);
            DeclareTaaBandRows(Builder);
            Builder.WriteTexture(TaaWriteHandle, RG_STATE_UNORDERED_ACCESS);
        }, [this, &Res, TaaRows](const FTemporalAAPassData& Data, FHIPCommandContext& Cmd)
        {
            if (!Plan.TemporalAA.bEnabled) return;
            RecordPassError(Plan.TaaOnBand() // the band alone (FinishPost): ur_temporal_aa_halo
                ? ur_temporal_aa_halo(Cmd.GetContext(), Res.LightingBand, TaaRows.CurAbove, TaaRows.CurBelow, Res.TaaHistory[Data.ReadIndex],
                                      Res.TaaHistory[Data.WriteIndex], TaaRows.Above2, TaaRows.HistAbove, TaaRows.Below2, TaaRows.HistBelow, TaaRows.ResolvedAbove,
                                      TaaRows.ResolvedBelow, Data.HistoryWeight, Data.UseHistory, Res.Width, Res.Height, Res.Row0, Res.Rows)
                : ur_temporal_aa(Cmd.GetContext(), Res.LightingBand, Res.TaaHistory[Data.ReadIndex], Res.TaaHistory[Data.WriteIndex], Data.HistoryWeight,
                                          Data.UseHistory, Res.Width, Res.Height, 0, Res.Height));
        });
    }

    struct FAutoExposurePassData
    {
        ur_auto_exposure_constants K = {};
        uint32 ReadIndex = 0, WriteIndex = 0;
    };
    if (Plan.AutoExposure.bExists) {
        Graph.AddPass<FAutoExposurePassData>("AutoExposure", [&](FAutoExposurePassData& Data, FRGPassBuilder& Builder)
        {
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
            Builder.ReadTexture(bFromRecords ? RecordsHandle : LightingHandle, RG_STATE_NON_PIXEL_SHADER_RESOURCE);
            Builder.ReadTexture(LuminanceHandles[Data.ReadIndex], RG_STATE_NON_PIXEL_SHADER_RESOURCE);
            Builder.WriteTexture(LuminanceHandles[Data.WriteIndex], RG_STATE_UNORDERED_ACCESS);
        }, [this, &Res](const FAutoExposurePassData& Data, FHIPCommandContext& Cmd)
        {
            const float* Prev = Data.K.UseHistory ? Res.Luminance[Data.ReadIndex] : nullptr;
            RecordPassError(Plan.bEndsAtPostRecord
                ? ur_auto_exposure_records(Cmd.GetContext(), &Data.K, Res.PostRecords, Plan.RecordRanks, Res.Width, Res.Height, Prev, Res.Luminance[Data.WriteIndex])
                : ur_auto_exposure(Cmd.GetContext(), &Data.K, Res.LightingBand, Res.Width, Res.Height, Prev, Res.Luminance[Data.WriteIndex]));
        });
    }

    struct FTonemapPassData
    {
        ur_tonemap_constants K;
        ur_cas_constants Cas;
        const float* ExposureEv = nullptr;
        uint32* Output = nullptr;
        const ur_half4* HaloAbove = nullptr;
        const ur_half4* HaloBelow = nullptr;
        const ur_half4* Input = nullptr; // Lighting, or TaaHistory_<Write> behind a TemporalAA pass
        float TaaHistoryWeight = 0.9f;   // of a launch that resolves TemporalAA too
        uint32 TaaUseHistory = 0, TaaReadIndex = 0, TaaWriteIndex = 0;
    };
    struct FCasPassData
    {
        ur_cas_constants K;
        ur_tonemap_constants Tonemap; // the band alone: the rows around it are Tonemap's input rows, tonemapped by the CAS launch
        const float* ExposureEv = nullptr;
        const ur_half4* HaloAbove = nullptr;
        const ur_half4* HaloBelow = nullptr;
    };
    if (!Plan.Tonemap.bExists) return;
    const FRGResourceHandle HaloRowsHandle = Plan.CasHaloRows == ECasHaloRows::Resolved ? TaaHaloHandle : RecordsHandle;
    // the back buffer: "TonemapOutput" itself when nothing follows Tonemap
    const FRGResourceHandle TonemapHandle = Plan.Cas.bExists ? Graph.ImportTexture("BackBuffer", Res.TonemapBand, &Res.TonemapState, {Res.Width, Res.Rows, RG_FORMAT_R8G8B8A8_UNORM})
                                                 : Graph.ImportTexture("TonemapOutput", Res.TonemapBand, &Res.TonemapState, {Res.Width, Res.Rows, RG_FORMAT_R8G8B8A8_UNORM_SRGB});
    const FRGResourceHandle ScratchHandle = Plan.bTonemapToScratch
        ? Graph.ImportTexture("TonemapOutput", Res.TonemapScratch, &Res.TonemapScratchState, {Res.Width, Res.Rows, RG_FORMAT_R8G8B8A8_UNORM})
        : FRGResourceHandle{};
    const ur_cas_constants CasK = {{1.0f / static_cast<float>(Res.Width), 1.0f / static_cast<float>(Res.Height)}, Constants.CasSharpness, 0.0f}; // :1533
    Graph.AddPass<FTonemapPassData>("Tonemap", [&](FTonemapPassData& Data, FRGPassBuilder& Builder)
    {
        Data.K = Constants.Tonemap;
        Data.K.EnableAutoExposure = Plan.AutoExposure.bEnabled ? 1u : 0u;
        Data.Cas = CasK;
        Data.ExposureEv = Plan.AutoExposure.bEnabled ? Res.Luminance[WriteIndex] : nullptr;
        Data.Output = Plan.bTonemapToScratch ? Res.TonemapScratch : Res.TonemapBand;
        Data.HaloAbove = HaloAbove;
        Data.HaloBelow = HaloBelow;
        Data.Input = Plan.TemporalAA.bExists ? Res.TaaHistory[Taa.Write] : Res.LightingBand;
        Data.TaaHistoryWeight = Constants.TaaHistoryWeight;
        Data.TaaUseHistory = Taa.bUseHistory ? 1u : 0u;
        Data.TaaReadIndex = Taa.Read;
        Data.TaaWriteIndex = Taa.Write;
        if (Plan.bFuseTaaTonemap) { // the TemporalAA pass's usages move here
            Builder.ReadTexture(LightingHandle, RG_STATE_NON_PIXEL_SHADER_RESOURCE);
            if (Taa.Read != Taa.Write) Builder.ReadTexture(TaaReadHandle, RG_STATE_NON_PIXEL_SHADER_RESOURCE);
            DeclareTaaBandRows(Builder);
            Builder.WriteTexture(TaaWriteHandle, RG_STATE_UNORDERED_ACCESS);
        } else {
            Builder.ReadTexture(Plan.TemporalAA.bExists ? TaaWriteHandle : LightingHandle, RG_STATE_PIXEL_SHADER_RESOURCE);
        }
        if (Plan.CasHaloRows != ECasHaloRows::None && !Plan.Cas.bEnabled) Builder.ReadTexture(HaloRowsHandle, RG_STATE_PIXEL_SHADER_RESOURCE); // (CAS in this pass's launch)
        if (Plan.AutoExposure.bEnabled) Builder.ReadTexture(LuminanceHandles[WriteIndex], RG_STATE_PIXEL_SHADER_RESOURCE);
        Builder.WriteTexture(Plan.bTonemapToScratch ? ScratchHandle : TonemapHandle, RG_STATE_RENDER_TARGET);
    }, [this, &Res, TaaRows](const FTonemapPassData& Data, FHIPCommandContext& Cmd)
    {
        int rc = UR_OK;
        switch (Plan.TonemapLaunch) {
        case ETonemapLaunch::TaaTonemapHalo:
            rc = ur_temporal_aa_tonemap_halo(Cmd.GetContext(), &Data.K, Res.LightingBand, TaaRows.CurAbove, TaaRows.CurBelow, Res.TaaHistory[Data.TaaReadIndex],
                                             Res.TaaHistory[Data.TaaWriteIndex], Data.ExposureEv, Data.Output, TaaRows.Above2, TaaRows.HistAbove, TaaRows.Below2,
                                             TaaRows.HistBelow, TaaRows.ResolvedAbove, TaaRows.ResolvedBelow, Data.TaaHistoryWeight, Data.TaaUseHistory, Res.Width,
                                             Res.Height, Res.Row0, Res.Rows);
            break;
        case ETonemapLaunch::TaaTonemap:
            rc = ur_temporal_aa_tonemap(Cmd.GetContext(), &Data.K, Res.LightingBand, Res.TaaHistory[Data.TaaReadIndex], Res.TaaHistory[Data.TaaWriteIndex],
                                        Data.ExposureEv, Data.Output, Data.TaaHistoryWeight, Data.TaaUseHistory, Res.Width, Res.Height, 0, Res.Height);
            break;
        case ETonemapLaunch::TonemapCasHalo:
            rc = ur_tonemap_cas_halo(Cmd.GetContext(), &Data.K, &Data.Cas, Data.Input, Data.HaloAbove, Data.HaloBelow, Data.ExposureEv, Data.Output, Res.Width,
                                     Res.Height, Res.Row0, Res.Rows);
            break;
        case ETonemapLaunch::TonemapCas:
            rc = ur_tonemap_cas(Cmd.GetContext(), &Data.K, &Data.Cas, Data.Input, Data.ExposureEv, Data.Output, Res.Width, Res.Height, Res.Row0, Res.Rows);
            break;
        case ETonemapLaunch::Tonemap:
            rc = ur_tonemap(Cmd.GetContext(), &Data.K, Data.Input, Data.ExposureEv, Data.Output, Res.Width, Res.Rows);
            break;
        }
        RecordPassError(rc);
        Res.LightingState = RG_STATE_RENDER_TARGET; // the reference transitions the lighting buffer back (:1511-1512)
    });
    if (Plan.Cas.bExists) {
        // fused: still in the graph, disabled and culled, like Sky under bFuseLightingAndSky
        Graph.AddPass<FCasPassData>("CAS", [&](FCasPassData& Data, FRGPassBuilder& Builder)
        {
            Data.K = CasK;
            if (!Plan.Cas.bEnabled) return;
            Data.Tonemap = Constants.Tonemap;
            Data.Tonemap.EnableAutoExposure = Plan.AutoExposure.bEnabled ? 1u : 0u;
            Data.ExposureEv = Plan.AutoExposure.bEnabled ? Res.Luminance[WriteIndex] : nullptr;
            Data.HaloAbove = HaloAbove;
            Data.HaloBelow = HaloBelow;
            Builder.ReadTexture(ScratchHandle, RG_STATE_PIXEL_SHADER_RESOURCE);
            if (Plan.CasLaunch == ECasLaunch::CasHalo) {
                Builder.ReadTexture(HaloRowsHandle, RG_STATE_PIXEL_SHADER_RESOURCE);
                if (Plan.AutoExposure.bEnabled) Builder.ReadTexture(LuminanceHandles[WriteIndex], RG_STATE_PIXEL_SHADER_RESOURCE);
            }
            Builder.WriteTexture(TonemapHandle, RG_STATE_RENDER_TARGET);
        }, [this, &Res](const FCasPassData& Data, FHIPCommandContext& Cmd)
        {
            if (Plan.CasLaunch == ECasLaunch::None) return;
            RecordPassError(Plan.CasLaunch == ECasLaunch::CasHalo
                ? ur_cas_halo(Cmd.GetContext(), &Data.Tonemap, &Data.K, Res.TonemapScratch, Data.HaloAbove, Data.HaloBelow, Data.ExposureEv, Res.TonemapBand,
                              Res.Width, Res.Height, Res.Row0, Res.Rows)
                : ur_cas(Cmd.GetContext(), &Data.K, Res.TonemapScratch, Res.TonemapBand, Res.Width, Res.Height, Res.Row0, Res.Rows));
        });
    }
    // ---- GpuDebugPrint (:1575-1598): last in the frame, DispatchGpuDebugPrintStats then RenderGpuDebugPrint onto the back buffer.
    // On a band the draw composites the part of the text inside it.
    struct FDebugPrintPassData
    {
        ur_debug_print_constants K = {};
    };
    if (Plan.bDebugPrint) {
        Graph.AddPass<FDebugPrintPassData>("GpuDebugPrint", [&](FDebugPrintPassData& Data, FRGPassBuilder& Builder)
        {
            Data.K.ScreenSize[0] = static_cast<float>(Res.Width);
            Data.K.ScreenSize[1] = static_cast<float>(Res.Height);
            Data.K.FirstChar = Res.DebugFirstChar;
            Data.K.CharCount = Res.DebugCharCount;
            Builder.ReadTexture(DebugPrint.Stats, RG_STATE_NON_PIXEL_SHADER_RESOURCE);
            Builder.WriteTexture(DebugPrint.Buffer, RG_STATE_UNORDERED_ACCESS);
            Builder.WriteTexture(TonemapHandle, RG_STATE_RENDER_TARGET);
        }, [this, &Res](const FDebugPrintPassData& Data, FHIPCommandContext& Cmd)
        {
            int rc = ur_debug_print_stats(Cmd.GetContext(), Res.CullStats, Res.DebugPrintBuffer);
            if (rc == UR_OK)
                rc = ur_debug_print_draw(Cmd.GetContext(), &Data.K, Res.DebugGlyphs, Res.DebugGlyphCount, Res.DebugAtlas, Res.DebugAtlasWidth, Res.DebugAtlasHeight,
                                         Res.DebugPrintBuffer, Res.TonemapBand, Res.Width, Res.Height, Res.Row0, Res.Rows);
            RecordPassError(rc);
        });
    }
}
