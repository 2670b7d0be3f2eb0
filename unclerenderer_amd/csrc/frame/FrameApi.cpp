// FrameApi.cpp — the C face of the frame (include/ur_frame.h): struct ur_frame, ur_frame_render's validation, the setters, the report.

#include <hip/hip_runtime.h>

#include <cstring>
#include <sstream>

#include "../../../include/ur_frame.h"
#include "../../../include/ur_host.h"
#include "../ur_checks.h"
#include "HotPathRenderer.h"
#include "LightingTimer.h"

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
    FLightingTimer Timer; // UR_FRAME_TIME_LIGHTING*
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

// What ur_frame_render refuses in more than one place; `what` names the flags that ask
static bool has_tonemap(const ur_frame_resources* r, uint32_t flags, const char* what)
{
    if ((flags & UR_FRAME_TONEMAP) && r->tonemap_band) return true;
    ur::set_error("ur_frame_render: %s UR_FRAME_TONEMAP and a tonemap_band", what);
    return false;
}
static bool has_post_records(const ur_frame* f, const char* what)
{
    if (f->PostRecord && f->PostRecords) return true;
    ur::set_error("ur_frame_render: %s needs ur_frame_set_post_records", what);
    return false;
}
static bool has_equal_band(const ur_frame* f, const ur_frame_resources* r, const char* what)
{
    if (equal_band(f, r->height, r->row0, r->rows)) return true;
    ur::set_error("ur_frame_render: %s needs rank's equal band (world_size | height)", what);
    return false;
}

ur_frame* ur_frame_create(ur_ctx* ctx, void* stream, uint32_t frames_in_flight, int rank, int world_size)
{
    if (!ctx) return nullptr;
    ur_frame* f = new ur_frame(ctx, static_cast<hipStream_t>(stream), frames_in_flight, rank, world_size);
    f->Renderer.SetLightingTimer([f](hipStream_t s, bool begin) { f->Timer.Mark(f->Cmd.GetContext(), s, begin); });
    return f;
}

uint32_t ur_frame_lighting_times_ex(ur_frame* f, float* out_ms, float* out_record_ms, uint32_t cap) { return f ? f->Timer.Read(out_ms, out_record_ms, cap) : 0; }

uint32_t ur_frame_lighting_times(ur_frame* f, float* out_ms, uint32_t cap) { return ur_frame_lighting_times_ex(f, out_ms, nullptr, cap); }

void ur_frame_destroy(ur_frame* f)
{
    if (!f) return;
    if (f->AsyncStream) (void)hipStreamSynchronize(f->AsyncStream);
    if (f->AsyncCtx) ur_destroy(f->AsyncCtx);
    if (f->AsyncStream) (void)hipStreamDestroy(f->AsyncStream);
    f->Timer.Destroy();
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
        if (!has_tonemap(r, flags, "AUTO_EXPOSURE / CAS need")) return UR_EINVAL;
        if ((flags & UR_FRAME_AUTO_EXPOSURE) && (!f->Post.luminance[0] || !f->Post.luminance[1])) { ur::set_error("ur_frame_render: AUTO_EXPOSURE needs ur_frame_set_post's luminance[2]"); return UR_EINVAL; }
        if (cas_pass && !f->Post.tonemap_scratch) { ur::set_error("ur_frame_render: a CAS pass of its own needs ur_frame_set_post's tonemap_scratch"); return UR_EINVAL; }
        const bool exchange = (flags & UR_FRAME_POST_EXCHANGE) && (flags & (UR_FRAME_AUTO_EXPOSURE | UR_FRAME_CAS));
        if ((flags & (UR_FRAME_AUTO_EXPOSURE | UR_FRAME_CAS)) && !exchange && (r->row0 != 0 || r->rows != r->height)) {
            ur::set_error("ur_frame_render: AutoExposure and CAS need the whole frame (rows == height), or UR_FRAME_POST_EXCHANGE on a band");
            return UR_EUNSUPPORTED;
        }
        if (exchange && (!has_post_records(f, "POST_EXCHANGE") || !has_equal_band(f, r, "POST_EXCHANGE"))) return UR_EINVAL;
    }
    if (flags & (UR_FRAME_TAA | UR_FRAME_FUSE_TAA_TONEMAP)) {
        if (!(flags & UR_FRAME_TAA)) { ur::set_error("ur_frame_render: FUSE_TAA_TONEMAP needs UR_FRAME_TAA"); return UR_EINVAL; }
        if (!has_tonemap(r, flags, "TAA needs")) return UR_EINVAL;
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
        if (!has_post_records(f, "TAA_BAND")) return UR_EINVAL;
        if (!f->TaaRecord || !f->TaaRecords) { ur::set_error("ur_frame_render: TAA_BAND needs ur_frame_set_taa_records"); return UR_EINVAL; }
        if (!has_equal_band(f, r, "TAA_BAND")) return UR_EINVAL;
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
        if (!has_tonemap(r, flags, "DEBUG_PRINT needs")) return UR_EINVAL;
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
    f->Timer.bKernelEvents = (flags & UR_FRAME_TIME_LIGHTING_KERNEL) != 0;
    f->Timer.bRecordAfter = (flags & UR_FRAME_TIME_LIGHTING_RECORD_COST) != 0;
    O.bGpuTiming = (flags & UR_FRAME_GPU_TIMING) != 0;
    O.bGraphDump = (flags & UR_FRAME_GRAPH_DUMP) != 0;
    O.bBarrierLogs = (flags & UR_FRAME_BARRIER_LOGS) != 0;
    f->Cmd.SetJoinAsyncAtEnd((flags & UR_FRAME_ASYNC_NO_JOIN) == 0);
    f->Cmd.BeginFrame();
    // Launch scheduling across two passes (include/ur_hotpath.h, ur_defer_hzb_tail): only when both run on the main stream
    const bool chain_with_lighting = (flags & UR_FRAME_HZB_WITH_LIGHTING) != 0 && !O.bAsyncCompute;
    const bool tail_with_lighting = (chain_with_lighting || (flags & UR_FRAME_HZB_TAIL_WITH_LIGHTING) != 0) && !O.bAsyncCompute;
    if (tail_with_lighting) (void)ur_defer_hzb_tail(f->Cmd.GetContext(), chain_with_lighting ? 2 : 1);
    const FFramePlan Plan = f->Renderer.PlanFrame(R, O, f->Cmd.GetWorldSize());
    // Two launches in this frame, the cull and the Lighting launch that carries Build HZB: the cull's own completion stamp starts the Lighting measurement
    f->Timer.bStartOnCull = false;
    if (f->Timer.bKernelEvents && chain_with_lighting && Plan.Cull.bEnabled && O.bHZBEnabled && O.bDoDepthPrepass) f->Timer.StartOnCull(f->Cmd.GetContext());
    const int rc = f->Renderer.RenderFrame(f->Cmd, R, K, Plan);
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
