/*
 * ur_frame.h — C face of the render-graph-driven frame (csrc/frame/HotPathRenderer): the four hot passes added to an
 * FRenderGraph in the reference's order and executed on the context's stream. This is what a host that does not link
 * C++ (the Python tests, bench.py) calls; a C++ renderer uses FRenderGraph / FHotPathRenderer directly.
 */
#ifndef UR_FRAME_H
#define UR_FRAME_H

#include "ur_hotpath.h"
#include "ur_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ur_frame ur_frame;

/* All device pointers; band-local images hold rows [row0,row0+rows) of the width x height frame. */
typedef struct ur_frame_resources {
    uint32_t width, height, row0, rows;
    const ur_half4* gbuffer_a;
    const ur_half4* gbuffer_b;
    const uint32_t* gbuffer_c;
    const float* depth_band;
    ur_half4* lighting_band;
    const float* depth_full;      /* src of the (replicated) HZB build */
    float* hzb;
    ur_mip_desc hzb_mips[UR_MAX_HZB_MIPS];
    uint32_t hzb_mip_count;
    ur_lighting_tables tables;
    const ur_float4* model_bounds;
    void* indirect_args;
    uint32_t indirect_command_count;
    uint32_t instance_index_base;
    uint32_t* visible_indices;    /* nullable */
    uint32_t* visible_count;      /* nullable */
    uint32_t* cull_stats;         /* nullable */
    uint32_t* tonemap_band;       /* nullable: R8G8B8A8_UNORM output of the optional Tonemap pass (UR_FRAME_TONEMAP) */
} ur_frame_resources;

#define UR_FRAME_INDIRECT_DRAW 0x1u
#define UR_FRAME_HZB 0x2u
#define UR_FRAME_DEPTH_PREPASS 0x4u
#define UR_FRAME_SHADOWS 0x8u
#define UR_FRAME_SKY 0x10u
#define UR_FRAME_FUSE_LIGHTING_SKY 0x20u
#define UR_FRAME_GPU_TIMING 0x40u
#define UR_FRAME_GRAPH_DUMP 0x80u
#define UR_FRAME_BARRIER_LOGS 0x100u
#define UR_FRAME_ASYNC_COMPUTE 0x200u /* GPU Culling + Build HZB on a second HIP stream, overlapping Lighting/Sky */
#define UR_FRAME_ASYNC_NO_JOIN 0x400u /* with ASYNC_COMPUTE: do not end the frame with a main<-async join; the caller calls ur_frame_join_async() */
#define UR_FRAME_TONEMAP 0x800u /* add the Tonemap pass after Sky (Exposure 0.9, Gamma 2.2, PBR-neutral curve) */
#define UR_FRAME_TIME_LIGHTING 0x1000u /* bracket the Lighting pass with a HIP event pair on its stream; read with ur_frame_lighting_times() */
#define UR_FRAME_HZB_TAIL_WITH_LIGHTING 0x2000u /* the single-workgroup tail of Build HZB rides along with the Lighting launch (ur_defer_hzb_tail); ignored with ASYNC_COMPUTE. The Build HZB pass then ends before the chain is complete; the frame is complete when ur_frame_render's launches are */
#define UR_FRAME_TIME_LIGHTING_RECORD_COST 0x8000u /* TIME_LIGHTING plus one more event recorded right behind the pair: its distance to the pair's closing event is what an event record costs on this queue (ur_frame_lighting_times_ex) */
#define UR_FRAME_HZB_WITH_LIGHTING 0x4000u /* the WHOLE Build HZB chain rides along with the Lighting launch (ur_defer_hzb_tail(ctx, 2)): its 128x32 pieces are walked by one wave of every lighting workgroup, its tail by an extra workgroup that waits for them; two launches per frame (cull, lighting). Ignored with ASYNC_COMPUTE */
#define UR_FRAME_TIME_LIGHTING_KERNEL 0x10000u /* time the Lighting pass by a HIP event pair carried on its kernel dispatch (ur_time_next_lighting): from the end of what precedes the kernel to the kernel's end, what rocprofv3's kernel trace reports for the dispatch; no event record behind the kernel; read with ur_frame_lighting_times() */
#define UR_FRAME_HZB_SHARD 0x20000u /* several ranks (ur_frame_create's world_size > 1): Build HZB builds only this rank's 128x32 pieces of mips 0..4 (ur_build_hzb_band; riding the Lighting launch with HZB_WITH_LIGHTING) and leaves the exchange of the slices and the tail (ur_build_hzb_tail) to the caller, who holds the communicator. One rank: the whole chain as usual */
/* The rest of the reference's post chain after Tonemap's input (DeferredRenderer.cpp:1363-1573). Each needs UR_FRAME_TONEMAP and a
 * tonemap_band (else UR_EINVAL), and the WHOLE frame in one call: rows == height, else UR_EUNSUPPORTED - unless UR_FRAME_POST_EXCHANGE
 * is set (a row band of several ranks). Resources and parameters: ur_frame_set_post. */
#define UR_FRAME_AUTO_EXPOSURE 0x40000u /* "AutoExposure" pass before Tonemap: Lighting -> luminance[W] (history luminance[1-W]); Tonemap then applies 2^EV */
#define UR_FRAME_CAS 0x80000u /* "CAS" pass after Tonemap: Tonemap writes tonemap_scratch, CAS sharpens it into tonemap_band */
#define UR_FRAME_FUSE_TONEMAP_CAS 0x100000u /* with CAS: Tonemap runs ur_tonemap_cas straight into tonemap_band (same bytes, no scratch); the CAS pass is then culled */
/* With AUTO_EXPOSURE and/or CAS (else ignored), on rank's equal band of world_size (ur_frame_create; world_size | height, one rank
 * included): ur_frame_render runs through Sky, then a "Post Record" pass packs the band's post record (ur_pack_post_record) into
 * ur_frame_set_post_records' own_record, and returns with the post passes pending. The caller all-gathers the records in rank order
 * into all_records and calls ur_frame_finish_post, which runs AutoExposure (from the records), Tonemap and CAS on the band with the
 * rows around it read from the neighbours' records. The band's bytes and luminance[W] are those of the unsplit frame, on every rank. */
#define UR_FRAME_POST_EXCHANGE 0x200000u
#define UR_FRAME_CULL_VIEWS 0x400000u /* the "GPU Culling" pass also culls the views of ur_frame_set_cull_views (ur_cull_indirect_args_views), on the async-compute lane too */
/* "TemporalAA" pass between Sky and AutoExposure (DeferredRenderer.cpp:1308-1361): Lighting + history[read] -> history[write] with
 * ur_temporal_aa; Tonemap (ur_tonemap_cas under FUSE_TONEMAP_CAS) then reads history[write] instead of Lighting, AutoExposure keeps
 * reading Lighting. Needs UR_FRAME_TONEMAP, a tonemap_band and ur_frame_set_taa's ring (else UR_EINVAL), and the whole frame: rows !=
 * height or UR_FRAME_POST_EXCHANGE is UR_EUNSUPPORTED (unless UR_FRAME_TAA_BAND asks for the band form). Without the flag the frame is
 * what it is without a ring. */
#define UR_FRAME_TAA 0x800000u
/* With TAA: the Tonemap pass runs ur_temporal_aa_tonemap (history[write] and the LDR image in one launch, the same bytes); the
 * TemporalAA pass is then culled. Not together with UR_FRAME_FUSE_TONEMAP_CAS (UR_EINVAL); with a CAS pass of its own the launch
 * writes tonemap_scratch. */
#define UR_FRAME_FUSE_TAA_TONEMAP 0x1000000u
/* TemporalAA on rank's equal row band through the post exchange (opt-in; without it TAA on a band or with POST_EXCHANGE stays
 * UR_EUNSUPPORTED). Needs UR_FRAME_TAA and UR_FRAME_POST_EXCHANGE, UR_FRAME_TONEMAP and a tonemap_band, ur_frame_set_taa's ring - its
 * images now band-local, width x rows -, ur_frame_set_post_records, ur_frame_set_taa_records and rank's equal band (else UR_EINVAL); a
 * one-row band of several ranks is UR_EUNSUPPORTED. The exchange is then active with or without AUTO_EXPOSURE / CAS: ur_frame_render
 * runs through Sky, the "Post Record" pass packs the post record and the TAA record (ur_pack_taa_record, from the history image the
 * frame reads), and the frame returns with the post passes pending. The caller all-gathers BOTH record buffers (they may be in flight
 * together) and calls ur_frame_finish_post: TemporalAA (ur_temporal_aa_halo) -> AutoExposure from the records (it keeps reading
 * Lighting) -> Tonemap of the resolved band -> CAS with the resolved rows around the band. FUSE_TAA_TONEMAP runs
 * ur_temporal_aa_tonemap_halo (the TemporalAA pass stays in the graph, disabled and culled), FUSE_TONEMAP_CAS ur_tonemap_cas_halo on the
 * resolved band; the two together stay UR_EINVAL. The history images, the LDR band and luminance[W] hold the bytes of the unsplit frame.
 * The written image becomes valid and the sample index advances when ur_frame_finish_post returns UR_OK; a frame that is never
 * finished, like any other frame, invalidates the ring. The ranks' histories stay in step only if ALL RANKS RENDER THE SAME FLAGS every
 * frame: a rank packs history rows exactly when its own ring is valid, and its neighbours read them exactly when theirs is. */
#define UR_FRAME_TAA_BAND 0x2000000u
/* "GpuDebugPrint", the reference's last pass (DeferredRenderer.cpp:1575-1598): the cull's two counters drawn onto the LDR band as
 * "FRUSTUM n" / "OCCLUDE n". Needs UR_FRAME_TONEMAP, a tonemap_band, cull_stats and ur_frame_set_debug_print's buffer and font (else
 * UR_EINVAL). The "GPU Culling" pass then first zeroes the buffer's count and cull_stats (PrepareGpuDebugPrint, on its own stream,
 * also when the cull itself does not run) and culls with DebugPrintEnabled (dword 45) = 1; "GpuDebugPrint" runs behind CAS (behind
 * Tonemap when there is no CAS pass): ur_debug_print_stats, then ur_debug_print_draw in place on tonemap_band, rows [row0,row0+rows).
 * With an active post exchange the pass runs in ur_frame_finish_post, behind CAS: cull_stats then hold this rank's counts, and the
 * caller sums them over the ranks (dist.allreduce_cull_stats) beside the record gathers so that every band prints the frame's totals.
 * Text the caller prints into the buffer between the cull and the pass (ur_debug_print_text, or its own kernels by the slot rule) comes
 * ahead of the two stats lines' entries in the buffer: it is blended first and lies beneath them where they overlap. Without the flag nothing of this happens: the frame is what it is today. */
#define UR_FRAME_DEBUG_PRINT 0x4000000u
/* "ShadowMap" pass directly behind "GPU Culling" (DeferredRenderer.cpp:551-633), with UR_FRAME_SHADOWS: ur_shadow_map of
 * ur_frame_set_shadow_pass' draws with scene->LightViewProjection into its shadow_map, scene->ShadowMapSize texels, on the main stream
 * (with UR_FRAME_ASYNC_COMPUTE behind a wait on the cull, whose lists and ranges it draws from); Lighting then reads that map:
 * tables.shadow_map must be the pass's shadow_map and a pass must be set (else UR_EINVAL). Without UR_FRAME_SHADOWS the pass is listed
 * and culled, as in the reference. On a row band every rank renders the whole map (a replicated side table, like the HZB). Without
 * the flag nothing of this happens: the frame is what it is today. */
#define UR_FRAME_SHADOW_PASS 0x8000000u
/* "DepthPrepass" pass behind "ShadowMap" (behind "GPU Culling" when there is none) and in front of "Build HZB"
 * (DeferredRenderer.cpp:635-718), with UR_FRAME_DEPTH_PREPASS: ur_depth_prepass of ur_frame_set_depth_pass' draws with scene->View and
 * scene->Projection into its depth, width x height texels, on the main stream (with UR_FRAME_ASYNC_COMPUTE behind a wait on the cull,
 * whose lists and ranges it draws from; Build HZB then waits for the pass). Build HZB reads that buffer: depth_full must be the pass's
 * depth and a pass must be set (else UR_EINVAL). The frame then runs cull -> DepthPrepass -> Build HZB -> next frame's cull with no
 * imported depth. Without UR_FRAME_DEPTH_PREPASS the pass is listed and culled, as in the reference when the prepass is off. On a row
 * band every rank renders the whole buffer (replicated, like the HZB and the shadow map). Without the flag nothing of this happens:
 * the frame is what it is today. */
#define UR_FRAME_DEPTH_PASS 0x10000000u
/* "GBuffer" pass behind "DepthPrepass" and in front of "Build HZB" and Lighting (DeferredRenderer.cpp:720-865; with targets.object_id
 * also the "ObjectId" pass, :867-980): ur_gbuffer_pass of ur_frame_set_gbuffer_pass' draws with scene->View and scene->Projection
 * against the prepass' depth, over the band [row0, row0 + rows) of the resources, into gbuffer_a/b/c and - the (emissive, 1) start
 * value Lighting adds to - lighting_band. Needs UR_FRAME_DEPTH_PASS and a pass set by ur_frame_set_gbuffer_pass whose flags equal the
 * depth pass' (both quantise to D24 or neither) and whose targets are the resources' gbuffer_a, gbuffer_b, gbuffer_c and lighting_band
 * (else UR_EINVAL); the depth it tests against is the depth pass' buffer. On the main stream, in stream order behind DepthPrepass
 * (with UR_FRAME_ASYNC_COMPUTE that pass has waited for the cull). Without UR_FRAME_DEPTH_PREPASS the pass is listed and culled, like
 * DepthPrepass. With it a frame goes from index and vertex buffers to pixels: no G-buffer is imported. Without the flag nothing of this
 * happens: the frame is what it is today. */
#define UR_FRAME_GBUFFER_PASS 0x20000000u
#define UR_FRAME_DEFAULT (UR_FRAME_INDIRECT_DRAW | UR_FRAME_HZB | UR_FRAME_DEPTH_PREPASS | UR_FRAME_SHADOWS | UR_FRAME_SKY)

ur_frame* ur_frame_create(ur_ctx* ctx, void* stream, uint32_t frames_in_flight, int rank, int world_size);
void ur_frame_destroy(ur_frame* f);
/* One frame: BeginFrame, build the graph (GPU Culling, Build HZB, Lighting, Sky), Execute. culling_constants: the 46
 * dwords of DispatchGpuCulling; dwords 40-44 (ModelCount, HZBEnabled, HZBMipCount, HZBWidth, HZBHeight) are overwritten
 * from the resources and from whether last frame built an HZB (bHZBReady). */
int ur_frame_render(ur_frame* f, const ur_frame_resources* res, const uint32_t* culling_constants, const ur_scene_constants* scene,
                    const ur_sky_constants* sky, uint32_t option_flags);
/* Main stream waits for everything the async-compute stream has been given so far (see UR_FRAME_ASYNC_NO_JOIN). */
void ur_frame_join_async(ur_frame* f);
/* Elapsed milliseconds of the Lighting passes recorded since the last call (UR_FRAME_TIME_LIGHTING; up to 1024 kept).
 * Call after the stream has been synchronised. Returns how many were written. */
uint32_t ur_frame_lighting_times(ur_frame* f, float* out_ms, uint32_t cap);
/* The same plus, per sample, the time from the bracket's closing event to one more event recorded right behind it: what a
 * single event record adds to the queue (the bracket contains one such record in front of the kernel); -1 for samples taken
 * without UR_FRAME_TIME_LIGHTING_RECORD_COST. */
uint32_t ur_frame_lighting_times_ex(ur_frame* f, float* out_ms, float* out_record_ms, uint32_t cap);
int ur_frame_hzb_ready(const ur_frame* f);
void ur_frame_reset_hzb(ur_frame* f);
/* Post-chain resources and parameters of the frames that follow (the reference's RendererConfig values in brackets). Without this
 * call: no luminance textures, no scratch, tonemap 0.9 / 2.2, CAS sharpness 0.5. The pointers must stay valid while frames use them. */
typedef struct ur_frame_post {
    float* luminance[2];        /* device, 1 float each: LuminanceA / B (R32_FLOAT 1x1, CreateLuminanceResources); needed by AUTO_EXPOSURE */
    uint32_t* tonemap_scratch;  /* device, width x rows R8G8B8A8 "TonemapOutput": Tonemap's output when CAS runs as its own pass; unused when fused */
    float delta_time;           /* RenderFrame's DeltaTime (seconds) */
    float tonemap_exposure, tonemap_gamma;                      /* [0.9, 2.2] */
    float ae_key, ae_min, ae_max, ae_speed_up, ae_speed_down;   /* [0.3, 0.1, 5, 3, 1] */
    float cas_sharpness;                                        /* [0.5] */
} ur_frame_post;
int ur_frame_set_post(ur_frame* f, const ur_frame_post* post);
/* The luminance history becomes invalid (like ur_frame_reset_hzb): the next AutoExposure pass runs with UseHistory = 0. The write
 * index is kept: a frame whose AutoExposure ran writes luminance[W], then W flips; any other frame invalidates the history. */
void ur_frame_reset_post(ur_frame* f);
/* The TemporalAA history ring of the frames that follow (CreateTaaResources, DeferredRenderer.cpp:2740-2785): history_count device
 * images of width x height ur_half4 each, owned by the caller like the luminance pair; all invalid after this call. history_count
 * must be the frame's frames_in_flight (ur_frame_create; 0 counts as 1) and no image may be null, else UR_EINVAL. NULL clears the ring.
 * The array is copied; the images must stay valid while frames use them. history_weight: TaaHistoryWeight [0.9]. */
typedef struct ur_frame_taa {
    ur_half4* const* history;
    uint32_t history_count;
    float history_weight;
} ur_frame_taa;
int ur_frame_set_taa(ur_frame* f, const ur_frame_taa* taa);
/* The reference's bookkeeping (:394-410, :1602-1610, OnFrameFenceSignaled :2787-2799): a frame with UR_FRAME_TAA at frame slot i of N
 * (the slot advances with every ur_frame_render) writes history[i % N] and reads history[(i + N - 1) % N], with UseHistory = whether
 * that image is valid. After such a frame returned UR_OK the image it wrote is valid and the sample index advances (mod 8); after any
 * other frame all images are invalid and the sample index is 0. ur_frame_reset_taa does the latter on request (a resize). */
void ur_frame_reset_taa(ur_frame* f);
/* What the next ur_frame_render with UR_FRAME_TAA will do: the slots, use_history, and the jitter of its sample index
 * (ur_host_taa_jitter; zero when use_history is 0). The caller jitters its projection with it (ur_host_apply_taa_jitter) before it
 * rasterises the G-buffer and fills the constant blocks. UR_EINVAL without a ring. While the post passes of a UR_FRAME_TAA_BAND frame are
 * pending the answer does not count that frame yet: ask after ur_frame_finish_post. */
typedef struct ur_frame_taa_info {
    uint32_t read_slot, write_slot, use_history;
    float jitter[2];
} ur_frame_taa_info;
int ur_frame_taa_next(const ur_frame* f, ur_frame_taa_info* info);
/* Device pointers of the post exchange (UR_FRAME_POST_EXCHANGE), each ur_post_record_bytes(width) per rank: own_record receives this
 * rank's record, all_records holds world_size gathered records in rank order (own_record may alias all_records + rank * bytes, for
 * an in-place all-gather). They must stay valid while frames use them. */
int ur_frame_set_post_records(ur_frame* f, void* own_record, const void* all_records);
/* The TAA records of UR_FRAME_TAA_BAND, each ur_taa_record_bytes(width) per rank, with the aliasing rule of the post records:
 * own_record receives this rank's record, all_records holds world_size gathered records in rank order (own_record may alias
 * all_records + rank * bytes). They must stay valid while frames use them. The two resolved HDR rows that CAS reads around the band
 * (2 * width ur_half4) are the frame's own: allocated at the first such frame with CAS, freed by ur_frame_destroy. */
int ur_frame_set_taa_records(ur_frame* f, void* own_record, const void* all_records);
/* The post passes of a frame rendered with UR_FRAME_POST_EXCHANGE, after the records are gathered: (with UR_FRAME_TAA_BAND,
 * TemporalAA,) AutoExposure, Tonemap and (unless
 * fused) CAS, with the luminance ping-pong and history of the unsplit frame. UR_EINVAL if nothing is pending or the band is not
 * rank's equal band. ur_frame_report then lists both halves in order. */
int ur_frame_finish_post(ur_frame* f);
/* Draw ranges of the "GPU Culling" pass (include/ur_hotpath.h, ur_draw_ranges) for the frames that follow: the pass then calls
 * ur_cull_indirect_args_draws, on the async-compute lane too, and fills commands / counts beside the InstanceCount words. The pass list,
 * its culling and ur_frame_report are the same with and without ranges; a frame whose cull pass does not run leaves commands and counts
 * alone. Offsets are local to the frame's indirect_args (a rank's command slice). NULL clears them. The pointers must stay valid while
 * frames use them. UR_EINVAL for a null frame, a null member or range_count == 0. */
int ur_frame_set_draw_ranges(ur_frame* f, const ur_draw_ranges* draws);
/* Extra views of the "GPU Culling" pass (include/ur_hotpath.h, ur_cull_view) for the frames rendered with UR_FRAME_CULL_VIEWS: the pass
 * then calls ur_cull_indirect_args_views, with the draw ranges of ur_frame_set_draw_ranges when those are set. The frame keeps a copy of
 * the views and of the ur_draw_ranges they point to; the buffers must stay valid while frames use them. count == 0 clears them.
 * Without the flag, or when the cull pass does not run, the views' buffers are left alone. UR_EINVAL for a null frame, count >
 * UR_MAX_CULL_VIEWS, views == NULL with count != 0, and the view errors of ur_cull_indirect_args_views that need no command count. */
int ur_frame_set_cull_views(ur_frame* f, const ur_cull_view* views, uint32_t count);
/* The text buffer (ur_debug_print_buffer_bytes(), device) and the font (device glyph table indexed by code, device R8 atlas; e.g.
 * ur_host_debug_font's, uploaded) of the frames rendered with UR_FRAME_DEBUG_PRINT. The pointers must stay valid while frames use them.
 * NULL clears. UR_EINVAL for a null frame, a null member, glyph_count == 0 or a zero-sized atlas. */
typedef struct ur_frame_debug_print {
    void* buffer;
    const ur_debug_glyph* glyphs;
    uint32_t glyph_count;
    const uint8_t* atlas;
    uint32_t atlas_w, atlas_h;
    uint32_t first_char, char_count; /* DebugPrintConstants.FirstChar / CharCount [32, 96] */
} ur_frame_debug_print;
int ur_frame_set_debug_print(ur_frame* f, const ur_frame_debug_print* dp);
/* The draws, the target and the optional counters (ur_shadow_map's stats4; the caller zeroes them) of the frames rendered with
 * UR_FRAME_SHADOW_PASS. The frame keeps a copy of the struct and of the ur_draw_ranges it points to; the buffers stay the caller's and
 * must stay valid while frames use them. NULL clears. UR_EINVAL for a null frame, a null shadow_map and what ur_shadow_map refuses
 * in the draws (both selections, a list without its count, a null member of ranges, a misaligned buffer). */
typedef struct ur_frame_shadow_pass {
    ur_raster_draws draws;
    float* shadow_map;
    uint32_t* stats4;
} ur_frame_shadow_pass;
int ur_frame_set_shadow_pass(ur_frame* f, const ur_frame_shadow_pass* pass);

/* The draws, the target, the optional counters (ur_depth_prepass' stats6; the caller zeroes them) and ur_depth_prepass' flags of the
 * frames rendered with UR_FRAME_DEPTH_PASS; kept as ur_frame_set_shadow_pass keeps its struct. NULL clears. UR_EINVAL for a null frame,
 * a null depth and what ur_depth_prepass refuses in the draws, the alignment and the flags. */
typedef struct ur_frame_depth_pass {
    ur_raster_draws draws;
    float* depth;
    uint32_t* stats6;
    uint32_t flags;
} ur_frame_depth_pass;
int ur_frame_set_depth_pass(ur_frame* f, const ur_frame_depth_pass* pass);

/* The draws, the targets, the optional counters (ur_gbuffer_pass' stats6; the caller zeroes them), ur_gbuffer_pass' flags and its
 * key_triangle_bits of the frames rendered with UR_FRAME_GBUFFER_PASS; kept as ur_frame_set_shadow_pass keeps its struct (the targets
 * are copied, their images stay the caller's). NULL clears. UR_EINVAL for a null frame, a null target other than object_id, and what
 * ur_gbuffer_pass refuses in the draws, the alignment, the flags and the key bits.
 * Not checked, here or at render: that targets.keys and targets.object_id hold rows * w elements. The band is the resources' row0 and
 * rows of the frame being rendered, which this call cannot know; gbuf_a/b/c and hdr are held to the resources' own images at render,
 * keys and object_id are the caller's to size for every band rendered with this pass. A row0 / rows of the resources that does not
 * fit their h is ur_gbuffer_pass' UR_EINVAL: ur_frame_render returns it (the first failing pass' code; the passes behind it still run). */
typedef struct ur_frame_gbuffer_pass {
    ur_raster_draws draws;
    ur_gbuffer_targets targets;
    uint32_t* stats6;
    uint32_t flags;
    uint32_t key_triangle_bits;
} ur_frame_gbuffer_pass;
int ur_frame_set_gbuffer_pass(ur_frame* f, const ur_frame_gbuffer_pass* pass);

/* The material table of the "GBuffer" pass (ur_material, include/ur_raster.h): with UR_FRAME_GBUFFER_PASS and a table
 * set, the pass is ur_gbuffer_pass_materials with it - one record per command slot of ur_frame_set_gbuffer_pass' draws, slots
 * >= material_count resolve as key 0. materials: device, 16-byte aligned, read at render by every following frame until it is replaced;
 * NULL clears it (material_count is then ignored). Without a table the pass list, the launches and the bytes are what they are without
 * this call. There is no flag and ur_frame_gbuffer_pass has no member for it. UR_EINVAL: a null frame, a misaligned table. */
int ur_frame_set_gbuffer_materials(ur_frame* f, const ur_material* materials, uint32_t material_count);
/* Last execution: one line per pass "name|culled(0/1)|transitions|async(0/1)|cross-stream waits". Returns bytes needed (incl. NUL). */
uint32_t ur_frame_report(const ur_frame* f, char* buf, uint32_t cap);
/* Sliding-window GPU timing (FRenderGraph::GetGpuTimingStats): "name|avg_ms|min_ms|max_ms|samples" lines. */
uint32_t ur_rg_timing_stats(char* buf, uint32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* UR_FRAME_H */
