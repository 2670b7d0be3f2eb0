// C-ABI of include/ur_hotpath.h: the error text, context and workspace management, options and timers, setup-time staging, and the
// Lighting and Sky entry points. The other entry points live beside their launches: Build HZB's in hzb.hip (its host decisions in
// hzb_plan.cpp), the cull's in cull_api.hip, GpuDebugPrint's in debug_print.hip, the all-gather in gather.hip.
// The kernels live in hzb.hip, cull.hip, lighting.hip and lighting_tiled.hip; Lighting's host side in lighting_host.hip and lighting_plan.cpp.

#include <cstdarg>
#include <cstring>
#include <vector>

#include "ur_internal.h"
#include "lighting_plan.h"

#include "../../include/ur_host.h"

namespace ur {

static thread_local char g_error[512] = "";

void set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

} // namespace ur

using ur::set_error;

namespace {

// ur_create: a device table of `bytes` bytes with the contents of `host`, or zeroed when there are none, filled on the context's own
// stream: everything the context launches is queued behind it, and creating a context waits for no other stream (a frame creates its
// async lane's context inside its first UR_FRAME_ASYNC_COMPUTE render). `host` outlives the copy. false: `what` is the error text
template <class T>
bool upload_table(hipStream_t stream, T** device, const T* host, size_t bytes, const char* what)
{
    if (hipMalloc(device, bytes) == hipSuccess &&
        (host ? hipMemcpyAsync(*device, host, bytes, hipMemcpyHostToDevice, stream) : hipMemsetAsync(*device, 0, bytes, stream)) == hipSuccess) return true;
    set_error("%s", what);
    return false;
}

// the three tables every context uploads, computed once
struct HostTables {
    float decode[256]; // sRGB8 -> linear (exact IEC 61966-2-1 curve, evaluated in double)
    float encode[255];
    float lod[127];
    HostTables()
    {
        ur_host_srgb_decode_table(decode);
        ur_host_srgb_encode_table(encode);
        ur_host_lod_table(lod);
    }
};

} // namespace

extern "C" {

const char* ur_last_error(void) { return ur::g_error; }
const char* ur_version(void) { return "unclerenderer_amd hotpath 0.5 (gfx950)"; }

ur_ctx* ur_create(int device, void* stream)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) {
        set_error("ur_create: no HIP device %d (count %d)", device, count);
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) {
        set_error("ur_create: hipSetDevice(%d) failed", device);
        return nullptr;
    }
    ur_ctx* ctx = new ur_ctx();
    ctx->device = device;
    ctx->stream = static_cast<hipStream_t>(stream);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    static const HostTables tables; // (static: the copies below are asynchronous)
    if (!upload_table<float>(ctx->stream, &ctx->srgb_table, tables.decode, sizeof(tables.decode), "ur_create: sRGB table upload failed") ||
        !upload_table<float>(ctx->stream, &ctx->srgb_encode_table, tables.encode, sizeof(tables.encode), "ur_create: sRGB encode table upload failed") ||
        !upload_table<float>(ctx->stream, &ctx->lod_table, tables.lod, sizeof(tables.lod), "ur_create: level-of-detail table upload failed") ||
        !upload_table<uint32_t>(ctx->stream, &ctx->hzb_done, nullptr, 64, "ur_create: HZB arrival counter allocation failed")) {
        ur_destroy(ctx);
        return nullptr;
    }
    {
        void* host = nullptr;
        void* devp = nullptr;
        if (hipHostMalloc(&host, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess || hipHostGetDevicePointer(&devp, host, 0) != hipSuccess) {
            if (host) (void)hipHostFree(host);
            set_error("ur_create: host-visible time-out flag allocation failed");
            ur_destroy(ctx);
            return nullptr;
        }
        ctx->hzb_timed_out = static_cast<volatile uint32_t*>(host);
        ctx->hzb_timed_out_dev = static_cast<uint32_t*>(devp);
        *ctx->hzb_timed_out = 0u;
        ctx->claim_timed_out = ctx->hzb_timed_out + 1;
        ctx->claim_timed_out_dev = ctx->hzb_timed_out_dev + 1;
        *ctx->claim_timed_out = 0u;
    }
    if (!upload_table<uint32_t>(ctx->stream, &ctx->claim_words, nullptr, (ur::kClaimWords + 1u) * ur::kClaimWordStride * sizeof(uint32_t),
                      "ur_create: tile-claim words allocation failed")) {
        ur_destroy(ctx);
        return nullptr;
    }
    if (ur_reserve(ctx, 1u << 20) != UR_OK) {
        ur_destroy(ctx);
        return nullptr;
    }
    return ctx;
}

void ur_destroy(ur_ctx* ctx)
{
    if (!ctx) return;
    // A held-back HZB tail is DISCARDED, not launched: the caller may already have freed the HZB buffer it points into (the
    // chain is complete only after ur_flush or a streaming Lighting launch — see ur_build_hzb in the header).
    ctx->held_hzb.discard();
    if (ctx->hzb_done) (void)hipFree(ctx->hzb_done);
    if (ctx->claim_words) (void)hipFree(ctx->claim_words);
    if (ctx->hzb_timed_out) (void)hipHostFree(const_cast<uint32_t*>(ctx->hzb_timed_out));
    if (ctx->srgb_table) (void)hipFree(ctx->srgb_table);
    if (ctx->srgb_encode_table) (void)hipFree(ctx->srgb_encode_table);
    if (ctx->lod_table) (void)hipFree(ctx->lod_table);
    if (ctx->block_counts) (void)hipFree(ctx->block_counts);
    if (ctx->wave_masks) (void)hipFree(ctx->wave_masks);
    if (ctx->raster_queue) (void)hipFree(ctx->raster_queue);
    delete ctx;
}

int ur_debug_timeline(ur_ctx* ctx, unsigned long long* device_pairs, uint32_t capacity_pairs)
{
    if (!ctx || (device_pairs != nullptr && capacity_pairs == 0)) { set_error("ur_debug_timeline: bad argument"); return UR_EINVAL; }
    ctx->timeline = device_pairs;
    ctx->timeline_cap = device_pairs ? capacity_pairs : 0u;
    ctx->timeline_pos = 0;
    return UR_OK;
}

int ur_time_next_lighting(ur_ctx* ctx, void* start_event, void* stop_event)
{
    if (!ctx || (start_event != nullptr && stop_event == nullptr)) { set_error("ur_time_next_lighting: a start event needs a stop event"); return UR_EINVAL; }
    ctx->time_start = static_cast<hipEvent_t>(start_event);
    ctx->time_stop = static_cast<hipEvent_t>(stop_event);
    return UR_OK;
}

int ur_time_next_cull(ur_ctx* ctx, void* stop_event)
{
    if (!ctx) { set_error("ur_time_next_cull: null context"); return UR_EINVAL; }
    ctx->time_cull_stop = static_cast<hipEvent_t>(stop_event);
    ctx->time_cull_carried = false; // (arming or clearing: nothing has carried THIS event)
    return UR_OK;
}

int ur_time_cull_carried(const ur_ctx* ctx) { return ctx && ctx->time_cull_carried ? 1 : 0; }

// option -> (field, lowest, highest, only these two values when `pair`)
namespace {
struct OptionSlot { int ur_ctx::Options::*field; int lo, hi; bool pair; };
bool option_slot(int option, OptionSlot& o)
{
    typedef ur_ctx::Options O;
    switch (option) {
    case UR_OPT_LIGHTING_STREAM: o = {&O::lighting_stream, 0, 1, false}; return true;
    case UR_OPT_LIGHTING_WAVES_PER_WG: o = {&O::lighting_wpb, 12, 16, true}; return true;
    case UR_OPT_LIGHTING_TILED_WAVES: o = {&O::tiled_waves, 4, 6, true}; return true;
    case UR_OPT_LIGHTING_LEAVE_CUS: o = {&O::leave_cus, 0, 128, false}; return true;
    case UR_OPT_RIDE_WALKERS: o = {&O::ride_walkers, 0, 16, false}; return true;
    case UR_OPT_CULL_STORE: o = {&O::cull_store, 0, 4, false}; return true;
    case UR_OPT_LIGHTING_BALANCE: o = {&O::balance, 0, 1, false}; return true;
    case UR_OPT_BALANCE_POOL_16THS: o = {&O::balance_pool_16ths, 1, 8, false}; return true;
    case UR_OPT_BALANCE_CHUNK_SHIFT: o = {&O::balance_chunk_shift, 2, 6, false}; return true;
    case UR_OPT_DEBUG_HZB_RIDE_STALL: o = {&O::debug_hzb_ride_stall, 0, 1, false}; return true;
    case UR_OPT_TAA_TONEMAP_HISTORY_STORE: o = {&O::taa_tonemap_history_store, 0, 1, false}; return true;
    default: return false;
    }
}
} // namespace

int ur_set_option(ur_ctx* ctx, int option, int value)
{
    OptionSlot o;
    if (!ctx || !option_slot(option, o)) { set_error("ur_set_option: unknown option %d", option); return UR_EINVAL; }
    if (value < o.lo || value > o.hi || (o.pair && value != o.lo && value != o.hi)) {
        set_error("ur_set_option: option %d takes %d%s%d, not %d", option, o.lo, o.pair ? " or " : " .. ", o.hi, value);
        return UR_EINVAL;
    }
    ctx->opt.*(o.field) = value;
    if (option == UR_OPT_CULL_STORE) ctx->cull_record_args = nullptr; // (setting it - also to the value it has - forgets the record of flavour 4)
    return UR_OK;
}

int ur_get_option(const ur_ctx* ctx, int option, int* value)
{
    OptionSlot o;
    if (!ctx || !value || !option_slot(option, o)) { set_error("ur_get_option: unknown option %d", option); return UR_EINVAL; }
    *value = ctx->opt.*(o.field);
    return UR_OK;
}

int ur_debug_lighting_schedule(const ur_ctx* ctx, uint32_t out8[8])
{
    if (!ctx || !out8) { set_error("ur_debug_lighting_schedule: null argument"); return UR_EINVAL; }
    std::memcpy(out8, ctx->last_schedule, sizeof(ctx->last_schedule));
    return UR_OK;
}

int ur_debug_set_hzb_timeout(ur_ctx* ctx)
{
    if (!ctx || !ctx->hzb_timed_out) { set_error("ur_debug_set_hzb_timeout: null context"); return UR_EINVAL; }
    *ctx->hzb_timed_out = 1u; // what the riding tail workgroup writes when it gives up
    return UR_OK;
}

int ur_reserve(ur_ctx* ctx, uint32_t max_instances)
{
    if (!ctx) return UR_EINVAL;
    if (max_instances <= ctx->ws_instances) return UR_OK;
    UR_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->block_counts) (void)hipFree(ctx->block_counts);
    if (ctx->wave_masks) (void)hipFree(ctx->wave_masks);
    ctx->block_counts = nullptr; ctx->wave_masks = nullptr; ctx->ws_instances = 0;
    ctx->cull_record_args = nullptr;
    const size_t blocks = ((size_t)max_instances + 255u) / 256u;
    const size_t slices = 1u + UR_MAX_CULL_VIEWS; // the camera's, then one per extra view (ur_cull_indirect_args_views)
    if (hipMalloc(&ctx->block_counts, slices * blocks * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&ctx->wave_masks, slices * blocks * 4u * sizeof(uint64_t)) != hipSuccess) {
        set_error("ur_reserve: workspace allocation for %u instances failed", max_instances);
        return UR_ENOMEM;
    }
    ctx->ws_instances = (uint32_t)(blocks * 256u);
    return UR_OK;
}

size_t ur_env_cube_texels(uint32_t base_size, uint32_t mip_count)
{
    return (size_t)ur::cube_layout(base_size, mip_count).texels; // (0: refused)
}

int ur_stage_env_cube(ur_ctx* ctx, const ur_half4* src, uint32_t base, uint32_t mip_count, ur_half4* dst_device)
{
    const ur::CubeLayout L = ur::cube_layout(base, mip_count); // csrc/lighting_plan.h: the two sections written below
    if (!ctx || !src || !dst_device || L.texels == 0) { set_error("ur_stage_env_cube: bad argument"); return UR_EINVAL; }
    std::vector<ur_half4> out(L.texels);
    ur::stage_env_cube_host(src, L, out.data());
    UR_HIP_TRY(hipMemcpy(dst_device, out.data(), out.size() * sizeof(ur_half4), hipMemcpyHostToDevice));
    return UR_OK;
}

int ur_deferred_lighting(ur_ctx* ctx, const ur_scene_constants* scene, const ur_half4* a, const ur_half4* b, const uint32_t* c,
                         const ur_lighting_tables* tables, ur_half4* hdr, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    const int rc = ur::check_band("ur_deferred_lighting", ctx, w, h, row0, rows);
    if (rc != UR_OK) return rc;
    if (!scene || !a || !b || !c || !tables || !hdr) { set_error("ur_deferred_lighting: null argument"); return UR_EINVAL; }
    const int trc = ur::check_hzb_timeout(ctx, "ur_deferred_lighting"); // (a launch behind one that gave up must not start from its leftovers)
    if (trc != UR_OK) return trc;
    return ur::launch_lighting(ctx, scene, nullptr, a, b, c, nullptr, tables, hdr, w, h, row0, rows, ur::UR_MODE_LIGHTING);
}

int ur_sky_atmosphere(ur_ctx* ctx, const ur_sky_constants* sky, const float* depth, ur_half4* hdr, uint32_t w, uint32_t h,
                      uint32_t row0, uint32_t rows)
{
    const int rc = ur::check_band("ur_sky_atmosphere", ctx, w, h, row0, rows);
    if (rc != UR_OK) return rc;
    if (!sky || !depth || !hdr) { set_error("ur_sky_atmosphere: null argument"); return UR_EINVAL; }
    return ur::launch_lighting(ctx, nullptr, sky, nullptr, nullptr, nullptr, depth, nullptr, hdr, w, h, row0, rows, ur::UR_MODE_SKY);
}

int ur_deferred_lighting_sky(ur_ctx* ctx, const ur_scene_constants* scene, const ur_sky_constants* sky, const ur_half4* a,
                             const ur_half4* b, const uint32_t* c, const float* depth, const ur_lighting_tables* tables,
                             ur_half4* hdr, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    const int rc = ur::check_band("ur_deferred_lighting_sky", ctx, w, h, row0, rows);
    if (rc != UR_OK) return rc;
    if (!scene || !sky || !a || !b || !c || !depth || !tables || !hdr) { set_error("ur_deferred_lighting_sky: null argument"); return UR_EINVAL; }
    const int trc = ur::check_hzb_timeout(ctx, "ur_deferred_lighting_sky");
    if (trc != UR_OK) return trc;
    return ur::launch_lighting(ctx, scene, sky, a, b, c, depth, tables, hdr, w, h, row0, rows, ur::UR_MODE_FUSED);
}

} // extern "C"
