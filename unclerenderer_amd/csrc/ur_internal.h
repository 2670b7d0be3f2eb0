// Internal declarations shared by the C-ABI translation units. Not installed.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/ur_hotpath.h"
#include "../../include/ur_raster.h"

#include "hzb_plan.h" // ur::kTailMaxLevels, ur::kTailTexels

namespace ur_envc { struct Plan; } // csrc/env_cube_rule.h

namespace ur {
// Arguments of the single-workgroup tail of the HZB chain (csrc/hzb_tail.h): the levels from `first_mip` on.
constexpr uint32_t kClaimWords = 32, kClaimWordStride = 32; // (stride in uint32: 128 bytes)
struct HzbTail {
    const float* src; // mip first_mip - 1 (global memory, written by the previous launch)
    uint32_t SW, SH, first_mip, levels;
    float* dst[kTailMaxLevels];
    uint32_t W[kTailMaxLevels], H[kTailMaxLevels];
    uint32_t magic[kTailMaxLevels]; // i / W[l] == __umulhi(i, magic[l]) for i < 16384 (magic = 2^32 / W + 1)
};
} // namespace ur
#include "hzb_wide.h"

namespace ur {
// The held-back Build HZB chain of a context (ur_defer_hzb_tail), and the only code that touches that state. The HZB tail may ride
// along with the next streaming Lighting launch as one extra workgroup: its single workgroup is ~5 us of latency during which the
// other 255 CUs would idle. ur_defer_hzb_tail(ctx, 2): the wide launch in front of the tail is held back too; the Lighting launch's
// workgroups take its 128x32 pieces along (one wave of each) and signal `hzb_done`, which the riding tail workgroup waits for.
// Whoever launches what is held launches the wide step before the tail (the tail reads what it writes); taking a step clears it;
// ur_destroy discards both and launches neither.
class HeldHzb {
public:
    struct Wide { HzbDispatch d; uint32_t grid_x, grid_y; };
    int mode() const { return mode_; } // ur_defer_hzb_tail's: 0 off, 1 tail, 2 whole chain
    // true: the new mode is narrower than the old one, and what is held has to go out (flush_hzb_tail)
    bool set_mode(int mode)
    {
        const bool narrower = (mode == 0) || (mode == 1 && mode_ == 2);
        mode_ = mode;
        return narrower;
    }
    void hold_tail(const HzbTail& t) { tail_ = t; has_tail_ = true; }
    void hold_wide(const HzbDispatch& d, uint32_t grid_x, uint32_t grid_y) { wide_ = Wide{d, grid_x, grid_y}; has_wide_ = true; }
    bool has_tail() const { return has_tail_; }
    bool has_wide() const { return has_wide_; }
    uint32_t wide_grid_x() const { return wide_.grid_x; } // (of the step held now or last: what plan_stream is told beside has_wide)
    uint32_t wide_grid_y() const { return wide_.grid_y; }
    const HzbTail& take_tail() { has_tail_ = false; return tail_; } // (valid until the next hold_tail)
    const Wide& take_wide() { has_wide_ = false; return wide_; }
    void discard() { has_tail_ = has_wide_ = false; }

private:
    int mode_ = 0;
    bool has_tail_ = false, has_wide_ = false;
    HzbTail tail_{};
    Wide wide_{};
};
} // namespace ur

struct ur_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // compaction workspace (grown by ur_reserve / lazily outside graph capture)
    // 1 + UR_MAX_CULL_VIEWS slices of ws_instances / 256 block counts (and 4x as many masks): the camera's, then one per view
    uint32_t* block_counts = nullptr; // one per 256-instance block
    uint64_t* wave_masks = nullptr;   // one per 64 instances
    uint32_t ws_instances = 0;
    // UR_OPT_CULL_STORE = 4: wave_masks describes the InstanceCount words of this command buffer / count (the last multi-block launch's)
    const void* cull_record_args = nullptr;
    uint32_t cull_record_n = 0;
    // sRGB8 -> linear table (256 floats), uploaded once
    float* srgb_table = nullptr;
    // linear -> sRGB8 thresholds (255 floats, ur_host_srgb_encode_table), uploaded once: the GBuffer resolve's encode
    float* srgb_encode_table = nullptr;
    // 127 thresholds 2^(j / 128) (ur_host_lod_table), uploaded once: the textured GBuffer resolve's level of detail
    float* lod_table = nullptr;
    int cu_count = 256;
    ur::HeldHzb held_hzb; // ur_defer_hzb_tail's mode and what it holds back of a Build HZB chain
    // ur_debug_timeline: device array of {first entry, last exit} pairs in s_memrealtime ticks (100 MHz), one pair per cull and per
    // streaming Lighting launch, in launch order (the caller initialises every pair to {~0, 0})
    unsigned long long* timeline = nullptr;
    uint32_t timeline_cap = 0, timeline_pos = 0;
    uint32_t* hzb_done = nullptr; // device: arrivals of the current launch (reset by the tail workgroup)
    // the riding tail's time-out flag: one word of mapped, coherent host memory the kernel writes (system scope) and the host
    // reads without a synchronisation at its next entry point that depends on the HZB (check_hzb_timeout)
    volatile uint32_t* hzb_timed_out = nullptr;
    uint32_t* hzb_timed_out_dev = nullptr; // its device address
    // ur_time_next_lighting: events the next Lighting launch carries on its dispatch (hipExtLaunchKernel); consumed by it
    hipEvent_t time_start = nullptr, time_stop = nullptr;
    hipEvent_t time_cull_stop = nullptr; // ur_time_next_cull: carried by the last launch of the next cull call, cleared by that call
    bool time_cull_carried = false;      // ... and whether a dispatch of that call took it (ur_time_cull_carried)
    // ur_set_option: launch-shape choices of this context (include/ur_hotpath.h, UR_OPT_*)
    struct Options {
        int lighting_stream = 1, lighting_wpb = 16, tiled_waves = 6, leave_cus = 0, ride_walkers = 0, cull_store = 3;
        int balance = 1, balance_pool_16ths = 3, balance_chunk_shift = 4;
        int debug_hzb_ride_stall = 0;
        int taa_tonemap_history_store = 0;
    } opt;
    // Inter-workgroup tile claims of the streaming lighting kernel (UR_OPT_LIGHTING_BALANCE): kClaimWords words, each on a 128-byte
    // line of its own, + the count of workgroups that have made their last claim. All zero between launches: the workgroup whose
    // last claim comes last zeroes them (csrc/lighting.hip; the split is planned in csrc/lighting_plan.cpp).
    uint32_t* claim_words = nullptr;
    uint32_t last_schedule[8] = {}; // ur_debug_lighting_schedule: the tile schedule of the context's last streaming Lighting launch (StreamPlan::reported)
    // host-visible (mapped, coherent) word beside hzb_timed_out: a wave of a balanced launch gave up waiting for a claim
    volatile uint32_t* claim_timed_out = nullptr;
    uint32_t* claim_timed_out_dev = nullptr;
    // ur_raster_reserve: the large-triangle queue of the raster passes (csrc/raster_params.h has its layout, csrc/raster_kernels.h its kernels): a 64-byte header (the count) + entries
    uint32_t* raster_queue = nullptr;
    uint32_t raster_queue_cap = 0;
};

#include "ur_checks.h" // ur::set_error, ur::raster_commands and the check_* functions: what host callers outside the C-ABI units need

namespace ur {

#define UR_HIP_TRY(expr)                                                                          \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            ::ur::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return UR_EHIP;                                                                       \
        }                                                                                         \
    } while (0)

// kernels (one file each)
int launch_build_hzb(ur_ctx* ctx, const float* depth, uint32_t src_w, uint32_t src_h, float* hzb_base,
                     const ur_mip_desc* mips, uint32_t mip_count);
int launch_build_hzb_band(ur_ctx* ctx, const float* depth, uint32_t src_w, uint32_t src_h, float* hzb_base, const ur_mip_desc* mips, uint32_t mip_count,
                          uint32_t piece_row0, uint32_t piece_rows);
int launch_build_hzb_tail(ur_ctx* ctx, float* hzb_base, const ur_mip_desc* mips, uint32_t mip_count);
int launch_cull(ur_ctx* ctx, const uint32_t* constants, const ur_float4* bounds, const float* hzb_base,
                const ur_mip_desc* mips, void* indirect_args, uint32_t* stats2, uint32_t* visible_idx,
                uint32_t* visible_count, uint32_t index_base, const ur_draw_ranges* draws, const ur_cull_view* views,
                uint32_t view_count);
// launch_cull with views (cull_views.hip), after launch_cull has flushed the HZB tail
int launch_cull_views(ur_ctx* ctx, const uint32_t* constants, const ur_float4* bounds, const float* hzb_base,
                      const ur_mip_desc* mips, void* indirect_args, uint32_t* stats2, uint32_t* visible_idx,
                      uint32_t* visible_count, uint32_t index_base, const ur_draw_ranges* draws, const ur_cull_view* views,
                      uint32_t view_count);
// GBuffer's raster (UR_GBUFFER_PART_RASTER): clears the key image of the band [row0, row0 + rows) and raises it to the winning keys
int launch_visibility_raster(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, const float* depth, uint32_t* keys, uint32_t w,
                             uint32_t h, uint32_t row0, uint32_t rows, uint32_t key_bits, bool d24, uint32_t* stats);
// GBuffer's masked raster and merge, behind launch_visibility_raster over the opaque draws: clears the 64-bit words of the
// band, raises them to the winning masked fragments, folds them into `keys` and raises `depth` in the band's rows where one won
int launch_masked_raster(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, float* depth, uint64_t* keys64, uint32_t* keys,
                         uint32_t w, uint32_t h, uint32_t row0, uint32_t rows, uint32_t key_bits, bool d24, uint32_t* stats, const ur_material* materials,
                         uint32_t material_count, uint32_t* won);
// The pick: zeroes point_count records, raises their first 8 bytes to the winning (key, depth bits) of the selected
// draws at the points (host, x | y << 16, inside the w x h target) and finishes them into ur_pick_result records
int launch_object_id_pick(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, const float* depth, uint32_t w, uint32_t h,
                          uint32_t key_bits, bool d24, const uint32_t* points, uint32_t point_count, ur_pick_result* results, uint32_t* stats);
int launch_lighting(ur_ctx* ctx, const ur_scene_constants* scene, const ur_sky_constants* sky, const ur_half4* gbuf_a,
                    const ur_half4* gbuf_b, const uint32_t* gbuf_c, const float* depth, const ur_lighting_tables* tables,
                    ur_half4* hdr, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows, int mode);
enum { UR_MODE_LIGHTING = 0, UR_MODE_SKY = 1, UR_MODE_FUSED = 2 };
// GpuDebugPrint (debug_print.hip); arguments checked by the entry points beside them
int launch_debug_print_reset(ur_ctx* ctx, void* buffer, uint32_t* stats);
int launch_debug_print_stats(ur_ctx* ctx, const uint32_t* stats, void* buffer);
int launch_debug_print_text(ur_ctx* ctx, void* buffer, uint32_t x, uint32_t y, uint32_t color, const char* text, uint32_t length);
int launch_debug_print_draw(ur_ctx* ctx, const ur_debug_print_constants* constants, const ur_debug_glyph* glyphs, uint32_t glyph_count,
                            const uint8_t* atlas_r8, uint32_t atlas_w, uint32_t atlas_h, const void* buffer, uint32_t* ldr_inout, uint32_t w,
                            uint32_t row0, uint32_t rows);
// (env_cube_build.hip) the bordered section of the staged cube from an RGBA16F payload: ur_env_cube_build's decode and border launches
void launch_env_cube_bordered(hipStream_t stream, const ur_envc::Plan& p, const void* src, uint64_t* dst);
// the next {entry, exit} pair of the debug timeline (nullptr when it is off)
inline unsigned long long* next_timeline_pair(ur_ctx* ctx)
{
    if (!ctx->timeline || ctx->timeline_pos >= ctx->timeline_cap) return nullptr; // full: later launches stamp nothing
    return ctx->timeline + 2u * (size_t)ctx->timeline_pos++;
}
// launches a deferred HZB tail on its own if one is pending (ur_flush and every launch that reads or rewrites the HZB)
int flush_hzb_tail(ur_ctx* ctx);
// UR_ETIMEOUT (once) if a riding tail has given up waiting since the last check: clears the flag and resets the arrival
// counter on the context's stream (the call that reports it does nothing else); UR_OK otherwise
int check_hzb_timeout(ur_ctx* ctx, const char* who);

} // namespace ur
