// frame_trace.cpp — the frame units (csrc/frame/*.cpp + csrc/rg/RenderGraph.cpp) traced on the CPU: every entry point they link against is a
// recording stand-in here (no GPU work, no HIP runtime), and what the frame asks of them is compared with a recording of the parent.
//
//   frame_trace --record          print the golden (tests/golden/frame_traces.txt): the curated cases, then one FNV-1a digest per cell of the two sweeps
//   frame_trace --check GOLDEN    compare with it; a mismatch names the first differing case or cell and prints its trace in full
//   frame_trace --case NAME       print one case's trace in full (a curated name, scene:<bits>, or post:<bits>:<world>:<ring>)
//
// A trace line is an entry point with every scalar argument and every constant-struct field the frame fills. Pointers are written as
// <buffer>+<byte offset> from the table of fake buffers below, the context as main / async, events in order of first appearance in a case.
// After each ur_frame_render / ur_frame_finish_post: the return code, ur_last_error's text on failure, ur_frame_report,
// ur_frame_hzb_ready, ur_frame_taa_next. (The persistent resource states are not visible through the C face; the report's transition
// counts are what they produce.)
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/ur_frame.h"
#include "../../include/ur_host.h"
#include "../../unclerenderer_amd/csrc/rg/RenderGraph.h"
#include "../../unclerenderer_amd/csrc/ur_checks.h"

struct ur_ctx { const char* name; };

namespace {

std::string g_trace, g_error;
std::map<std::string, int> g_calls, g_fail; // fail the n-th call of a named entry point
std::map<const void*, int> g_events;
std::set<uintptr_t> g_mallocs;
int g_malloc_next = 0;
void* g_cull_event = nullptr;
bool g_cull_carried = false;
ur_ctx g_main{"main"};

void T(const char* fmt, ...)
{
    char buf[2048];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_trace += buf;
    g_trace += '\n';
}

// ---- fake device buffers: buffer i lives at (i + 1) << 32 -------------------------------------------------------------------------------
const char* const kBuffers[] = {
    "gbuffer_a", "gbuffer_b", "gbuffer_c", "depth_band", "lighting_band", "depth_full", "hzb", "shadow_map", "env_cube", "brdf_lut", "model_bounds",
    "indirect_args", "visible_indices", "visible_count", "cull_stats", "tonemap_band", "tonemap_scratch", "luminance0", "luminance1", "taa_history0",
    "taa_history1", "taa_history2", "post_record", "post_records", "taa_record", "taa_records", "debug_buffer", "debug_glyphs", "debug_atlas",
    "range_offsets", "range_commands", "range_counts", "view_mask", "view_idx", "view_count", "view_offsets", "view_commands", "view_counts",
    "shadow_commands", "shadow_stats", "depth_commands", "depth_stats", "gbuffer_commands", "gbuffer_stats", "gbuffer_keys", "object_id", "materials",
    "stream_main", "other_shadow_map"};
constexpr size_t kBufferCount = sizeof kBuffers / sizeof *kBuffers;
constexpr uintptr_t kMallocBase = 0x7f0000000000ull;

void* B(const char* name, uint64_t off = 0)
{
    for (size_t i = 0; i < kBufferCount; ++i)
        if (!strcmp(kBuffers[i], name)) return reinterpret_cast<void*>(((i + 1) << 32) + off);
    fprintf(stderr, "no fake buffer %s\n", name);
    abort();
}
template <class X> X* BT(const char* name, uint64_t off = 0) { return static_cast<X*>(B(name, off)); }

std::string P(const void* p)
{
    if (!p) return "null";
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    char buf[64];
    if (a >= kMallocBase && a < kMallocBase + (1ull << 40)) {
        snprintf(buf, sizeof buf, "hipMalloc%u+%llu", unsigned((a - kMallocBase) >> 28), (unsigned long long)((a - kMallocBase) & 0xfffffffull));
        return buf;
    }
    const uintptr_t i = (a >> 32) - 1;
    if ((a >> 32) == 0 || i >= kBufferCount) return "?";
    snprintf(buf, sizeof buf, "%s+%llu", kBuffers[i], (unsigned long long)(a & 0xffffffffull));
    return buf;
}
#define PS(p) P(p).c_str()

std::string E(const void* e)
{
    if (!e) return "null";
    auto it = g_events.find(e);
    if (it == g_events.end()) it = g_events.emplace(e, int(g_events.size())).first;
    return "ev" + std::to_string(it->second);
}
#define ES(e) E(e).c_str()
const char* S(const void* s) { return s == B("stream_main") ? "main" : s ? "async" : "null"; }

uint64_t fnv(const void* data, size_t n, uint64_t h = 0xcbf29ce484222325ull)
{
    const unsigned char* p = static_cast<const unsigned char*>(data);
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h;
}
template <class X> unsigned long long H(const X* x) { return x ? (unsigned long long)fnv(x, sizeof(X)) : 0ull; }
unsigned long long HM(const float* m) { return m ? (unsigned long long)fnv(m, 64) : 0ull; }

// The call's outcome: UR_OK, or UR_EHIP when the case asked for this call of `name` to fail. Closes the trace line.
int R(const char* name)
{
    const int n = ++g_calls[name];
    auto it = g_fail.find(name);
    const int rc = it != g_fail.end() && it->second == n ? UR_EHIP : UR_OK;
    if (rc != UR_OK) { g_trace.insert(g_trace.size() - 1, " -> " + std::to_string(rc)); ur::set_error("%s: failed on request", name); }
    return rc;
}

std::string ranges(const ur_draw_ranges* d)
{
    if (!d) return "null";
    return "{" + P(d->offsets) + " n=" + std::to_string(d->range_count) + " " + P(d->commands) + " " + P(d->counts) + "}";
}
std::string draws(const ur_raster_draws* d)
{
    if (!d) return "null";
    return "{" + P(d->commands) + " n=" + std::to_string(d->command_count) + " " + P(d->visible_idx) + " " + P(d->visible_count) + " base=" +
           std::to_string(d->index_base) + " ranges=" + ranges(d->ranges) + "}";
}
std::string tonemap(const ur_tonemap_constants* k)
{
    char buf[128];
    snprintf(buf, sizeof buf, "{%u %u %.9g %.9g}", k->EnableTonemap, k->EnableAutoExposure, k->Exposure, k->Gamma);
    return buf;
}
std::string cas(const ur_cas_constants* k)
{
    char buf[128];
    snprintf(buf, sizeof buf, "{%.9g %.9g %.9g %.9g}", k->TexelDelta[0], k->TexelDelta[1], k->Sharpness, k->Padding);
    return buf;
}

} // namespace

// ---- stand-ins: ur:: ---------------------------------------------------------------------------------------------------------------------
namespace ur {
void set_error(const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
}
int check_cull_views(const ur_cull_view* views, uint32_t n)
{
    T("check_cull_views n=%u", n);
    (void)views;
    return R("check_cull_views");
}
int check_raster_draws(const char* who, const ur_raster_draws& d, const void* target, const char* target_name, const void* stats)
{
    T("check_raster_draws %s %s %s=%s stats=%s", who, draws(&d).c_str(), target_name, PS(target), PS(stats));
    return R("check_raster_draws");
}
int check_gbuffer_targets(const char* who, const ur_gbuffer_targets* t)
{
    T("check_gbuffer_targets %s {%s %s %s %s %s %s}", who, PS(t->gbuf_a), PS(t->gbuf_b), PS(t->gbuf_c), PS(t->hdr), PS(t->object_id), PS(t->keys));
    return R("check_gbuffer_targets");
}
} // namespace ur

// ---- stand-ins: the HIP runtime (tokens, no device) ----------------------------------------------------------------------------------------
extern "C" {
int hipMalloc(void** p, size_t n)
{
    T("hipMalloc %zu", n);
    if (R("hipMalloc") != UR_OK) return 2; // hipErrorOutOfMemory
    const uintptr_t a = kMallocBase + (uintptr_t(g_malloc_next++) << 28);
    g_mallocs.insert(a);
    *p = reinterpret_cast<void*>(a);
    g_trace.insert(g_trace.size() - 1, " = " + P(*p));
    return 0;
}
int hipFree(void* p)
{
    T("hipFree %s", PS(p));
    g_mallocs.erase(reinterpret_cast<uintptr_t>(p));
    return 0;
}
// (creation, destruction and queries of events are not traced: the render graph pools its events for the process, the trace of a case must not depend on the cases before it)
// (and events are tokens, not allocations: the render graph keeps its pooled events and a context's join event for the life of the process)
static uintptr_t g_event_next = 0x7e0000000000ull;
int hipEventCreate(void** e) { *e = reinterpret_cast<void*>(g_event_next += 16); return 0; }
int hipEventCreateWithFlags(void** e, unsigned) { return hipEventCreate(e); }
int hipEventDestroy(void*) { return 0; }
int hipEventQuery(void*) { return 0; }
int hipEventRecord(void* e, void* s) { T("hipEventRecord %s %s", ES(e), S(s)); return 0; }
int hipStreamWaitEvent(void* s, void* e, unsigned) { T("hipStreamWaitEvent %s %s", S(s), ES(e)); return 0; }
int hipEventElapsedTime(float* ms, void* a, void* b) { T("hipEventElapsedTime %s %s", ES(a), ES(b)); *ms = 0.25f; return 0; }
int hipGetDevice(int* d) { *d = 0; return 0; }
int hipStreamCreateWithPriority(void** s, unsigned flags, int priority)
{
    T("hipStreamCreateWithPriority flags=%u priority=%d", flags, priority);
    if (R("hipStreamCreateWithPriority") != UR_OK) return 1;
    *s = new char;
    return 0;
}
int hipStreamDestroy(void* s) { T("hipStreamDestroy %s", S(s)); delete static_cast<char*>(s); return 0; }
int hipStreamSynchronize(void* s) { T("hipStreamSynchronize %s", S(s)); return 0; }

// ---- stand-ins: the C ABI of the kernels ----------------------------------------------------------------------------------------------------
#define C (ctx ? ctx->name : "null")
const char* ur_last_error(void) { return g_error.c_str(); }
ur_ctx* ur_create(int device, void* stream) { T("ur_create %d %s", device, S(stream)); return R("ur_create") == UR_OK ? new ur_ctx{"async"} : nullptr; }
void ur_destroy(ur_ctx* ctx) { T("ur_destroy %s", C); delete ctx; }
uint64_t ur_post_record_bytes(uint32_t w) { return (2ull * w + 1024u) * 8u; }
uint64_t ur_taa_record_bytes(uint32_t w) { return 4ull * w * 8u; }
uint64_t ur_debug_print_buffer_bytes(void) { return 4u + (uint64_t)UR_DEBUG_PRINT_MAX_ENTRIES * 16u; }
void ur_host_taa_jitter(uint32_t i, float out[2]) { out[0] = (float(i) + 1.0f) / 16.0f; out[1] = -(float(i) + 1.0f) / 32.0f; }
int ur_hzb_band_pieces(uint32_t src_h, uint32_t n, uint32_t rank, uint32_t* row0, uint32_t* rows)
{
    const uint32_t pieces = (src_h + 31u) / 32u, per = (pieces + n - 1u) / n, first = rank * per < pieces ? rank * per : pieces;
    *row0 = first;
    *rows = per < pieces - first ? per : pieces - first;
    T("ur_hzb_band_pieces %u %u %u = %u %u", src_h, n, rank, *row0, *rows);
    return R("ur_hzb_band_pieces");
}
int ur_defer_hzb_tail(ur_ctx* ctx, int mode) { T("ur_defer_hzb_tail %s %d", C, mode); return R("ur_defer_hzb_tail"); }
int ur_flush(ur_ctx* ctx) { T("ur_flush %s", C); return R("ur_flush"); }
int ur_time_next_cull(ur_ctx* ctx, void* e)
{
    T("ur_time_next_cull %s %s", C, ES(e));
    g_cull_event = e;
    if (e) g_cull_carried = false;
    return R("ur_time_next_cull");
}
int ur_time_cull_carried(const ur_ctx* ctx) { T("ur_time_cull_carried %s = %d", C, g_cull_carried ? 1 : 0); return g_cull_carried ? 1 : 0; }
int ur_time_next_lighting(ur_ctx* ctx, void* a, void* b) { T("ur_time_next_lighting %s %s %s", C, ES(a), ES(b)); return R("ur_time_next_lighting"); }

int ur_cull_indirect_args_views(ur_ctx* ctx, const uint32_t* k, const ur_float4* bounds, const float* hzb, const ur_mip_desc* mips, void* args, uint32_t* stats2,
                                uint32_t* vis_idx, uint32_t* vis_count, uint32_t index_base, const ur_draw_ranges* d, const ur_cull_view* views, uint32_t view_count)
{
    std::string v;
    for (uint32_t i = 0; views && i < view_count; ++i)
        v += " view{" + std::to_string(views[i].planes[0]) + " " + P(views[i].mask) + " " + P(views[i].visible_idx) + " " + P(views[i].visible_count) + " " + ranges(views[i].draws) + "}";
    T("ur_cull_indirect_args_views %s k=%016llx dw40-45=%u,%u,%u,%u,%u,%u %s %s mip0={%u %u %u} %s %s %s %s base=%u ranges=%s views=%u%s", C,
      (unsigned long long)fnv(k, 4 * UR_CULL_CONSTANT_DWORDS), k[40], k[41], k[42], k[43], k[44], k[45], PS(bounds), PS(hzb), mips[0].offset, mips[0].width, mips[0].height,
      PS(args), PS(stats2), PS(vis_idx), PS(vis_count), index_base, ranges(d).c_str(), view_count, v.c_str());
    const int rc = R("ur_cull_indirect_args_views");
    if (rc == UR_OK && g_cull_event) g_cull_carried = true; // (the last launch of the call carries ur_time_next_cull's event)
    return rc;
}
int ur_shadow_map(ur_ctx* ctx, const float m[16], const ur_raster_draws* d, float* map, uint32_t w, uint32_t h, uint32_t* stats4)
{
    T("ur_shadow_map %s m=%016llx %s %s %u %u %s", C, HM(m), draws(d).c_str(), PS(map), w, h, PS(stats4));
    return R("ur_shadow_map");
}
int ur_depth_prepass(ur_ctx* ctx, const float v[16], const float p[16], const ur_raster_draws* d, float* depth, uint32_t w, uint32_t h, uint32_t flags, uint32_t* stats6)
{
    T("ur_depth_prepass %s v=%016llx p=%016llx %s %s %u %u flags=%u %s", C, HM(v), HM(p), draws(d).c_str(), PS(depth), w, h, flags, PS(stats6));
    return R("ur_depth_prepass");
}
int ur_gbuffer_pass_materials(ur_ctx* ctx, const float v[16], const float p[16], const ur_raster_draws* d, const float* depth, const ur_gbuffer_targets* t, uint32_t w,
                              uint32_t h, uint32_t row0, uint32_t rows, uint32_t flags, uint32_t key_bits, uint32_t* stats6, const ur_material* materials, uint32_t material_count)
{
    T("ur_gbuffer_pass_materials %s v=%016llx p=%016llx %s %s {%s %s %s %s %s %s} %u %u %u %u flags=%u bits=%u %s %s n=%u", C, HM(v), HM(p), draws(d).c_str(), PS(depth),
      PS(t->gbuf_a), PS(t->gbuf_b), PS(t->gbuf_c), PS(t->hdr), PS(t->object_id), PS(t->keys), w, h, row0, rows, flags, key_bits, PS(stats6), PS(materials), material_count);
    return R("ur_gbuffer_pass_materials");
}
int ur_build_hzb(ur_ctx* ctx, const float* depth, uint32_t sw, uint32_t sh, float* hzb, const ur_mip_desc* mips, uint32_t n)
{
    T("ur_build_hzb %s %s %u %u %s mip0={%u %u %u} n=%u", C, PS(depth), sw, sh, PS(hzb), mips[0].offset, mips[0].width, mips[0].height, n);
    return R("ur_build_hzb");
}
int ur_build_hzb_band(ur_ctx* ctx, const float* depth, uint32_t sw, uint32_t sh, float* hzb, const ur_mip_desc* mips, uint32_t n, uint32_t row0, uint32_t rows)
{
    T("ur_build_hzb_band %s %s %u %u %s mip0={%u %u %u} n=%u pieces %u %u", C, PS(depth), sw, sh, PS(hzb), mips[0].offset, mips[0].width, mips[0].height, n, row0, rows);
    return R("ur_build_hzb_band");
}
static std::string tables(const ur_lighting_tables* t)
{
    return "{" + P(t->shadow_map) + " " + P(t->env_cube) + " " + std::to_string(t->env_base_size) + " " + std::to_string(t->env_mip_count) + " " + P(t->brdf_lut_rg16) + " " +
           std::to_string(t->lut_width) + " " + std::to_string(t->lut_height) + " " + std::to_string(t->env_cube_texels) + "}";
}
int ur_deferred_lighting(ur_ctx* ctx, const ur_scene_constants* s, const ur_half4* a, const ur_half4* b, const uint32_t* c, const ur_lighting_tables* t, ur_half4* hdr, uint32_t w,
                         uint32_t h, uint32_t row0, uint32_t rows)
{
    T("ur_deferred_lighting %s scene=%016llx shadow=%.9g %s %s %s %s %s %u %u %u %u", C, H(s), s->ShadowStrength, PS(a), PS(b), PS(c), tables(t).c_str(), PS(hdr), w, h, row0, rows);
    return R("ur_deferred_lighting");
}
int ur_deferred_lighting_sky(ur_ctx* ctx, const ur_scene_constants* s, const ur_sky_constants* sky, const ur_half4* a, const ur_half4* b, const uint32_t* c, const float* depth,
                             const ur_lighting_tables* t, ur_half4* hdr, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    T("ur_deferred_lighting_sky %s scene=%016llx shadow=%.9g sky=%016llx %s %s %s %s %s %s %u %u %u %u", C, H(s), s->ShadowStrength, H(sky), PS(a), PS(b), PS(c), PS(depth),
      tables(t).c_str(), PS(hdr), w, h, row0, rows);
    return R("ur_deferred_lighting_sky");
}
int ur_sky_atmosphere(ur_ctx* ctx, const ur_sky_constants* sky, const float* depth, ur_half4* hdr, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    T("ur_sky_atmosphere %s sky=%016llx %s %s %u %u %u %u", C, H(sky), PS(depth), PS(hdr), w, h, row0, rows);
    return R("ur_sky_atmosphere");
}
int ur_pack_post_record(ur_ctx* ctx, const ur_half4* hdr, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows, void* record)
{
    T("ur_pack_post_record %s %s %u %u %u %u %s", C, PS(hdr), w, h, row0, rows, PS(record));
    return R("ur_pack_post_record");
}
int ur_pack_taa_record(ur_ctx* ctx, const ur_half4* hdr, const ur_half4* hist, uint32_t use_history, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows, void* record)
{
    T("ur_pack_taa_record %s %s %s use=%u %u %u %u %u %s", C, PS(hdr), PS(hist), use_history, w, h, row0, rows, PS(record));
    return R("ur_pack_taa_record");
}
static std::string ae(const ur_auto_exposure_constants* k)
{
    char buf[256];
    snprintf(buf, sizeof buf, "{%.9g %.9g %.9g %.9g %.9g %u %.9g %.9g %.9g}", k->InputSize[0], k->InputSize[1], k->DeltaTime, k->AdaptationSpeedUp, k->AdaptationSpeedDown,
             k->UseHistory, k->AutoExposureKey, k->AutoExposureMin, k->AutoExposureMax);
    return buf;
}
int ur_auto_exposure(ur_ctx* ctx, const ur_auto_exposure_constants* k, const ur_half4* hdr, uint32_t w, uint32_t h, const float* prev, float* out)
{
    T("ur_auto_exposure %s %s %s %u %u %s %s", C, ae(k).c_str(), PS(hdr), w, h, PS(prev), PS(out));
    return R("ur_auto_exposure");
}
int ur_auto_exposure_records(ur_ctx* ctx, const ur_auto_exposure_constants* k, const void* records, uint32_t n, uint32_t w, uint32_t h, const float* prev, float* out)
{
    T("ur_auto_exposure_records %s %s %s ranks=%u %u %u %s %s", C, ae(k).c_str(), PS(records), n, w, h, PS(prev), PS(out));
    return R("ur_auto_exposure_records");
}
int ur_temporal_aa(ur_ctx* ctx, const ur_half4* cur, const ur_half4* hist, ur_half4* out, float weight, uint32_t use, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    T("ur_temporal_aa %s %s %s %s %.9g use=%u %u %u %u %u", C, PS(cur), PS(hist), PS(out), weight, use, w, h, row0, rows);
    return R("ur_temporal_aa");
}
int ur_temporal_aa_halo(ur_ctx* ctx, const ur_half4* cur, const ur_half4* ca, const ur_half4* cb, const ur_half4* hist, ur_half4* out, const ur_half4* a2, const ur_half4* ha,
                        const ur_half4* b2, const ur_half4* hb, ur_half4* ra, ur_half4* rb, float weight, uint32_t use, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    T("ur_temporal_aa_halo %s %s %s %s %s %s %s %s %s %s %s %s %.9g use=%u %u %u %u %u", C, PS(cur), PS(ca), PS(cb), PS(hist), PS(out), PS(a2), PS(ha), PS(b2), PS(hb), PS(ra), PS(rb),
      weight, use, w, h, row0, rows);
    return R("ur_temporal_aa_halo");
}
int ur_temporal_aa_tonemap(ur_ctx* ctx, const ur_tonemap_constants* k, const ur_half4* cur, const ur_half4* hist, ur_half4* hist_out, const float* ev, uint32_t* ldr, float weight,
                           uint32_t use, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    T("ur_temporal_aa_tonemap %s %s %s %s %s %s %s %.9g use=%u %u %u %u %u", C, tonemap(k).c_str(), PS(cur), PS(hist), PS(hist_out), PS(ev), PS(ldr), weight, use, w, h, row0, rows);
    return R("ur_temporal_aa_tonemap");
}
int ur_temporal_aa_tonemap_halo(ur_ctx* ctx, const ur_tonemap_constants* k, const ur_half4* cur, const ur_half4* ca, const ur_half4* cb, const ur_half4* hist, ur_half4* hist_out,
                                const float* ev, uint32_t* ldr, const ur_half4* a2, const ur_half4* ha, const ur_half4* b2, const ur_half4* hb, ur_half4* ra, ur_half4* rb,
                                float weight, uint32_t use, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    T("ur_temporal_aa_tonemap_halo %s %s %s %s %s %s %s %s %s %s %s %s %s %s %s %.9g use=%u %u %u %u %u", C, tonemap(k).c_str(), PS(cur), PS(ca), PS(cb), PS(hist), PS(hist_out), PS(ev),
      PS(ldr), PS(a2), PS(ha), PS(b2), PS(hb), PS(ra), PS(rb), weight, use, w, h, row0, rows);
    return R("ur_temporal_aa_tonemap_halo");
}
int ur_tonemap(ur_ctx* ctx, const ur_tonemap_constants* k, const ur_half4* hdr, const float* ev, uint32_t* out, uint32_t w, uint32_t rows)
{
    T("ur_tonemap %s %s %s %s %s %u %u", C, tonemap(k).c_str(), PS(hdr), PS(ev), PS(out), w, rows);
    return R("ur_tonemap");
}
int ur_tonemap_cas(ur_ctx* ctx, const ur_tonemap_constants* k, const ur_cas_constants* c, const ur_half4* hdr, const float* ev, uint32_t* out, uint32_t w, uint32_t h, uint32_t row0,
                   uint32_t rows)
{
    T("ur_tonemap_cas %s %s %s %s %s %s %u %u %u %u", C, tonemap(k).c_str(), cas(c).c_str(), PS(hdr), PS(ev), PS(out), w, h, row0, rows);
    return R("ur_tonemap_cas");
}
int ur_tonemap_cas_halo(ur_ctx* ctx, const ur_tonemap_constants* k, const ur_cas_constants* c, const ur_half4* hdr, const ur_half4* above, const ur_half4* below, const float* ev,
                        uint32_t* out, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    T("ur_tonemap_cas_halo %s %s %s %s %s %s %s %s %u %u %u %u", C, tonemap(k).c_str(), cas(c).c_str(), PS(hdr), PS(above), PS(below), PS(ev), PS(out), w, h, row0, rows);
    return R("ur_tonemap_cas_halo");
}
int ur_cas(ur_ctx* ctx, const ur_cas_constants* c, const uint32_t* ldr, uint32_t* out, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    T("ur_cas %s %s %s %s %u %u %u %u", C, cas(c).c_str(), PS(ldr), PS(out), w, h, row0, rows);
    return R("ur_cas");
}
int ur_cas_halo(ur_ctx* ctx, const ur_tonemap_constants* k, const ur_cas_constants* c, const uint32_t* ldr, const ur_half4* above, const ur_half4* below, const float* ev,
                uint32_t* out, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    T("ur_cas_halo %s %s %s %s %s %s %s %s %u %u %u %u", C, tonemap(k).c_str(), cas(c).c_str(), PS(ldr), PS(above), PS(below), PS(ev), PS(out), w, h, row0, rows);
    return R("ur_cas_halo");
}
int ur_debug_print_reset(ur_ctx* ctx, void* buffer, uint32_t* stats) { T("ur_debug_print_reset %s %s %s", C, PS(buffer), PS(stats)); return R("ur_debug_print_reset"); }
int ur_debug_print_stats(ur_ctx* ctx, const uint32_t* stats, void* buffer) { T("ur_debug_print_stats %s %s %s", C, PS(stats), PS(buffer)); return R("ur_debug_print_stats"); }
int ur_debug_print_draw(ur_ctx* ctx, const ur_debug_print_constants* k, const ur_debug_glyph* glyphs, uint32_t glyph_count, const uint8_t* atlas, uint32_t aw, uint32_t ah,
                        const void* buffer, uint32_t* ldr, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    T("ur_debug_print_draw %s {%.9g %.9g %u %u} %s n=%u %s %u %u %s %s %u %u %u %u", C, k->ScreenSize[0], k->ScreenSize[1], k->FirstChar, k->CharCount, PS(glyphs), glyph_count,
      PS(atlas), aw, ah, PS(buffer), PS(ldr), w, h, row0, rows);
    return R("ur_debug_print_draw");
}
#undef C
} // extern "C"

// ---- the cases ------------------------------------------------------------------------------------------------------------------------------
namespace {

const struct { const char* name; uint32_t bit; } kFlags[] = {
    {"INDIRECT_DRAW", UR_FRAME_INDIRECT_DRAW}, {"HZB", UR_FRAME_HZB}, {"DEPTH_PREPASS", UR_FRAME_DEPTH_PREPASS}, {"SHADOWS", UR_FRAME_SHADOWS}, {"SKY", UR_FRAME_SKY},
    {"FUSE_LIGHTING_SKY", UR_FRAME_FUSE_LIGHTING_SKY}, {"GPU_TIMING", UR_FRAME_GPU_TIMING}, {"GRAPH_DUMP", UR_FRAME_GRAPH_DUMP}, {"BARRIER_LOGS", UR_FRAME_BARRIER_LOGS},
    {"ASYNC_COMPUTE", UR_FRAME_ASYNC_COMPUTE}, {"ASYNC_NO_JOIN", UR_FRAME_ASYNC_NO_JOIN}, {"TONEMAP", UR_FRAME_TONEMAP}, {"TIME_LIGHTING", UR_FRAME_TIME_LIGHTING},
    {"HZB_TAIL_WITH_LIGHTING", UR_FRAME_HZB_TAIL_WITH_LIGHTING}, {"TIME_LIGHTING_RECORD_COST", UR_FRAME_TIME_LIGHTING_RECORD_COST}, {"HZB_WITH_LIGHTING", UR_FRAME_HZB_WITH_LIGHTING},
    {"TIME_LIGHTING_KERNEL", UR_FRAME_TIME_LIGHTING_KERNEL}, {"HZB_SHARD", UR_FRAME_HZB_SHARD}, {"AUTO_EXPOSURE", UR_FRAME_AUTO_EXPOSURE}, {"CAS", UR_FRAME_CAS},
    {"FUSE_TONEMAP_CAS", UR_FRAME_FUSE_TONEMAP_CAS}, {"POST_EXCHANGE", UR_FRAME_POST_EXCHANGE}, {"CULL_VIEWS", UR_FRAME_CULL_VIEWS}, {"TAA", UR_FRAME_TAA},
    {"FUSE_TAA_TONEMAP", UR_FRAME_FUSE_TAA_TONEMAP}, {"TAA_BAND", UR_FRAME_TAA_BAND}, {"DEBUG_PRINT", UR_FRAME_DEBUG_PRINT}, {"SHADOW_PASS", UR_FRAME_SHADOW_PASS},
    {"DEPTH_PASS", UR_FRAME_DEPTH_PASS}, {"GBUFFER_PASS", UR_FRAME_GBUFFER_PASS}, {"DEFAULT", UR_FRAME_DEFAULT}};

uint32_t parse_flags(const std::string& s)
{
    uint32_t flags = 0;
    std::stringstream ss(s);
    std::string name;
    while (std::getline(ss, name, '+')) {
        if (name == "0") continue;
        bool found = false;
        for (const auto& f : kFlags)
            if (name == f.name) { flags |= f.bit; found = true; }
        if (!found) { fprintf(stderr, "unknown flag %s\n", name.c_str()); abort(); }
    }
    return flags;
}
std::string flag_names(uint32_t flags)
{
    std::string s;
    if ((flags & UR_FRAME_DEFAULT) == UR_FRAME_DEFAULT) { s = "DEFAULT"; flags &= ~UR_FRAME_DEFAULT; }
    for (size_t i = 0; i + 1 < sizeof kFlags / sizeof *kFlags; ++i)
        if (flags & kFlags[i].bit) s += (s.empty() ? "" : "+") + std::string(kFlags[i].name);
    return s.empty() ? "0" : s;
}

// What a case's calls work on. Every struct is zeroed, then filled with a pattern: no padding byte is left to chance.
struct Harness
{
    ur_frame* f = nullptr;
    uint32_t world = 1, rank = 0, ring = 3, w = 16, h = 8;
    ur_frame_resources res;
    uint32_t culling[UR_CULL_CONSTANT_DWORDS];
    ur_scene_constants scene;
    ur_sky_constants sky;
    ur_draw_ranges ranges, view_ranges;

    void create()
    {
        f = ur_frame_create(&g_main, B("stream_main"), ring, int(rank), int(world));
        make_resources();
    }
    void make_resources()
    {
        memset(&res, 0, sizeof res);
        res.width = w; res.height = h; res.rows = h / world; res.row0 = rank * res.rows;
        res.gbuffer_a = BT<ur_half4>("gbuffer_a"); res.gbuffer_b = BT<ur_half4>("gbuffer_b"); res.gbuffer_c = BT<uint32_t>("gbuffer_c");
        res.depth_band = BT<float>("depth_band"); res.lighting_band = BT<ur_half4>("lighting_band"); res.depth_full = BT<float>("depth_full");
        res.hzb = BT<float>("hzb");
        res.hzb_mip_count = 3;
        for (uint32_t i = 0, off = 0; i < 3; ++i) { res.hzb_mips[i] = {off, (w / 2) >> i, (h / 2) >> i}; off += res.hzb_mips[i].width * res.hzb_mips[i].height; }
        res.tables.shadow_map = BT<float>("shadow_map"); res.tables.env_cube = BT<ur_half4>("env_cube"); res.tables.env_base_size = 4; res.tables.env_mip_count = 2;
        res.tables.brdf_lut_rg16 = BT<uint16_t>("brdf_lut"); res.tables.lut_width = 128; res.tables.lut_height = 32; res.tables.env_cube_texels = 1234;
        res.model_bounds = BT<ur_float4>("model_bounds"); res.indirect_args = B("indirect_args"); res.indirect_command_count = 25; res.instance_index_base = 100;
        res.visible_indices = BT<uint32_t>("visible_indices"); res.visible_count = BT<uint32_t>("visible_count"); res.cull_stats = BT<uint32_t>("cull_stats");
        res.tonemap_band = BT<uint32_t>("tonemap_band");
        for (uint32_t i = 0; i < UR_CULL_CONSTANT_DWORDS; ++i) culling[i] = 1000u + i;
        memset(&scene, 0, sizeof scene);
        float* s = reinterpret_cast<float*>(&scene);
        for (size_t i = 0; i < sizeof scene / 4; ++i) s[i] = 0.5f + float(i);
        scene.ShadowStrength = 0.75f; scene.ShadowMapSize[0] = 32.0f; scene.ShadowMapSize[1] = 16.0f; scene.AlphaMode = 1; scene.ObjectId = 7;
        memset(&sky, 0, sizeof sky);
        s = reinterpret_cast<float*>(&sky);
        for (size_t i = 0; i < sizeof sky / 4; ++i) s[i] = 0.25f + float(i);
    }
    void destroy() { ur_frame_destroy(f); f = nullptr; }

    void after(const char* what, int rc)
    {
        T("%s = %d", what, rc);
        if (rc != UR_OK) T("error: %s", ur_last_error());
        char buf[4096];
        ur_frame_report(f, buf, sizeof buf);
        T("report:\n%shzb_ready = %d", buf, ur_frame_hzb_ready(f));
        ur_frame_taa_info info;
        const std::string keep = g_error;
        if (ur_frame_taa_next(f, &info) == UR_OK) T("taa_next = read %u write %u use %u jitter %.9g %.9g", info.read_slot, info.write_slot, info.use_history, info.jitter[0], info.jitter[1]);
        else T("taa_next = none");
        g_error = keep;
    }

    int set(const std::string& what, bool on)
    {
        if (what == "post" || what == "post_noscratch" || what == "post_nolum") {
            ur_frame_post p;
            memset(&p, 0, sizeof p);
            if (what != "post_nolum") { p.luminance[0] = BT<float>("luminance0"); p.luminance[1] = BT<float>("luminance1"); }
            if (what != "post_noscratch") p.tonemap_scratch = BT<uint32_t>("tonemap_scratch");
            p.delta_time = 0.016f; p.tonemap_exposure = 1.25f; p.tonemap_gamma = 2.4f; p.ae_key = 0.18f; p.ae_min = 0.2f; p.ae_max = 4.0f; p.ae_speed_up = 2.0f; p.ae_speed_down = 0.5f;
            p.cas_sharpness = 0.6f;
            return ur_frame_set_post(f, on ? &p : nullptr);
        }
        if (what == "taa") {
            ur_half4* images[3] = {BT<ur_half4>("taa_history0"), BT<ur_half4>("taa_history1"), BT<ur_half4>("taa_history2")};
            const ur_frame_taa t = {images, ring, 0.85f};
            return ur_frame_set_taa(f, on ? &t : nullptr);
        }
        if (what == "records") return ur_frame_set_post_records(f, on ? B("post_record") : nullptr, B("post_records"));
        if (what == "taarecords") return ur_frame_set_taa_records(f, on ? B("taa_record") : nullptr, B("taa_records"));
        if (what == "debug") {
            const ur_frame_debug_print d = {B("debug_buffer"), BT<ur_debug_glyph>("debug_glyphs"), 128, BT<uint8_t>("debug_atlas"), 64, 32, 32, 96};
            return ur_frame_set_debug_print(f, on ? &d : nullptr);
        }
        if (what == "ranges") {
            ranges = {BT<uint32_t>("range_offsets"), 2, B("range_commands"), BT<uint32_t>("range_counts")};
            return ur_frame_set_draw_ranges(f, on ? &ranges : nullptr);
        }
        if (what == "views") {
            view_ranges = {BT<uint32_t>("view_offsets"), 1, B("view_commands"), BT<uint32_t>("view_counts")};
            ur_cull_view v[2];
            memset(v, 0, sizeof v);
            v[0].planes[0] = 1.0f; v[0].mask = BT<uint32_t>("view_mask"); v[0].draws = &view_ranges;
            v[1].planes[0] = 2.0f; v[1].visible_idx = BT<uint32_t>("view_idx"); v[1].visible_count = BT<uint32_t>("view_count");
            return ur_frame_set_cull_views(f, v, on ? 2u : 0u);
        }
        // the raster passes draw from what the cull wrote: the shadow pass from view 0's ranges, the depth pass from the camera's list, GBuffer from its own commands
        if (what == "shadow" || what == "shadow_other") {
            view_ranges = {BT<uint32_t>("view_offsets"), 1, B("view_commands"), BT<uint32_t>("view_counts")};
            ur_frame_shadow_pass p;
            memset(&p, 0, sizeof p);
            p.draws.command_count = 25; p.draws.ranges = &view_ranges;
            p.shadow_map = BT<float>(what == "shadow" ? "shadow_map" : "other_shadow_map"); p.stats4 = BT<uint32_t>("shadow_stats");
            return ur_frame_set_shadow_pass(f, on ? &p : nullptr);
        }
        if (what == "depth" || what == "depth_d24" || what == "depth_other") {
            ur_frame_depth_pass p;
            memset(&p, 0, sizeof p);
            p.draws.commands = B("depth_commands"); p.draws.command_count = 25; p.draws.visible_idx = BT<uint32_t>("visible_indices"); p.draws.visible_count = BT<uint32_t>("visible_count");
            p.draws.index_base = 100;
            p.depth = BT<float>(what == "depth_other" ? "depth_band" : "depth_full"); p.stats6 = BT<uint32_t>("depth_stats"); p.flags = what == "depth_d24" ? UR_DEPTH_QUANTIZE_D24 : 0u;
            return ur_frame_set_depth_pass(f, on ? &p : nullptr);
        }
        if (what == "gbuffer" || what == "gbuffer_other") {
            ur_frame_gbuffer_pass p;
            memset(&p, 0, sizeof p);
            p.draws.commands = B("gbuffer_commands"); p.draws.command_count = 25;
            p.targets = {BT<ur_half4>("gbuffer_a"), BT<ur_half4>("gbuffer_b"), BT<uint32_t>("gbuffer_c"), BT<ur_half4>(what == "gbuffer" ? "lighting_band" : "gbuffer_a", what == "gbuffer" ? 0 : 64),
                         BT<uint32_t>("object_id"), BT<uint32_t>("gbuffer_keys")};
            p.stats6 = BT<uint32_t>("gbuffer_stats"); p.key_triangle_bits = 12;
            return ur_frame_set_gbuffer_pass(f, on ? &p : nullptr);
        }
        if (what == "materials") return ur_frame_set_gbuffer_materials(f, on ? BT<ur_material>("materials") : nullptr, 9);
        fprintf(stderr, "unknown setter %s\n", what.c_str());
        abort();
    }

    // resources of the frames that follow
    void resource(const std::string& what)
    {
        if (what == "no_tonemap") res.tonemap_band = nullptr;
        else if (what == "no_stats") res.cull_stats = nullptr;
        else if (what == "no_hzb") res.hzb_mip_count = 0;
        else if (what == "no_args") res.indirect_args = nullptr;
        else if (what == "no_commands") res.indirect_command_count = 0;
        else if (what == "no_depth_band") res.depth_band = nullptr;
        else if (what == "whole") { res.row0 = 0; res.rows = h; }
        else if (what == "one_row") { h = world; res.height = h; res.rows = 1; res.row0 = rank; }
        else if (what == "wide") res.width = 2 * w;
        else if (what == "all") make_resources();
        else { fprintf(stderr, "unknown resource change %s\n", what.c_str()); abort(); }
    }

    // One op: "render FLAGS", "finish", "set X", "clear X", "res X", "fail ENTRY N", "reset hzb|post|taa", "times", "join"
    void op(const std::string& line)
    {
        std::stringstream ss(line);
        std::string verb, a, b;
        ss >> verb >> a >> b;
        if (verb == "render") {
            T("> render %s", flag_names(parse_flags(a)).c_str());
            after("ur_frame_render", ur_frame_render(f, &res, culling, &scene, &sky, parse_flags(a)));
        } else if (verb == "render_null") { // each null argument of ur_frame_render, and a null frame everywhere it is refused
            const int rcs[] = {ur_frame_render(nullptr, &res, culling, &scene, &sky, 0), ur_frame_render(f, nullptr, culling, &scene, &sky, 0), ur_frame_render(f, &res, nullptr, &scene, &sky, 0),
                               ur_frame_render(f, &res, culling, nullptr, &sky, 0), ur_frame_render(f, &res, culling, &scene, nullptr, 0), ur_frame_finish_post(nullptr)};
            T("> render_null = %d %d %d %d %d; finish(null) = %d: %s", rcs[0], rcs[1], rcs[2], rcs[3], rcs[4], rcs[5], ur_last_error());
        } else if (verb == "finish") {
            T("> finish");
            after("ur_frame_finish_post", ur_frame_finish_post(f));
        } else if (verb == "set" || verb == "clear") {
            T("> %s %s", verb.c_str(), a.c_str());
            const int rc = set(a, verb == "set");
            T("= %d%s%s", rc, rc != UR_OK ? " error: " : "", rc != UR_OK ? ur_last_error() : "");
        } else if (verb == "res") {
            T("> res %s", a.c_str());
            resource(a);
        } else if (verb == "fail") {
            T("> fail %s %s", a.c_str(), b.c_str());
            g_fail[a] = g_calls[a] + atoi(b.c_str());
        } else if (verb == "reset") {
            T("> reset %s", a.c_str());
            if (a == "hzb") ur_frame_reset_hzb(f); else if (a == "post") ur_frame_reset_post(f); else ur_frame_reset_taa(f);
        } else if (verb == "times") {
            float ms[8], rec[8];
            const uint32_t n = ur_frame_lighting_times_ex(f, ms, rec, 8);
            std::string s;
            for (uint32_t i = 0; i < n; ++i) s += " " + std::to_string(ms[i]) + "/" + std::to_string(rec[i]);
            T("> times = %u%s", n, s.c_str());
        } else if (verb == "join") {
            T("> join");
            ur_frame_join_async(f);
        } else { fprintf(stderr, "unknown op %s\n", line.c_str()); abort(); }
    }
};

// "world=2 rank=1 ring=3 h=8; op; op; ..." -> the case's trace
std::string run_case(const std::string& spec)
{
    g_trace.clear(); g_error.clear(); g_calls.clear(); g_fail.clear(); g_events.clear(); g_mallocs.clear();
    g_malloc_next = 0; g_cull_event = nullptr; g_cull_carried = false;
    Harness hn;
    std::stringstream ss(spec);
    std::string part;
    bool first = true;
    while (std::getline(ss, part, ';')) {
        const size_t a = part.find_first_not_of(' ');
        if (a == std::string::npos) continue;
        part = part.substr(a);
        if (first) {
            first = false;
            std::stringstream head(part);
            std::string kv;
            while (head >> kv) {
                const uint32_t v = uint32_t(atoi(kv.substr(kv.find('=') + 1).c_str()));
                if (!kv.compare(0, 6, "world=")) hn.world = v; else if (!kv.compare(0, 5, "rank=")) hn.rank = v; else if (!kv.compare(0, 5, "ring=")) hn.ring = v;
                else if (!kv.compare(0, 2, "h=")) hn.h = v; else if (!kv.compare(0, 2, "w=")) hn.w = v; else { fprintf(stderr, "unknown key %s\n", kv.c_str()); abort(); }
            }
            hn.create();
            continue;
        }
        hn.op(part);
    }
    T("> destroy");
    hn.destroy();
    if (!g_mallocs.empty()) T("LEAK: %zu hipMalloc allocations outlive the frame", g_mallocs.size());
    return g_trace;
}

struct Case { const char* name; const char* spec; };
#define ALLSET "set post; set taa; set records; set taarecords; set debug; set ranges; set views; set shadow; set depth; set gbuffer; set materials; "
const char* const kAllSet = ALLSET;
const Case kCurated[] = {
    // ---- the scene passes ----
    {"default_three_frames", "world=1; render DEFAULT; render DEFAULT; reset hzb; render DEFAULT"},
    {"no_hzb_resources", "world=1; res no_hzb; render DEFAULT; render DEFAULT"},
    {"cull_off_each_way", "world=1; render HZB+DEPTH_PREPASS+SKY; res no_args; render DEFAULT; res all; res no_commands; render DEFAULT; res all; render DEFAULT"},
    {"sky_variants", "world=1; render INDIRECT_DRAW+SKY; render INDIRECT_DRAW+SKY+FUSE_LIGHTING_SKY; res no_depth_band; render DEFAULT+FUSE_LIGHTING_SKY; render INDIRECT_DRAW"},
    {"prepass_off_then_on", "world=1; render INDIRECT_DRAW+HZB+SHADOWS; render DEFAULT; render INDIRECT_DRAW+HZB; render DEFAULT"},
    {"async_compute", "world=1; render DEFAULT+ASYNC_COMPUTE; render DEFAULT+ASYNC_COMPUTE+ASYNC_NO_JOIN; join; render DEFAULT"},
    {"async_raster_passes", "world=1; " ALLSET "render DEFAULT+ASYNC_COMPUTE+CULL_VIEWS+SHADOW_PASS+DEPTH_PASS+GBUFFER_PASS; render DEFAULT+ASYNC_COMPUTE+CULL_VIEWS+SHADOW_PASS+DEPTH_PASS+GBUFFER_PASS"},
    {"raster_passes", "world=1; " ALLSET "render DEFAULT+CULL_VIEWS+SHADOW_PASS+DEPTH_PASS+GBUFFER_PASS+FUSE_LIGHTING_SKY; render INDIRECT_DRAW+HZB+SKY+SHADOW_PASS+DEPTH_PASS+GBUFFER_PASS; "
                      "clear materials; clear ranges; render DEFAULT+SHADOW_PASS+DEPTH_PASS+GBUFFER_PASS; render HZB+DEPTH_PREPASS+SHADOWS+SHADOW_PASS+DEPTH_PASS"},
    {"raster_passes_band", "world=2 rank=1; " ALLSET "render DEFAULT+SHADOW_PASS+DEPTH_PASS+GBUFFER_PASS+HZB_SHARD; render DEFAULT+SHADOW_PASS+DEPTH_PASS+GBUFFER_PASS+HZB_SHARD+HZB_WITH_LIGHTING"},
    {"setters_cleared", "world=1; " ALLSET "render DEFAULT+CULL_VIEWS+SHADOW_PASS+DEPTH_PASS+GBUFFER_PASS+TONEMAP+DEBUG_PRINT; clear views; clear ranges; clear shadow; clear gbuffer; clear debug; "
                        "render DEFAULT+CULL_VIEWS+DEPTH_PASS+TONEMAP; clear depth; render DEFAULT+CULL_VIEWS+TONEMAP; render DEFAULT+DEPTH_PASS"},
    {"hzb_shard", "world=4 rank=2 h=256; render DEFAULT+HZB_SHARD; render DEFAULT+HZB_SHARD+HZB_TAIL_WITH_LIGHTING; render DEFAULT+HZB_SHARD+ASYNC_COMPUTE"},
    {"hzb_shard_one_rank", "world=1; render DEFAULT+HZB_SHARD; render DEFAULT+HZB_SHARD"},
    {"ride_flags", "world=1; render DEFAULT+HZB_TAIL_WITH_LIGHTING; render DEFAULT+HZB_WITH_LIGHTING; render DEFAULT+HZB_WITH_LIGHTING+ASYNC_COMPUTE; fail ur_flush 1; render DEFAULT+HZB_TAIL_WITH_LIGHTING"},
    {"ride_tail_fails", "world=1; fail ur_defer_hzb_tail 2; render DEFAULT+HZB_WITH_LIGHTING; render DEFAULT"},
    {"timing_flags_with_cull", "world=1; render DEFAULT+TIME_LIGHTING; render DEFAULT+TIME_LIGHTING_RECORD_COST; render DEFAULT+TIME_LIGHTING_KERNEL; render DEFAULT+TIME_LIGHTING_KERNEL+HZB_WITH_LIGHTING; times"},
    {"timing_flags_without_cull", "world=1; res no_commands; render DEFAULT+TIME_LIGHTING; render DEFAULT+TIME_LIGHTING_RECORD_COST; render DEFAULT+TIME_LIGHTING_KERNEL+HZB_WITH_LIGHTING; "
                                  "render SKY+TIME_LIGHTING_KERNEL+HZB_WITH_LIGHTING; times"},
    {"timing_kernel_cull_fails", "world=1; render DEFAULT+TIME_LIGHTING_KERNEL+HZB_WITH_LIGHTING; fail ur_cull_indirect_args_views 1; render DEFAULT+TIME_LIGHTING_KERNEL+HZB_WITH_LIGHTING; "
                                 "render DEFAULT+TIME_LIGHTING_KERNEL+HZB_WITH_LIGHTING+ASYNC_COMPUTE; times"},
    {"timing_kernel_without_hzb", "world=1; res no_hzb; render DEFAULT+TIME_LIGHTING_KERNEL+HZB_WITH_LIGHTING; render DEFAULT+TIME_LIGHTING_KERNEL+HZB_WITH_LIGHTING; times"},
    {"graph_logs_and_timing", "world=1; render DEFAULT+GPU_TIMING+GRAPH_DUMP+BARRIER_LOGS+TONEMAP; render DEFAULT+GPU_TIMING"},
    {"scene_pass_fails", "world=1; set post; set taa; fail ur_build_hzb 1; render DEFAULT+TONEMAP+AUTO_EXPOSURE+TAA; render DEFAULT+TONEMAP+AUTO_EXPOSURE+TAA; fail ur_deferred_lighting 1; "
                         "render INDIRECT_DRAW+TONEMAP+AUTO_EXPOSURE+TAA; render DEFAULT+TONEMAP+AUTO_EXPOSURE+TAA"},
    {"every_scene_pass_fails_first_wins", "world=1; " ALLSET "fail ur_debug_print_reset 1; fail ur_cull_indirect_args_views 1; fail ur_shadow_map 1; fail ur_depth_prepass 1; fail ur_gbuffer_pass_materials 1; "
                                          "fail ur_sky_atmosphere 1; render DEFAULT+SHADOW_PASS+DEPTH_PASS+GBUFFER_PASS+TONEMAP+DEBUG_PRINT; render DEFAULT"},
    // ---- the post chain on the whole frame: the five Tonemap launches and both CAS launches are reached between here and the band cases ----
    {"tonemap_alone", "world=1; render DEFAULT+TONEMAP; res no_tonemap; render DEFAULT+TONEMAP"},
    {"auto_exposure_history", "world=1; set post; render DEFAULT+TONEMAP+AUTO_EXPOSURE; render DEFAULT+TONEMAP+AUTO_EXPOSURE; render DEFAULT+TONEMAP; render DEFAULT+TONEMAP+AUTO_EXPOSURE; "
                              "reset post; render DEFAULT+TONEMAP+AUTO_EXPOSURE"},
    {"cas_own_pass_and_fused", "world=1; set post; render DEFAULT+TONEMAP+CAS; render DEFAULT+TONEMAP+CAS+FUSE_TONEMAP_CAS; render DEFAULT+TONEMAP+AUTO_EXPOSURE+CAS; "
                               "render DEFAULT+TONEMAP+FUSE_TONEMAP_CAS"},
    {"taa_ring_of_three", "world=1 ring=3; set post; set taa; render DEFAULT+TONEMAP+TAA; render DEFAULT+TONEMAP+TAA; render DEFAULT+TONEMAP+TAA+FUSE_TAA_TONEMAP; "
                          "render DEFAULT+TONEMAP+TAA+AUTO_EXPOSURE+CAS"},
    {"taa_ring_of_one", "world=1 ring=1; set post; set taa; render DEFAULT+TONEMAP+TAA; render DEFAULT+TONEMAP+TAA+FUSE_TAA_TONEMAP; render DEFAULT+TONEMAP+TAA+CAS+FUSE_TONEMAP_CAS; "
                        "render DEFAULT+TONEMAP+TAA+FUSE_TAA_TONEMAP+CAS"},
    {"taa_dropped_and_reset", "world=1 ring=3; set taa; render DEFAULT+TONEMAP+TAA; render DEFAULT+TONEMAP; render DEFAULT+TONEMAP+TAA; render DEFAULT+TONEMAP+TAA; reset taa; render DEFAULT+TONEMAP+TAA; "
                              "clear taa; render DEFAULT+TONEMAP"},
    {"debug_print", "world=1; set post; set debug; render DEFAULT+TONEMAP+DEBUG_PRINT; render DEFAULT+TONEMAP+CAS+DEBUG_PRINT; render SKY+TONEMAP+DEBUG_PRINT+ASYNC_COMPUTE; "
                    "render DEFAULT+TONEMAP+CAS+FUSE_TONEMAP_CAS+DEBUG_PRINT+ASYNC_COMPUTE"},
    {"post_pass_fails", "world=1; set post; set taa; set debug; render DEFAULT+TONEMAP+AUTO_EXPOSURE+TAA+CAS+DEBUG_PRINT; fail ur_temporal_aa 1; fail ur_auto_exposure 1; fail ur_tonemap 1; fail ur_cas 1; "
                        "fail ur_debug_print_stats 1; render DEFAULT+TONEMAP+AUTO_EXPOSURE+TAA+CAS+DEBUG_PRINT; render DEFAULT+TONEMAP+AUTO_EXPOSURE+TAA+CAS+DEBUG_PRINT; "
                        "fail ur_debug_print_draw 1; render DEFAULT+TONEMAP+AUTO_EXPOSURE+TAA+CAS+DEBUG_PRINT"},
    // ---- the exchange without TAA_BAND: world 1, 2, 4; ranks at the top, in the middle and at the bottom ----
    {"exchange_world1", "world=1; set post; set records; render DEFAULT+TONEMAP+AUTO_EXPOSURE+CAS+POST_EXCHANGE; finish; render DEFAULT+TONEMAP+AUTO_EXPOSURE+CAS+POST_EXCHANGE; finish; "
                        "render DEFAULT+TONEMAP+CAS+FUSE_TONEMAP_CAS+POST_EXCHANGE; finish"},
    {"exchange_world2_top", "world=2 rank=0; set post; set records; render DEFAULT+TONEMAP+AUTO_EXPOSURE+CAS+POST_EXCHANGE; finish; render DEFAULT+TONEMAP+CAS+FUSE_TONEMAP_CAS+POST_EXCHANGE; finish; "
                            "render DEFAULT+TONEMAP+AUTO_EXPOSURE+POST_EXCHANGE; finish"},
    {"exchange_world2_bottom", "world=2 rank=1; set post; set records; set debug; render DEFAULT+TONEMAP+AUTO_EXPOSURE+CAS+POST_EXCHANGE+DEBUG_PRINT; finish; "
                               "render DEFAULT+TONEMAP+AUTO_EXPOSURE+CAS+FUSE_TONEMAP_CAS+POST_EXCHANGE+DEBUG_PRINT; finish; render DEFAULT+TONEMAP+CAS+POST_EXCHANGE; finish"},
    {"exchange_world4_middle", "world=4 rank=2; set post; set records; render DEFAULT+TONEMAP+AUTO_EXPOSURE+CAS+POST_EXCHANGE; finish; render DEFAULT+TONEMAP+AUTO_EXPOSURE+CAS+FUSE_TONEMAP_CAS+POST_EXCHANGE; "
                               "finish; render DEFAULT+TONEMAP+POST_EXCHANGE; render DEFAULT+TONEMAP+AUTO_EXPOSURE+POST_EXCHANGE; finish"},
    {"exchange_world4_top_bottom", "world=4 rank=0; set post; set records; render DEFAULT+TONEMAP+CAS+POST_EXCHANGE; finish; render DEFAULT+TONEMAP+AUTO_EXPOSURE+CAS+POST_EXCHANGE+ASYNC_COMPUTE; finish"},
    {"exchange_world4_bottom", "world=4 rank=3; set post; set records; render DEFAULT+TONEMAP+CAS+POST_EXCHANGE; finish; render DEFAULT+TONEMAP+AUTO_EXPOSURE+CAS+FUSE_TONEMAP_CAS+POST_EXCHANGE; finish"},
    {"exchange_finish_skipped", "world=2 rank=1; set post; set records; set taa; set taarecords; render DEFAULT+TONEMAP+AUTO_EXPOSURE+POST_EXCHANGE; finish; render DEFAULT+TONEMAP+AUTO_EXPOSURE+POST_EXCHANGE; "
                                "render DEFAULT+TONEMAP+AUTO_EXPOSURE+POST_EXCHANGE; finish; render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE; finish; render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE; "
                                "render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE; finish"},
    {"exchange_first_half_fails", "world=2 rank=0; set post; set records; set taa; set taarecords; render DEFAULT+TONEMAP+AUTO_EXPOSURE+TAA+TAA_BAND+POST_EXCHANGE; finish; fail ur_pack_post_record 1; "
                                  "render DEFAULT+TONEMAP+AUTO_EXPOSURE+TAA+TAA_BAND+POST_EXCHANGE; finish; render DEFAULT+TONEMAP+AUTO_EXPOSURE+TAA+TAA_BAND+POST_EXCHANGE; finish; "
                                  "fail ur_pack_taa_record 1; render DEFAULT+TONEMAP+AUTO_EXPOSURE+TAA+TAA_BAND+POST_EXCHANGE; fail ur_sky_atmosphere 1; render DEFAULT+TONEMAP+AUTO_EXPOSURE+POST_EXCHANGE; finish"},
    {"exchange_second_half_fails", "world=2 rank=0; set post; set records; set taa; set taarecords; set debug; render DEFAULT+TONEMAP+AUTO_EXPOSURE+CAS+TAA+TAA_BAND+POST_EXCHANGE+DEBUG_PRINT; finish; "
                                   "render DEFAULT+TONEMAP+AUTO_EXPOSURE+CAS+TAA+TAA_BAND+POST_EXCHANGE+DEBUG_PRINT; fail ur_temporal_aa_halo 1; fail ur_auto_exposure_records 1; fail ur_cas_halo 1; finish; "
                                   "render DEFAULT+TONEMAP+AUTO_EXPOSURE+CAS+TAA+TAA_BAND+POST_EXCHANGE+DEBUG_PRINT; finish; render DEFAULT+TONEMAP+AUTO_EXPOSURE+CAS+FUSE_TONEMAP_CAS+POST_EXCHANGE; "
                                   "fail ur_tonemap_cas_halo 1; finish; render DEFAULT+TONEMAP+AUTO_EXPOSURE+CAS+FUSE_TONEMAP_CAS+POST_EXCHANGE; finish"},
    // ---- the exchange with TAA_BAND ----
    {"taa_band_world1_ring3", "world=1 ring=3; set post; set records; set taa; set taarecords; render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE; finish; render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE+CAS; finish; "
                              "render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE+FUSE_TAA_TONEMAP; finish; render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE+AUTO_EXPOSURE+CAS+FUSE_TONEMAP_CAS; finish"},
    {"taa_band_world2_top_ring1", "world=2 rank=0 ring=1; set post; set records; set taa; set taarecords; render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE+CAS; finish; "
                                  "render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE+CAS; finish; render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE+FUSE_TAA_TONEMAP+CAS; finish; "
                                  "render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE+FUSE_TAA_TONEMAP; finish"},
    {"taa_band_world2_bottom_ring3", "world=2 rank=1 ring=3; set post; set records; set taa; set taarecords; set debug; render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE+AUTO_EXPOSURE+CAS+DEBUG_PRINT; finish; "
                                     "render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE+AUTO_EXPOSURE+CAS+FUSE_TONEMAP_CAS+DEBUG_PRINT; finish; render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE; finish"},
    {"taa_band_world4_middle_ring3", "world=4 rank=1 ring=3; set post; set records; set taa; set taarecords; render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE+CAS; finish; "
                                     "render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE+CAS; finish; render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE+FUSE_TAA_TONEMAP+CAS+AUTO_EXPOSURE; finish; "
                                     "render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE+CAS+FUSE_TONEMAP_CAS; finish"},
    {"taa_band_world4_top_ring1", "world=4 rank=0 ring=1; set post; set records; set taa; set taarecords; render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE+CAS; finish; "
                                  "render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE+CAS+FUSE_TAA_TONEMAP; finish; res wide; render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE+CAS; finish"},
    {"taa_band_world4_bottom_ring3", "world=4 rank=3 ring=3; set post; set records; set taa; set taarecords; render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE+CAS+AUTO_EXPOSURE; finish; "
                                     "render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE+CAS+AUTO_EXPOSURE; finish; render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE+FUSE_TAA_TONEMAP; finish"},
    // ---- every refusal, in the order ur_frame_render makes them ----
    {"refusals_post", "world=2 rank=1; render DEFAULT+AUTO_EXPOSURE; res no_tonemap; render DEFAULT+TONEMAP+CAS; res all; render DEFAULT+TONEMAP+AUTO_EXPOSURE; set post_nolum; "
                      "render DEFAULT+TONEMAP+AUTO_EXPOSURE+CAS; set post_noscratch; render DEFAULT+TONEMAP+AUTO_EXPOSURE+CAS; render DEFAULT+TONEMAP+CAS+FUSE_TONEMAP_CAS; "
                      "render DEFAULT+TONEMAP+FUSE_TONEMAP_CAS+POST_EXCHANGE; set post; render DEFAULT+TONEMAP+CAS; render DEFAULT+TONEMAP+CAS+POST_EXCHANGE; set records; res whole; "
                      "render DEFAULT+TONEMAP+CAS+POST_EXCHANGE; render DEFAULT+TONEMAP+CAS"},
    {"refusals_taa", "world=2 rank=1; set post; render DEFAULT+FUSE_TAA_TONEMAP; render DEFAULT+TAA; res no_tonemap; render DEFAULT+TONEMAP+TAA; res all; render DEFAULT+TONEMAP+TAA; set taa; "
                     "render DEFAULT+TONEMAP+TAA+FUSE_TAA_TONEMAP+FUSE_TONEMAP_CAS; render DEFAULT+TONEMAP+TAA; res whole; render DEFAULT+TONEMAP+TAA+POST_EXCHANGE; render DEFAULT+TONEMAP+TAA"},
    {"refusals_taa_band", "world=2 rank=1; set post; set taa; render DEFAULT+TONEMAP+TAA_BAND; render DEFAULT+TONEMAP+TAA+TAA_BAND; render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE; set records; "
                          "render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE; set taarecords; res whole; render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE; res one_row; "
                          "render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE; render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE+CAS"},
    {"refusals_debug_print", "world=1; res no_tonemap; render DEFAULT+TONEMAP+DEBUG_PRINT; render DEFAULT+DEBUG_PRINT; res all; res no_stats; render DEFAULT+TONEMAP+DEBUG_PRINT; res all; "
                             "render DEFAULT+TONEMAP+DEBUG_PRINT; set debug; render DEFAULT+TONEMAP+DEBUG_PRINT"},
    {"refusals_raster_passes", "world=1; render DEFAULT+SHADOW_PASS; set shadow_other; render DEFAULT+SHADOW_PASS; render INDIRECT_DRAW+SHADOW_PASS; render DEFAULT+DEPTH_PASS; set depth_other; "
                               "render DEFAULT+DEPTH_PASS; set depth; render DEFAULT+GBUFFER_PASS; render DEFAULT+DEPTH_PASS+GBUFFER_PASS; set gbuffer_other; render DEFAULT+DEPTH_PASS+GBUFFER_PASS; "
                               "set gbuffer; set depth_d24; render DEFAULT+DEPTH_PASS+GBUFFER_PASS; set depth; render DEFAULT+DEPTH_PASS+GBUFFER_PASS"},
    {"refusals_null_and_runtime", "world=2 rank=1; set post; set records; set taa; set taarecords; render_null; fail hipMalloc 1; render DEFAULT+TONEMAP+TAA+TAA_BAND+POST_EXCHANGE+CAS; "
                                  "fail hipStreamCreateWithPriority 1; render DEFAULT+ASYNC_COMPUTE; render DEFAULT+ASYNC_COMPUTE; render DEFAULT"},
    {"refusals_async_context", "world=1; fail ur_create 1; render DEFAULT+ASYNC_COMPUTE"},
    {"refusals_finish_post", "world=2 rank=1; set post; set records; finish; render DEFAULT+TONEMAP; finish; render DEFAULT+TONEMAP+CAS+POST_EXCHANGE; finish; finish"},
    // a render that fails behind its validation has overwritten the resources of the frame whose post passes are pending: the band is no longer the rank's
    {"refusals_finish_post_band", "world=2 rank=1; set post; set records; render DEFAULT+TONEMAP+CAS+POST_EXCHANGE; res whole; fail hipStreamCreateWithPriority 1; "
                                  "render DEFAULT+ASYNC_COMPUTE; finish; res all; render DEFAULT+TONEMAP+CAS+POST_EXCHANGE; finish"},
    {"refusals_setters", "world=1; fail check_cull_views 1; set views; fail check_raster_draws 1; set shadow; fail check_raster_draws 1; set depth; fail check_gbuffer_targets 1; set gbuffer; "
                         "fail check_raster_draws 1; set gbuffer; render DEFAULT+SHADOW_PASS"},
};
constexpr size_t kCuratedCount = sizeof kCurated / sizeof *kCurated;

// ---- the sweeps ---------------------------------------------------------------------------------------------------------------------------------
// Scene sweep: every combination of the scene-side flags with the post chain off, two frames each (the second with the first's HZB), on rank 1 of 2
// with every setter set. (GPU_TIMING, GRAPH_DUMP and BARRIER_LOGS change logs and timers alone: the curated list has them.)
const uint32_t kSceneBits[] = {UR_FRAME_INDIRECT_DRAW, UR_FRAME_HZB, UR_FRAME_DEPTH_PREPASS, UR_FRAME_SHADOWS, UR_FRAME_SKY, UR_FRAME_FUSE_LIGHTING_SKY, UR_FRAME_ASYNC_COMPUTE,
                               UR_FRAME_ASYNC_NO_JOIN, UR_FRAME_HZB_TAIL_WITH_LIGHTING, UR_FRAME_HZB_WITH_LIGHTING, UR_FRAME_TIME_LIGHTING, UR_FRAME_TIME_LIGHTING_RECORD_COST,
                               UR_FRAME_TIME_LIGHTING_KERNEL, UR_FRAME_HZB_SHARD, UR_FRAME_CULL_VIEWS, UR_FRAME_SHADOW_PASS, UR_FRAME_DEPTH_PASS, UR_FRAME_GBUFFER_PASS};
constexpr uint32_t kSceneCases = 1u << (sizeof kSceneBits / sizeof *kSceneBits), kSceneCell = 1024;
// Post sweep: every combination of the nine post flags over world size {1, 4} and ring {1, 3}, four frames each (finished when pending), rank 1 of 4.
const uint32_t kPostBits[] = {UR_FRAME_TONEMAP, UR_FRAME_AUTO_EXPOSURE, UR_FRAME_CAS, UR_FRAME_FUSE_TONEMAP_CAS, UR_FRAME_POST_EXCHANGE, UR_FRAME_TAA, UR_FRAME_FUSE_TAA_TONEMAP,
                              UR_FRAME_TAA_BAND, UR_FRAME_DEBUG_PRINT};
constexpr uint32_t kPostCases = 512u * 4u, kPostCell = 16;

std::string scene_spec(uint32_t i)
{
    uint32_t flags = 0;
    for (size_t b = 0; b < sizeof kSceneBits / sizeof *kSceneBits; ++b)
        if (i >> b & 1u) flags |= kSceneBits[b];
    const std::string r = "render " + flag_names(flags);
    return std::string("world=2 rank=1; ") + kAllSet + r + "; " + r;
}
std::string post_spec(uint32_t bits, uint32_t world, uint32_t ring)
{
    uint32_t flags = UR_FRAME_DEFAULT;
    for (size_t b = 0; b < sizeof kPostBits / sizeof *kPostBits; ++b)
        if (bits >> b & 1u) flags |= kPostBits[b];
    const std::string r = "render " + flag_names(flags) + "; finish";
    return "world=" + std::to_string(world) + " rank=" + std::to_string(world == 4 ? 1 : 0) + " ring=" + std::to_string(ring) + "; " + kAllSet + r + "; " + r + "; " + r + "; " + r;
}
std::string post_spec(uint32_t i) { return post_spec(i & 511u, (i >> 9 & 1u) ? 4u : 1u, (i >> 10 & 1u) ? 3u : 1u); }

// What a case's golden shows of its trace: one line per op that calls or refuses something, with the entry points called in order (less their ur_; @async on that lane, ! failed on request),
// the result, the report, hzb_ready and taa_next. The arguments are held by the digest of the full trace in the case's header; --case prints them.
std::string brief(const std::string& trace)
{
    std::stringstream in(trace);
    std::string line, out, calls, report, all, last_calls, last_report, tail;
    int logs = 0;
    bool in_report = false;
    const auto flush = [&] {
        // (an op that called nothing and refused nothing is in the case's header already)
        if (out.empty() || (calls.empty() && report.empty() && tail.empty() && out.find(" = -") == std::string::npos && out.find("times") != 0)) { out.clear(); return; }
        // "=": as on the line before (finish: the first half's passes). [scene]: the four calls / passes of a default scene. Every render ends
        // with time_next_cull(null): not shown.
        const std::string kSceneCalls = " cull_indirect_args_views build_hzb deferred_lighting sky_atmosphere", kScenePasses = "GPU Culling, Build HZB, Lighting, Sky";
        const std::string kEnd = " time_next_cull";
        if (calls.size() >= kEnd.size() && !calls.compare(calls.size() - kEnd.size(), kEnd.size(), kEnd)) calls.resize(calls.size() - kEnd.size());
        std::string c = calls, r = report;
        if (!c.empty() && c == last_calls) c = " =";
        else if (c.find(kSceneCalls) != std::string::npos) c.replace(c.find(kSceneCalls), kSceneCalls.size(), " [scene]");
        if (!r.empty() && r == last_report) r = "=";
        else if (!last_report.empty() && !r.compare(0, last_report.size() + 2, last_report + ", ")) r = "=, " + r.substr(last_report.size() + 2);
        else if (!r.compare(0, kScenePasses.size(), kScenePasses)) r.replace(0, kScenePasses.size(), "[scene]");
        if (!c.empty()) out += " | calls:" + c;
        if (!r.empty()) out += " | passes: " + r;
        out += tail;
        tail.clear();
        last_calls = calls; last_report = report;
        if (logs) out += " | " + std::to_string(logs) + " log lines";
        all += out + "\n";
        out.clear(); calls.clear(); report.clear(); logs = 0;
    };
    while (std::getline(in, line)) {
        if (!line.compare(0, 2, "> ")) { flush(); out = line.substr(2); in_report = false; }
        else if (!line.compare(0, 11, "hzb_ready =")) { in_report = false; tail += " | hzb " + line.substr(12); }
        else if (in_report) { // "name|culled|transitions|async|waits": the name, -culled, @async; the counts are in the digest
            std::stringstream f(line);
            std::string name, culled, transitions, async;
            std::getline(f, name, '|'); std::getline(f, culled, '|'); std::getline(f, transitions, '|'); std::getline(f, async, '|');
            report += (report.empty() ? "" : ", ") + name + (culled == "1" ? "-culled" : "") + (async == "1" ? "@async" : "");
        }
        else if (line == "report:") in_report = true;
        else if (!line.compare(0, 10, "taa_next =")) tail += line == "taa_next = none" ? "" : " | taa" + line.substr(10);
        else if (!line.compare(0, 5, "log: ")) ++logs;
        else if (!line.compare(0, 2, "= ") || !line.compare(0, 7, "error: ") || !line.compare(0, 6, "LEAK: ")) out += " " + line;
        else if (!line.compare(0, 9, "ur_frame_")) out += line.substr(line.find(" = "));
        else {
            std::stringstream words(line);
            std::string name, ctx;
            words >> name >> ctx;
            calls += " " + (name.compare(0, 3, "ur_") ? name : name.substr(3)) + (ctx == "async" ? "@async" : "") + (line.find(" -> ") != std::string::npos ? "!" : "");
        }
    }
    flush();
    return all;
}

std::string curated_entry(const Case& c)
{
    const std::string trace = run_case(c.spec);
    char digest[32];
    snprintf(digest, sizeof digest, "%016llx", (unsigned long long)fnv(trace.data(), trace.size()));
    return std::string("==== ") + c.name + " " + digest + "\n" + brief(trace); // (the case's ops are in kCurated)
}

// cell -> digest of the traces of its cases, in order
std::string cell_digest(bool scene, uint32_t cell)
{
    const uint32_t n = scene ? kSceneCell : kPostCell;
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint32_t i = cell * n; i < (cell + 1) * n; ++i) { const std::string t = run_case(scene ? scene_spec(i) : post_spec(i)); h = fnv(t.data(), t.size(), h); }
    char buf[64];
    snprintf(buf, sizeof buf, "%s %u %016llx\n", scene ? "scene" : "post", cell, (unsigned long long)h);
    return buf;
}

std::string read_file(const char* path)
{
    std::ifstream in(path, std::ios::binary);
    if (!in) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    std::stringstream s;
    s << in.rdbuf();
    return s.str();
}

} // namespace

int main(int argc, char** argv)
{
    FRenderGraph::SetLogSink([](const std::string& line) { T("log: %s", line.c_str()); });
    const std::string mode = argc > 1 ? argv[1] : "";
    const uint32_t scene_cells = kSceneCases / kSceneCell, cells = scene_cells + kPostCases / kPostCell;
    if (mode == "--record") {
        for (const Case& c : kCurated) fputs(curated_entry(c).c_str(), stdout);
        for (uint32_t i = 0; i < cells; ++i) fputs(cell_digest(i < scene_cells, i < scene_cells ? i : i - scene_cells).c_str(), stdout);
        return 0;
    }
    if (mode == "--case" && argc > 2) {
        const std::string name = argv[2];
        std::string spec;
        for (const Case& c : kCurated) if (name == c.name) spec = c.spec;
        unsigned a = 0, b = 0, c = 0;
        if (sscanf(name.c_str(), "scene:%u", &a) == 1) spec = scene_spec(a);
        if (sscanf(name.c_str(), "post:%u:%u:%u", &a, &b, &c) == 3) spec = post_spec(a, b, c);
        if (spec.empty()) { fprintf(stderr, "no case %s\n", name.c_str()); return 2; }
        printf("==== %s: %s\n%s", name.c_str(), spec.c_str(), run_case(spec).c_str());
        return 0;
    }
    if ((mode == "--check" || mode == "--check-curated") && argc > 2) { // (--check-curated: without the sweeps, what the sanitizer build runs)
        const std::string want = read_file(argv[2]);
        size_t at = 0;
        for (const Case& c : kCurated) {
            const std::string got = curated_entry(c);
            if (want.compare(at, got.size(), got) != 0) {
                printf("MISMATCH in curated case %s: now\n%sits trace in full:\n%s", c.name, got.c_str(), run_case(c.spec).c_str());
                return 1;
            }
            at += got.size();
        }
        if (mode == "--check-curated") { printf("OK frame trace: %zu curated cases\n", kCuratedCount); return 0; }
        for (uint32_t i = 0; i < cells; ++i) {
            const bool scene = i < scene_cells;
            const uint32_t cell = scene ? i : i - scene_cells, n = scene ? kSceneCell : kPostCell;
            const std::string got = cell_digest(scene, cell);
            if (want.compare(at, got.size(), got) != 0) {
                // the cell's digest chains its cases: the first case in full, --case prints any other
                printf("MISMATCH in %s cell %u, now %scases %u .. %u of that sweep (%s); the first one's trace:\n%s", scene ? "scene" : "post", cell, got.c_str(), cell * n,
                       cell * n + n - 1, scene ? "--case scene:<i>" : "--case post:<i & 511>:<world>:<ring>, world 4 from 512 on, ring 3 from 1024 on",
                       run_case(scene ? scene_spec(cell * n) : post_spec(cell * n)).c_str());
                return 1;
            }
            at += got.size();
        }
        if (at != want.size()) { puts("MISMATCH: the golden holds more than the cases"); return 1; }
        printf("OK frame trace: %zu curated cases, %u scene and %u post cases\n", kCuratedCount, kSceneCases, kPostCases);
        return 0;
    }
    fprintf(stderr, "usage: frame_trace --record | --check GOLDEN | --check-curated GOLDEN | --case NAME\n");
    return 2;
}
