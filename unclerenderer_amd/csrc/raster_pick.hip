// The ObjectId pick for gfx950 (restated in tests/object_id_ref.py): the keyed raster's answer at up to 64 given
// texels, from the triangles alone. pick_kernel runs the raster's walk and per-triangle front half (csrc/raster_front.h) and tests the points
// against each surviving triangle instead of serving its fragments; a word per point takes (key << 32) | depth bits, and a one-wave finish
// turns the words into records. Built with -ffp-contract=off.

#include "raster_front.h"
#include "raster_policies.h"
#include "visibility_key.h"

namespace {

// Rules 4-5 and the depth test of the raster's fragment for one triangle at one point, whose depth rides in `point_depth`: a passing
// fragment raises the point's word to (key << 32) | depth bits, so the greatest key wins and carries its own depth
template <class P>
__device__ __forceinline__ void pick_fragment(const Tri& t, int b01, int b12, int b20, int px, int py, float point_depth, uint32_t key,
                                              unsigned long long* __restrict__ word_at)
{
    float z;
    if (!covered_depth<P>(t, b01, b12, b20, px, py, z)) return;
    if (!(z >= point_depth)) return;
    const unsigned long long word = ((unsigned long long)key << 32) | (__float_as_uint(z) & 0x7FFFFFFFu); // z += 0.0f
    if (word <= __hip_atomic_load(word_at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return; // (words only increase)
    (void)__hip_atomic_fetch_max(word_at, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The raster's walk; behind the shared front half a surviving lane tests the points against its triangle's box - not clamped: a point
// lies inside the target - instead of serving fragments. Lane j of every wave holds point j's depth
template <class P>
__global__ __launch_bounds__(kThreads) void pick_kernel(PickParams p)
{
    const uint32_t lane = threadIdx.x & 63u;
    float point_depth = 0.0f;
    if (lane < p.point_count) {
        const uint32_t xy = p.points[lane];
        point_depth = p.depth[(size_t)(xy >> 16) * p.w + (xy & 0xFFFFu)];
    }
    WaveCounts n;
    walk_draws<P>(p, lane, n, [&](uint32_t cand, uint32_t t, const Draw& d) __attribute__((always_inline)) {
        const uint32_t key = ((cand + 1u) << p.key_bits) | t;
        LaneVerts verts;
        const uint32_t passes = lane_triangle<P>(p, d, t, verts, n);
        for (uint32_t e = 0u; e < passes; ++e) {
            Tri tri = {};
            int bx0 = 0, by0 = 0, bx1 = -1, by1 = -1;
            const bool drawn = snap_triangle<P>(verts, e, tri, n);
            if (drawn) centre_box(tri, bx0, by0, bx1, by1);
            if (__ballot(drawn && bx0 <= bx1 && by0 <= by1) == 0ull) continue;
            // ---- the points against the lane's triangle: a uniform loop, the point and its depth in scalar registers
            const int b01 = edge_bias(tri.x0, tri.y0, tri.x1, tri.y1), b12 = edge_bias(tri.x1, tri.y1, tri.x2, tri.y2), b20 = edge_bias(tri.x2, tri.y2, tri.x0, tri.y0);
            for (uint32_t j = 0u; j < p.point_count; ++j) {
                const uint32_t xy = p.points[j];
                const int px = (int)(xy & 0xFFFFu), py = (int)(xy >> 16);
                const float depth = rlf(point_depth, j);
                if (drawn && px >= bx0 && px <= bx1 && py >= by0 && py <= by1) pick_fragment<P>(tri, b01, b12, b20, px, py, depth, key, p.results + 2u * j);
            }
        }
    });
    flush_counts<P>(p.stats, lane, n);
}

// One wave behind pick_kernel: lane i turns record i's word into {ObjectId, key, slot, depth bits}; a word of 0 is {0, 0, ~0, 0}
__global__ __launch_bounds__(64) void pick_finish_kernel(PickParams p)
{
    const uint32_t i = threadIdx.x;
    if (i >= p.point_count) return;
    const unsigned long long word = p.results[2u * i];
    const uint32_t key = (uint32_t)(word >> 32), zbits = (uint32_t)word;
    u32x4_t record = {0u, 0u, 0xFFFFFFFFu, 0u};
    if (key != 0u) {
        uint32_t t;
        const uint32_t slot = key_slot<false>(p, key, 0u, t);
        const u32x4_t c2 = reinterpret_cast<const u32x4_t*>(p.commands + (size_t)slot * UR_INDIRECT_COMMAND_STRIDE)[2];
        const uint32_t* cb = reinterpret_cast<const uint32_t*>((uint64_t)c2.x | ((uint64_t)c2.y << 32));
        record = u32x4_t{cb[148], key, slot, zbits};
    }
    reinterpret_cast<u32x4_t*>(p.results)[i] = record;
}

} // namespace

int ur::launch_object_id_pick(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, const float* depth, uint32_t w, uint32_t h,
                              uint32_t key_bits, bool d24, const uint32_t* points, uint32_t point_count, ur_pick_result* results, uint32_t* stats)
{
    static_assert(sizeof(ur_pick_result) == 16, "a pick record is 16 bytes");
    UR_HIP_TRY(hipMemsetAsync(results, 0, (size_t)point_count * sizeof(ur_pick_result), ctx->stream));
    PickParams p{};
    p.point_count = point_count;
    for (uint32_t i = 0; i < point_count; ++i) p.points[i] = points[i];
    p.results = reinterpret_cast<unsigned long long*>(results);
    if (draws->command_count != 0u) {
        const VisArgs vis{depth, 0u, h, key_bits};
        const uint32_t blocks = fill_raster_params(p, ctx, view, projection, draws, w, h, stats, &vis);
        if (d24) hipLaunchKernelGGL(pick_kernel<VisPolicy<true>>, dim3(blocks), dim3(kThreads), 0, ctx->stream, p);
        else hipLaunchKernelGGL(pick_kernel<VisPolicy<false>>, dim3(blocks), dim3(kThreads), 0, ctx->stream, p);
        UR_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(pick_finish_kernel, dim3(1), dim3(64), 0, ctx->stream, p); // (every word is 0 without commands)
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}
