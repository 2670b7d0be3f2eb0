// The kernels of the raster passes for gfx950 and their launches — what turns draws of indexed triangle lists (include/ur_raster.h) into
// depth or visibility keys: one set of kernels, a policy per pass (csrc/raster_policies.h), instantiated by csrc/raster.hip (ShadowMap,
// DepthPrepass, GBuffer's keys) and csrc/raster_mask.hip (GBuffer's alpha-masked draws).
//
// Three launches, nothing read back:
//   clear   every texel = 1.0f (16-byte nontemporal stores), the large queue's count = 0;
//   raster  a wave per (draw candidate, segment): it walks the 64-triangle chunks c = segment, segment + S, ... of its command, a lane
//           per triangle (rules 1-3: csrc/raster_front.h) and the bounding box, then serves the survivors: a triangle of at most 4 centres
//           by its own lane, the others by the whole wave as an 8 x 8 pixel stamp, the triangle broadcast by readlane. Triangles of more
//           than 64 stamps go to the queue, one (triangle, 64 x 64 tile) entry per tile under the bounding box, one atomic reservation per
//           triangle; without room the wave rasterises the triangle itself (stats[3]);
//   large   a fixed grid whose waves stride over the entries: a tile the triangle cannot touch is rejected at its corners, the rest
//           is stamped.
// A fragment is one device-scope atomic unsigned minimum of the depth's bit pattern (depths lie in [0, 1]); a plain load in front
// skips it when the texel is already nearer (texels only decrease, so a stale value only costs an atomic, never a fragment).
#pragma once

#include "raster_front.h"
#include "raster_policies.h"
#include "visibility_key.h"

namespace {

typedef float f32x4_t __attribute__((ext_vector_type(4)));

// The masked policy's alpha test (csrc/raster_mask.hip); no other policy calls it
template <class P>
__device__ __forceinline__ bool alpha_discards(const AlphaCtx& a, uint32_t key, int px, int py);

// Rules 4-6 for one pixel
template <class P>
__device__ __forceinline__ void shade(const Tri& t, int b01, int b12, int b20, uint32_t* __restrict__ map, uint32_t w, int px, int py,
                                      const float* __restrict__ depth, uint32_t row0, uint32_t key, const typename P::Alpha& alpha)
{
    float z;
    if (!covered_depth<P>(t, b01, b12, b20, px, py, z)) return;
    if constexpr (P::kKeyed) {
        if (!(z >= depth[(size_t)py * w + (uint32_t)px])) return; // the value ur_depth_prepass stores, under GREATER_EQUAL against the prepass' maximum
        if constexpr (P::kMasked) {
            // section 3.11: the word's order is (depth, key); the alpha test runs only for a fragment that would raise the texel
            unsigned long long* k64 = reinterpret_cast<unsigned long long*>(map) + (size_t)((uint32_t)py - row0) * w + (uint32_t)px;
            const unsigned long long word = ((unsigned long long)(__float_as_uint(z) & 0x7FFFFFFFu) << 32) | key; // z += 0.0f
            if (word <= __hip_atomic_load(k64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return; // (words only increase)
            if (alpha_discards<P>(alpha, key, px, py)) return;
            (void)__hip_atomic_fetch_max(k64, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        uint32_t* k = map + (size_t)((uint32_t)py - row0) * w + (uint32_t)px;
        if (key <= __hip_atomic_load(k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return; // (keys only increase)
        (void)__hip_atomic_fetch_max(k, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    uint32_t* p = map + (size_t)py * w + (uint32_t)px;
    if constexpr (P::kNearest) {
        if (!(z >= 0.0f && z <= 1.0f)) return; // depth clip (a NaN goes too)
        uint32_t bits = __float_as_uint(z);
        if (bits == 0x80000000u) bits = 0u; // z += 0.0f
        if (bits >= __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return;
        (void)__hip_atomic_fetch_min(p, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        const uint32_t bits = __float_as_uint(z) & 0x7FFFFFFFu; // z += 0.0f
        if (bits <= __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return; // (texels only increase)
        (void)__hip_atomic_fetch_max(p, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The whole wave stamps the pixels [px0, px1] x [py0, py1] (inside the target) of one triangle, uniform arguments
template <class P>
__device__ __forceinline__ void stamp_rect(const Tri& t, uint32_t* __restrict__ map, uint32_t w, int px0, int py0, int px1, int py1, uint32_t lane,
                                           const float* __restrict__ depth, uint32_t row0, uint32_t key, const typename P::Alpha& alpha)
{
    const int b01 = edge_bias(t.x0, t.y0, t.x1, t.y1), b12 = edge_bias(t.x1, t.y1, t.x2, t.y2), b20 = edge_bias(t.x2, t.y2, t.x0, t.y0);
    const int lx = (int)(lane & 7u), ly = (int)(lane >> 3);
    for (int sy = py0 & ~7; sy <= py1; sy += 8) {
        const int py = sy + ly;
        for (int sx = px0 & ~7; sx <= px1; sx += 8) {
            const int px = sx + lx;
            if (px >= px0 && px <= px1 && py >= py0 && py <= py1) shade<P>(t, b01, b12, b20, map, w, px, py, depth, row0, key, alpha);
        }
    }
}

__device__ __forceinline__ Tri broadcast(const Tri& t, uint32_t s)
{
    Tri r;
    r.x0 = rl(t.x0, s); r.y0 = rl(t.y0, s); r.x1 = rl(t.x1, s); r.y1 = rl(t.y1, s); r.x2 = rl(t.x2, s); r.y2 = rl(t.y2, s);
    r.z0 = rlf(t.z0, s); r.k1 = rlf(t.k1, s); r.k2 = rlf(t.k2, s);
    return r;
}

__global__ __launch_bounds__(kThreads) void shadow_clear_kernel(float* __restrict__ map, uint32_t n, uint32_t head, uint32_t* __restrict__ queue, float value)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i == 0u && queue != nullptr) queue[0] = queue[1] = 0u; // (a 64-bit count: it never wraps)
    // `head` floats up to the first 16-byte boundary, then whole 16-byte groups, then what is left
    const uint32_t groups = (n - head) / 4u, tail = head + groups * 4u;
    if (i < head) map[i] = value;
    if (i < n - tail) map[tail + i] = value;
    f32x4_t* body = reinterpret_cast<f32x4_t*>(map + head);
    const f32x4_t fill = {value, value, value, value};
    for (uint32_t g = i; g < groups; g += gridDim.x * kThreads) __builtin_nontemporal_store(fill, body + g);
}

template <class P>
__global__ __launch_bounds__(kThreads) void raster_kernel(typename P::Params p)
{
    typename P::Alpha alpha{};
    if constexpr (P::kMasked) {
        __shared__ float sampler_tables[kLdsFloats];
        fill_sampler_tables<false>(sampler_tables, nullptr, p.mask.lod);
        __syncthreads();
        alpha.p = &p; alpha.lds = sampler_tables;
    }
    const uint32_t lane = threadIdx.x & 63u;
    WaveCounts n;
    walk_draws<P>(p, lane, n, [&](uint32_t cand, uint32_t t, const Draw& d) __attribute__((always_inline)) {
        const uint32_t key = P::kKeyed ? (((cand + 1u) << p.key_bits) | t) : 0u;
        LaneVerts verts;
        const uint32_t passes = lane_triangle<P>(p, d, t, verts, n);
        for (uint32_t e = 0u; e < passes; ++e) {
            // ---- emitted triangle e of the lane and the box of its centres, clamped to the target
            Tri tri = {};
            int bx0 = 0, by0 = 0, bx1 = -1, by1 = -1;
            uint32_t kind = 0u; // 0 nothing to draw, 1 own lane, 2 wave, 3 large
            if (snap_triangle<P>(verts, e, tri, n)) {
                centre_box(tri, bx0, by0, bx1, by1);
                bx0 = max(bx0, 0); bx1 = min(bx1, (int)p.w - 1);
                by0 = max(by0, 0); by1 = min(by1, (int)p.h - 1);
                if constexpr (P::kKeyed) { by0 = max(by0, (int)p.row0); by1 = min(by1, (int)(p.row0 + p.rows) - 1); } // the band scissor
                if (bx0 <= bx1 && by0 <= by1) { // (else no centre under the box)
                    const uint32_t pixels = (uint32_t)(bx1 - bx0 + 1) * (uint32_t)(by1 - by0 + 1);
                    const uint32_t stamps = (uint32_t)((bx1 >> 3) - (bx0 >> 3) + 1) * (uint32_t)((by1 >> 3) - (by0 >> 3) + 1);
                    kind = pixels <= kOwnPixels ? 1u : (stamps <= kLargeStamps ? 2u : 3u);
                }
            }

            // ---- the smallest by their own lanes
            if (kind == 1u) {
                const int b01 = edge_bias(tri.x0, tri.y0, tri.x1, tri.y1), b12 = edge_bias(tri.x1, tri.y1, tri.x2, tri.y2), b20 = edge_bias(tri.x2, tri.y2, tri.x0, tri.y0);
                for (int py = by0; py <= by1; ++py)
                    for (int px = bx0; px <= bx1; ++px) shade<P>(tri, b01, b12, b20, p.map, p.w, px, py, p.depth, p.row0, key, alpha);
            }
            // ---- the middle ones by the wave
            unsigned long long todo = __ballot(kind == 2u);
            while (todo != 0ull) {
                const uint32_t s = (uint32_t)__ffsll((long long)todo) - 1u;
                todo &= todo - 1ull;
                const Tri u = broadcast(tri, s);
                stamp_rect<P>(u, p.map, p.w, rl(bx0, s), rl(by0, s), rl(bx1, s), rl(by1, s), lane, p.depth, p.row0, (uint32_t)rl((int)key, s), alpha);
            }
            // ---- the large ones to the queue, or by the wave when there is no room
            todo = __ballot(kind == 3u);
            while (todo != 0ull) {
                const uint32_t s = (uint32_t)__ffsll((long long)todo) - 1u;
                todo &= todo - 1ull;
                const Tri u = broadcast(tri, s);
                const int x0 = rl(bx0, s), y0 = rl(by0, s), x1 = rl(bx1, s), y1 = rl(by1, s);
                const uint32_t ukey = (uint32_t)rl((int)key, s);
                const uint32_t tx0 = (uint32_t)x0 >> 6, ty0 = (uint32_t)y0 >> 6, tnx = ((uint32_t)x1 >> 6) - tx0 + 1u, tny = ((uint32_t)y1 >> 6) - ty0 + 1u;
                const uint32_t tiles = tnx * tny;
                bool queued = false;
                if (p.queue_cap != 0u) {
                    unsigned long long at = 0ull;
                    if (lane == 0u) at = __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(p.queue), (unsigned long long)tiles, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    at = ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(at >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)at);
                    queued = at + tiles <= p.queue_cap;
                    // the slots this reservation took and cannot use are marked empty
                    const uint32_t base = (uint32_t)min(at, (unsigned long long)p.queue_cap), end = (uint32_t)min(at + tiles, (unsigned long long)p.queue_cap);
                    for (uint32_t q_at = base + lane; q_at < end; q_at += 64u) {
                        const uint32_t k = q_at - base, tx = tx0 + k % tnx, ty = ty0 + k / tnx;
                        u32x4_t* q = reinterpret_cast<u32x4_t*>(p.queue + kQueueHeaderDwords + (size_t)q_at * P::kEntryDwords);
                        const u32x4_t q0 = {(uint32_t)u.x0, (uint32_t)u.y0, (uint32_t)u.x1, (uint32_t)u.y1};
                        const u32x4_t q1 = {(uint32_t)u.x2, (uint32_t)u.y2, __float_as_uint(u.z0), __float_as_uint(u.k1)};
                        const u32x4_t q2 = {__float_as_uint(u.k2), queued ? (tx | (ty << 16)) : kNoTile, (uint32_t)x0 | ((uint32_t)y0 << 16), (uint32_t)x1 | ((uint32_t)y1 << 16)};
                        q[0] = q0; q[1] = q1; q[2] = q2;
                        if constexpr (P::kKeyed) q[3] = u32x4_t{ukey, 0u, 0u, 0u};
                    }
                }
                if (!queued) {
                    ++n.unqueued;
                    stamp_rect<P>(u, p.map, p.w, x0, y0, x1, y1, lane, p.depth, p.row0, ukey, alpha);
                }
            }
        }
    });
    flush_counts<P>(p.stats, lane, n);
}

// The largest value of the edge function a->b over the centres of the pixels [px0, px1] x [py0, py1]: below zero, no centre passes
__device__ __forceinline__ long long edge_max(int ax, int ay, int bx, int by, int px0, int py0, int px1, int py1)
{
    const int dx = bx - ax, dy = by - ay;
    const int sy = 256 * (dx > 0 ? py1 : py0) + 128, sx = 256 * (dy > 0 ? px0 : px1) + 128;
    return (long long)dx * (sy - ay) - (long long)dy * (sx - ax);
}

template <class P>
__device__ __forceinline__ void large_body(const uint32_t* __restrict__ queue, uint32_t queue_cap, uint32_t* __restrict__ map, uint32_t w,
                                           const float* __restrict__ depth, uint32_t row0, const typename P::Alpha& alpha)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
    const uint32_t wave_count = gridDim.x * kWaves;
    const uint32_t count = (uint32_t)min(*reinterpret_cast<const unsigned long long*>(queue), (unsigned long long)queue_cap);
    for (uint32_t e = wave; e < count; e += wave_count) {
        const u32x4_t* q = reinterpret_cast<const u32x4_t*>(queue + kQueueHeaderDwords + (size_t)e * P::kEntryDwords);
        const u32x4_t q0 = q[0], q1 = q[1], q2 = q[2];
        uint32_t key = 0u;
        if constexpr (P::kKeyed) key = q[3].x;
        if (q2.y == kNoTile) continue;
        Tri t;
        t.x0 = (int)q0.x; t.y0 = (int)q0.y; t.x1 = (int)q0.z; t.y1 = (int)q0.w; t.x2 = (int)q1.x; t.y2 = (int)q1.y;
        t.z0 = __uint_as_float(q1.z); t.k1 = __uint_as_float(q1.w); t.k2 = __uint_as_float(q2.x);
        const int tx = (int)(q2.y & 0xFFFFu) * 64, ty = (int)(q2.y >> 16) * 64;
        const int px0 = max((int)(q2.z & 0xFFFFu), tx), py0 = max((int)(q2.z >> 16), ty);
        const int px1 = min((int)(q2.w & 0xFFFFu), tx + 63), py1 = min((int)(q2.w >> 16), ty + 63);
        if (edge_max(t.x0, t.y0, t.x1, t.y1, px0, py0, px1, py1) < 0 || edge_max(t.x1, t.y1, t.x2, t.y2, px0, py0, px1, py1) < 0 ||
            edge_max(t.x2, t.y2, t.x0, t.y0, px0, py0, px1, py1) < 0)
            continue;
        stamp_rect<P>(t, map, w, px0, py0, px1, py1, lane, depth, row0, key, alpha);
    }
}

template <class P>
__global__ __launch_bounds__(kThreads) void large_kernel(const uint32_t* __restrict__ queue, uint32_t queue_cap, uint32_t* __restrict__ map, uint32_t w,
                                                         const float* __restrict__ depth, uint32_t row0)
{
    large_body<P>(queue, queue_cap, map, w, depth, row0, NoAlpha{});
}

// The masked policy's (csrc/raster_mask.hip): what the alpha test reads rides in the parameters, its tables in LDS
template <class P>
__global__ __launch_bounds__(kThreads) void large_masked_kernel(MaskedParams p);

// clear, raster, large: the launches every pass shares. `map` holds n = w * (rows of the map) dwords: the whole target of a depth pass
// (vis null), GBuffer's key image of its band. m1 is null for ShadowMap.
template <class P>
int launch_raster(ur_ctx* ctx, const float* m0, const float* m1, const ur_raster_draws* draws, uint32_t* map, uint32_t n, uint32_t w, uint32_t h, float clear,
                  uint32_t* stats, const VisArgs* vis, const MaskArgs* mask = nullptr)
{
    const uint32_t head = min((uint32_t)((16u - (reinterpret_cast<uintptr_t>(map) & 15u)) & 15u) / 4u, n);
    uint32_t* queue = ctx->raster_queue_cap != 0u ? ctx->raster_queue : nullptr;
    const uint32_t clear_blocks = min((n / 4u + kThreads - 1u) / kThreads + 1u, (uint32_t)ctx->cu_count * 16u);
    hipLaunchKernelGGL(shadow_clear_kernel, dim3(clear_blocks), dim3(kThreads), 0, ctx->stream, reinterpret_cast<float*>(map), n, head, queue, clear);
    UR_HIP_TRY(hipGetLastError());
    if (draws->command_count == 0u) return UR_OK;

    typename P::Params p{};
    if constexpr (P::kMasked) p.mask = *mask;
    p.map = map;
    p.queue = queue; p.queue_cap = queue ? ctx->raster_queue_cap : 0u;
    const uint32_t blocks = fill_raster_params(p, ctx, m0, m1, draws, w, h, stats, vis);
    hipLaunchKernelGGL(raster_kernel<P>, dim3(blocks), dim3(kThreads), 0, ctx->stream, p);
    UR_HIP_TRY(hipGetLastError());
    if (queue) {
        if constexpr (P::kMasked) hipLaunchKernelGGL(large_masked_kernel<P>, dim3((uint32_t)ctx->cu_count * 8u), dim3(kThreads), 0, ctx->stream, p);
        else hipLaunchKernelGGL(large_kernel<P>, dim3((uint32_t)ctx->cu_count * 8u), dim3(kThreads), 0, ctx->stream, queue, p.queue_cap, p.map, w, p.depth, p.row0);
        UR_HIP_TRY(hipGetLastError());
    }
    return UR_OK;
}

} // namespace
