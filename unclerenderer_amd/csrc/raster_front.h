// The front half that raster_kernel (csrc/raster_kernels.h) and pick_kernel (csrc/raster_pick.hip) share, and so the one place in device
// code where the rules of DESIGN.md sections 3.7-3.9 up to the snapped triangle are written: the walk over the draws - the work split,
// the selection, the command and its refusals, the 64-triangle chunks -, the lane's triangle through P::project / P::assemble, the guard
// band, the snap, rule 3 and the depth plane, the per-wave counters, and rules 4-5 for one pixel centre. What is done with a surviving
// triangle is the caller's: the raster clamps its box to the target and the band and serves fragments, the pick keeps the box as it is
// and tests its points.
//
// The walk is a loop template around a functor and not a function that hands the command back, and it says with uniform() which of the
// command's dwords live in scalar registers: so every kernel keeps its occupancy step (DESIGN.md section 3.16 has the figures of each shape).
#pragma once

#include "raster_params.h"

namespace {

__device__ __forceinline__ int rl(int v, uint32_t s) { return __builtin_amdgcn_readlane(v, (int)s); }
__device__ __forceinline__ float rlf(float v, uint32_t s) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int)s)); }

// Four dwords the wave loaded from a uniform address (a vector load: the kernels store, so the compiler issues no scalar one), said to be
// uniform: they then live in scalar registers. Called with every lane active
__device__ __forceinline__ u32x4_t uniform(u32x4_t v)
{
    u32x4_t r;
    r.x = __builtin_amdgcn_readfirstlane(v.x); r.y = __builtin_amdgcn_readfirstlane(v.y);
    r.z = __builtin_amdgcn_readfirstlane(v.z); r.w = __builtin_amdgcn_readfirstlane(v.w);
    return r;
}

// What a wave counts, uniform, and adds to stats once at its end. `unqueued` is the raster's alone: the pick never counts it, so it never
// touches stats[3]; a pass that emits one triangle per lane never touches [4] and [5]
struct WaveCounts {
    uint32_t drawn = 0, unsupported = 0, dropped = 0, unqueued = 0, cut = 0, behind = 0;
};

template <class P>
__device__ __forceinline__ void flush_counts(uint32_t* stats, uint32_t lane, const WaveCounts& n)
{
    if (stats == nullptr || lane != 0u) return;
    if (n.drawn) (void)__hip_atomic_fetch_add(stats + 0, n.drawn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n.unsupported) (void)__hip_atomic_fetch_add(stats + 1, n.unsupported, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n.dropped) (void)__hip_atomic_fetch_add(stats + 2, n.dropped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n.unqueued) (void)__hip_atomic_fetch_add(stats + 3, n.unqueued, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if constexpr (P::kEmit > 1u) {
        if (n.cut) (void)__hip_atomic_fetch_add(stats + 4, n.cut, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n.behind) (void)__hip_atomic_fetch_add(stats + 5, n.behind, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// What a command that passed the refusals says (uniform)
struct Draw {
    const uint32_t* indices;
    const uint8_t* vertices;
    uint64_t index_slots;
    uint32_t vb_size, stride, tri_count, start_index;
    long long base_vertex;
    float W[16]; // World, the head of the draw's constants
};

// A wave per (draw candidate, segment): it walks the 64-triangle chunks c = segment, segment + S, ... of its command and calls
// body(candidate, triangle index of the lane, draw) for each. The candidate is the ordinal under every selection
template <class P, class Params, class Body>
__device__ __forceinline__ void walk_draws(const Params& p, uint32_t lane, WaveCounts& n, Body body)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
    const uint32_t wave_count = gridDim.x * kWaves;
    for (uint32_t item = wave; item < p.items; item += wave_count) {
        const uint32_t cand = item / p.segments, seg = item - cand * p.segments;
        // ---- selection: the candidate's slot, or none
        uint32_t slot = cand;
        if (p.mode == 1u) {
            if (cand >= *p.visible_count) continue;
            slot = p.visible_idx[cand] - p.index_base;
        } else if (p.mode == 2u) {
            uint32_t lo = 0u, hi = p.range_count + 1u; // first k with offsets[k] > cand
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (p.offsets[mid] > cand) hi = mid; else lo = mid + 1u;
            }
            if (lo == 0u || lo > p.range_count) continue;
            const uint32_t r = lo - 1u;
            if (cand - p.offsets[r] >= p.counts[r]) continue;
        }
        slot = __builtin_amdgcn_readfirstlane(slot);
        if (slot >= p.command_count) continue;
        // ---- the command (uniform): the vertex buffer's and the constants' vectors to scalar registers, the other two as the compiler likes
        const u32x4_t* cmd = reinterpret_cast<const u32x4_t*>(p.commands + (size_t)slot * UR_INDIRECT_COMMAND_STRIDE);
        const u32x4_t c0 = uniform(cmd[0]), c1 = cmd[1], c2 = uniform(cmd[2]), c3 = cmd[3];
        if (c2.w == 0u) continue; // InstanceCount
        const uint64_t vb = (uint64_t)c0.x | ((uint64_t)c0.y << 32), ib = (uint64_t)c1.x | ((uint64_t)c1.y << 32), cb = (uint64_t)c2.x | ((uint64_t)c2.y << 32);
        const uint32_t stride = c0.w, format = c1.w, tri_count = c2.z / 3u;
        bool too_many = false;
        if constexpr (P::kKeyed) too_many = tri_count > (1u << p.key_bits);
        if (too_many || format != UR_RASTER_INDEX_FORMAT_R32_UINT || stride < P::kVertexBytes || (stride & 3u) != 0u || vb == 0u || (vb & 3u) != 0u || ib == 0u || (ib & 3u) != 0u ||
            cb == 0u || (cb & 3u) != 0u) {
            if (seg == 0u) n.unsupported += tri_count;
            continue;
        }
        const uint32_t chunks = (tri_count + 63u) / 64u;
        if (seg >= chunks) continue;
        Draw d;
        d.indices = reinterpret_cast<const uint32_t*>(ib);
        d.vertices = reinterpret_cast<const uint8_t*>(vb);
        d.index_slots = c1.z / 4u; // ib_size
        d.vb_size = c0.z; d.stride = stride; d.tri_count = tri_count; d.start_index = c3.x;
        d.base_vertex = (int)c3.y;
        {
            const float* wp = reinterpret_cast<const float*>(cb);
#pragma unroll
            for (int k = 0; k < 16; ++k) d.W[k] = wp[k];
        }
        for (uint32_t chunk = seg; chunk < chunks; chunk += p.segments) body(cand, chunk * 64u + lane, d);
    }
}

// The lane's triangle in target space: up to four vertices S0..S3, `emit` triangles (S0, S[1 + e], S[2 + e])
struct LaneVerts {
    float SX[4] = {}, SY[4] = {}, SZ[4] = {};
    uint32_t emit = 0u;
};

// A lane per triangle: rules 1-2 (and the near clip) for triangle t of the draw. Returns how many emitted triangles the wave has to go
// over: 2 when a ballot finds a lane that was cut into two
template <class P, class Params>
__device__ __forceinline__ uint32_t lane_triangle(const Params& p, const Draw& d, uint32_t t, LaneVerts& s, WaveCounts& n)
{
    bool unsupported = false, cut = false, behind = false;
    if (t < d.tri_count) {
        const uint64_t first = (uint64_t)d.start_index + 3ull * t;
        float clip[3][4] = {};
        if (first + 2u >= d.index_slots) unsupported = true;
        if (!unsupported) {
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                const long long vi = d.base_vertex + (long long)d.indices[first + (uint32_t)v];
                if (vi < 0 || (uint64_t)vi * d.stride + P::kVertexBytes > (uint64_t)d.vb_size) { unsupported = true; continue; }
                P::project(reinterpret_cast<const float*>(d.vertices + (uint64_t)vi * d.stride), d.W, p, clip[v]);
            }
        }
        if (!unsupported) s.emit = P::assemble(clip, p, s.SX, s.SY, s.SZ, unsupported, cut, behind);
    }
    n.unsupported += (uint32_t)__popcll(__ballot(unsupported));
    uint32_t passes = 1u;
    if constexpr (P::kEmit > 1u) {
        n.cut += (uint32_t)__popcll(__ballot(cut));
        n.behind += (uint32_t)__popcll(__ballot(behind));
        if (__ballot(s.emit > 1u) != 0ull) passes = 2u;
    }
    return passes;
}

// Emitted triangle e of the lane: the guard band, the snap, rule 3 and rule 5's depth plane. True iff the triangle is drawn, and `tri`
// is then whole; every lane of the wave calls it (the counters are ballots)
template <class P>
__device__ __forceinline__ bool snap_triangle(const LaneVerts& s, uint32_t e, Tri& tri, WaveCounts& n)
{
    bool drawn = false, dropped = false;
    if (e < s.emit) {
        float X[3], Y[3], Z[3];
        const bool second = P::kEmit > 1u && e != 0u;
        const int i1 = P::kSwap12 ? 2 : 1, i2 = P::kSwap12 ? 1 : 2; // (DepthPrepass: (u0, u2, u1))
        X[0] = s.SX[0]; Y[0] = s.SY[0]; Z[0] = s.SZ[0];
        X[i1] = second ? s.SX[2] : s.SX[1]; Y[i1] = second ? s.SY[2] : s.SY[1]; Z[i1] = second ? s.SZ[2] : s.SZ[1];
        X[i2] = second ? s.SX[3] : s.SX[2]; Y[i2] = second ? s.SY[3] : s.SY[2]; Z[i2] = second ? s.SZ[3] : s.SZ[2];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const bool finite = fabsf(X[v]) <= kFloatMax && fabsf(Y[v]) <= kFloatMax && fabsf(Z[v]) <= kFloatMax; // (false for NaN)
            if (!finite || fabsf(X[v]) > P::kGuardBand || fabsf(Y[v]) > P::kGuardBand) dropped = true;
        }
        if (!dropped) {
            tri.x0 = (int)rintf(X[0] * 256.0f); tri.y0 = (int)rintf(Y[0] * 256.0f);
            tri.x1 = (int)rintf(X[1] * 256.0f); tri.y1 = (int)rintf(Y[1] * 256.0f);
            tri.x2 = (int)rintf(X[2] * 256.0f); tri.y2 = (int)rintf(Y[2] * 256.0f);
            const long long A = (long long)(tri.x1 - tri.x0) * (tri.y2 - tri.y0) - (long long)(tri.x2 - tri.x0) * (tri.y1 - tri.y0); // rule 3
            if (A > 0) {
                drawn = true;
                const float inv = 1.0f / (float)A; // rule 5
                tri.z0 = Z[0];
                tri.k1 = (Z[1] - Z[0]) * inv;
                tri.k2 = (Z[2] - Z[0]) * inv;
            }
        }
    }
    n.drawn += (uint32_t)__popcll(__ballot(drawn));
    n.dropped += (uint32_t)__popcll(__ballot(dropped));
    return drawn;
}

// The pixels whose centres 256 p + 128 lie inside the triangle's [min, max], not clamped to anything; empty when a maximum is below its minimum
__device__ __forceinline__ void centre_box(const Tri& t, int& bx0, int& by0, int& bx1, int& by1)
{
    const int minx = min(t.x0, min(t.x1, t.x2)), maxx = max(t.x0, max(t.x1, t.x2));
    const int miny = min(t.y0, min(t.y1, t.y2)), maxy = max(t.y0, max(t.y1, t.y2));
    bx0 = (minx + 127) >> 8; bx1 = (maxx - 128) >> 8;
    by0 = (miny + 127) >> 8; by1 = (maxy - 128) >> 8;
}

// Rules 4-5 for the centre of pixel (px, py): false when an edge function rejects it, else z from the plane. A pass over a reverse-Z target
// (not P::kNearest) also drops z below 0 or NaN, clamps to 1 - the geometry lies inside z <= w: only rounding goes above - and quantises to D24
template <class P>
__device__ __forceinline__ bool covered_depth(const Tri& t, int b01, int b12, int b20, int px, int py, float& z)
{
    const int sx = 256 * px + 128, sy = 256 * py + 128;
    const long long e01 = (long long)(t.x1 - t.x0) * (sy - t.y0) - (long long)(t.y1 - t.y0) * (sx - t.x0);
    const long long e12 = (long long)(t.x2 - t.x1) * (sy - t.y1) - (long long)(t.y2 - t.y1) * (sx - t.x1);
    const long long e20 = (long long)(t.x0 - t.x2) * (sy - t.y2) - (long long)(t.y0 - t.y2) * (sx - t.x2);
    if (((e01 - b01) | (e12 - b12) | (e20 - b20)) < 0) return false;
    z = t.z0 + ((float)e20 * t.k1 + (float)e01 * t.k2);
    if constexpr (!P::kNearest) {
        if (!(z >= 0.0f)) return false;
        if (z > 1.0f) z = 1.0f;
        if constexpr (P::kD24) z = (float)(__builtin_rint((double)z * 16777215.0) / 16777215.0);
    }
    return true;
}

} // namespace
