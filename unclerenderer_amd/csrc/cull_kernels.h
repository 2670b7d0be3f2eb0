// The CullIndirectArgs kernels (see cull.hip) and their one host launch path (cull_launches), shared by the two translation units that
// launch them: cull.hip the camera-only instantiations, cull_views.hip those with extra views. Each kernel is instantiated in one of
// them only, so the camera-only kernels are compiled in a module of their own, as they were before the views existed.
#pragma once

#include "ur_internal.h"
#include "ur_device.h"

#include <hip/hip_ext.h>

#include <algorithm>
#include <cstring>

namespace {

struct CullParams {
    // CullingConstants, CullIndirectArgs.hlsl:1-11
    float4 FrustumPlanes[6];
    float ViewProjection[16];
    uint32_t ModelCount, HZBEnabled, HZBMipCount, HZBWidth, HZBHeight, DebugPrintEnabled;
    const float4* bounds;
    const float* hzb;
    uint8_t* args;
    uint32_t* stats;
    uint32_t* visible_idx;
    uint32_t* visible_count;
    uint32_t* block_counts;
    uint64_t* wave_masks;
    uint32_t index_base;
    uint32_t store_flavour;
    uint32_t record_valid; // store_flavour 4: wave_masks holds the visible bits this context's previous launch left in THIS command buffer
    uint32_t mip_offset[UR_MAX_HZB_MIPS];
    uint32_t mip_width[UR_MAX_HZB_MIPS];
    unsigned long long* timeline; // debug: {first entry, last exit} of this launch (ur_debug_timeline), else null
};

// ur_draw_ranges on the device
struct DrawParams {
    const uint32_t* offsets; // [range_count + 1], offsets[0] = 0, non-decreasing, offsets[range_count] = ModelCount
    uint8_t* commands;
    uint32_t* counts;
    uint32_t range_count;
};

// ur_cull_view[] on the device. A view without ranges has D.range_count == 0; block_counts / wave_masks are its slice of the
// context's scratch (set when the view has a list or ranges and the call has more than one block)
struct ViewParams {
    float4 planes[UR_MAX_CULL_VIEWS][6];
    uint32_t* mask[UR_MAX_CULL_VIEWS];
    uint32_t* visible_idx[UR_MAX_CULL_VIEWS];
    uint32_t* visible_count[UR_MAX_CULL_VIEWS];
    DrawParams D[UR_MAX_CULL_VIEWS];
    uint32_t* block_counts[UR_MAX_CULL_VIEWS];
    uint64_t* wave_masks[UR_MAX_CULL_VIEWS];
    uint32_t count; // 1..UR_MAX_CULL_VIEWS
};

// The kernel arguments: CullParams alone without ranges (the layout the kernels always had), CullParams + DrawParams with them;
// + ViewParams with views
template <bool RANGES, bool VIEWS = false> struct CullArgs : CullParams { DrawParams D; ViewParams V; };
template <> struct CullArgs<false, true> : CullParams { ViewParams V; };
template <> struct CullArgs<true, false> : CullParams { DrawParams D; };
template <> struct CullArgs<false, false> : CullParams {};

__device__ __forceinline__ float saturate_f(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

__device__ __forceinline__ bool IsAabbVisible(const CullParams& C, float3 mn, float3 mx)
{
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const float4 plane = C.FrustumPlanes[i];
        const float px = plane.x >= 0.0f ? mx.x : mn.x;
        const float py = plane.y >= 0.0f ? mx.y : mn.y;
        const float pz = plane.z >= 0.0f ? mx.z : mn.z;
        if (dot3(plane.x, plane.y, plane.z, px, py, pz) + plane.w < 0.0f) return false;
    }
    return true;
}

// RendererUtils::IsAabbInCameraFrustum (RendererUtils.cpp:1192-1218) as oracle/ur_oracle.cpp restates it - the test of the reference's
// CPU visibility loops, kept apart from IsAabbVisible: a plane component >= 0 (-0 included, NaN not) picks max, d is summed in this
// order without contraction, and only d < 0 rejects (a NaN d, the camera's plane 4 under the reverse-Z infinite projection, never does)
__device__ __forceinline__ bool IsAabbInCameraFrustum(const float4* planes, float4 bmin, float4 bmax)
{
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const float4 P = planes[i];
        const float X = P.x >= 0.0f ? bmax.x : bmin.x;
        const float Y = P.y >= 0.0f ? bmax.y : bmin.y;
        const float Z = P.z >= 0.0f ? bmax.z : bmin.z;
        const float d = ((P.x * X + P.y * Y) + P.z * Z) + P.w * 1.0f;
        if (d < 0.0f) return false;
    }
    return true;
}

__device__ __forceinline__ bool IsOccluded(const CullParams& C, float3 mn, float3 mx)
{
    if (C.HZBEnabled == 0 || C.HZBWidth == 0 || C.HZBHeight == 0 || C.HZBMipCount == 0) return false;
    const float* M = C.ViewProjection;
    float minUx = 1.0f, minUy = 1.0f, maxUx = 0.0f, maxUy = 0.0f, maxDepth = 0.0f;
    bool anyBehind = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float cx = (i & 1) ? mx.x : mn.x, cy = (i & 2) ? mx.y : mn.y, cz = (i & 4) ? mx.z : mn.z;
        const float clx = ((cx * M[0] + cy * M[4]) + cz * M[8]) + 1.0f * M[12];
        const float cly = ((cx * M[1] + cy * M[5]) + cz * M[9]) + 1.0f * M[13];
        const float clz = ((cx * M[2] + cy * M[6]) + cz * M[10]) + 1.0f * M[14];
        const float clw = ((cx * M[3] + cy * M[7]) + cz * M[11]) + 1.0f * M[15];
        if (clw <= 0.0f) anyBehind = true; // the HLSL breaks out here; nothing after the break feeds the result
        const float nx = clx / clw, ny = cly / clw, nz = clz / clw;
        const float ux = nx * 0.5f + 0.5f;
        const float uy = 1 - (ny * 0.5f + 0.5f);
        minUx = fminf(minUx, ux); minUy = fminf(minUy, uy);
        maxUx = fmaxf(maxUx, ux); maxUy = fmaxf(maxUy, uy);
        maxDepth = fmaxf(maxDepth, nz);
    }
    if (anyBehind) return false;
    if (maxUx < 0.0f || maxUy < 0.0f || minUx > 1.0f || minUy > 1.0f) return false;
    minUx = saturate_f(minUx); minUy = saturate_f(minUy);
    maxUx = saturate_f(maxUx); maxUy = saturate_f(maxUy);
    const float ex = maxUx - minUx, ey = maxUy - minUy;
    const float psx = ex * (float)C.HZBWidth, psy = ey * (float)C.HZBHeight;
    const float maxDim = fmaxf(psx, psy);
    uint32_t mipLevel = 0;
    if (maxDim > 1.0f) {
        const uint32_t e = ((__float_as_uint(maxDim) >> 23) & 0xFFu) - 127u; // floor(log2(maxDim)), exact
        const float l = fminf(fmaxf((float)e, 0.0f), (float)(C.HZBMipCount - 1u));
        mipLevel = (uint32_t)l;
    }
    const uint32_t mipWidth = max(1u, C.HZBWidth >> mipLevel);
    const uint32_t mipHeight = max(1u, C.HZBHeight >> mipLevel);
    uint32_t minX = (uint32_t)(minUx * (float)mipWidth), minY = (uint32_t)(minUy * (float)mipHeight);
    uint32_t maxX = (uint32_t)(maxUx * (float)mipWidth), maxY = (uint32_t)(maxUy * (float)mipHeight);
    minX = min(minX, mipWidth - 1u); minY = min(minY, mipHeight - 1u);
    maxX = min(maxX, mipWidth - 1u); maxY = min(maxY, mipHeight - 1u);
    const float* mip = C.hzb + C.mip_offset[mipLevel];
    const uint32_t pitch = C.mip_width[mipLevel];
    // HLSL min ignores a NaN texel, signalling or quiet: the loads are quieted first (a raw sNaN operand of v_min_f32 gives NaN)
    float hzbDepth = 1.0f;
    hzbDepth = fminf(hzbDepth, __builtin_canonicalizef(mip[(size_t)minY * pitch + minX]));
    hzbDepth = fminf(hzbDepth, __builtin_canonicalizef(mip[(size_t)minY * pitch + maxX]));
    hzbDepth = fminf(hzbDepth, __builtin_canonicalizef(mip[(size_t)maxY * pitch + minX]));
    hzbDepth = fminf(hzbDepth, __builtin_canonicalizef(mip[(size_t)maxY * pitch + maxX]));
    return maxDepth < hzbDepth;
}

// Scatter the visible indices of one 256-instance block. masks[w] = ballot of wave w; base = visible before this block.
__device__ __forceinline__ void ScatterBlock(uint32_t* visible_idx, uint32_t index_base, uint32_t block, const uint64_t* masks, uint32_t base)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t wave_base = base;
    for (uint32_t w = 0; w < wave; ++w) wave_base += __popcll(masks[w]);
    const uint64_t m = masks[wave];
    if ((m >> lane) & 1ull) {
        const uint32_t rank = __popcll(m & ((1ull << lane) - 1ull));
        visible_idx[wave_base + rank] = block * 256u + threadIdx.x + index_base;
    }
}

// The range r in [lo, hi) holding command i: offsets[r] <= i < offsets[r + 1] (needs offsets[lo] <= i < offsets[hi]).
__device__ __forceinline__ uint32_t RangeOf(const uint32_t* offsets, uint32_t lo, uint32_t hi, uint32_t i)
{
    while (lo + 1u < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The command whose mask writes counts[r]: a non-empty range's last, an empty range's first (the last command if it starts at n).
// Non-decreasing in r, so the ranges one compaction workgroup writes are a run found by binary search.
__device__ __forceinline__ uint32_t CountOwner(const uint32_t* offsets, uint32_t r, uint32_t n)
{
    const uint32_t o0 = offsets[r], o1 = offsets[r + 1u];
    return min(o1 > o0 ? o1 - 1u : o0, n - 1u);
}

// The first range in [0, R) whose count owner is >= t (R if none).
__device__ __forceinline__ uint32_t FirstRangeOwnedFrom(const uint32_t* offsets, uint32_t R, uint32_t n, uint32_t t)
{
    uint32_t lo = 0, hi = R;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (CountOwner(offsets, mid, n) < t) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// One 64-byte command, InstanceCount (dword 11) set to 1 instead of read: four 16-byte loads, four 16-byte stores.
__device__ __forceinline__ void CopyCommand(const uint8_t* args, uint8_t* commands, uint32_t src, uint32_t dst)
{
    const uint4* s = reinterpret_cast<const uint4*>(args + (size_t)src * UR_INDIRECT_COMMAND_STRIDE);
    uint4* d = reinterpret_cast<uint4*>(commands + (size_t)dst * UR_INDIRECT_COMMAND_STRIDE);
    const uint4 a = s[0], b = s[1], e = s[3];
    uint4 c = s[2];
    c.w = 1u;
    d[0] = a; d[1] = b; d[2] = c; d[3] = e;
}

// Visible commands below x (<= 256) of the single block, from its four wave masks.
__device__ __forceinline__ uint32_t BlockRankAt(const uint64_t* masks, uint32_t x)
{
    uint32_t r = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4u; ++w) {
        const uint32_t lo = w * 64u;
        if (x >= lo + 64u) r += (uint32_t)__popcll(masks[w]);
        else if (x > lo) r += (uint32_t)__popcll(masks[w] & ((1ull << (x - lo)) - 1ull));
    }
    return r;
}

// The single block's ranges: each visible command goes to offsets[r] + (visible in r before it); counts[r] from the masks.
// (A destination past the commands can only come from offsets that break the documented precondition: it is skipped.)
__device__ __forceinline__ void PlaceBlock(const DrawParams& D, const uint8_t* args, const uint64_t* masks, uint32_t n)
{
    const uint32_t tid = threadIdx.x;
    if (tid < n && ((masks[tid >> 6] >> (tid & 63u)) & 1ull)) {
        const uint32_t r = RangeOf(D.offsets, 0, D.range_count, tid);
        const uint32_t start = D.offsets[r];
        const uint32_t dst = start + BlockRankAt(masks, tid) - BlockRankAt(masks, start);
        if (dst < n) CopyCommand(args, D.commands, tid, dst);
    }
    for (uint32_t r = tid; r < D.range_count; r += 256u) D.counts[r] = BlockRankAt(masks, D.offsets[r + 1u]) - BlockRankAt(masks, D.offsets[r]);
}

// The views' tests on the staged AABBs. Each view's ballot goes to its mask (lanes 0 and 1 of wave k store u32 words 2k and 2k + 1, those
// below ceil(n / 32)), to LDS, and to the view's scratch slice when a later launch compacts it
template <bool SINGLE_BLOCK>
__device__ __forceinline__ void CullViews(const ViewParams& V, uint32_t n, bool active, const float4* sb, uint64_t (*svmask)[4])
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t wave_global = blockIdx.x * 4u + wave, words = (n + 31u) >> 5;
    float4 bmin = make_float4(0.0f, 0.0f, 0.0f, 0.0f), bmax = bmin;
    if (active) { bmin = sb[2u * tid]; bmax = sb[2u * tid + 1u]; }
#pragma unroll
    for (uint32_t v = 0; v < UR_MAX_CULL_VIEWS; ++v) {
        if (v >= V.count) break; // (launch-uniform)
        const uint64_t m = __ballot(active && IsAabbInCameraFrustum(V.planes[v], bmin, bmax));
        if (V.mask[v] != nullptr && lane < 2u) {
            const uint32_t w = wave_global * 2u + lane;
            if (w < words) V.mask[v][w] = (uint32_t)(m >> (32u * lane));
        }
        if (lane == 0) {
            svmask[v][wave] = m;
            if (!SINGLE_BLOCK && V.wave_masks[v] != nullptr) V.wave_masks[v][wave_global] = m;
        }
    }
}

// After the barrier that publishes svmask: the single block scatters each view's list and places its ranges, a block of a larger call
// writes each compacted view's block count
template <bool SINGLE_BLOCK>
__device__ __forceinline__ void FinishViews(const ViewParams& V, const uint8_t* args, uint32_t n, uint32_t index_base, const uint64_t (*svmask)[4])
{
    const uint32_t tid = threadIdx.x;
#pragma unroll
    for (uint32_t v = 0; v < UR_MAX_CULL_VIEWS; ++v) {
        if (v >= V.count) break;
        const uint32_t total = __popcll(svmask[v][0]) + __popcll(svmask[v][1]) + __popcll(svmask[v][2]) + __popcll(svmask[v][3]);
        if (SINGLE_BLOCK) {
            if (V.visible_idx[v] != nullptr) {
                ScatterBlock(V.visible_idx[v], index_base, 0, svmask[v], 0);
                if (tid == 0) *V.visible_count[v] = total;
            }
            if (V.D[v].range_count != 0) PlaceBlock(V.D[v], args, svmask[v], n);
        } else if (tid == v && V.block_counts[v] != nullptr) V.block_counts[v][blockIdx.x] = total;
    }
}

template <bool SINGLE_BLOCK, bool RANGES, bool VIEWS = false>
__global__ __launch_bounds__(256) void cull_kernel(CullArgs<RANGES, VIEWS> C)
{
    __shared__ float4 sb[512];
    __shared__ uint64_t smask[4];
    __shared__ uint32_t scand[4];
    __shared__ uint8_t slist[256], socc[256];

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t first = blockIdx.x * 256u;
    const uint32_t index = first + tid;
    ur::timeline_entry(C.timeline);

    // stage this block's AABBs: 512 float4, lane-consecutive 16-byte loads. Every load of the thread goes out before the first LDS
    // write (clamped indices instead of branches: one memory latency, not two or three in a row)
    const uint32_t nb = min(512u, (C.ModelCount - first) * 2u); // >= 2: the block has an instance
    const float4* src = C.bounds + (size_t)first * 2u;
    typedef float cf32x4_t __attribute__((ext_vector_type(4)));
    const cf32x4_t* srcv = reinterpret_cast<const cf32x4_t*>(src);
    const cf32x4_t v0 = __builtin_nontemporal_load(srcv + min(tid, nb - 1u)), v1 = __builtin_nontemporal_load(srcv + min(tid + 256u, nb - 1u)); // read once per launch: the hint keeps 32 MB of AABBs from pushing the command lines out of the caches (1 M, cold: 25.3 -> 23.7 us; blind stores 36 -> 26)
    const float4 s0 = make_float4(v0.x, v0.y, v0.z, v0.w), s1 = make_float4(v1.x, v1.y, v1.z, v1.w);

    bool visible = false, frustumVisible = true, occluded = false;
    const bool active = index < C.ModelCount;
    // UR_OPT_CULL_STORE = 3: the word's present value, fetched with the AABBs (its latency lies under the barrier and the tests)
    // UR_OPT_CULL_STORE = 4: ... taken from the context's record instead - one bit per instance, the wave masks of its previous launch on
    // this command buffer (125 KB for 1 M instances instead of 64 MB of command lines); without a valid record, as 3
    uint32_t old_word = 0xFFFFFFFFu;
    const bool from_record = !SINGLE_BLOCK && C.store_flavour == 4u && C.record_valid != 0u; // (launch-uniform)
    uint64_t old_mask = 0;
    if (from_record) old_mask = C.wave_masks[(size_t)blockIdx.x * 4u + wave];
    else if (C.store_flavour >= 3u)
        old_word = *reinterpret_cast<const uint32_t*>(C.args + (size_t)min(index, C.ModelCount - 1u) * UR_INDIRECT_COMMAND_STRIDE + UR_INDIRECT_INSTANCE_COUNT_OFFSET);
    if (tid < nb) sb[tid] = s0;
    if (tid + 256u < nb) sb[tid + 256u] = s1;
    __syncthreads();
    if (active) {
        const float4 bmin = sb[2u * tid], bmax = sb[2u * tid + 1u];
        frustumVisible = IsAabbVisible(C, make_float3(bmin.x, bmin.y, bmin.z), make_float3(bmax.x, bmax.y, bmax.z));
    }
    if (SINGLE_BLOCK) { // a few instances (the frame's own cull: 25 commands): lane by lane, no barrier in the way of the one workgroup's latency
        if (active && frustumVisible && C.HZBEnabled != 0) {
            const float4 bmin = sb[2u * tid], bmax = sb[2u * tid + 1u];
            occluded = IsOccluded(C, make_float3(bmin.x, bmin.y, bmin.z), make_float3(bmax.x, bmax.y, bmax.z));
        }
    } else if (C.HZBEnabled != 0) { // (launch-uniform)
        // The occlusion test (eight corners projected with IEEE divides, a mip choice, four taps) is several times the frustum test, and
        // only what the frustum lets through takes it - one instance in nine of the 1 M stress set: run lane by lane, every wave paid for
        // it at a ninth of its lanes. The block's survivors are packed first (ballots + popcounts, their indices in LDS) and tested
        // densely by the block's first wave(s); every instance still runs the same statements on its own bounds.
        const bool cand = active && frustumVisible;
        const uint64_t cm = __ballot(cand);
        if (lane == 0) scand[wave] = (uint32_t)__popcll(cm);
        __syncthreads();
        uint32_t at = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4u; ++w) { at += w < wave ? scand[w] : 0u; total += scand[w]; }
        if (cand) slist[at + (uint32_t)__popcll(cm & ((1ull << lane) - 1ull))] = (uint8_t)tid;
        __syncthreads();
        if (tid < total) {
            const uint32_t j = slist[tid];
            const float4 bmin = sb[2u * j], bmax = sb[2u * j + 1u];
            socc[j] = IsOccluded(C, make_float3(bmin.x, bmin.y, bmin.z), make_float3(bmax.x, bmax.y, bmax.z)) ? 1u : 0u;
        }
        __syncthreads();
        occluded = cand && socc[tid] != 0u;
    }
    if (active) {
        visible = frustumVisible && !occluded;
        uint32_t* word = reinterpret_cast<uint32_t*>(C.args + (size_t)index * UR_INDIRECT_COMMAND_STRIDE + UR_INDIRECT_INSTANCE_COUNT_OFFSET);
        const uint32_t value = visible ? 1u : 0u;
        // Write-through (sc1): each word is alone in its 64-byte command, so a store is one fabric write whenever it leaves L2; leaving at
        // once means the launch ends with nothing dirty to write back (1 M instances: 22.6 -> 20.0 us words only, 29.1 -> 26.7 with
        // the list; nontemporal stores changed nothing). UR_OPT_CULL_STORE = 0 / 1 select plain / nontemporal stores for comparison.
        // UR_OPT_CULL_STORE = 3 (default): a word that already holds its value is left alone. The command buffer lives across frames
        // (the reference uploads it once per scene, Source/Render/DeferredRenderer.cpp:3397-3442, and its shader rewrites dword 11 in
        // place every frame), and from one frame to the next few instances change sides: the store - a 4-byte write into a 64-byte
        // line of its own, i.e. a read-modify-write of that line in memory - then happens for those few only, the rest costs the
        // 4-byte read. Memory ends up the same in every case (1 M instances over cold buffers: see DESIGN.md 3.2).
        if (C.store_flavour >= 3u) {
            if (from_record) old_word = (uint32_t)(old_mask >> lane) & 1u;
            if (old_word != value) asm volatile("global_store_dword %0, %1, off sc1" ::"v"(word), "v"(value) : "memory");
        } else if (C.store_flavour == 2u) asm volatile("global_store_dword %0, %1, off sc1" ::"v"(word), "v"(value) : "memory");
        else if (C.store_flavour == 1u) __builtin_nontemporal_store(value, word);
        else *word = value;
    }
    [[maybe_unused]] __shared__ uint64_t svmask[VIEWS ? UR_MAX_CULL_VIEWS : 1][4]; // VIEWS
    if constexpr (VIEWS) CullViews<SINGLE_BLOCK>(C.V, C.ModelCount, active, sb, svmask);

    if (C.DebugPrintEnabled != 0 && C.stats != nullptr) { // one atomic per wave instead of one per lane
        const uint32_t nf = __popcll(__ballot(active && !frustumVisible));
        const uint32_t no = __popcll(__ballot(active && frustumVisible && occluded));
        if (lane == 0) {
            if (nf) atomicAdd(&C.stats[0], nf);
            if (no) atomicAdd(&C.stats[1], no);
        }
    }

    if (!RANGES && !VIEWS && C.visible_idx == nullptr) { // uniform (with ranges or views the masks are needed below, list or not)
        if (!SINGLE_BLOCK && C.store_flavour == 4u) { // the record of what the command buffer holds now (a launch with a list writes it below)
            const uint64_t m = __ballot(visible);
            if (lane == 0) C.wave_masks[(size_t)blockIdx.x * 4u + wave] = m;
        }
        ur::timeline_exit(C.timeline, tid == 0);
        return;
    }
    const uint64_t mask = __ballot(visible);
    if (lane == 0) smask[wave] = mask;
    __syncthreads();
    if (SINGLE_BLOCK) {
        if ((!RANGES && !VIEWS) || C.visible_idx != nullptr) {
            ScatterBlock(C.visible_idx, C.index_base, 0, smask, 0);
            if (tid == 0) *C.visible_count = __popcll(smask[0]) + __popcll(smask[1]) + __popcll(smask[2]) + __popcll(smask[3]);
        }
        if constexpr (RANGES) PlaceBlock(C.D, C.args, smask, C.ModelCount); // (each visible lane copies the command whose word it stored)
    } else {
        if (lane == 0) C.wave_masks[(size_t)blockIdx.x * 4u + wave] = mask;
        if (tid == 0) C.block_counts[blockIdx.x] = __popcll(smask[0]) + __popcll(smask[1]) + __popcll(smask[2]) + __popcll(smask[3]);
    }
    if constexpr (VIEWS) FinishViews<SINGLE_BLOCK>(C.V, C.args, C.ModelCount, C.index_base, svmask);
    ur::timeline_exit(C.timeline, tid == 0);
}

// Pass 2: one thread per wave mask (64 instances), one workgroup per 256 masks = 64 cull blocks. The workgroup's base is
// the sum of the block counts in front of it (a few loads per thread), a thread's offset the exclusive scan of the mask
// popcounts inside the workgroup; the few set bits of a mask are written out in ascending order.
// RANGES: a visible command i of range r goes to slot offsets[r] + rank(i) - rank(offsets[r]) (rank = visible commands in front).
// The ranks inside the workgroup's span of 16384 commands are its threads' prefixes + popcounts (in LDS); the one range start in
// front of the span that matters - that of the range holding the span's first command - is summed in the same sweep over the
// block counts (a second accumulator up to that start's block) plus the masks of its block below it. counts[r] is written by
// the workgroup that holds CountOwner(r).
template <bool VIEWS, class Args> __device__ __forceinline__ const auto* SelectRow(const Args* C, const CullArgs<true>* W)
{
    if constexpr (VIEWS) return W;
    else return C;
}

// With views (VIEWS): one row of workgroups per list / set of ranges - row 0 the camera's, row 1 + v view v's, each running the body on
// its own arguments (A), with or without ranges at run time. Without views A is C.
template <bool RANGES, bool VIEWS> struct CompactRow { typedef CullArgs<true> type; };
template <bool RANGES> struct CompactRow<RANGES, false> { typedef CullArgs<RANGES> type; };

template <bool RANGES, bool VIEWS = false>
__global__ __launch_bounds__(256) void compact_kernel(CullArgs<RANGES, VIEWS> C, uint32_t num_blocks)
{
    [[maybe_unused]] CullArgs<true> W{}; // VIEWS
    if constexpr (VIEWS) {
        W.ModelCount = C.ModelCount;
        W.args = C.args;
        W.index_base = C.index_base;
        if (blockIdx.y == 0) { // (uniform)
            W.wave_masks = C.wave_masks;
            W.block_counts = C.block_counts;
            W.visible_idx = C.visible_idx;
            W.visible_count = C.visible_count;
            if constexpr (RANGES) W.D = C.D;
        } else {
#pragma unroll
            for (uint32_t v = 0; v < UR_MAX_CULL_VIEWS; ++v) {
                if (v + 1u != blockIdx.y) continue;
                W.wave_masks = C.V.wave_masks[v];
                W.block_counts = C.V.block_counts[v];
                W.visible_idx = C.V.visible_idx[v];
                W.visible_count = C.V.visible_count[v];
                W.D = C.V.D[v];
            }
        }
        if (W.D.range_count == 0 && W.visible_idx == nullptr) return; // (a row with nothing to compact)
    }
    const typename CompactRow<RANGES, VIEWS>::type& A = *SelectRow<VIEWS>(&C, &W);
    __shared__ uint32_t spart[4], swave[4];
    [[maybe_unused]] __shared__ uint32_t spart2[4]; // RANGES (VIEWS)
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t num_masks = num_blocks * 4u, mi = blockIdx.x * 256u + tid;
    const uint64_t m = mi < num_masks ? A.wave_masks[mi] : 0ull;
    // the counts of the blocks in front: sixteen loads per thread in flight at once (a loop of dependent-looking loads made the last
    // workgroups of a 1 M-instance cull wait for fifteen memory round trips in a row), then the rare rest
    uint32_t s = 0;
    const uint32_t limit = blockIdx.x * 64u;
    // RANGES: span_start = the span's first command, r0 = the range holding it, s0 = that range's start (<= span_start), s0_block its block
    const uint32_t span_start = blockIdx.x * 16384u;
    uint32_t r0 = 0, s0 = 0, s0_block = 0, s2 = 0;
    if (limit != 0u) { // uniform
        uint32_t part[16];
#pragma unroll
        for (uint32_t k = 0; k < 16u; ++k) part[k] = A.block_counts[min(tid + k * 256u, limit - 1u)];
        if constexpr (RANGES || VIEWS) if (!VIEWS || A.D.range_count != 0) { // (uniform: scalar loads, under the vector loads above)
            r0 = RangeOf(A.D.offsets, 0, A.D.range_count, span_start);
            s0 = A.D.offsets[r0];
            s0_block = s0 >> 8;
        }
#pragma unroll
        for (uint32_t k = 0; k < 16u; ++k) s += tid + k * 256u < limit ? part[k] : 0u;
        if constexpr (RANGES || VIEWS) if (!VIEWS || A.D.range_count != 0) {
#pragma unroll
            for (uint32_t k = 0; k < 16u; ++k) s2 += tid + k * 256u < s0_block ? part[k] : 0u;
        }
        for (uint32_t b = tid + 4096u; b < limit; b += 256u) {
            const uint32_t v = A.block_counts[b];
            s += v;
            if constexpr (RANGES || VIEWS) s2 += b < s0_block ? v : 0u;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    // inclusive scan of the popcounts across the wave, then across the four waves
    const uint32_t c = __popcll(m);
    uint32_t incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o);
        if (lane >= (uint32_t)o) incl += up;
    }
    if (lane == 0) spart[wave] = s;
    if (lane == 63) swave[wave] = incl;
    if constexpr (RANGES || VIEWS) if (!VIEWS || A.D.range_count != 0) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s2 += __shfl_xor(s2, o);
        if (lane == 0) spart2[wave] = s2;
    }
    __syncthreads();
    uint32_t at = spart[0] + spart[1] + spart[2] + spart[3] + incl - c;
    for (uint32_t w = 0; w < wave; ++w) at += swave[w];
    if constexpr (RANGES || VIEWS) if (!VIEWS || A.D.range_count != 0) {
        __shared__ uint32_t sat[257];
        __shared__ uint64_t sbits[256];
        const DrawParams& D = A.D;
        const uint32_t n = A.ModelCount;
        // rank(s0): the blocks in front of its block, then its block's masks below it (s0 == span_start: nothing more)
        uint32_t rank_s0 = spart2[0] + spart2[1] + spart2[2] + spart2[3];
        for (uint32_t j = s0_block * 4u; j < (s0 >> 6); ++j) rank_s0 += (uint32_t)__popcll(A.wave_masks[j]);
        if (s0 & 63u) rank_s0 += (uint32_t)__popcll(A.wave_masks[s0 >> 6] & ((1ull << (s0 & 63u)) - 1ull));
        sat[tid] = at;
        sbits[tid] = m;
        if (tid == 255u) sat[256] = at + c;
        // the ranges whose counts this workgroup writes, and the last range a command of the span can lie in
        const uint32_t r_first = FirstRangeOwnedFrom(D.offsets, D.range_count, n, span_start);
        const uint32_t r_end = FirstRangeOwnedFrom(D.offsets, D.range_count, n, span_start + 16384u);
        const uint32_t r_hi = min(r_end + 1u, D.range_count);
        __syncthreads();
        // rank(x) for x = s0 or x in (span_start, span_start + 16384]
        auto rank_at = [&](uint32_t x) -> uint32_t {
            if (x < span_start) return rank_s0;
            const uint32_t d = x - span_start;
            if (d >= 16384u) return sat[256];
            return sat[d >> 6] + (uint32_t)__popcll(sbits[d >> 6] & ((1ull << (d & 63u)) - 1ull));
        };
        uint64_t bits = m;
        uint32_t rank = at, r = r0;
        while (bits) {
            const uint32_t i = mi * 64u + (uint32_t)__builtin_ctzll(bits);
            r = RangeOf(D.offsets, r, r_hi, i);
            const uint32_t start = D.offsets[r];
            const uint32_t dst = start + rank - rank_at(start);
            if (dst < n) CopyCommand(A.args, D.commands, i, dst); // (only offsets that break the precondition could send it further)
            ++rank;
            bits &= bits - 1ull;
        }
        for (uint32_t q = r_first + tid; q < r_end; q += 256u) {
            const uint32_t o0 = D.offsets[q], o1 = D.offsets[q + 1u];
            D.counts[q] = o1 > o0 ? rank_at(o1) - rank_at(o0) : 0u;
        }
        if (A.visible_idx == nullptr) return; // (the list is optional with ranges)
    }
    uint64_t bits = m;
    const uint32_t first = mi * 64u + A.index_base;
    while (bits) {
        const uint32_t b = __builtin_ctzll(bits);
        A.visible_idx[at++] = first + b;
        bits &= bits - 1ull;
    }
    if (mi == num_masks - 1u) *A.visible_count = at;
}

// ModelCount == 0: every count (camera's and views') and every counts[r], one launch
struct ZeroArgs {
    uint32_t* count[1 + UR_MAX_CULL_VIEWS];
    uint32_t* counts[1 + UR_MAX_CULL_VIEWS];
    uint32_t range_count[1 + UR_MAX_CULL_VIEWS];
};
__global__ void zero_views_kernel(ZeroArgs Z)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
#pragma unroll
    for (uint32_t k = 0; k < 1u + UR_MAX_CULL_VIEWS; ++k) {
        if (i == 0 && Z.count[k]) *Z.count[k] = 0;
        if (i < Z.range_count[k]) Z.counts[k][i] = 0;
    }
}

// One 256-thread launch on the context's stream; with `stop` (ur_time_next_cull) its dispatch carries the event
template <class K, class... Args>
int launch_stop(ur_ctx* ctx, hipEvent_t stop, K kernel, dim3 grid, const Args&... args)
{
    if (stop != nullptr) hipExtLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, nullptr, stop, 0, args...);
    else hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, args...);
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

DrawParams draw_params(const ur_draw_ranges& d) { return {d.offsets, static_cast<uint8_t*>(d.commands), d.counts, d.range_count}; }

// The launches of one cull call after the HZB tail is flushed: the camera alone (VIEWS = false, cull.hip) or with view_count >= 1
// extra views (cull_views.hip). Each translation unit instantiates it once, so each module holds its own set of kernels only.
template <bool VIEWS>
int cull_launches(ur_ctx* ctx, const uint32_t* constants, const ur_float4* bounds, const float* hzb, const ur_mip_desc* mips,
                  void* indirect_args, uint32_t* stats2, uint32_t* visible_idx, uint32_t* visible_count, uint32_t index_base,
                  const ur_draw_ranges* draws, const ur_cull_view* views, uint32_t view_count)
{
    if constexpr (!VIEWS) view_count = 0;
    CullArgs<true, VIEWS> P{};
    static_assert(sizeof(float4) * 6 + sizeof(float) * 16 + 6 * 4 == UR_CULL_CONSTANT_DWORDS * 4, "46 dwords");
    std::memcpy(static_cast<CullParams*>(&P), constants, UR_CULL_CONSTANT_DWORDS * 4);
    P.bounds = reinterpret_cast<const float4*>(bounds);
    P.hzb = hzb;
    P.args = static_cast<uint8_t*>(indirect_args);
    P.stats = stats2;
    P.visible_idx = visible_idx;
    P.visible_count = visible_count;
    P.index_base = index_base;
    P.store_flavour = (uint32_t)ctx->opt.cull_store; // UR_OPT_CULL_STORE
    P.timeline = P.ModelCount != 0 ? ur::next_timeline_pair(ctx) : nullptr; // (the compaction launch of a large cull is not stamped)
    if (P.HZBEnabled != 0) {
        for (uint32_t m = 0; m < P.HZBMipCount && m < UR_MAX_HZB_MIPS; ++m) {
            P.mip_offset[m] = mips[m].offset;
            P.mip_width[m] = mips[m].width;
        }
    }
    if (draws) P.D = draw_params(*draws);
    if constexpr (VIEWS) {
        P.V.count = view_count;
        for (uint32_t v = 0; v < view_count; ++v) {
            std::memcpy(P.V.planes[v], views[v].planes, sizeof(P.V.planes[v]));
            P.V.mask[v] = views[v].mask;
            P.V.visible_idx[v] = views[v].visible_idx;
            P.V.visible_count[v] = views[v].visible_count;
            if (views[v].draws) P.V.D[v] = draw_params(*views[v].draws);
        }
    }
    // UR_OPT_CULL_STORE = 4: the wave masks ARE the record of what a multi-block launch leaves in the command buffer; they describe the
    // buffer the next launch meets if that launch is on the same buffer with the same count (and the caller keeps the promise of the
    // option). The record is forgotten here and kept again only once every launch of this call has gone out.
    const uint32_t n = P.ModelCount;
    bool record_valid = P.store_flavour == 4u && ctx->cull_record_args == indirect_args && ctx->cull_record_n == n;
    ctx->cull_record_args = nullptr;
    // ur_time_next_cull: the call's LAST launch carries the event on its dispatch (its completion stamp is somebody's start time).
    // (The entry point clears the context's copy behind this function on every path: a raw hipEvent_t must not stay in the context.)
    hipEvent_t stop = ctx->time_cull_stop;
    // a view with a list or ranges (compacted, with a scratch slice of its own, above one block)
    auto compacted = [&](uint32_t v) { return views[v].visible_idx != nullptr || views[v].draws != nullptr; };

    if (n == 0) { // one launch zeroes every count and every counts[r], if there are any (no mask word is written)
        ZeroArgs Z{};
        Z.count[0] = visible_count;
        if (draws) { Z.counts[0] = draws->counts; Z.range_count[0] = draws->range_count; }
        bool zero = visible_count != nullptr || draws != nullptr;
        uint32_t most = Z.range_count[0];
        for (uint32_t v = 0; v < view_count; ++v) {
            zero = zero || views[v].visible_count || views[v].draws;
            Z.count[1 + v] = views[v].visible_count;
            if (views[v].draws) {
                Z.counts[1 + v] = views[v].draws->counts;
                Z.range_count[1 + v] = views[v].draws->range_count;
                most = std::max(most, views[v].draws->range_count);
            }
        }
        if (!zero) return UR_OK;
        const int rc = launch_stop(ctx, stop, zero_views_kernel, dim3(std::max(1u, (uint32_t)(((uint64_t)most + 255u) / 256u))), Z);
        if (rc != UR_OK) return rc;
        ctx->time_cull_carried = stop != nullptr;
        return UR_OK;
    }
    CullArgs<false, VIEWS> Q{}; // (the same parameters without the camera's ranges; filled in front of the launches)
    const uint32_t blocks = (n + 255u) / 256u;
    int rc = UR_OK;
    if (blocks == 1) { // (one block keeps no masks: no record)
        static_cast<CullParams&>(Q) = P;
        if constexpr (VIEWS) Q.V = P.V;
        rc = draws ? launch_stop(ctx, stop, cull_kernel<true, true, VIEWS>, dim3(1), P) : launch_stop(ctx, stop, cull_kernel<true, false, VIEWS>, dim3(1), Q);
        if (rc != UR_OK) return rc;
        ctx->time_cull_carried = stop != nullptr;
        return UR_OK;
    }
    // the masks and block counts: the compaction's input, flavour 4's record (with views the camera's are always written)
    bool compact = draws != nullptr || visible_idx != nullptr;
    if (VIEWS || compact || P.store_flavour == 4u) {
        if (n > ctx->ws_instances) {
            rc = ur_reserve(ctx, n);
            if (rc != UR_OK) return rc;
            record_valid = false; // (a new workspace holds no record)
        }
        P.block_counts = ctx->block_counts;
        P.wave_masks = ctx->wave_masks;
        if constexpr (VIEWS) { // slice 0 is the camera's (and flavour 4's record); view v's is slice 1 + v
            const uint32_t stride = ctx->ws_instances / 256u;
            for (uint32_t v = 0; v < view_count; ++v) {
                if (!compacted(v)) continue;
                compact = true;
                P.V.block_counts[v] = ctx->block_counts + (size_t)(1u + v) * stride;
                P.V.wave_masks[v] = ctx->wave_masks + (size_t)(1u + v) * stride * 4u;
            }
        }
    }
    P.record_valid = record_valid ? 1u : 0u;
    static_cast<CullParams&>(Q) = P;
    if constexpr (VIEWS) Q.V = P.V;
    // the cull, then the compaction when there is a list or there are ranges: one row of workgroups for the camera, one per view
    const dim3 compaction_grid((blocks * 4u + 255u) / 256u, 1u + view_count);
    if (draws) {
        rc = launch_stop(ctx, compact ? nullptr : stop, cull_kernel<false, true, VIEWS>, dim3(blocks), P);
        if (rc == UR_OK && compact) rc = launch_stop(ctx, stop, compact_kernel<true, VIEWS>, compaction_grid, P, blocks);
    } else {
        rc = launch_stop(ctx, compact ? nullptr : stop, cull_kernel<false, false, VIEWS>, dim3(blocks), Q);
        if (rc == UR_OK && compact) rc = launch_stop(ctx, stop, compact_kernel<false, VIEWS>, compaction_grid, Q, blocks);
    }
    if (rc != UR_OK) return rc;
    if (P.store_flavour == 4u) {
        ctx->cull_record_args = indirect_args;
        ctx->cull_record_n = n;
    }
    ctx->time_cull_carried = stop != nullptr;
    return UR_OK;
}

} // namespace
