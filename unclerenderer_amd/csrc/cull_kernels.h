// The CullIndirectArgs kernels (see cull.hip), shared by the two translation units that launch them: cull.hip the camera-only
// instantiations, cull_views.hip those with extra views. Each kernel is instantiated in one of them only, so the camera-only kernels are
// compiled in a module of their own, as they were before the views existed. Here: cull_kernel (pass 1, and the whole call up to 256
// instances) with its views' part, and the zeroing kernel; the arguments are in cull_params.h, the three visibility tests in cull_tests.h,
// the compaction (pass 2, compact_kernel) and its helpers in cull_compact.h. Their one host launch path, cull_launches, is in
// cull_launch.h; what it decides is planned in cull_plan.cpp.
#pragma once

#include "cull_params.h"
#include "cull_tests.h"
#include "cull_compact.h"

namespace {

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

// ModelCount == 0: every count (camera's and views') and every counts[r], one launch (ZeroArgs)
__global__ void zero_views_kernel(ZeroArgs Z)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
#pragma unroll
    for (uint32_t k = 0; k < 1u + UR_MAX_CULL_VIEWS; ++k) {
        if (i == 0 && Z.count[k]) *Z.count[k] = 0;
        if (i < Z.range_count[k]) Z.counts[k][i] = 0;
    }
}

} // namespace
