// The compaction of CullIndirectArgs (cull_kernels.h): from wave masks to an ascending visible list and to draw ranges. The rank, range
// and placement helpers (the single block of cull_kernel uses them on its own masks in LDS) and compact_kernel, pass 2 of a larger call.
#pragma once

#include "cull_params.h"

namespace {

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

} // namespace
