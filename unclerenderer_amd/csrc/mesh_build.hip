// ur_mesh_build (include/ur_mesh.h): a glTF buffer becomes 64-byte vertices and R32 indices on the device, by
// the rule of csrc/mesh_rule.h, the file the serial host build (csrc/mesh_host.cpp) runs. The reference's per-vertex sums run over the
// incident triangles in triangle order, in fp32; here every vertex gets its corners (3 * triangle + corner) as a CSR segment, and a sum
// walks its segment in ascending corner order, so the bits are the serial ones whatever order the atomics filled the segment in.
//
//   clear      the header (flags, counters, bounds keys) and the per-vertex counts: the scratch arrives with any content
//   assemble   a lane per vertex: gathers the streams, four 16-byte stores; a wave reduction and one atomic per wave for the two
//              "all valid" flags and the bounds (64-bit keys: the ordered value above the vertex index, so that of equal values the
//              first wins as in the serial std::min / std::max, -0 and +0 being equal)
//   triangles  a lane per triangle: expands and writes its three indices; when a pass will run, counts its corners per vertex and
//              writes its contributions (12 bytes for the normal pass, 24 and a skip byte for the tangent pass)
//   scan       reduce / scan of sums / add, three launches, no workgroup waits on another; vertices with more than kLaneSegment corners
//              go into the long queue
//   fill       a lane per triangle: an atomic cursor per vertex places the corners; the order inside a segment is not defined
//   sort       a workgroup per queued vertex: bitonic sort of the segment in place (2048-corner tiles in LDS, the wider strides in
//              global memory; every compare-exchange ascending, so a segment of any length sorts with virtual padding behind it)
//   sums       per pass a lane per vertex (repeated selection of the next-greater corner, fused with the sum) and a workgroup per
//              queued vertex (contributions fetched by 256 lanes into LDS, one lane adds in order)
//   info       one lane writes ur_mesh_info
// Every launch is unconditional; the kernels of a pass read its flag from the header and leave when nothing is to be regenerated.

#include <algorithm>
#include <vector>

#include "mesh_rule.h"
#include "ur_internal.h"

namespace ur {
namespace {

using namespace ur_mesh;

constexpr uint32_t kThreads = 256u, kSortTile = 2048u, kLongGrid = 1024u;
// header words
enum : uint32_t { kNormalsInvalid = 0u, kTangentsInvalid = 1u, kSkipped = 2u, kOutOfRange = 3u, kQueueCount = 4u, kBoundsKeys = 8u /* 6 x 64 bits */, kHeaderWords = kHeaderBytes / 4u };

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

struct MeshParams {
    const uint8_t* buffer;
    uint32_t* header;
    const Prim* prims;
    uint32_t* counts;   // per vertex: corner count, then (scan) the segment's start, then (fill) its end
    uint32_t* sums;     // per scan tile
    uint32_t* corners;  // the segments
    uint32_t* queue;    // vertices with long segments
    float* normals;     // per triangle: 3 floats
    float* tangents;    // per triangle: 6 floats
    uint8_t* skips;     // per triangle: 1 when |det| < 1e-8
    float* vertices;
    uint32_t* indices;
    ur_mesh_info* info;
    uint32_t n, V, I, T;
};

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

// the last primitive whose first vertex / first index is not above `at`
template <bool BY_INDEX>
__device__ __forceinline__ uint32_t find_prim(const Prim* prims, uint32_t n, uint32_t at)
{
    uint32_t lo = 0u, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        const uint32_t first = BY_INDEX ? prims[mid].index_start : prims[mid].vertex_offset;
        if (first <= at) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kThreads) void mesh_clear_kernel(MeshParams p)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < kHeaderWords) {
        const bool min_key = i >= kBoundsKeys && i < kBoundsKeys + 6u;
        p.header[i] = min_key ? 0xFFFFFFFFu : 0u;
    } else if (i - kHeaderWords < p.V) {
        p.counts[i - kHeaderWords] = 0u;
    }
}

// monotonic in the float's value, -0 and +0 equal
__device__ __forceinline__ uint32_t ordered_bits(float f)
{
    uint32_t b = f == 0.0f ? 0u : __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ __launch_bounds__(kThreads) void mesh_assemble_kernel(MeshParams p)
{
    const uint64_t at = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const bool live = at < p.V;
    const uint32_t v = (uint32_t)at;
    bool normal_bad = false, tangent_bad = false;
    unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull};
    if (live) {
        const Prim& prim = p.prims[find_prim<false>(p.prims, p.n, v)];
        uint32_t w[16];
        assemble_vertex(p.buffer, prim.p, v - prim.vertex_offset, w);
        u32x4_t* out = reinterpret_cast<u32x4_t*>(p.vertices + 16u * (size_t)v);
        out[0] = u32x4_t{w[0], w[1], w[2], w[3]};
        out[1] = u32x4_t{w[4], w[5], w[6], w[7]};
        out[2] = u32x4_t{w[8], w[9], w[10], w[11]};
        out[3] = u32x4_t{w[12], w[13], w[14], w[15]};
        normal_bad = !normal_valid({as_float(w[3]), as_float(w[4]), as_float(w[5])});
        tangent_bad = !tangent_valid({as_float(w[8]), as_float(w[9]), as_float(w[10])});
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float f = as_float(w[k]);
            if (f == f) {
                const unsigned long long o = (unsigned long long)ordered_bits(f) << 32;
                lo[k] = o | v;
                hi[k] = o | (0xFFFFFFFFu - v);
            }
        }
    }
    const bool any_normal_bad = __ballot(normal_bad) != 0ull, any_tangent_bad = __ballot(tangent_bad) != 0ull;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int step = 1; step < 64; step <<= 1) {
            const unsigned long long a = __shfl_xor(lo[k], step), b = __shfl_xor(hi[k], step);
            lo[k] = a < lo[k] ? a : lo[k];
            hi[k] = b > hi[k] ? b : hi[k];
        }
    }
    if (lane_id() == 0u) {
        if (any_normal_bad) atomicOr(&p.header[kNormalsInvalid], 1u);
        if (any_tangent_bad) atomicOr(&p.header[kTangentsInvalid], 1u);
        unsigned long long* keys = reinterpret_cast<unsigned long long*>(p.header + kBoundsKeys);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (lo[k] != ~0ull) { atomicMin(&keys[k], lo[k]); atomicMax(&keys[3 + k], hi[k]); }
        }
    }
}

__device__ __forceinline__ F3 vertex_position(const float* vertices, uint32_t v)
{
    const float* at = vertices + 16u * (size_t)v;
    return {at[0], at[1], at[2]};
}

__global__ __launch_bounds__(kThreads) void mesh_triangles_kernel(MeshParams p)
{
    const uint64_t at = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const bool live = at < p.T;
    const uint32_t t = (uint32_t)at;
    const bool normals = p.header[kNormalsInvalid] != 0u, tangents = p.header[kTangentsInvalid] != 0u;
    bool outside = false, skipped = false;
    if (live) {
        const Prim& prim = p.prims[find_prim<true>(p.prims, p.n, 3u * t)];
        const uint32_t j = 3u * t - prim.index_start;
        uint32_t i[3];
#pragma unroll
        for (uint32_t c = 0u; c < 3u; ++c) {
            i[c] = raw_index(p.buffer, prim.p, raw_position(prim.p.mode, j + c)) + prim.vertex_offset;
            p.indices[3u * (size_t)t + c] = i[c];
        }
        outside = i[0] >= p.V || i[1] >= p.V || i[2] >= p.V;
        if (!outside && (normals || tangents)) {
            atomicAdd(&p.counts[i[0]], 1u);
            atomicAdd(&p.counts[i[1]], 1u);
            atomicAdd(&p.counts[i[2]], 1u);
            const F3 p0 = vertex_position(p.vertices, i[0]), p1 = vertex_position(p.vertices, i[1]), p2 = vertex_position(p.vertices, i[2]);
            if (normals) {
                const F3 face = face_normal(p0, p1, p2);
                float* out = p.normals + 3u * (size_t)t;
                out[0] = face.x; out[1] = face.y; out[2] = face.z;
            }
            if (tangents) {
                const float *a = p.vertices + 16u * (size_t)i[0] + 6u, *b = p.vertices + 16u * (size_t)i[1] + 6u, *c = p.vertices + 16u * (size_t)i[2] + 6u;
                F3 tangent, bitangent;
                skipped = !face_tangent(p0, p1, p2, a[0], a[1], b[0], b[1], c[0], c[1], tangent, bitangent);
                float* out = p.tangents + 6u * (size_t)t;
                out[0] = tangent.x; out[1] = tangent.y; out[2] = tangent.z;
                out[3] = bitangent.x; out[4] = bitangent.y; out[5] = bitangent.z;
                p.skips[t] = skipped ? 1u : 0u;
            }
        }
    }
    const uint32_t outside_count = (uint32_t)__popcll(__ballot(outside)), skipped_count = (uint32_t)__popcll(__ballot(skipped));
    if (lane_id() == 0u) {
        if (outside_count) atomicAdd(&p.header[kOutOfRange], outside_count);
        if (skipped_count) atomicAdd(&p.header[kSkipped], skipped_count);
    }
}

__device__ __forceinline__ bool any_pass(const MeshParams& p) { return (p.header[kNormalsInvalid] | p.header[kTangentsInvalid]) != 0u; }

// inclusive scan of one value per thread over the workgroup; `shared` holds kThreads words
__device__ __forceinline__ uint32_t block_inclusive_scan(uint32_t value, uint32_t* shared)
{
    shared[threadIdx.x] = value;
    __syncthreads();
    for (uint32_t step = 1u; step < kThreads; step <<= 1) {
        const uint32_t other = threadIdx.x >= step ? shared[threadIdx.x - step] : 0u;
        __syncthreads();
        shared[threadIdx.x] += other;
        __syncthreads();
    }
    return shared[threadIdx.x];
}

__global__ __launch_bounds__(kThreads) void mesh_scan_reduce_kernel(MeshParams p)
{
    __shared__ uint32_t shared[kThreads];
    if (!any_pass(p)) return;
    const uint64_t first = (uint64_t)blockIdx.x * kScanTile + 4u * threadIdx.x;
    uint32_t sum = 0u;
#pragma unroll
    for (uint32_t k = 0u; k < 4u; ++k) sum += first + k < p.V ? p.counts[first + k] : 0u;
    const uint32_t total = block_inclusive_scan(sum, shared);
    if (threadIdx.x == kThreads - 1u) p.sums[blockIdx.x] = total;
}

// one workgroup: the tile sums become their exclusive scan, 256 at a time with a carry
__global__ __launch_bounds__(kThreads) void mesh_scan_sums_kernel(MeshParams p, uint32_t tiles)
{
    __shared__ uint32_t shared[kThreads];
    if (!any_pass(p)) return;
    uint32_t carry = 0u;
    for (uint32_t base = 0u; base < tiles; base += kThreads) {
        const uint32_t at = base + threadIdx.x;
        const uint32_t value = at < tiles ? p.sums[at] : 0u;
        const uint32_t inclusive = block_inclusive_scan(value, shared);
        if (at < tiles) p.sums[at] = carry + inclusive - value;
        carry += shared[kThreads - 1u];
        __syncthreads(); // (the next round rewrites `shared`)
    }
}

__global__ __launch_bounds__(kThreads) void mesh_scan_add_kernel(MeshParams p)
{
    __shared__ uint32_t shared[kThreads];
    if (!any_pass(p)) return;
    const uint64_t first = (uint64_t)blockIdx.x * kScanTile + 4u * threadIdx.x;
    uint32_t count[4], sum = 0u;
#pragma unroll
    for (uint32_t k = 0u; k < 4u; ++k) { count[k] = first + k < p.V ? p.counts[first + k] : 0u; sum += count[k]; }
    uint32_t start = p.sums[blockIdx.x] + block_inclusive_scan(sum, shared) - sum;
#pragma unroll
    for (uint32_t k = 0u; k < 4u; ++k) {
        if (first + k < p.V) {
            p.counts[first + k] = start;
            if (count[k] > kLaneSegment) p.queue[atomicAdd(&p.header[kQueueCount], 1u)] = (uint32_t)(first + k);
        }
        start += count[k];
    }
}

__global__ __launch_bounds__(kThreads) void mesh_fill_kernel(MeshParams p)
{
    if (!any_pass(p)) return;
    const uint64_t at = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (at >= p.T) return;
    const uint32_t t = (uint32_t)at;
    const uint32_t i0 = p.indices[3u * (size_t)t], i1 = p.indices[3u * (size_t)t + 1u], i2 = p.indices[3u * (size_t)t + 2u];
    if (i0 >= p.V || i1 >= p.V || i2 >= p.V) return;
    p.corners[atomicAdd(&p.counts[i0], 1u)] = 3u * t;
    p.corners[atomicAdd(&p.counts[i1], 1u)] = 3u * t + 1u;
    p.corners[atomicAdd(&p.counts[i2], 1u)] = 3u * t + 2u;
}

// after the fill counts[v] is the end of segment v, and the end of segment v - 1 its start
__device__ __forceinline__ uint32_t segment_start(const MeshParams& p, uint32_t v) { return v ? p.counts[v - 1u] : 0u; }

__device__ __forceinline__ void compare_exchange(uint32_t* a, uint64_t i, uint64_t j)
{
    const uint32_t x = a[i], y = a[j];
    if (x > y) { a[i] = y; a[j] = x; }
}

// the strides from `from` down to 1 of one merge inside each kSortTile-aligned tile, in LDS; flip: the first of them is the merge's own
// first step (partner i ^ (size - 1)), which only happens when the whole merge fits a tile
__device__ void sort_tiles(uint32_t* seg, uint32_t k, uint32_t* tile, uint32_t first_size, uint32_t last_size)
{
    for (uint64_t base = 0u; base < k; base += kSortTile) {
        for (uint32_t i = threadIdx.x; i < kSortTile; i += kThreads) tile[i] = base + i < k ? seg[base + i] : 0xFFFFFFFFu;
        __syncthreads();
        for (uint32_t size = first_size; size <= last_size; size <<= 1) {
            const uint32_t half = size >> 1;
            if (size <= kSortTile) { // the flip step of a merge that fits the tile
                for (uint32_t q = threadIdx.x; q < kSortTile / 2u; q += kThreads) {
                    const uint32_t block = q / half, off = q - block * half;
                    compare_exchange(tile, block * size + off, block * size + size - 1u - off);
                }
                __syncthreads();
            }
            for (uint32_t stride = (size <= kSortTile ? half : kSortTile) >> 1; stride > 0u; stride >>= 1) {
                for (uint32_t q = threadIdx.x; q < kSortTile / 2u; q += kThreads) {
                    const uint32_t i = (q / stride) * 2u * stride + (q & (stride - 1u));
                    compare_exchange(tile, i, i + stride);
                }
                __syncthreads();
            }
        }
        for (uint32_t i = threadIdx.x; i < kSortTile; i += kThreads)
            if (base + i < k) seg[base + i] = tile[i];
        __syncthreads();
    }
}

// seg[0, k) ascending. The network is the bitonic sort in which every compare-exchange puts the smaller value at the lower index; the
// values behind k are a virtual padding of the largest value, which such a network never moves, so pairs that reach behind k are left out.
__device__ void sort_segment(uint32_t* seg, uint32_t k, uint32_t* tile)
{
    sort_tiles(seg, k, tile, 2u, kSortTile);
    for (uint64_t size = 2u * kSortTile; (size >> 1) < k; size <<= 1) {
        const uint64_t half = size >> 1, blocks = ((uint64_t)k + size - 1u) / size;
        for (uint64_t q = threadIdx.x; q < blocks * half; q += kThreads) { // the flip step
            const uint64_t block = q / half, off = q - block * half;
            const uint64_t i = block * size + off, j = block * size + size - 1u - off;
            if (j < k) compare_exchange(seg, i, j);
        }
        __threadfence_block();
        __syncthreads();
        for (uint64_t stride = half >> 1; stride >= kSortTile; stride >>= 1) {
            for (uint64_t q = threadIdx.x; q < blocks * half; q += kThreads) {
                const uint64_t i = (q / stride) * 2u * stride + (q & (stride - 1u));
                if (i + stride < k) compare_exchange(seg, i, i + stride);
            }
            __threadfence_block();
            __syncthreads();
        }
        // the strides below a tile: size > kSortTile, so sort_tiles runs strides kSortTile / 2 .. 1 and no flip
        sort_tiles(seg, k, tile, 2u * kSortTile, 2u * kSortTile);
    }
}

__global__ __launch_bounds__(kThreads) void mesh_sort_long_kernel(MeshParams p)
{
    __shared__ uint32_t tile[kSortTile];
    if (!any_pass(p)) return;
    const uint32_t queued = p.header[kQueueCount];
    for (uint32_t e = blockIdx.x; e < queued; e += gridDim.x) {
        const uint32_t v = p.queue[e], start = segment_start(p, v);
        sort_segment(p.corners + start, p.counts[v] - start, tile);
    }
}

struct Sums { F3 a, b; };

template <bool TANGENTS>
__device__ __forceinline__ void add_contribution(const MeshParams& p, uint32_t triangle, Sums& s)
{
    if constexpr (TANGENTS) {
        if (p.skips[triangle]) return;
        const float* c = p.tangents + 6u * (size_t)triangle;
        s.a = add(s.a, F3{c[0], c[1], c[2]});
        s.b = add(s.b, F3{c[3], c[4], c[5]});
    } else {
        const float* c = p.normals + 3u * (size_t)triangle;
        s.a = add(s.a, F3{c[0], c[1], c[2]});
    }
}

template <bool TANGENTS>
__device__ __forceinline__ void finish_vertex(const MeshParams& p, uint32_t v, const Sums& s)
{
    float* out = p.vertices + 16u * (size_t)v;
    if constexpr (TANGENTS) {
        const F4 t = finish_tangent(F3{out[3], out[4], out[5]}, s.a, s.b);
        *reinterpret_cast<u32x4_t*>(out + 8) = u32x4_t{__float_as_uint(t.x), __float_as_uint(t.y), __float_as_uint(t.z), __float_as_uint(t.w)};
    } else {
        const F3 n = finish_normal(s.a);
        out[3] = n.x; out[4] = n.y; out[5] = n.z;
    }
}

template <bool TANGENTS>
__global__ __launch_bounds__(kThreads) void mesh_sum_short_kernel(MeshParams p)
{
    if (p.header[TANGENTS ? kTangentsInvalid : kNormalsInvalid] == 0u) return;
    const uint64_t at = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (at >= p.V) return;
    const uint32_t v = (uint32_t)at, start = segment_start(p, v), end = p.counts[v];
    if (end - start > kLaneSegment) return; // the long kernel's
    Sums s = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
    uint32_t last = 0u;
    for (uint32_t taken = 0u; taken < end - start; ++taken) { // the next-greater corner: ascending corner order is triangle order
        uint32_t best = 0xFFFFFFFFu;
        for (uint32_t slot = start; slot < end; ++slot) {
            const uint32_t c = p.corners[slot];
            if ((taken == 0u || c > last) && c < best) best = c;
        }
        add_contribution<TANGENTS>(p, best / 3u, s);
        last = best;
    }
    finish_vertex<TANGENTS>(p, v, s);
}

template <bool TANGENTS>
__global__ __launch_bounds__(kThreads) void mesh_sum_long_kernel(MeshParams p)
{
    constexpr uint32_t kFloats = TANGENTS ? 6u : 3u;
    __shared__ float fetched[kThreads * kFloats];
    __shared__ uint8_t skip[kThreads];
    if (p.header[TANGENTS ? kTangentsInvalid : kNormalsInvalid] == 0u) return;
    const uint32_t queued = p.header[kQueueCount];
    for (uint32_t e = blockIdx.x; e < queued; e += gridDim.x) {
        const uint32_t v = p.queue[e], start = segment_start(p, v), k = p.counts[v] - start;
        Sums s = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
        for (uint32_t base = 0u; base < k; base += kThreads) {
            if (base + threadIdx.x < k) {
                const uint32_t triangle = p.corners[start + base + threadIdx.x] / 3u;
                const float* c = (TANGENTS ? p.tangents : p.normals) + kFloats * (size_t)triangle;
#pragma unroll
                for (uint32_t f = 0u; f < kFloats; ++f) fetched[kFloats * threadIdx.x + f] = c[f];
                skip[threadIdx.x] = TANGENTS ? p.skips[triangle] : 0u;
            }
            __syncthreads();
            if (threadIdx.x == 0u) {
                const uint32_t here = k - base < kThreads ? k - base : kThreads;
                for (uint32_t i = 0u; i < here; ++i) {
                    if (skip[i]) continue;
                    const float* c = fetched + kFloats * i;
                    s.a = add(s.a, F3{c[0], c[1], c[2]});
                    if constexpr (TANGENTS) s.b = add(s.b, F3{c[3], c[4], c[5]});
                }
            }
            __syncthreads();
        }
        if (threadIdx.x == 0u) finish_vertex<TANGENTS>(p, v, s);
    }
}

__global__ void mesh_info_kernel(MeshParams p)
{
    if (threadIdx.x != 0u || blockIdx.x != 0u) return;
    ur_mesh_info info;
    const unsigned long long* keys = reinterpret_cast<const unsigned long long*>(p.header + kBoundsKeys);
    for (int k = 0; k < 3; ++k) {
        const float first = p.vertices[k];
        const bool nan = first != first; // a coordinate is NaN iff vertex 0's is: its very bits
        info.min[k] = nan ? first : p.vertices[16u * (size_t)(uint32_t)keys[k] + k];
        info.max[k] = nan ? first : p.vertices[16u * (size_t)(0xFFFFFFFFu - (uint32_t)keys[3 + k]) + k];
    }
    finish_bounds(info);
    info.normals_regenerated = p.header[kNormalsInvalid];
    info.tangents_regenerated = p.header[kTangentsInvalid];
    info.skipped_determinant_triangles = p.header[kSkipped];
    info.out_of_range_triangles = p.header[kOutOfRange];
    *p.info = info;
}

uint32_t blocks_for(uint64_t items, uint32_t per_block) { return (uint32_t)((items + per_block - 1u) / per_block); }

} // namespace
} // namespace ur

extern "C" {

int ur_mesh_layout_of(const ur_mesh_primitive* primitives, uint32_t n, uint64_t buffer_size, ur_mesh_layout* out_layout, ur_mesh_section* sections)
{
    char text[256];
    if (!out_layout) { ur::set_error("ur_mesh_layout_of: null out_layout"); return UR_EINVAL; }
    if (ur_mesh::check_primitives("ur_mesh_layout_of", primitives, n, buffer_size, out_layout, nullptr, sections, text, sizeof text)) {
        ur::set_error("%s", text);
        return UR_EINVAL;
    }
    return UR_OK;
}

int ur_mesh_build(ur_ctx* ctx, const void* buffer, uint64_t buffer_size, const ur_mesh_primitive* primitives, uint32_t n, void* vertices, void* indices,
                  void* scratch, uint64_t scratch_bytes, ur_mesh_info* info)
{
    using namespace ur;
    if (!ctx || !buffer || !vertices || !indices || !scratch || !info) { set_error("ur_mesh_build: null context, buffer, vertices, indices, scratch or info"); return UR_EINVAL; }
    char text[256];
    ur_mesh_layout layout{};
    std::vector<Prim> prims(n ? n : 1u);
    if (check_primitives("ur_mesh_build", primitives, n, buffer_size, &layout, prims.data(), nullptr, text, sizeof text)) { set_error("%s", text); return UR_EINVAL; }
    if (reinterpret_cast<uintptr_t>(buffer) % 4u != 0u) { set_error("ur_mesh_build: buffer not 4-byte aligned"); return UR_EINVAL; }
    if (reinterpret_cast<uintptr_t>(vertices) % 16u != 0u) { set_error("ur_mesh_build: vertices not 16-byte aligned"); return UR_EINVAL; }
    if (reinterpret_cast<uintptr_t>(indices) % 4u != 0u || reinterpret_cast<uintptr_t>(info) % 4u != 0u) { set_error("ur_mesh_build: indices or info not 4-byte aligned"); return UR_EINVAL; }
    if (reinterpret_cast<uintptr_t>(scratch) % 16u != 0u) { set_error("ur_mesh_build: scratch not 16-byte aligned"); return UR_EINVAL; }
    if (scratch_bytes < layout.scratch_bytes) {
        set_error("ur_mesh_build: %llu scratch bytes, %llu needed (ur_mesh_layout_of)", (unsigned long long)scratch_bytes, (unsigned long long)layout.scratch_bytes);
        return UR_EINVAL;
    }
    const uint32_t V = layout.vertex_count, I = layout.index_count;
    const struct { const void* at; size_t bytes; const char* name; } parts[5] = {
        {vertices, 64u * (size_t)V, "vertices"}, {indices, 4u * (size_t)I, "indices"}, {scratch, (size_t)layout.scratch_bytes, "scratch"},
        {info, sizeof(ur_mesh_info), "info"}, {buffer, (size_t)buffer_size, "buffer"}};
    for (int a = 0; a < 4; ++a)
        for (int b = a + 1; b < 5; ++b)
            if (overlaps(parts[a].at, parts[a].bytes, parts[b].at, parts[b].bytes)) { set_error("ur_mesh_build: %s and %s overlap", parts[a].name, parts[b].name); return UR_EINVAL; }

    const Scratch s = scratch_layout(n, V, I);
    uint8_t* base = static_cast<uint8_t*>(scratch);
    MeshParams p{};
    p.buffer = static_cast<const uint8_t*>(buffer);
    p.header = reinterpret_cast<uint32_t*>(base);
    p.prims = reinterpret_cast<const Prim*>(base + s.table);
    p.counts = reinterpret_cast<uint32_t*>(base + s.counts);
    p.sums = reinterpret_cast<uint32_t*>(base + s.sums);
    p.corners = reinterpret_cast<uint32_t*>(base + s.corners);
    p.queue = reinterpret_cast<uint32_t*>(base + s.queue);
    p.normals = reinterpret_cast<float*>(base + s.normals);
    p.tangents = reinterpret_cast<float*>(base + s.tangents);
    p.skips = base + s.skips;
    p.vertices = static_cast<float*>(vertices);
    p.indices = static_cast<uint32_t*>(indices);
    p.info = info;
    p.n = n; p.V = V; p.I = I; p.T = I / 3u;

    // (pageable host memory: the runtime has copied the table into its staging memory when the call returns)
    UR_HIP_TRY(hipMemcpyAsync(base + s.table, prims.data(), (size_t)n * sizeof(Prim), hipMemcpyHostToDevice, ctx->stream));
    const uint32_t tiles = blocks_for(V, kScanTile), per_vertex = blocks_for(V, kThreads), per_triangle = blocks_for(p.T, kThreads);
    const uint32_t long_grid = (uint32_t)std::min<uint64_t>(kLongGrid, (uint64_t)I / (kLaneSegment + 1u) + 1u);
    hipLaunchKernelGGL(mesh_clear_kernel, dim3(blocks_for((uint64_t)V + kHeaderWords, kThreads)), dim3(kThreads), 0, ctx->stream, p);
    hipLaunchKernelGGL(mesh_assemble_kernel, dim3(per_vertex), dim3(kThreads), 0, ctx->stream, p);
    hipLaunchKernelGGL(mesh_triangles_kernel, dim3(per_triangle), dim3(kThreads), 0, ctx->stream, p);
    hipLaunchKernelGGL(mesh_scan_reduce_kernel, dim3(tiles), dim3(kThreads), 0, ctx->stream, p);
    hipLaunchKernelGGL(mesh_scan_sums_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, p, tiles);
    hipLaunchKernelGGL(mesh_scan_add_kernel, dim3(tiles), dim3(kThreads), 0, ctx->stream, p);
    hipLaunchKernelGGL(mesh_fill_kernel, dim3(per_triangle), dim3(kThreads), 0, ctx->stream, p);
    hipLaunchKernelGGL(mesh_sort_long_kernel, dim3(long_grid), dim3(kThreads), 0, ctx->stream, p);
    hipLaunchKernelGGL(mesh_sum_short_kernel<false>, dim3(per_vertex), dim3(kThreads), 0, ctx->stream, p);
    hipLaunchKernelGGL(mesh_sum_long_kernel<false>, dim3(long_grid), dim3(kThreads), 0, ctx->stream, p);
    hipLaunchKernelGGL(mesh_sum_short_kernel<true>, dim3(per_vertex), dim3(kThreads), 0, ctx->stream, p);
    hipLaunchKernelGGL(mesh_sum_long_kernel<true>, dim3(long_grid), dim3(kThreads), 0, ctx->stream, p);
    hipLaunchKernelGGL(mesh_info_kernel, dim3(1), dim3(64), 0, ctx->stream, p);
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

} // extern "C"
