// ur_scene_build (include/ur_scene_build.h): built meshes and tables of transforms, factors and draws become the
// bounds, command slots and constants records of the cull and the raster passes, on the device, by the rule of csrc/scene_rule.h, the
// file the serial host build (csrc/scene_host.cpp) runs.
//
// The arithmetic of a draw is small; the cost is what it writes: 32 bytes of bounds, 16 of centre, a 64-byte command and a 608-byte
// constants record behind a slot number, 720 bytes. A lane that wrote its own record would put 64 lanes on 64 records with every
// store. So a workgroup is one wave and its 64 draws, in two halves:
//   compute   lane l places draw 64 * block + l and leaves World, the command, the bounds and (record offset, ObjectId, material) in LDS;
//             the centre, 16 bytes a lane in command order, goes out as it is
//   write     the wave walks the 64 records in 16-byte pieces, lane after lane: piece q of the walk is piece q % 38 of draw q / 38, so a
//             store instruction covers 1 KiB of consecutive record bytes (broken only where a record ends), whatever the slots are.
//             Pieces 0-3 are World from LDS; a piece behind them is the template's (38 pieces in LDS, read from the kernel arguments
//             once) with the material's fields put in, from the draws' factor records, which the wave has gathered into LDS 11 pieces
//             a draw. Commands and bounds are contiguous in command order and leave LDS the same way.
// The scene box: every lane folds its centre +- radius into order-preserving integer images, the wave reduces them, lane 0 writes the
// workgroup's partial (32 bytes of the scratch); the finish launch, one workgroup, reduces the partials and one lane runs the rule's
// finish. Every partial it reads was written by the launch in front of it: nothing of the scratch needs to arrive cleared. No atomics.
// Vector stores only.

#include <cstddef>

#include "scene_rule.h"
#include "ur_internal.h"

namespace ur {
namespace {

using namespace ur_scene;

constexpr uint32_t kWave = 64u, kFinishThreads = 1024u, kPartialWords = 8u; // a partial: lo[3], hi[3], skipped draws, 0
constexpr uint32_t kSkipped = 0xFFFFFFFFu;                                  // in the material word of a draw's LDS record

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

struct SceneParams {
    ur_scene_constants frame; // first: the kernel reads its pieces from the head of the kernel-argument segment
    ur_scene_build_tables t;
    ur_scene_build_outputs o;
    uint32_t* partials;
};
static_assert(offsetof(SceneParams, frame) == 0, "the template is read from the head of the kernel arguments");

__device__ __forceinline__ u32x4_t float4_bits(float x, float y, float z, float w) { return u32x4_t{__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), __float_as_uint(w)}; }

__device__ __forceinline__ ur_scene_node load_node(const ur_scene_node* at)
{
    const u32x4_t* src = reinterpret_cast<const u32x4_t*>(at);
    u32x4_t q[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) q[k] = src[k];
    ur_scene_node n;
    __builtin_memcpy(&n, q, sizeof n);
    return n;
}

template <bool FULL>
__global__ __launch_bounds__(kWave) void scene_build_kernel(SceneParams p)
{
    constexpr uint32_t kPieces = FULL ? kConstantsPieces : 4u; // of a record, written
    __shared__ u32x4_t s_template[kConstantsPieces];
    __shared__ u32x4_t s_world[kWave * 4u];
    __shared__ u32x4_t s_command[kWave * 4u];
    __shared__ u32x4_t s_bounds[kWave * 2u];
    __shared__ u32x4_t s_record[kWave]; // the record's byte offset (two words), ObjectId, material or kSkipped
    __shared__ u32x4_t s_factors[FULL ? kWave * kFactorPieces : 1u];

    const uint32_t lane = threadIdx.x, first = blockIdx.x * kWave, D = p.t.draw_count;
    const uint32_t here = D - first < kWave ? D - first : kWave;
    if (FULL && lane < kConstantsPieces)
        s_template[lane] = ((const __attribute__((address_space(4))) u32x4_t*)__builtin_amdgcn_kernarg_segment_ptr())[lane];

    Box box = empty_box();
    bool skipped = false;
    if (lane < here) {
        const uint32_t i = first + lane;
        const u32x4_t* dq = reinterpret_cast<const u32x4_t*>(p.t.draws + i);
        const u32x4_t d0 = dq[0], d1 = dq[1];
        const ur_scene_draw d = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
        const u32x4_t zero = {0u, 0u, 0u, 0u};
        u32x4_t center = zero;
        skipped = !draw_in_range(d, p.t.node_count, p.t.mesh_count, p.t.material_count, p.o.slot_count);
        if (!skipped) {
            const ur_scene_node n = load_node(p.t.nodes + d.node);
            const ur_mesh_info info = p.t.mesh_infos[d.mesh];
            const Placed pl = place(n, info);
#pragma unroll
            for (int r = 0; r < 4; ++r) s_world[lane * 4u + r] = float4_bits(pl.world.m[r][0], pl.world.m[r][1], pl.world.m[r][2], pl.world.m[r][3]);
            s_bounds[lane * 2u] = float4_bits(pl.bounds_min[0], pl.bounds_min[1], pl.bounds_min[2], 0.0f);
            s_bounds[lane * 2u + 1u] = float4_bits(pl.bounds_max[0], pl.bounds_max[1], pl.bounds_max[2], 0.0f);
            center = float4_bits(pl.center[0], pl.center[1], pl.center[2], pl.radius);
            box_add(box, pl.center, pl.radius);
            const uint64_t offset = (uint64_t)d.constants_slot * p.o.constants_stride;
            s_record[lane] = u32x4_t{(uint32_t)offset, (uint32_t)(offset >> 32), d.object_id, d.material};
            if (FULL) {
                const u32x4_t* mq = reinterpret_cast<const u32x4_t*>(p.t.meshes + d.mesh);
                const u32x4_t m0 = mq[0], m1 = mq[1];
                const ur_scene_mesh mesh = {(uint64_t)m0.x | ((uint64_t)m0.y << 32), (uint64_t)m0.z | ((uint64_t)m0.w << 32), m1.x, m1.y, m1.z, m1.w};
                uint32_t w[16];
                command_words(mesh, d, reinterpret_cast<uint64_t>(p.o.constants) + offset, w);
#pragma unroll
                for (int k = 0; k < 4; ++k) s_command[lane * 4u + k] = u32x4_t{w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]};
            }
        } else {
            s_bounds[lane * 2u] = zero;
            s_bounds[lane * 2u + 1u] = zero;
            s_record[lane] = u32x4_t{0u, 0u, 0u, kSkipped};
            if (FULL) {
#pragma unroll
                for (int k = 0; k < 4; ++k) s_command[lane * 4u + k] = zero;
            }
        }
        if (p.o.centers) reinterpret_cast<u32x4_t*>(p.o.centers)[i] = center;
    }
    __syncthreads();

    if (FULL) { // the draws' factor records, 11 pieces each, lane after lane
        const u32x4_t* factors = reinterpret_cast<const u32x4_t*>(p.t.materials);
        for (uint32_t q = lane; q < kWave * kFactorPieces; q += kWave) {
            const uint32_t draw = q / kFactorPieces, piece = q - draw * kFactorPieces;
            if (draw < here) {
                const uint32_t material = s_record[draw].w;
                if (material != kSkipped) s_factors[q] = factors[(size_t)material * kFactorPieces + piece];
            }
        }
        u32x4_t* commands = reinterpret_cast<u32x4_t*>(p.o.commands) + 4u * (size_t)first;
        for (uint32_t q = lane; q < kWave * 4u; q += kWave)
            if ((q >> 2) < here) commands[q] = s_command[q];
    }
    u32x4_t* bounds = reinterpret_cast<u32x4_t*>(p.o.bounds) + 2u * (size_t)first;
    for (uint32_t q = lane; q < kWave * 2u; q += kWave)
        if ((q >> 1) < here) bounds[q] = s_bounds[q];
    __syncthreads();

    uint8_t* constants = static_cast<uint8_t*>(p.o.constants);
    for (uint32_t q = lane; q < kWave * kPieces; q += kWave) {
        const uint32_t draw = q / kPieces, piece = q - draw * kPieces;
        if (draw >= here) break; // (q ascends with the lane and the round: every later piece of this lane is behind the last draw too)
        const u32x4_t record = s_record[draw];
        if (record.w == kSkipped) continue;
        u32x4_t value;
        if (!FULL || piece < 4u) {
            value = s_world[draw * 4u + piece];
        } else {
            const u32x4_t t = s_template[piece];
            const uint32_t tw[4] = {t.x, t.y, t.z, t.w};
            uint32_t w[4];
            constants_piece(piece, tw, reinterpret_cast<const uint32_t*>(&s_factors[FULL ? draw * kFactorPieces : 0u]), record.z, w);
            value = u32x4_t{w[0], w[1], w[2], w[3]};
        }
        const uint64_t offset = (uint64_t)record.x | ((uint64_t)record.y << 32);
        *reinterpret_cast<u32x4_t*>(constants + offset + 16u * piece) = value;
    }

    // the wave's box and its count of skipped draws
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int step = 1; step < 64; step <<= 1) {
            const uint32_t lo = __shfl_xor(box.lo[a], step), hi = __shfl_xor(box.hi[a], step);
            box.lo[a] = lo < box.lo[a] ? lo : box.lo[a];
            box.hi[a] = hi > box.hi[a] ? hi : box.hi[a];
        }
    }
    const uint32_t skipped_count = (uint32_t)__popcll(__ballot(skipped));
    if (lane == 0u) {
        u32x4_t* out = reinterpret_cast<u32x4_t*>(p.partials + (size_t)blockIdx.x * kPartialWords);
        out[0] = u32x4_t{box.lo[0], box.lo[1], box.lo[2], box.hi[0]};
        out[1] = u32x4_t{box.hi[1], box.hi[2], skipped_count, 0u};
    }
}

__global__ __launch_bounds__(kFinishThreads) void scene_finish_kernel(const uint32_t* partials, uint32_t blocks, uint32_t draw_count, ur_scene_build_summary* summary)
{
    __shared__ uint32_t s_part[kFinishThreads / kWave][kPartialWords];
    Box box = empty_box();
    uint32_t skipped = 0u;
    for (uint32_t b = threadIdx.x; b < blocks; b += kFinishThreads) {
        const u32x4_t* in = reinterpret_cast<const u32x4_t*>(partials + (size_t)b * kPartialWords);
        const u32x4_t a = in[0], c = in[1];
        const uint32_t lo[3] = {a.x, a.y, a.z}, hi[3] = {a.w, c.x, c.y};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            box.lo[k] = lo[k] < box.lo[k] ? lo[k] : box.lo[k];
            box.hi[k] = hi[k] > box.hi[k] ? hi[k] : box.hi[k];
        }
        skipped += c.z;
    }
#pragma unroll
    for (int step = 1; step < 64; step <<= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t lo = __shfl_xor(box.lo[k], step), hi = __shfl_xor(box.hi[k], step);
            box.lo[k] = lo < box.lo[k] ? lo : box.lo[k];
            box.hi[k] = hi > box.hi[k] ? hi : box.hi[k];
        }
        skipped += __shfl_xor(skipped, step);
    }
    const uint32_t wave = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1u)) == 0u) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { s_part[wave][k] = box.lo[k]; s_part[wave][3 + k] = box.hi[k]; }
        s_part[wave][6] = skipped;
    }
    __syncthreads();
    if (threadIdx.x != 0u) return;
    for (uint32_t w = 1u; w < kFinishThreads / kWave; ++w) {
        for (int k = 0; k < 3; ++k) {
            box.lo[k] = s_part[w][k] < box.lo[k] ? s_part[w][k] : box.lo[k];
            box.hi[k] = s_part[w][3 + k] > box.hi[k] ? s_part[w][3 + k] : box.hi[k];
        }
        skipped += s_part[w][6];
    }
    ur_scene_build_summary s;
    finish_summary(box, draw_count, skipped, s);
    u32x4_t* out = reinterpret_cast<u32x4_t*>(summary);
    out[0] = float4_bits(s.scene_min[0], s.scene_min[1], s.scene_min[2], s.scene_max[0]);
    out[1] = float4_bits(s.scene_max[1], s.scene_max[2], s.scene_center[0], s.scene_center[1]);
    out[2] = u32x4_t{__float_as_uint(s.scene_center[2]), __float_as_uint(s.scene_radius), s.draw_count, s.skipped_draws};
}

uint32_t scene_blocks(uint32_t draw_count) { return (draw_count + kWave - 1u) / kWave; }

} // namespace
} // namespace ur

extern "C" {

uint64_t ur_scene_build_scratch_bytes(uint32_t draw_count)
{
    if (draw_count == 0u || draw_count >= UR_SCENE_BUILD_MAX_DRAWS) return 0u;
    return (uint64_t)ur::scene_blocks(draw_count) * ur::kPartialWords * 4u;
}

int ur_scene_build(ur_ctx* ctx, const ur_scene_build_tables* tables, const ur_scene_constants* frame, const ur_scene_build_outputs* outputs, void* scratch,
                   uint64_t scratch_bytes, uint32_t flags)
{
    using namespace ur;
    if (!ctx || !scratch) { set_error("ur_scene_build: null context or scratch"); return UR_EINVAL; }
    char text[256];
    if (ur_scene::check_tables("ur_scene_build", tables, frame, outputs, flags, text, sizeof text)) { set_error("%s", text); return UR_EINVAL; }
    const ur_scene_build_tables& t = *tables;
    const ur_scene_build_outputs& o = *outputs;
    const uint64_t need = ur_scene_build_scratch_bytes(t.draw_count);
    const size_t D = t.draw_count;
    struct Part { const void* at; size_t bytes; const char* name; };
    const Part parts[11] = {{o.bounds, 32u * D, "bounds"},
                            {o.commands, 64u * D, "commands"},
                            {o.constants, (size_t)o.slot_count * o.constants_stride, "constants"},
                            {o.centers, 16u * D, "centers"},
                            {o.summary, sizeof(ur_scene_build_summary), "summary"},
                            {scratch, (size_t)need, "scratch"},
                            {t.nodes, sizeof(ur_scene_node) * (size_t)t.node_count, "nodes"},
                            {t.meshes, sizeof(ur_scene_mesh) * (size_t)t.mesh_count, "meshes"},
                            {t.mesh_infos, sizeof(ur_mesh_info) * (size_t)t.mesh_count, "mesh_infos"},
                            {t.materials, sizeof(ur_scene_material_factors) * (size_t)t.material_count, "materials"},
                            {t.draws, sizeof(ur_scene_draw) * D, "draws"}};
    for (const Part& part : parts)
        if (reinterpret_cast<uintptr_t>(part.at) % 16u != 0u) { set_error("ur_scene_build: %s not 16-byte aligned", part.name); return UR_EINVAL; }
    if (scratch_bytes < need) {
        set_error("ur_scene_build: %llu scratch bytes, %llu needed (ur_scene_build_scratch_bytes)", (unsigned long long)scratch_bytes, (unsigned long long)need);
        return UR_EINVAL;
    }
    for (int a = 0; a < 6; ++a) // an output or the scratch against everything behind it; the tables are only read and may share bytes
        for (int b = a + 1; b < 11; ++b)
            if (parts[a].at && parts[b].at && overlaps(parts[a].at, parts[a].bytes, parts[b].at, parts[b].bytes)) {
                set_error("ur_scene_build: %s and %s overlap", parts[a].name, parts[b].name);
                return UR_EINVAL;
            }

    SceneParams p;
    p.frame = *frame;
    p.t = t;
    p.o = o;
    p.partials = static_cast<uint32_t*>(scratch);
    const uint32_t blocks = scene_blocks(t.draw_count);
    if (flags & UR_SCENE_BUILD_TRANSFORMS_ONLY)
        hipLaunchKernelGGL(scene_build_kernel<false>, dim3(blocks), dim3(kWave), 0, ctx->stream, p);
    else
        hipLaunchKernelGGL(scene_build_kernel<true>, dim3(blocks), dim3(kWave), 0, ctx->stream, p);
    hipLaunchKernelGGL(scene_finish_kernel, dim3(1), dim3(kFinishThreads), 0, ctx->stream, p.partials, blocks, t.draw_count, o.summary);
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

} // extern "C"
