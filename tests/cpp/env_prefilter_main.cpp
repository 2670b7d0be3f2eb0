// A stand-alone program over the environment prefilter's host code, for the compiler's sanitizers: no Python, no
// device. Built with csrc/env_prefilter_host.cpp, csrc/env_cube_host.cpp, csrc/env_cube_stage.cpp and csrc/lighting_plan.cpp by
// tests/test_env_prefilter_abi.py.
//   env_prefilter_main layout      the closed forms of csrc/cube_sample.h and csrc/env_prefilter_rule.h (where a level starts in the payload and
//                                  in the bordered section, the sizes) against ur::cube_layout and ur_env_cube_source_bytes for every base
//                                  1 .. 2048; the fp16 conversions over all 65536 halves and at every rounding boundary between them
//   env_prefilter_main build FILE  FILE = { u32 base, samples, 0, 0; the source's 6 * base^2 * 8 bytes }: the table and
//                                  ur_host_env_prefilter into heap buffers of exactly their sizes; then the launches of
//                                  csrc/env_prefilter.hip as the device runs them - the items of the rule, each launch's in turn,
//                                  descending, into a destination and a scratch that arrive as 0xFF and of exactly their sizes - which
//                                  must give the same bytes. Prints "rc sum" (sum: of the destination's bytes).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/ur_host.h"
#include "../../unclerenderer_amd/csrc/env_prefilter_rule.h"

static void* aligned(size_t bytes)
{
    void* p = nullptr;
    if (posix_memalign(&p, 16, bytes ? bytes : 1) != 0) exit(2);
    return p;
}

static int layout()
{
    for (uint32_t base = 1u; base <= ur_envp::kMaxBase; base *= 2u) {
        const uint32_t L = ur_envp::levels_of(base);
        const ur::CubeLayout c = ur::cube_layout(base, L);
        uint32_t texels = 0u;
        for (uint32_t m = 0u; m < L; ++m) {
            if (c.bordered[m] != ur_cube::bordered_start(base, m) || texels != ur_envp::level_start(base, m) || c.size(m) != (base >> m)) {
                printf("base %u level %u: bordered %llu against %u, payload %u against %u\n", base, m, (unsigned long long)c.bordered[m],
                       ur_cube::bordered_start(base, m), texels, ur_envp::level_start(base, m));
                return 1;
            }
            texels += (base >> m) * (base >> m);
        }
        if (texels != ur_envp::face_texels_of(base) || ur_envp::payload_bytes(base) != ur_env_cube_source_bytes(UR_ENV_SOURCE_RGBA16F, base, L) ||
            ur_envp::staged_bytes(base) != (size_t)c.pairs[0] || ur_env_prefilter_scratch_bytes(base) != ur_envp::payload_bytes(base) + (size_t)c.pairs[0]) {
            printf("base %u: sizes\n", base);
            return 1;
        }
    }
    for (uint32_t h = 0u; h < 65536u; ++h) {
        const float v = ur_cube::half_value(h);
        if ((h & 0x7C00u) == 0x7C00u && (h & 0x3FFu) != 0u) continue; // NaN
        if (ur_cube::half_bits(v) != h) { printf("half %04x does not come back\n", h); return 1; }
        const uint32_t next = h + 1u;
        if ((h & 0x7FFFu) >= 0x7BFFu) continue; // the largest finite half: the boundary to infinity is 65520, below
        // between two neighbours the midpoint goes to the even one, a float on either side of it to the nearer
        const float w = ur_cube::half_value(next), mid = 0.5f * v + 0.5f * w; // exact: both have at most 11 significant bits
        const uint32_t even = (h & 1u) ? next : h;
        if (ur_cube::half_bits(mid) != even || ur_cube::half_bits(nextafterf(mid, v)) != h || ur_cube::half_bits(nextafterf(mid, w)) != next) {
            printf("rounding between %04x and %04x\n", h, next);
            return 1;
        }
    }
    if (ur_cube::half_bits(65519.996f) != 0x7BFFu || ur_cube::half_bits(65520.0f) != 0x7C00u || ur_cube::half_bits(-65520.0f) != 0xFC00u) { printf("overflow\n"); return 1; }
    printf("layout ok\n");
    return 0;
}

static int build(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    unsigned h[4];
    if (fread(h, 4, 4, f) != 4) return 2;
    const uint32_t base = h[0], samples = h[1];
    const size_t src_bytes = 48u * (size_t)base * base, table_bytes = ur_env_prefilter_table_bytes(base, samples);
    const size_t dst_bytes = ur_envp::payload_bytes(base), staged_bytes = ur_envp::staged_bytes(base);
    void* src = aligned(src_bytes);
    if (fread(src, 1, src_bytes, f) != src_bytes) return 2;
    fclose(f);
    void* table = aligned(table_bytes);
    uint64_t* want = (uint64_t*)aligned(dst_bytes);
    uint64_t* got = (uint64_t*)aligned(dst_bytes);
    uint64_t* pyramid = (uint64_t*)aligned(dst_bytes);
    uint64_t* staged = (uint64_t*)aligned(staged_bytes);
    memset(want, 0, dst_bytes);
    memset(got, 0xFF, dst_bytes);
    memset(pyramid, 0xFF, dst_bytes);
    memset(staged, 0xFF, staged_bytes);
    int rc = ur_host_env_prefilter_table(base, samples, table, table_bytes);
    if (rc == 0) rc = ur_host_env_prefilter(src, src_bytes, base, samples, table, table_bytes, want, dst_bytes);
    if (rc != 0) { printf("%d 0\n", rc); return 1; }
    // the device's launches, on the host; within a launch in descending order: no item may depend on another of its launch
    const ur_envp::Plan p = ur_envp::make_plan(base, samples);
    for (uint32_t item = 6u * base * base; item-- > 0u;) ur_envp::top_item(p, (const uint64_t*)src, got, pyramid, item);
    for (uint32_t m = 1u; m < p.levels; ++m)
        for (uint32_t item = 6u * (base >> m) * (base >> m); item-- > 0u;) ur_envp::down_item(p, pyramid, m, item);
    if (p.levels > 1u) {
        const ur_envc::Plan stage = ur_envc::make_plan(ur_envc::kRGBA16F, base, p.levels);
        for (uint32_t item = 6u * stage.decode_face; item-- > 0u;) ur_envc::decode_item(stage, pyramid, staged, item, false, false, nullptr);
        for (uint32_t item = 6u * stage.border_face; item-- > 0u;) ur_envc::border_item(stage, staged, item);
        // the filter's groups as the kernel deals them: a group's level by the plan, its texels bounded by the level's count
        for (uint32_t group = p.groups; group-- > 0u;) {
            const uint32_t k = ur_envc::level_of(p.group_start, group), n = base >> k;
            for (uint32_t w = ur_envp::kGroupTexels; w-- > 0u;) {
                const uint32_t t = (group - ur_envc::at32(p.group_start, k)) * ur_envp::kGroupTexels + w;
                if (t < 6u * n * n) ur_envp::filter_item(p, staged, table, got, k, t);
            }
        }
    }
    if (memcmp(want, got, dst_bytes) != 0) {
        size_t at = 0;
        while (at < dst_bytes && ((const uint8_t*)want)[at] == ((const uint8_t*)got)[at]) ++at;
        printf("the items differ from the host build: first at byte %zu of %zu\n", at, dst_bytes);
        return 1;
    }
    unsigned long long sum = 0;
    for (size_t i = 0; i < dst_bytes; ++i) sum += ((const uint8_t*)want)[i];
    printf("%d %llu\n", rc, sum);
    free(src); free(table); free(want); free(got); free(pyramid); free(staged);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && strcmp(argv[1], "layout") == 0) return layout();
    if (argc == 3 && strcmp(argv[1], "build") == 0) return build(argv[2]);
    return 2;
}
