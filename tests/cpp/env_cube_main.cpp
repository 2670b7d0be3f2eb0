// A stand-alone program over the environment cube build's host code, for the compiler's sanitizers: no Python,
// no device. Built with csrc/env_cube_host.cpp, csrc/env_cube_stage.cpp and csrc/lighting_plan.cpp by tests/test_env_cube_abi.py.
//   env_cube_main rule           the integer border rule of csrc/env_cube_rule.h against ur_stage_env_cube's own (in doubles), through
//                                ur::stage_env_cube_host over cubes whose texels carry their own (face, i, j): every edge 1..64, and 256
//   env_cube_main build FILE     FILE = { u32 format, base, mips, 0; the payload }: ur_host_env_cube_build into heap buffers of exactly
//                                their sizes; then the three launches of csrc/env_cube_build.hip as the device runs them - the items of
//                                csrc/env_cube_rule.h, each launch's in turn, descending, into a destination that arrives as 0xFF - which
//                                must give the same bytes. Prints "rc sum reserved" (sum: of the destination's bytes).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/ur_host.h"
#include "../../unclerenderer_amd/csrc/env_cube_rule.h"

static void* aligned(size_t bytes)
{
    void* p = nullptr;
    if (posix_memalign(&p, 16, bytes ? bytes : 1) != 0) exit(2);
    return p;
}

static int rule()
{
    for (int N = 1; N <= 256; N = N == 64 ? 256 : N + 1) {
        const ur::CubeLayout L = ur::cube_layout((uint32_t)N, 1);
        std::vector<ur_half4> src((size_t)6 * N * N), out((size_t)L.texels);
        for (int f = 0; f < 6; ++f)
            for (int j = 0; j < N; ++j)
                for (int i = 0; i < N; ++i) src[((size_t)f * N + j) * N + i] = ur_half4{(uint16_t)f, (uint16_t)i, (uint16_t)j, 0x3C00};
        ur::stage_env_cube_host(src.data(), L, out.data());
        const int E = N + 2;
        for (int f = 0; f < 6; ++f)
            for (int j = -1; j <= N; ++j)
                for (int i = -1; i <= N; ++i) {
                    const ur_half4 t = out[((size_t)f * E + (j + 1)) * E + (i + 1)];
                    const bool ring = i < 0 || i >= N || j < 0 || j >= N;
                    const ur_envc::Texel s = ring ? ur_envc::border_source(N, f, i, j) : ur_envc::Texel{f, i, j};
                    if (t.x != s.face || t.y != s.i || t.z != s.j) {
                        printf("edge %d face %d (%d, %d): staged from (%d; %d, %d), the integer rule says (%d; %d, %d)\n", N, f, i, j, t.x, t.y, t.z, s.face, s.i, s.j);
                        return 1;
                    }
                }
    }
    printf("rule ok\n");
    return 0;
}

static int build(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    unsigned h[4];
    if (fread(h, 4, 4, f) != 4) return 2;
    const uint32_t format = h[0], base = h[1], mips = h[2];
    const size_t src_bytes = ur_env_cube_source_bytes(format, base, mips), texels = (size_t)ur::cube_layout(base, mips).texels;
    void* src = aligned(src_bytes);
    if (fread(src, 1, src_bytes, f) != src_bytes) return 2;
    fclose(f);
    ur_half4* want = (ur_half4*)aligned(texels * 8);
    uint64_t* got = (uint64_t*)aligned(texels * 8);
    memset(want, 0, texels * 8);
    memset(got, 0xFF, texels * 8);
    uint32_t reserved = ~0u;
    const int rc = ur_host_env_cube_build(src, src_bytes, format, base, mips, want, texels, &reserved);
    if (rc != 0) { printf("%d 0 0\n", rc); return 1; }
    // the device's three launches, on the host; within a launch in descending order: no item may depend on another of its launch
    const ur_envc::Plan p = ur_envc::make_plan(format, base, mips);
    for (uint32_t item = 6u * p.decode_face; item-- > 0u;) ur_envc::decode_item(p, src, got, item, ur_envc::is_bc6h(format), format == ur_envc::kSF16, &ur_bc6h::kTables);
    for (uint32_t item = 6u * p.border_face; item-- > 0u;) ur_envc::border_item(p, got, item);
    for (uint32_t item = 6u * p.pair_face; item-- > 0u;) ur_envc::pair_item(p, got, item);
    uint32_t counted = 0u;
    for (uint32_t b = 0u; b < p.total_blocks; ++b) counted += ur_bc6h::reserved_mode(static_cast<const uint8_t*>(src)[16u * (size_t)b]) ? 1u : 0u;
    if (memcmp(want, got, texels * 8) != 0 || counted != reserved) {
        size_t at = 0;
        while (at < texels * 8 && ((const uint8_t*)want)[at] == ((const uint8_t*)got)[at]) ++at;
        printf("the items differ from the host build: first at byte %zu of %zu; reserved %u against %u\n", at, texels * 8, counted, reserved);
        return 1;
    }
    unsigned long long sum = 0;
    for (size_t i = 0; i < texels * 8; ++i) sum += ((const uint8_t*)want)[i];
    printf("%d %llu %u\n", rc, sum, reserved);
    free(src); free(want); free(got);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && strcmp(argv[1], "rule") == 0) return rule();
    if (argc == 3 && strcmp(argv[1], "build") == 0) return build(argv[2]);
    return 2;
}
