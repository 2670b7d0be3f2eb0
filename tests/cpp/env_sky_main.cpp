// A stand-alone program over the host code of the sky capture and the BRDF LUT, for the compiler's sanitizers: no
// Python, no device. Built with csrc/env_sky_host.cpp and csrc/brdf_lut_host.cpp by tests/test_env_sky_abi.py.
//   env_sky_main sky BASE TAPS CAMERA_Y DX DY DZ R G B   ur_host_env_sky into a heap buffer of exactly the cube's size; then the launch of
//                                  csrc/env_sky.hip as the device runs it - the waves of the rule, descending, whole workgroups - into a
//                                  destination that arrives as 0xFF, which must give the same bytes. Prints "rc sum" (sum: of the
//                                  destination's bytes).
//   env_sky_main lut W H S         ur_host_brdf_lut_table into a heap buffer of exactly ur_brdf_lut_table_bytes, ur_host_brdf_lut into
//                                  one of exactly 4 W H bytes; then the launch of csrc/brdf_lut.hip - a wave a texel, descending - into a
//                                  destination that arrives as 0xFF: the same bytes. Prints "rc sum".
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/ur_host.h"
#include "../../unclerenderer_amd/csrc/brdf_lut_rule.h"
#include "../../unclerenderer_amd/csrc/env_sky_rule.h"

static void* aligned(size_t bytes)
{
    void* p = nullptr;
    if (posix_memalign(&p, 16, bytes ? bytes : 1) != 0) exit(2);
    return p;
}

static int differ(const void* want, const void* got, size_t bytes)
{
    if (memcmp(want, got, bytes) == 0) return 0;
    size_t at = 0;
    while (at < bytes && ((const uint8_t*)want)[at] == ((const uint8_t*)got)[at]) ++at;
    printf("the waves differ from the host build: first at byte %zu of %zu\n", at, bytes);
    return 1;
}

static unsigned long long sum_of(const void* p, size_t bytes)
{
    unsigned long long sum = 0;
    for (size_t i = 0; i < bytes; ++i) sum += ((const uint8_t*)p)[i];
    return sum;
}

static int sky(char** a)
{
    const uint32_t base = (uint32_t)atoi(a[0]), taps = (uint32_t)atoi(a[1]);
    ur_sky_constants k;
    memset(&k, 0, sizeof k);
    k.CameraPosition[1] = (float)atof(a[2]);
    for (int c = 0; c < 3; ++c) { k.LightDirection[c] = (float)atof(a[3 + c]); k.LightColor[c] = (float)atof(a[6 + c]); }
    const size_t bytes = 48u * (size_t)base * base;
    uint64_t* want = (uint64_t*)aligned(bytes);
    uint64_t* got = (uint64_t*)aligned(bytes);
    memset(want, 0, bytes);
    memset(got, 0xFF, bytes);
    const int rc = ur_host_env_sky(&k, base, taps, want, bytes);
    if (rc != 0) { printf("%d 0\n", rc); return 1; }
    float folded[10];
    if (ur_host_env_sky_params(&k, folded) != 0) return 1;
    const ur_sky::Params params = ur_sky::fold(k.CameraPosition, k.LightDirection, k.LightColor);
    if (memcmp(folded, &params, sizeof params) != 0) return 1;
    const ur_sky::Plan p = ur_sky::make_plan(params, base, taps);
    const uint32_t launched = (p.waves + 3u) / 4u * 4u; // whole workgroups of four waves: the last ones may hold no texel
    for (uint32_t wave = launched; wave-- > 0u;) ur_sky::wave_item(p, got, wave);
    if (differ(want, got, bytes)) return 1;
    printf("%d %llu\n", rc, sum_of(want, bytes));
    free(want); free(got);
    return 0;
}

static int lut(char** a)
{
    const uint32_t w = (uint32_t)atoi(a[0]), h = (uint32_t)atoi(a[1]), s = (uint32_t)atoi(a[2]);
    const size_t table_bytes = ur_brdf_lut_table_bytes(h, s), bytes = 4u * (size_t)w * h;
    if (table_bytes != 16u * (size_t)h * s) return 1;
    void* table = aligned(table_bytes);
    uint32_t* want = (uint32_t*)aligned(bytes);
    uint32_t* got = (uint32_t*)aligned(bytes);
    memset(want, 0, bytes);
    memset(got, 0xFF, bytes);
    int rc = ur_host_brdf_lut_table(h, s, table, table_bytes);
    if (rc == 0) rc = ur_host_brdf_lut(w, h, s, table, table_bytes, want, bytes);
    if (rc != 0) { printf("%d 0\n", rc); return 1; }
    const ur_lut::Plan p = ur_lut::make_plan(w, h, s);
    for (uint32_t texel = p.texels; texel-- > 0u;) ur_lut::texel_item(p, table, got, texel); // (a launched wave past the last texel returns at once)
    if (differ(want, got, bytes)) return 1;
    printf("%d %llu\n", rc, sum_of(want, bytes));
    free(table); free(want); free(got);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 11 && strcmp(argv[1], "sky") == 0) return sky(argv + 2);
    if (argc == 5 && strcmp(argv[1], "lut") == 0) return lut(argv + 2);
    return 2;
}
