// A stand-alone program over the host code of the environment from a panorama, for the compiler's sanitizers: no
// Python, no device. Built with csrc/hdr.cpp and csrc/env_panorama_host.cpp by tests/test_env_panorama_abi.py.
//   env_panorama_main value M E    the bits of the texel value m * 2^(e - 136) as the rule builds it, in hex
//   env_panorama_main values       every (m, e) against ldexp in double, and through the fp32 bits back: prints "values ok"
//   env_panorama_main file FILE    a .hdr file through ur_hdr_parse and ur_hdr_unpack into a heap buffer of exactly 4 W H bytes, then every
//                                  prefix of the file the same way (a truncated file may be refused or, where only bytes behind the image
//                                  are missing, read; it may not be read outside its bytes). Prints "rc width height rle sum refused",
//                                  sum of the texels' bytes, refused the number of prefixes refused.
//   env_panorama_main build FILE   FILE = { u32 width, height, base, taps; the panorama's 4 W H bytes }: ur_host_env_panorama into a heap
//                                  buffer of exactly its size; then the launch of csrc/env_panorama.hip as the device runs it - the
//                                  waves of the rule, descending, into a destination that arrives as 0xFF - which must give the same
//                                  bytes. Prints "rc sum" (sum: of the destination's bytes).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/ur_assets.h"
#include "../../include/ur_host.h"
#include "../../unclerenderer_amd/csrc/env_panorama_rule.h"

static void* aligned(size_t bytes)
{
    void* p = nullptr;
    if (posix_memalign(&p, 16, bytes ? bytes : 1) != 0) exit(2);
    return p;
}

static uint8_t* read_file(const char* path, size_t& size)
{
    FILE* f = fopen(path, "rb");
    if (!f) exit(2);
    fseek(f, 0, SEEK_END);
    size = (size_t)ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t* data = (uint8_t*)malloc(size ? size : 1);
    if (fread(data, 1, size, f) != size) exit(2);
    fclose(f);
    return data;
}

static int values()
{
    for (uint32_t e = 0u; e < 256u; ++e)
        for (uint32_t m = 0u; m < 256u; ++m) {
            const float got = ur_pano::rgbe_value(m, e);
            const double want = e == 0u ? 0.0 : ldexp((double)m, (int)e - 136);
            if ((double)got != want || (float)want != got || std::signbit(got)) { printf("m %u e %u: %a against %a\n", m, e, (double)got, want); return 1; }
        }
    printf("values ok\n");
    return 0;
}

static int file(const char* path)
{
    size_t size = 0;
    uint8_t* whole = read_file(path, size);
    ur_hdr_info info;
    int rc = ur_hdr_parse(whole, size, &info);
    unsigned long long sum = 0;
    size_t bytes = 0;
    if (rc == 0) {
        bytes = 4u * (size_t)info.width * info.height;
        uint8_t* out = (uint8_t*)malloc(bytes);
        rc = ur_hdr_unpack(whole, size, &info, out);
        if (rc == 0)
            for (size_t i = 0; i < bytes; ++i) sum += out[i];
        free(out);
    }
    unsigned refused = 0;
    for (size_t n = 0; n < size; ++n) { // a copy of exactly n bytes: a read behind it is a read outside the heap block
        uint8_t* part = (uint8_t*)malloc(n ? n : 1);
        memcpy(part, whole, n);
        ur_hdr_info cut;
        int r = ur_hdr_parse(part, n, &cut);
        if (r == 0) {
            uint8_t* out = (uint8_t*)malloc(4u * (size_t)cut.width * cut.height);
            r = ur_hdr_unpack(part, n, &cut, out);
            free(out);
        }
        if (r != 0) {
            ++refused;
            if (ur_hdr_last_error()[0] == 0) { printf("a refusal without text at %zu bytes\n", n); return 1; }
        }
        free(part);
    }
    printf("%d %u %u %u %llu %u\n", rc, rc == 0 ? info.width : 0u, rc == 0 ? info.height : 0u, rc == 0 ? info.rle : 0u, sum, refused);
    free(whole);
    return 0;
}

static int build(const char* path)
{
    size_t size = 0;
    uint8_t* whole = read_file(path, size);
    if (size < 16) return 2;
    uint32_t h[4];
    memcpy(h, whole, 16);
    const uint32_t width = h[0], height = h[1], base = h[2], taps = h[3];
    const size_t src_bytes = 4u * (size_t)width * height, dst_bytes = 48u * (size_t)base * base;
    if (size != 16u + src_bytes) return 2;
    uint32_t* src = (uint32_t*)aligned(src_bytes);
    memcpy(src, whole + 16, src_bytes);
    free(whole);
    uint64_t* want = (uint64_t*)aligned(dst_bytes);
    uint64_t* got = (uint64_t*)aligned(dst_bytes);
    memset(want, 0, dst_bytes);
    memset(got, 0xFF, dst_bytes);
    const int rc = ur_host_env_panorama(src, src_bytes, width, height, base, taps, want, dst_bytes);
    if (rc != 0) { printf("%d 0\n", rc); return 1; }
    if (ur_host_env_panorama_taps(width, height, base) != ur_pano::recommended_taps(width, height, base)) return 1;
    // the device's launch, on the host; the waves in descending order: no wave may depend on another
    const ur_pano::Plan p = ur_pano::make_plan(width, height, base, taps);
    const uint32_t launched = (p.waves + 3u) / 4u * 4u; // whole workgroups of four waves: the last ones may hold no texel
    for (uint32_t wave = launched; wave-- > 0u;) ur_pano::wave_item(p, src, got, wave);
    if (memcmp(want, got, dst_bytes) != 0) {
        size_t at = 0;
        while (at < dst_bytes && ((const uint8_t*)want)[at] == ((const uint8_t*)got)[at]) ++at;
        printf("the waves differ from the host build: first at byte %zu of %zu\n", at, dst_bytes);
        return 1;
    }
    unsigned long long sum = 0;
    for (size_t i = 0; i < dst_bytes; ++i) sum += ((const uint8_t*)want)[i];
    printf("%d %llu\n", rc, sum);
    free(src); free(want); free(got);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && strcmp(argv[1], "value") == 0) {
        const float v = ur_pano::rgbe_value((uint32_t)atoi(argv[2]), (uint32_t)atoi(argv[3]));
        uint32_t bits;
        memcpy(&bits, &v, 4);
        printf("%08x\n", bits);
        return 0;
    }
    if (argc == 2 && strcmp(argv[1], "values") == 0) return values();
    if (argc == 3 && strcmp(argv[1], "file") == 0) return file(argv[2]);
    if (argc == 3 && strcmp(argv[1], "build") == 0) return build(argv[2]);
    return 2;
}
