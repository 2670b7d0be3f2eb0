// Radiance .hdr (RGBE) container: header parse and scanline expansion to the file's own texels, four bytes R G B E each (include/ur_assets.h,
// DESIGN.md section 3.21). The reference reads such files with stb_image's HDR loader (ThirdParty/stb/stb_image.h, stbi__hdr_load); this is
// its rule, written from the format - "#?RADIANCE" header lines, a "-Y H +X W" resolution line, new-style run-length coded scanlines whose
// four channel planes follow one another - and stops at the bytes: the decode to numbers is ur_env_panorama's, on the device.
// The expansion stays on the host: where a scanline starts is known only once the runs in front of it have been walked, and that walk costs
// what the expansion costs. Plain C++17, no device code.

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/ur_assets.h"

namespace {

thread_local char g_text[256] = "";

int refuse(int code, const char* fmt, ...)
{
    va_list args;
    va_start(args, fmt);
    vsnprintf(g_text, sizeof g_text, fmt, args);
    va_end(args);
    return code;
}

// The line that starts at `at`: its length without the '\n', and where the next one starts. false when the file ends before a '\n'.
bool line(const uint8_t* p, size_t size, size_t at, size_t& length, size_t& next)
{
    for (size_t i = at; i < size; ++i)
        if (p[i] == '\n') { length = i - at; next = i + 1u; return true; }
    return false;
}

bool is(const uint8_t* p, size_t length, const char* text) { return length == strlen(text) && memcmp(p, text, length) == 0; }

// Decimal digits at p[at ..]: the value (saturating) and where they end. false when there is none.
bool number(const uint8_t* p, size_t end, size_t& at, uint32_t& value)
{
    const size_t first = at;
    uint64_t v = 0u;
    while (at < end && p[at] >= '0' && p[at] <= '9') {
        v = v * 10u + (uint64_t)(p[at] - '0');
        if (v > 0xFFFFFFFFull) v = 0xFFFFFFFFull;
        ++at;
    }
    value = (uint32_t)v;
    return at != first;
}

bool coded(const uint8_t* p, size_t size, size_t at, uint32_t width)
{
    return width >= 8u && width < 32768u && size - at >= 4u && p[at] == 2u && p[at + 1u] == 2u && p[at + 2u] < 128u;
}

} // namespace

extern "C" {

const char* ur_hdr_last_error(void) { return g_text; }

int ur_hdr_parse(const void* file, size_t size, ur_hdr_info* out)
{
    if (!file || !out) return refuse(UR_EINVAL, "ur_hdr_parse: null file or info");
    const uint8_t* p = static_cast<const uint8_t*>(file);
    size_t at = 0u, length = 0u, next = 0u;
    if (!line(p, size, at, length, next) || !(is(p, length, "#?RADIANCE") || is(p, length, "#?RGBE")))
        return refuse(UR_EINVAL, "ur_hdr_parse: the first line is neither #?RADIANCE nor #?RGBE");
    bool format = false;
    for (;;) {
        at = next;
        if (!line(p, size, at, length, next)) return refuse(UR_EINVAL, "ur_hdr_parse: the file ends inside the header");
        if (length == 0u) break;
        if (is(p + at, length, "FORMAT=32-bit_rle_rgbe")) format = true;
    }
    if (!format) return refuse(UR_EINVAL, "ur_hdr_parse: no FORMAT=32-bit_rle_rgbe line");
    at = next;
    if (!line(p, size, at, length, next)) return refuse(UR_EINVAL, "ur_hdr_parse: the file ends before the resolution line");
    const size_t end = at + length;
    // two axes, each a sign, a letter, a blank and a number; only "-Y H +X W" is read
    if (length < 3u || (p[at] != '-' && p[at] != '+') || (p[at + 1u] != 'X' && p[at + 1u] != 'Y') || p[at + 2u] != ' ')
        return refuse(UR_EINVAL, "ur_hdr_parse: no resolution line behind the header");
    if (p[at] != '-' || p[at + 1u] != 'Y') return refuse(UR_EUNSUPPORTED, "ur_hdr_parse: the resolution line is not -Y H +X W");
    uint32_t width = 0u, height = 0u;
    size_t i = at + 3u;
    if (!number(p, end, i, height)) return refuse(UR_EINVAL, "ur_hdr_parse: no height in the resolution line");
    while (i < end && p[i] == ' ') ++i;
    if (end - i < 3u || (p[i] != '-' && p[i] != '+') || (p[i + 1u] != 'X' && p[i + 1u] != 'Y') || p[i + 2u] != ' ')
        return refuse(UR_EINVAL, "ur_hdr_parse: no second axis in the resolution line");
    if (p[i] != '+' || p[i + 1u] != 'X') return refuse(UR_EUNSUPPORTED, "ur_hdr_parse: the resolution line is not -Y H +X W");
    i += 3u;
    if (!number(p, end, i, width) || i != end) return refuse(UR_EINVAL, "ur_hdr_parse: no width at the end of the resolution line");
    if (width < 1u || width > UR_HDR_MAX_WIDTH || height < 1u || height > UR_HDR_MAX_HEIGHT)
        return refuse(UR_EINVAL, "ur_hdr_parse: %u x %u (1..%u x 1..%u)", width, height, UR_HDR_MAX_WIDTH, UR_HDR_MAX_HEIGHT);
    if (next > 0xFFFFFFFFull) return refuse(UR_EINVAL, "ur_hdr_parse: a header of more than 4 GiB");
    out->width = width;
    out->height = height;
    out->payload_offset = (uint32_t)next;
    out->rle = coded(p, size, next, width) ? 1u : 0u;
    return UR_OK;
}

int ur_hdr_unpack(const void* file, size_t size, const ur_hdr_info* info, uint8_t* rgbe_out)
{
    if (!file || !info || !rgbe_out) return refuse(UR_EINVAL, "ur_hdr_unpack: null file, info or destination");
    const uint8_t* p = static_cast<const uint8_t*>(file);
    const uint32_t W = info->width, H = info->height;
    if (W < 1u || W > UR_HDR_MAX_WIDTH || H < 1u || H > UR_HDR_MAX_HEIGHT || info->payload_offset > size || info->rle > 1u ||
        (info->rle != 0u) != coded(p, size, info->payload_offset, W))
        return refuse(UR_EINVAL, "ur_hdr_unpack: the info is not ur_hdr_parse's of this file");
    size_t at = info->payload_offset;
    if (!info->rle) {
        const size_t need = 4u * (size_t)W * H;
        if (size - at < need) return refuse(UR_EINVAL, "ur_hdr_unpack: truncated: %zu payload bytes, %zu needed", size - at, need);
        memcpy(rgbe_out, p + at, need);
        return UR_OK;
    }
    for (uint32_t y = 0u; y < H; ++y) {
        if (size - at < 4u) return refuse(UR_EINVAL, "ur_hdr_unpack: truncated in front of scanline %u", y);
        if (p[at] != 2u || p[at + 1u] != 2u || p[at + 2u] >= 128u) return refuse(UR_EINVAL, "ur_hdr_unpack: scanline %u has no run-length marker", y);
        const uint32_t marked = ((uint32_t)p[at + 2u] << 8) | p[at + 3u];
        if (marked != W) return refuse(UR_EINVAL, "ur_hdr_unpack: scanline %u is marked %u texels long, the width is %u", y, marked, W);
        at += 4u;
        uint8_t* row = rgbe_out + 4u * (size_t)W * y;
        for (uint32_t c = 0u; c < 4u; ++c) {
            uint32_t x = 0u;
            while (x < W) {
                if (at >= size) return refuse(UR_EINVAL, "ur_hdr_unpack: truncated in scanline %u", y);
                const uint32_t count = p[at++];
                if (count == 0u) return refuse(UR_EINVAL, "ur_hdr_unpack: a count of 0 in scanline %u", y);
                if (count > 128u) {
                    const uint32_t run = count - 128u;
                    if (run > W - x) return refuse(UR_EINVAL, "ur_hdr_unpack: a run past the width in scanline %u", y);
                    if (at >= size) return refuse(UR_EINVAL, "ur_hdr_unpack: truncated in scanline %u", y);
                    const uint8_t value = p[at++];
                    for (uint32_t k = 0u; k < run; ++k) row[4u * (x + k) + c] = value;
                    x += run;
                } else {
                    if (count > W - x) return refuse(UR_EINVAL, "ur_hdr_unpack: literals past the width in scanline %u", y);
                    if (size - at < count) return refuse(UR_EINVAL, "ur_hdr_unpack: truncated in scanline %u", y);
                    for (uint32_t k = 0u; k < count; ++k) row[4u * (x + k) + c] = p[at + k];
                    at += count;
                    x += count;
                }
            }
        }
    }
    return UR_OK;
}

} // extern "C"
