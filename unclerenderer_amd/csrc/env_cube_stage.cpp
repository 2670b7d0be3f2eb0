// The staged environment cube's contents (lighting_plan.h has its layout): border folding and the two sections, written into a host
// buffer. Plain C++17 (no HIP header), so tests/cpp/sanitize_main.cpp drives it beside the oracle's staging; ur_stage_env_cube
// (ur_api.hip) checks its arguments, calls it and copies the buffer to the device.
#include "lighting_plan.h"

#include <cmath>
#include <vector>

#include "../../include/ur_hotpath.h"

namespace {

// ---- bordered cube staging (host) ------------------------------------------------------------------------------------
// Face addressing is D3D's (+X,-X,+Y,-Y,+Z,-Z; ties z > y > x). A border texel is the texel of the adjacent face that the
// one-texel overshoot lands on when the face plane is folded over the shared edge; a corner border texel first clamps its
// second coordinate into the face (same rule as the oracle's FetchCubeTexel — the rule is the specification).
struct FaceAxes { int major, su, sv; double ms, us, vs; }; // p[major]=ms, p[su]=us*s, p[sv]=vs*t
const FaceAxes kFaces[6] = {
    {0, 2, 1, +1, -1, -1}, // +X: (1, -t, -s)
    {0, 2, 1, -1, +1, -1}, // -X: (-1, -t, s)
    {1, 0, 2, +1, +1, +1}, // +Y: (s, 1, t)
    {1, 0, 2, -1, +1, -1}, // -Y: (s, -1, -t)
    {2, 0, 1, +1, +1, -1}, // +Z: (s, -t, 1)
    {2, 0, 1, -1, -1, -1}, // -Z: (-s, -t, -1)
};

void resolve_border(int N, int face, int i, int j, int& oface, int& oi, int& oj)
{
    const bool iOut = i < 0 || i >= N, jOut = j < 0 || j >= N;
    if (!iOut && !jOut) { oface = face; oi = i; oj = j; return; }
    if (iOut && jOut) j = j < 0 ? 0 : N - 1;
    const double s = 2.0 * (i + 0.5) / N - 1.0, t = 2.0 * (j + 0.5) / N - 1.0;
    const FaceAxes& F = kFaces[face];
    double p[3];
    p[F.major] = F.ms; p[F.su] = F.us * s; p[F.sv] = F.vs * t;
    const double over = (iOut ? std::fabs(s) : std::fabs(t)) - 1.0;
    p[F.major] *= (1.0 - over);
    const int oa = iOut ? F.su : F.sv;
    p[oa] = p[oa] > 0 ? 1.0 : -1.0;
    // the folded point lies on the face whose axis is `oa`
    const int nf = oa * 2 + (p[oa] > 0 ? 0 : 1);
    const FaceAxes& G = kFaces[nf];
    const double ns = p[G.su] / G.us, nt = p[G.sv] / G.vs;
    oface = nf;
    oi = (int)std::floor((ns + 1.0) * 0.5 * N);
    oj = (int)std::floor((nt + 1.0) * 0.5 * N);
    oi = oi < 0 ? 0 : (oi >= N ? N - 1 : oi);
    oj = oj < 0 ? 0 : (oj >= N ? N - 1 : oj);
}

} // namespace

namespace ur {

void stage_env_cube_host(const ur_half4* src, const CubeLayout& L, ur_half4* out)
{
    const uint32_t mip_count = L.mips;
    std::vector<size_t> mip_off(mip_count);
    size_t face_stride = 0;
    for (uint32_t m = 0; m < mip_count; ++m) {
        mip_off[m] = face_stride;
        const size_t n = L.size(m);
        face_stride += n * n;
    }
    for (uint32_t m = 0; m < mip_count; ++m) {
        const int N = (int)L.size(m), E = N + 2;
        const size_t off = L.bordered[m];
        for (int f = 0; f < 6; ++f)
            for (int j = -1; j <= N; ++j)
                for (int i = -1; i <= N; ++i) {
                    int sf, si, sj;
                    resolve_border(N, f, i, j, sf, si, sj);
                    out[off + ((size_t)f * E + (j + 1)) * E + (i + 1)] = src[(size_t)sf * face_stride + mip_off[m] + (size_t)sj * N + si];
                }
    }
    // Second section, behind all bordered mips: every mip once more as RGB ROW PAIRS. Entry (f, j, i), j in [0, E-2], is the 12 bytes
    // {R G B of texel (i, j), R G B of texel (i, j + 1)} of the bordered face (the alpha channel is never sampled:
    // DeferredLighting.hlsl:82,86 take .rgb), entries of a pair-row contiguous: the 2x2 bilinear footprint at (i, j) is the 24
    // bytes at entry ((f (E-1) + j) E + i) - two 12-byte loads that almost always fall into ONE cache line where the bordered
    // layout's two rows are two lines and two 16-byte loads. The streaming lighting kernel gathers its prefiltered taps here.
    {
        for (uint32_t m = 0; m < mip_count; ++m) {
            const size_t E = L.edge[m], boff = L.bordered[m];
            uint16_t* rgb = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(out) + L.pairs[m]);
            size_t e = 0;
            for (size_t f = 0; f < 6; ++f)
                for (size_t j = 0; j + 1 < E; ++j)
                    for (size_t i = 0; i < E; ++i) {
                        const ur_half4& t0 = out[boff + (f * E + j) * E + i];
                        const ur_half4& t1 = out[boff + (f * E + j + 1) * E + i];
                        rgb[e++] = t0.x; rgb[e++] = t0.y; rgb[e++] = t0.z;
                        rgb[e++] = t1.x; rgb[e++] = t1.y; rgb[e++] = t1.z;
                    }
        }
    }
}

} // namespace ur
