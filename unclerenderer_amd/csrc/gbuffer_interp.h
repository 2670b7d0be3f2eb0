// From a visibility key's triangle to a texel's attribute weights — what the two resolves (csrc/gbuffer_resolve.hip,
// csrc/forward_resolve.hip) and the alpha test of the masked raster (csrc/raster_mask.hip) must compute alike, operation for operation: the near
// clip restated with a weight row per polygon vertex, the piece of the triangle that covers a centre with its
// exact edge values, the perspective-correct weights over the original three vertices, and TEXCOORD at the texel's quad partners
// (section 3.10). Device inline functions only; csrc/visibility_key.h has what comes before and after them.
#pragma once

#include "raster_rule.h"

namespace ur_raster {

// Rule 2 again (DepthPolicy::assemble) from the three clip-space vertices: the target-space polygon (SX, SY)[0..3], its clip w and, per
// polygon vertex, the weight row B over the original three; `one` = one vertex lies behind the near plane (two triangles are emitted)
__device__ __forceinline__ void clip_polygon(const float (&c)[3][4], float half_w, float half_h, float (&SX)[4], float (&SY)[4], float (&vw)[4], float (&B)[4][3],
                                             bool& one)
{
    const float d0 = c[0][3] - c[0][2], d1 = c[1][3] - c[1][2], d2 = c[2][3] - c[2][2];
    const bool o0 = d0 < 0.0f, o1 = d1 < 0.0f, o2 = d2 < 0.0f;
    const uint32_t n_out = (o0 ? 1u : 0u) + (o1 ? 1u : 0u) + (o2 ? 1u : 0u);
    const uint32_t rot = n_out == 1u ? (o0 ? 1u : (o1 ? 2u : 0u)) : (n_out == 2u ? (!o0 ? 0u : (!o1 ? 1u : 2u)) : 0u);
    const uint32_t ia = rot, ib = rot == 2u ? 0u : rot + 1u, ic = rot == 0u ? 2u : rot - 1u;
    const float ax = sel3(rot, c[0][0], c[1][0], c[2][0]), ay = sel3(rot, c[0][1], c[1][1], c[2][1]);
    const float aw = sel3(rot, c[0][3], c[1][3], c[2][3]), ad = sel3(rot, d0, d1, d2);
    const float bx = sel3(rot, c[1][0], c[2][0], c[0][0]), by = sel3(rot, c[1][1], c[2][1], c[0][1]);
    const float bw = sel3(rot, c[1][3], c[2][3], c[0][3]), bd = sel3(rot, d1, d2, d0);
    const float cx = sel3(rot, c[2][0], c[0][0], c[1][0]), cy = sel3(rot, c[2][1], c[0][1], c[1][1]);
    const float cw = sel3(rot, c[2][3], c[0][3], c[1][3]), cd = sel3(rot, d2, d0, d1);
    const bool two = n_out == 2u, whole = n_out == 0u;
    one = n_out == 1u;
    const float ix = one ? bx : ax, iy = one ? by : ay, iw = one ? bw : aw, id = one ? bd : ad;
    const float ox = one ? cx : bx, oy = one ? cy : by, ow = one ? cw : bw, od = one ? cd : bd;
    const uint32_t ii = one ? ib : ia, io = one ? ic : ib;
    const float tp = id / (id - od), tq = ad / (ad - cd);
    const float px = ix + tp * (ox - ix), py = iy + tp * (oy - iy), pw = iw + tp * (ow - iw);
    const float qx = ax + tq * (cx - ax), qy = ay + tq * (cy - ay), qw = aw + tq * (cw - aw);
    float vx[4], vy[4];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float ua = (uint32_t)j == ia ? 1.0f : 0.0f, ub = (uint32_t)j == ib ? 1.0f : 0.0f, uc = (uint32_t)j == ic ? 1.0f : 0.0f;
        const float up = (uint32_t)j == ii ? 1.0f - tp : ((uint32_t)j == io ? tp : 0.0f);
        const float uq = (uint32_t)j == ia ? 1.0f - tq : ((uint32_t)j == ic ? tq : 0.0f);
        B[0][j] = ua;
        B[1][j] = two ? up : ub;
        B[2][j] = whole ? uc : (one ? up : uq);
        B[3][j] = uq;
    }
    vx[0] = ax; vy[0] = ay; vw[0] = aw;
    vx[1] = two ? px : bx; vy[1] = two ? py : by; vw[1] = two ? pw : bw;
    vx[2] = whole ? cx : (one ? px : qx); vy[2] = whole ? cy : (one ? py : qy); vw[2] = whole ? cw : (one ? pw : qw);
    vx[3] = qx; vy[3] = qy; vw[3] = qw;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        SX[k] = (vx[k] / vw[k] + 1.0f) * half_w;
        SY[k] = (1.0f - vy[k] / vw[k]) * half_h;
    }
}

// Rules 3-4 at one centre for the target-space triangle (X, Y)[0..2], already reordered: false when it is dropped, culled or does not
// cover (sx, sy); else the exact edge values l0 = E12, l1 = E20, l2 = E01
__device__ __forceinline__ bool cover(const float (&X)[3], const float (&Y)[3], int sx, int sy, long long& l0, long long& l1, long long& l2)
{
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const bool finite = fabsf(X[v]) <= kFloatMax && fabsf(Y[v]) <= kFloatMax;
        if (!finite || fabsf(X[v]) > kDepthGuardBand || fabsf(Y[v]) > kDepthGuardBand) return false;
    }
    const int x0 = (int)rintf(X[0] * 256.0f), y0 = (int)rintf(Y[0] * 256.0f), x1 = (int)rintf(X[1] * 256.0f), y1 = (int)rintf(Y[1] * 256.0f);
    const int x2 = (int)rintf(X[2] * 256.0f), y2 = (int)rintf(Y[2] * 256.0f);
    const long long A = (long long)(x1 - x0) * (y2 - y0) - (long long)(x2 - x0) * (y1 - y0);
    if (A <= 0) return false;
    const long long e01 = (long long)(x1 - x0) * (sy - y0) - (long long)(y1 - y0) * (sx - x0);
    const long long e12 = (long long)(x2 - x1) * (sy - y1) - (long long)(y2 - y1) * (sx - x1);
    const long long e20 = (long long)(x0 - x2) * (sy - y2) - (long long)(y0 - y2) * (sx - x2);
    l0 = e12; l1 = e20; l2 = e01;
    return ((e01 - edge_bias(x0, y0, x1, y1)) | (e12 - edge_bias(x1, y1, x2, y2)) | (e20 - edge_bias(x2, y2, x0, y0))) >= 0;
}

// The piece of the polygon that covers a centre: the reordered triangle, its edge values at the centre and its vertices' clip w
struct Piece {
    float X[3], Y[3];
    long long l0, l1, l2;
    float cw0, cw1, cw2;
    bool second;
};

// Emitted triangle 0 if rule 4 says it covers (sx, sy), else 1; reordered (r0, r1, r2) = (S0, S[2 + e], S[1 + e])
__device__ __forceinline__ void covering_piece(const float (&SX)[4], const float (&SY)[4], const float (&vw)[4], bool one, int sx, int sy, Piece& pc)
{
    pc.l0 = 0; pc.l1 = 0; pc.l2 = 0;
    pc.X[0] = SX[0]; pc.X[1] = SX[2]; pc.X[2] = SX[1];
    pc.Y[0] = SY[0]; pc.Y[1] = SY[2]; pc.Y[2] = SY[1];
    pc.second = false;
    if (!cover(pc.X, pc.Y, sx, sy, pc.l0, pc.l1, pc.l2) && one) {
        pc.second = true;
        pc.X[1] = SX[3]; pc.Y[1] = SY[3]; pc.X[2] = SX[2]; pc.Y[2] = SY[2];
        (void)cover(pc.X, pc.Y, sx, sy, pc.l0, pc.l1, pc.l2);
    }
    pc.cw0 = vw[0]; pc.cw1 = pc.second ? vw[3] : vw[2]; pc.cw2 = pc.second ? vw[2] : vw[1];
}

// The perspective-correct weights b over the original three vertices from the piece's edge values (m0, m1, m2) at a point
__device__ __forceinline__ void piece_weights(const Piece& pc, long long m0, long long m1, long long m2, const float (&B)[4][3], float (&b)[3])
{
    const float q0 = (float)m0 / pc.cw0, q1 = (float)m1 / pc.cw1, q2 = (float)m2 / pc.cw2;
    const float s = (q0 + q1) + q2;
    const float g0 = q0 / s, g1 = q1 / s, g2 = q2 / s;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float B1 = pc.second ? B[3][j] : B[2][j], B2 = pc.second ? B[2][j] : B[1][j];
        b[j] = (g0 * B[0][j] + g1 * B1) + g2 * B2;
    }
}

// TEXCOORD at the centre (point 0), the horizontal (1) and the vertical (2) quad partner of the texel (column, row) on its own triangle:
// the edge functions are affine, so a step of one pixel adds the coefficient times 256
__device__ __forceinline__ void quad_texcoords(const Piece& pc, const float (&B)[4][3], const float (&uv)[3][2], bool odd_column, bool odd_row, float (&pu)[3],
                                               float (&pv)[3])
{
    const int x0 = (int)rintf(pc.X[0] * 256.0f), y0 = (int)rintf(pc.Y[0] * 256.0f), x1 = (int)rintf(pc.X[1] * 256.0f), y1 = (int)rintf(pc.Y[1] * 256.0f);
    const int x2 = (int)rintf(pc.X[2] * 256.0f), y2 = (int)rintf(pc.Y[2] * 256.0f);
    const long long step_x = odd_column ? -256 : 256, step_y = odd_row ? -256 : 256;
#pragma unroll
    for (int point = 0; point < 3; ++point) {
        long long m0 = pc.l0, m1 = pc.l1, m2 = pc.l2;
        if (point == 1) { m0 -= step_x * (y2 - y1); m1 -= step_x * (y0 - y2); m2 -= step_x * (y1 - y0); }
        if (point == 2) { m0 += step_y * (x2 - x1); m1 += step_y * (x0 - x2); m2 += step_y * (x1 - x0); }
        float bb[3];
        piece_weights(pc, m0, m1, m2, B, bb);
        pu[point] = (bb[0] * uv[0][0] + bb[1] * uv[1][0]) + bb[2] * uv[2][0];
        pv[point] = (bb[0] * uv[0][1] + bb[1] * uv[1][1]) + bb[2] * uv[2][1];
    }
}

} // namespace ur_raster
