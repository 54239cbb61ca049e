// slice_pretest.h — "no voxel of this slice can be a candidate in this frame", decided from the slice's bounding box in
// the image and a tile-max depth map, before the integrate's frame loop (tsdf_integrate.h integrate_body).  One text for the
// device prologue and for the host program that checks it against brute force (tests/test_slice_pretest_bound.py).
//
// A coarse slice is 8 x 8 x 4 voxels of a unit (slice s: x in [4 (s & 2), +8), y in [8 (s & 1), +8), z in
// [4 (s >> 2), +4)).  The integrate projects each voxel CENTRE: in camera space pc = E p + t, computed in float32, the
// z steps by repeated adds of es = E.col(2) * vl (frame_tap).  A voxel is a candidate iff its pixel (ui, vi) lies in
// the image, the staged depth dv there is > 0 and fl(dv - pc.z) > -trunc (voxel_candidate).
//
// The bound is computed in float32 (in float64 the prologue cost the integrate what the dropped frames saved:
// DESIGN.md §4.3), with every rounding of its own inside the pads.  Why it is safe:
//  (1) Box.  With c the centre of the slice's voxel centres and h = (3.5, 3.5, 1.5) vl their half extents, every exact
//      E p + t lies in c_r +- sum_j |E_rj| h_j per row r (interval arithmetic).  The kernel's float32 pc differs from the
//      exact one by at most ~22 roundings (two in the voxel's position, three products, three sums, up to 15 z adds, es
//      itself), each at most 2^-24 of a magnitude bounded by M_r = sum_j |E_rj| max|p_j| + |t_r| + 16 |es_r|: below
//      2^-19 M_r.  The box's own float32 evaluation here (centre, radius, the pad and its subtraction: fewer than 16
//      roundings of magnitudes within M_r) adds less than 2^-20 M_r.  The box is padded by 1e-4 m + 2^-18 M_r per row, so
//      the kernel's own pc lies inside it, with 1e-4 m to spare.
//  (2) z_lo (the padded box's nearest z) at or below PRE_Z_GUARD: may be live (the quotients below need z > 0).
//  (3) Pixels.  For z > 0, u = fx x / z + cx + 0.5 over the box takes its extremes at the four corner quotients.  Both
//      the kernel's u_f (certified reciprocal or IEEE quotient, then two adds) and the corner values here (an IEEE
//      reciprocal, two products, an add) are within a few 2^-24 max(|u|, W) of the exact values: below
//      0.005 + 2^-21 max(W, H) pixels each wherever the result can land in or beside the image, so the range is widened
//      by twice that and then by one whole pixel: floor(u_f) lies in [floor(u_min) - 1, floor(u_max) + 1].  Open3D's
//      border slivers [0, 1e-4) and [W - 1e-4, W) only shrink the image: a superset of the gathered pixels is still
//      covered.  A range wholly outside the image: every lane gathers depth 0, idle.
//  (4) Depth.  D = the largest staged depth over the tiles the pixel range covers (the map holds the float bits of the
//      largest depth > 0 of each tile, 0 if none: unsigned order is float order there; NaN and negatives enter as 0, +inf
//      stays and reads as live).  D == 0: no gathered depth is > 0, idle.  Otherwise every gathered dv <= D and every
//      kernel pc.z >= z_lo + 1e-4, so dv - pc.z <= D - z_lo - 1e-4; if fl(D - z_lo) <= -trunc then D - z_lo <= -trunc +
//      2^-24 |D - z_lo|, the exact dv - pc.z is below -trunc, and fl(dv - pc.z) <= -trunc by monotone rounding (-trunc
//      is a float): the candidate test fails.
//  (5) A box over more than PRE_CAP tiles in x or y counts as live (a close or grazing brick; bounds the prologue).
// The map is read four consecutive tiles at a time (tile4: one 16-B load on the device), one read per tile row and
// PRE_CAP rows, every read issued whether the box needs it or not (PRE_NONE: an index past every map) so that none
// waits for another; the entries beyond the box's last column are masked out of the maximum.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OT_PRE_HD __host__ __device__ inline
#else
#define OT_PRE_HD inline
#endif

namespace ot {

constexpr int PRE_TILE = 8;            // tile edge in pixels
constexpr int PRE_CAP = 4;             // tiles per axis a box may cover and still be tested (one read of four per row)
constexpr int PRE_NONE = 1 << 28;      // a tile index no batch's maps have (their words in all stay below it)
constexpr int PRE_SLACK = 8;           // words kept readable past a batch's maps: a read of four tiles never straddles
                                       // the end of the buffer
constexpr float PRE_Z_GUARD = 0.01f;   // metres
constexpr float PRE_PAD_ABS = 1e-4f;   // metres
constexpr float PRE_PAD_REL = 3.814697265625e-06f;  // 2^-18

struct PreTile4 {
    uint32_t k[4];
};

struct PreIntrinsics {
    int W, H;
    float fx, fy, cx, cy;
};

OT_PRE_HD int pre_tiles(int n) { return (n + PRE_TILE - 1) / PRE_TILE; }

// the map's entry of one staged depth
OT_PRE_HD uint32_t pre_depth_key(float d) {
    uint32_t b = 0u;
    if (d > 0.0f) __builtin_memcpy(&b, &d, 4);
    return b;
}

// true: no voxel of slice s of the unit (kx, ky, kz) can pass voxel_candidate in the frame with extrinsic rows E (the
// integrate's float32 E[12]).  vl: the integrate's float voxel length, unit_len its float64 unit length, trunc its float
// truncation; tile4(i): entries i .. i + 3 of the frame's map, row-major over pre_tiles(W) x pre_tiles(H) tiles (the
// entries past the frame's last are the next frame's or the slack's: masked here), zeros for i >= PRE_NONE.
template <class TileFn>
OT_PRE_HD bool slice_idle(const float* E, const PreIntrinsics& in, float vl, double unit_len, int kx, int ky, int kz,
                          int s, float trunc, TileFn&& tile4) {
    const float half = vl * 0.5f;
    const int x0 = (s & 2) * 4, y0 = (s & 1) * 8, z0 = (s >> 2) * 4;
    // the kernel's float origins (integrate_item), then the voxel centres' extremes per axis
    const float o[3] = {(float)((double)kx * unit_len), (float)((double)ky * unit_len), (float)((double)kz * unit_len)};
    const float lo[3] = {half + vl * (float)x0 + o[0], half + vl * (float)y0 + o[1], half + vl * (float)z0 + o[2]};
    // (7 vl and 3 vl by sums of vl's exact multiples: as products the device keeps the pair (7, 3) in registers through
    // the integrate's frame loop, which has none to spare)
    const float vl2 = vl + vl, vl3 = vl2 + vl, vl7 = (vl2 + vl2) + vl3;
    const float ext[3] = {vl7, vl7, vl3};
    const float mid[3] = {lo[0] + 0.5f * ext[0], lo[1] + 0.5f * ext[1], lo[2] + 0.5f * ext[2]};
    const float far_[3] = {fabsf(lo[0]) + ext[0], fabsf(lo[1]) + ext[1], fabsf(half + o[2]) + 32.0f * vl};
    float bl[3], bh[3];
    for (int a = 0; a < 3; ++a) {
        const float e0 = E[a * 4 + 0], e1 = E[a * 4 + 1], e2 = E[a * 4 + 2], t = E[a * 4 + 3];
        const float a0 = fabsf(e0), a1 = fabsf(e1), a2 = fabsf(e2);
        const float c = e0 * mid[0] + e1 * mid[1] + e2 * mid[2] + t;
        const float r = 0.5f * (a0 * ext[0] + a1 * ext[1] + a2 * ext[2]);
        const float m = a0 * far_[0] + a1 * far_[1] + a2 * far_[2] + fabsf(t);
        const float pad = r + (PRE_PAD_ABS + PRE_PAD_REL * m);
        bl[a] = c - pad, bh[a] = c + pad;
    }
    const float zl = bl[2], zh = bh[2];
    if (!(zl > PRE_Z_GUARD) || !(zh < 1e30f)) return false;  // (a NaN or infinite pose: live)
    const float izl = 1.0f / zl, izh = 1.0f / zh;
    const float xl = in.fx * bl[0], xh = in.fx * bh[0], yl = in.fy * bl[1], yh = in.fy * bh[1];
    const float ua = xl * izl, ub = xl * izh, uc = xh * izl, ud = xh * izh;
    const float va = yl * izl, vb = yl * izh, vc = yh * izl, vd = yh * izh;
    float umin = fminf(fminf(ua, ub), fminf(uc, ud)) + (in.cx + 0.5f);
    float umax = fmaxf(fmaxf(ua, ub), fmaxf(uc, ud)) + (in.cx + 0.5f);
    float vmin = fminf(fminf(va, vb), fminf(vc, vd)) + (in.cy + 0.5f);
    float vmax = fmaxf(fmaxf(va, vb), fmaxf(vc, vd)) + (in.cy + 0.5f);
    if (!(umin <= umax) || !(vmin <= vmax)) return false;  // NaN: live
    const float W = (float)in.W, H = (float)in.H;
    const float wide = 0.01f + 9.5367431640625e-07f * (W > H ? W : H);  // (3): 2 (0.005 + 2^-21 max(W, H))
    umin = fmaxf(umin - wide, -4.0f), umax = fminf(umax + wide, W + 4.0f);
    vmin = fmaxf(vmin - wide, -4.0f), vmax = fminf(vmax + wide, H + 4.0f);
    int u0 = (int)floorf(umin) - 1, u1 = (int)floorf(umax) + 1;
    int v0 = (int)floorf(vmin) - 1, v1 = (int)floorf(vmax) + 1;
    if (u1 < 0 || v1 < 0 || u0 > in.W - 1 || v0 > in.H - 1 || u0 > u1 || v0 > v1) return true;  // outside the image
    u0 = u0 < 0 ? 0 : u0, v0 = v0 < 0 ? 0 : v0;
    u1 = u1 > in.W - 1 ? in.W - 1 : u1, v1 = v1 > in.H - 1 ? in.H - 1 : v1;
    const int tx0 = u0 / PRE_TILE, tx1 = u1 / PRE_TILE, ty0 = v0 / PRE_TILE, ty1 = v1 / PRE_TILE;
    if (tx1 - tx0 >= PRE_CAP || ty1 - ty0 >= PRE_CAP) return false;
    const int tmx = pre_tiles(in.W);
    PreTile4 q[PRE_CAP];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < PRE_CAP; ++r)  // every read before any use
        q[r] = tile4(ty0 + r <= ty1 ? (ty0 + r) * tmx + tx0 : PRE_NONE);
    const int last = tx1 - tx0;  // columns 0 .. last of a row's four entries belong to the box
    uint32_t best = 0u;
    for (int j = 0; j < 4; ++j) {  // the rows of a column first, then the box's columns
        uint32_t k = 0u;
        for (int r = 0; r < PRE_CAP; ++r) k = q[r].k[j] > k ? q[r].k[j] : k;
        k = j <= last ? k : 0u;
        best = k > best ? k : best;
    }
    if (best == 0u) return true;  // no depth > 0 under the box
    float D;
    __builtin_memcpy(&D, &best, 4);
    return D - zl <= -trunc;  // (+inf, or a NaN that cannot be there, fails: live)
}

}  // namespace ot
