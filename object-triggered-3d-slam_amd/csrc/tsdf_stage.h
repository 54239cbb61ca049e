// tsdf_stage.h — device text of the TSDF batch staging: the per-pixel (depth, colour) records of a batch's frames and
// their tile-max depth maps (slice_pretest.h), and the buffer-resource helpers the staged records are read through.
// Included by the kernels that stage (tsdf_frontend.hip) and, through tsdf_touch.h and tsdf_integrate.h, by those that
// read what was staged.
#pragma once

#include "slice_pretest.h"
#include "tsdf.h"

namespace ot {

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Raw buffer resource over [base, base + bytes): gfx9 dword3 (0x00020000, 32-bit raw data); loads past the end
// return 0 instead of faulting.
__device__ inline __amdgpu_buffer_rsrc_t make_rsrc(const void* base, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, bytes, 0x00020000);
}

// element i of a float64 array behind a buffer resource (32-bit offsets: no per-lane 64-bit address registers)
__device__ inline double ld_f64(__amdgpu_buffer_rsrc_t r, int i) {
    const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, i * 8, 0, 0);
    return __hiloint2double((int)v.y, (int)v.x);
}
__device__ inline void st_f64(__amdgpu_buffer_rsrc_t r, int i, double x) {
    u32x2 v;
    v.x = (unsigned)__double2loint(x);
    v.y = (unsigned)__double2hiint(x);
    __builtin_amdgcn_raw_buffer_store_b64(v, r, i * 8, 0, 0);
}

// Per-pixel staging of a batch: (depth, colour) as one 8-B record (colour word 0 for a frame without colour), so the
// integrate kernel fetches a voxel's per-frame inputs with one aligned load it can issue ahead of use.  The ray
// multiplier depends on the pixel and the intrinsics alone: it is not staged per frame, the integrate gathers it from
// the volume's one table (vol->mult, IntegrateParams::mult), and only on the lanes that can update.
// depth: u16 path converted exactly as Image::ConvertDepthToFloatImage; float path copied.
__device__ inline float prep_depth(float scale, double trunc, uint32_t raw16) {
    float dv = (float)raw16;
    dv = dv / scale;
    if ((double)dv >= trunc) dv = 0.0f;
    return dv;
}
__device__ inline float prep_depth(const BatchFrame& fr, uint32_t raw16) { return prep_depth(fr.scale, fr.trunc, raw16); }

// the staged records of 4 consecutive pixels (depths d, the 12 colour bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3 as
// three words; zeros without colour): two 16-B stores
__device__ inline void store_quad(uint2* dc, float d0, float d1, float d2, float d3, uint32_t w0, uint32_t w1,
                                  uint32_t w2) {
    const uint32_t p0 = w0 & 0xFFFFFFu;
    const uint32_t p1 = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
    const uint32_t p2 = (w1 >> 16) | ((w2 & 0xFFu) << 16);
    const uint32_t p3 = w2 >> 8;
    uint4* q = reinterpret_cast<uint4*>(dc);
    q[0] = make_uint4(__float_as_uint(d0), p0, __float_as_uint(d1), p1);
    q[1] = make_uint4(__float_as_uint(d2), p2, __float_as_uint(d3), p3);
}

// 4 pixels per lane: 8-B depth load, 12-B colour load (3 aligned dwords), 2 x 16-B (depth, colour) stores.
__device__ inline void prep_quad(const BatchFrame& fr, int64_t i0, int64_t npx) {
    const bool aligned = ((reinterpret_cast<uintptr_t>(fr.depth16) & 7) == 0) &&
                         ((reinterpret_cast<uintptr_t>(fr.depthf) & 15) == 0) &&
                         ((reinterpret_cast<uintptr_t>(fr.color) & 3) == 0);
    if (aligned && i0 + 4 <= npx && (npx & 3) == 0) {
        float d[4];
        if (fr.depth16) {
            const uint2 raw = *reinterpret_cast<const uint2*>(fr.depth16 + i0);
            d[0] = prep_depth(fr, raw.x & 0xFFFFu);
            d[1] = prep_depth(fr, raw.x >> 16);
            d[2] = prep_depth(fr, raw.y & 0xFFFFu);
            d[3] = prep_depth(fr, raw.y >> 16);
        } else {
            const float4 v = *reinterpret_cast<const float4*>(fr.depthf + i0);
            d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        }
        uint32_t w0 = 0u, w1 = 0u, w2 = 0u;  // colour loaded before the stores (char data may alias them)
        if (fr.color) {
            const uint32_t* c = reinterpret_cast<const uint32_t*>(fr.color + i0 * 3);  // 12 B, 4-B aligned
            w0 = c[0], w1 = c[1], w2 = c[2];
        }
        store_quad(fr.dc + i0, d[0], d[1], d[2], d[3], w0, w1, w2);
    } else {
        for (int64_t i = i0; i < npx && i < i0 + 4; ++i) {
            const float dv = fr.depth16 ? prep_depth(fr, fr.depth16[i]) : fr.depthf[i];
            uint32_t cw = 0u;
            if (fr.color) {
                const uint8_t* c = fr.color + i * 3;
                cw = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16);
            }
            fr.dc[i] = make_uint2(__float_as_uint(dv), cw);
        }
    }
}

// Quads [q, q1) with stride 256 (one lane's share of a chunk): on the common path (u16 depth, RGB8, aligned, W*H
// a multiple of 4) PREP_K quads per step with all of their loads issued before any store.
constexpr int PREP_K = 2;  // 3 or 4 (more VGPRs, fewer resident touch waves): step +2-3 %
__device__ inline void prep_range(const BatchFrame& fr, int64_t q, int64_t q1, int64_t npx) {
    const bool fast = fr.depth16 && fr.color && (npx & 3) == 0 &&
                      ((reinterpret_cast<uintptr_t>(fr.depth16) & 7) == 0) &&
                      ((reinterpret_cast<uintptr_t>(fr.color) & 3) == 0);
    if (fast) {
        for (; q + 256 * (PREP_K - 1) < q1; q += 256 * PREP_K) {
            uint2 raw[PREP_K];
            uint32_t w[PREP_K][3];
#pragma unroll
            for (int k = 0; k < PREP_K; ++k) {
                const int64_t i0 = (q + 256 * k) * 4;
                raw[k] = *reinterpret_cast<const uint2*>(fr.depth16 + i0);
                const uint32_t* c = reinterpret_cast<const uint32_t*>(fr.color + i0 * 3);
                w[k][0] = c[0], w[k][1] = c[1], w[k][2] = c[2];
            }
#pragma unroll
            for (int k = 0; k < PREP_K; ++k) {
                const int64_t i0 = (q + 256 * k) * 4;
                const float d0 = prep_depth(fr, raw[k].x & 0xFFFFu), d1 = prep_depth(fr, raw[k].x >> 16);
                const float d2 = prep_depth(fr, raw[k].y & 0xFFFFu), d3 = prep_depth(fr, raw[k].y >> 16);
                store_quad(fr.dc + i0, d0, d1, d2, d3, w[k][0], w[k][1], w[k][2]);
            }
        }
    }
    for (; q < q1; q += 256) prep_quad(fr, q * 4, npx);
}

// lanes of k_copy_frames' one workgroup (tsdf_frontend.hip): a batch's per-frame parameters, up to two 16-B words a lane
static_assert(sizeof(BatchFrame) % 16 == 0, "BatchFrame is copied in 16-B words");
constexpr int COPY_FRAMES_LANES = 1024;
static_assert(sizeof(BatchFrame) / 16 * MAX_BATCH <= 2 * COPY_FRAMES_LANES, "two words per lane");

// The tile-max depth map of a frame (slice_pretest.h): eight lanes own a PRE_TILE x PRE_TILE pixel tile, one row each
// (lane-rows i0, i0 + step, ...: i0 and step are multiples of 8 apart from the lane's own 3 bits, so a tile's eight lanes
// run together), combine over the group and store the tile's word -- no atomics, and every word of the map is written
// by every batch, so nothing is cleared.  The values are the staged ones (prep_depth of the same raw depth: the
// staging's own stores may not be visible yet).  u16 depth: prep_depth is monotone in the raw value up to the
// truncation, so the tile's largest raw value decides with one conversion unless the truncation removed it; then, and
// for float depth or a width that is no multiple of the tile, pixel by pixel.
// Not inlined: inside the touch kernel it took that kernel from 78 to 82 VGPRs, a wave per SIMD off its occupancy.
__device__ inline unsigned group8_max(unsigned v) {
    v = max(v, (unsigned)__shfl_xor((int)v, 1));
    v = max(v, (unsigned)__shfl_xor((int)v, 2));
    return max(v, (unsigned)__shfl_xor((int)v, 4));
}
__device__ __noinline__ void tile_max_range(const BatchFrame& fr, unsigned* __restrict__ map, int W, int H, int i0,
                                            int step) {
    const int tmx = pre_tiles(W), total = tmx * pre_tiles(H) * PRE_TILE;
    const bool rows16 = fr.depth16 && (W & 7) == 0 && (reinterpret_cast<uintptr_t>(fr.depth16) & 15) == 0;
    for (int i = i0; i < total; i += step) {  // (total is a multiple of 8: a group is in or out as one)
        const int t = i >> 3, y = (t / tmx) * PRE_TILE + (i & 7), x0 = (t % tmx) * PRE_TILE;
        const int cols = min(PRE_TILE, W - x0);
        const bool inside = y < H;  // (a ragged tile's rows past the image hold nothing)
        unsigned key = 0u;
        bool done = false;  // the same for a tile's eight lanes
        if (rows16) {  // (cols == PRE_TILE) the row is one aligned 16-B load
            unsigned m = 0u;
            if (inside) {
                const uint4 v = *reinterpret_cast<const uint4*>(fr.depth16 + (int64_t)y * W + x0);
                const unsigned w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) m = max(m, max(w4[k] & 0xFFFFu, w4[k] >> 16));
            }
            m = group8_max(m);
            const float d = prep_depth(fr, m);
            done = m == 0u || d > 0.0f;
            key = pre_depth_key(d);
        }
        if (!done) {
            key = 0u;
            if (inside)
                for (int c = 0; c < cols; ++c) {
                    const int64_t px = (int64_t)y * W + x0 + c;
                    key = max(key, pre_depth_key(fr.depth16 ? prep_depth(fr, fr.depth16[px]) : fr.depthf[px]));
                }
            key = group8_max(key);
        }
        if ((i & 7) == 0) map[t] = key;
    }
}

// Staging and map in one pass (u16 depth in 16-B aligned rows of whole tiles, colour absent or 4-B aligned:
// stage_onepass): the frame is staged in tile order and a tile's word is the largest pre_depth_key of the CONVERTED
// depths its lanes hold, so the raw depth is read once and the truncation needs no second look.  A wave takes a strip of
// eight consecutive tiles, 16 quads wide and 8 rows high, a lane two quads of it: lane-quad i has bits 0..3 the quad of
// the row (bit 0 the half of the tile), bits 4..5 the row r, the rest the strip, and the lane stages rows r and r + 4 --
// per row as prep_quad does (8-B depth load, 12 B of colour, two 16-B stores), both rows' loads issued before the first
// store.  Sixteen adjacent lanes read 128 B of depth and 192 B of colour and write 512 B of one image row, the
// pattern of the chunked staging (a lane per tile row, 16 B of depth and four 16-B stores 64 B apart, was 12 us per
// batch slower: DESIGN.md 4.3).  A tile's eight lanes (1, 16 and 32 apart) share a wave: i0 and step are multiples of
// 64 apart from the lane's own 6 bits, and the strips' lane-quads in all a multiple of 64.  Rows past H are not stored
// and count 0, and neither are the tiles past the frame's last (a last strip of fewer than eight); their lanes load the
// nearest row or tile inside instead, so the loads stay straight-line code.  The accesses are global_, not flat_: the
// pointers come out of BatchFrame in memory with no address space, and a flat access also waits on the LDS counter.
// Not inlined, as tile_max_range: inside the touch kernel it took that kernel from 79 to 86 VGPRs.
typedef const uint32_t __attribute__((address_space(1))) * gc_u32;
typedef u32x4 __attribute__((address_space(1))) * g_u32x4;
typedef unsigned __attribute__((address_space(1))) * g_u32;
__device__ inline bool stage_onepass(const BatchFrame& fr, int W) {
    return fr.depth16 && (reinterpret_cast<uintptr_t>(fr.depth16) & 15) == 0 && (W & 7) == 0 &&
           (reinterpret_cast<uintptr_t>(fr.color) & 3) == 0;
}
typedef const u32x2 __attribute__((address_space(1))) * gc_u32x2;
__device__ __noinline__ void stage_tile_quads(const BatchFrame& fr, unsigned* map, int W, int H, int i0, int step) {
    const int tmx = W >> 3, ntiles = tmx * pre_tiles(H), total = ((ntiles + 7) >> 3) * 64;
    const BatchFrame __attribute__((address_space(1)))* g = (const BatchFrame __attribute__((address_space(1)))*)&fr;
    const uint16_t* depth = g->depth16;
    const uint8_t* color = g->color;
    uint2* dc = g->dc;
    const float scale = g->scale;  // (read once: the stores below may alias the frame's parameters)
    const double trunc = g->trunc;
    for (int i = i0; i < total; i += step) {  // (a wave is in or out as one)
        const int c = i & 15, t = (i >> 6) * 8 + (c >> 1), tc = min(t, ntiles - 1);
        const int ty = tc / tmx, y = ty * PRE_TILE + ((i >> 4) & 3), x = (tc - ty * tmx) * PRE_TILE + (c & 1) * 4;
        const int rows = t < ntiles ? (y + 4 < H ? 2 : y < H ? 1 : 0) : 0;  // of the lane's two, those inside the image
        // every lane loads (a row past the image or a tile past the last: the nearest one inside, and nothing stored),
        // so the loads are straight-line code, all in flight before the first store
        int64_t px[2];
        u32x2 raw[2];
        uint32_t w[2][3] = {{0u, 0u, 0u}, {0u, 0u, 0u}};  // colour loaded before the stores (char data may alias them)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            px[k] = (int64_t)min(y + 4 * k, H - 1) * W + x;
            raw[k] = *(gc_u32x2)(depth + px[k]);
        }
        if (color) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                gc_u32 cw = (gc_u32)(color + px[k] * 3);  // 12 B, 4-B aligned
                w[k][0] = cw[0], w[k][1] = cw[1], w[k][2] = cw[2];
            }
        }
        unsigned key = 0u;
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (k < rows) {  // as store_quad
                const float d0 = prep_depth(scale, trunc, raw[k].x & 0xFFFFu), d1 = prep_depth(scale, trunc, raw[k].x >> 16);
                const float d2 = prep_depth(scale, trunc, raw[k].y & 0xFFFFu), d3 = prep_depth(scale, trunc, raw[k].y >> 16);
                const uint32_t w0 = w[k][0], w1 = w[k][1], w2 = w[k][2];
                g_u32x4 out = (g_u32x4)(dc + px[k]);
                out[0] = u32x4{__float_as_uint(d0), w0 & 0xFFFFFFu, __float_as_uint(d1), (w0 >> 24) | ((w1 & 0xFFFFu) << 8)};
                out[1] = u32x4{__float_as_uint(d2), (w1 >> 16) | ((w2 & 0xFFu) << 16), __float_as_uint(d3), w2 >> 8};
                key = max(max(key, max(pre_depth_key(d0), pre_depth_key(d1))),
                          max(pre_depth_key(d2), pre_depth_key(d3)));
            }
        key = max(key, (unsigned)__shfl_xor((int)key, 1));
        key = max(key, (unsigned)__shfl_xor((int)key, 16));
        key = max(key, (unsigned)__shfl_xor((int)key, 32));
        if ((i & 0x31) == 0 && t < ntiles) *(g_u32)(map + t) = key;
    }
}

// staging share `part` of `parts` of the pixels of frame group `grp`, and of the tiles of their tile-max maps
__device__ inline void stage_share(const BatchFrame* __restrict__ frames, const BatchTouchParams& p, int nframes,
                                   int grp, int part, int parts) {
    const int64_t quads = (p.npx + 3) >> 2;
    const int64_t per = (quads + parts - 1) / parts;
    const int64_t q0 = (int64_t)part * per, q1 = q0 + per < quads ? q0 + per : quads;
    for (int f = grp * p.tf; f < grp * p.tf + p.tf && f < nframes; ++f) {
        if (p.tmax && p.onepass && stage_onepass(frames[f], p.W)) {  // workgroup-uniform
            unsigned* map = p.tmax + (size_t)f * (pre_tiles(p.W) * pre_tiles(p.H));
            stage_tile_quads(frames[f], map, p.W, p.H, part * 256 + (int)threadIdx.x, parts * 256);
            continue;
        }
        prep_range(frames[f], q0 + threadIdx.x, q1, p.npx);
        if (p.tmax)
            tile_max_range(frames[f], p.tmax + (size_t)f * (pre_tiles(p.W) * pre_tiles(p.H)), p.W, p.H,
                           part * 256 + (int)threadIdx.x, parts * 256);
    }
}

}  // namespace ot
