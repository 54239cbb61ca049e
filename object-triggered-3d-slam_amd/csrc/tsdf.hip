// tsdf.hip — ScalableTSDFVolume on MI355X: GPU block hash + block pool in HBM, batched touched-unit detection and
// temporally blocked integration.
//
// Reference semantics (Open3D ScalableTSDFVolume::Integrate and
// UniformTSDFVolume::IntegrateWithDepthToCameraDistanceMultiplier), called from
// reconstruct_rgbd_filter.py:105, reconstruct_rgbd.py:107, multi_reconstruct_rgbd_filter.py:98,
// reconstruct_rgbd_gt.py:82:
//   (i)   multiplier image m(i,j) = sqrtf(xx^2 + yy^2 + 1)                      (cached per intrinsic)
//   (ii)  stride-4 unprojection with camera_pose = inverse(extrinsic) in float64
//   (iii) touched units = union over samples of [floor((p - trunc)/L), floor((p + trunc)/L)]^3
//   (iv)  per touched unit, per voxel: project, sample depth, sdf update — all f32, z walked incrementally.
// Every flush is a batch of 1..128 frames (batch_cap; a single frame is a batch of one): k_batch_touch -> k_batch_units ->
// k_batch_integrate, below.  The unit pool is unbounded like Open3D's: when a batch needs more units than the pool
// holds, the pool and the hash grow (records copied, keys rehashed) and the batch's dropped units are integrated
// again from its staged frames (settle_batch), so the result is the one an unbounded pool gives.
// This file: the touch, units, staging and integrate kernels and the host batch pipeline that launches them
// (integrate_batch, settle_batch, grow_pool, tsdf_flush).  The unit exchange is tsdf_exchange.hip, the volume's life
// cycle, settings and read-outs tsdf_volume.hip.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <utility>

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

// ============================================================================ batched (temporal blocking)
// One launch per batch of F <= MAX_BATCH frames (128 for a whole volume's direct batches, else 64: batch_cap):
//   staging           : one 8-B record per pixel of every frame, (float depth, colour r | g << 8 | b << 16), done by
//                       k_batch_touch's workgroups (each stages a contiguous pixel chunk of its frames)
//   k_batch_touch     : stride samples of every frame; a unit touched by frame f gets bit f & 63 in word f >> 6 of its
//                       slot's fmask (64-bit atomicOr); the batch's first touch of a unit appends the slot to bslots
//                       (touch_slot: the word's first bits, and in a batch of both words the slot's claim)
//   k_batch_units     : per touched slot: allocate the unit if new, move its two mask words into a 32-B header
//   k_batch_integrate : persistent independent waves over (unit, slice) items: a slice's 64 x BZ voxels are
//                       loaded into registers (5 x BZ VGPRs/lane), the batch's frames are applied in call order
//                       (ascending bits of the mask) and the state is written back once.  Per-voxel arithmetic is
//                       the per-frame path's, so results are bit-identical to integrating frame by frame.
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

// The batch's per-frame parameters from the pinned host staging into device memory: one small kernel reading host
// memory instead of a copy command (the runtime's blit copy cost ~5 us of host API time and left the stream idle ~4 us
// behind it, on every batch's critical path: one object's timeline, r05m).  Up to two 16-B words per lane (the second
// only past 78 frames), both loaded before either is stored, so every PCIe read is in flight at once (a 256-lane loop
// took 8.4 us: four round trips, r05n)
static_assert(sizeof(BatchFrame) % 16 == 0, "BatchFrame is copied in 16-B words");
constexpr int COPY_FRAMES_LANES = 1024;
static_assert(sizeof(BatchFrame) / 16 * MAX_BATCH <= 2 * COPY_FRAMES_LANES, "two words per lane");
__global__ __launch_bounds__(COPY_FRAMES_LANES) void k_copy_frames(const uint4* __restrict__ src,
                                                                   uint4* __restrict__ dst, int n16) {
    const int i = threadIdx.x, j = i + COPY_FRAMES_LANES;
    uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
    if (i < n16) a = src[i];
    if (j < n16) b = src[j];
    if (i < n16) dst[i] = a;
    if (j < n16) dst[j] = b;
}

// floor(RN(a / b)) -- Open3D's LocateVolumeUnit on a float64 quotient -- with one multiply in the common case: v =
// RN(a * RN(1/b)) is within 2^-52 |a/b| of a/b (and RN(a/b) within 2^-53), so when v lies farther than 1e-14 |v| (+ an
// absolute floor far below any unit index) from every integer, floor(v) is floor(RN(a/b)); otherwise the IEEE division.
__device__ inline int floor_div(double a, double b, double inv_b) {
    const double v = a * inv_b;
    const double fv = floor(v);
    const double eps = 1e-14 * fabs(v) + 1e-300;
    if (v - fv > eps && (fv + 1.0) - v > eps) return (int)fv;
    return (int)floor(a / b);
}

// Bits `bits` of the mask word of frame f of `slot`; true: this call lists the slot in bslots (the batch's first touch
// of the unit).  WIDE: the batch has frames in both words, and the first touch of a word draws the slot's claim
// (tsdf.h).  !WIDE (a batch of at most WORD_FRAMES frames: every sharded, split, fused and deferred batch): word 0 alone
// and no claim, the single atomicOr a one-word mask takes.
template <bool WIDE>
__device__ inline bool touch_slot(const TsdfDev& d, int slot, int f, unsigned long long bits) {
    if constexpr (WIDE) {
        if (atomicOr(&d.fmask[(unsigned)slot * FMASK_STRIDE + (f >> 6)], bits) != 0ull) return false;
        return atomicExch(&d.fmask[(unsigned)slot * FMASK_STRIDE + FMASK_CLAIM], 1ull) == 0ull;
    } else {
        return atomicOr(&d.fmask[(unsigned)slot * FMASK_STRIDE], bits) == 0ull;
    }
}

template <bool WIDE>
__device__ inline void touch_unit_batch(const TsdfDev& d, int f, int slot_cap, int pc, int x, int y, int z) {
    if (!key_in_range(x, y, z)) {
        atomicOr(&d.counters[C_HASHERR], 2);
        return;
    }
    const unsigned long long key = pack_key(x, y, z);
    if (!unit_owned(d, key)) return;
    const int slot = hash_insert(d, key);
    if (slot < 0) {
        atomicOr(&d.counters[C_HASHERR], 1);
        return;
    }
    const unsigned long long bit = 1ull << (WIDE ? f & 63 : f);
    // fast path; a stale read only costs the atomic below
    if (d.fmask[(unsigned)slot * FMASK_STRIDE + (WIDE ? f >> 6 : 0)] & bit) return;
    if (touch_slot<WIDE>(d, slot, f, bit)) {
        const int pos = atomicAdd(&d.counters[pc], 1);
        if (pos < slot_cap) d.bslots[pos] = slot;
        else atomicOr(&d.counters[C_HASHERR], 1);
    }
}

// Touch pass with LDS de-duplication.  A workgroup owns a 16x16 tile of stride samples and a group of TF frames;
// each (unit key, frame) hit is first merged into an LDS table (key -> frame bitmask, 64-bit LDS atomics), then
// every distinct unit of the tile does ONE global hash insert + ONE atomicOr of its merged mask.  A key that does
// not fit the LDS table falls back to the direct global path.
constexpr int TT = 16;          // tile edge in samples
// frames per workgroup: 2 since the staging-only workgroups (r05au / r05av, tools/touch_stage_ab.py: unsharded step
// within 0.2 % of 4, a rank of 8 shards 3 % faster -- front end 99 vs 105 us per batch; 8: +10 %); with every touch
// workgroup staging a share first, 4 was 1 % faster than 2 (round 3)
constexpr int TF = 2;
constexpr int LTAB = 1024;   // LDS table entries (16 B each + a 4-B slot in the list of used entries)

// Frame groups: group g is frames g tf ... g tf + tf - 1.  A group's frames lie in one mask word, so a touch workgroup's
// LDS masks stay 64-bit and it merges them with one atomicOr: a batch of more than WORD_FRAMES frames takes a group size
// that divides WORD_FRAMES (touch_group_frames, on the host; TF = 2 does).
static int touch_group_frames(int tf, int n) {
    while (n > WORD_FRAMES && WORD_FRAMES % tf) --tf;
    return tf;
}

__device__ inline bool lds_merge(unsigned long long* keys, unsigned long long* masks, unsigned short* used, int* nused,
                                 unsigned long long key, unsigned long long bit) {
    unsigned h = (unsigned)mix64(key) & (LTAB - 1);
    for (int probe = 0; probe < 64; ++probe) {
        unsigned long long k = keys[h];
        if (k == KEY_EMPTY) {
            const unsigned long long old = atomicCAS(&keys[h], KEY_EMPTY, key);
            if (old == KEY_EMPTY) used[atomicAdd(nused, 1)] = (unsigned short)h;  // the inserting lane lists the entry
            k = (old == KEY_EMPTY) ? key : old;
        }
        if (k == key) {
            atomicOr(&masks[h], bit);
            return true;
        }
        h = (h + 1) & (LTAB - 1);
    }
    return false;
}

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

// Staging (every pixel of the batch: HBM streaming) and the touch (stride samples: LDS merges and global hash atomics)
// as separate workgroups: stage_blocks > 0 staging-only workgroups follow each frame group's touch tiles in the grid
// (blockIdx.x >= tiles), so the touches' global atomics are spread over the time the staging streams.  Measured
// (tools/touch_stage_ab.py, front end per 64-frame batch): every touch workgroup staging a share first (stage_blocks 0,
// the round-4 form) 115 us, 1 / 2 / 4 / 8 staging workgroups per tile 120 / 111 / 112 / 122 us (r05aq, r05ar: step
// -1.2 % at 2); all touch workgroups dispatched first and the staging after them 123-128 us (r05as: the touches'
// atomics then contend at once).  The touch reads raw depth itself, so nothing in it waits on the staging stores.
// Every rank of a spatially sharded volume stages every pixel: integrating from the raw frames instead (a u16 depth +
// a multiplier-table gather per voxel visit) made the integrate 1.9x slower per unit (round 4,
// tools/shard_frontend.py), more than the staging it saves.
// REPLAY (settle_batch, after the pool grew): the batch's touch again from its STAGED depths (the caller's frames may be
// gone by then; the staged depth is exactly the value the first pass computed from them), no staging.
// LDS of one touch workgroup (k_batch_touch, and the touch half of k_integrate_touch)
struct TouchLds {
    unsigned long long keys[LTAB];
    unsigned long long masks[LTAB];
    unsigned short used[LTAB];  // 16-bit entry indices: 18 KiB in all, so 8 workgroups fit a CU's 160 KiB
    int nused;
};
// STAGE: the staging code paths (stage_blocks >= 0) are compiled in; the split front end's touch has none (the touch half
// of k_integrate_touch: without them it fits 64 VGPRs instead of 96)
// WIDE: the batch may have more than WORD_FRAMES frames (touch_slot); the host launches that form for such a batch only
template <bool REPLAY, bool STAGE = !REPLAY, bool WIDE = false>
__device__ __forceinline__ void touch_body(const BatchFrame* __restrict__ frames, const BatchTouchParams& p,
                                           const TsdfDev& d, int nframes, TouchLds& L, int tile, int grp) {
    unsigned long long* s_keys = L.keys;
    unsigned long long* s_masks = L.masks;
    unsigned short* s_used = L.used;
    int& s_nused = L.nused;
    const int tid = threadIdx.x;
    if constexpr (STAGE) {
        if (p.stage_blocks > 0 && tile >= p.tiles) {  // block-uniform
            stage_share(frames, p, nframes, grp, tile - p.tiles, p.stage_blocks);
            return;
        }
    }
    for (int e = tid; e < LTAB; e += 256) {
        s_keys[e] = KEY_EMPTY;
        s_masks[e] = 0ull;
    }
    if (tid == 0) s_nused = 0;
    // (stage_blocks 0) this touch workgroup also stages a contiguous 1/tiles of its frames' pixels
    if constexpr (STAGE) {
        if (p.stage_blocks == 0) stage_share(frames, p, nframes, grp, tile, p.tiles);
    }
    __syncthreads();
    const int tiles_x = (p.ws + TT - 1) / TT;
    const int sx = (tile % tiles_x) * TT + (tid & (TT - 1));
    const int sy = (tile / tiles_x) * TT + (tid / TT);
    const int f0 = grp * p.tf;  // (the group's frames share a mask word: touch_group_frames)
    if (sx < p.ws && sy < p.hs) {
        const int r = sy * p.stride, c = sx * p.stride;
        for (int f = f0; f < f0 + p.tf && f < nframes; ++f) {
            const BatchFrame& fr = frames[f];
            const int64_t pix = (int64_t)r * p.W + c;  // the staged depth, computed as the staging does
            const float df = REPLAY           ? __uint_as_float(fr.dc[pix].x)
                             : fr.depth16 ? prep_depth(fr, fr.depth16[pix])
                                          : fr.depthf[pix];
            if constexpr (!REPLAY) {
                if (p.sample_stage) {  // what the staging writes there
                    uint32_t cw = 0u;
                    if (fr.color) {
                        const uint8_t* c = fr.color + pix * 3;
                        cw = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16);
                    }
                    fr.dc[pix] = make_uint2(__float_as_uint(df), cw);
                }
            }
            if (!(df > 0.0f)) continue;
            const double z = (double)df;
            const double x = ((double)c - p.cx) * z / p.fx;
            const double y = ((double)r - p.cy) * z / p.fy;
            double q[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double a = fr.pose[k * 4 + 0] * x;
                const double b = fr.pose[k * 4 + 1] * y;
                const double cc = fr.pose[k * 4 + 2] * z;
                q[k] = ((a + b) + cc) + fr.pose[k * 4 + 3];
            }
            int lo[3], hi[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                lo[k] = floor_div(q[k] - p.trunc, p.unit_len, p.inv_unit);
                hi[k] = floor_div(q[k] + p.trunc, p.unit_len, p.inv_unit);
            }
            const unsigned long long bit = 1ull << (WIDE ? f & 63 : f);
            for (int ux = lo[0]; ux <= hi[0]; ++ux)
                for (int uy = lo[1]; uy <= hi[1]; ++uy)
                    for (int uz = lo[2]; uz <= hi[2]; ++uz) {
                        if (!key_in_range(ux, uy, uz)) {
                            atomicOr(&d.counters[C_HASHERR], 2);
                            continue;
                        }
                        const unsigned long long key = pack_key(ux, uy, uz);
                        if (!unit_owned(d, key)) continue;
                        if (!lds_merge(s_keys, s_masks, s_used, &s_nused, key, bit))
                            touch_unit_batch<WIDE>(d, f, p.slot_cap, p.pc, ux, uy, uz);
                    }
        }
    }
    __syncthreads();
    // only the entries this tile filled (listed by their inserting lanes), not the whole table
    // The slots this batch touches first get a place in its list through ONE counter atomic per wave (ballot, the
    // first such lane adds the wave's count, each lane takes its rank): a batch's thousands of first touches on one
    // counter word no longer serialise in L2 one lane at a time
    const int nused = s_nused;
    for (int t0 = 0; t0 < nused; t0 += 256) {  // block-uniform trip count: every lane reaches the ballot
        const int t = t0 + tid;
        bool fresh = false;
        int slot = -1;
        if (t < nused) {
            const int e = s_used[t];
            slot = hash_insert(d, s_keys[e]);
            if (slot < 0) {
                atomicOr(&d.counters[C_HASHERR], 1);
            } else {
                // no read of the mask first: another frame group's workgroup set the unit's other bits, so the
                // bits are almost never all present, and the read was one more dependent global round trip on
                // every tile's chain (front end 112 -> 104 us per 64-frame batch, r05ax)
                fresh = touch_slot<WIDE>(d, slot, f0, s_masks[e]);
            }
        }
        int cnt;
        const int rank = wave_excl_count(fresh, cnt);
        if (cnt) {  // wave-uniform
            const int leader = __ffsll((long long)__ballot(fresh)) - 1;
            int base = 0;
            if ((int)lane_id() == leader) base = atomicAdd(&d.counters[p.pc], cnt);
            base = __builtin_amdgcn_readlane(base, leader);
            if (fresh) {
                const int pos = base + rank;
                if (pos < p.slot_cap) d.bslots[pos] = slot;
                else atomicOr(&d.counters[C_HASHERR], 1);
            }
        }
    }
}

template <bool REPLAY, bool WIDE>
__global__ __launch_bounds__(256) void k_batch_touch(const BatchFrame* __restrict__ frames, BatchTouchParams p,
                                                     TsdfDev d, int nframes) {
    __shared__ TouchLds lds;
    touch_body<REPLAY, !REPLAY, WIDE>(frames, p, d, nframes, lds, (int)blockIdx.x, (int)blockIdx.y);
}
// the split front end's touch (no staging paths compiled in: 69 instead of 96 VGPRs)
__global__ __launch_bounds__(256) void k_batch_touch_split(const BatchFrame* __restrict__ frames, BatchTouchParams p,
                                                           TsdfDev d, int nframes) {
    __shared__ TouchLds lds;
    touch_body<false, false>(frames, p, d, nframes, lds, (int)blockIdx.x, (int)blockIdx.y);
}

// ------------------------------------------------------------------------------------------------ integrate
// Work item = (unit, slice): a slice is one wave of 64 (x, y) columns times BZ consecutive z, so a unit is
// SLICES = 4 * (16 / BZ) independent waves.  Lane (x, y) of slice (g, h) owns z in [BZ*h, BZ*h + BZ); its
// camera-space position still advances by exactly z sequential additions of Es.col(2) from the column origin,
// as in Open3D, so every slice reproduces the single-lane z walk bit for bit.  Waves never synchronise: the
// unit header (id, key, frame mask) is resolved once by k_batch_units and read with scalar loads.
constexpr int BZ = 4;                         // voxels per lane along z (2: slower, profiles/r03w_*)
constexpr int SLICES = 4 * (UNIT_RES / BZ);   // waves per unit
// waves per workgroup of the fine and the fused integrates, and the unit of the coarse / fine rules: a quarter unit
// (measured per 32-frame launch, float64 colour: 16 waves 0.511 ms, 8 waves 0.452 ms, 4 waves 0.426 ms; float32 colour
// 0.402 / 0.383 / 0.378).  The coarse launch of its own goes down to one wave (integrate_form).
constexpr int INT_WG = 4;
constexpr int INT_PARTS = SLICES / INT_WG;  // four-wave workgroups per unit

// Unit headers of the batch: allocate new units, move and clear the frame masks (ready for the next batch).  A unit the
// pool cannot hold is dropped (id -1, C_OVERFLOW; not counted) and integrated by the replay once the pool has grown.
// REPLAY: units that already have an id were integrated by the batch's first pass: skipped (id -1, not counted).
constexpr int WORK_HEAVY_FRAMES = 32;
// a work-list position for each live lane: one atomic per wave and class (every lane of the wave calls it)
__device__ inline int work_slot(TsdfDev& d, int n, bool live, bool heavy) {
    int nh, nl;
    const int rh = wave_excl_count(live && heavy, nh), rl = wave_excl_count(live && !heavy, nl);
    int bh = 0, bl = 0;
    if (lane_id() == 0) {
        if (nh) bh = atomicAdd(&d.counters[C_ORDER_HEAVY], nh);
        if (nl) bl = atomicAdd(&d.counters[C_ORDER_LIGHT], nl);
    }
    bh = __builtin_amdgcn_readlane(bh, 0);
    bl = __builtin_amdgcn_readlane(bl, 0);
    return heavy ? bh + rh : n - 1 - (bl + rl);
}

// WIDE: the batch has frames in both mask words (the host knows: more than WORD_FRAMES frames); else word 0 alone is
// read and cleared -- nothing set the second word or the claim
template <bool REPLAY, bool WIDE>
// wcount: where the integrate reads the batch's work-list length (the pair counter itself, or -- with the front end
// double-buffered -- a per-set copy, since the next batch's units kernel zeroes the other pair counter while this
// batch's integrate may still run)
// early_mail: hmail + OT_MAIL_WORDS; its last word (MAIL_SEQ_UNITS) receives `seq` once the counters are stored
__global__ __launch_bounds__(256) void k_batch_units(TsdfDev d, UnitWork* __restrict__ work, int pc,
                                                     unsigned* __restrict__ early_mail, int* __restrict__ wcount,
                                                     unsigned seq) {
    __shared__ unsigned long long red[4];
    const int n = d.counters[pc];
    // the other counter belongs to the next batch; the previous batch's integrate (its last reader) has finished
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        d.counters[pc ^ 1] = 0;
        if (wcount) *wcount = n;
    }
    // only the workgroups that have slots take part (a batch's few thousand units need a tenth of the grid): the rest
    // leave before the done ticket below, which the last of the active ones draws
    const int active = min((int)gridDim.x, max(1, (n + 255) / 256));
    if ((int)blockIdx.x >= active) return;  // block-uniform
    unsigned long long pairs = 0;
    // the new units' key bounds (note_unit_key's counters), reduced over the wave before its atomics: a fresh volume
    // allocates thousands of units in one batch, and one atomic per unit on six shared words serialised in L2
    int kmax[3] = {0, 0, 0}, kneg[3] = {0, 0, 0};  // 0: none (the counters hold k + KEY_BIAS + 1 >= 1)
    // block-uniform trip count, so every lane reaches the wave's one allocation atomic (ballot + rank, as the touch)
    for (int t0 = blockIdx.x * 256; t0 < n; t0 += gridDim.x * 256) {
        const int t = t0 + (int)threadIdx.x;
        const bool live = t < n;
        const int slot = live ? d.bslots[t] : 0;
        int id = live ? d.hvals[slot] : 0;
        // requested with the id, ahead of the allocation atomic (the compiler keeps loads behind an atomic)
        const unsigned long long mask = live ? d.fmask[(unsigned)slot * FMASK_STRIDE] : 0ull;
        const unsigned long long mask1 = WIDE && live ? d.fmask[(unsigned)slot * FMASK_STRIDE + 1] : 0ull;
        const unsigned long long hkey = live ? d.hkeys[slot] : 0ull;
        int cnt;
        const int rank = wave_excl_count(live && id < 0, cnt);
        if (cnt) {  // wave-uniform
            const int leader = __ffsll((long long)__ballot(live && id < 0)) - 1;
            int base = 0;
            if ((int)lane_id() == leader) base = atomicAdd(&d.counters[C_UNITS], cnt);
            base = __builtin_amdgcn_readlane(base, leader);
            if (live && id < 0) id = -2 - (base + rank);  // the new id, encoded below -1 until it is checked
        }
        // the entry's place in the work list.  A spatial shard's batch is ~1.5 rounds of resident workgroups, so its
        // heavy units (seen by >= WORK_HEAVY_FRAMES of the batch's frames) go to the front and the rest to the back:
        // the integrate's workgroups (dispatched in item order) start the long items first and the short ones fill
        // the tail (8 sector ranks: 174 -> 165 us per batch).  A whole volume keeps the touch's order, whose
        // neighbouring units share staged pixels in L2 (heavy-first there: 715 -> 734 us per batch)
        const int wpos = d.shard_world > 1 ? work_slot(d, n, live, __popcll(mask) + __popcll(mask1) >= WORK_HEAVY_FRAMES) : t;
        if (!live) continue;
        d.fmask[(unsigned)slot * FMASK_STRIDE] = 0ull;
        if constexpr (WIDE) {
            d.fmask[(unsigned)slot * FMASK_STRIDE + 1] = 0ull;
            d.fmask[(unsigned)slot * FMASK_STRIDE + FMASK_CLAIM] = 0ull;
        }
        int kx, ky, kz;
        unpack_key(hkey, kx, ky, kz);
        if (id <= -2) {
            id = -2 - id;
            if (id >= d.max_units) {
                atomicOr(&d.counters[C_OVERFLOW], 1);
                id = -1;
            } else {
                d.hvals[slot] = id;
                d.unit_keys[id * 3 + 0] = kx;
                d.unit_keys[id * 3 + 1] = ky;
                d.unit_keys[id * 3 + 2] = kz;
                const int k3[3] = {kx, ky, kz};
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    kmax[a] = max(kmax[a], k3[a] + KEY_BIAS + 1);
                    kneg[a] = max(kneg[a], KEY_BIAS - k3[a] + 1);
                }
                id |= (int)0x80000000u;
            }
        } else if (REPLAY) {
            id = -1;
        }
        UnitWork w;
        w.id = id;
        w.kx = kx;
        w.ky = ky;
        w.kz = kz;
        w.mask = mask;
        w.mask1 = mask1;
        work[wpos] = w;
        if (id != -1) pairs += (unsigned long long)(__popcll(mask) + __popcll(mask1));
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        kmax[a] = wave_max(kmax[a]);
        kneg[a] = wave_max(kneg[a]);
    }
    if (lane_id() == 0) {  // before this workgroup's done ticket below: the last workgroup mails the final bounds
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (kmax[a]) atomicMax(&d.counters[C_KMAX + a], kmax[a]);
            if (kneg[a]) atomicMax(&d.counters[C_KNEG + a], kneg[a]);
        }
    }
    pairs = wave_sum(pairs);
    if (lane_id() == 0) red[threadIdx.x >> 6] = pairs;
    __syncthreads();
    __shared__ int s_last;
    if (threadIdx.x == 0) {
        const unsigned long long tot = red[0] + red[1] + red[2] + red[3];
        if (tot) atomicAdd(&d.stats[S_UNIT_INTEGRATIONS], tot);
        __threadfence();
        s_last = atomicAdd(&d.counters[C_UNITS_DONE], 1) == active - 1;
    }
    __syncthreads();
    if (s_last && threadIdx.x < 64) {  // every workgroup's counter atomics are done: wave 0 mails the final values
        if (threadIdx.x < N_COUNTERS) {
            const int v = __hip_atomic_load(&d.counters[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            early_mail[threadIdx.x] = threadIdx.x == C_UNITS_DONE ? 0u : (unsigned)v;
            // the heavy units' count (the list's front; the light ones fill the back in reverse touch order, which
            // integrate_body reads forward again) next to the length the integrate reads
            if (threadIdx.x == C_ORDER_HEAVY && wcount) wcount[2] = d.shard_world > 1 ? v : n;
            if (threadIdx.x == C_UNITS_DONE || threadIdx.x == C_ORDER_HEAVY || threadIdx.x == C_ORDER_LIGHT)
                d.counters[threadIdx.x] = 0;
        }
        __threadfence_system();  // the values reach the host before the sequence word
        if (threadIdx.x == 0)
            __hip_atomic_store(early_mail + (MAIL_SEQ_UNITS - OT_MAIL_WORDS), seq, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ------------------------------------------------------------------------------------ split front end (sharded)
// A rank of a spatially sharded volume integrates only its own units, so it reads only the pixels those units project
// to.  With sector ownership (tsdf.h unit_owner) that is a fraction of every frame (tools/shard_sector_model.py, the
// configs[1] ring scan: 0.23 of the 32x16 tiles at 8 ranks; 0.54 with hashed blocks), so the front end splits:
// touch (no staging) -> units -> k_stage_mask (the tiles each (owned unit, frame) pair can project to) -> k_stage_tiles
// (only those tiles).  The staged values are a pure function of the pixel, so staging a superset changes no bit.
constexpr int STX = 32, STY = 16;  // staging tile: 32 pixels (one 8-lane group of quads per row) x 16 rows
// Footprint of a unit in a frame: the voxel centres span the box [p(0), p(15)] per axis (the integrate's own float
// expressions for x, y = 0 and 15; z from the unit origin by 15 voxel lengths), so in exact arithmetic their projections
// lie in the projected corners' bounding box (the box is in front of the camera).  The integrate's float projection of a
// voxel differs from the exact one by < 0.02 px here (|pc| error ~6e-6 m at z >= 0.05 m); the box is widened by 2 px
// and any corner nearer than 5 cm marks the whole frame.
// One workgroup per FRAME: its threads walk the batch's work list, each unit whose frame mask has this frame's bit ORs
// its footprint's tiles into the frame's map in LDS, and the map is stored whole -- no global atomics (one per (unit,
// frame, tile row) had contended on the frames' few words: 8-18 us per batch, r06e), nothing to clear between batches.
// SM_PARTS workgroups per frame, each over every SM_PARTS-th 256-unit chunk of the list into its own map (64 workgroups
// for a 64-frame batch had left the mask kernel latency-bound: 5-8 us per batch, r06st); the staging kernel ORs them.
constexpr int SM_WORDS = 2048;  // LDS map words: tile rows * words per row (8 KiB; 16K x 16K-pixel frames)
constexpr int SM_PARTS = 4;
__global__ __launch_bounds__(256) void k_stage_mask(const BatchFrame* __restrict__ frames, StageMaskParams q,
                                                    const UnitWork* __restrict__ work, const int* __restrict__ wcount,
                                                    unsigned* __restrict__ mask) {
    __shared__ unsigned s_map[SM_WORDS];
    const int f = blockIdx.x, part = blockIdx.y;
    const int words = q.tiles_y * q.wpr;
    for (int i = threadIdx.x; i < words; i += 256) s_map[i] = 0u;
    __syncthreads();
    const int n = *wcount;
    const BatchFrame& fr = frames[f];
    for (int u = part * 256 + threadIdx.x; u < n; u += 256 * SM_PARTS) {
        const UnitWork& w = work[u];
        if (!((w.mask >> f) & 1ull)) continue;
        const float ox = (float)((double)w.kx * q.unit_len);
        const float oy = (float)((double)w.ky * q.unit_len);
        const float oz = (float)((double)w.kz * q.unit_len);
        const double xs[2] = {(double)((q.half + q.vl * 0.0f) + ox), (double)((q.half + q.vl * 15.0f) + ox)};
        const double ys[2] = {(double)((q.half + q.vl * 0.0f) + oy), (double)((q.half + q.vl * 15.0f) + oy)};
        const double zs[2] = {(double)(q.half + oz), (double)(q.half + oz) + 15.0 * (double)q.vl};
        bool full = false;
        double umin = 1e300, umax = -1e300, vmin = 1e300, vmax = -1e300;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const double px = xs[c & 1], py = ys[(c >> 1) & 1], pz = zs[c >> 2];
            double pc[3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
                pc[r] = (double)fr.E[r * 4 + 0] * px + (double)fr.E[r * 4 + 1] * py + (double)fr.E[r * 4 + 2] * pz +
                        (double)fr.E[r * 4 + 3];
            if (!(pc[2] >= 0.05)) {
                full = true;
            } else {
                const double rz = 1.0 / pc[2];
                const double uf = (double)q.fx * pc[0] * rz + (double)q.cx + 0.5;
                const double vf = (double)q.fy * pc[1] * rz + (double)q.cy + 0.5;
                umin = fmin(umin, uf), umax = fmax(umax, uf), vmin = fmin(vmin, vf), vmax = fmax(vmax, vf);
            }
        }
        int u0 = 0, u1 = q.W - 1, v0 = 0, v1 = q.H - 1;
        if (!full) {
            if (umax < -2.0 || vmax < -2.0 || umin > (double)q.W + 2.0 || vmin > (double)q.H + 2.0) continue;
            u0 = max(0, (int)floor(umin) - 2), u1 = min(q.W - 1, (int)floor(umax) + 2);
            v0 = max(0, (int)floor(vmin) - 2), v1 = min(q.H - 1, (int)floor(vmax) + 2);
            if (u0 > u1 || v0 > v1) continue;
        }
        const int tx0 = u0 / STX, tx1 = u1 / STX, ty0 = v0 / STY, ty1 = v1 / STY;
        for (int ty = ty0; ty <= ty1; ++ty)
            for (int k = tx0 >> 5; k <= (tx1 >> 5); ++k) {
                const int a = max(tx0, k * 32) - k * 32, b = min(tx1, k * 32 + 31) - k * 32;  // bits [a, b]
                const unsigned bits = (b == 31 ? ~0u : ((1u << (b + 1)) - 1u)) & ~((1u << a) - 1u);
                atomicOr(&s_map[ty * q.wpr + k], bits);
            }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < words; i += 256) mask[((size_t)f * SM_PARTS + part) * words + i] = s_map[i];
}

// Stage the marked tiles: one workgroup per (tile row, frame); its lanes take the marked tiles' quads in turn (a row of
// a 32-pixel tile is 8 quads, 9 slots when W % 4 != 0 lets a quad straddle the tile edge), so the work of a sparse row is
// spread over all 256 lanes (one wave per tile left 77 % of the waves idle: 23 us per batch, r06e).  A quad staged
// twice writes the same bytes.
constexpr int ST_MAX_TILES_X = 256;
constexpr int ST_K = 4;  // quads per lane per step on the common path
__global__ __launch_bounds__(256) void k_stage_tiles(const BatchFrame* __restrict__ frames,
                                                     const unsigned* __restrict__ mask, int W, int H, int tiles_x,
                                                     int tiles_y, int wpr, int64_t npx) {
    __shared__ int s_tx[ST_MAX_TILES_X];
    __shared__ int s_m;
    const int ty = blockIdx.x, f = blockIdx.y;
    if (threadIdx.x == 0) s_m = 0;
    __syncthreads();
    const size_t words = (size_t)tiles_y * wpr;
    const unsigned* row = mask + (size_t)f * SM_PARTS * words + (size_t)ty * wpr;
    for (int tx = threadIdx.x; tx < tiles_x; tx += 256) {
        unsigned w = 0u;
#pragma unroll
        for (int part = 0; part < SM_PARTS; ++part) w |= row[part * words + (tx >> 5)];
        if ((w >> (tx & 31)) & 1u) s_tx[atomicAdd(&s_m, 1)] = tx;
    }
    __syncthreads();
    const int m = s_m;
    if (m == 0) return;
    const int y0 = ty * STY, rows = min(H, y0 + STY) - y0;
    const int slots = (W & 3) ? STX / 4 + 1 : STX / 4;
    const int per_tile = rows * slots;
    const BatchFrame& fr = frames[f];
    const bool fast = fr.depth16 && fr.color && (npx & 3) == 0 && (W & 3) == 0 &&
                      ((reinterpret_cast<uintptr_t>(fr.depth16) & 7) == 0) &&
                      ((reinterpret_cast<uintptr_t>(fr.color) & 3) == 0);
    if (fast) {  // (u16 depth, RGB8, W % 4 == 0: every slot is a whole quad) a lane's ST_K quads' loads before any store
        const int total = m * per_tile;
        for (int i0 = threadIdx.x; i0 < total; i0 += 256 * ST_K) {
            int64_t px[ST_K];
            uint2 raw[ST_K];
            uint32_t w[ST_K][3];
#pragma unroll
            for (int k = 0; k < ST_K; ++k) {
                const int i = i0 + 256 * k;
                px[k] = -1;
                const int t = i / per_tile, rem = i - t * per_tile;
                const int r = y0 + rem / slots, x = s_tx[min(t, m - 1)] * STX + (rem - (rem / slots) * slots) * 4;
                if (i < total && x < W) {  // (the frame's last tile column may be narrower than STX)
                    px[k] = (int64_t)r * W + x;
                    raw[k] = *reinterpret_cast<const uint2*>(fr.depth16 + px[k]);
                    const uint32_t* c = reinterpret_cast<const uint32_t*>(fr.color + px[k] * 3);
                    w[k][0] = c[0], w[k][1] = c[1], w[k][2] = c[2];
                }
            }
#pragma unroll
            for (int k = 0; k < ST_K; ++k) {
                if (px[k] < 0) continue;
                const float d0 = prep_depth(fr, raw[k].x & 0xFFFFu), d1 = prep_depth(fr, raw[k].x >> 16);
                const float d2 = prep_depth(fr, raw[k].y & 0xFFFFu), d3 = prep_depth(fr, raw[k].y >> 16);
                store_quad(fr.dc + px[k], d0, d1, d2, d3, w[k][0], w[k][1], w[k][2]);
            }
        }
        return;
    }
    for (int i = threadIdx.x; i < m * per_tile; i += 256) {
        const int t = i / per_tile, rem = i - t * per_tile;
        const int r = y0 + rem / slots, kq = rem - (rem / slots) * slots;
        const int x0 = s_tx[t] * STX, x1 = min(W, x0 + STX);
        const int64_t qa = ((int64_t)r * W + x0) >> 2, qb = ((int64_t)r * W + x1 - 1) >> 2;
        if (qa + kq <= qb) prep_quad(fr, (qa + kq) * 4, npx);
    }
}

// compile-time loops over slot indices (std::integral_constant arguments): f(0), ..., f(N - 1); static_all stops at the
// first false
template <int N, class F>
__device__ __forceinline__ void static_for(F& f) {
    if constexpr (N > 0) {
        static_for<N - 1>(f);
        f(std::integral_constant<int, N - 1>{});
    }
}
template <int N, class F>
__device__ __forceinline__ bool static_all(F& f) {
    if constexpr (N == 0) {
        return true;
    } else {
        if (!static_all<N - 1>(f)) return false;
        return f(std::integral_constant<int, N - 1>{});
    }
}

// Occupancy: the integrate lives on it: 64 VGPRs, 8 waves per SIMD for both colour precisions with
// quarter-unit workgroups (float64 colour at 5 / 6 / 8 waves: 0.426 / 0.428 / 0.414 ms per 32-frame launch; the IEEE-
// division float64 kernel needs more registers and runs at 5).  Measured and settled: slices with no
// update in the batch are not written back (-1.5 %).  The (depth, colour) gathers: in the coarse loop every lane loads,
// a voxel outside the image from past the end of the frame (frame_tap<.., true>: -1.4 % of the headline step against the
// exec-masked gathers, which round 1 had measured 1.5 % better on the kernel of its time); in the fine pipeline the
// lanes outside the image issue no gather, as before.
constexpr int INT_WAVES_PER_EU = 8;
// Reciprocal table: y[n] = RN(1/n) for n in [1, RCP_N].  For b = w + 1 an integer in that range, q0 = RN(a*y),
// r = fma(-b, q0, a) (exact), q = RN(q0 + r*y) is RN(a/b) -- Markstein's theorem (y correctly rounded, q0 within one
// ulp, no underflow in r; binary32 and binary64 alike): the IEEE quotient bit for bit with 3 operations and an LDS
// load instead of the ~10-instruction division sequence.  The host takes this kernel (FAST) only while every weight
// is an integer count of updates below RCP_N (frames since reset + the batch < RCP_N) and the state comes from
// integration alone (no imported units): then |a| is 0 or far above the underflow range (tsdf: a sum of a running
// mean and a term quantised by the depth / camera-distance floats; colour: c*w + rgb >= 0 with c a mean of bytes).
// Otherwise the IEEE divisions (FAST = false: tests/test_gpu_tsdf.py::test_long_scan_crosses_reciprocal_table and
// ::test_ieee_division_kernel_after_import run both across the switch).
constexpr int RCP_N = 2048;  // at most 16 KiB (float64) / 8 KiB (float32) of LDS per workgroup (the table's first
                             // rcp_hi entries: integrate_form sizes the launch's dynamic LDS to the batch)

// Phases A and B of one frame for a lane's ZB voxels at column position (px, py, pz), slice start z0: the certified
// projections and the (depth, colour) gathers.  No voxel state is read, so the fine slices' frame pipeline issues them
// ahead of earlier frames' updates (integrate_item).
// LINE: the coarse loop's straight-line form -- the unsure lanes' exact quotients out of line behind
// one wave-uniform branch, a certified lane's image bounds from its integer pixel, and a gather by every lane, the
// voxels outside the image from past the end of the frame.  !LINE: the fine pipeline's form -- the exact quotients and
// the gathers in exec-masked regions, -1 for a voxel outside the image.
//
// A pixel index no frame has (check_frame: W * H < PIX_NONE): as an unsigned byte offset it is 2^31 into the 8-B
// records, past the end of the frame without 32-bit wrap-around (offset + access size stays below 2^32, where -1 * 8 + 8
// would wrap to 0), so the descriptor's range check answers 0 (make_rsrc).
constexpr unsigned PIX_NONE = 1u << 28;

// floor(x) as an integer, saturating, NaN -> 0: one instruction for any x (a C++ conversion is undefined out of range)
__device__ __forceinline__ int floor_to_int(float x) {
    int i;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(i) : "v"(x));
    return i;
}

template <int ZB, bool LINE>
__device__ __forceinline__ void frame_tap(const BatchFrame& fr, const IntegrateParams& p, int npx, float px, float py,
                                          float pz, int z0, int (&pixv)[ZB], float (&pcz)[ZB], float (&dv)[ZB],
                                          uint32_t (&cv)[ZB]) {
    const __amdgpu_buffer_rsrc_t dc_rsrc = make_rsrc(fr.dc, npx * 8);
    constexpr int NONE = LINE ? (int)PIX_NONE : -1;  // a voxel outside the image
    float pc[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float a = fr.E[r * 4 + 0] * px;
        const float b = fr.E[r * 4 + 1] * py;
        const float c = fr.E[r * 4 + 2] * pz;
        pc[r] = ((a + b) + c) + fr.E[r * 4 + 3];
    }
    const float es0 = fr.es[0], es1 = fr.es[1], es2 = fr.es[2];
    // wave-uniform: advance to this slice's first voxel by the same sequence of adds, ZB to a trip (z0 is a multiple
    // of ZB): one taken branch per ZB steps instead of one per step
    for (int k = 0; k < z0; k += ZB) {
#pragma unroll
        for (int j = 0; j < ZB; ++j) {
            pc[0] += es0;
            pc[1] += es1;
            pc[2] += es2;
        }
    }
    // phase A: projections of the ZB voxels
#pragma unroll
    for (int k = 0; k < ZB; ++k) {
        const float nu = pc[0] * p.fx, nv = pc[1] * p.fy;
        // Certified fast projection.  Only floor(u), floor(v) and the bound tests are used, so u = nu * rcp(z) decides
        // them exactly unless u lies within proj_eps of an integer (the bound tests 0.0001 and W - 0.0001 sit 1e-4
        // from integers); those rare lanes redo the IEEE quotients.  A NaN fails the > and is not certified.
        const float rz = __builtin_amdgcn_rcpf(pc[2]);
        float u_f = (nu * rz + p.cx) + 0.5f;
        float v_f = (nv * rz + p.cy) + 0.5f;
        if constexpr (LINE) {
            // Select form: every lane computes the mask of unsure lanes (no exec region around the rint and compare
            // steps), and the wave branches once, uniformly and seldom (0.17 % of the voxel visits are unsure at
            // 640 x 480, a tenth of a wave's voxel steps), to the exact block, which is laid out of line.  The block
            // serves this voxel step alone: merged over the wave's ZB steps it would run on a third of the wave-frames.
            const bool front = pc[2] > 0.0f;
            const bool cert = (int)(fabsf(u_f - __builtin_rintf(u_f)) > p.proj_eps) &
                              (int)(fabsf(v_f - __builtin_rintf(v_f)) > p.proj_eps);
            const bool unsure = front & !cert;
            // Bounds of a certified lane from its integer pixel.  Its u_f is farther than proj_eps from every integer
            // (so |u_f| < 2^23; infinities and NaN fail the compare), and proj_eps > 1.2e-4 + 2^-21 max(W, H) exceeds
            // both of Open3D's margins: 1e-4, and W - safe_w <= 1e-4 + ulp(W) / 2 <= 1e-4 + 2^-24 W (safe_w is
            // W - 1e-4 rounded to float).  So u_f lies neither in [0, 1e-4) nor in [safe_w, W), and
            //   u_f >= 0.0001f && u_f < safe_w  <=>  0 <= floor(u_f) < W  <=>  (unsigned)floor(u_f) < W,
            // likewise v_f and H; and the certification itself says that the exact u takes the same floor and the same
            // side of both bounds.  An unsure lane's pixel from this test is replaced below; behind the camera front
            // is false whatever the conversions gave.
            const int ui = floor_to_int(u_f), vi = floor_to_int(v_f);
            const bool ok = front & ((unsigned)ui < (unsigned)p.W) & ((unsigned)vi < (unsigned)p.H);
            int pix = ok ? (int)__umul24((unsigned)vi, (unsigned)p.W) + ui : NONE;
            if (__builtin_expect(__builtin_amdgcn_ballot_w64(unsure) != 0ull, 0)) {
                // the exact quotients take Open3D's own tests: there the slivers [0, 1e-4) and [W - 1e-4, W), which
                // floor() would place inside, are outside
                const float ue = ((nu / pc[2]) + p.cx) + 0.5f;
                const float ve = ((nv / pc[2]) + p.cy) + 0.5f;
                const bool oke = (ue >= 0.0001f) & (ue < p.safe_w) & (ve >= 0.0001f) & (ve < p.safe_h);
                const int pe = oke ? (int)__umul24((unsigned)(int)ve, (unsigned)p.W) + (int)ue : NONE;
                pix = unsure ? pe : pix;
            }
            pixv[k] = pix;
        } else {
            const bool sure = !(pc[2] > 0.0f) || ((int)(fabsf(u_f - __builtin_rintf(u_f)) > p.proj_eps) &
                                                  (int)(fabsf(v_f - __builtin_rintf(v_f)) > p.proj_eps));
            if (!sure) {
                u_f = ((nu / pc[2]) + p.cx) + 0.5f;
                v_f = ((nv / pc[2]) + p.cy) + 0.5f;
            }
            // non-short-circuit test keeps all ZB projections in one basic block
            const bool ok = (pc[2] > 0.0f) & (u_f >= 0.0001f) & (u_f < p.safe_w) & (v_f >= 0.0001f) & (v_f < p.safe_h);
            pixv[k] = ok ? (int)__umul24((unsigned)(int)v_f, (unsigned)p.W) + (int)u_f : NONE;
        }
        pcz[k] = pc[2];
        pc[0] += es0;
        pc[1] += es1;
        pc[2] += es2;
    }
    // phase B: every gather issued before any use (buffer loads: wave-uniform resource + 32-bit byte offset, no per-lane
    // 64-bit address math)
#pragma unroll
    for (int k = 0; k < ZB; ++k) {
        if constexpr (LINE) {
            // every lane loads, back to back; a voxel outside the image carries PIX_NONE: depth 0, colour 0
            const u32x2 raw = __builtin_amdgcn_raw_buffer_load_b64(dc_rsrc, (int)((unsigned)pixv[k] * 8u), 0, 0);
            dv[k] = __uint_as_float(raw.x);
            cv[k] = raw.y;
        } else {
            dv[k] = 0.0f;
            cv[k] = 0u;
            if (pixv[k] >= 0) {  // lanes projecting outside the image issue no gather
                const u32x2 raw = __builtin_amdgcn_raw_buffer_load_b64(dc_rsrc, pixv[k] * 8, 0, 0);
                dv[k] = __uint_as_float(raw.x);
                cv[k] = raw.y;
            }
        }
    }
}

// Phase C of one frame, state-independent too, in two pieces per voxel.  The test: the candidate lanes on df = d - z.
// The ray multiplier m is >= 1 and rounding is monotone, so (d - z) * m > -trunc implies d - z > -trunc: cand is a
// superset of the updating lanes and needs no m; the update's test on the product is then Open3D's.  A frame none of
// whose lanes is a candidate for any of the wave's voxels ends there for a coarse wave (integrate_frames): cand false
// already meant "select the old value" on every lane, so nothing after the test can change a voxel, the update count
// or the write-back decision.  LINE (frame_tap's): a voxel outside the image gathered depth 0 and fails dv > 0 by itself.
template <bool LINE>
__device__ __forceinline__ bool voxel_candidate(const IntegrateParams& p, int pix, float pcz, float dv, float& df) {
    df = dv - pcz;
    if constexpr (LINE) return (dv > 0.0f) & (df > -p.trunc);
    else return (pix >= 0) & (dv > 0.0f) & (df > -p.trunc);
}
// The multiplier gather (the volume's one table, not a per-frame copy), by the candidate lanes only: the gathered
// multiplier's float bits on the candidate lanes.  On the other lanes the result is not a multiplier -- SHARE (the
// coarse loop): the gather's byte offset, offset and result in one register, which the 64-VGPR float64-colour kernel
// needs; !SHARE (the fine pipeline's slots, 3-4 % faster per launch so): zero -- so df * mv may be anything there, NaN
// included; cand is false on those lanes and voxel_update only selects.  Use mv or the product outside a select on
// cand nowhere.  (A gather by every lane, the others from past the end of the table, measured no gain: DESIGN.md §4.3.)
template <bool SHARE>
__device__ __forceinline__ unsigned voxel_multiplier(const __amdgpu_buffer_rsrc_t& mult_rsrc, int pix, bool cand) {
    unsigned mv = SHARE ? (unsigned)pix * 4u : 0u;
    if (cand) mv = __builtin_amdgcn_raw_buffer_load_b32(mult_rsrc, SHARE ? (int)mv : pix * 4, 0, 0);
    return mv;
}

// Phase D for one voxel and one frame: the update of a candidate lane whose scaled distance sdf = (d - z) * m passes
// Open3D's test, in select form (identical values, no exec-mask branches).  c: the frame's packed colour at the pixel.
// The order of the floating-point operations is Open3D's, bit for bit (no contraction; the explicit fma calls are
// Markstein's correction).
template <bool C64, bool FAST, typename CT>
__device__ __forceinline__ void voxel_update(bool cand, float sdf, uint32_t c, bool use_color, const IntegrateParams& p,
                                             const float* s_r32, const double* s_r64, float& ts, float& wt, CT& cr,
                                             CT& cg, CT& cb, unsigned& upd) {
    const bool doit = cand & (sdf > -p.trunc);
    const float sv = sdf * p.trunc_inv;
    const float tn = (sv < 1.0f) ? sv : 1.0f;
    const float wv = wt;
    const float w1 = wv + 1.0f;
    const float ta = ts * wv + tn;
    float tsn;  // (tsdf * w + t) / (w + 1): the IEEE quotient, tsdf bit-exact
    // one table read per voxel for the tsdf and the colour quotients (round 3: +0.8 %)
    const double y64 = (FAST && C64) ? s_r64[(int)w1] : 0.0;
    if constexpr (FAST) {
        const float y = C64 ? (float)y64 : s_r32[(int)w1];
        const float q0 = ta * y;
        tsn = __builtin_fmaf(__builtin_fmaf(-w1, q0, ta), y, q0);
    } else {
        tsn = ta / w1;
    }
    ts = doit ? tsn : ts;
    // the colour means, selected by (update & the frame has colour): one select per lane, where a branch on the
    // wave-uniform use_color around each voxel's select cost the float64-colour frame pipeline 2-9 % per launch
    const bool docol = doit & use_color;
    if constexpr (C64) {  // Open3D: color = (color * weight + rgb) / (weight + 1.0f) in float64
        // every lane, in select form (skipping voxels without an updating lane: slower)
        const double wd = (double)wv, w1d = (double)w1;
        const double ar = cr * wd + (double)(c & 0xFFu);
        const double ag = cg * wd + (double)((c >> 8) & 0xFFu);
        const double ab = cb * wd + (double)((c >> 16) & 0xFFu);
        double nr, ng, nb;
        if constexpr (FAST) {
            const double y = y64;
            const double q0r = ar * y, q0g = ag * y, q0b = ab * y;
            nr = __builtin_fma(__builtin_fma(-w1d, q0r, ar), y, q0r);
            ng = __builtin_fma(__builtin_fma(-w1d, q0g, ag), y, q0g);
            nb = __builtin_fma(__builtin_fma(-w1d, q0b, ab), y, q0b);
        } else {
            nr = ar / w1d;
            ng = ag / w1d;
            nb = ab / w1d;
        }
        cr = docol ? nr : cr;
        cg = docol ? ng : cg;
        cb = docol ? nb : cb;
    } else {  // float32 state, one reciprocal for the three channels (|rel| <= 1e-4)
        const float rw = __builtin_amdgcn_rcpf(w1);
        const float nr = ((float)cr * wv + (float)(c & 0xFFu)) * rw;
        const float ng = ((float)cg * wv + (float)((c >> 8) & 0xFFu)) * rw;
        const float nb = ((float)cb * wv + (float)((c >> 16) & 0xFFu)) * rw;
        cr = docol ? nr : cr;
        cg = docol ? ng : cg;
        cb = docol ? nb : cb;
    }
    wt = doit ? w1 : wv;
    upd += doit ? 1u : 0u;
}

// The frames of `mask` for a coarse slice: one frame's phases A to D after the other (the unit's other waves hide the
// gathers' latency).
template <bool C64, bool FAST, int ZB, typename CT>
__device__ __forceinline__ void integrate_frames(const BatchFrame* __restrict__ frames, const IntegrateParams& p,
                                                 int npx, unsigned long long mask, float px, float py, float pz, int z0,
                                                 const float* s_r32, const double* s_r64, float (&ts)[ZB],
                                                 float (&wt)[ZB], CT (&cr)[ZB], CT (&cg)[ZB], CT (&cb)[ZB],
                                                 unsigned& upd) {
    for (unsigned long long m = mask; m; m &= m - 1) {
        const int f = __ffsll((long long)m) - 1;
        const BatchFrame& fr = frames[f];
        const bool use_color = fr.color != nullptr;
        // per-frame copies of the voxel column's position: the compiler pairs the rows' products (packed float32 math)
        // and would otherwise keep px, py, pz duplicated in register pairs across the whole frame loop (8 VGPRs for 3
        // values: the float64-colour kernel then spills)
        float fpx = px, fpy = py, fpz = pz;
        asm volatile("" : "+v"(fpx), "+v"(fpy), "+v"(fpz));
        int pixv[ZB];
        float pcz[ZB], dv[ZB], df[ZB];
        uint32_t cv[ZB];
        bool cand[ZB];
        unsigned mv[ZB];
        frame_tap<ZB, true>(fr, p, npx, fpx, fpy, fpz, z0, pixv, pcz, dv, cv);
        bool some = false;
#pragma unroll
        for (int k = 0; k < ZB; ++k) some |= cand[k] = voxel_candidate<true>(p, pixv[k], pcz[k], dv[k], df[k]);
        // an idle wave-frame (no candidate lane: the surface is elsewhere in this frame, or its depth is missing) leaves
        // before the multiplier gathers, the reciprocal reads and the updates -- the loop's one new uniform branch, a
        // scalar compare of the lane mask
        if (__builtin_amdgcn_ballot_w64(some) == 0ull) continue;
        const __amdgpu_buffer_rsrc_t mult_rsrc = make_rsrc(p.mult, npx * 4);
#pragma unroll
        for (int k = 0; k < ZB; ++k) mv[k] = voxel_multiplier<true>(mult_rsrc, pixv[k], cand[k]);
        // updates in frame order
#pragma unroll
        for (int k = 0; k < ZB; ++k)
            voxel_update<C64, FAST>(cand[k], df[k] * __uint_as_float(mv[k]), cv[k], use_color, p, s_r32, s_r64, ts[k],
                                    wt[k], cr[k], cg[k], cb[k], upd);
    }
}

// The slice pre-test (slice_pretest.h), in the coarse item's prologue, once per non-empty mask word: lane f decides
// frame fb + f of the batch (`frames` is the word's first frame, frame fb; `mask` the item's mask word) from
// the slice's bounding box in that frame's image and the frame's tile-max depth map -- the map read through a buffer
// resource over the whole set's maps, so a wrong index reads 0 or another tile and cannot fault -- and the ballot is the
// frames in which no voxel of the slice can be a candidate.  Such a frame is one integrate_frames leaves at its idle
// branch with every lane selecting the old value: dropping its bit changes no voxel, no update count and no write-back
// decision.  Float64 and per-lane loops are fine here: once per item, before the voxel state is loaded.
__device__ __forceinline__ unsigned long long pretest_idle(const BatchFrame* __restrict__ frames,
                                                           const IntegrateParams& p, const UnitWork& w, int s,
                                                           int fb, unsigned long long mask) {
    // per-item copies of the lane index and the launch's constants: what derives from them alone (the frame's address,
    // float64 forms and products) would otherwise be computed before the item loop and kept through the frame loop,
    // which has no register to spare (they were spilled)
    unsigned tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int f = (int)(tid & 63u);
    bool idle = false;
    PreIntrinsics in;
    in.W = p.W, in.H = p.H, in.fx = p.fx, in.fy = p.fy, in.cx = p.cx, in.cy = p.cy;
    float vl = p.vl, trunc = p.trunc;
    double unit_len = p.unit_len;
    asm volatile("" : "+s"(in.fx), "+s"(in.fy), "+s"(in.cx), "+s"(in.cy), "+s"(vl), "+s"(trunc), "+s"(unit_len));
    asm volatile("" : "+s"(in.W), "+s"(in.H));
    if ((mask >> f) & 1ull) {
        const __amdgpu_buffer_rsrc_t map = make_rsrc(p.tmax, (p.tmax_words + PRE_SLACK) * 4);
        const int base = (fb + f) * p.tmax_tiles;
        idle = slice_idle(frames[f].E, in, vl, unit_len, w.kx, w.ky, w.kz, s, trunc, [&](int i) {
            // (PRE_NONE: 2^30 bytes or more into a buffer of fewer: the range check answers zeros)
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(map, (base + i) * 4, 0, 0);
            PreTile4 q;
            q.k[0] = v.x, q.k[1] = v.y, q.k[2] = v.z, q.k[3] = v.w;
            return q;
        });
    }
    return __builtin_amdgcn_ballot_w64(idle);
}

// One work item: slice s (this wave's) of the unit of work entry w -- its ZB voxels per lane loaded (or zero for a
// fresh unit), taken through the batch's frames of its WORDS mask words (w.mask, w.mask1, less the frames the pre-test
// dropped) and written back: the state is loaded once, word 0's frames run, then word 1's (frames 64 ..., in call
// order), and it is stored once.  ZB == 2: the fine slices (KT their pipeline's depth).
template <bool C64, bool FAST, int ZB, int KT, int WORDS>
__device__ __forceinline__ void integrate_item(const BatchFrame* __restrict__ batch, const IntegrateParams& p,
                                               const TsdfDev& d, const UnitWork& w, unsigned long long mask0,
                                               unsigned long long mask1, int s, int npx, const float* s_r32,
                                               const double* s_r64, unsigned& upd) {
    using CT = typename std::conditional<C64, double, float>::type;
    const int ent = w.id;
    if (ent == -1) return;
    const int id = ent & 0x7FFFFFFF;
    const bool fresh = ent < 0;
    // the lane's column from a per-item copy of the thread index: the compiler would otherwise hoist lane, lane >> 3 and
    // lane & 7 out of the item loop and keep them in registers through the frame loop, which has none to spare (the
    // float64-colour kernels then spill them)
    unsigned tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63;
    // wave = 8 x 8 columns: a square patch of the unit's xy plane projects to fewer pixel rows
    const int x = (s & 2) * 4 + (lane >> 3), y = (s & 1) * 8 + (lane & 7);
    const int col = x * 16 + y;
    const int z0 = (s >> 2) * ZB;
    float* base = d.vox + (size_t)id * (C64 ? UNIT_FLOATS_C64 : UNIT_FLOATS);
    // colour plane c of voxel vi: float32 planes addressed from base (one address register for the whole record: a
    // separate colour pointer costs ~34 VGPRs in this kernel), float64 through a buffer resource over the record's
    // float64 planes
    const __amdgpu_buffer_rsrc_t col64 = make_rsrc(base + 2 * UNIT_VOX, 3 * UNIT_VOX * 8);
    float ts[ZB], wt[ZB];
    CT cr[ZB], cg[ZB], cb[ZB];
#pragma unroll
    for (int k = 0; k < ZB; ++k) {
        const int vi = (z0 + k) * 256 + col;
        if (fresh) {
            ts[k] = wt[k] = 0.0f;
            cr[k] = cg[k] = cb[k] = (CT)0;
        } else {
            ts[k] = base[vi];
            wt[k] = base[UNIT_VOX + vi];
            if constexpr (C64) {
                cr[k] = ld_f64(col64, vi);
                cg[k] = ld_f64(col64, UNIT_VOX + vi);
                cb[k] = ld_f64(col64, 2 * UNIT_VOX + vi);
            } else {
                cr[k] = base[2 * UNIT_VOX + vi];
                cg[k] = base[3 * UNIT_VOX + vi];
                cb[k] = base[4 * UNIT_VOX + vi];
            }
        }
    }
    const float ox = (float)((double)w.kx * p.unit_len);
    const float oy = (float)((double)w.ky * p.unit_len);
    const float oz = (float)((double)w.kz * p.unit_len);
    const float px = (p.half + p.vl * (float)x) + ox;
    const float py = (p.half + p.vl * (float)y) + oy;
    const float pz = p.half + oz;
    unsigned iu = 0;  // this item's updates
    // one frame loop, run once per non-empty mask word (the fused launches read one word)
#pragma nounroll
    for (int word = 0; word < WORDS; ++word) {
        const unsigned long long mask = (WORDS > 1 && word) ? mask1 : mask0;
        if (WORDS > 1 && !mask) continue;
        const BatchFrame* frames = batch + word * WORD_FRAMES;  // the word's first frame
        if constexpr (ZB == 2) {
            // Frame pipeline (the fine slices serve batches with few units, whose waves cannot hide a frame's dependent
            // gathers behind other waves: the wave's chain of frames IS the batch's time).  Every load of a frame is
            // state-independent -- the projections and (depth, colour) gathers (frame_tap), the candidate test and the
            // multiplier gather (voxel_candidate, voxel_multiplier) -- only the update (voxel_update) waits for it and reads
            // the voxel state.  So frame f+KT's tap and frame f+KC's candidate stage are issued before frame f's update, from
            // KT + 1 register slots (the loop is unrolled over the slots so every slot is a fixed register set: a
            // rotating copy would wait for the loads in flight).  The updates still run in frame order with the same
            // arithmetic: the bits are the unpipelined loop's.  KT = 1, KC = 0 is the round-5 one-frame skew.
            // The pipeline stands here, not in a function of its own as the coarse loop does: with the voxel state passed
            // by reference the float64-colour kernels took 6 more VGPRs and the fused fine launch ran 5 % slower.
            constexpr int KC = KT - 1, RS = KT + 1;
            unsigned long long mt = mask;  // frames not yet tapped
            int fs[RS];                     // frame of each slot (wave-uniform), -1: past the last frame
            int pixv[RS][ZB];
            float pcz[RS][ZB], dv[RS][ZB], df[RS][ZB];
            uint32_t cv[RS][ZB];
            bool cand[RS][ZB];
            unsigned mv[RS][ZB];
            auto tap = [&](auto J) __attribute__((always_inline)) {
                constexpr int j = decltype(J)::value;
                if (mt) {
                    const int f = __ffsll((long long)mt) - 1;
                    mt &= mt - 1;
                    fs[j] = f;
                    frame_tap<ZB, false>(frames[f], p, npx, px, py, pz, z0, pixv[j], pcz[j], dv[j], cv[j]);
                } else {
                    fs[j] = -1;
                }
            };
            auto stage_c = [&](auto J) __attribute__((always_inline)) {
                constexpr int j = decltype(J)::value;
                if (fs[j] < 0) return;
                const __amdgpu_buffer_rsrc_t mult_rsrc = make_rsrc(p.mult, npx * 4);
#pragma unroll
                for (int k = 0; k < ZB; ++k) {  // test and gather voxel by voxel: no frame is left early here
                    cand[j][k] = voxel_candidate<false>(p, pixv[j][k], pcz[j][k], dv[j][k], df[j][k]);
                    mv[j][k] = voxel_multiplier<false>(mult_rsrc, pixv[j][k], cand[j][k]);
                }
            };
            auto stage_d = [&](auto J) __attribute__((always_inline)) -> bool {
                constexpr int j = decltype(J)::value;
                if (fs[j] < 0) return false;
                const bool use_color = frames[fs[j]].color != nullptr;
#pragma unroll
                for (int k = 0; k < ZB; ++k)
                    voxel_update<C64, FAST>(cand[j][k], df[j][k] * __uint_as_float(mv[j][k]), cv[j][k], use_color, p, s_r32,
                                            s_r64, ts[k], wt[k], cr[k], cg[k], cb[k], iu);
                return true;
            };
            // one iteration = frame f in slot J: the candidate stage of f + KC, the tap of f + KT (into the slot frame f - 1
            // left), the update of f.  The pipeline drains at the end of a mask word.
            auto iter = [&](auto J) __attribute__((always_inline)) -> bool {
                constexpr int j = decltype(J)::value;
                stage_c(std::integral_constant<int, (j + KC) % RS>{});
                tap(std::integral_constant<int, (j + KT) % RS>{});
                return stage_d(J);
            };
            // prologue: taps of the first KT frames, candidate stages of the first KC
            static_for<KT>(tap);
            static_for<KC>(stage_c);
            while (static_all<RS>(iter)) {
            }
        } else
            integrate_frames<C64, FAST, ZB>(frames, p, npx, mask, px, py, pz, z0, s_r32, s_r64, ts, wt, cr, cg, cb, iu);
    }
    upd += iu;
    // a slice none of whose voxels updated in this batch still holds its HBM values (fresh ones: zeros)
    if (!fresh && !__any(iu != 0u)) return;
    // the write-back's column from a second copy of the thread index, so that no voxel index lives through the frame
    // loop (with the idle-frame branch in it the fused float64 kernel spilled one)
    unsigned tidw = threadIdx.x;
    asm volatile("" : "+v"(tidw));
    const int lanew = tidw & 63;
    const int colw = ((s & 2) * 4 + (lanew >> 3)) * 16 + (s & 1) * 8 + (lanew & 7);
#pragma unroll
    for (int k = 0; k < ZB; ++k) {
        const int vi = (z0 + k) * 256 + colw;
        base[vi] = ts[k];
        base[UNIT_VOX + vi] = wt[k];
        if constexpr (C64) {
            st_f64(col64, vi, cr[k]);
            st_f64(col64, UNIT_VOX + vi, cg[k]);
            st_f64(col64, 2 * UNIT_VOX + vi, cb[k]);
        } else {
            base[2 * UNIT_VOX + vi] = cr[k];
            base[3 * UNIT_VOX + vi] = cg[k];
            base[4 * UNIT_VOX + vi] = cb[k];
        }
    }
}

// One workgroup of WG waves per unit part.  The waves of a workgroup never meet after the table's barrier, but the
// workgroup keeps its place on the CU until its slowest wave ends, and a wave behind the surface leaves every frame at
// the idle-frame branch while its neighbour does not: the smaller the workgroup, the sooner a finished wave's slot is
// refilled.  The product's coarse launch has one wave per workgroup (a sixteenth of a unit; integrate_form), the fine
// slices and the fused launches INT_WG (a quarter unit at BZ).  Per launch of the headline scan, 16 / 8 / 4 waves: 0.511
// / 0.452 / 0.426 ms (round 3); 4 / 2 / 1 waves: DESIGN.md §4.1.  The parts of a unit run on one XCD.  Work items are
// assigned by a static grid stride that every wave derives on its own: no atomics, and one barrier (the reciprocal
// table) where the workgroup has more than one wave.
// C64: colour state in float64 (Open3D's TSDFVoxel::color_ is Eigen::Vector3d), in the record's float64 planes.
// one table per kernel: float64 reciprocals for the float64-colour kernel (its float32 ones are their roundings:
// (float)RN64(1/n) == RN32(1/n) for every n <= 2^20, no double-rounding case -- tools/markstein_check.cpp), float32
// ones otherwise
template <bool C64, bool FAST>
struct RcpLds {
    float r32[(FAST && !C64) ? RCP_N + 1 : 1];
    double r64[(FAST && C64) ? RCP_N + 1 : 1];
};
// The integrate of a batch as workgroup `bid` of `nblk`: the one text behind k_batch_integrate (the product kernel) and
// the integrate half of k_integrate_touch / k_integrate_touch_fine.  Everything per item is shared (integrate_item: the
// record's load and store, the frame loops, the tap, the candidate stage, the per-voxel update, each written once
// above); the callers differ in three things only, all passed in: the workgroup's id and count (blockIdx.x /
// gridDim.x against the fused launch's split of the grid), the home of the reciprocal table (s_r32 / s_r64: the
// launch's dynamic LDS, sized to the batch, against a member of the fused kernels' LDS union) and the work-list index
// (HEAVY: the fused launch walks heavy units first, the rest back to front -- k_batch_units).  WG: waves per workgroup.
// Decision and measurements: DESIGN.md §4.2.
//
// work item = (unit, part): the PARTS parts of a unit are items 8 apart, so they run on one XCD (blocks are dealt
// round-robin over the 8 XCDs) at about the same time and share its L2's copy of the footprint.
// The grid is sized for large batches (8x the resident workgroups): a workgroup without an item leaves before
// building the reciprocal table -- for a batch of few units (a spatial shard) the idle workgroups' tables had cost
// more than the integrate itself (r05e: a 1/8 shard's 64-frame batch 165-200 us whatever its slicing)
// PRE: the launch of its own with coarse slices runs the slice pre-test when the batch has tile-max maps (p.tmax).
// WORDS: the mask words an item reads: FMASK_WORDS for the launch of its own (a whole volume's Direct batch has up to
// MAX_BATCH frames), 1 for the fused launches (their batches keep WORD_FRAMES).
template <bool C64, bool FAST, int ZB, int KT, bool HEAVY, int WG, bool PRE = false, int WORDS = 1>
__device__ __forceinline__ void integrate_body(const BatchFrame* __restrict__ frames, const IntegrateParams& p,
                                               const TsdfDev& d, const UnitWork* __restrict__ work,
                                               const int* __restrict__ wcount, float* s_r32, double* s_r64, int bid,
                                               int nblk) {
    constexpr int PARTS = 4 * (UNIT_RES / ZB) / WG;  // workgroups per unit
    {
        const int n0 = __builtin_amdgcn_readfirstlane(__hip_atomic_load(wcount, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (bid >= (PARTS == 1 ? n0 : ((n0 + 7) / 8) * 8 * PARTS)) return;
    }
    if constexpr (FAST) {
        for (int r = 1 + threadIdx.x; r <= p.rcp_hi; r += 64 * WG) {  // entries 1 .. the batch's largest weight + 1
            if constexpr (C64) s_r64[r] = 1.0 / (double)r;  // IEEE (correctly rounded) quotients
            else s_r32[r] = 1.0f / (float)r;
        }
        // a single wave's LDS operations complete in order: it needs no barrier to read what its own lanes wrote
        if constexpr (WG > 1) __syncthreads();
        else __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // once, in a scalar register
    const int n = *wcount;
    const int nh = HEAVY ? wcount[2] : 0;  // heavy units first; the rest are stored back to front (k_batch_units)
    const int npx = p.W * p.H;
    unsigned upd = 0;  // per lane: <= ZB voxels x MAX_BATCH frames x units per workgroup, far below 2^32
    unsigned dropped = 0;  // wave-uniform: wave-frames the pre-test dropped
    const int items = PARTS == 1 ? n : ((n + 7) / 8) * 8 * PARTS;
    for (int it = bid; it < items; it += nblk) {
        const int u = PARTS == 1 ? it : (it / (8 * PARTS)) * 8 + (it & 7);
        if (PARTS > 1 && u >= n) continue;
        const int part = PARTS == 1 ? 0 : (it >> 3) % PARTS;
        const int s = part * WG + wave;  // slice of this wave
        const UnitWork& w = work[!HEAVY || u < nh ? u : n - 1 - (u - nh)];
        unsigned long long mask0 = w.mask, mask1 = WORDS > 1 ? w.mask1 : 0ull;
        if constexpr (PRE) {
            if (p.tmax && w.id != -1) {  // wave-uniform
#pragma nounroll
                for (int word = 0; word < WORDS; ++word) {
                    const unsigned long long mask = word ? mask1 : mask0;
                    if (!mask) continue;
                    const unsigned long long idle =
                        pretest_idle(frames + word * WORD_FRAMES, p, w, s, word * WORD_FRAMES, mask);
                    if (word) mask1 &= ~idle;
                    else mask0 &= ~idle;
                    dropped += (unsigned)__popcll(idle);
                }
                if (!(mask0 | mask1) && w.id >= 0) continue;  // (a fresh unit still writes its zeros)
            }
        }
        integrate_item<C64, FAST, ZB, KT, WORDS>(frames, p, d, w, mask0, mask1, s, npx, s_r32, s_r64, upd);
    }
    const unsigned long long tot = wave_sum((unsigned long long)upd);
    if ((threadIdx.x & 63) == 0 && tot)
        atomicAdd(&d.stats[S_UPD_BASE + (bid & (S_DROP_LINES - 1)) * S_DROP_STRIDE], tot);
    if constexpr (PRE) {
        if ((threadIdx.x & 63) == 0 && dropped)
            atomicAdd(&d.stats[S_DROP_BASE + (bid & (S_DROP_LINES - 1)) * S_DROP_STRIDE], (unsigned long long)dropped);
    }
}

// the integrate of a batch as a launch of its own (the product kernel: <C64, FAST, BZ, 1, 1>; ZB == 2: fine slices).
// The reciprocal table is the launch's dynamic LDS: rcp_hi + 1 entries of the kernel's precision (integrate_form), so a
// CU holds as many one-wave workgroups as it has wave slots until the table passes 5 KiB.
extern __shared__ double s_rcp_dyn[];
// WORDS: the batch's mask words (2 only for a batch of more than WORD_FRAMES frames: integrate_form)
template <bool C64, bool FAST, int ZB = BZ, int KT = 1, int WG = INT_WG, int WORDS = 1>
__global__ __launch_bounds__(64 * WG, (C64 && !FAST) ? 5 : (ZB == 2 ? 4 : INT_WAVES_PER_EU)) void k_batch_integrate(
    const BatchFrame* __restrict__ frames, IntegrateParams p, TsdfDev d, const UnitWork* __restrict__ work,
    const int* __restrict__ wcount) {
    integrate_body<C64, FAST, ZB, KT, false, WG, ZB == BZ, WORDS>(frames, p, d, work, wcount,
                                                                  reinterpret_cast<float*>(s_rcp_dyn), s_rcp_dyn,
                                                                  (int)blockIdx.x, (int)gridDim.x);
}

// The deferred integrate of a sharded volume's batch k and the touch of batch k + 1 in ONE launch (round 6): workgroups
// [0, nint) integrate batch k (its set's staging and work list), the rest are batch k + 1's touch tiles (frame groups
// along the grid).  A rank's integrate fills few of the CUs (a shard's batch is a few hundred units), so its latency-bound
// touch runs in the gaps, with no second stream and no event between them (two streams' fork + join cost ~25 us of idle
// GPU per batch: the double-buffered front end).  The touch writes only batch k + 1's state: its frame
// masks / slot list / pair counter, hash inserts of its units, and the staged pixels of its samples in its own set --
// nothing the integrate of batch k reads.  LDS: the touch's tables and the reciprocal table share one block.
// The IEEE-division float64 integrate needs 67 VGPRs: it takes the 5-wave bound k_batch_integrate gives it (under the
// 8-wave bound it spilled 20-32 B inside the frame loop; per launch the two measure the same).
template <bool C64, bool FAST>
__global__ __launch_bounds__(64 * INT_WG, (C64 && !FAST) ? 5 : INT_WAVES_PER_EU) void k_integrate_touch(
    const BatchFrame* __restrict__ frames, IntegrateParams p, TsdfDev d, const UnitWork* __restrict__ work,
    const int* __restrict__ wcount, int nint, const BatchFrame* __restrict__ tframes, BatchTouchParams tp, int tn) {
    union Lds {
        TouchLds t;
        RcpLds<C64, FAST> r;
    };
    __shared__ Lds lds;
    const int b = (int)blockIdx.x;
    if (b < nint) {
        integrate_body<C64, FAST, BZ, 1, true, INT_WG>(frames, p, d, work, wcount, lds.r.r32, lds.r.r64, b, nint);
    } else {
        const int t = b - nint;
        touch_body<false, false>(tframes, tp, d, tn, lds.t, t % tp.tiles, t / tp.tiles);
    }
}
// The same launch with the integrate in fine slices (2 voxels per lane along z, k_batch_integrate<.., 2, 1>'s per-voxel
// code and occupancy): the deferred batch's unit count is known on the host by then (its units kernel mailed it), so a
// batch of few units takes the fine slices without the guess the direct path makes from the previous batch
template <bool C64, bool FAST>
__global__ __launch_bounds__(64 * INT_WG, (C64 && !FAST) ? 5 : 4) void k_integrate_touch_fine(
    const BatchFrame* __restrict__ frames, IntegrateParams p, TsdfDev d, const UnitWork* __restrict__ work,
    const int* __restrict__ wcount, int nint, const BatchFrame* __restrict__ tframes, BatchTouchParams tp, int tn) {
    union Lds {
        TouchLds t;
        RcpLds<C64, FAST> r;
    };
    __shared__ Lds lds;
    const int b = (int)blockIdx.x;
    if (b < nint) {
        integrate_body<C64, FAST, 2, 1, true, INT_WG>(frames, p, d, work, wcount, lds.r.r32, lds.r.r64, b, nint);
    } else {
        const int t = b - nint;
        touch_body<false, false>(tframes, tp, d, tn, lds.t, t % tp.tiles, t / tp.tiles);
    }
}

// ------------------------------------------------------------------------------------ host helpers
static IntegrateParams make_integrate_params(const ot_tsdf* vol, const float* depth, const uint8_t* color,
                                             const float* mult, const ot_intrinsics* in, const double* ext) {
    IntegrateParams p;
    p.depth = depth;
    p.color = (vol->color_type == OT_COLOR_RGB8) ? color : nullptr;
    p.mult = mult;
    p.W = in->width;
    p.H = in->height;
    p.fx = (float)in->fx;
    p.fy = (float)in->fy;
    p.cx = (float)in->cx;
    p.cy = (float)in->cy;
    p.inv_fx = 1.0f / (float)in->fx;
    p.inv_fy = 1.0f / (float)in->fy;
    float E[16];
    for (int k = 0; k < 16; ++k) E[k] = (float)ext[k];
    for (int k = 0; k < 12; ++k) p.E[k] = E[k];
    const double unit_voxel_length = vol->unit_length / (double)UNIT_RES;
    p.vl = (float)unit_voxel_length;
    p.half = p.vl * 0.5f;
    p.es0 = E[0 * 4 + 2] * p.vl;
    p.es1 = E[1 * 4 + 2] * p.vl;
    p.es2 = E[2 * 4 + 2] * p.vl;
    p.trunc = (float)vol->sdf_trunc;
    p.trunc_inv = 1.0f / p.trunc;
    p.safe_w = (float)in->width - 0.0001f;
    p.safe_h = (float)in->height - 0.0001f;
    // |fast u - IEEE u| <= 2^-21 (max(W, H) + 2) on [-1, W + 1] (rcp 1 ulp, four roundings); the bound tests sit
    // 1e-4 from integers, so any margin above both keeps every decision identical (see k_batch_integrate)
    p.proj_eps = (float)(std::ldexp((double)std::max(in->width, in->height) + 2.0, -21) + 1.2e-4);
    p.rcp_hi = RCP_N;  // (integrate_batch narrows it to the batch)
    p.unit_len = vol->unit_length;
    p.tmax = nullptr;  // (integrate_batch: the batch's maps, when its plan has the pre-test)
    p.tmax_tiles = p.tmax_words = 0;
    return p;
}

static ot_status launch_deferred(ot_tsdf* vol, hipStream_t stream, const BatchCtx* next);
static ot_status ensure_mult(ot_tsdf* vol, const ot_intrinsics* in, hipStream_t stream) {
    if (vol->mult_valid && std::memcmp(&vol->mult_intr, in, sizeof(ot_intrinsics)) == 0) return OT_OK;
    if (vol->mult) {
        // the integrate reads the table: a deferred batch's runs first, one on the integrate stream is waited for
        ot_status sd = launch_deferred(vol, stream, nullptr);
        if (sd != OT_OK) return sd;
        if (vol->istream) OT_HIP_TRY(hipStreamSynchronize(vol->istream));
        OT_HIP_TRY(hipStreamSynchronize(stream));
        OT_HIP_TRY(hipFree(vol->mult));
        vol->mult = nullptr;
    }
    OT_HIP_TRY(hipMalloc(&vol->mult, sizeof(float) * (size_t)in->width * in->height));
    ot_status st = ot_depth_multiplier(in, vol->mult, stream);
    if (st != OT_OK) return st;
    vol->mult_intr = *in;
    vol->mult_valid = true;
    return OT_OK;
}

static ot_status check_frame(const ot_tsdf* vol, const void* depth, const uint8_t* color, const ot_intrinsics* in,
                             const double* ext) {
    if (!vol) return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume::Integrate] volume is NULL");
    if (!depth || !in || !ext || in->width <= 0 || in->height <= 0 ||
        (vol->color_type == OT_COLOR_RGB8 && !color))
        return fail(OT_ERR_UNSUPPORTED_FORMAT, "[ScalableTSDFVolume::Integrate] Unsupported image format.");
    // the integrate's gathers address a frame by 32-bit byte offsets and send the voxels outside it to pixel PIX_NONE
    if ((int64_t)in->width * in->height >= (int64_t)PIX_NONE)
        return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume::Integrate] image of 2^28 pixels or more");
    return OT_OK;
}

// Grid of k_batch_integrate: INT_GRID_MULT x the co-resident workgroups (integrate_resident).  Measured with four-wave
// workgroups: a 64-frame batch of the configs[1] scan has ~12k (unit, quarter) items; at 8x (16k workgroups) nearly
// every workgroup takes one item and the dispatcher balances them; at 4x some take two in a static stride (0.77 vs
// 0.72 ms per launch; 6x / 12x / 16x / 32x: within 2 %, slower).  One-wave workgroups keep the ratio: 64k workgroups
// for the headline batch's 60k (unit, slice) items.
constexpr int INT_GRID_MULT = 8;

// the integrate instantiation of a batch: colour precision 64 (bit 1), reciprocal table (bit 0), fine slices (bit 2:
// 2 voxels per lane along z, 32 waves per unit instead of 16 -- for batches with few units, slice_form below);
// bits 3-4 of a fine variant: the frame pipeline's depth KT - 1 (k_batch_integrate's ZB == 2 loop)
constexpr int INT_FINE_KT = 1;
// Waves per workgroup of the coarse integrate: a finished wave frees its wave slot at once, but its
// workgroup's place on the CU only when the slowest wave ends, so the smaller the workgroup the sooner the dispatcher
// refills the slot.  The fine slices and the fused launches keep INT_WG waves.
constexpr int INT_WG_DEFAULT = 1;
template <int ZB, int KT, int WG, int WORDS>
static const void* integrate_kernels(int variant) {
    static const void* const k[4] = {(const void*)k_batch_integrate<false, false, ZB, KT, WG, WORDS>,
                                     (const void*)k_batch_integrate<false, true, ZB, KT, WG, WORDS>,
                                     (const void*)k_batch_integrate<true, false, ZB, KT, WG, WORDS>,
                                     (const void*)k_batch_integrate<true, true, ZB, KT, WG, WORDS>};
    return k[variant & 3];
}
// wg: waves per workgroup of a coarse variant (1, 2 or 4); the fine variants have INT_WG.  words: the batch's mask words
template <int WORDS>
static const void* integrate_kernel_w(int variant, int wg) {
    if (!(variant & 4))
        return wg == 1   ? integrate_kernels<BZ, 1, 1, WORDS>(variant)
               : wg == 2 ? integrate_kernels<BZ, 1, 2, WORDS>(variant)
                         : integrate_kernels<BZ, 1, 4, WORDS>(variant);
    const int kt = ((variant >> 3) & 3) + 1;
    return kt == 3   ? integrate_kernels<2, 3, INT_WG, WORDS>(variant)
           : kt == 2 ? integrate_kernels<2, 2, INT_WG, WORDS>(variant)
                     : integrate_kernels<2, 1, INT_WG, WORDS>(variant);
}
static const void* integrate_kernel(int variant, int wg, int words) {
    return words > 1 ? integrate_kernel_w<FMASK_WORDS>(variant, wg) : integrate_kernel_w<1>(variant, wg);
}

// LDS of a launch: the table's entries 0 .. rcp_hi in the variant's precision (the hardware allocates whole granules)
constexpr unsigned LDS_GRANULE = 1280;
constexpr unsigned RCP_LDS_MAX = ((RCP_N + 1) * 8 + LDS_GRANULE - 1) / LDS_GRANULE;  // in granules
static unsigned rcp_lds_bytes(int variant, int rcp_hi) {
    if (!(variant & 1)) return 0;  // IEEE divisions: no table
    const unsigned bytes = (unsigned)(std::min(std::max(rcp_hi, 1), RCP_N) + 1) * ((variant & 2) ? 8u : 4u);
    return (bytes + 15u) & ~15u;
}

// Co-resident workgroups of an integrate kernel on the device, by its waves per workgroup and its dynamic LDS in whole
// granules (cached per device, kernel and size; a benign race at worst computes the same value twice).  0: the query
// failed.
static int integrate_resident(int variant, int wg, unsigned lds, int words = 1) {
    static int cache[2][32][3][RCP_LDS_MAX + 1][64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    const unsigned granules = std::min((lds + LDS_GRANULE - 1) / LDS_GRANULE, RCP_LDS_MAX);
    int* c = &cache[words > 1][variant & 31][wg == 1 ? 0 : wg == 2 ? 1 : 2][granules][dev];
    if (!*c) {
        int per_cu = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, integrate_kernel(variant, wg, words), 64 * wg,
                                                         granules * LDS_GRANULE) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || per_cu <= 0 ||
            cus <= 0)
            return 0;
        *c = per_cu * cus;
    }
    return *c;
}

// Grid of a four-wave integrate with the whole table: INT_GRID_MULT x its co-resident workgroups.  The unit of the
// rules that choose between coarse and fine slices, and the integrate's share of a fused launch.
static int integrate_grid(int variant) {
    const int r = integrate_resident(variant, INT_WG, rcp_lds_bytes(variant, RCP_N));
    return r ? r * INT_GRID_MULT : 4096;
}

// The launch of k_batch_integrate for a batch: kernel, waves per workgroup, dynamic LDS and grid.  A coarse variant takes
// the smallest workgroup from the default up that keeps as many waves resident as four-wave workgroups would: the
// table's LDS bounds the workgroups per CU, so late in a long scan (rcp_hi towards RCP_N) one-wave workgroups would
// leave wave slots empty and the launch falls back to two and four waves.  The grid stays INT_GRID_MULT x the resident
// workgroups, so a headline batch's (unit, slice) items get one workgroup each.
struct IntForm {
    const void* fn;
    int wg, grid;
    unsigned lds;
};
static IntForm integrate_form(int variant, int rcp_hi, int words) {
    IntForm f;
    f.lds = rcp_lds_bytes(variant, rcp_hi);
    f.wg = INT_WG;
    if (!(variant & 4)) {
        const int want = integrate_resident(variant, INT_WG, f.lds, words) * INT_WG;  // waves
        const int forced = g_tsdf_hooks.int_wg;  // otx_integrate_workgroup: 1, 2 or 4 at every table size
        f.wg = forced > 0 ? forced : INT_WG_DEFAULT;
        while (forced <= 0 && f.wg < INT_WG && integrate_resident(variant, f.wg, f.lds, words) * f.wg < want) f.wg *= 2;
    }
    f.fn = integrate_kernel(variant, f.wg, words);
    const int r = integrate_resident(variant, f.wg, f.lds, words);
    f.grid = r ? r * INT_GRID_MULT : 4096 * (INT_WG / f.wg);
    return f;
}

// Coarse or fine slices for a batch of `est` units (est < 0: unknown, coarse), one rule with two thresholds:
// Few units (a spatial shard, a small object): a (unit, quarter) item is a chain of the batch's frames, each frame
// two dependent gather round trips plus ~270 dependent VALU instructions, so a batch too small to fill the GPU is
// bound by that chain -- ~130 us per 64 frames whatever the unit count (tools/shard_scaling.py, r05g: rank 0 of
// 16 / 32 / 64 shards 142 / 134 / 132 us).  Such batches take the fine slices (2 voxels per lane along z, twice
// the items, the next frame's gathers issued beside this frame's colour gathers: 107 / 90 / 85 us; the same
// per-voxel arithmetic, the same bits).
// An integrate launched with its batch (Direct, Overlap): fine below 3/4 of the resident workgroups in (unit, quarter)
// items -- with a quarter of the GPU's resident workgroups in items or more the coarse slices are as fast or faster
// (1/8 shard 167 / 167 us, 1/4 242 / 280 us).  The estimate is the previous batch's count (direct_estimate).
// A deferred integrate knows its batch's count (settle_batch read the mail of its units kernel): fine below 21/8 of
// the resident workgroups, 336 units -- 8 sector ranks' batches of 135 / 161 / 317 units ran fine in 112 / 126 / 131 us
// against 146 / 146 / 142 coarse, one of 367 units 167 against 148 (r06fn) -- or below otx_integrate_fine's unit count,
// a threshold sweep that only the deferred launch reads; its fused kernels have one pipeline depth, INT_FINE_KT, the
// launch with the batch also otx_integrate_depth's.
constexpr int DIRECT_FINE_NUM = 3, DIRECT_FINE_DEN = 1;
constexpr int DEFER_FINE_NUM = 21, DEFER_FINE_DEN = 8;
static int slice_form(int variant, int64_t est, bool deferred) {
    const TsdfHooks& h = g_tsdf_hooks;
    const int64_t resident = integrate_grid(variant) / INT_GRID_MULT;
    const int num = deferred ? DEFER_FINE_NUM : DIRECT_FINE_NUM, den = deferred ? DEFER_FINE_DEN : DIRECT_FINE_DEN;
    const bool small = est >= 0 && est * INT_PARTS * 4 * den < resident * num;
    const bool fine = h.int_fine > 0 || (deferred && h.fine_units >= 2 ? est >= 0 && est < h.fine_units
                                                                       : h.int_fine < 0 && small);
    if (!fine) return variant;
    const int kt = !deferred && h.int_depth > 0 ? h.int_depth : INT_FINE_KT;
    return variant | 4 | ((kt - 1) << 3);
}
// The unit count of a batch is known on the device only: the previous batch's (mailed) stands in for it, and a sharded
// volume's first batch counts as small from 16 ranks on.
// 2..15 ranks: coarse always.  A sector rank's batches swing between a few units and a full arc (r06e, rank 0
// of 8: 135 / 677 / 662 / 317 units), so the previous batch mispredicts: the 677-unit batch took 214 us fine
// against ~145 us coarse, and coarse-only steps were the faster (0.985 vs 1.053 ms, r06i)
static int64_t direct_estimate(const ot_tsdf* vol) {
    const int world = vol->dev.shard_world;
    if (world > 1 && world < 16) return (int64_t)1 << 30;
    return vol->last_batch_slots >= 0 ? vol->last_batch_slots : (world >= 16 ? 0 : (int64_t)1 << 30);
}

// auto (-1): on for sharded volumes (round 6, with their split front end: rank steps at 2 / 4 / 8 sector ranks 2.025 /
// 1.383 / 1.024 ms with it against 2.117 / 1.416 / 1.050 without, r06h; 0.953 vs 0.985 at 8 with coarse slices, r06i),
// off for whole volumes.  Round 5 had found it slower at every shard count when every rank still staged whole frames
// (its cross-stream events cost more than the co-running front end saved: DESIGN_HISTORY.md D).
static bool overlap_on(const ot_tsdf* vol) {
    return vol->overlap_mode > 0 || (vol->overlap_mode < 0 && vol->dev.shard_world > 1);
}
// the split front end: sharded volumes.  Its tile masks are written and read on the caller's stream only (mask kernel,
// then staging), so one buffer serves the double-buffered front end too: the integrate on istream never reads them.
static bool split_on(const ot_tsdf* vol) {
    const int mode = g_tsdf_hooks.split >= 0 ? g_tsdf_hooks.split : vol->split_mode;
    return mode > 0 || (mode < 0 && vol->dev.shard_world > 1);
}
// tile masks for w x h frames (each split batch's mask kernel writes its frames' maps whole)
static bool tmask_fits(int w, int h) {
    const int tx = (w + STX - 1) / STX;
    return tx <= ST_MAX_TILES_X && (int64_t)((h + STY - 1) / STY) * ((tx + 31) / 32) <= SM_WORDS;
}
static ot_status ensure_tmask(ot_tsdf* vol, int w, int h, hipStream_t stream) {
    if (vol->tmask && vol->tmask_w == w && vol->tmask_h == h) return OT_OK;
    const int64_t words = (int64_t)WORD_FRAMES * SM_PARTS * ((h + STY - 1) / STY) * (((w + STX - 1) / STX + 31) / 32);
    if (vol->tmask) {
        OT_HIP_TRY(hipStreamSynchronize(stream));
        OT_HIP_TRY(hipFree(vol->tmask));
        vol->tmask = nullptr;
    }
    OT_HIP_TRY(hipMalloc(&vol->tmask, sizeof(unsigned) * words));
    vol->tmask_words = words;
    vol->tmask_w = w, vol->tmask_h = h;
    note_alloc();
    return OT_OK;
}
// mark the tiles the units of the work list (`wcount` entries) project to, then stage those tiles
static void launch_stage(const BatchFrame* bf, const StageMaskParams& q, const UnitWork* work, const int* wcount,
                         unsigned* smask, hipStream_t stream) {
    hipLaunchKernelGGL(k_stage_mask, dim3((unsigned)q.nframes, SM_PARTS), dim3(256), 0, stream, bf, q, work, wcount,
                       smask);
    hipLaunchKernelGGL(k_stage_tiles, dim3((unsigned)q.tiles_y, (unsigned)q.nframes), dim3(256), 0, stream, bf,
                       (const unsigned*)smask, q.W, q.H, q.tiles_x, q.tiles_y, q.wpr, (int64_t)q.W * q.H);
}
static void* set_work(ot_tsdf* vol, int s) { return s == 0 ? vol->dev.work : vol->bset[1].work; }
// Deferred integrate (round 6): a sharded volume with the split front end launches batch k's integrate together with
// batch k + 1's touch (k_integrate_touch, one stream, no events) -- the default from 4 ranks on (r06k, sector rank steps:
// 0.919 vs 1.003 ms at 8, 1.301 vs 1.336 at 4, but 2.165 vs 2.075 at 2, where the rank's integrate fills the GPU and the
// double-buffered front end stays the default) unless the double-buffered front end is asked for (overlap mode 1)
static bool defer_on(const ot_tsdf* vol, bool split) {
    const int hook = g_tsdf_hooks.defer;
    if (!split || hook == 0 || vol->overlap_mode > 0) return false;
    return hook > 0 || vol->dev.shard_world >= 4;
}

// Frames per batch of the volume as it is set now: ot_tsdf_set_batch's count, at most MAX_BATCH for a whole volume whose
// batches run BatchMode::Direct with the full staging, at most WORD_FRAMES for every other -- a sharded volume, the
// double-buffered front end, the split front end and the deferred integrate (which needs the split) read one mask word.
// tsdf_flush, the integrate calls' auto-flush and the staging buffers' sizes all ask here; integrate_batch refuses a
// longer batch than its plan reads.
static int batch_cap(const ot_tsdf* vol) {
    const bool wide = vol->dev.shard_world <= 1 && !overlap_on(vol) && !split_on(vol);
    return std::min(vol->batch_max, wide ? MAX_BATCH : WORD_FRAMES);
}
// Frames a staging buffer of the volume is sized for when a batch of n frames finds it too small: the batch itself, the
// volume's cap once a batch has passed WORD_FRAMES, and otherwise no more than WORD_FRAMES -- a volume that is flushed
// every 64 frames or fewer (an object's) never pays for 128 frames of staging (315 MB at 640 x 480).
static int64_t staging_frames(const ot_tsdf* vol, int n) {
    const int cap = batch_cap(vol);
    return std::max(n, n > WORD_FRAMES ? cap : std::min(cap, WORD_FRAMES));
}

// order `stream` after the last batch's integrate when it ran on the volume's integrate stream
static ot_status join_integrate(ot_tsdf* vol, hipStream_t stream) {
    if (vol->last_set >= 0) {
        OT_HIP_TRY(hipStreamWaitEvent(stream, vol->bset[vol->last_set].ev_done, 0));
        vol->last_set = -1;
    }
    return OT_OK;
}

// the second batch set, the integrate stream and the sets' events (once per volume)
static ot_status ensure_overlap(ot_tsdf* vol) {
    if (vol->istream) return OT_OK;
    OT_HIP_TRY(hipStreamCreateWithFlags(&vol->istream, hipStreamNonBlocking));
    if (!vol->wcount) OT_HIP_TRY(hipMalloc(&vol->wcount, sizeof(int) * 4));  // [set]: length, [2 + set]: heavy units
    if (!vol->bset[1].bframes) OT_HIP_TRY(hipMalloc(&vol->bset[1].bframes, sizeof(BatchFrame) * MAX_BATCH));
    if (!vol->bset[1].work) OT_HIP_TRY(hipMalloc(&vol->bset[1].work, sizeof(UnitWork) * vol->hash_cap));
    for (auto& b : vol->bset) {
        if (!b.ev_units) OT_HIP_TRY(hipEventCreateWithFlags(&b.ev_units, hipEventDisableTiming));
        if (!b.ev_done) OT_HIP_TRY(hipEventCreateWithFlags(&b.ev_done, hipEventDisableTiming));
    }
    note_alloc();
    return OT_OK;
}

// ------------------------------------------------------------------------------------------ unbounded unit pool
// Open3D's ScalableTSDFVolume allocates blocks without bound (a fixed pool dropped units and failed at the
// next read, outside the reference caller's per-frame try/except).  Here the pool grows: records, keys and the sorted
// order are copied into pools twice as large (or more), and the hash is rebuilt from the unit keys at >= 4x the pool.

__global__ __launch_bounds__(256) void k_rehash(TsdfDev d, int n) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= n) return;
    const int slot = hash_insert(d, pack_key(d.unit_keys[id * 3], d.unit_keys[id * 3 + 1], d.unit_keys[id * 3 + 2]));
    if (slot < 0) atomicOr(&d.counters[C_HASHERR], 1);  // cannot happen: capacity >= 4x the units
    else d.hvals[slot] = id;
}

// Grow to hold at least `need` units (stream-ordered copies; the stream is synchronised first: the kernels queued on
// the volume may still read the old buffers).  Every allocation is made before any old buffer is freed, so a failed
// allocation leaves the volume as it was and is reported as the error of the call that needed the room.
static ot_status grow_pool(ot_tsdf* vol, int64_t need, int n_used, hipStream_t stream) {
    constexpr int64_t MAX_UNITS = 1 << 24;
    if (need > MAX_UNITS) return fail(OT_ERR_CAPACITY, "[ScalableTSDFVolume] more than 2^24 units");
    int64_t nmax = std::max<int64_t>(2 * vol->max_units, need + need / 2);
    nmax = std::min<int64_t>(nmax, MAX_UNITS);
    int64_t cap = 1;
    while (cap < 4 * nmax) cap <<= 1;
    ot_status st = wait_normals(vol, stream);
    if (st != OT_OK) return st;
    OT_HIP_TRY(hipStreamSynchronize(stream));
    if (vol->istream) OT_HIP_TRY(hipStreamSynchronize(vol->istream));
    TsdfDev& d = vol->dev;
    TsdfDev nd = d;
    unsigned* nsorted = nullptr;
    void* work1 = nullptr;
    void* fresh[9] = {nullptr};
    auto alloc = [&](void** p, size_t bytes, int k) {
        const hipError_t e = hipMalloc(p, bytes);
        fresh[k] = *p;
        return e;
    };
    hipError_t e = hipSuccess;
    if ((e = alloc((void**)&nd.vox, sizeof(float) * (size_t)d.unit_floats * nmax, 0)) == hipSuccess &&
        (e = alloc((void**)&nd.unit_keys, sizeof(int) * 3 * nmax, 1)) == hipSuccess &&
        (e = alloc((void**)&nsorted, sizeof(unsigned) * nmax, 2)) == hipSuccess &&
        (e = alloc((void**)&nd.hkeys, sizeof(unsigned long long) * cap, 3)) == hipSuccess &&
        (e = alloc((void**)&nd.hvals, sizeof(int) * cap, 4)) == hipSuccess &&
        (e = alloc((void**)&nd.fmask, fmask_bytes(cap), 5)) == hipSuccess &&
        (e = alloc((void**)&nd.bslots, sizeof(int) * cap, 6)) == hipSuccess &&
        (e = alloc((void**)&nd.work, sizeof(UnitWork) * cap, 7)) == hipSuccess &&
        (!vol->bset[1].work || (e = alloc(&work1, sizeof(UnitWork) * cap, 8)) == hipSuccess)) {
    }
    if (e != hipSuccess) {
        for (void* p : fresh)
            if (p) (void)hipFree(p);
        (void)hipGetLastError();
        return fail(OT_ERR_HIP, std::string("[ScalableTSDFVolume] allocation failed while growing the unit pool to ") +
                                    std::to_string(nmax) + " units: " + hipGetErrorString(e));
    }
    note_alloc();
    const size_t rec = sizeof(float) * (size_t)d.unit_floats;
    if (n_used > 0) {
        OT_HIP_TRY(hipMemcpyAsync(nd.vox, d.vox, rec * n_used, hipMemcpyDeviceToDevice, stream));
        OT_HIP_TRY(hipMemcpyAsync(nd.unit_keys, d.unit_keys, sizeof(int) * 3 * n_used, hipMemcpyDeviceToDevice, stream));
        OT_HIP_TRY(hipMemcpyAsync(nsorted, vol->sorted_ids, sizeof(unsigned) * n_used, hipMemcpyDeviceToDevice, stream));
    }
    OT_HIP_TRY(hipMemsetAsync(nd.hkeys, 0xFF, sizeof(unsigned long long) * cap, stream));
    OT_HIP_TRY(hipMemsetAsync(nd.hvals, 0xFF, sizeof(int) * cap, stream));
    OT_HIP_TRY(hipMemsetAsync(nd.fmask, 0, fmask_bytes(cap), stream));
    nd.hash_mask = (int)(cap - 1);
    nd.max_units = (int)nmax;
    if (n_used > 0) hipLaunchKernelGGL(k_rehash, dim3((unsigned)((n_used + 255) / 256)), dim3(256), 0, stream, nd, n_used);
    OT_LAUNCH_CHECK();
    OT_HIP_TRY(hipStreamSynchronize(stream));
    for (void* p : {(void*)d.vox, (void*)d.unit_keys, (void*)vol->sorted_ids, (void*)d.hkeys, (void*)d.hvals,
                    (void*)d.fmask, (void*)d.bslots, d.work, vol->bset[1].work})
        if (p) (void)hipFree(p);
    d = nd;
    vol->bset[1].work = work1;
    vol->sorted_ids = nsorted;
    vol->max_units = nmax;
    vol->hash_cap = cap;
    return OT_OK;
}

// ------------------------------------------------------------------------------------------ the batch pipeline
// integrate_batch: plan_batch chooses how the batch runs, once; the launchers below are each written once and read the
// plan (through the batch's context); settle_batch replays with the same launchers after pool growth.

// How a batch of frames with intrinsics `in` and pair counter `pc` runs: the mode, the split front end, the batch's set
// and where its work list's length lives.  Nothing after this asks the volume or the hooks for the mode again.
static ot_status plan_batch(ot_tsdf* vol, const ot_intrinsics& in, int pc, BatchPlan& p) {
    p.split = split_on(vol) && tmask_fits(in.width, in.height);
    // the slice pre-test needs every pixel of every frame staged, with its tile-max map: not the split front end's
    // marked tiles.  Default: whole volumes (a shard's few units per batch take the fused launches or the fine slices)
    const int pre = g_tsdf_hooks.pretest;
    p.pretest = !p.split && (pre > 0 || (pre < 0 && vol->dev.shard_world <= 1)) &&
                (int64_t)pre_tiles(in.width) * pre_tiles(in.height) * MAX_BATCH + PRE_SLACK < (int64_t)PRE_NONE;
    p.mode = defer_on(vol, p.split) ? BatchMode::Deferred : overlap_on(vol) ? BatchMode::Overlap : BatchMode::Direct;
    p.wcount = vol->dev.counters + pc;
    if (p.mode != BatchMode::Direct) {  // the sets alternate; each has its own copy of the count
        ot_status st = ensure_overlap(vol);
        if (st != OT_OK) return st;
        p.set = vol->bset_next;
        vol->bset_next ^= 1;
        p.wcount = p.wcopy = vol->wcount + p.set;
    }
    return OT_OK;
}

// per-frame parameters of a batch into its pinned staging half; frame k's staged records at bdc + npx * k
static void fill_batch_frames(const ot_tsdf* vol, const PendingFrame* frames, int n, uint2* bdc, int64_t npx, float vl,
                              BatchFrame* host) {
    for (int k = 0; k < n; ++k) {
        const PendingFrame& f = frames[k];
        BatchFrame& b = host[k];
        b.depth16 = f.depth;
        b.depthf = f.depth ? nullptr : f.depthf;
        b.color = (vol->color_type == OT_COLOR_RGB8) ? f.color : nullptr;
        b.dc = bdc + npx * k;
        b.pad = 0;
        double pose[16];
        inverse4(f.extrinsic, pose);
        for (int i = 0; i < 12; ++i) b.pose[i] = pose[i];
        float E[12];  // (the pinned staging is only written)
        for (int i = 0; i < 12; ++i) b.E[i] = E[i] = (float)f.extrinsic[i];
        for (int i = 0; i < 3; ++i) b.es[i] = E[i * 4 + 2] * vl;
        b.scale = (float)f.depth_scale;
        b.trunc = f.depth_trunc;
    }
}

static BatchTouchParams make_touch_params(const ot_tsdf* vol, const ot_intrinsics& in, int pc, bool split) {
    BatchTouchParams tp;
    tp.npx = (int64_t)in.width * in.height;
    tp.pc = pc;
    tp.W = in.width, tp.stride = vol->stride;
    tp.ws = (in.width + vol->stride - 1) / vol->stride;
    tp.hs = (in.height + vol->stride - 1) / vol->stride;
    tp.fx = in.fx, tp.fy = in.fy, tp.cx = in.cx, tp.cy = in.cy;
    tp.trunc = vol->sdf_trunc;
    tp.unit_len = vol->unit_length, tp.inv_unit = 1.0 / vol->unit_length;
    tp.slot_cap = (int)vol->hash_cap;
    tp.tiles = ((tp.ws + TT - 1) / TT) * ((tp.hs + TT - 1) / TT);
    tp.stage_blocks = g_tsdf_hooks.stage_blocks < 0 ? 2 * tp.tiles : g_tsdf_hooks.stage_blocks;
    tp.tf = g_tsdf_hooks.touch_tf > 0 ? g_tsdf_hooks.touch_tf : TF;
    // sharded volume: split front end (touch without staging -> units -> tile mask -> staging of the marked tiles)
    tp.sample_stage = split ? 1 : 0;
    if (split) tp.stage_blocks = -1;
    tp.tmax = nullptr;  // (integrate_batch: the set's maps, when the batch's plan has the pre-test)
    tp.H = in.height;
    tp.onepass = g_tsdf_hooks.onepass != 0;
    return tp;
}

static StageMaskParams make_stage_params(const ot_tsdf* vol, const ot_intrinsics& in, const IntegrateParams& ip, int n) {
    StageMaskParams q;
    q.W = in.width, q.H = in.height;
    q.tiles_x = (in.width + STX - 1) / STX;
    q.tiles_y = (in.height + STY - 1) / STY;
    q.wpr = (q.tiles_x + 31) / 32;
    q.fx = ip.fx, q.fy = ip.fy, q.cx = ip.cx, q.cy = ip.cy;
    q.vl = ip.vl, q.half = ip.half;
    q.unit_len = vol->unit_length;
    q.nframes = n;
    return q;
}

// a profiling event pair around work on a stream (ot_tsdf_set_profiling; nothing when it is off)
struct ProfPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
};
static ot_status prof_open(const ot_tsdf* vol, ProfPair& p, hipStream_t stream) {
    if (!vol->profiling) return OT_OK;
    OT_HIP_TRY(hipEventCreate(&p.e0));
    OT_HIP_TRY(hipEventCreate(&p.e1));
    OT_HIP_TRY(hipEventRecord(p.e0, stream));
    return OT_OK;
}
static ot_status prof_close(const ProfPair& p, hipStream_t stream, decltype(ot_tsdf::prof_events)& list) {
    if (!p.e0) return OT_OK;
    OT_HIP_TRY(hipEventRecord(p.e1, stream));
    list.emplace_back(p.e0, p.e1);
    return OT_OK;
}

// A batch's front end on `stream`: touch -> units (-> tile mask -> staging of the marked tiles when split).
// First pass (replay false; touch false: a fused launch has run the batch's touch already), or the replay after pool
// growth: touch again from the staged depths, then list the units the batch's integrate skipped (those without an id),
// counted in the batch's own pair counter -- or, Deferred, the whole list again into the set's count (nothing of the
// batch is integrated yet, and it stays deferred).
static void launch_front_end(ot_tsdf* vol, const BatchCtx& bc, bool replay, bool touch, hipStream_t stream) {
    const BatchPlan& plan = bc.plan;
    const BatchFrame* bf = vol->bset[plan.set].bframes;
    UnitWork* work = (UnitWork*)set_work(vol, plan.set);
    BatchTouchParams tp = bc.tp;
    tp.slot_cap = (int)vol->hash_cap;  // (a replay's hash has grown)
    if (touch) {  // the staging-only workgroups (stage_blocks > 0) belong to the first pass of an unsplit batch
        const bool wide = bc.n > WORD_FRAMES;  // (never split: integrate_batch)
        const auto touch_k = replay       ? (wide ? k_batch_touch<true, true> : k_batch_touch<true, false>)
                             : plan.split ? k_batch_touch_split
                             : wide       ? k_batch_touch<false, true>
                                          : k_batch_touch<false, false>;
        const unsigned tiles = (unsigned)tp.tiles + (replay ? 0u : (unsigned)std::max(0, tp.stage_blocks));
        hipLaunchKernelGGL(touch_k, dim3(tiles, (unsigned)((bc.n + tp.tf - 1) / tp.tf)), dim3(256), 0, stream, bf, tp,
                           vol->dev, bc.n);
    }
    const bool missing_only = replay && plan.mode != BatchMode::Deferred;
    int* wcopy = missing_only ? nullptr : plan.wcopy;
    const bool wide_units = bc.n > WORD_FRAMES;
    const auto units_k = missing_only ? (wide_units ? k_batch_units<true, true> : k_batch_units<true, false>)
                                      : (wide_units ? k_batch_units<false, true> : k_batch_units<false, false>);
    hipLaunchKernelGGL(units_k, dim3(256), dim3(256), 0, stream, vol->dev, work, bc.pc, vol->hmail + OT_MAIL_WORDS, wcopy,
                       ++vol->units_seq);
    if (plan.split)  // (a replay: from the caller's frames, valid until this flush returns)
        launch_stage(bf, bc.sq, (const UnitWork*)work, (const int*)(wcopy ? wcopy : vol->dev.counters + bc.pc), bc.smask,
                     stream);
}

// k_batch_integrate over batch `bc`'s work list (`wcount` entries) on `stream`, in the form `variant`
static ot_status launch_integrate(ot_tsdf* vol, const BatchCtx& bc, int variant, const int* wcount, hipStream_t stream) {
    const BatchFrame* bf = vol->bset[bc.plan.set].bframes;
    const UnitWork* uw = (const UnitWork*)set_work(vol, bc.plan.set);
    void* args[] = {(void*)&bf, (void*)&bc.ip0, (void*)&vol->dev, (void*)&uw, (void*)&wcount};
    const IntForm f = integrate_form(variant, bc.ip0.rcp_hi, bc.n > WORD_FRAMES ? FMASK_WORDS : 1);
    OT_HIP_TRY(hipLaunchKernel(f.fn, dim3(f.grid), dim3(64 * f.wg), args, f.lds, stream));
    OT_LAUNCH_CHECK();
    return OT_OK;
}

// order `stream` after the deferred batch's front end (and all before it) when that ran on another stream
static ot_status follow_deferred(ot_tsdf* vol, hipStream_t stream) {
    if (stream == vol->dfr_stream) return OT_OK;
    if (!vol->ev_dfr) OT_HIP_TRY(hipEventCreateWithFlags(&vol->ev_dfr, hipEventDisableTiming));
    OT_HIP_TRY(hipEventRecord(vol->ev_dfr, vol->dfr_stream));
    OT_HIP_TRY(hipStreamWaitEvent(stream, vol->ev_dfr, 0));
    vol->dfr_stream = stream;
    return OT_OK;
}

// Launch the deferred batch's integrate on `stream`: with the touch of batch `next` in one launch (k_integrate_touch), or
// alone (next == nullptr: a flush, or a next batch that does not fuse).  The variant's colour precision and division
// form; its slices by the batch's unit count, known here (slice_form).
static ot_status launch_deferred(ot_tsdf* vol, hipStream_t stream, const BatchCtx* next) {
    if (!vol->dfr_on) return OT_OK;
    ot_status st = follow_deferred(vol, stream);
    if (st != OT_OK) return st;
    vol->dfr_on = false;
    const BatchCtx& D = vol->dfr;
    const int variant = slice_form(D.variant & 3, vol->last_batch_slots, true);
    ProfPair timed;
    if ((st = prof_open(vol, timed, stream)) != OT_OK) return st;
    if (next) {
        const BatchFrame* bf = vol->bset[D.plan.set].bframes;
        const UnitWork* uw = (const UnitWork*)set_work(vol, D.plan.set);
        const int* wc = D.plan.wcount;
        const BatchFrame* tf = vol->bset[next->plan.set].bframes;
        const BatchTouchParams& tp = next->tp;
        const int tn = next->n, ni = integrate_grid(variant);
        void* args[] = {(void*)&bf, (void*)&D.ip0, (void*)&vol->dev, (void*)&uw, (void*)&wc, (void*)&ni,
                        (void*)&tf, (void*)&tp, (void*)&tn};
        static const void* const kt[8] = {
            (const void*)k_integrate_touch<false, false>,      (const void*)k_integrate_touch<false, true>,
            (const void*)k_integrate_touch<true, false>,       (const void*)k_integrate_touch<true, true>,
            (const void*)k_integrate_touch_fine<false, false>, (const void*)k_integrate_touch_fine<false, true>,
            (const void*)k_integrate_touch_fine<true, false>,  (const void*)k_integrate_touch_fine<true, true>};
        const unsigned grid = (unsigned)ni + (unsigned)tp.tiles * (unsigned)((tn + tp.tf - 1) / tp.tf);
        OT_HIP_TRY(hipLaunchKernel(kt[variant & 7], dim3(grid), dim3(64 * INT_WG), args, 0, stream));
        OT_LAUNCH_CHECK();
    } else if ((st = launch_integrate(vol, D, variant, D.plan.wcount, stream)) != OT_OK) {
        return st;
    }
    return prof_close(timed, stream, vol->prof_events);
}

// After each batch: the counters its units kernel mailed (mail_wait on units_seq: the host waits for the units kernel,
// not for the integrate queued behind it, so the GPU keeps its queue).  Units the pool could not hold (C_OVERFLOW), or keys the
// hash could not hold (C_HASHERR bit 0), were skipped by the batch's integrate: grow, then replay the batch for exactly
// those units -- touch again from the staged depths (still resident: the next batch has not been staged yet), allocate
// the missing units (units that have an id were integrated and are skipped), integrate them with the batch's frames.
// Units are independent and each sees the batch's frames in call order, so the volume equals an unbounded pool's.
// A pool more than 3/4 full also grows here, ahead of need.
static ot_status settle_batch(ot_tsdf* vol, const BatchCtx& bc, hipStream_t stream) {
    for (int round = 0;; ++round) {
        ot_status ws = mail_wait(vol->hmail + MAIL_SEQ_UNITS, vol->units_seq, stream);
        if (ws != OT_OK) return ws;
        int c[N_COUNTERS];
        std::memcpy(c, vol->hmail + OT_MAIL_WORDS, sizeof(c));
        vol->last_batch_slots = c[bc.pc];  // units the batch touched: the next batch's item estimate
        if (round == 0) {
            ++vol->stat_batches;
            vol->stat_unit_batches += c[bc.pc];
        }
        const bool short_of_room = c[C_OVERFLOW] != 0 || (c[C_HASHERR] & 1) != 0;
        if (!short_of_room) {
            if (vol->stat_prev_units >= 0) vol->stat_fresh += c[C_UNITS] - vol->stat_prev_units;
            vol->stat_prev_units = c[C_UNITS];
            if ((int64_t)c[C_UNITS] * 4 > vol->max_units * 3)
                return grow_pool(vol, (int64_t)c[C_UNITS] * 2, c[C_UNITS], stream);
            return OT_OK;
        }
        if (round >= 8) return fail(OT_ERR_CAPACITY, "[ScalableTSDFVolume] unit pool: growth did not converge");
        // ids below the old capacity were all handed out; the allocations past it were dropped (C_UNITS overshoots)
        const int used = (int)std::min<int64_t>(c[C_UNITS], vol->max_units);
        const int64_t need = std::max<int64_t>((int64_t)c[C_UNITS], vol->max_units) + 1;
        ot_status st = grow_pool(vol, need, used, stream);  // synchronises both of the volume's streams
        if (st != OT_OK) return st;
        int h[N_COUNTERS];
        OT_HIP_TRY(hipMemcpy(h, vol->dev.counters, sizeof(h), hipMemcpyDeviceToHost));
        h[C_UNITS] = used;
        h[C_OVERFLOW] = 0;
        h[C_HASHERR] &= ~1;
        h[bc.pc] = 0;  // the replay's touched-slot count (the batch's own pair counter; the next batch's stays zero)
        OT_HIP_TRY(hipMemcpy(vol->dev.counters, h, sizeof(h), hipMemcpyHostToDevice));
        // the replay, all on the caller's stream, from the batch's set (its staging is intact: nothing restaged it)
        launch_front_end(vol, bc, true, true, stream);
        if (bc.plan.mode == BatchMode::Deferred) {  // the whole work list is rebuilt; the batch stays deferred
            OT_LAUNCH_CHECK();
            continue;
        }
        st = launch_integrate(vol, bc, bc.variant, vol->dev.counters + bc.pc, stream);
        if (st != OT_OK) return st;
        vol->last_set = -1;  // the replay ran on the caller's stream, after both streams drained
        vol->sorted_frame = -1;
    }
}

static ot_status integrate_batch(ot_tsdf* vol, const PendingFrame* frames, int n, hipStream_t stream) {
    const ot_intrinsics& in = frames[0].intr;
    ot_status st = wait_normals(vol, stream);  // deferred vertex normals of the last mesh still read the volume
    if (st != OT_OK || (st = ensure_mult(vol, &in, stream)) != OT_OK) return st;
    BatchCtx bc;
    // this batch's pair counter: zeroed by reset, or by the previous batch's k_batch_units (no memset here)
    bc.pc = vol->batch_pc;
    bc.n = n;
    if ((st = plan_batch(vol, in, bc.pc, bc.plan)) != OT_OK) return st;
    const BatchPlan& plan = bc.plan;
    if (n > MAX_BATCH || (n > WORD_FRAMES && (plan.mode != BatchMode::Direct || plan.split)))
        return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume::Integrate] batch longer than its plan's frame masks");
    // A pending deferred batch is handed over here, before anything below restages a set.  On another stream than its
    // front end's, this stream first waits for that one: this batch's set was last integrated there, inside the launch
    // with the deferred batch's touch (queued before its units kernel).  And a batch that does not fuse with it (the mode changed: the hooks, the overlap
    // setting, an image size the tile masks do not fit) launches it alone first -- else it would stay pending while its
    // set is restaged.  On one stream with a constant mode neither issues a call.
    if (vol->dfr_on) {
        if ((st = follow_deferred(vol, stream)) != OT_OK) return st;
        if (plan.mode != BatchMode::Deferred && (st = launch_deferred(vol, stream, nullptr)) != OT_OK) return st;
    }
    auto& bs = vol->bset[plan.set];
    // Overlap: the set's previous batch (two batches ago) must have finished its integrate before its buffers are
    // restaged (an event never recorded counts as complete)
    if (plan.mode == BatchMode::Overlap) OT_HIP_TRY(hipStreamWaitEvent(stream, bs.ev_done, 0));
    const int64_t npx = (int64_t)in.width * in.height;
    if (bs.cap < npx * n) {
        if (bs.bdc) {
            OT_HIP_TRY(hipStreamSynchronize(stream));
            if (vol->istream) OT_HIP_TRY(hipStreamSynchronize(vol->istream));
            OT_HIP_TRY(hipFree(bs.bdc));
            bs.bdc = nullptr;
        }
        const int64_t cap = npx * staging_frames(vol, n);
        OT_HIP_TRY(hipMalloc(&bs.bdc, sizeof(uint2) * cap));
        bs.cap = cap;
    }
    // per-frame parameters: pinned host staging (double-buffered) -> device
    BatchFrame* host = vol->hbframes + vol->hb_next * MAX_BATCH;  // (the last batch from this half was copied:
    vol->hb_next ^= 1;                                            // settle_batch saw its units kernel mail)
    bc.ip0 = make_integrate_params(vol, nullptr, nullptr, vol->mult, &in, frames[0].extrinsic);
    fill_batch_frames(vol, frames, n, bs.bdc, npx, bc.ip0.vl, host);
    hipLaunchKernelGGL(k_copy_frames, dim3(1), dim3(COPY_FRAMES_LANES), 0, stream, (const uint4*)host,
                       (uint4*)bs.bframes, (int)(sizeof(BatchFrame) / 16) * n);
    bc.tp = make_touch_params(vol, in, bc.pc, plan.split);
    bc.tp.tf = touch_group_frames(bc.tp.tf, n);
    if (plan.pretest) {  // the set's tile-max maps: written by this batch's staging, read by its integrate and a replay's
        const int64_t tiles = (int64_t)pre_tiles(in.width) * pre_tiles(in.height);
        if (bs.tmax_cap < tiles * n) {
            if (bs.tmax) {
                OT_HIP_TRY(hipStreamSynchronize(stream));
                if (vol->istream) OT_HIP_TRY(hipStreamSynchronize(vol->istream));
                OT_HIP_TRY(hipFree(bs.tmax));
                bs.tmax = nullptr, bs.tmax_cap = 0;
            }
            const int64_t cap = tiles * staging_frames(vol, n);
            OT_HIP_TRY(hipMalloc(&bs.tmax, sizeof(unsigned) * (cap + PRE_SLACK)));
            bs.tmax_cap = cap;
        }
        bc.tp.tmax = bs.tmax;
        // one-pass staging (stage_tile_quads): a wave per strip of eight tiles and frame, so no staging workgroup idles
        // (640 x 480: 150 workgroups per frame group instead of 160, front end 82.8 -> 79.4 us per batch; 80: 83.1)
        if (bc.tp.onepass && g_tsdf_hooks.stage_blocks < 0 && bc.tp.stage_blocks > 0 && in.width % PRE_TILE == 0)
            bc.tp.stage_blocks = (int)((tiles + 31) / 32);
        bc.ip0.tmax = bs.tmax;
        bc.ip0.tmax_tiles = (int)tiles;
        bc.ip0.tmax_words = (int)(tiles * n);
    }
    if (plan.split) {
        if ((st = ensure_tmask(vol, in.width, in.height, stream)) != OT_OK) return st;
        bc.sq = make_stage_params(vol, in, bc.ip0, n);
        bc.smask = vol->tmask;
    }
    // reciprocal-table kernel while every weight + 1 is an integer <= RCP_N: weights count updates, at most one
    // per frame since reset, unless units were imported (k_batch_integrate: Markstein's exact correction)
    const bool fast = !vol->imported && (int64_t)vol->frame_id + n < RCP_N;
    bc.variant = (vol->color64 ? 2 : 0) + (fast ? 1 : 0);
    // the table entries the batch can read: a weight is at most the frames since reset, so weight + 1 <= frame_id + n
    // (before frame_id advances; kept in the batch's context for a deferred launch or a replay)
    bc.ip0.rcp_hi = (int)std::min<int64_t>((int64_t)vol->frame_id + n, RCP_N);
    // (a deferred integrate takes its slices when it is launched, by its own unit count)
    if (plan.mode != BatchMode::Deferred) bc.variant = slice_form(bc.variant, direct_estimate(vol), false);

    ProfPair fe;  // front end (staging + touch + units): the part a sharded volume repeats
    if ((st = prof_open(vol, fe, stream)) != OT_OK) return st;
    // Deferred: the last batch's integrate and this batch's touch in one launch
    const bool fused = plan.mode == BatchMode::Deferred && vol->dfr_on;
    if (fused && (st = launch_deferred(vol, stream, &bc)) != OT_OK) return st;
    launch_front_end(vol, bc, false, !fused, stream);
    if (plan.mode == BatchMode::Deferred) {  // the integrate waits for the next batch's touch (or the next flush)
        if ((st = prof_close(fe, stream, vol->prof_fe_events)) != OT_OK) return st;
        vol->dfr = bc;
        vol->dfr_on = true, vol->dfr_stream = stream;
    } else {
        // Overlap: the integrate on istream behind this set's units kernel (and the previous batch's integrate: same
        // stream), so the caller's stream is free for the next batch's front end
        hipStream_t is = stream;
        if (plan.mode == BatchMode::Overlap) {
            OT_HIP_TRY(hipEventRecord(bs.ev_units, stream));
            OT_HIP_TRY(hipStreamWaitEvent(vol->istream, bs.ev_units, 0));
            is = vol->istream;
        }
        if ((st = prof_close(fe, stream, vol->prof_fe_events)) != OT_OK) return st;
        ProfPair timed;
        if ((st = prof_open(vol, timed, is)) != OT_OK) return st;
        if ((st = launch_integrate(vol, bc, bc.variant, plan.wcount, is)) != OT_OK) return st;
        if ((st = prof_close(timed, is, vol->prof_events)) != OT_OK) return st;
        if (plan.mode == BatchMode::Overlap) {
            OT_HIP_TRY(hipEventRecord(bs.ev_done, is));
            vol->last_set = plan.set;
        }
    }
    vol->batch_pc ^= 1;  // only once this batch's kernels are queued (its units kernel zeroes the other counter)
    vol->staged_set = plan.set, vol->staged_n = n, vol->staged_w = in.width, vol->staged_h = in.height;
    vol->staged_map = bc.tp.tmax != nullptr;
    vol->frame_id += n;
    vol->sorted_frame = -1;
    vol->early_frame = vol->frame_id;  // the mailed counters are final for this frame count (see units_seq)
    return settle_batch(vol, bc, stream);
}

// room for `extra` more units before a kernel that allocates up to that many (imports): grow now if needed
ot_status reserve_units(ot_tsdf* vol, int64_t extra, hipStream_t stream) {
    int nu = 0;
    OT_HIP_TRY(hipMemcpyAsync(&nu, vol->dev.counters + C_UNITS, sizeof(int), hipMemcpyDeviceToHost, stream));
    OT_HIP_TRY(hipStreamSynchronize(stream));
    const int used = (int)std::min<int64_t>(nu, vol->max_units);
    if (used + extra <= vol->max_units) return OT_OK;
    return grow_pool(vol, used + extra, used, stream);
}

ot_status wait_normals(ot_tsdf* vol, hipStream_t stream) {
    if (!vol->normals_pending) return OT_OK;
    const hipError_t q = hipEventQuery(vol->ev_normals);
    if (q == hipSuccess) {
        vol->normals_pending = false;
        return OT_OK;
    }
    if (q != hipErrorNotReady) OT_HIP_TRY(q);
    OT_HIP_TRY(hipStreamWaitEvent(stream, vol->ev_normals, 0));
    return OT_OK;
}

ot_status tsdf_flush(ot_tsdf* vol, hipStream_t stream, bool join) {
    size_t i = 0;
    std::vector<PendingFrame> frames;
    frames.swap(vol->pending);
    // the volume changes: the last extractions' structures are stale
    if (!frames.empty()) vol->mesh.valid = vol->cloud.valid = false;
    while (i < frames.size()) {
        // a batch: consecutive frames with identical intrinsics, at most batch_cap (<= MAX_BATCH)
        size_t n = 1;
        const int cap = batch_cap(vol);
        while (i + n < frames.size() && (int)n < cap &&
               std::memcmp(&frames[i + n].intr, &frames[i].intr, sizeof(ot_intrinsics)) == 0)
            ++n;
        ot_status st = integrate_batch(vol, frames.data() + i, (int)n, stream);
        if (st != OT_OK) return st;
        i += n;
    }
    if (!join) return OT_OK;
    ot_status st = launch_deferred(vol, stream, nullptr);  // a reader needs the last batch integrated
    if (st != OT_OK) return st;
    return join_integrate(vol, stream);
}

}  // namespace ot

using namespace ot;

extern "C" {

ot_status ot_tsdf_integrate(ot_tsdf* vol, const float* depth, const uint8_t* color, const ot_intrinsics* in,
                            const double extrinsic[16], void* stream) {
    ot_status st = check_frame(vol, depth, color, in, extrinsic);
    if (st != OT_OK) return st;
    PendingFrame f;
    f.depth = nullptr;
    f.depthf = depth;
    f.color = color;
    f.intr = *in;
    std::memcpy(f.extrinsic, extrinsic, sizeof(double) * 16);
    f.depth_scale = 1.0;
    f.depth_trunc = 0.0;
    vol->pending.push_back(f);
    // a full queue is integrated; the integrate may keep running on the volume's integrate stream (overlap mode)
    if ((int)vol->pending.size() >= batch_cap(vol)) return tsdf_flush(vol, S(stream), false);
    return OT_OK;
}

ot_status ot_tsdf_integrate_u16(ot_tsdf* vol, const uint16_t* depth, const uint8_t* color, const ot_intrinsics* in,
                                const double extrinsic[16], double depth_scale, double depth_trunc, void* stream) {
    ot_status st = check_frame(vol, depth, color, in, extrinsic);
    if (st != OT_OK) return st;
    PendingFrame f;
    f.depth = depth;
    f.depthf = nullptr;
    f.color = color;
    f.intr = *in;
    std::memcpy(f.extrinsic, extrinsic, sizeof(double) * 16);
    f.depth_scale = depth_scale;
    f.depth_trunc = depth_trunc;
    vol->pending.push_back(f);
    if ((int)vol->pending.size() >= batch_cap(vol)) return tsdf_flush(vol, S(stream), false);
    return OT_OK;
}

ot_status ot_tsdf_integrate_u16_frames(ot_tsdf* vol, int32_t n, const uint16_t* depth, const uint8_t* color,
                                       const ot_intrinsics* in, const double* extrinsics, double depth_scale,
                                       double depth_trunc, void* stream) {
    if (!vol || n < 0 || !in || (n > 0 && (!depth || !extrinsics)))
        return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume::Integrate] invalid arguments");
    const int64_t npx = (int64_t)in->width * in->height;
    for (int32_t k = 0; k < n; ++k) {  // exactly n calls of ot_tsdf_integrate_u16, without n host round trips
        ot_status st = ot_tsdf_integrate_u16(vol, depth + (size_t)k * npx, color ? color + (size_t)k * npx * 3 : nullptr,
                                             in, extrinsics + 16 * (size_t)k, depth_scale, depth_trunc, stream);
        if (st != OT_OK) return st;
    }
    // A scan handed over in one call does not wait for the next reader: what the call leaves queued starts now once it
    // is as long as a one-word batch (the frames that, frame by frame under a cap of WORD_FRAMES, had started at the
    // 64th call), so the host's work up to the reader runs beside the integrate -- an object's 64-frame scan under the
    // default cap of 128.  Fewer frames stay queued for the calls that follow.
    if ((int)vol->pending.size() >= std::min(vol->batch_max, WORD_FRAMES)) return tsdf_flush(vol, S(stream), false);
    return OT_OK;
}

ot_status ot_tsdf_flush(ot_tsdf* vol, void* stream) {
    if (!vol) return fail(OT_ERR_INVALID_ARGUMENT, "volume is NULL");
    return tsdf_flush(vol, S(stream));
}

}  // extern "C"
