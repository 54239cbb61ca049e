// tsdf_frontend.hip — the kernels of a TSDF batch's front end and their launchers: the copy of the per-frame
// parameters, the touch (with the staging), the units kernel and the split front end's tile mask and tile staging.
// The host batch pipeline (tsdf.hip) calls the launch_* functions below (declared in tsdf.h); the selections between a
// kernel's forms are made here.
#include <algorithm>

#include "tsdf_touch.h"

namespace ot {

// The batch's per-frame parameters from the pinned host staging into device memory: one small kernel reading host
// memory instead of a copy command (the runtime's blit copy cost ~5 us of host API time and left the stream idle ~4 us
// behind it, on every batch's critical path: one object's timeline, r05m).  Up to two 16-B words per lane (the second
// only past 78 frames), both loaded before either is stored, so every PCIe read is in flight at once (a 256-lane loop
// took 8.4 us: four round trips, r05n)
__global__ __launch_bounds__(COPY_FRAMES_LANES) void k_copy_frames(const uint4* __restrict__ src,
                                                                   uint4* __restrict__ dst, int n16) {
    const int i = threadIdx.x, j = i + COPY_FRAMES_LANES;
    uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
    if (i < n16) a = src[i];
    if (j < n16) b = src[j];
    if (i < n16) dst[i] = a;
    if (j < n16) dst[j] = b;
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

// Unit headers of the batch: allocate new units, move and clear the frame masks (ready for the next batch).  A unit the
// pool cannot hold is dropped (id -1, C_OVERFLOW; not counted) and integrated by the replay once the pool has grown.
// REPLAY: units that already have an id were integrated by the batch's first pass: skipped (id -1, not counted).
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
// (The staging tile STX x STY and the masks' layout constants SM_WORDS, SM_PARTS, ST_MAX_TILES_X: tsdf.h.)
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

// ------------------------------------------------------------------------------------------------ launchers
void launch_copy_frames(const BatchFrame* host, BatchFrame* dev, int n, hipStream_t stream) {
    hipLaunchKernelGGL(k_copy_frames, dim3(1), dim3(COPY_FRAMES_LANES), 0, stream, (const uint4*)host, (uint4*)dev,
                       (int)(sizeof(BatchFrame) / 16) * n);
}

// the staging-only workgroups (stage_blocks > 0) belong to the first pass of an unsplit batch
void launch_touch(const BatchFrame* frames, const BatchTouchParams& tp, const TsdfDev& dev, int n, bool replay,
                  bool split, hipStream_t stream) {
    const bool wide = n > WORD_FRAMES;  // (never split: integrate_batch)
    const auto touch_k = replay  ? (wide ? k_batch_touch<true, true> : k_batch_touch<true, false>)
                         : split ? k_batch_touch_split
                         : wide  ? k_batch_touch<false, true>
                                 : k_batch_touch<false, false>;
    const unsigned tiles = (unsigned)tp.tiles + (replay ? 0u : (unsigned)std::max(0, tp.stage_blocks));
    hipLaunchKernelGGL(touch_k, dim3(tiles, (unsigned)((n + tp.tf - 1) / tp.tf)), dim3(256), 0, stream, frames, tp, dev,
                       n);
}

void launch_units(const TsdfDev& dev, UnitWork* work, int pc, unsigned* early_mail, int* wcount, unsigned seq, int n,
                  bool missing_only, hipStream_t stream) {
    const bool wide = n > WORD_FRAMES;
    const auto units_k = missing_only ? (wide ? k_batch_units<true, true> : k_batch_units<true, false>)
                                      : (wide ? k_batch_units<false, true> : k_batch_units<false, false>);
    hipLaunchKernelGGL(units_k, dim3(256), dim3(256), 0, stream, dev, work, pc, early_mail, wcount, seq);
}

void launch_stage_mask(const BatchFrame* frames, const StageMaskParams& q, const UnitWork* work, const int* wcount,
                       unsigned* smask, hipStream_t stream) {
    hipLaunchKernelGGL(k_stage_mask, dim3((unsigned)q.nframes, SM_PARTS), dim3(256), 0, stream, frames, q, work, wcount,
                       smask);
}

void launch_stage_tiles(const BatchFrame* frames, const StageMaskParams& q, const unsigned* smask, hipStream_t stream) {
    hipLaunchKernelGGL(k_stage_tiles, dim3((unsigned)q.tiles_y, (unsigned)q.nframes), dim3(256), 0, stream, frames,
                       smask, q.W, q.H, q.tiles_x, q.tiles_y, q.wpr, (int64_t)q.W * q.H);
}

}  // namespace ot
