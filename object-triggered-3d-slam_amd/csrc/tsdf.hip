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
// k_batch_integrate.  The unit pool is unbounded like Open3D's: when a batch needs more units than the pool
// holds, the pool and the hash grow (records copied, keys rehashed) and the batch's dropped units are integrated
// again from its staged frames (settle_batch), so the result is the one an unbounded pool gives.
//
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
//
// This file is host code: the launch policy (integrate_form, slice_form, the mode predicates, batch_cap), the batch
// pipeline (plan_batch, integrate_batch, settle_batch, tsdf_flush), pool growth (grow_pool, with its small k_rehash) and
// the C entry points.  The kernels live in translation units of their own and are reached through the launchers declared
// in tsdf.h alone:
//   tsdf_frontend.hip                              k_copy_frames, k_batch_touch, k_batch_touch_split, k_batch_units,
//                                                  k_stage_mask, k_stage_tiles
//   tsdf_integrate.hip, tsdf_integrate_wide.hip    k_batch_integrate, one and two mask words (tsdf_integrate_kernel.h)
//   tsdf_fused.hip                                 k_integrate_touch, k_integrate_touch_fine
// over the device text of tsdf_stage.h (staging), tsdf_touch.h (touch) and tsdf_integrate.h (integrate), from which this
// file reads constants only.  The unit exchange is tsdf_exchange.hip, the volume's life cycle, settings and read-outs
// tsdf_volume.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "slice_pretest.h"
#include "tsdf.h"
#include "tsdf_integrate.h"
#include "tsdf_touch.h"

namespace ot {

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

// the fused kernels' one frame pipeline depth of the fine slices (and the default of the launch with the batch)
constexpr int INT_FINE_KT = 1;
// Waves per workgroup of the coarse integrate: a finished wave frees its wave slot at once, but its
// workgroup's place on the CU only when the slowest wave ends, so the smaller the workgroup the sooner the dispatcher
// refills the slot.  The fine slices and the fused launches keep INT_WG waves.
constexpr int INT_WG_DEFAULT = 1;
// the k_batch_integrate of a form: wg waves per workgroup (a coarse form: 1, 2 or 4), the batch's mask words
static const void* integrate_kernel(IntegrateForm form, int wg, int words) {
    return words > 1 ? integrate_kernel_wide(form, wg) : integrate_kernel_word(form, wg);
}

// LDS of a launch: the table's entries 0 .. rcp_hi in the form's precision (the hardware allocates whole granules)
constexpr unsigned LDS_GRANULE = 1280;
constexpr unsigned RCP_LDS_MAX = ((RCP_N + 1) * 8 + LDS_GRANULE - 1) / LDS_GRANULE;  // in granules
static unsigned rcp_lds_bytes(IntegrateForm form, int rcp_hi) {
    if (!form.fast) return 0;  // IEEE divisions: no table
    const unsigned bytes = (unsigned)(std::min(std::max(rcp_hi, 1), RCP_N) + 1) * (form.c64 ? 8u : 4u);
    return (bytes + 15u) & ~15u;
}

// Co-resident workgroups of an integrate kernel on the device, by its waves per workgroup and its dynamic LDS in whole
// granules (cached per device, kernel and size; a benign race at worst computes the same value twice).  0: the query
// failed.
static int integrate_resident(IntegrateForm form, int wg, unsigned lds, int words = 1) {
    static int cache[2][IntegrateForm::N_INDEX][3][RCP_LDS_MAX + 1][64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    const unsigned granules = std::min((lds + LDS_GRANULE - 1) / LDS_GRANULE, RCP_LDS_MAX);
    int* c = &cache[words > 1][form.index()][wg == 1 ? 0 : wg == 2 ? 1 : 2][granules][dev];
    if (!*c) {
        int per_cu = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, integrate_kernel(form, wg, words), 64 * wg,
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
static int integrate_grid(IntegrateForm form) {
    const int r = integrate_resident(form, INT_WG, rcp_lds_bytes(form, RCP_N));
    return r ? r * INT_GRID_MULT : 4096;
}

// The launch of k_batch_integrate for a batch: kernel, waves per workgroup, dynamic LDS and grid.  A coarse form takes
// the smallest workgroup from the default up that keeps as many waves resident as four-wave workgroups would: the
// table's LDS bounds the workgroups per CU, so late in a long scan (rcp_hi towards RCP_N) one-wave workgroups would
// leave wave slots empty and the launch falls back to two and four waves.  The grid stays INT_GRID_MULT x the resident
// workgroups, so a headline batch's (unit, slice) items get one workgroup each.
struct IntLaunch {
    const void* fn;
    int wg, grid;
    unsigned lds;
};
static IntLaunch integrate_form(IntegrateForm form, int rcp_hi, int words) {
    IntLaunch f;
    f.lds = rcp_lds_bytes(form, rcp_hi);
    f.wg = INT_WG;
    if (!form.fine) {
        const int want = integrate_resident(form, INT_WG, f.lds, words) * INT_WG;  // waves
        const int forced = g_tsdf_hooks.int_wg;  // otx_integrate_workgroup: 1, 2 or 4 at every table size
        f.wg = forced > 0 ? forced : INT_WG_DEFAULT;
        while (forced <= 0 && f.wg < INT_WG && integrate_resident(form, f.wg, f.lds, words) * f.wg < want) f.wg *= 2;
    }
    f.fn = integrate_kernel(form, f.wg, words);
    const int r = integrate_resident(form, f.wg, f.lds, words);
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
// `form`: the batch's colour precision and division form; its slices (fine, kt) are set here, whatever they were.
static IntegrateForm slice_form(IntegrateForm form, int64_t est, bool deferred) {
    const TsdfHooks& h = g_tsdf_hooks;
    form.fine = false, form.kt = 1;
    const int64_t resident = integrate_grid(form) / INT_GRID_MULT;
    const int num = deferred ? DEFER_FINE_NUM : DIRECT_FINE_NUM, den = deferred ? DEFER_FINE_DEN : DIRECT_FINE_DEN;
    const bool small = est >= 0 && est * INT_PARTS * 4 * den < resident * num;
    const bool fine = h.int_fine > 0 || (deferred && h.fine_units >= 2 ? est >= 0 && est < h.fine_units
                                                                       : h.int_fine < 0 && small);
    if (!fine) return form;
    form.fine = true;
    form.kt = !deferred && h.int_depth > 0 ? h.int_depth : INT_FINE_KT;
    return form;
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
    launch_stage_mask(bf, q, work, wcount, smask, stream);
    launch_stage_tiles(bf, q, smask, stream);
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
    if (touch) launch_touch(bf, tp, vol->dev, bc.n, replay, plan.split, stream);
    const bool missing_only = replay && plan.mode != BatchMode::Deferred;
    int* wcopy = missing_only ? nullptr : plan.wcopy;
    launch_units(vol->dev, work, bc.pc, vol->hmail + OT_MAIL_WORDS, wcopy, ++vol->units_seq, bc.n, missing_only, stream);
    if (plan.split)  // (a replay: from the caller's frames, valid until this flush returns)
        launch_stage(bf, bc.sq, (const UnitWork*)work, (const int*)(wcopy ? wcopy : vol->dev.counters + bc.pc), bc.smask,
                     stream);
}

// k_batch_integrate over batch `bc`'s work list (`wcount` entries) on `stream`, in the form `form`
static ot_status launch_integrate(ot_tsdf* vol, const BatchCtx& bc, IntegrateForm form, const int* wcount,
                                  hipStream_t stream) {
    const BatchFrame* bf = vol->bset[bc.plan.set].bframes;
    const UnitWork* uw = (const UnitWork*)set_work(vol, bc.plan.set);
    void* args[] = {(void*)&bf, (void*)&bc.ip0, (void*)&vol->dev, (void*)&uw, (void*)&wcount};
    const IntLaunch f = integrate_form(form, bc.ip0.rcp_hi, bc.n > WORD_FRAMES ? FMASK_WORDS : 1);
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
// alone (next == nullptr: a flush, or a next batch that does not fuse).  The batch's colour precision and division
// form; its slices by the batch's unit count, known here (slice_form).
static ot_status launch_deferred(ot_tsdf* vol, hipStream_t stream, const BatchCtx* next) {
    if (!vol->dfr_on) return OT_OK;
    ot_status st = follow_deferred(vol, stream);
    if (st != OT_OK) return st;
    vol->dfr_on = false;
    const BatchCtx& D = vol->dfr;
    const IntegrateForm form = slice_form(D.form, vol->last_batch_slots, true);
    ProfPair timed;
    if ((st = prof_open(vol, timed, stream)) != OT_OK) return st;
    if (next) {
        OT_HIP_TRY(launch_integrate_touch(form, vol->bset[D.plan.set].bframes, D.ip0, vol->dev,
                                          (const UnitWork*)set_work(vol, D.plan.set), D.plan.wcount,
                                          integrate_grid(form), vol->bset[next->plan.set].bframes, next->tp, next->n,
                                          stream));
        OT_LAUNCH_CHECK();
    } else if ((st = launch_integrate(vol, D, form, D.plan.wcount, stream)) != OT_OK) {
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
        st = launch_integrate(vol, bc, bc.form, vol->dev.counters + bc.pc, stream);
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
    launch_copy_frames(host, bs.bframes, n, stream);
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
    bc.form.c64 = vol->color64, bc.form.fast = fast;
    // the table entries the batch can read: a weight is at most the frames since reset, so weight + 1 <= frame_id + n
    // (before frame_id advances; kept in the batch's context for a deferred launch or a replay)
    bc.ip0.rcp_hi = (int)std::min<int64_t>((int64_t)vol->frame_id + n, RCP_N);
    // (a deferred integrate takes its slices when it is launched, by its own unit count)
    if (plan.mode != BatchMode::Deferred) bc.form = slice_form(bc.form, direct_estimate(vol), false);

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
        if ((st = launch_integrate(vol, bc, bc.form, plan.wcount, is)) != OT_OK) return st;
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
