// tsdf.h — device layout of the scalable TSDF volume (pipelines.integration.ScalableTSDFVolume).
//
// HBM layout (one allocation per field group, sized at create time):
//   hash table  : open addressing, linear probing, capacity = pow2 >= 4 * max_units
//                 hkeys u64 (packed int3 unit key, KEY_EMPTY = ~0), hvals i32 (unit id, -1 = not allocated),
//                 fmask 3 x u64 (frames of the current batch touching the unit, two words, and a claim word)
//   unit pool   : max_units blocks of 16^3 voxels, field-planar inside a block:
//                 vox[id][field][z][x*16 + y], field = {tsdf, weight, r, g, b} (f32).  One 256-lane
//                 workgroup owns a block; lane (x, y) walks z, so every z step is one coalesced 1-KiB row
//                 per field (the per-column z walk is what reproduces Open3D's incremental float math).
//   unit_keys   : int32 [max_units][3]
// max_units and the hash capacity grow on demand (tsdf.hip grow_pool): Open3D's volume is unbounded.
#pragma once

#include <vector>

#include "common.h"

namespace ot {

constexpr int UNIT_RES = 16;
constexpr int UNIT_VOX = UNIT_RES * UNIT_RES * UNIT_RES;  // 4096
constexpr int UNIT_FIELDS = 5;
constexpr int UNIT_FLOATS = UNIT_FIELDS * UNIT_VOX;  // float32 colour record: 20480 floats = 80 KiB
constexpr int UNIT_FLOATS_C64 = 8 * UNIT_VOX;        // float64 colour record: tsdf, weight (f32) + r, g, b (f64) = 128 KiB

// counters[] slots
constexpr int C_UNUSED0 = 0;  // (was the per-frame path's touched count)
constexpr int C_UNITS = 1;     // units allocated
constexpr int C_OVERFLOW = 2;  // pool exhausted (units dropped)
constexpr int C_HASHERR = 3;   // hash full or key out of range
constexpr int C_BATCH_PAIRS = 4;  // (frame, unit) pairs of a batch: counters[4 + parity] (batches alternate, see k_batch_units)
constexpr int C_ORDER_HEAVY = 6;  // k_batch_units: work-list entries placed from the front (units seen by >= half the
constexpr int C_ORDER_LIGHT = 7;  // batch's frames) / from the back (the rest); the last workgroup zeroes both
constexpr int C_KMAX = 8;   // [8, 11): max over allocated units of key_a + KEY_BIAS + 1 (0: no unit yet)
constexpr int C_KNEG = 11;  // [11, 14): max over allocated units of KEY_BIAS - key_a + 1 (so min key_a = KEY_BIAS + 1 - it)
constexpr int C_UNITS_DONE = 14;  // k_batch_units: workgroups finished (the last one mails the counters, then zeroes it)
constexpr int N_COUNTERS = 16;

// stats[] slots (u64)
constexpr int S_UPDATES = 0;
constexpr int S_UNIT_INTEGRATIONS = 1;
// Wave-frames the slice pre-test took out of the coarse integrate's frame masks: counted over S_DROP_LINES words a
// cache line apart (one add per wave, the word by the workgroup's index -- tens of thousands of waves a launch on one
// more shared word queued behind one another in memory), summed into slot S_PRETEST_DROPPED by the read-out
constexpr int S_PRETEST_DROPPED = 2;
constexpr int S_DROP_BASE = 8, S_DROP_LINES = 256, S_DROP_STRIDE = 8;
// the integrate's voxel updates, spread the same way (lines of their own) and summed into S_UPDATES by the read-outs
constexpr int S_UPD_BASE = S_DROP_BASE + S_DROP_LINES * S_DROP_STRIDE;
constexpr int N_STATS = S_UPD_BASE + S_DROP_LINES * S_DROP_STRIDE;

struct TsdfDev {
    unsigned long long* hkeys;
    int* hvals;
    int* counters;
    unsigned long long* stats;
    int* unit_keys;
    float* vox;                 // unit pool: max_units records of unit_floats floats
    int unit_floats;            // record stride: UNIT_FLOATS (float32 colour / NoColor) or UNIT_FLOATS_C64
    int color64;                // 1: the record's colour planes are float64 (colour precision 64, RGB8 volumes)
    // per hash slot, FMASK_STRIDE words: the frames of the current batch that touch the unit (frame f is bit f & 63 of
    // word f >> 6, at fmask[slot * FMASK_STRIDE + (f >> 6)]), then the slot's claim word (FMASK_CLAIM)
    unsigned long long* fmask;
    int* bslots;                // hash slots touched by the current batch (first-touch order)
    void* work;                 // per touched slot of the batch: unit header (UnitWork, 32 B) for the integrate
    int hash_mask;
    int max_units;
    int shard_rank;   // spatial sharding of one volume over `shard_world` GPUs: this volume keeps only the units
    int shard_world;  // with owner(key) == shard_rank (<= 1: no sharding)
    int shard_shift;  // ownership granularity: blocks of 2^shift units per axis share an owner
    int shard_mode;   // SHARD_BLOCKS: hashed blocks of 2^shift units; SHARD_SECTORS: azimuth sectors around a centre
    int shard_cx2, shard_cy2;  // sector centre in half units (round(2 * centre / unit_length)) per axis
};
// Frame masks: two 64-bit words per slot, so a batch has up to 128 frames.  A touch workgroup's frames lie in one word
// and it merges its bits with one atomicOr on that word.  In a batch of more than 64 frames the first bits of the two
// words may be set by different workgroups at the same time, so "the old word was 0" no longer says "first touch of the
// batch": the workgroup that sets a word's first bits then also draws the slot's claim (atomicExch on the slot's third
// word), and the one that finds it free lists the slot in bslots -- once per batch, whichever word came first.
// k_batch_units clears all three words.
constexpr int FMASK_WORDS = 2;
constexpr int FMASK_CLAIM = FMASK_WORDS;       // index of the claim word in a slot's words
constexpr int FMASK_STRIDE = FMASK_WORDS + 1;  // u64 words per slot
constexpr int WORD_FRAMES = 64;  // frames per mask word: the batch cap of everything that reads one word only
inline size_t fmask_bytes(int64_t cap) { return sizeof(unsigned long long) * FMASK_STRIDE * (size_t)cap; }
constexpr int SHARD_BLOCKS = 0;
constexpr int SHARD_SECTORS = 1;

// owner rank of a unit, a function of its key alone (exact on host and device: integers only).
// SHARD_BLOCKS: a hash of its block key (unit key >> shard_shift per axis), independent of the table's slot hash
// mix64(key), so a shard's keys still spread over all slots.  Blocks of units keep most marching-cubes neighbours on one
// rank (the border halo only crosses block faces) while still balancing the ranks' units.
// SHARD_SECTORS (round 6): the azimuth sector of the unit's centre around the scan centre (x, y).  A ring scan's frames
// each see a contiguous arc of the object, so a rank's units project into a fraction of every frame and its front end
// stages only those tiles (tools/shard_sector_model.py: 0.23 of the pixels at 8 ranks against 0.54 for blocks).  The
// sector is floor(N * pa / 4) of the pseudo-angle pa = quadrant + a / (a + b) in [0, 4), exact in int64 (the octants at
// N = 8 and the quadrants at N = 4 are the true 45 / 90 degree sectors); the centre point itself goes to sector 0.
__host__ __device__ inline int unit_sector(long long X, long long Y, int n) {
    if (X == 0 && Y == 0) return 0;
    long long a, b, q;
    if (X > 0 && Y >= 0) { q = 0; a = Y; b = X; }
    else if (X <= 0 && Y > 0) { q = 1; a = -X; b = Y; }
    else if (X < 0 && Y <= 0) { q = 2; a = -Y; b = -X; }
    else { q = 3; a = X; b = -Y; }
    return (int)(((q * (a + b) + a) * (long long)n) / (4 * (a + b)));
}
__host__ __device__ inline int unit_owner(const TsdfDev& d, int x, int y, int z) {
    if (d.shard_mode == SHARD_SECTORS)
        return unit_sector(2ll * x + 1 - d.shard_cx2, 2ll * y + 1 - d.shard_cy2, d.shard_world);
    const unsigned long long bk = pack_key(x >> d.shard_shift, y >> d.shard_shift, z >> d.shard_shift);
    return (int)((unsigned)(mix64(bk + 0x9E3779B97F4A7C15ull) >> 32) % (unsigned)d.shard_world);
}
__host__ __device__ inline bool unit_owned(const TsdfDev& d, unsigned long long key) {
    if (d.shard_world <= 1) return true;
    int x, y, z;
    unpack_key(key, x, y, z);
    if (d.shard_mode == SHARD_SECTORS) {  // unit_sector(...) == rank without the division: 4 r s <= N v < 4 (r + 1) s
        const long long X = 2ll * x + 1 - d.shard_cx2, Y = 2ll * y + 1 - d.shard_cy2;
        if (X == 0 && Y == 0) return d.shard_rank == 0;
        long long a, b, q;
        if (X > 0 && Y >= 0) { q = 0; a = Y; b = X; }
        else if (X <= 0 && Y > 0) { q = 1; a = -X; b = Y; }
        else if (X < 0 && Y <= 0) { q = 2; a = -Y; b = -X; }
        else { q = 3; a = X; b = -Y; }
        const long long s = a + b, v = (q * s + a) * (long long)d.shard_world;
        return v >= 4ll * d.shard_rank * s && v < 4ll * (d.shard_rank + 1) * s;
    }
    return unit_owner(d, x, y, z) == d.shard_rank;
}

// a newly allocated unit widens the volume's key bounds (read back with the counters: the sorted-unit order packs keys
// on their actual ranges without a bounds pass)
__device__ inline void note_unit_key(const TsdfDev& d, int x, int y, int z) {
    const int k[3] = {x, y, z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        atomicMax(&d.counters[C_KMAX + a], k[a] + KEY_BIAS + 1);
        atomicMax(&d.counters[C_KNEG + a], KEY_BIAS - k[a] + 1);
    }
}

__device__ inline int hash_insert(const TsdfDev& d, unsigned long long key) {
    unsigned slot = (unsigned)mix64(key) & (unsigned)d.hash_mask;
    for (int probe = 0; probe <= d.hash_mask; ++probe) {
        const unsigned long long k = d.hkeys[slot];
        if (k == key) return (int)slot;
        if (k == KEY_EMPTY) {
            const unsigned long long old = atomicCAS(&d.hkeys[slot], KEY_EMPTY, key);
            if (old == KEY_EMPTY || old == key) return (int)slot;
        }
        slot = (slot + 1) & (unsigned)d.hash_mask;
    }
    return -1;
}

__device__ inline int hash_find(const TsdfDev& d, unsigned long long key) {
    unsigned slot = (unsigned)mix64(key) & (unsigned)d.hash_mask;
    for (int probe = 0; probe <= d.hash_mask; ++probe) {
        const unsigned long long k = d.hkeys[slot];
        if (k == key) return (int)slot;
        if (k == KEY_EMPTY) return -1;
        slot = (slot + 1) & (unsigned)d.hash_mask;
    }
    return -1;
}

// a unit's record: tsdf plane, weight plane, then the colour planes r, g, b (4096 each, voxel vi = z*256 + x*16 + y)
// in float32 or, when the volume keeps colour at Open3D's precision, float64 (the record is then 128 KiB)
__host__ __device__ inline float* unit_base(const TsdfDev& d, int id) { return d.vox + (size_t)id * d.unit_floats; }
template <typename CT>
__device__ inline CT* color_base(const TsdfDev& d, int id) {
    return reinterpret_cast<CT*>(unit_base(d, id) + 2 * UNIT_VOX);
}

// Border voxels of a unit: every voxel with x == 0, y == 0 or z == 0 (3 * 256 - 3 * 16 + 1 = 721), the only
// voxels of a unit that marching cubes reads from its -x/-y/-z neighbours (the 17^3 tile of a unit is the unit plus
// the low faces of its +1 neighbours).  Order: increasing Open3D index x*256 + y*16 + z.
constexpr int BORDER_VOX = 721;
__host__ __device__ inline void border_voxel(int b, int& x, int& y, int& z) {
    if (b < 256) {
        x = 0, y = b >> 4, z = b & 15;
        return;
    }
    const int c = b - 256, r = c % 31;
    x = 1 + c / 31;
    if (r < 16) y = 0, z = r;
    else y = r - 15, z = 0;
}

// frames per batch: one bit each in a slot's FMASK_WORDS mask words.  A whole volume whose batches run BatchMode::Direct
// takes up to MAX_BATCH; a sharded volume and the overlap, deferred and split modes read one word and keep WORD_FRAMES
// (tsdf.hip batch_cap decides, once, for every caller)
constexpr int MAX_BATCH = FMASK_WORDS * WORD_FRAMES;
constexpr int OT_MAIL_WORDS = 64;  // capacity of the pinned host mailbox (4-B words per read-back, mail_words)
// sequence words of the kernels that mail on their own (mail_wait): the marching-cubes scans (words 62, 63: one per
// scan block) and the units kernel's counters (the last word of the second half)
constexpr int MAIL_SEQ_MC = OT_MAIL_WORDS - 2;
constexpr int MAIL_SEQ_UNITS = 2 * OT_MAIL_WORDS - 1;

// per-frame parameters of a batch (device resident)
struct BatchFrame {
    const uint16_t* depth16;  // raw depth (u16 path) or nullptr
    const float* depthf;      // caller's float depth (float path) or nullptr
    const uint8_t* color;     // caller's RGB8 or nullptr
    uint2* dc;                // staged per-pixel record: .x the float depth's bits, .y the colour r | g << 8 | b << 16
                              // (0 without colour); 8 B per pixel -- the ray multiplier is the volume's one table
    uint64_t pad;             // (the struct is copied in 16-B words)
    double pose[12];          // rows 0..2 of inverse(extrinsic) (stride unprojection, float64)
    float E[12];              // rows 0..2 of (float)extrinsic
    float es[3];              // column 2 of (float)extrinsic * voxel_length
    float scale;              // (float)depth_scale
    double trunc;             // depth_trunc
};

// parameters of the integrate kernels (tsdf.hip make_integrate_params)
struct IntegrateParams {
    const float* depth;
    const uint8_t* color;
    const float* mult;  // the volume's ray-multiplier table [H][W]: gathered by the lanes that can update
    int W, H;
    float fx, fy, cx, cy;
    float E[12];
    float es0, es1, es2;
    float vl, half, trunc, trunc_inv, safe_w, safe_h;
    float inv_fx, inv_fy;  // (float)(1 / (float)fx) as CreateDepthToCameraDistanceMultiplierFloatImage
    float proj_eps;  // certified fast projection: |u - rint(u)| > proj_eps decides floor and bounds exactly
    int rcp_hi;      // FAST kernels: the largest weight + 1 of the batch (frames since reset + the batch's), <= RCP_N
    double unit_len;
    // slice pre-test (slice_pretest.h): the batch's tile-max depth maps, frame f's at tmax + f * tmax_tiles; nullptr: none
    // (the batch was not staged in full, or the pre-test is off), and the integrate is the one without it
    const unsigned* tmax;
    int tmax_tiles;  // tiles per frame
    int tmax_words;  // the maps' words in all (frames x tiles: the gathers' range check)
};

// parameters of the touch kernels (tsdf.hip make_touch_params)
struct BatchTouchParams {
    int W, stride, ws, hs;
    double fx, fy, cx, cy;
    double trunc, unit_len;
    double inv_unit;    // RN(1 / unit_len): floor_div's certified product
    int slot_cap;
    int64_t npx;        // pixels per frame (fused staging: k_batch_touch stages the batch's pixels too)
    int pc;             // this batch's pair counter index
    int tiles;          // touch workgroups per frame group (blockIdx.x below it)
    int stage_blocks;   // staging-only workgroups per frame group after them (0: each touch workgroup stages a share)
    int tf;             // frames per group (TF)
    int sample_stage;   // split front end (stage_blocks < 0): each stride sample stores its own pixel's staged record
                        // (a replay touch reads it; k_stage_tiles stages only the owned units' footprints)
    unsigned* tmax;     // the set's tile-max depth maps, written by the staging (frame f's at tmax + f * tiles); nullptr: none
    int H;
    int onepass;        // eligible frames are staged in 8 x 8 tile order and their map words reduced from the depths in
                        // registers (tsdf_stage.h stage_tile_quads); 0: every frame by pixel chunks, the map from a second read
};

// The split front end's staging tile and the layout of its tile masks (k_stage_mask, k_stage_tiles: tsdf_frontend.hip;
// the host sizes the masks and refuses frames they do not fit: tsdf.hip tmask_fits)
constexpr int STX = 32, STY = 16;  // staging tile: 32 pixels (one 8-lane group of quads per row) x 16 rows
constexpr int SM_WORDS = 2048;  // LDS map words: tile rows * words per row (8 KiB; 16K x 16K-pixel frames)
constexpr int SM_PARTS = 4;     // mask workgroups (and maps) per frame
constexpr int ST_MAX_TILES_X = 256;
// parameters of the split front end's tile-mask kernel (tsdf.hip make_stage_params)
struct StageMaskParams {
    int W, H, tiles_x, tiles_y, wpr;  // wpr: 32-bit mask words per tile row
    float fx, fy, cx, cy, vl, half;
    double unit_len;
    int nframes;
};

// an entry of a batch's work list (k_batch_units -> the integrate)
struct UnitWork {
    int id;                   // pool id, | 0x80000000 when fresh (state starts at zero), -1 when dropped
    int kx, ky, kz;           // unit key
    unsigned long long mask;   // frames of the batch that touch the unit (bit f = frame f), frames 0..63
    unsigned long long mask1;  // frames 64..127 (bit f - 64); 0 in a batch of at most 64 frames
};
// a sharded volume's work list: units seen by this many of the batch's frames or more are listed from the front, the
// rest from the back (k_batch_units writes it so, the fused launches' integrate_body reads it so)
constexpr int WORK_HEAVY_FRAMES = 32;

// The form of a batch's integrate: which instantiation of k_batch_integrate / k_integrate_touch runs it.
struct IntegrateForm {
    bool c64 = false;   // colour state in float64 (the volume's colour precision)
    bool fast = false;  // quotients from the reciprocal table (tsdf_integrate.h RCP_N) instead of IEEE divisions
    bool fine = false;  // fine slices: 2 voxels per lane along z, 32 waves per unit instead of 16 -- for batches with
                        // few units (tsdf.hip slice_form)
    int kt = 1;         // a fine form's frame pipeline depth KT, 1..3 (integrate_item's ZB == 2 loop); 1 when coarse
    // dense index over the forms, below N_INDEX (the occupancy cache)
    static constexpr int N_INDEX = 32;
    int index() const { return (c64 ? 2 : 0) + (fast ? 1 : 0) + (fine ? 4 + ((kt - 1) << 3) : 0); }
};

// How a batch runs (tsdf.hip plan_batch chooses once per batch; everything after it reads the plan):
//   Direct   : front end and integrate on the caller's stream, set 0
//   Overlap  : double-buffered front end -- the integrate on the volume's integrate stream behind the set's units kernel
//   Deferred : the integrate waits to be launched with the next batch's touch (k_integrate_touch), or alone
enum class BatchMode { Direct, Overlap, Deferred };
struct BatchPlan {
    BatchMode mode = BatchMode::Direct;
    bool split = false;     // split front end: touch without staging -> units -> tile mask -> staging of the marked tiles
    bool pretest = false;   // the staging builds the tile-max maps and the coarse integrate drops idle frames per slice
    int set = 0;            // the batch's staging set (ot_tsdf::bset; its work list: tsdf.hip set_work -- resolved at each
                            // launch, pool growth reallocates the lists)
    int* wcount = nullptr;  // where the integrate reads the work list's length: the batch's pair counter, or ...
    int* wcopy = nullptr;   // ... the set's copy the units kernel writes (Overlap, Deferred; nullptr: Direct)
};

// the context a batch's settle, a replay and a deferred launch need
struct BatchCtx {
    BatchPlan plan;
    BatchTouchParams tp;
    IntegrateParams ip0;
    StageMaskParams sq{};       // split: a replay stages its units' tiles too (units the full hash dropped were in no
    unsigned* smask = nullptr;  // work list of the first pass, so their footprints were never staged); the tile masks
    int n, pc;
    IntegrateForm form;
};

struct PendingFrame {
    const uint16_t* depth;  // u16 path (nullptr for the float path)
    const float* depthf;    // float path
    const uint8_t* color;
    ot_intrinsics intr;
    double extrinsic[16];
    double depth_scale, depth_trunc;
};

struct MeshBuffers {
    // the marching-cubes structure of the last extraction (per-unit cube bytes, triangle offsets, ...; mc.hip
    // mc_layout), kept with the volume so ComputeVertexNormals can walk each vertex's cubes instead of sorting corners
    void* ws = nullptr;
    size_t ws_bytes = 0;
    int64_t ws_units = 0;
    int64_t serial = 0;   // extraction count; the structure is valid for `serial` while `valid`
    bool valid = false;   // cleared by anything that changes the volume (integrate, reset, import)
    bool internal = false;  // the last extraction's mesh sits in v / c / t (else it was emitted to the caller)
    bool emitted = false;   // the merge keys vk / tk of the last extraction are written (by an emission)
    double* v = nullptr;
    double* c = nullptr;
    int32_t* t = nullptr;
    int4* vk = nullptr;     // per vertex: owner unit key (x, y, z) and edge bit (local voxel * 3 + axis)
    int* vown = nullptr;    // per vertex: owner unit id (the vertex-normal walk starts from it: no hash probe)
    int32_t* tk = nullptr;  // per triangle: its cube's unit key (x, y, z)
    int64_t nv = 0, nt = 0;
    int64_t cap_v = 0, cap_t = 0, cap_vk = 0, cap_tk = 0, cap_vown = 0;
};

// Per-unit counts and output bases of the last point-cloud count (tsdf_cloud.hip), by unit rank in key order: the
// zero-crossing cloud's points and the voxel cloud's points.  Its own workspace: a cloud extraction leaves the
// marching-cubes structure (MeshBuffers) as it is.
struct CloudBuffers {
    void* ws = nullptr;  // long long [4][units]: surface counts, voxel counts, surface bases, voxel bases
    size_t ws_bytes = 0;
    int64_t units = 0;
    int64_t n_surface = 0, n_voxel = 0;
    bool valid = false;  // cleared by anything that changes the volume (integrate, reset, import)
};

}  // namespace ot

struct ot_tsdf {
    int device = 0;
    double voxel_length = 0.0, sdf_trunc = 0.0, unit_length = 0.0;
    int color_type = 1, stride = 4;
    bool color64 = false;  // colour state in float64 (Open3D's Vector3d) instead of float32
    int64_t max_units = 0;  // current pool capacity (grows: grow_pool)
    int64_t hash_cap = 0;
    ot::TsdfDev dev{};
    int frame_id = 0;
    bool imported = false;  // units imported since reset (arbitrary state: no reciprocal-table integrate)
    // multiplier image cache
    float* mult = nullptr;
    ot_intrinsics mult_intr{};
    bool mult_valid = false;
    // batching of integrate_u16: frames per fused launch (ot_tsdf_set_batch; capped by tsdf.hip batch_cap; default: §4.1)
    int batch_max = ot::MAX_BATCH;
    std::vector<ot::PendingFrame> pending;
    ot::BatchFrame* hbframes = nullptr;    // pinned host staging [2][MAX_BATCH]
    unsigned* hmail = nullptr;             // pinned coherent host mailbox [OT_MAIL_WORDS]: small read-backs stored
                                           // by a one-wave kernel (mail_words) instead of staged D2H copies
    // staging half of the next batch; a batch's parameter copy has run once its units kernel has mailed (tsdf.hip
    // settle_batch waits for that before integrate_batch returns), so the halves need no event
    int hb_next = 0;
    // the counters as the last batch's units kernel left them (the integrate does not change them), mailed by its last
    // workgroup to hmail + OT_MAIL_WORDS, then sequence number `units_seq` to word MAIL_SEQ_UNITS: the host spins on
    // that word (mail_wait) instead of an event behind the units kernel -- an event recorded between two kernels of a
    // stream idles the GPU ~4 us (tools/event_gap.hip, r05j) -- and an extraction reads the unit count without waiting
    // for the integrate (valid while early_frame == frame_id, no reset or import since)
    unsigned units_seq = 0;
    int early_frame = -1;
    unsigned mc_seq = 0;  // the marching-cubes totals' sequence number (words MAIL_SEQ_MC, MAIL_SEQ_MC + 1)
    int batch_pc = ot::C_BATCH_PAIRS;      // pair counter of the next batch (alternates 4, 5)
    // A batch's staging: per-frame parameters, the packed (depth, colour) record per pixel, and the unit work list.
    // Two sets: with the front end double-buffered (overlap, ot_tsdf_set_frontend_overlap: off by default, measured slower
    // sharded volume, whose integrate is 1/N of the work) batch k+1's staging / touch / units run on the caller's stream
    // while batch k's integrate runs on `istream`; otherwise set 0 only, everything on the caller's stream.
    struct BatchSet {
        ot::BatchFrame* bframes = nullptr;  // device [MAX_BATCH]
        uint2* bdc = nullptr;               // device [batch][h][w] packed (depth, colour) records
        int64_t cap = 0;                    // pixels (frames * h * w) the buffer holds
        unsigned* tmax = nullptr;           // device [batch][tile rows][tile columns]: largest staged depth per 8 x 8
        int64_t tmax_cap = 0;               // pixel tile (slice_pretest.h), words the buffer holds
        void* work = nullptr;               // UnitWork [hash_cap]; set 0 uses dev.work
        hipEvent_t ev_units = nullptr;      // the set's units kernel (its integrate waits for it)
        hipEvent_t ev_done = nullptr;       // the set's integrate (the set's next front end waits for it)
    } bset[2];
    int overlap_mode = -1;        // -1 (default) and 0 off, 1 on
    // Split front end of a sharded volume (round 6): the touch stages nothing (only each stride sample's own pixel, for a
    // replay), k_stage_mask marks the image tiles the batch's owned units can project to, k_stage_tiles stages those.
    unsigned* tmask = nullptr;    // device [WORD_FRAMES][tile rows][words per row] (split batches keep one mask word)
    int64_t tmask_words = 0;
    int tmask_w = 0, tmask_h = 0;  // the image size the masks are laid out for
    int split_mode = -1;          // -1 (default): split for sharded volumes; 0 off; 1 on (test hook)
    // Deferred integrate of a sharded volume's last batch (round 6): its front end ran, its integrate waits to be launched
    // together with the next batch's touch (k_integrate_touch) or alone -- by the next flush, or by the next batch when
    // that one does not fuse (tsdf.hip integrate_batch owns the hand-over).  dfr holds the batch's context while dfr_on,
    // dfr_stream the stream its front end ran on.
    bool dfr_on = false;
    hipStream_t dfr_stream = nullptr;
    hipEvent_t ev_dfr = nullptr;  // dfr_stream -> the next batch or a flush on another stream
    ot::BatchCtx dfr;
    // batch statistics since reset (ot_tsdf_batch_stats; the bench's compulsory-bytes figure): batches, units touched
    // summed over batches, units new in their batch; units the last batch left (-1: unknown after an import)
    int64_t stat_batches = 0, stat_unit_batches = 0, stat_fresh = 0, stat_prev_units = 0;
    int64_t last_batch_slots = -1;  // units the last batch touched (mailed): the next batch's integrate granularity
    int bset_next = 0;            // set of the next batch (alternates in overlap mode)
    // the last batch's staging (otx_tsdf_staged): its set, frames, image size and whether it wrote tile-max maps
    int staged_set = -1, staged_n = 0, staged_w = 0, staged_h = 0;
    bool staged_map = false;
    int last_set = -1;            // set of the last batch whose integrate ran on istream (joined by readers)
    hipStream_t istream = nullptr;
    int* wcount = nullptr;        // device [2]: the sets' work-list lengths (k_batch_units -> k_batch_integrate)
    // sorted-unit cache (rank -> id), valid for `sorted_units` units
    unsigned* sorted_ids = nullptr;
    int64_t sorted_units = -1;
    int sorted_frame = -1;
    // extracted mesh
    ot::MeshBuffers mesh;
    ot::CloudBuffers cloud;
    // a second stream for independent extraction stages (vertex positions beside triangle indices), fork / join
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // deferred vertex normals (ot_tsdf_mesh_vertex_normals on the caller's side stream) read the marching-cubes
    // structure (mesh.ws, vk, vown): work that rewrites it or the units waits for this event first (wait_normals)
    hipEvent_t ev_normals = nullptr;
    bool normals_pending = false;
    hipEvent_t ev_made = nullptr;  // ot_tsdf_extract_sample_min_z: the mesh arrays are complete (the normals wait on it)
    // kernel timing (events around the dominant integration kernel)
    bool profiling = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
    double prof_ms = 0.0;
    int64_t prof_launches = 0;
    // and around each batch's front end (staging + touch + units), the part a sharded volume does not divide
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_fe_events;
    double prof_fe_ms = 0.0;
    int64_t prof_fe_batches = 0;
};

namespace ot {
// The TSDF test hooks (process-wide; set by the otx_* entry points of tsdf_volume.hip, -1 / false: the default rule).
struct TsdfHooks {
    int int_fine = -1;     // otx_integrate_fine: slice form by the batch's size (-1), 0 coarse, 1 fine
    int fine_units = -1;   // otx_integrate_fine >= 2: the deferred integrate takes the fine slices below this many units
    int int_depth = -1;    // otx_integrate_depth: frame pipeline depth KT of the fine slices, 1..3
    int int_wg = -1;       // otx_integrate_workgroup: waves per workgroup of the coarse integrate, 1, 2 or 4
    int stage_blocks = -1; // otx_touch_stage_blocks: staging-only touch workgroups (-1: two per tile)
    int touch_tf = -1;     // otx_touch_frames: frames per touch workgroup (-1: TF)
    int split = -1;        // otx_split_frontend: by the volume (-1), 0 never, 1 always (unsharded too)
    int defer = -1;        // otx_defer_integrate: by the volume (-1), 0 never, 1 with any split batch
    int pretest = -1;      // otx_slice_pretest: whole volumes' full staging (-1), 0 never, 1 every batch staged in full
    int onepass = -1;      // otx_stage_onepass: staging and tile-max map in one pass where eligible (-1), 0 never
    bool unit_sort_radix = false;  // otx_unit_sort_radix: the radix sort at every key width
};
extern TsdfHooks g_tsdf_hooks;

// The launchers of the integrate pipeline's kernels: the only way from the host batch pipeline (tsdf.hip) to a kernel.
// Each translation unit below holds its kernels and chooses between their forms; no other file names them.
// tsdf_frontend.hip -- n: the batch's frames (more than WORD_FRAMES: the two-word forms)
void launch_copy_frames(const BatchFrame* host, BatchFrame* dev, int n, hipStream_t stream);
// replay: from the staged depths, no staging; split: the split front end's touch (k_batch_touch_split)
void launch_touch(const BatchFrame* frames, const BatchTouchParams& tp, const TsdfDev& dev, int n, bool replay,
                  bool split, hipStream_t stream);
// missing_only: a replay that lists only the units without an id (k_batch_units<true, ..>)
void launch_units(const TsdfDev& dev, UnitWork* work, int pc, unsigned* early_mail, int* wcount, unsigned seq, int n,
                  bool missing_only, hipStream_t stream);
void launch_stage_mask(const BatchFrame* frames, const StageMaskParams& q, const UnitWork* work, const int* wcount,
                       unsigned* smask, hipStream_t stream);
void launch_stage_tiles(const BatchFrame* frames, const StageMaskParams& q, const unsigned* smask, hipStream_t stream);
// tsdf_integrate.hip, tsdf_integrate_wide.hip -- the k_batch_integrate of a form with `wg` waves per workgroup (coarse:
// 1, 2 or 4; fine: INT_WG) reading one mask word / FMASK_WORDS, as hipLaunchKernel and the occupancy query take it
const void* integrate_kernel_word(IntegrateForm form, int wg);
const void* integrate_kernel_wide(IntegrateForm form, int wg);
// tsdf_fused.hip -- k_integrate_touch / k_integrate_touch_fine: `nint` integrate workgroups over the deferred batch, then
// the touch tiles of the next batch's `tn` frames
hipError_t launch_integrate_touch(IntegrateForm form, const BatchFrame* frames, const IntegrateParams& p,
                                  const TsdfDev& dev, const UnitWork* work, const int* wcount, int nint,
                                  const BatchFrame* tframes, const BatchTouchParams& tp, int tn, hipStream_t stream);

// shared by tsdf.hip (the batch pipeline), tsdf_exchange.hip (unit order, export, import, border halo) and
// tsdf_volume.hip (create, reset, settings, read-outs, hooks):
// room for `extra` more units before a kernel that allocates up to that many (imports): the pool grows now if needed
ot_status reserve_units(ot_tsdf* vol, int64_t extra, hipStream_t stream);
// the units an export lists: every unit in key order or, for a sharded volume, its own
ot_status export_list(ot_tsdf* vol, hipStream_t stream, const unsigned** ids, int64_t* n);
// shared with mc.hip
ot_status tsdf_sorted_units(ot_tsdf* vol, hipStream_t stream, int64_t* n_units);
// small read-back: the 4-byte words at p[0 .. n) copied to vol->hmail by one kernel, then the stream synchronised
struct MailSrc {
    const unsigned* p[ot::OT_MAIL_WORDS];
    int n;
};
ot_status mail_words(ot_tsdf* vol, const MailSrc& s, hipStream_t stream);
// spin until a kernel on `stream` stores `seq` to the mailbox word (system-scope release after its mailed values); the
// stream is polled now and then, so a fault or a drained stream without the mail ends the wait with an error
ot_status mail_wait(const unsigned* word, unsigned seq, hipStream_t stream);
// integrate the queued frames; readers (join = true) also order `stream` after the last batch's integrate when it ran on
// the volume's integrate stream (double-buffered front end)
ot_status tsdf_flush(ot_tsdf* vol, hipStream_t stream, bool join = true);
// order `stream` after the volume's deferred vertex normals, if any are still in flight
ot_status wait_normals(ot_tsdf* vol, hipStream_t stream);
// the fused sampler's two phases (mesh_ops.hip): queue the chains + emission on `stream`, then wait for the kept counts.
// mark (nullable) is recorded on `stream` just before the area-sum walk (mark_at 1) or the CDF walk (mark_at 2)
ot_status sample_min_z_enqueue(const ot_mesh_sample_job* jobs, int32_t n_jobs, int64_t n_points, uint64_t seed,
                               double z_min, hipStream_t stream, hipStream_t* hs, hipEvent_t mark = nullptr,
                               int mark_at = 0);
ot_status sample_min_z_wait(hipStream_t hs, int32_t n_jobs, int64_t* n_kept_host);
}  // namespace ot
