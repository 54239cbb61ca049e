// tsdf_volume.hip — a ScalableTSDFVolume's life cycle and everything around the integrate: create, destroy, reset,
// settings, counters, statistics, the profiling read-out, the shard setters, the pinned mailbox and the test hooks
// (layout: tsdf.h; the integrate: tsdf.hip and the kernel files it launches; the unit exchange: tsdf_exchange.hip).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <sched.h>
#include <thread>

#include "slice_pretest.h"
#include "tsdf.h"

namespace ot {

TsdfHooks g_tsdf_hooks;

// the host state a reset returns to its start (the device side: the callers' clears)
static void reset_host_state(ot_tsdf* v) {
    v->batch_pc = C_BATCH_PAIRS;
    v->frame_id = 0;
    v->imported = false;
    v->early_frame = -1;
    v->last_batch_slots = -1;
    v->stat_batches = v->stat_unit_batches = v->stat_fresh = v->stat_prev_units = 0;
    v->sorted_frame = -1;
    v->sorted_units = -1;
    v->mesh.nv = v->mesh.nt = 0;
    v->mesh.valid = false;
    v->cloud.valid = false;
}

// one wave copies n <= OT_MAIL_WORDS 4-byte words into the volume's pinned coherent mailbox (plain vector stores over
// PCIe); the caller synchronises the stream and reads vol->hmail.  One launch replaces a staged D2H copy per value
__global__ void k_mail_words(MailSrc s, unsigned* __restrict__ out) {
    const int i = threadIdx.x;
    if (i < s.n) out[i] = *s.p[i];
}

ot_status mail_words(ot_tsdf* vol, const MailSrc& s, hipStream_t stream) {
    if (s.n > MAIL_SEQ_MC) return fail(OT_ERR_INVALID_ARGUMENT, "mailbox overflow");
    hipLaunchKernelGGL(k_mail_words, dim3(1), dim3(64), 0, stream, s, vol->hmail);
    OT_LAUNCH_CHECK();
    OT_HIP_TRY(hipStreamSynchronize(stream));
    return OT_OK;
}

// The stream is polled only once the wait has lasted 20 ms (then every ~1 ms): a stream query puts commands on the
// stream's queue, and while the host spins the queue already holds the work launched after the mailing kernel -- polling
// every ~20 us had left ~6 us of idle GPU behind that work at each wait (host launch trace against the kernel trace,
// tools/launch_lag.py, r05ah: the gaps before the unit sort and before the sampler).
// Host CPU bound: the loop spins with `pause` only for the first ~50 us -- the mails the headline
// waits for arrive within that (the units kernel ~10 us after the touch, the marching-cubes totals) -- then yields the
// core on every check (sched_yield: a rank's other threads and RCCL's proxy threads get it), and past 2 ms sleeps
// 20 us per check, so 8 ranks x 2 object streams waiting on a long kernel do not hold 16 cores at 100 %.
ot_status mail_wait(const unsigned* word, unsigned seq, hipStream_t stream) {
    using clk = std::chrono::steady_clock;
    const clk::time_point t0 = clk::now();
    const clk::time_point t_yield = t0 + std::chrono::microseconds(50);
    const clk::time_point t_sleep = t0 + std::chrono::milliseconds(2);
    clk::time_point next = t0 + std::chrono::milliseconds(20);
    for (unsigned it = 1;; ++it) {
        if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == seq) return OT_OK;
        const bool spin = (it & 63u) != 0;
        if (spin && it < (1u << 20)) {  // the clock is read every 64 polls while spinning
            __builtin_ia32_pause();
            continue;
        }
        const clk::time_point now = clk::now();
        if (now < t_yield) {
            __builtin_ia32_pause();
            continue;
        }
        it = 1u << 20;  // from here every poll reads the clock
        if (now >= next) {  // has the stream faulted, or drained without the mail?
            next = now + std::chrono::milliseconds(1);
            const hipError_t q = hipStreamQuery(stream);
            if (q == hipSuccess) {
                if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == seq) return OT_OK;
                return fail(OT_ERR_HIP, "mailbox: the stream drained without the kernel's mail");
            }
            if (q != hipErrorNotReady) OT_HIP_TRY(q);
        }
        if (now < t_sleep) sched_yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}

__global__ __launch_bounds__(256) void k_tsdf_clear(TsdfDev d, int64_t cap) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cap; i += (int64_t)gridDim.x * 256) {
        d.hkeys[i] = ~0ull;
        d.hvals[i] = -1;
        for (int k = 0; k < FMASK_STRIDE; ++k) d.fmask[i * FMASK_STRIDE + k] = 0ull;
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x < N_COUNTERS) d.counters[threadIdx.x] = 0;
        for (int i = threadIdx.x; i < N_STATS; i += 256) d.stats[i] = 0ull;
    }
}

}  // namespace ot

using namespace ot;

extern "C" {

ot_status ot_tsdf_create(double voxel_length, double sdf_trunc, int32_t color_type, int32_t unit_res, int32_t stride,
                         int64_t max_units, ot_tsdf** out) {
    if (!out) return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume] out is NULL");
    *out = nullptr;
    if (!(voxel_length > 0.0) || !(sdf_trunc > 0.0))
        return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume] voxel_length and sdf_trunc must be positive");
    if (unit_res != UNIT_RES)
        return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume] only volume_unit_resolution=16 is supported");
    if (stride < 1) return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume] depth_sampling_stride must be >= 1");
    if (color_type != OT_COLOR_NONE && color_type != OT_COLOR_RGB8)
        return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume] unsupported color_type (NoColor or RGB8)");
    if (max_units <= 0) max_units = 32768;
    if (max_units > (1 << 24)) return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume] max_units too large");
    ot_tsdf* v = new ot_tsdf();
    (void)hipGetDevice(&v->device);
    v->voxel_length = voxel_length;
    v->sdf_trunc = sdf_trunc;
    v->unit_length = voxel_length * (double)UNIT_RES;
    v->color_type = color_type;
    v->stride = stride;
    v->max_units = max_units;
    int64_t cap = 1;
    while (cap < 4 * max_units) cap <<= 1;
    v->hash_cap = cap;
    TsdfDev& d = v->dev;
    d.hash_mask = (int)(cap - 1);
    d.max_units = (int)max_units;
    auto cleanup = [&](hipError_t e) {
        set_error(std::string("[ScalableTSDFVolume] allocation failed: ") + hipGetErrorString(e));
        ot_tsdf_destroy(v);
        return OT_ERR_HIP;
    };
    hipError_t e;
    if ((e = hipMalloc(&d.hkeys, sizeof(unsigned long long) * cap)) != hipSuccess) return cleanup(e);
    if ((e = hipMalloc(&d.hvals, sizeof(int) * cap)) != hipSuccess) return cleanup(e);
    if ((e = hipMalloc(&d.counters, sizeof(int) * N_COUNTERS)) != hipSuccess) return cleanup(e);
    if ((e = hipMalloc(&d.stats, sizeof(unsigned long long) * N_STATS)) != hipSuccess) return cleanup(e);
    if ((e = hipMalloc(&d.unit_keys, sizeof(int) * 3 * max_units)) != hipSuccess) return cleanup(e);
    // RGB8 volumes keep colour at Open3D's precision (float64, 128-KiB records) unless set_color_precision(32)
    v->color64 = color_type == OT_COLOR_RGB8;
    d.color64 = v->color64 ? 1 : 0;
    d.unit_floats = v->color64 ? UNIT_FLOATS_C64 : UNIT_FLOATS;
    if ((e = hipMalloc(&d.vox, sizeof(float) * (size_t)d.unit_floats * max_units)) != hipSuccess) return cleanup(e);
    if ((e = hipMalloc(&v->sorted_ids, sizeof(unsigned) * max_units)) != hipSuccess) return cleanup(e);
    if ((e = hipMalloc(&d.fmask, fmask_bytes(cap))) != hipSuccess) return cleanup(e);
    if ((e = hipMalloc(&d.bslots, sizeof(int) * cap)) != hipSuccess) return cleanup(e);
    if ((e = hipMalloc(&d.work, sizeof(UnitWork) * cap)) != hipSuccess) return cleanup(e);
    if ((e = hipMalloc(&v->bset[0].bframes, sizeof(BatchFrame) * MAX_BATCH)) != hipSuccess) return cleanup(e);
    // coherent: k_copy_frames reads the staging straight from host memory, and non-coherent host memory may be cached
    // by the GPU (the halves are rewritten every other batch)
    if ((e = hipHostMalloc(&v->hbframes, sizeof(BatchFrame) * MAX_BATCH * 2, hipHostMallocCoherent)) != hipSuccess)
        return cleanup(e);
    if ((e = hipHostMalloc(&v->hmail, sizeof(unsigned) * 2 * OT_MAIL_WORDS, hipHostMallocCoherent)) != hipSuccess)
        return cleanup(e);
    std::memset(v->hmail, 0, sizeof(unsigned) * 2 * OT_MAIL_WORDS);  // sequence words start below every seq sent (>= 1)
    ot_status st = ot_tsdf_reset(v);
    if (st != OT_OK) {
        ot_tsdf_destroy(v);
        return st;
    }
    *out = v;
    return OT_OK;
}

ot_status ot_tsdf_destroy(ot_tsdf* v) {
    if (!v) return OT_OK;
    (void)hipDeviceSynchronize();
    TsdfDev& d = v->dev;
    ot_tsdf_set_profiling(v, 0);
    void* ptrs[] = {d.hkeys, d.hvals, d.counters, d.stats, d.unit_keys, d.vox, v->mult, v->sorted_ids, v->mesh.ws,
                    v->mesh.v, v->mesh.c, v->mesh.t, v->mesh.vk, v->mesh.tk, v->mesh.vown, d.fmask, d.bslots, d.work,
                    v->cloud.ws, v->wcount, v->bset[0].bframes, v->bset[0].bdc, v->bset[1].bframes, v->bset[1].bdc,
                    v->bset[1].work, v->tmask, v->bset[0].tmax, v->bset[1].tmax};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (v->hbframes) (void)hipHostFree(v->hbframes);
    if (v->hmail) (void)hipHostFree(v->hmail);
    if (v->ev_fork) (void)hipEventDestroy(v->ev_fork);
    if (v->ev_join) (void)hipEventDestroy(v->ev_join);
    if (v->ev_normals) (void)hipEventDestroy(v->ev_normals);
    if (v->ev_made) (void)hipEventDestroy(v->ev_made);
    if (v->ev_dfr) (void)hipEventDestroy(v->ev_dfr);
    if (v->side) (void)hipStreamDestroy(v->side);
    if (v->istream) (void)hipStreamDestroy(v->istream);
    for (auto& b : v->bset) {
        if (b.ev_units) (void)hipEventDestroy(b.ev_units);
        if (b.ev_done) (void)hipEventDestroy(b.ev_done);
    }
    delete v;
    return OT_OK;
}

ot_status ot_tsdf_reset(ot_tsdf* v) {
    if (!v) return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume::Reset] volume is NULL");
    TsdfDev& d = v->dev;
    OT_HIP_TRY(hipDeviceSynchronize());  // queued work on the volume (deferred normals included) first
    v->normals_pending = false;
    v->last_set = -1;
    OT_HIP_TRY(hipMemset(d.hkeys, 0xFF, sizeof(unsigned long long) * v->hash_cap));
    OT_HIP_TRY(hipMemset(d.hvals, 0xFF, sizeof(int) * v->hash_cap));
    OT_HIP_TRY(hipMemset(d.fmask, 0, fmask_bytes(v->hash_cap)));
    OT_HIP_TRY(hipMemset(d.counters, 0, sizeof(int) * N_COUNTERS));
    OT_HIP_TRY(hipMemset(d.stats, 0, sizeof(unsigned long long) * N_STATS));
    OT_HIP_TRY(hipDeviceSynchronize());
    v->pending.clear();
    v->dfr_on = false;  // a deferred batch's integrate belongs to the old contents (its work list is stale now)
    reset_host_state(v);
    return OT_OK;
}

ot_status ot_tsdf_reset_async(ot_tsdf* v, void* stream_) {
    if (!v) return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume::Reset] volume is NULL");
    hipStream_t stream = S(stream_);
    ot_status st = tsdf_flush(v, stream);  // queued frames belong to the old contents: apply, then clear
    if (st != OT_OK) return st;
    st = wait_normals(v, stream);  // the last mesh's deferred normals may still read the volume
    if (st != OT_OK) return st;
    // the hash table, frame masks, counters and statistics in one launch (six fill commands cost ~5 us of host time
    // each, on one object's critical path)
    const unsigned blocks = (unsigned)std::min<int64_t>((v->hash_cap + 255) / 256, 2048);
    hipLaunchKernelGGL(k_tsdf_clear, dim3(blocks), dim3(256), 0, stream, v->dev, (int64_t)v->hash_cap);
    OT_LAUNCH_CHECK();
    reset_host_state(v);  // (the flush above left no queued frame and no deferred batch)
    return OT_OK;
}

ot_status ot_tsdf_pending_frames(const ot_tsdf* vol, int32_t* n_host) {
    if (!vol || !n_host) return fail(OT_ERR_INVALID_ARGUMENT, "invalid arguments");
    *n_host = (int32_t)vol->pending.size();
    return OT_OK;
}

ot_status ot_tsdf_set_batch(ot_tsdf* vol, int32_t max_frames) {
    if (!vol || max_frames < 1) return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume] batch must be >= 1");
    vol->batch_max = max_frames;
    return OT_OK;
}

ot_status ot_tsdf_set_frontend_overlap(ot_tsdf* vol, int32_t mode) {
    if (!vol || mode < -1 || mode > 1)
        return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume] front-end overlap mode must be -1, 0 or 1");
    // the mode changes only on a drained volume: queued frames would be staged on whichever stream this call named,
    // not the one their producers ran on -- flush or read the volume on the frames' stream first
    if (!vol->pending.empty())
        return fail(OT_ERR_INVALID_ARGUMENT,
                    "[ScalableTSDFVolume] front-end overlap can change only with no queued frames (flush first)");
    if (vol->istream) OT_HIP_TRY(hipStreamSynchronize(vol->istream));  // a running integrate of the old mode
    vol->last_set = -1;
    vol->overlap_mode = mode;
    return OT_OK;
}

ot_status ot_tsdf_num_units(ot_tsdf* vol, int64_t* n, void* stream_) {
    if (!vol || !n) return fail(OT_ERR_INVALID_ARGUMENT, "invalid arguments");
    hipStream_t stream = S(stream_);
    ot_status st = tsdf_flush(vol, stream);  // queued frames, on the caller's stream
    if (st != OT_OK) return st;
    if (vol->dev.shard_world > 1) {  // a shard counts its own units (halo units are not exported)
        const unsigned* ids = nullptr;
        return export_list(vol, stream, &ids, n);
    }
    int nu = 0;
    OT_HIP_TRY(hipMemcpyAsync(&nu, vol->dev.counters + C_UNITS, sizeof(int), hipMemcpyDeviceToHost, stream));
    OT_HIP_TRY(hipStreamSynchronize(stream));
    *n = std::min<int64_t>(nu, vol->max_units);
    return OT_OK;
}

ot_status ot_tsdf_batch_stats(ot_tsdf* vol, int64_t* batches, int64_t* unit_batches, int64_t* new_units) {
    if (!vol) return fail(OT_ERR_INVALID_ARGUMENT, "invalid arguments");
    if (batches) *batches = vol->stat_batches;  // batches run (frames still queued are not counted: flush first)
    if (unit_batches) *unit_batches = vol->stat_unit_batches;
    if (new_units) *new_units = vol->stat_fresh;
    return OT_OK;
}

ot_status ot_tsdf_counters(ot_tsdf* vol, int64_t* updates, int64_t* unit_integrations, void* stream_) {
    if (!vol) return fail(OT_ERR_INVALID_ARGUMENT, "invalid arguments");
    hipStream_t stream = S(stream_);
    ot_status st = tsdf_flush(vol, stream);
    if (st != OT_OK) return st;
    std::vector<unsigned long long> s(N_STATS);
    OT_HIP_TRY(hipMemcpyAsync(s.data(), vol->dev.stats, sizeof(unsigned long long) * N_STATS, hipMemcpyDeviceToHost,
                              stream));
    OT_HIP_TRY(hipStreamSynchronize(stream));
    for (int i = 0; i < S_DROP_LINES; ++i) s[S_UPDATES] += s[S_UPD_BASE + i * S_DROP_STRIDE];
    if (updates) *updates = (int64_t)s[S_UPDATES];
    if (unit_integrations) *unit_integrations = (int64_t)s[S_UNIT_INTEGRATIONS];
    return OT_OK;
}

ot_status ot_tsdf_set_color_precision(ot_tsdf* vol, int32_t bits) {
    if (!vol || (bits != 32 && bits != 64))
        return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume] colour precision must be 32 or 64 bits");
    int nu = 0;
    OT_HIP_TRY(hipMemcpy(&nu, vol->dev.counters + C_UNITS, sizeof(int), hipMemcpyDeviceToHost));
    if (nu != 0 || !vol->pending.empty())
        return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume] set the colour precision before the first integrate");
    // NoColor volumes keep no colour state: the float32 record (zero colour planes) whatever the precision
    const bool c64 = bits == 64 && vol->color_type == OT_COLOR_RGB8;
    if (c64 != vol->color64) {  // the record stride changes: reallocate the (still empty) pool
        const int uf = c64 ? UNIT_FLOATS_C64 : UNIT_FLOATS;
        OT_HIP_TRY(hipDeviceSynchronize());
        // the new pool first: if the allocation fails the volume keeps its old, consistent layout
        float* pool = nullptr;
        OT_HIP_TRY(hipMalloc(&pool, sizeof(float) * (size_t)uf * vol->max_units));
        (void)hipFree(vol->dev.vox);
        vol->dev.vox = pool;
        vol->dev.unit_floats = uf;
        vol->dev.color64 = c64 ? 1 : 0;
        vol->color64 = c64;
    }
    return OT_OK;
}

ot_status ot_tsdf_get_color_precision(const ot_tsdf* vol, int32_t* bits) {
    if (!vol || !bits) return fail(OT_ERR_INVALID_ARGUMENT, "invalid arguments");
    *bits = vol->color64 ? 64 : 32;
    return OT_OK;
}

ot_status ot_tsdf_set_profiling(ot_tsdf* vol, int32_t enable) {
    if (!vol) return fail(OT_ERR_INVALID_ARGUMENT, "invalid arguments");
    vol->profiling = enable != 0;
    vol->prof_ms = vol->prof_fe_ms = 0.0;
    vol->prof_launches = vol->prof_fe_batches = 0;
    for (auto* lst : {&vol->prof_events, &vol->prof_fe_events}) {
        for (auto& e : *lst) {
            (void)hipEventDestroy(e.first);
            (void)hipEventDestroy(e.second);
        }
        lst->clear();
    }
    return OT_OK;
}

// accumulate (and release) an event-pair list into (ms, count)
static ot_status drain_events(std::vector<std::pair<hipEvent_t, hipEvent_t>>& lst, double& ms_acc, int64_t& n_acc) {
    for (auto& e : lst) {
        OT_HIP_TRY(hipEventSynchronize(e.second));
        float ms = 0.0f;
        OT_HIP_TRY(hipEventElapsedTime(&ms, e.first, e.second));
        ms_acc += ms;
        n_acc += 1;
        (void)hipEventDestroy(e.first);
        (void)hipEventDestroy(e.second);
    }
    lst.clear();
    return OT_OK;
}

ot_status ot_tsdf_kernel_time(ot_tsdf* vol, double* total_ms, int64_t* launches) {
    if (!vol) return fail(OT_ERR_INVALID_ARGUMENT, "invalid arguments");
    ot_status st = tsdf_flush(vol, nullptr);
    if (st != OT_OK) return st;
    if ((st = drain_events(vol->prof_events, vol->prof_ms, vol->prof_launches)) != OT_OK) return st;
    if (total_ms) *total_ms = vol->prof_ms;
    if (launches) *launches = vol->prof_launches;
    return OT_OK;
}

ot_status ot_tsdf_frontend_time(ot_tsdf* vol, double* total_ms, int64_t* batches) {
    if (!vol) return fail(OT_ERR_INVALID_ARGUMENT, "invalid arguments");
    ot_status st = tsdf_flush(vol, nullptr);
    if (st != OT_OK) return st;
    if ((st = drain_events(vol->prof_fe_events, vol->prof_fe_ms, vol->prof_fe_batches)) != OT_OK) return st;
    if (total_ms) *total_ms = vol->prof_fe_ms;
    if (batches) *batches = vol->prof_fe_batches;
    return OT_OK;
}

// test / diagnostic hook (not part of the drop-in boundary): the volume's raw u64 stats[4] (0 voxel updates,
// 1 unit integrations, 2 wave-frames the slice pre-test dropped since reset; 3 unused)
ot_status otx_tsdf_stats(ot_tsdf* vol, uint64_t* out4) {
    if (!vol || !out4) return fail(OT_ERR_INVALID_ARGUMENT, "invalid arguments");
    ot_status st = tsdf_flush(vol, nullptr);
    if (st != OT_OK) return st;
    std::vector<unsigned long long> s(N_STATS);
    OT_HIP_TRY(hipMemcpy(s.data(), vol->dev.stats, sizeof(unsigned long long) * N_STATS, hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) out4[i] = s[i];
    for (int i = 0; i < S_DROP_LINES; ++i) {
        out4[S_PRETEST_DROPPED] += s[S_DROP_BASE + i * S_DROP_STRIDE];
        out4[S_UPDATES] += s[S_UPD_BASE + i * S_DROP_STRIDE];
    }
    return OT_OK;
}

// test hook: the integrate's slice granularity (-1 = by the batch's estimated unit count, 0 = 4 voxels per lane along z
// always, 1 = 2 always; >= 2: the deferred integrate takes the fine slices below that many units, a threshold sweep):
// A/B timing and the parity of both instantiations
ot_status otx_integrate_fine(int32_t mode) {
    g_tsdf_hooks.int_fine = mode < 0 ? -1 : (mode == 1 ? 1 : 0);
    g_tsdf_hooks.fine_units = mode >= 2 ? mode : -1;
    return OT_OK;
}

// test hook: waves per workgroup of the coarse integrate (-1 = the default rule of integrate_form; 1, 2 or 4 forced at
// every table size): A/B timing and the parity of the three forms
ot_status otx_integrate_workgroup(int32_t waves) {
    if (waves != -1 && waves != 1 && waves != 2 && waves != 4)
        return fail(OT_ERR_INVALID_ARGUMENT, "otx_integrate_workgroup: -1, 1, 2 or 4 waves");
    g_tsdf_hooks.int_wg = waves;
    return OT_OK;
}

// test hook: the batch touch's staging-only workgroups per frame group (-1 = two per touch tile, the default;
// 0 = every touch workgroup stages a share first): A/B timing and the parity of both forms
ot_status otx_touch_stage_blocks(int32_t blocks) {
    if (blocks > 4096) return fail(OT_ERR_INVALID_ARGUMENT, "otx_touch_stage_blocks: at most 4096");
    g_tsdf_hooks.stage_blocks = blocks < 0 ? -1 : blocks;
    return OT_OK;
}

// test hook: frames per touch workgroup (1..64, default TF): A/B timing and the parity of other groupings.  A group never
// crosses a mask word (tsdf_touch.h touch_group_frames), whatever the count
ot_status otx_touch_frames(int32_t tf) {
    if (tf < 1 || tf > WORD_FRAMES) return fail(OT_ERR_INVALID_ARGUMENT, "otx_touch_frames: 1..64");
    g_tsdf_hooks.touch_tf = tf;
    return OT_OK;
}

// test hook: 1 = sort units with the radix sort at every key width (the rank sort's parity test), 0 = default
ot_status otx_unit_sort_radix(int32_t on) {
    g_tsdf_hooks.unit_sort_radix = on != 0;
    return OT_OK;
}

ot_status ot_tsdf_set_shard(ot_tsdf* vol, int32_t rank, int32_t world) {
    if (!vol || world < 1 || rank < 0 || rank >= world)
        return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume] shard needs 0 <= rank < world");
    int nu = 0;
    OT_HIP_TRY(hipMemcpy(&nu, vol->dev.counters + C_UNITS, sizeof(int), hipMemcpyDeviceToHost));
    if (nu != 0 || !vol->pending.empty())
        return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume] set the shard before the first integrate");
    vol->dev.shard_rank = rank;
    vol->dev.shard_world = world;
    vol->dev.shard_mode = SHARD_BLOCKS;
    // ownership blocks: 4^3 units up to 4 ranks, 2^3 beyond (configs[1] scan, 5 mm: largest shard / mean 1.09 / 1.13 /
    // 1.09 at 2 / 4 / 8 ranks; border rows sent 0.42 / 0.25 / 0.24 of an all-gather's)
    vol->dev.shard_shift = world <= 4 ? 2 : 1;
    return OT_OK;
}

ot_status ot_tsdf_set_shard_sector(ot_tsdf* vol, int32_t rank, int32_t world, double cx, double cy) {
    if (!vol || world < 1 || rank < 0 || rank >= world || !std::isfinite(cx) || !std::isfinite(cy))
        return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume] shard needs 0 <= rank < world and a finite centre");
    const double hx = std::nearbyint(2.0 * cx / vol->unit_length), hy = std::nearbyint(2.0 * cy / vol->unit_length);
    if (std::fabs(hx) > (double)(1 << 22) || std::fabs(hy) > (double)(1 << 22))
        return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume] sector centre out of the unit key range");
    ot_status st = ot_tsdf_set_shard(vol, rank, world);
    if (st != OT_OK) return st;
    vol->dev.shard_mode = SHARD_SECTORS;
    vol->dev.shard_cx2 = (int)hx;
    vol->dev.shard_cy2 = (int)hy;
    return OT_OK;
}

ot_status otx_integrate_depth(int32_t kt) {
    if (kt != -1 && (kt < 1 || kt > 3)) return fail(OT_ERR_INVALID_ARGUMENT, "integrate pipeline depth must be -1 or 1..3");
    g_tsdf_hooks.int_depth = kt;
    return OT_OK;
}

ot_status otx_defer_integrate(int32_t mode) {
    if (mode < -1 || mode > 1) return fail(OT_ERR_INVALID_ARGUMENT, "deferred integrate mode must be -1, 0 or 1");
    g_tsdf_hooks.defer = mode;
    return OT_OK;
}

// test hook: the coarse integrate's slice pre-test (-1 = whole volumes' batches staged in full, the default; 0 = never;
// 1 = every batch staged in full, a sharded volume's too): A/B timing and the parity of both forms
ot_status otx_slice_pretest(int32_t mode) {
    if (mode < -1 || mode > 1) return fail(OT_ERR_INVALID_ARGUMENT, "slice pre-test mode must be -1, 0 or 1");
    g_tsdf_hooks.pretest = mode;
    return OT_OK;
}

// test hook: the staging's one-pass form (-1 = the default: an eligible frame of a batch with tile-max maps is staged
// in tile order and its map reduced from the depths in registers; 0 = every frame by pixel chunks and the map from a
// second read of the raw depth): A/B timing and the parity of both forms
ot_status otx_stage_onepass(int32_t mode) {
    if (mode < -1 || mode > 0) return fail(OT_ERR_INVALID_ARGUMENT, "one-pass staging mode must be -1 or 0");
    g_tsdf_hooks.onepass = mode;
    return OT_OK;
}

// test / diagnostic hook: frame `frame` of the last batch's staging set as the staging left it -- its W x H 8-B records
// (float depth bits, colour word) to records_out and, unless map_out is null, the pre_tiles(W) x pre_tiles(H) words of
// its tile-max map (host memory both).  An error if that batch built no map and one is asked for.
ot_status otx_tsdf_staged(ot_tsdf* vol, int32_t frame, uint64_t* records_out, uint32_t* map_out) {
    if (!vol || !records_out) return fail(OT_ERR_INVALID_ARGUMENT, "invalid arguments");
    ot_status st = tsdf_flush(vol, nullptr);
    if (st != OT_OK) return st;
    if (vol->staged_set < 0 || frame < 0 || frame >= vol->staged_n)
        return fail(OT_ERR_INVALID_ARGUMENT, "otx_tsdf_staged: no such frame in the last batch");
    if (map_out && !vol->staged_map) return fail(OT_ERR_INVALID_ARGUMENT, "otx_tsdf_staged: the last batch built no map");
    OT_HIP_TRY(hipDeviceSynchronize());
    const auto& bs = vol->bset[vol->staged_set];
    const int64_t npx = (int64_t)vol->staged_w * vol->staged_h;
    OT_HIP_TRY(hipMemcpy(records_out, bs.bdc + npx * frame, sizeof(uint2) * npx, hipMemcpyDeviceToHost));
    if (map_out) {
        const int64_t tiles = (int64_t)pre_tiles(vol->staged_w) * pre_tiles(vol->staged_h);
        OT_HIP_TRY(hipMemcpy(map_out, bs.tmax + tiles * frame, sizeof(unsigned) * tiles, hipMemcpyDeviceToHost));
    }
    return OT_OK;
}

ot_status otx_split_frontend(int32_t mode) {
    if (mode < -1 || mode > 1) return fail(OT_ERR_INVALID_ARGUMENT, "split front end mode must be -1, 0 or 1");
    g_tsdf_hooks.split = mode;
    return OT_OK;
}

ot_status ot_tsdf_set_shard_block(ot_tsdf* vol, int32_t log2_units) {
    if (!vol || log2_units < 0 || log2_units > 8)
        return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume] shard block must be 2^0 .. 2^8 units per axis");
    int nu = 0;
    OT_HIP_TRY(hipMemcpy(&nu, vol->dev.counters + C_UNITS, sizeof(int), hipMemcpyDeviceToHost));
    if (nu != 0 || !vol->pending.empty())
        return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume] set the shard before the first integrate");
    vol->dev.shard_shift = log2_units;
    return OT_OK;
}

}  // extern "C"
