// tsdf_integrate.h — device text of the TSDF batch integrate: a (unit, slice) work item's voxels taken through the
// batch's frames (integrate_item) and the walk over a batch's work list (integrate_body).  One text behind
// k_batch_integrate (tsdf_integrate_kernel.h: its one-word forms in tsdf_integrate.hip, its two-word forms in
// tsdf_integrate_wide.hip) and the integrate half of k_integrate_touch / k_integrate_touch_fine (tsdf_fused.hip).
#pragma once

#include <type_traits>
#include <utility>

#include "tsdf_stage.h"

namespace ot {

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

}  // namespace ot
