// scan_cluster.hip — the object trigger between the scans and the ScanObject goal (DESIGN.md §4 "scan clustering").
//
//   ot_scan_cluster         : lidar_cluster_publisher.cpp:151-291 — gap-separated clusters of each scan, the 360°
//                             seam merge, WALL / OBJECT / UNKNOWN from length, linearity and point count, and the
//                             three published clouds.  One workgroup stages one scan in LDS; validity, the
//                             previous-valid link, break flags, cluster ids and the per-cluster reductions are wave64
//                             scans over LDS, combined across the scan's <= 64 chunks of 64 beams by one wave.
//   ot_object_map_filter    : object_filter.cpp:51-155 — object points closer than proximity_threshold to a wall
//                             point of the virtual scan are dropped; walls tiled through LDS.
//   ot_cluster_observations : 3_multi_object_goal_selector.cpp:172-215 — consecutive-gap clusters of a cloud and
//                             their (centre, width, height, lock radius) rows; the same segmented machinery.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <vector>

#include "compact.h"
#include "scan.h"

namespace ot {

constexpr int SC_THREADS = 256;
constexpr int SC_WAVES = SC_THREADS / 64;
constexpr int SC_MAX_CHUNKS = 64;                  // one wave combines the chunk aggregates
constexpr int SC_MAX_BEAMS = SC_MAX_CHUNKS * 64;   // == OT_SCAN_CLUSTER_MAX_BEAMS
constexpr int SC_MAX_BLOCKS = 512;                 // workgroups walk the scans grid-stride; bounds the cluster workspace
static_assert(SC_MAX_BEAMS == OT_SCAN_CLUSTER_MAX_BEAMS, "header and kernel disagree");

// rows 0, 1 of the rotation of a quaternion (tf2 Matrix3x3::setRotation) and the translation, host-computed
struct PoseM {
    double m00, m01, m10, m11, tx, ty;
};

// per raw cluster (before the min-points filter and the seam merge), in a per-workgroup global workspace
struct Raw {
    int start, last;  // first and last valid beam
    int cls, n;
    float mnx, mxx, mny, mxy;
    double sx, sy;         // sums of the points (widened to double)
    double mx, my;         // mean of the final cluster this one belongs to
    double cxx, cxy, cyy;  // centred sums about (mx, my)
};

template <typename T>
__device__ inline T shfl_up_t(const T& v, int o) {
    static_assert(sizeof(T) % 4 == 0, "word-wise shuffle");
    int w[sizeof(T) / 4];
    __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
    for (int k = 0; k < (int)(sizeof(T) / 4); ++k) w[k] = __shfl_up(w[k], o, 64);
    T r;
    __builtin_memcpy(&r, w, sizeof(T));
    return r;
}

template <typename T, class Op>
__device__ inline T wave_scan_incl(T v, Op op) {
    const int lane = (int)lane_id();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = shfl_up_t(v, o);
        if (lane >= o) v = op(u, v);
    }
    return v;
}

// In-place inclusive scan of a[0 .. n) (LDS, n <= SC_MAX_BEAMS) by the whole workgroup: each wave scans chunks of 64,
// wave 0 scans the chunk totals (agg: LDS, SC_MAX_CHUNKS entries), every element takes its chunk's carry.  Ends in a
// barrier; the caller's writes to `a` must be followed by one.
template <typename T, class Op>
__device__ inline void block_scan(T* a, int n, Op op, T identity, T* agg) {
    const int lane = (int)lane_id(), wid = threadIdx.x >> 6;
    const int nch = (n + 63) >> 6;
    for (int c = wid; c < nch; c += SC_WAVES) {
        const int i = c * 64 + lane;
        T v = i < n ? a[i] : identity;
        v = wave_scan_incl(v, op);
        if (i < n) a[i] = v;
        if (lane == 63) agg[c] = v;
    }
    __syncthreads();
    if (wid == 0) {
        T v = lane < nch ? agg[lane] : identity;
        v = wave_scan_incl(v, op);
        T e = shfl_up_t(v, 1);
        if (lane == 0) e = identity;
        agg[lane] = e;  // exclusive: the carry into chunk `lane`
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += SC_THREADS) a[i] = op(agg[i >> 6], a[i]);
    __syncthreads();
}

struct OpMax {
    __device__ int operator()(int a, int b) const { return a > b ? a : b; }
};
template <typename T>
struct OpAdd {
    __device__ T operator()(T a, T b) const { return a + b; }
};

// ---- segmented reductions over runs of equal keys (keys non-decreasing along the beams)
// first pass: count, bounding box (initial values as the node's 1e6 / -1e6) and the double sums
struct P1 {
    int key, n;
    float mnx, mxx, mny, mxy;
    double sx, sy;
    __device__ static P1 identity() { return P1{-2, 0, 1e6f, -1e6f, 1e6f, -1e6f, 0.0, 0.0}; }
    __device__ static P1 point(float x, float y, double sx, double sy) {  // min(1e6, x), max(-1e6, x) as :116-122
        return P1{0, 1, x < 1e6f ? x : 1e6f, x > -1e6f ? x : -1e6f, y < 1e6f ? y : 1e6f, y > -1e6f ? y : -1e6f, sx, sy};
    }
    __device__ void absorb(const P1& l) {  // this = l (earlier beams) combined with this
        n += l.n;
        mnx = l.mnx < mnx ? l.mnx : mnx;
        mxx = l.mxx > mxx ? l.mxx : mxx;
        mny = l.mny < mny ? l.mny : mny;
        mxy = l.mxy > mxy ? l.mxy : mxy;
        sx = l.sx + sx;
        sy = l.sy + sy;
    }
};
// second pass: centred sums
struct P2 {
    int key, pad;
    double cxx, cxy, cyy;
    __device__ static P2 identity() { return P2{-2, 0, 0.0, 0.0, 0.0}; }
    __device__ void absorb(const P2& l) {
        cxx = l.cxx + cxx;
        cxy = l.cxy + cxy;
        cyy = l.cyy + cyy;
    }
};

template <class V>
struct OpSeg {
    __device__ V operator()(const V& l, V r) const {
        if (l.key == r.key) r.absorb(l);
        return r;
    }
};

// Reduce V over every run of equal key = cid[i] - 1 (cid: LDS, the inclusive count of cluster starts, so a run is a
// cluster's beams plus the invalid beams after them, which load the identity).  load(i, key) gives beam i's value,
// store(c, v) / fetch(c) keep cluster c's value.  Level 1: wave-segmented scan per chunk of 64, the run's last beam
// stores its within-chunk value; level 2: wave 0 scans the chunks' trailing runs; level 3: a cluster whose run began
// in an earlier chunk takes the carry of the chunk before its tail.  run_start(c) / run_tail(c): first / last beam of
// run c.  Ends in a barrier.
template <class V, class Load, class Store, class Fetch, class RunStart, class RunTail>
__device__ inline void seg_reduce(int n, int n_runs, const int* cid, V* chunk, Load load, Store store, Fetch fetch,
                                  RunStart run_start, RunTail run_tail) {
    const int lane = (int)lane_id(), wid = threadIdx.x >> 6;
    const int nch = (n + 63) >> 6;
    OpSeg<V> op;
    for (int c = wid; c < nch; c += SC_WAVES) {
        const int i = c * 64 + lane;
        V v = V::identity();
        if (i < n) {
            const int key = cid[i] - 1;
            v = load(i, key);
            v.key = key;
        }
        v = wave_scan_incl(v, op);
        const int next = i + 1 < n ? cid[i + 1] - 1 : -2;
        if (i < n && v.key >= 0 && next != v.key) store(v.key, v);
        if (i < n && (lane == 63 || i == n - 1)) chunk[c] = v;
    }
    __syncthreads();
    if (wid == 0) {
        V v = lane < nch ? chunk[lane] : V::identity();
        v = wave_scan_incl(v, op);
        if (lane < nch) chunk[lane] = v;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < n_runs; c += SC_THREADS) {
        const int ch = run_tail(c) >> 6;
        if (ch > 0 && run_start(c) < ch * 64) {  // chunk ch - 1 ends inside run c
            V v = fetch(c);
            v.key = c;
            v = op(chunk[ch - 1], v);
            store(c, v);
        }
    }
    __syncthreads();
}

struct ScBlock {
    int F, L, second, merge;
};

// the node's size_t comparisons of a point count with an int parameter
__device__ inline bool count_ge(int n, int p) { return (unsigned long long)n >= (unsigned long long)(long long)p; }
__device__ inline bool count_gt(int n, int p) { return (unsigned long long)n > (unsigned long long)(long long)p; }

extern __shared__ double s_scan_dyn[];  // X[n] Y[n] (float) A[n] B[n] (int); 8-byte aligned for the overlay P

constexpr unsigned long long CLS_MASK = (1ull << 21) - 1ull;

__global__ __launch_bounds__(SC_THREADS) void k_scan_cluster(
    const float* __restrict__ ranges, int n_scans, int N, const float2* __restrict__ cs, float r_use,
    ot_scan_cluster_params prm, const PoseM* __restrict__ poses, Raw* ws, int32_t* beam_cluster, uint8_t* beam_class,
    float* beam_xy_out, int32_t* n_clusters, ot_scan_cluster_row* rows, int32_t* beam_pos, int32_t* counts) {
    float* X = (float*)s_scan_dyn;
    float* Y = X + N;
    int* A = (int*)(Y + N);
    int* B = A + N;
    unsigned long long* P = (unsigned long long*)X;  // overlays X, Y once they are written out
    __shared__ int aggI[SC_MAX_CHUNKS];
    __shared__ unsigned long long aggU[SC_MAX_CHUNKS];
    __shared__ P1 chunk1[SC_MAX_CHUNKS];
    __shared__ P2 chunk2[SC_MAX_CHUNKS];
    __shared__ ScBlock sb;
    Raw* raw = ws + (size_t)blockIdx.x * N;
    const int tid = threadIdx.x;

    for (int s = blockIdx.x; s < n_scans; s += gridDim.x) {
        const float* R = ranges + (int64_t)s * N;
        const int64_t o = (int64_t)s * N;
        // --- 1. validity (:162-163), sensor-frame points (:165-167), the last valid beam up to each beam
        for (int i = tid; i < N; i += SC_THREADS) {
            const float r = R[i];
            const bool ok = !(isnan(r) || isinf(r)) && !(r > r_use);
            float x = NAN, y = NAN;
            if (ok) beam_xy(r, cs, i, x, y);
            X[i] = x;
            Y[i] = y;
            A[i] = ok ? i : -1;
        }
        __syncthreads();
        block_scan(A, N, OpMax(), -1, aggI);
        // --- 2. cluster starts: the first valid beam, and a gap to the previous valid beam (:169-179)
        for (int i = tid; i < N; i += SC_THREADS) {
            int f = 0;
            if (A[i] == i) {
                const int pv = i > 0 ? A[i - 1] : -1;
                f = pv < 0 || hypot_f(X[i] - X[pv], Y[i] - Y[pv]) > prm.gap_threshold;
            }
            B[i] = f;
        }
        __syncthreads();
        block_scan(B, N, OpAdd<int>(), 0, aggI);
        const int n_raw = B[N - 1];
        // --- 3. first / last beam of every raw cluster
        for (int i = tid; i < N; i += SC_THREADS) {
            const int bi = B[i], bp = i > 0 ? B[i - 1] : 0;
            if (bi != bp) {  // only a valid beam starts a cluster
                raw[bi - 1].start = i;
                if (bi > 1) raw[bi - 2].last = A[i - 1];
            }
        }
        if (tid == 0 && n_raw > 0) raw[n_raw - 1].last = A[N - 1];
        __syncthreads();
        auto run_start = [&](int c) { return raw[c].start; };
        auto run_tail = [&](int c) { return c == n_raw - 1 ? N - 1 : raw[c + 1].start - 1; };
        // --- 4. count, bounding box, sums per raw cluster
        seg_reduce<P1>(
            N, n_raw, B, chunk1,
            [&](int i, int) {
                const float x = X[i], y = Y[i];
                return isnan(x) ? P1::identity() : P1::point(x, y, (double)x, (double)y);
            },
            [&](int c, const P1& v) {
                Raw& q = raw[c];
                q.n = v.n;
                q.mnx = v.mnx, q.mxx = v.mxx, q.mny = v.mny, q.mxy = v.mxy;
                q.sx = v.sx, q.sy = v.sy;
            },
            [&](int c) {
                const Raw& q = raw[c];
                return P1{c, q.n, q.mnx, q.mxx, q.mny, q.mxy, q.sx, q.sy};
            },
            run_start, run_tail);
        // --- 5. min_cluster_points (:175, :182), then the seam merge (:186-199)
        for (int c = tid; c < n_raw; c += SC_THREADS) A[c] = count_ge(raw[c].n, prm.min_cluster_points) ? 1 : 0;
        __syncthreads();
        block_scan(A, n_raw, OpAdd<int>(), 0, aggI);
        const int K = n_raw > 0 ? A[n_raw - 1] : 0;
        for (int c = tid; c < n_raw; c += SC_THREADS)
            if (count_ge(raw[c].n, prm.min_cluster_points)) {
                const int j = A[c] - 1;
                if (j == 0) sb.F = c;
                if (j == 1) sb.second = c;
                if (j == K - 1) sb.L = c;
            }
        __syncthreads();
        if (tid == 0) {
            int merge = 0;
            if (K >= 2) {  // K == 1: the ring cluster is kept once (the node's self-insert is undefined)
                const int a = raw[sb.L].last, b = raw[sb.F].start;
                merge = hypot_f(X[a] - X[b], Y[a] - Y[b]) < prm.gap_threshold;
            }
            sb.merge = merge;
        }
        __syncthreads();
        const int F = sb.F, L = sb.L, merge = sb.merge;
        const int n_final = K - merge;
        // final list index: the kept clusters in order, the merged one (last + first) at the end
        for (int c = tid; c < n_raw; c += SC_THREADS) {
            int fid = -1;
            if (count_ge(raw[c].n, prm.min_cluster_points)) {
                const int j = A[c] - 1;
                fid = merge ? (j == 0 ? K - 2 : j - 1) : j;
            }
            A[c] = fid;
            // --- 6. mean of the final cluster (the merged one: last cluster first)
            const bool mg = merge && (c == F || c == L);
            const int n = mg ? raw[L].n + raw[F].n : raw[c].n;
            const double sx = mg ? raw[L].sx + raw[F].sx : raw[c].sx;
            const double sy = mg ? raw[L].sy + raw[F].sy : raw[c].sy;
            raw[c].mx = sx / (double)n;
            raw[c].my = sy / (double)n;
        }
        __syncthreads();
        // --- 7. centred sums
        seg_reduce<P2>(
            N, n_raw, B, chunk2,
            [&](int i, int key) {
                const float x = X[i], y = Y[i];
                if (isnan(x)) return P2::identity();
                const double dx = (double)x - raw[key].mx, dy = (double)y - raw[key].my;
                return P2{0, 0, dx * dx, dx * dy, dy * dy};
            },
            [&](int c, const P2& v) {
                Raw& q = raw[c];
                q.cxx = v.cxx, q.cxy = v.cxy, q.cyy = v.cyy;
            },
            [&](int c) {
                const Raw& q = raw[c];
                return P2{c, 0, q.cxx, q.cxy, q.cyy};
            },
            run_start, run_tail);
        // --- 8. length, linearity, class (:238-256); the merged cluster is computed by both halves, written by the last
        for (int c = tid; c < n_raw; c += SC_THREADS) {
            const int fid = A[c];
            if (fid < 0) continue;
            const bool mg = merge && (c == F || c == L);
            const Raw& a = mg ? raw[L] : raw[c];
            int n = a.n;
            float mnx = a.mnx, mxx = a.mxx, mny = a.mny, mxy = a.mxy;
            double cxx = a.cxx, cxy = a.cxy, cyy = a.cyy;
            if (mg) {
                const Raw& b = raw[F];
                n += b.n;
                mnx = b.mnx < mnx ? b.mnx : mnx;
                mxx = b.mxx > mxx ? b.mxx : mxx;
                mny = b.mny < mny ? b.mny : mny;
                mxy = b.mxy > mxy ? b.mxy : mxy;
                cxx += b.cxx, cxy += b.cxy, cyy += b.cyy;
            }
            const float dx = mxx - mnx, dy = mxy - mny;
            const float length = sqrtf(dx * dx + dy * dy);
            double lin = 0.0;
            if (n >= 3) {
                const double d = (double)(n - 1);
                const double va = cxx / d, vb = cxy / d, vc = cyy / d;
                const double half = (va + vc) / 2.0, hd = (va - vc) / 2.0;
                const double root = sqrt(hd * hd + vb * vb);
                const double l0 = half - root, l1 = half + root;
                if (!(l0 + l1 < 1e-6)) lin = l0 / (l1 + 1e-6);
            }
            int cls = OT_SCAN_CLASS_UNKNOWN;
            if (lin < (double)prm.wal_lin_max && length > prm.wal_len_min && count_gt(n, prm.wal_nmp_min))
                cls = OT_SCAN_CLASS_WALL;
            else if (length < prm.obj_len_max && count_gt(n, prm.obj_nmp_min))
                cls = OT_SCAN_CLASS_OBJECT;
            raw[c].cls = cls;
            if (!(mg && c == F)) {
                ot_scan_cluster_row row;
                row.first_beam = raw[c].start;
                row.n_points = n;
                row.length = length;
                row.cls = cls;
                row.linearity = lin;
                rows[o + fid] = row;
            }
        }
        __syncthreads();
        // --- 9. per-beam outputs; map-frame points (:265-274)
        const PoseM T = poses[s];
        for (int i = tid; i < N; i += SC_THREADS) {
            const float x = X[i], y = Y[i];
            const bool ok = !isnan(x);
            const int c = B[i] - 1;
            const int fid = ok ? A[c] : -1;
            beam_cluster[o + i] = fid;
            beam_class[o + i] = (uint8_t)(fid >= 0 ? raw[c].cls : 0);
            float px = NAN, py = NAN;
            if (ok) {
                px = (float)(((double)x * T.m00 + (double)y * T.m01) + T.tx);
                py = (float)(((double)x * T.m10 + (double)y * T.m11) + T.ty);
            }
            beam_xy_out[(o + i) * 2 + 0] = px;
            beam_xy_out[(o + i) * 2 + 1] = py;
        }
        __syncthreads();
        // --- 10. position of every beam in its class's cloud: one stable compaction in beam order rotated to start
        // just after the seam cluster; the three class counters ride one 64-bit scan, 21 bits each
        for (int i = tid; i < N; i += SC_THREADS) {
            const int cls = beam_class[o + i];  // this thread's own store
            P[i] = cls ? 1ull << (21 * (cls - 1)) : 0ull;
        }
        __syncthreads();
        block_scan(P, N, OpAdd<unsigned long long>(), 0ull, aggU);
        const unsigned long long tot = P[N - 1];
        const int b0 = merge ? raw[sb.second].start : 0;
        const unsigned long long e0 = b0 > 0 ? P[b0 - 1] : 0ull;
        for (int i = tid; i < N; i += SC_THREADS) {
            const int cls = beam_class[o + i];
            int pos = -1;
            if (cls) {
                const int sh = 21 * (cls - 1);
                const int e = (int)((P[i] >> sh) & CLS_MASK) - 1, z = (int)((e0 >> sh) & CLS_MASK),
                          t = (int)((tot >> sh) & CLS_MASK);
                pos = i >= b0 ? e - z : (t - z) + e;
            }
            beam_pos[o + i] = pos;
        }
        if (tid < 3) counts[s * 3 + tid] = (int)((tot >> (21 * tid)) & CLS_MASK);
        if (tid == 0) n_clusters[s] = n_final;
        __syncthreads();  // X / Y / A / B and the workspace are rewritten by the next scan
    }
}

// the three clouds, concatenated over scans: beam (s, i) of class k goes to row off[k][s] + its position
__global__ __launch_bounds__(256) void k_scan_cluster_emit(int n_scans, int N, const uint8_t* __restrict__ beam_class,
                                                           const float* __restrict__ bxy,
                                                           const int32_t* __restrict__ beam_pos,
                                                           const int64_t* __restrict__ off, float* wall, float* object,
                                                           float* unknown) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)n_scans * N) return;
    const int cls = beam_class[t];
    if (!cls) return;
    const int s = (int)(t / N);
    float* out = cls == OT_SCAN_CLASS_WALL ? wall : cls == OT_SCAN_CLASS_OBJECT ? object : unknown;
    const int64_t row = off[(int64_t)(cls - 1) * (n_scans + 1) + s] + beam_pos[t];
    out[row * 3 + 0] = bxy[t * 2 + 0];
    out[row * 3 + 1] = bxy[t * 2 + 1];
    out[row * 3 + 2] = 0.0f;
}

// ------------------------------------------------------------------------------------------- object map filter
__global__ __launch_bounds__(256) void k_object_filter(const float* __restrict__ obj, const int64_t* __restrict__ off,
                                                       const float* __restrict__ virt, int N,
                                                       const float2* __restrict__ cs, float r_max,
                                                       const ScanPose* __restrict__ poses, double prox2,
                                                       uint8_t* __restrict__ mask, int32_t* kept) {
    __shared__ double WX[256], WY[256];
    const int s = blockIdx.x;
    const int64_t base = off[s], n = off[s + 1] - base;
    const int64_t p = (int64_t)blockIdx.y * 256 + threadIdx.x;
    if ((int64_t)blockIdx.y * 256 >= n) return;  // the whole workgroup
    const bool have = p < n;
    float ox = 0.0f, oy = 0.0f;
    if (have) {
        ox = obj[(base + p) * 3 + 0];
        oy = obj[(base + p) * 3 + 1];
    }
    const ScanPose T = poses[s];
    const float* V = virt + (int64_t)s * N;
    bool near = false;
    int any_wall = 0;
    for (int j0 = 0; j0 < N; j0 += 256) {
        const int j = j0 + (int)threadIdx.x;
        double wx = NAN, wy = NAN;  // no wall point: every comparison below is false
        int ok = 0;
        if (j < N) {
            const float r = V[j];
            if (!(isinf(r) || isnan(r) || r > r_max)) {
                float lx, ly;
                beam_xy(r, cs, j, lx, ly);
                wx = T.tx + ((double)lx * T.cyaw - (double)ly * T.syaw);
                wy = T.ty + ((double)lx * T.syaw + (double)ly * T.cyaw);
                ok = 1;
            }
        }
        WX[threadIdx.x] = wx;
        WY[threadIdx.x] = wy;
        any_wall |= __syncthreads_or(ok);
        if (have && !near) {
            const int m = min(256, N - j0);
            for (int k = 0; k < m; ++k) {
                const float dx = (float)((double)ox - WX[k]);
                const float dy = (float)((double)oy - WY[k]);
                if ((double)(dx * dx + dy * dy) < prox2) {
                    near = true;
                    break;
                }
            }
        }
        __syncthreads();
    }
    const bool keep = have && any_wall && !near;
    if (have) mask[base + p] = keep ? 1 : 0;
    const unsigned long long m = __ballot(keep);
    if (lane_id() == 0 && m) atomicAdd(&kept[s], __popcll(m));
}

struct MaskPred {
    const uint8_t* m;
    __device__ bool operator()(int64_t i) const { return m[i] != 0; }
};
struct Row3Emit {
    const float* in;
    float* out;
    __device__ void operator()(int64_t i, int64_t pos) const {
        out[pos * 3 + 0] = in[i * 3 + 0];
        out[pos * 3 + 1] = in[i * 3 + 1];
        out[pos * 3 + 2] = in[i * 3 + 2];
    }
};

// ------------------------------------------------------------------------------------------- goal observations
__global__ __launch_bounds__(SC_THREADS) void k_cluster_obs(const float* __restrict__ pts, int stride,
                                                            const int64_t* __restrict__ off, int n_clouds, int cap,
                                                            ot_observation_params prm,
                                                            const PoseM* __restrict__ poses, Raw* ws, float* out_rows,
                                                            int32_t* n_obs) {
    float* X = (float*)s_scan_dyn;
    float* Y = X + cap;
    int* A = (int*)(Y + cap);
    int* B = A + cap;
    __shared__ int aggI[SC_MAX_CHUNKS];
    __shared__ P1 chunk1[SC_MAX_CHUNKS];
    Raw* raw = ws + (size_t)blockIdx.x * cap;
    const int tid = threadIdx.x;

    for (int j = blockIdx.x; j < n_clouds; j += gridDim.x) {
        const int64_t base = off[j];
        const int N = (int)(off[j + 1] - base);
        if (N == 0) {  // :176
            if (tid == 0) n_obs[j] = 0;
            continue;
        }
        for (int i = tid; i < N; i += SC_THREADS) {
            X[i] = pts[(base + i) * stride + 0];
            Y[i] = pts[(base + i) * stride + 1];
        }
        __syncthreads();
        // :181-189: a break where consecutive points are further apart than the threshold
        for (int i = tid; i < N; i += SC_THREADS) {
            int f = 1;
            if (i > 0) {
                const float dx = X[i] - X[i - 1], dy = Y[i] - Y[i - 1];
                f = (double)sqrtf(dx * dx + dy * dy) > prm.cluster_distance_threshold;
            }
            B[i] = f;
        }
        __syncthreads();
        block_scan(B, N, OpAdd<int>(), 0, aggI);
        const int n_raw = B[N - 1];
        for (int i = tid; i < N; i += SC_THREADS)
            if (B[i] != (i > 0 ? B[i - 1] : 0)) raw[B[i] - 1].start = i;
        __syncthreads();
        seg_reduce<P1>(
            N, n_raw, B, chunk1,
            [&](int i, int) {
                return P1::point(X[i], Y[i], 0.0, 0.0);
            },
            [&](int c, const P1& v) {
                Raw& q = raw[c];
                q.n = v.n;
                q.mnx = v.mnx, q.mxx = v.mxx, q.mny = v.mny, q.mxy = v.mxy;
            },
            [&](int c) {
                const Raw& q = raw[c];
                return P1{c, q.n, q.mnx, q.mxx, q.mny, q.mxy, 0.0, 0.0};
            },
            [&](int c) { return raw[c].start; }, [&](int c) { return c == n_raw - 1 ? N - 1 : raw[c + 1].start - 1; });
        // :185 / :190 min_cluster_points, :199-200 wall thickness
        auto emits = [&](int c, float& w, float& h) {
            const Raw& q = raw[c];
            w = q.mxx - q.mnx;
            h = q.mxy - q.mny;
            const float thin = h < w ? h : w;
            return count_ge(q.n, prm.min_cluster_points) && !((double)thin < prm.wall_thickness_threshold);
        };
        for (int c = tid; c < n_raw; c += SC_THREADS) {
            float w, h;
            A[c] = emits(c, w, h) ? 1 : 0;
        }
        __syncthreads();
        block_scan(A, n_raw, OpAdd<int>(), 0, aggI);
        const PoseM T = poses[j];
        for (int c = tid; c < n_raw; c += SC_THREADS) {
            float w, h;
            if (!emits(c, w, h)) continue;
            const Raw& q = raw[c];
            const float lcx = (q.mnx + q.mxx) / 2.0f, lcy = (q.mny + q.mxy) / 2.0f;  // :202-203
            const float diagonal = sqrtf(w * w + h * h);                             // :135
            float* row = out_rows + (base + (A[c] - 1)) * 5;
            row[0] = (float)(((double)lcx * T.m00 + (double)lcy * T.m01) + T.tx);
            row[1] = (float)(((double)lcx * T.m10 + (double)lcy * T.m11) + T.ty);
            row[2] = w;
            row[3] = h;
            row[4] = (float)((double)(diagonal / 2.0f) + prm.lock_margin);  // :136
        }
        if (tid == 0) n_obs[j] = A[n_raw - 1];
        __syncthreads();
    }
}

// rows 0 / 1 of tf2's Matrix3x3::setRotation(q) and the translation; NULL poses = identity
static void pose_rows(const double* poses_host, int n, std::vector<PoseM>& out) {
    out.resize((size_t)std::max(n, 1));
    for (int b = 0; b < n; ++b) {
        if (!poses_host) {
            out[b] = PoseM{1.0, 0.0, 0.0, 1.0, 0.0, 0.0};
            continue;
        }
        const double* p = poses_host + (size_t)b * 7;  // tx ty tz qx qy qz qw
        const double x = p[3], y = p[4], z = p[5], w = p[6];
        const double d = ((x * x + y * y) + z * z) + w * w;
        const double s = 2.0 / d;
        const double xs = x * s, ys = y * s, zs = z * s;
        const double wz = w * zs, xx = x * xs, xy = x * ys, yy = y * ys, zz = z * zs;
        out[b] = PoseM{1.0 - (yy + zz), xy - wz, xy + wz, 1.0 - (xx + zz), p[0], p[1]};
    }
}

static ot_status set_dynamic_lds(const void* kernel, size_t bytes, std::atomic<bool>& done) {
    // static + dynamic LDS may pass 64 KiB: the kernel must opt in (once per process)
    if (bytes > 48 * 1024 && !done.load()) {
        OT_HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)((size_t)SC_MAX_BEAMS * 16)));
        done.store(true);
    }
    return OT_OK;
}

}  // namespace ot

using namespace ot;


extern "C" {

ot_status ot_scan_cluster(const float* ranges, int32_t n_scans, int32_t n_beams, float angle_min,
                          float angle_increment, float range_max, const double* poses_host,
                          const ot_scan_cluster_params* params, int32_t* beam_cluster, uint8_t* beam_class,
                          float* beam_xy_out, int32_t* n_clusters, ot_scan_cluster_row* clusters, float* wall_xyz,
                          float* object_xyz, float* unknown_xyz, int64_t* cloud_offsets_host, void* stream_) {
    hipStream_t stream = S(stream_);
    if (n_scans < 0 || n_beams <= 0 || !params || !cloud_offsets_host)
        return fail(OT_ERR_INVALID_ARGUMENT, "[LidarClusterer] invalid arguments");
    // 0 would make the node push an empty cluster for a scan without valid beams; negative values keep nothing
    if (params->min_cluster_points < 1)
        return fail(OT_ERR_INVALID_ARGUMENT, "[LidarClusterer] min_cluster_points must be at least 1");
    if (n_beams > SC_MAX_BEAMS)
        return fail(OT_ERR_INVALID_ARGUMENT, "[LidarClusterer] n_beams " + std::to_string(n_beams) +
                                                 " exceeds the " + std::to_string(SC_MAX_BEAMS) +
                                                 " beams one workgroup stages");
    for (int64_t i = 0; i < 3 * ((int64_t)n_scans + 1); ++i) cloud_offsets_host[i] = 0;
    if (n_scans == 0) return OT_OK;
    if (!ranges || !beam_cluster || !beam_class || !beam_xy_out || !n_clusters || !clusters || !wall_xyz ||
        !object_xyz || !unknown_xyz)
        return fail(OT_ERR_INVALID_ARGUMENT, "[LidarClusterer] invalid buffers");
    const int64_t nt = (int64_t)n_scans * n_beams;
    // beam directions: angle = angle_min + i * increment in float, then std::cos / std::sin of that float (:165-167)
    std::vector<float2> cs((size_t)n_beams);
    for (int i = 0; i < n_beams; ++i) {
        const float a = angle_min + i * angle_increment;
        cs[i] = make_float2(std::cos(a), std::sin(a));
    }
    std::vector<PoseM> hp;
    pose_rows(poses_host, n_scans, hp);
    const float r_use = range_max * params->max_range_ratio;  // :153, float
    const int blocks = std::min<int>(n_scans, SC_MAX_BLOCKS);
    float2* dcs = (float2*)scratch(sizeof(float2) * cs.size() + 64, Slot::SCAN_CS);
    PoseM* dp = (PoseM*)scratch(sizeof(PoseM) * hp.size() + 64, Slot::SCAN_POSE);
    Raw* raw = (Raw*)scratch(sizeof(Raw) * (size_t)blocks * n_beams + 64, Slot::SCAN_RAW);
    int32_t* pos = (int32_t*)scratch(sizeof(int32_t) * (size_t)nt + 64, Slot::SCAN_POS);
    int32_t* counts = (int32_t*)scratch(sizeof(int32_t) * 3 * (size_t)n_scans + 64, Slot::SCAN_COUNTS);
    int64_t* doff = (int64_t*)scratch(sizeof(int64_t) * 3 * ((size_t)n_scans + 1) + 64, Slot::SCAN_OFFSETS);
    if (!dcs || !dp || !raw || !pos || !counts || !doff) return fail(OT_ERR_HIP, "scratch allocation failed");
    OT_HIP_TRY(hipMemcpyAsync(dcs, cs.data(), sizeof(float2) * cs.size(), hipMemcpyHostToDevice, stream));
    OT_HIP_TRY(hipMemcpyAsync(dp, hp.data(), sizeof(PoseM) * (size_t)n_scans, hipMemcpyHostToDevice, stream));
    const size_t lds = (size_t)n_beams * 16;
    static std::atomic<bool> attr_set{false};
    ot_status st = set_dynamic_lds((const void*)k_scan_cluster, lds, attr_set);
    if (st != OT_OK) return st;
    hipLaunchKernelGGL(k_scan_cluster, dim3((unsigned)blocks), dim3(SC_THREADS), lds, stream, ranges, n_scans, n_beams,
                       (const float2*)dcs, r_use, *params, (const PoseM*)dp, raw, beam_cluster, beam_class, beam_xy_out,
                       n_clusters, clusters, pos, counts);
    OT_LAUNCH_CHECK();
    std::vector<int32_t> hc((size_t)n_scans * 3);
    OT_HIP_TRY(hipMemcpyAsync(hc.data(), counts, sizeof(int32_t) * hc.size(), hipMemcpyDeviceToHost, stream));
    OT_HIP_TRY(hipStreamSynchronize(stream));  // also releases cs / hp
    for (int k = 0; k < 3; ++k) {
        int64_t* o = cloud_offsets_host + (size_t)k * (n_scans + 1);
        for (int s = 0; s < n_scans; ++s) o[s + 1] = o[s] + hc[(size_t)s * 3 + k];
    }
    OT_HIP_TRY(hipMemcpyAsync(doff, cloud_offsets_host, sizeof(int64_t) * 3 * ((size_t)n_scans + 1),
                              hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_scan_cluster_emit, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, stream, n_scans, n_beams,
                       (const uint8_t*)beam_class, (const float*)beam_xy_out, (const int32_t*)pos,
                       (const int64_t*)doff, wall_xyz, object_xyz, unknown_xyz);
    OT_LAUNCH_CHECK();
    OT_HIP_TRY(hipStreamSynchronize(stream));
    return OT_OK;
}

ot_status ot_object_map_filter(const float* object_xyz, const int64_t* offsets_host, int32_t n_scans,
                               const float* virtual_ranges, int32_t n_beams, float angle_min, float angle_increment,
                               float range_max, const double* poses_host, double proximity_threshold,
                               uint8_t* keep_mask, float* out_xyz, int64_t* out_offsets_host, void* stream_) {
    hipStream_t stream = S(stream_);
    if (n_scans < 0 || n_beams <= 0 || !offsets_host || !out_offsets_host)
        return fail(OT_ERR_INVALID_ARGUMENT, "[ObjectMapFilter] invalid arguments");
    int64_t most = 0;
    for (int s = 0; s < n_scans; ++s) {
        const int64_t m = offsets_host[s + 1] - offsets_host[s];
        if (m < 0 || offsets_host[0] != 0)
            return fail(OT_ERR_INVALID_ARGUMENT, "[ObjectMapFilter] offsets must start at 0 and not decrease");
        most = std::max(most, m);
    }
    for (int s = 0; s <= n_scans; ++s) out_offsets_host[s] = 0;
    const int64_t total = n_scans > 0 ? offsets_host[n_scans] : 0;
    if (total == 0) return OT_OK;
    if (!object_xyz || !virtual_ranges || !keep_mask || !out_xyz || total > 0x7FFFFFFF ||
        (most + 255) / 256 > 65535)
        return fail(OT_ERR_INVALID_ARGUMENT, "[ObjectMapFilter] invalid buffers");
    std::vector<float2> cs((size_t)n_beams);
    for (int i = 0; i < n_beams; ++i) {
        const float a = angle_min + i * angle_increment;  // :68
        cs[i] = make_float2(std::cos(a), std::sin(a));
    }
    std::vector<ScanPose> hp((size_t)n_scans);
    for (int b = 0; b < n_scans; ++b) {
        if (!poses_host) {
            hp[b] = ScanPose{0.0, 0.0, 1.0, 0.0};
            continue;
        }
        const double* p = poses_host + (size_t)b * 7;
        const double qx = p[3], qy = p[4], qz = p[5], qw = p[6];
        const double yaw = std::atan2(2.0 * (qw * qz + qx * qy), 1.0 - 2.0 * (qy * qy + qz * qz));  // :166
        hp[b] = ScanPose{p[0], p[1], std::cos(yaw), std::sin(yaw)};
    }
    float2* dcs = (float2*)scratch(sizeof(float2) * cs.size() + 64, Slot::SCAN_CS);
    ScanPose* dp = (ScanPose*)scratch(sizeof(ScanPose) * hp.size() + 64, Slot::SCAN_POSE);
    int32_t* kept = (int32_t*)scratch(sizeof(int32_t) * (size_t)n_scans + 64, Slot::SCAN_COUNTS);
    int64_t* doff = (int64_t*)scratch(sizeof(int64_t) * ((size_t)n_scans + 1) + 64, Slot::SCAN_OFFSETS);
    if (!dcs || !dp || !kept || !doff) return fail(OT_ERR_HIP, "scratch allocation failed");
    OT_HIP_TRY(hipMemcpyAsync(dcs, cs.data(), sizeof(float2) * cs.size(), hipMemcpyHostToDevice, stream));
    OT_HIP_TRY(hipMemcpyAsync(dp, hp.data(), sizeof(ScanPose) * hp.size(), hipMemcpyHostToDevice, stream));
    OT_HIP_TRY(hipMemcpyAsync(doff, offsets_host, sizeof(int64_t) * ((size_t)n_scans + 1), hipMemcpyHostToDevice,
                              stream));
    OT_HIP_TRY(hipMemsetAsync(kept, 0, sizeof(int32_t) * (size_t)n_scans, stream));
    hipLaunchKernelGGL(k_object_filter, dim3((unsigned)n_scans, (unsigned)((most + 255) / 256)), dim3(256), 0, stream,
                       object_xyz, (const int64_t*)doff, virtual_ranges, n_beams, (const float2*)dcs, range_max,
                       (const ScanPose*)dp, proximity_threshold * proximity_threshold, keep_mask, kept);
    OT_LAUNCH_CHECK();
    int64_t n_kept = 0;
    ot_status st = compact(total, MaskPred{keep_mask}, Row3Emit{object_xyz, out_xyz}, stream, &n_kept, Slot::SCAN_COMPACT);
    if (st != OT_OK) return st;
    std::vector<int32_t> hk((size_t)n_scans);
    OT_HIP_TRY(hipMemcpyAsync(hk.data(), kept, sizeof(int32_t) * hk.size(), hipMemcpyDeviceToHost, stream));
    OT_HIP_TRY(hipStreamSynchronize(stream));
    for (int s = 0; s < n_scans; ++s) out_offsets_host[s + 1] = out_offsets_host[s] + hk[s];
    return OT_OK;
}

ot_status ot_cluster_observations(const float* points, int32_t point_stride, const int64_t* offsets_host,
                                  int32_t n_clouds, const double* poses_host, const ot_observation_params* params,
                                  float* out_rows, int32_t* n_obs_host, void* stream_) {
    hipStream_t stream = S(stream_);
    if (n_clouds < 0 || point_stride < 2 || !offsets_host || !params || (n_clouds > 0 && !n_obs_host))
        return fail(OT_ERR_INVALID_ARGUMENT, "[cluster_observations] invalid arguments");
    int64_t most = 0;
    for (int j = 0; j < n_clouds; ++j) {
        const int64_t m = offsets_host[j + 1] - offsets_host[j];
        if (m < 0 || offsets_host[0] != 0)
            return fail(OT_ERR_INVALID_ARGUMENT, "[cluster_observations] offsets must start at 0 and not decrease");
        most = std::max(most, m);
        n_obs_host[j] = 0;
    }
    if (most > SC_MAX_BEAMS)
        return fail(OT_ERR_INVALID_ARGUMENT, "[cluster_observations] a cloud of " + std::to_string(most) +
                                                 " points exceeds the " + std::to_string(SC_MAX_BEAMS) +
                                                 " points one workgroup stages");
    if (n_clouds == 0 || most == 0) return OT_OK;
    if (!points || !out_rows) return fail(OT_ERR_INVALID_ARGUMENT, "[cluster_observations] invalid buffers");
    std::vector<PoseM> hp;
    pose_rows(poses_host, n_clouds, hp);
    const int cap = (int)most;
    const int blocks = std::min<int>(n_clouds, SC_MAX_BLOCKS);
    PoseM* dp = (PoseM*)scratch(sizeof(PoseM) * hp.size() + 64, Slot::SCAN_POSE);
    Raw* raw = (Raw*)scratch(sizeof(Raw) * (size_t)blocks * cap + 64, Slot::SCAN_RAW);
    int32_t* counts = (int32_t*)scratch(sizeof(int32_t) * (size_t)n_clouds + 64, Slot::SCAN_COUNTS);
    int64_t* doff = (int64_t*)scratch(sizeof(int64_t) * ((size_t)n_clouds + 1) + 64, Slot::SCAN_OFFSETS);
    if (!dp || !raw || !counts || !doff) return fail(OT_ERR_HIP, "scratch allocation failed");
    OT_HIP_TRY(hipMemcpyAsync(dp, hp.data(), sizeof(PoseM) * (size_t)n_clouds, hipMemcpyHostToDevice, stream));
    OT_HIP_TRY(hipMemcpyAsync(doff, offsets_host, sizeof(int64_t) * ((size_t)n_clouds + 1), hipMemcpyHostToDevice,
                              stream));
    const size_t lds = (size_t)cap * 16;
    static std::atomic<bool> attr_set{false};
    ot_status st = set_dynamic_lds((const void*)k_cluster_obs, lds, attr_set);
    if (st != OT_OK) return st;
    hipLaunchKernelGGL(k_cluster_obs, dim3((unsigned)blocks), dim3(SC_THREADS), lds, stream, points, point_stride,
                       (const int64_t*)doff, n_clouds, cap, *params, (const PoseM*)dp, raw, out_rows, counts);
    OT_LAUNCH_CHECK();
    OT_HIP_TRY(hipMemcpyAsync(n_obs_host, counts, sizeof(int32_t) * (size_t)n_clouds, hipMemcpyDeviceToHost, stream));
    OT_HIP_TRY(hipStreamSynchronize(stream));
    return OT_OK;
}

}  // extern "C"
