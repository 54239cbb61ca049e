// tsdf_exchange.hip — units in and out of a ScalableTSDFVolume: the sorted unit order, export and import of whole units,
// and the border halo a spatially sharded volume sends its neighbours (layout: tsdf.h; the integrate: tsdf.hip and the kernel files it launches).
#include <algorithm>
#include <cstring>

#include "compact.h"
#include "sort.h"
#include "tsdf.h"

namespace ot {

// export: units in sorted order, voxels transposed to Open3D IndexOf order (x*256 + y*16 + z); colour as CT
// (float export of a float64 volume rounds to nearest)
template <typename CT, typename OT>
__global__ __launch_bounds__(256) void k_export(TsdfDev d, const unsigned* sorted_ids, int32_t* keys, float* tsdf,
                                                float* weight, OT* color) {
    const int r = blockIdx.x;
    const int id = (int)sorted_ids[r];
    const int tid = threadIdx.x;
    const float* base = unit_base(d, id);
    const CT* cbase = color_base<CT>(d, id);
    if (keys && tid < 3) keys[(int64_t)r * 3 + tid] = d.unit_keys[id * 3 + tid];
    for (int z = 0; z < UNIT_RES; ++z) {
        const int vi = z * 256 + tid;
        const int64_t o = (int64_t)r * UNIT_VOX + tid * 16 + z;
        if (tsdf) tsdf[o] = base[vi];
        if (weight) weight[o] = base[UNIT_VOX + vi];
        if (color) {
            color[o * 3 + 0] = (OT)cbase[vi];
            color[o * 3 + 1] = (OT)cbase[UNIT_VOX + vi];
            color[o * 3 + 2] = (OT)cbase[2 * UNIT_VOX + vi];
        }
    }
}

// border export: the BORDER_VOX low-face voxels of every unit, units in sorted order; colour as the volume keeps it
template <typename CT>
__global__ __launch_bounds__(256) void k_export_border(TsdfDev d, const unsigned* sorted_ids, int32_t* keys,
                                                       float* tsdf, float* weight, CT* color) {
    const int r = blockIdx.x;
    const int id = (int)sorted_ids[r];
    const float* base = unit_base(d, id);
    const CT* cbase = color_base<CT>(d, id);
    if (threadIdx.x < 3) keys[(int64_t)r * 3 + threadIdx.x] = d.unit_keys[id * 3 + threadIdx.x];
    for (int b = threadIdx.x; b < BORDER_VOX; b += 256) {
        int x, y, z;
        border_voxel(b, x, y, z);
        const int vi = z * 256 + x * 16 + y;
        const int64_t o = (int64_t)r * BORDER_VOX + b;
        tsdf[o] = base[vi];
        weight[o] = base[UNIT_VOX + vi];
        if (color) {
            color[o * 3 + 0] = cbase[vi];
            color[o * 3 + 1] = cbase[UNIT_VOX + vi];
            color[o * 3 + 2] = cbase[2 * UNIT_VOX + vi];
        }
    }
}

__device__ inline int find_unit_id(const TsdfDev& d, int x, int y, int z) {
    if (!key_in_range(x, y, z)) return -1;
    const unsigned long long key = pack_key(x, y, z);
    unsigned slot = (unsigned)mix64(key) & (unsigned)d.hash_mask;
    for (int probe = 0; probe <= d.hash_mask; ++probe) {
        const unsigned long long k = d.hkeys[slot];
        if (k == key) {
            const int id = d.hvals[slot];
            return id < d.max_units ? id : -1;
        }
        if (k == KEY_EMPTY) return -1;
        slot = (slot + 1) & (unsigned)d.hash_mask;
    }
    return -1;
}

// border import (halo): a row becomes a halo unit of this volume when its key is not owned here and one of its
// -x/-y/-z neighbours (the units whose marching cubes read it) is; a new halo unit is zeroed (weight 0 = unobserved)
// and receives the border voxels.  Rows of owned or unneeded units are skipped.
template <typename CT>
__global__ __launch_bounds__(256) void k_import_border(TsdfDev d, const int32_t* __restrict__ keys,
                                                       const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                       const CT* __restrict__ color) {
    __shared__ int s_id, s_fresh;
    const int r = blockIdx.x;
    if (threadIdx.x == 0) {
        const int x = keys[(int64_t)r * 3], y = keys[(int64_t)r * 3 + 1], z = keys[(int64_t)r * 3 + 2];
        int id = -1, fresh = 0;
        bool needed = false;
        if (key_in_range(x, y, z) && !unit_owned(d, pack_key(x, y, z))) {
            for (int t = 1; t < 8 && !needed; ++t) {
                const int nx = x - ((t >> 2) & 1), ny = y - ((t >> 1) & 1), nz = z - (t & 1);
                needed = key_in_range(nx, ny, nz) && unit_owned(d, pack_key(nx, ny, nz)) &&
                         find_unit_id(d, nx, ny, nz) >= 0;
            }
        }
        if (needed) {
            const int slot = hash_insert(d, pack_key(x, y, z));
            if (slot < 0) {
                atomicOr(&d.counters[C_HASHERR], 1);
            } else {
                id = d.hvals[slot];
                if (id < 0) {
                    id = atomicAdd(&d.counters[C_UNITS], 1);
                    if (id >= d.max_units) {
                        atomicOr(&d.counters[C_OVERFLOW], 1);
                        id = -1;
                    } else {
                        d.hvals[slot] = id;
                        d.unit_keys[id * 3 + 0] = x;
                        d.unit_keys[id * 3 + 1] = y;
                        d.unit_keys[id * 3 + 2] = z;
                        fresh = 1;
                        note_unit_key(d, x, y, z);
                    }
                }
            }
        }
        s_id = id;
        s_fresh = fresh;
    }
    __syncthreads();
    const int id = s_id;
    if (id < 0) return;
    float* base = unit_base(d, id);
    CT* cbase = color_base<CT>(d, id);
    if (s_fresh) {
        for (int vi = threadIdx.x; vi < UNIT_VOX; vi += 256) {
            base[vi] = 0.0f;
            base[UNIT_VOX + vi] = 0.0f;
            cbase[vi] = cbase[UNIT_VOX + vi] = cbase[2 * UNIT_VOX + vi] = (CT)0;
        }
        __syncthreads();
    }
    for (int b = threadIdx.x; b < BORDER_VOX; b += 256) {
        int x, y, z;
        border_voxel(b, x, y, z);
        const int vi = z * 256 + x * 16 + y;
        const int64_t o = (int64_t)r * BORDER_VOX + b;
        base[vi] = tsdf[o];
        base[UNIT_VOX + vi] = weight[o];
        cbase[vi] = color ? color[o * 3 + 0] : (CT)0;
        cbase[UNIT_VOX + vi] = color ? color[o * 3 + 1] : (CT)0;
        cbase[2 * UNIT_VOX + vi] = color ? color[o * 3 + 2] : (CT)0;
    }
}

// destinations of a border row (SURVEY §8(e) halo): the ranks owning the unit's 7 -x/-y/-z neighbours (the units whose
// marching cubes read its low faces), this rank excluded -- a superset of the rows k_import_border keeps there
__global__ __launch_bounds__(256) void k_border_dest(TsdfDev d, int64_t n, const int32_t* __restrict__ keys,
                                                     unsigned long long* __restrict__ mask) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int x = keys[r * 3], y = keys[r * 3 + 1], z = keys[r * 3 + 2];
    unsigned long long m = 0ull;
    if (d.shard_world > 1)
        for (int t = 1; t < 8; ++t) {
            const int nx = x - ((t >> 2) & 1), ny = y - ((t >> 1) & 1), nz = z - (t & 1);
            if (key_in_range(nx, ny, nz)) m |= 1ull << unit_owner(d, nx, ny, nz);
        }
    mask[r] = m & ~(1ull << d.shard_rank);
}

// owned units of the sorted order (a sharded volume's own units; every unit when unsharded)
struct OwnedPred {
    TsdfDev d;
    const unsigned* sorted_ids;
    __device__ bool operator()(int64_t r) const {
        const int id = (int)sorted_ids[r];
        return d.shard_world <= 1 ||
               unit_owned(d, pack_key(d.unit_keys[id * 3], d.unit_keys[id * 3 + 1], d.unit_keys[id * 3 + 2]));
    }
};
struct OwnedEmit {
    const unsigned* sorted_ids;
    unsigned* out;
    __device__ void operator()(int64_t r, int64_t pos) const { out[pos] = sorted_ids[r]; }
};

// Units an export lists: every unit in sorted key order or, for a spatially sharded volume, only its own units -- the
// halo units imported for marching cubes (k_import_border) are copies of other shards' border rows, and exporting
// them would hand their keys to an assembly twice (the second time with zeros inside the unit).
ot_status export_list(ot_tsdf* vol, hipStream_t stream, const unsigned** ids, int64_t* n) {
    int64_t nu = 0;
    ot_status st = tsdf_sorted_units(vol, stream, &nu);
    if (st != OT_OK) return st;
    *ids = vol->sorted_ids;
    *n = nu;
    if (vol->dev.shard_world <= 1 || nu == 0) return OT_OK;
    unsigned* own = (unsigned*)scratch(sizeof(unsigned) * (size_t)nu + 256, Slot::MESH_NORMALS_WS);
    if (!own) return fail(OT_ERR_HIP, "scratch allocation failed");
    int64_t no = 0;
    st = compact(nu, OwnedPred{vol->dev, vol->sorted_ids}, OwnedEmit{vol->sorted_ids, own}, stream, &no, Slot::OP_COMPACT);
    if (st != OT_OK) return st;
    *ids = own;
    *n = no;
    return OT_OK;
}

// import: the inverse of k_export (keys unique within one call; an existing unit is overwritten); colour as the
// volume keeps it (CT)
template <typename CT>
__global__ __launch_bounds__(256) void k_import(TsdfDev d, const int32_t* __restrict__ keys,
                                                const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                const CT* __restrict__ color) {
    __shared__ int s_id;
    const int r = blockIdx.x;
    const int tid = threadIdx.x;
    if (tid == 0) {
        const int x = keys[(int64_t)r * 3], y = keys[(int64_t)r * 3 + 1], z = keys[(int64_t)r * 3 + 2];
        int id = -1;
        if (!key_in_range(x, y, z)) {
            atomicOr(&d.counters[C_HASHERR], 2);
        } else {
            const int slot = hash_insert(d, pack_key(x, y, z));
            if (slot < 0) {
                atomicOr(&d.counters[C_HASHERR], 1);
            } else {
                id = d.hvals[slot];
                if (id < 0) {
                    id = atomicAdd(&d.counters[C_UNITS], 1);
                    if (id >= d.max_units) {
                        atomicOr(&d.counters[C_OVERFLOW], 1);
                        id = -1;
                    } else {
                        d.hvals[slot] = id;
                        d.unit_keys[id * 3 + 0] = x;
                        d.unit_keys[id * 3 + 1] = y;
                        d.unit_keys[id * 3 + 2] = z;
                        note_unit_key(d, x, y, z);
                    }
                }
            }
        }
        s_id = id;
    }
    __syncthreads();
    const int id = s_id;
    if (id < 0) return;
    float* base = unit_base(d, id);
    CT* cbase = color_base<CT>(d, id);
    for (int z = 0; z < UNIT_RES; ++z) {
        const int vi = z * 256 + tid;
        const int64_t o = (int64_t)r * UNIT_VOX + tid * 16 + z;
        base[vi] = tsdf[o];
        base[UNIT_VOX + vi] = weight[o];
        cbase[vi] = color ? color[o * 3 + 0] : (CT)0;
        cbase[UNIT_VOX + vi] = color ? color[o * 3 + 1] : (CT)0;
        cbase[2 * UNIT_VOX + vi] = color ? color[o * 3 + 2] : (CT)0;
    }
}

// order-preserving compact keys: (x - x0) << (by + bz) | (y - y0) << bz | (z - z0), only the bits the ranges need
struct UnitKeyPack {
    int x0, y0, z0, sy, sx;
};

__global__ void k_pack_unit_keys(TsdfDev d, int n, UnitKeyPack pk, unsigned long long* keys, unsigned* ids) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    keys[i] = ((unsigned long long)(d.unit_keys[i * 3 + 0] - pk.x0) << pk.sx) |
              ((unsigned long long)(d.unit_keys[i * 3 + 1] - pk.y0) << pk.sy) |
              (unsigned long long)(d.unit_keys[i * 3 + 2] - pk.z0);
    ids[i] = (unsigned)i;
}

// Unit order in ONE launch when the packed keys need <= USORT_BITS bits (a volume a few metres across): unit keys are
// distinct (one id per hash slot), so a unit's place in key order is the number of smaller keys -- a presence bitmap
// of the key space in LDS, a block scan of its popcounts per 8-word group, then per unit the group prefix plus the
// popcounts before its bit.  The same ids as the radix sort (k_pack_unit_keys + 4 launches of sort_pairs_u64_u32),
// whose launches dominated the unit sort of a single object (38 us for 5.6k units, profiles/r04z_obj_timeline.txt).
constexpr int USORT_BITS = 20;                   // 2^20-bit bitmap: 128 KiB of LDS
constexpr int USORT_WORDS = 1 << (USORT_BITS - 5);
constexpr int USORT_GROUPS = USORT_WORDS / 8;    // 4096 group prefixes: 16 KiB
__device__ inline unsigned unit_key_bits(const TsdfDev& d, const UnitKeyPack& pk, int i) {
    return ((unsigned)(d.unit_keys[i * 3 + 0] - pk.x0) << pk.sx) | ((unsigned)(d.unit_keys[i * 3 + 1] - pk.y0) << pk.sy) |
           (unsigned)(d.unit_keys[i * 3 + 2] - pk.z0);
}
__global__ __launch_bounds__(1024) void k_unit_rank_sort(TsdfDev d, int n, UnitKeyPack pk, int kb,
                                                         unsigned* __restrict__ sorted_ids) {
    __shared__ unsigned s_bits[USORT_WORDS];
    __shared__ unsigned s_gp[USORT_GROUPS];
    __shared__ unsigned s_w[16];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int words = kb > 5 ? 1 << (kb - 5) : 1, groups = (words + 7) >> 3;
    for (int q = t; q < words; q += 1024) s_bits[q] = 0u;
    __syncthreads();
    for (int i = t; i < n; i += 1024) {
        const unsigned k = unit_key_bits(d, pk, i);
        atomicOr(&s_bits[k >> 5], 1u << (k & 31));
    }
    __syncthreads();
    // thread t: groups [g0, g1), a contiguous stretch (4 groups = 32 words at 20 bits)
    const int per = (groups + 1023) >> 10, g0 = t * per, g1 = g0 + per < groups ? g0 + per : groups;
    unsigned loc = 0u;
    for (int g = g0; g < g1; ++g)
        for (int q = g * 8; q < g * 8 + 8 && q < words; ++q) loc += __popc(s_bits[q]);
    unsigned inc = loc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
    }
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    unsigned run = inc - loc;
    for (int q = 0; q < w; ++q) run += s_w[q];
    for (int g = g0; g < g1; ++g) {
        s_gp[g] = run;
        for (int q = g * 8; q < g * 8 + 8 && q < words; ++q) run += __popc(s_bits[q]);
    }
    __syncthreads();
    for (int i = t; i < n; i += 1024) {
        const unsigned k = unit_key_bits(d, pk, i);
        const int q = (int)(k >> 5);
        unsigned r = s_gp[q >> 3] + __popc(s_bits[q] & ((1u << (k & 31)) - 1u));
        for (int p = q & ~7; p < q; ++p) r += __popc(s_bits[p]);
        sorted_ids[r] = (unsigned)i;
    }
}

static ot_status counter_errors(const int* c) {
    if (c[C_OVERFLOW]) return fail(OT_ERR_CAPACITY, "[ScalableTSDFVolume] volume unit pool exhausted (max_units)");
    if (c[C_HASHERR] & 1) return fail(OT_ERR_CAPACITY, "[ScalableTSDFVolume] unit hash table full");
    if (c[C_HASHERR] & 2) return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume] unit index out of range");
    return OT_OK;
}

static ot_status check_errors(ot_tsdf* vol, hipStream_t stream) {
    int c[N_COUNTERS];
    OT_HIP_TRY(hipMemcpyAsync(c, vol->dev.counters, sizeof(c), hipMemcpyDeviceToHost, stream));
    OT_HIP_TRY(hipStreamSynchronize(stream));
    if (c[C_OVERFLOW]) return fail(OT_ERR_CAPACITY, "[ScalableTSDFVolume] volume unit pool exhausted (max_units)");
    if (c[C_HASHERR] & 1) return fail(OT_ERR_CAPACITY, "[ScalableTSDFVolume] unit hash table full");
    if (c[C_HASHERR] & 2) return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume] unit index out of range");
    return OT_OK;
}

ot_status tsdf_sorted_units(ot_tsdf* vol, hipStream_t stream, int64_t* n_units) {
    ot_status st = tsdf_flush(vol, stream);
    if (st != OT_OK) return st;
    int c[N_COUNTERS];  // error flags and the unit count in one read-back (the pinned mailbox)
    if (vol->early_frame == vol->frame_id && !vol->imported && vol->units_seq != 0) {
        // mailed by the last batch's units kernel (settle_batch saw it): not waiting for the integrate behind it
        st = mail_wait(vol->hmail + MAIL_SEQ_UNITS, vol->units_seq, stream);
        if (st != OT_OK) return st;
        std::memcpy(c, vol->hmail + OT_MAIL_WORDS, sizeof(c));
    } else {
        MailSrc ms;
        ms.n = N_COUNTERS;
        for (int i = 0; i < N_COUNTERS; ++i) ms.p[i] = (const unsigned*)vol->dev.counters + i;
        st = mail_words(vol, ms, stream);
        if (st != OT_OK) return st;
        std::memcpy(c, vol->hmail, sizeof(c));
    }
    st = counter_errors(c);
    if (st != OT_OK) return st;
    int nu = (int)std::min<int64_t>(c[C_UNITS], vol->max_units);
    *n_units = nu;
    if (vol->sorted_frame == vol->frame_id && vol->sorted_units == nu) return OT_OK;
    if (nu > 0) {
        int hb[6];  // per-axis key bounds, kept by the allocating kernels (note_unit_key)
        for (int a = 0; a < 3; ++a) {
            hb[a] = KEY_BIAS + 1 - c[C_KNEG + a];
            hb[3 + a] = c[C_KMAX + a] - KEY_BIAS - 1;
        }
        int bits[3];
        for (int a = 0; a < 3; ++a) {
            const long long span = (long long)hb[3 + a] - hb[a];
            bits[a] = 1;
            while (bits[a] < 31 && (span >> bits[a]) != 0) ++bits[a];
        }
        const UnitKeyPack pk{hb[0], hb[1], hb[2], bits[2], bits[1] + bits[2]};
        const int kb = bits[0] + bits[1] + bits[2];
        if (kb <= USORT_BITS && !g_tsdf_hooks.unit_sort_radix) {  // (the hook: the radix path's parity)
            hipLaunchKernelGGL(k_unit_rank_sort, dim3(1), dim3(1024), 0, stream, vol->dev, nu, pk, kb, vol->sorted_ids);
            OT_LAUNCH_CHECK();
            vol->sorted_units = nu;
            vol->sorted_frame = vol->frame_id;
            return OT_OK;
        }
        char* ws = (char*)scratch((size_t)nu * 24 + 256, Slot::TSDF_UNIT_SORT);
        if (!ws) return fail(OT_ERR_HIP, "scratch allocation failed");
        unsigned long long* kin = (unsigned long long*)(ws + 256);
        unsigned long long* kout = kin + nu;
        unsigned* vin = (unsigned*)(kout + nu);
        hipLaunchKernelGGL(k_pack_unit_keys, dim3((nu + 255) / 256), dim3(256), 0, stream, vol->dev, nu, pk, kin, vin);
        OT_LAUNCH_CHECK();
        st = sort_pairs_u64_u32(kin, kout, vin, vol->sorted_ids, (size_t)nu, std::min(63, bits[0] + bits[1] + bits[2]),
                                stream, Slot::SORT_TMP);
        if (st != OT_OK) return st;
    }
    vol->sorted_units = nu;
    vol->sorted_frame = vol->frame_id;
    return OT_OK;
}

}  // namespace ot

using namespace ot;

extern "C" {

ot_status ot_tsdf_export_units(ot_tsdf* vol, int64_t capacity, int32_t* keys, float* tsdf, float* weight, float* color,
                               void* stream) {
    if (!vol) return fail(OT_ERR_INVALID_ARGUMENT, "invalid arguments");
    int64_t nu = 0;
    const unsigned* ids = nullptr;
    ot_status st = export_list(vol, S(stream), &ids, &nu);
    if (st != OT_OK) return st;
    if (nu > capacity) return fail(OT_ERR_CAPACITY, "[ScalableTSDFVolume] export: more units than the output capacity");
    if (nu == 0) return OT_OK;
    if (vol->color64)
        hipLaunchKernelGGL((k_export<double, float>), dim3((unsigned)nu), dim3(256), 0, S(stream), vol->dev, ids, keys,
                           tsdf, weight, color);
    else
        hipLaunchKernelGGL((k_export<float, float>), dim3((unsigned)nu), dim3(256), 0, S(stream), vol->dev, ids, keys,
                           tsdf, weight, color);
    OT_LAUNCH_CHECK();
    OT_HIP_TRY(hipStreamSynchronize(S(stream)));
    return OT_OK;
}

ot_status ot_tsdf_export_color64(ot_tsdf* vol, int64_t capacity, double* color, void* stream) {
    if (!vol || !color) return fail(OT_ERR_INVALID_ARGUMENT, "invalid arguments");
    int64_t nu = 0;
    const unsigned* ids = nullptr;
    ot_status st = export_list(vol, S(stream), &ids, &nu);
    if (st != OT_OK) return st;
    if (nu > capacity) return fail(OT_ERR_CAPACITY, "[ScalableTSDFVolume] export: more units than the output capacity");
    if (nu == 0) return OT_OK;
    if (vol->color64)
        hipLaunchKernelGGL((k_export<double, double>), dim3((unsigned)nu), dim3(256), 0, S(stream), vol->dev, ids,
                           nullptr, nullptr, nullptr, color);
    else  // float32 colour state (or NoColor's zero planes) widens exactly
        hipLaunchKernelGGL((k_export<float, double>), dim3((unsigned)nu), dim3(256), 0, S(stream), vol->dev, ids,
                           nullptr, nullptr, nullptr, color);
    OT_LAUNCH_CHECK();
    OT_HIP_TRY(hipStreamSynchronize(S(stream)));
    return OT_OK;
}

ot_status ot_tsdf_border_destinations(const ot_tsdf* vol, int64_t n, const int32_t* keys, int64_t* dest_mask,
                                      void* stream) {
    if (!vol || n < 0 || (n > 0 && (!keys || !dest_mask)) || vol->dev.shard_world > 64)
        return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume] border_destinations: invalid arguments");
    if (n == 0) return OT_OK;
    hipLaunchKernelGGL(k_border_dest, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), vol->dev, n, keys,
                       (unsigned long long*)dest_mask);
    OT_LAUNCH_CHECK();
    return OT_OK;
}

}  // extern "C"

template <typename CT>
static ot_status import_units(ot_tsdf* vol, int64_t n, const int32_t* keys, const float* tsdf, const float* weight,
                              const CT* color, hipStream_t stream) {
    if (!vol || n < 0 || (n > 0 && (!keys || !tsdf || !weight)))
        return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume] import: invalid arguments");
    const bool rgb8 = vol->color_type == OT_COLOR_RGB8;
    if (rgb8 && vol->color64 != (sizeof(CT) == 8))
        return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume] import: colour dtype does not match the volume's "
                                             "colour precision");
    ot_status st = tsdf_flush(vol, stream);
    if (st != OT_OK) return st;
    if (n == 0) return OT_OK;
    st = reserve_units(vol, n, stream);  // the pool grows instead of dropping imported units
    if (st != OT_OK) return st;
    if (rgb8)
        hipLaunchKernelGGL(k_import<CT>, dim3((unsigned)n), dim3(256), 0, stream, vol->dev, keys, tsdf, weight, color);
    else  // NoColor: float32 record, zero colour planes
        hipLaunchKernelGGL(k_import<float>, dim3((unsigned)n), dim3(256), 0, stream, vol->dev, keys, tsdf, weight,
                           (const float*)nullptr);
    OT_LAUNCH_CHECK();
    vol->sorted_units = -1;  // the sorted-unit cache no longer matches
    vol->imported = true;    // arbitrary state: the IEEE-division integrate from now on
    vol->stat_prev_units = -1;
    vol->mesh.valid = false;
    vol->cloud.valid = false;
    st = check_errors(vol, stream);
    if (st != OT_OK) return st;
    OT_HIP_TRY(hipStreamSynchronize(stream));
    return OT_OK;
}

extern "C" {

ot_status ot_tsdf_import_units(ot_tsdf* vol, int64_t n, const int32_t* keys, const float* tsdf, const float* weight,
                               const float* color, void* stream) {
    return import_units<float>(vol, n, keys, tsdf, weight, color, S(stream));
}

ot_status ot_tsdf_import_units_color64(ot_tsdf* vol, int64_t n, const int32_t* keys, const float* tsdf,
                                       const float* weight, const double* color, void* stream) {
    return import_units<double>(vol, n, keys, tsdf, weight, color, S(stream));
}

ot_status ot_tsdf_export_border(ot_tsdf* vol, int64_t capacity, int32_t* keys, float* tsdf, float* weight, void* color,
                                int64_t* n_exported_host, void* stream) {
    if (!vol || !keys || !tsdf || !weight || !n_exported_host) return fail(OT_ERR_INVALID_ARGUMENT, "invalid arguments");
    *n_exported_host = 0;
    int64_t no = 0;  // the own units (halo units imported earlier are not this shard's border)
    const unsigned* own = nullptr;
    ot_status st = export_list(vol, S(stream), &own, &no);
    if (st != OT_OK) return st;
    if (no == 0) return OT_OK;
    if (no > capacity) return fail(OT_ERR_CAPACITY, "[ScalableTSDFVolume] export: more units than the output capacity");
    if (no > 0) {
        if (vol->color_type != OT_COLOR_RGB8)  // NoColor: no colour rows (the caller's buffer is left as it is)
            hipLaunchKernelGGL(k_export_border<float>, dim3((unsigned)no), dim3(256), 0, S(stream), vol->dev, own,
                               keys, tsdf, weight, (float*)nullptr);
        else if (vol->color64)
            hipLaunchKernelGGL(k_export_border<double>, dim3((unsigned)no), dim3(256), 0, S(stream), vol->dev, own,
                               keys, tsdf, weight, (double*)color);
        else
            hipLaunchKernelGGL(k_export_border<float>, dim3((unsigned)no), dim3(256), 0, S(stream), vol->dev, own,
                               keys, tsdf, weight, (float*)color);
        OT_LAUNCH_CHECK();
    }
    OT_HIP_TRY(hipStreamSynchronize(S(stream)));
    *n_exported_host = no;
    return OT_OK;
}

ot_status ot_tsdf_import_border(ot_tsdf* vol, int64_t n, const int32_t* keys, const float* tsdf, const float* weight,
                                const void* color, void* stream_) {
    hipStream_t stream = S(stream_);
    if (!vol || n < 0 || (n > 0 && (!keys || !tsdf || !weight)))
        return fail(OT_ERR_INVALID_ARGUMENT, "[ScalableTSDFVolume] import_border: invalid arguments");
    ot_status st = tsdf_flush(vol, stream);
    if (st != OT_OK) return st;
    if (n == 0) return OT_OK;
    st = reserve_units(vol, n, stream);  // halo units: room for every row (a superset of those kept)
    if (st != OT_OK) return st;
    const void* c = vol->color_type == OT_COLOR_RGB8 ? color : nullptr;
    if (vol->color64)  // (only RGB8 volumes store float64 colour)
        hipLaunchKernelGGL(k_import_border<double>, dim3((unsigned)n), dim3(256), 0, stream, vol->dev, keys, tsdf,
                           weight, (const double*)c);
    else
        hipLaunchKernelGGL(k_import_border<float>, dim3((unsigned)n), dim3(256), 0, stream, vol->dev, keys, tsdf,
                           weight, (const float*)c);
    OT_LAUNCH_CHECK();
    vol->sorted_units = -1;
    vol->imported = true;  // halo units hold other shards' state (read by marching cubes; kept exact anyway)
    vol->stat_prev_units = -1;
    vol->mesh.valid = false;
    vol->cloud.valid = false;
    st = check_errors(vol, stream);
    if (st != OT_OK) return st;
    OT_HIP_TRY(hipStreamSynchronize(stream));
    return OT_OK;
}

}  // extern "C"
