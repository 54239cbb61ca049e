// workspace.h — one buffer cut into typed arrays, described once (host only; no HIP types, so any C++ compiler
// builds it).
//
//     auto [keys, heads] = carve(scratch_of(Slot::...), Arr<unsigned long long>{n}, Arr<int>{n});
//
// alloc(size_t bytes) answers the base.  The size asked of it and the pointers cut from its answer come from the same
// list, so they cannot disagree.  Every array starts on CARVE_ALIGN bytes from the base (hipMalloc aligns the base at
// least as much); all arithmetic is size_t.  A zero-count array takes no bytes; the request is never zero bytes; when
// the allocator answers nullptr every pointer is null.
#pragma once

#include <cstddef>
#include <tuple>

namespace ot {

template <typename T>
struct Arr {
    size_t count;
};

constexpr size_t CARVE_ALIGN = 256;
inline size_t carve_up(size_t bytes) { return (bytes + CARVE_ALIGN - 1) & ~(CARVE_ALIGN - 1); }

template <typename Alloc, typename... T>
std::tuple<T*...> carve(Alloc&& alloc, Arr<T>... a) {
    size_t off[sizeof...(T)], end = 0, i = 0;
    ((off[i++] = end = carve_up(end), end += a.count * sizeof(T)), ...);
    char* base = static_cast<char*>(alloc(end ? end : CARVE_ALIGN));
    i = 0;
    return std::tuple<T*...>{(base ? reinterpret_cast<T*>(base + off[i++]) : nullptr)...};
}

// ---- the grid's and the SOR statistics' workspaces: here, so tests/workspace_check.cpp lays out what the library does
struct alignas(8) IntPair {  // int2 without HIP
    int x, y;
};

// build_grid_frames: error word, keys (in / out; 32-bit sorts run in the first array's bytes: n keys in, n keys out)
// and values (in / out) of the cell sort, cell heads, point -> cell, the re-laid-out points
template <typename Alloc>
auto grid_points_ws(Alloc&& alloc, size_t n) {
    return carve(alloc, Arr<int>{1}, Arr<unsigned long long>{n}, Arr<unsigned long long>{n}, Arr<unsigned>{n},
                 Arr<unsigned>{n}, Arr<int>{n}, Arr<int>{n}, Arr<double>{3 * n});
}

// the column hash (cap keys and values) and, for ncells occupied cells, the 3x3 and 5x5 column ranges (when built),
// the cells' point ranges and their z
template <typename Alloc>
auto grid_cells_ws(Alloc&& alloc, size_t cap, size_t ncells, bool w3, bool w5) {
    return carve(alloc, Arr<unsigned long long>{cap}, Arr<IntPair>{cap}, Arr<IntPair>{w3 ? ncells * 9 : 0},
                 Arr<IntPair>{w5 ? ncells * 25 : 0}, Arr<IntPair>{ncells}, Arr<int>{ncells});
}

// sor_stats_frames over n points in F frames: the chains' inputs, their sums, valid-count partials (nvb blocks per
// frame), the chains' auxiliary arrays (aux_bytes: chain.h, summed over the frames) and the job table
template <typename Alloc>
auto sor_stats_ws(Alloc&& alloc, size_t n, size_t F, size_t nvb, size_t aux_bytes, size_t job_bytes) {
    return carve(alloc, Arr<double>{n}, Arr<double>{F}, Arr<int>{F * nvb}, Arr<char>{aux_bytes},
                 Arr<char>{F * job_bytes});
}

}  // namespace ot
