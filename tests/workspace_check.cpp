// workspace_check — csrc/workspace.h on the host, under ASan + UBSan (tests/test_workspace_carve.py builds and runs it).
//
// Every description is laid out into a host allocation of exactly the bytes carve() asks for; every element of every
// array is written through its typed pointer (a misaligned or out-of-bounds array is a sanitizer report), then read
// back (an overlap shows as a foreign tag), and the intervals are checked directly: each starts on CARVE_ALIGN, they
// are pairwise disjoint, the last ends within the bytes asked for.  One line per description: "<name> <parameters ...>
// <bytes>", which the test compares with its own arithmetic.  The last lines are size-only passes at n = 0x7FFFFFFF.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "workspace.h"

using namespace ot;

struct Region {
    size_t off, bytes;
    unsigned char tag;
};

static int g_failures = 0;
static void fail(const char* what, const char* name, size_t a, size_t b) {
    std::fprintf(stderr, "FAIL %s: %s (%zu, %zu)\n", name, what, a, b);
    ++g_failures;
}

// the allocator handed to carve(): an allocation of exactly the bytes asked for (size_only: none, every pointer null)
struct Layout {
    char* base = nullptr;
    size_t bytes = 0;
    bool size_only;
    std::vector<Region> regions;

    explicit Layout(bool size_only_ = false) : size_only(size_only_) {}
    ~Layout() { std::free(base); }
    void* operator()(size_t b) {
        bytes = b;
        void* p = nullptr;
        if (!size_only && posix_memalign(&p, CARVE_ALIGN, b) != 0) std::abort();
        return base = static_cast<char*>(p);
    }

    template <typename T>
    void write(T* p, size_t count) {
        const unsigned char tag = (unsigned char)(regions.size() + 1);
        T v;
        std::memset(&v, tag, sizeof(T));
        for (size_t i = 0; i < count; ++i) p[i] = v;
        regions.push_back(Region{(size_t)(reinterpret_cast<char*>(p) - base), count * sizeof(T), tag});
    }

    void check(const char* name) const {
        for (size_t i = 0; i < regions.size(); ++i) {
            const Region& r = regions[i];
            if (r.off % CARVE_ALIGN) fail("array not on its alignment", name, i, r.off);
            if (r.off + r.bytes > bytes) fail("array ends past the bytes asked for", name, i, r.off + r.bytes);
            for (size_t k = 0; k < r.bytes; ++k)
                if ((unsigned char)base[r.off + k] != r.tag) {
                    fail("array overwritten by another", name, i, k);
                    break;
                }
            for (size_t j = i + 1; j < regions.size(); ++j) {
                const Region& s = regions[j];
                if (r.bytes && s.bytes && r.off < s.off + s.bytes && s.off < r.off + r.bytes)
                    fail("arrays overlap", name, i, j);
            }
        }
    }
};

static size_t grid_points(size_t n, bool size_only = false) {
    Layout l(size_only);
    auto [err, kin, kout, vin, vout, heads, pcell, sxyz] = grid_points_ws(l, n);
    if (size_only) return l.bytes;
    l.write(err, 1);
    l.write(kin, n);
    l.write(kout, n);
    l.write(vin, n);
    l.write(vout, n);
    l.write(heads, n);
    l.write(pcell, n);
    l.write(sxyz, 3 * n);
    l.check("grid_points");
    std::printf("grid_points %zu %zu\n", n, l.bytes);
    return l.bytes;
}

static size_t grid_cells(size_t cap, size_t ncells, bool w3, bool w5, bool size_only = false) {
    Layout l(size_only);
    auto [hkeys, hval, nbr3, nbr5, crange, cz] = grid_cells_ws(l, cap, ncells, w3, w5);
    if (size_only) return l.bytes;
    l.write(hkeys, cap);
    l.write(hval, cap);
    l.write(nbr3, w3 ? ncells * 9 : 0);  // a zero-count array in the middle when the block is not built
    l.write(nbr5, w5 ? ncells * 25 : 0);
    l.write(crange, ncells);
    l.write(cz, ncells);
    l.check("grid_cells");
    std::printf("grid_cells %zu %zu %d %d %zu\n", cap, ncells, (int)w3, (int)w5, l.bytes);
    return l.bytes;
}

static size_t sor_stats(size_t n, size_t F, size_t nvb, size_t aux_bytes, size_t job, bool size_only = false) {
    Layout l(size_only);
    auto [x, sums, vpart, aux, jobs] = sor_stats_ws(l, n, F, nvb, aux_bytes, job);
    if (size_only) return l.bytes;
    l.write(x, n);
    l.write(sums, F);
    l.write(vpart, F * nvb);
    l.write(aux, aux_bytes);
    l.write(jobs, F * job);
    l.check("sor_stats");
    std::printf("sor_stats %zu %zu %zu %zu %zu %zu\n", n, F, nvb, aux_bytes, job, l.bytes);
    return l.bytes;
}

static void plain() {  // carve itself: mixed element sizes, a zero-count array in the middle, and nothing at all
    Layout l;
    auto [a, z, b, d] = carve(l, Arr<int>{5}, Arr<double>{0}, Arr<char>{3}, Arr<unsigned long long>{33});
    l.write(a, 5);
    l.write(z, 0);
    l.write(b, 3);
    l.write(d, 33);
    l.check("plain");
    std::printf("plain %zu\n", l.bytes);
    Layout e;
    auto [none] = carve(e, Arr<double>{0});
    e.write(none, 0);
    e.check("empty");
    std::printf("empty %zu\n", e.bytes);
}

static size_t hash_cap(size_t ncells) {  // the grid build's capacity rule
    size_t cap = 1;
    while (cap < 2 * ncells + 2) cap <<= 1;
    return cap;
}

int main() {
    const size_t JOB = 120;  // sizeof(ChainJob)
    for (size_t n : {(size_t)0, (size_t)1, (size_t)255, (size_t)256, (size_t)257}) {
        grid_points(n);
        for (int nbr = 0; nbr < 4; ++nbr) grid_cells(hash_cap(n), n, nbr & 1, nbr & 2);
        for (size_t F : {(size_t)1, (size_t)3}) {
            const size_t nvb = (n + 255) / 256 ? (n + 255) / 256 : 1;
            const size_t aux = F * (((n + 255) / 256 + 1) * 64 + 512);  // chain.h's bound, one chain per frame
            sor_stats(n, F, nvb, aux, JOB);
        }
    }
    plain();
    // size only: the largest n the entry points accept (nothing is allocated)
    const size_t big = 0x7FFFFFFF;
    std::printf("big_grid_points %zu %zu\n", big, grid_points(big, true));
    std::printf("big_grid_cells %zu %zu 1 1 %zu\n", hash_cap(big), big, grid_cells(hash_cap(big), big, true, true, true));
    const size_t big_aux = ((big + 255) / 256 + 1) * 64 + 512;
    std::printf("big_sor_stats %zu 1 %zu %zu %zu %zu\n", big, (big + 255) / 256, big_aux, JOB,
                sor_stats(big, 1, (big + 255) / 256, big_aux, JOB, true));
    if (g_failures) return 1;
    std::printf("OK\n");
    return 0;
}
