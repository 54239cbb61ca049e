// Host check of csrc/slice_pretest.h against brute force (built and run by tests/test_slice_pretest_bound.py).
//
//   slice_pretest_check <cases.bin>
//
// cases.bin (little endian), repeated until the end of the file:
//   int32 W, H; float fx, fy, cx, cy; float vl; double unit_len; float trunc; int32 n_units
//   float E[12]                      rows 0..2 of (float)extrinsic
//   float depth[H][W]                the staged depth (what the integrate gathers)
//   int32 keys[n_units][3]
// Per case one line: "<wave-frames> <dropped by the header> <idle by brute force> <dropped with a candidate>".
// Brute force: all 256 voxel centres of a slice taken through the integrate's own float32 steps (position, rows of E,
// the z walk by repeated adds, Open3D's projection and bounds, the candidate test on d - z).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "slice_pretest.h"

namespace {

struct Case {
    int32_t W, H;
    float fx, fy, cx, cy, vl;
    double unit_len;
    float trunc;
    int32_t n_units;
    float E[12];
    std::vector<float> depth;
    std::vector<int32_t> keys;
};

template <class T>
bool rd(FILE* f, T* p, size_t n = 1) {
    return fread(p, sizeof(T), n, f) == n;
}

bool read_case(FILE* f, Case& c) {
    if (!rd(f, &c.W)) return false;
    bool ok = rd(f, &c.H) && rd(f, &c.fx) && rd(f, &c.fy) && rd(f, &c.cx) && rd(f, &c.cy) && rd(f, &c.vl) &&
              rd(f, &c.unit_len) && rd(f, &c.trunc) && rd(f, &c.n_units) && rd(f, c.E, 12);
    if (!ok || c.W <= 0 || c.H <= 0 || c.n_units < 0) return false;
    c.depth.resize((size_t)c.W * c.H);
    c.keys.resize((size_t)c.n_units * 3);
    return rd(f, c.depth.data(), c.depth.size()) && (c.n_units == 0 || rd(f, c.keys.data(), c.keys.size()));
}

// does any voxel of slice s of the unit pass the integrate's candidate test?
bool brute_live(const Case& c, const int32_t* key, int s) {
    const float half = c.vl * 0.5f;
    const float safe_w = (float)c.W - 0.0001f, safe_h = (float)c.H - 0.0001f;
    const float ox = (float)((double)key[0] * c.unit_len);
    const float oy = (float)((double)key[1] * c.unit_len);
    const float oz = (float)((double)key[2] * c.unit_len);
    const float es[3] = {c.E[2] * c.vl, c.E[6] * c.vl, c.E[10] * c.vl};
    const int x0 = (s & 2) * 4, y0 = (s & 1) * 8, z0 = (s >> 2) * 4;
    for (int x = x0; x < x0 + 8; ++x)
        for (int y = y0; y < y0 + 8; ++y) {
            const float px = (half + c.vl * (float)x) + ox;
            const float py = (half + c.vl * (float)y) + oy;
            const float pz = half + oz;
            float pc[3];
            for (int r = 0; r < 3; ++r) {
                const float a = c.E[r * 4 + 0] * px, b = c.E[r * 4 + 1] * py, cc = c.E[r * 4 + 2] * pz;
                pc[r] = ((a + b) + cc) + c.E[r * 4 + 3];
            }
            for (int z = 0; z < z0 + 4; ++z) {
                if (z >= z0 && pc[2] > 0.0f) {
                    const float u = ((pc[0] * c.fx) / pc[2] + c.cx) + 0.5f;
                    const float v = ((pc[1] * c.fy) / pc[2] + c.cy) + 0.5f;
                    if (u >= 0.0001f && u < safe_w && v >= 0.0001f && v < safe_h) {
                        const float d = c.depth[(size_t)(int)v * c.W + (int)u];
                        if (d > 0.0f && d - pc[2] > -c.trunc) return true;
                    }
                }
                pc[0] += es[0], pc[1] += es[1], pc[2] += es[2];
            }
        }
    return false;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    Case c;
    while (read_case(f, c)) {
        const int tmx = ot::pre_tiles(c.W), tmy = ot::pre_tiles(c.H);
        std::vector<uint32_t> map((size_t)tmx * tmy, 0u);
        for (int y = 0; y < c.H; ++y)
            for (int x = 0; x < c.W; ++x) {
                uint32_t& m = map[(size_t)(y / ot::PRE_TILE) * tmx + x / ot::PRE_TILE];
                const uint32_t k = ot::pre_depth_key(c.depth[(size_t)y * c.W + x]);
                m = k > m ? k : m;
            }
        ot::PreIntrinsics in{c.W, c.H, c.fx, c.fy, c.cx, c.cy};
        long long total = 0, dropped = 0, idle = 0, wrong = 0;
        for (int u = 0; u < c.n_units; ++u)
            for (int s = 0; s < 16; ++s) {
                const int32_t* key = &c.keys[(size_t)u * 3];
                const bool drop = ot::slice_idle(c.E, in, c.vl, c.unit_len, key[0], key[1], key[2], s, c.trunc,
                                                 [&](int i) {  // past the map: another frame's tiles or slack
                                                     ot::PreTile4 q;
                                                     for (int j = 0; j < 4; ++j)
                                                         q.k[j] = i >= ot::PRE_NONE           ? 0u
                                                                  : i + j < tmx * tmy ? map[i + j]
                                                                                      : 0x7F000000u + (uint32_t)j;
                                                     return q;
                                                 });
                const bool live = brute_live(c, key, s);
                ++total;
                dropped += drop;
                idle += !live;
                wrong += drop && live;
            }
        printf("%lld %lld %lld %lld\n", total, dropped, idle, wrong);
    }
    fclose(f);
    return 0;
}
