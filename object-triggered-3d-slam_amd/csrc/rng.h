// rng.h — the counter RNG shared by the mesh sampler (mesh_ops.hip) and the RANSAC sampler (segment_plane.hip).
//
// Open3D's samplers are unseeded (std::random_device), so this build draws from a counter RNG instead: word `ctr` of
// stream `seed` is splitmix64's output for the state seed + (ctr + 1) * 0x9E3779B97F4A7C15.  Any lane can form any
// draw on its own, and the numpy restatements in tests/ form the same words.
#pragma once

namespace ot {

__host__ __device__ inline unsigned long long rng_word(unsigned long long seed, unsigned long long ctr) {
    unsigned long long z = seed + (ctr + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// uniform in [0, 1): the word's top 53 bits
__host__ __device__ inline double rng_u01(unsigned long long seed, unsigned long long ctr) {
    return (double)(rng_word(seed, ctr) >> 11) * (1.0 / 9007199254740992.0);
}

}  // namespace ot
