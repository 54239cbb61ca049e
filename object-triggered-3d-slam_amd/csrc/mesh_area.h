// mesh_area.h — the triangle area shared by the sampler (mesh_ops.hip) and the cluster areas (mesh_components.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ot {

// TriangleMesh::GetTriangleArea: 0.5 * |(p0 - p1) x (p0 - p2)|, Open3D's expression order
__device__ inline double tri_area(const double* __restrict__ V, const int32_t* __restrict__ T, int64_t t) {
    const double* p0 = V + (int64_t)T[t * 3] * 3;
    const double* p1 = V + (int64_t)T[t * 3 + 1] * 3;
    const double* p2 = V + (int64_t)T[t * 3 + 2] * 3;
    double x[3], y[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        x[d] = p0[d] - p1[d];
        y[d] = p0[d] - p2[d];
    }
    const double c0 = x[1] * y[2] - x[2] * y[1];
    const double c1 = x[2] * y[0] - x[0] * y[2];
    const double c2 = x[0] * y[1] - x[1] * y[0];
    return 0.5 * sqrt((c0 * c0 + c1 * c1) + c2 * c2);
}

}  // namespace ot
