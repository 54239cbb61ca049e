// scan.h — LaserScan beam helpers shared by change.hip (scan diff) and scan_cluster.hip (clustering, object filter).
#pragma once

#include "common.h"

namespace ot {

struct ScanPose {
    double tx, ty, cyaw, syaw;  // translation and cos / sin of the map-frame yaw (host-computed)
};

// beam endpoint in the sensor frame, float as the reference: r * std::cos(angle), angle = angle_min + i * inc.
// The per-beam cos / sin tables are computed on the host with the same libm float functions the node calls
// (glibc cosf / sinf are not correctly rounded, so a device-side evaluation would differ in the last ulp).
__device__ inline void beam_xy(float r, const float2* __restrict__ cs, int i, float& x, float& y) {
    const float2 c = cs[i];
    x = r * c.x;
    y = r * c.y;
}

// hypotf(dx, dy) as glibc computes it: sqrt of the double sum of double squares, rounded to float
__device__ inline float hypot_f(float dx, float dy) {
    const double x = dx, y = dy;
    return (float)sqrt(x * x + y * y);
}

}  // namespace ot
