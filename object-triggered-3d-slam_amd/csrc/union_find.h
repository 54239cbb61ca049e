// union_find.h — lock-free union-find over an int parent[] array in global memory (cluster.hip's DBSCAN hook,
// mesh_components.hip's edge hook).  The larger root is hooked under the smaller by compare-and-swap, so parent[x] <= x
// always, every find is a walk of at most x steps whatever other lanes do, and a failed compare-and-swap means another
// lane's hook succeeded.  No lane waits for another.  The root of a finished component is its smallest element whatever
// the interleaving.  Every access to parent[] while hooks run is a relaxed agent-scope atomic (other workgroups, on
// other XCDs, write it).
#pragma once

#include <hip/hip_runtime.h>

namespace ot {

__device__ inline int uf_load(int* parent, int x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// parent[x] <= x, and < x for every hooked x: the walk strictly descends, so it ends after at most x steps
__device__ inline int uf_find(int* parent, int x) {
    int p = uf_load(parent, x);
    while (p != x) {
        x = p;
        p = uf_load(parent, x);
    }
    return x;
}
// unite the sets of a and b; returns the root both now share (as far as this lane has seen)
__device__ inline int uf_union(int* parent, int a, int b) {
    while (true) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return a;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        int expect = a;  // a > b: hook root a under b, unless another lane hooked a first (then start again from a)
        if (__hip_atomic_compare_exchange_strong(parent + a, &expect, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return b;
    }
}

}  // namespace ot
