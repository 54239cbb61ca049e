// mesh_components.h — the host helpers of mesh_components.hip that other mesh operators stand on (mesh_filter.hip).
#pragma once

#include "common.h"

namespace ot {

// bit width of the largest valid vertex index, n_vertices <= 2^31 - 1
int index_bits(int64_t n_vertices);

// the sizes every mesh entry refuses before any device work: negative, or 3 n_triangles / n_vertices beyond 31 bits
ot_status check_sizes(const char* who, int64_t n_triangles, int64_t n_vertices);

// any triangle index outside [0, n_vertices)?  "[who] triangle index out of range [0, n_vertices)".  Synchronises.
ot_status check_indices(const char* who, const int32_t* triangles, int64_t n_triangles, int64_t n_vertices,
                        hipStream_t stream);

// TriangleMesh::RemoveDuplicatedTriangles' mask of range-checked triangles: out_remove_mask[t] = 1 when an earlier
// triangle has the same canonical rotation.  Workspace: Slot::MCC_WS and the sort's; queued on the stream, no
// synchronisation.
ot_status flag_duplicated_triangles(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices,
                                    unsigned char* out_remove_mask, hipStream_t stream);

}  // namespace ot
