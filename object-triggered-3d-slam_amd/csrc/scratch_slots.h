// scratch_slots.h — who owns which buffer of the scratch arenas (common.h: scratch / pinned_scratch).
//
// A slot is one grow-only buffer per host thread and device; growing it frees the old one.  So two users may share a
// slot only when neither needs its contents across a call of the other, and a helper that takes workspace of its own
// names a slot no caller of it holds live data in.  This file is the only place that says who owns what: one name per
// buffer, the sharers listed where a buffer is shared on purpose.  New workspace gets a new name before COUNT.
#pragma once

namespace ot {

enum class Slot : int {
    // image_ops.hip: block counts of its three compactions
    IMG_UNPROJECT_COMPACT,
    IMG_MIN_Z_COMPACT,
    IMG_OCCUPANCY_COMPACT,
    // sort.hip: the temporaries of every sort of the library (shared by all callers of sort.h: a sort's temporaries
    // are dead when it returns)
    SORT_TMP,
    // tsdf_exchange.hip: keys / values of the unit sort
    TSDF_UNIT_SORT,
    // voxel.hip: bounds, keys, values, heads of ot_voxel_down_sample
    VOXEL_WS,
    // voxel-head compaction block counts (voxel.hip) and the batch filter's head counts and head compactions
    // (filter_batch.hip); shared: each is consumed before its call returns
    VOXEL_HEADS,
    // grid.hip bounds_host: the bounds record and the per-block partials
    BOUNDS,
    BOUNDS_PARTIALS,
    // op-level workspace of the operators that stand on the cloud grid; shared (an operator's workspace is dead when
    // it returns, and neither bounds_host nor the grid builders use it): ROR keep flags and SOR stats + avg
    // (outlier.hip), normals' covariances (normals.hip), DBSCAN's tables (cluster.hip)
    OP_WS,
    // block counts of the compaction that ends an operator; shared (consumed inside compact()): outlier.hip,
    // filter_batch.hip, cluster.hip, icp.hip, segment_plane.hip, tsdf_exchange.hip
    OP_COMPACT,
    // vertex-normal workspace (mesh_ops.hip) and the owned-unit list (tsdf_exchange.hip); shared: neither calls the
    // other
    MESH_NORMALS_WS,
    // mesh_ops.hip: sampler tables and chain-sum workspaces (one pending sampling per thread)
    MESH_SAMPLE_WS,
    // voxel.hip: bounds partials
    VOXEL_BOUNDS_PARTIALS,
    // grid.hip single_frame_grid: device origin and frame offsets {0, n}
    CLOUD_FRAME,
    // the cloud grid (grid.hip single_frame_grid): sorted points and keys, cell-head compaction, hash + cell tables
    CLOUD_GRID_POINTS,
    CLOUD_GRID_COMPACT,
    CLOUD_GRID_CELLS,
    // the batch filter's grid over all frames' voxels (filter_batch.hip): the same three
    BATCH_GRID_POINTS,
    BATCH_GRID_COMPACT,
    BATCH_GRID_CELLS,
    // the batch filter's SOR: statistics workspace, pending lists
    BATCH_SOR_STATS,
    BATCH_SOR_PENDING,
    // change.hip
    CHG_PASTE_COUNT,   // smart paste: changed-cell counter
    CHG_UNIQ_NEW,      // unique keys of the new cloud
    CHG_UNIQ_OLD,      // unique keys of the old cloud
    CHG_KEYS_WS,       // unique_keys / unique_obj_keys: keys and values of the sort
    CHG_KEYS_COMPACT,  // ... and the block counts of their unique compaction
    CHG_ADDED_COMPACT,
    CHG_REMOVED_COMPACT,
    CHG_BOUNDS_POSES,  // object diff: lattice bounds; scan diff: scan poses (shared: different entry points)
    CHG_SCAN_CS,
    CHG_GOAL_CS,
    CHG_GOAL_ROBOT,
    // the cloud SOR (outlier.hip): statistics workspace, pending lists
    CLOUD_SOR_STATS,
    CLOUD_SOR_PENDING,
    // icp.hip
    ICP_PCD,
    ICP_NN,
    ICP_PARTIALS,
    // scan_cluster.hip
    SCAN_CS,
    SCAN_POSE,
    SCAN_RAW,
    SCAN_POS,
    SCAN_COUNTS,
    SCAN_OFFSETS,
    SCAN_COMPACT,
    // mesh_components.hip
    MCC_WS,
    MCC_COMPACT,
    MCC_BAD,  // the refusal word of check_indices; shared with mesh_filter.hip's CSR check (each reads it back at once)
    // segment_plane.hip
    SP_CANDIDATES,
    SP_TIES,
    SP_FINAL,
    // mesh_filter.hip
    MF_WS,               // adjacency: keys / values of the sort; clustering: bounds, sort, heads, rows, mapped triangles
    MF_COMPACT,          // block counts of its compactions (consumed inside compact())
    MF_BOUNDS_PARTIALS,  // clustering: bounds partials
    MF_PING,             // filters: the second buffer of the ping-pong
    // features.hip
    FEAT_LISTS,    // FPFH: per point the neighbour list (length, indices, d2), read by the SPFH and the FPFH kernel
    FEAT_SPFH,     // FPFH: the SPFH rows when the caller does not ask for them
    FEAT_MATCH,    // matching: the per-split (d2, index) minima and the two match tables
    FEAT_COMPACT,  // matching: block counts of the mutual filter's compaction (consumed inside compact())
    COUNT
};

// pinned host memory: an arena of its own
enum class PinnedSlot : int {
    MESH_SAMPLE_UPLOAD,  // mesh_ops.hip: the sampler's job tables on their way to the device
    MESH_SAMPLE_KEPT,    // mesh_ops.hip: the fused sampler's kept counts (coherent)
    ICP_MAIL,            // icp.hip: the iteration mailboxes (coherent)
    SP_MAIL,             // segment_plane.hip: the candidates' scores (coherent)
    COUNT
};

// the buffers a neighbour-grid build cuts its tables from (grid.h)
struct GridSlots {
    Slot points, compact, cells;
};
constexpr GridSlots CLOUD_GRID_SLOTS{Slot::CLOUD_GRID_POINTS, Slot::CLOUD_GRID_COMPACT, Slot::CLOUD_GRID_CELLS};
constexpr GridSlots BATCH_GRID_SLOTS{Slot::BATCH_GRID_POINTS, Slot::BATCH_GRID_COMPACT, Slot::BATCH_GRID_CELLS};

// the buffers of a SOR over a built grid (sor.h)
struct SorSlots {
    Slot stats, pending;
};
constexpr SorSlots CLOUD_SOR_SLOTS{Slot::CLOUD_SOR_STATS, Slot::CLOUD_SOR_PENDING};
constexpr SorSlots BATCH_SOR_SLOTS{Slot::BATCH_SOR_STATS, Slot::BATCH_SOR_PENDING};

}  // namespace ot
