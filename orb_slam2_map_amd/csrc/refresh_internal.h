// What orbgpu_mappoint_table_refresh (map_table.hip) hands to the refresh query of the observation graph (covis.hip).
#pragma once

#include "orbgpu.h"

#include <cstdint>
#include <vector>

namespace orbgpu {

// The table side of a refresh: device arrays, entry i for the caller's i-th id.
struct RefreshTableIO {
    const float *pos;     // [n][3] the row's world position (unread where pre[i] != 0)
    const uint8_t *pre;   // [n] ORBGPU_REFRESH_UNKNOWN / ORBGPU_REFRESH_BAD, 0: refresh
    const int32_t *row;   // [n] the table row the results go to (unread where pre[i] != 0)
    float *normal, *min_dist, *max_dist;  // the table's columns
    uint8_t *desc;
};

// Every refusal of orbgpu_covis_refresh_points that does not concern world_pos; no device is touched.  perm: the ids in
// ascending order as positions in mp_ids -- the call's one sort, which also finds a repeated id.
int covis_refresh_check(const orbgpu_covis_graph *g, int32_t n, const int64_t *mp_ids, const int64_t *ref_kf_ids, uint32_t what,
                        const int32_t *n_slots, const uint8_t *status, const orbgpu_covis_refresh_result *res,
                        std::vector<int32_t> &perm);
int covis_refresh_device_id(const orbgpu_covis_graph *g);

// The query after covis_refresh_check.  tio == nullptr: positions from world_pos (host).  Otherwise world_pos is not read,
// and the kernels also write into the table's rows.  Returns synchronised.
int covis_refresh_run(orbgpu_covis_graph *g, int32_t n, const int64_t *mp_ids, const int64_t *ref_kf_ids, const float *world_pos,
                      uint32_t what, float *normal, float *min_dist, float *max_dist, uint8_t *desc, int64_t *desc_kf,
                      int32_t *desc_idx, int32_t *n_slots, uint8_t *status, orbgpu_covis_refresh_result *res,
                      const std::vector<int32_t> &perm, const RefreshTableIO *tio);

}  // namespace orbgpu
