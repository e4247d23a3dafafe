// launch_geometry.hip -- pnr_launch_geometry: what grid a capped-grid entry launches for a batch, asked of the translation unit that owns the
// entry.  Host code only: each *_launch_geometry (pnr_common.hpp) calls the helper its launcher forms the grid with, so the answer cannot drift
// from the launch.  A test that wants rows on a workgroup's second trip through its tile loop takes the batch from here instead of a constant.
#include "pnr_common.hpp"

using namespace pnr;

extern "C" {

int pnr_launch_geometry(const char* entry, uint64_t rows, uint32_t* workgroups, uint32_t* rows_per_trip) {
    if (!entry || !workgroups || !rows_per_trip) return PNR_ERR_INVALID;
    for (auto unit : {heads_launch_geometry, smooth_launch_geometry, shade_launch_geometry, field_launch_geometry, mlp_launch_geometry, occupancy_launch_geometry,
                      extract_launch_geometry, lut_launch_geometry})
        if (unit(entry, rows, workgroups, rows_per_trip) == PNR_OK) return PNR_OK;
    return PNR_ERR_INVALID;
}

}  // extern "C"
