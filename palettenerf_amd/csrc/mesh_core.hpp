// mesh_core.hpp -- the density lattice of the mesh export (include/pnr.h, "mesh export"): one statement of the coordinate formula for every
// kernel that forms lattice points (mesh.hip: pnr_lattice_points).
#pragma once
#include "pnr_common.hpp"

namespace pnr {

constexpr uint32_t kLatticeMaxAxis = 512;

struct LatticeGeom {
    uint32_t n[3];
    float lo[3], hi[3], step[3];      // step = (hi - lo) / (n - 1), formed in fp32 on the host
};

inline bool make_lattice(const float* box_min, const float* box_max, const uint32_t* n, LatticeGeom* g) {
    if (!box_min || !box_max || !n) return false;
    for (int d = 0; d < 3; d++) {
        if (n[d] < 2 || n[d] > kLatticeMaxAxis) return false;
        g->n[d] = n[d]; g->lo[d] = box_min[d]; g->hi[d] = box_max[d];
        g->step[d] = (box_max[d] - box_min[d]) / (float)(n[d] - 1);
    }
    return true;
}
inline uint64_t lattice_total(const LatticeGeom& g) { return (uint64_t)g.n[0] * g.n[1] * g.n[2]; }

// torch.linspace's two-sided form (nerf/utils.py:189-191): the lower half steps up from min, the upper half down from max; a product and a
// sum, each rounded (the translation units are built without contraction).  i = n - 1 is exactly max.
__device__ __forceinline__ float lattice_coord(const LatticeGeom& g, int d, uint32_t i) {
    return i < g.n[d] / 2 ? g.lo[d] + g.step[d] * (float)i : g.hi[d] - g.step[d] * (float)(g.n[d] - 1 - i);
}
// lattice index (C order, z fastest) -> point
__device__ __forceinline__ void lattice_point(const LatticeGeom& g, uint32_t idx, float (&p)[3]) {
    const uint32_t z = idx % g.n[2], xy = idx / g.n[2];
    p[0] = lattice_coord(g, 0, xy / g.n[1]); p[1] = lattice_coord(g, 1, xy % g.n[1]); p[2] = lattice_coord(g, 2, z);
}

}  // namespace pnr
