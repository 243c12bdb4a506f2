// The nearest-neighbour index as its kernels read it (nn.hip), and what capi.hip calls: the plan itself is host logic and
// lives in capi.hip with the other argument checks.
#pragma once
#include "common.hpp"

namespace miso {

struct NnK {
  float lo[3];      // bound_min
  float cell;       // the cell actually used
  float mag;        // miso_nn_plan_t.coord_mag: the coordinate magnitude the stop test's slack scales with
  int dims[3];
  int max_rings;
  int64_t n_tgt;
};

}  // namespace miso
