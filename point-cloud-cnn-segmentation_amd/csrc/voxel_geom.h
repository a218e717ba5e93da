// The geometry of the voxel grid, shared by every file that quantises a point (voxel.hip,
// sparse.hip, pointvoxel.hip): the bounding box, the one expression of a point's voxel id (the ids
// and keys of these files are bit-exact with each other because there is no second one), and the
// grid of their one-thread-per-item kernels.
#pragma once
#include "common.h"

namespace pcs_geom {

struct Box {
  float lo[3], hi[3];
};

// (ix * G + iy) * G + iz, i_d = clamp(floor((p_d - lo_d) / (hi_d - lo_d) * G), 0, G - 1): fp32, IEEE
// division and multiply in this order (bit-exact with numpy float32)
PCS_DEV int64_t voxel_of(const float *p, int G, const Box &b) {
  int64_t id = 0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float t = (p[d] - b.lo[d]) / (b.hi[d] - b.lo[d]);
    int i = (int)floorf(t * (float)G);
    i = i < 0 ? 0 : (i > G - 1 ? G - 1 : i);
    id = id * G + i;
  }
  return id;
}

// blocks of 256 threads for n items walked with a grid stride: at least 1, at most 8192
inline int blocks_1d(int64_t n) { return (int)pcs_max64(1, pcs_min64(8192, (n + 255) / 256)); }

}  // namespace pcs_geom
