// gps_box_dev.h -- the axis-aligned box and box3d_iou of the ScanRefer target path, stated once for gps_refer.hip
// (gps_refer_targets) and gps_obj_select_pred.hip (gps_proposal_labels, gps_obj_select_pred).  Every translation unit
// that includes this file is compiled with -ffp-contract=off (csrc/build.py): the results are pinned bit for bit to
// box3d_iou (data/data_utils.py:212-234) on construct_bbox_corners' corners (:266-277, get_box3d_min_max :194-209).
#pragma once
#include <hip/hip_runtime.h>

namespace gps_box {

struct Box {
  double lo[3], hi[3], vol;
  // construct_bbox_corners + get_box3d_min_max: the corners are c + s/2 and c + (-(s/2)); s >= 0
  __device__ __forceinline__ void load(const double *__restrict__ b) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double h = b[3 + c] / 2.0;
      lo[c] = b[c] + (-h);
      hi[c] = b[c] + h;
    }
    vol = ((hi[0] - lo[0]) * (hi[1] - lo[1])) * (hi[2] - lo[2]);
  }
};

// box3d_iou, data/data_utils.py:221-232, in its own order of operations (compiled without contraction)
__device__ __forceinline__ double iou(const Box &a, const Box &b) {
  const double dx = fmin(a.hi[0], b.hi[0]) - fmax(a.lo[0], b.lo[0]);
  const double dy = fmin(a.hi[1], b.hi[1]) - fmax(a.lo[1], b.lo[1]);
  const double dz = fmin(a.hi[2], b.hi[2]) - fmax(a.lo[2], b.lo[2]);
  const double inter = (fmax(dx, 0.0) * fmax(dy, 0.0)) * fmax(dz, 0.0);
  return inter / (((a.vol + b.vol) - inter) + 1e-8);
}

}  // namespace gps_box
