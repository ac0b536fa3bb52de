// pp_box_geom.h -- the car-space box geometry shared by the training augmentation (pp_augment.hip) and the
// ground-truth paste (pp_paste.hip): a footprint, the collision rule of two footprints, and a box as the
// point-in-box test reads it.  All f64, every product and sum rounded separately (the including file sets
// `#pragma clang fp contract(off)` before it includes this header).
#pragma once

#include "pp_common.h"

#pragma clang fp contract(off)

namespace pp {

constexpr int kAugMaxBoxes = 1024;   // boxes per sample: their footprints live in LDS
constexpr double kAugParked = -1e6;  // canvas-space x, y of a box the target kernels are to drop

// A footprint in LDS: centre, half length (along the yaw direction), half width, cosine and sine of the yaw.
struct Rect {
  double x, y, hl, hw, c, s;
};

// The largest separation of two rectangles over their four edge directions: > 0 iff the projection
// intervals are strictly disjoint along one of them.  NaN compares false: it collides.
__device__ __forceinline__ bool rects_separated(const Rect &a, const Rect &b) {
  const double dx = b.x - a.x, dy = b.y - a.y;
  const double cc = fabs(a.c * b.c + a.s * b.s), ss = fabs(a.c * b.s - a.s * b.c);
  const double s1 = fabs(dx * a.c + dy * a.s) - (a.hl + (b.hl * cc + b.hw * ss));
  const double s2 = fabs(dy * a.c - dx * a.s) - (a.hw + (b.hl * ss + b.hw * cc));
  const double s3 = fabs(dx * b.c + dy * b.s) - (b.hl + (a.hl * cc + a.hw * ss));
  const double s4 = fabs(dy * b.c - dx * b.s) - (b.hw + (a.hl * ss + a.hw * cc));
  return s1 > 0.0 || s2 > 0.0 || s3 > 0.0 || s4 > 0.0;
}

// A box in car space as the point-in-box test reads it: centre, half extents, cosine and sine of the yaw.
struct OwnerBox {
  double x, y, z, hl, hw, hh, c, s;
};

}  // namespace pp
