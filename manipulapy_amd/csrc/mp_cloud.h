// Point-cloud world of the sphere collision model: M points with one radius r_c, truncated at d_max, queried through a uniform hash
// grid (the contract: include/manipula_hip.h, mp_collision_set_cloud).  Header-only like mp_collision.h, which includes it: the
// kernels (mp_kernels.hip) and the CPU twins (mp_cpu.cpp) instantiate the same query, the grid is built on the host by
// mp_cloud_build (mp_cloud_build.cpp) for both.
//
// One image, 32-byte aligned, the same bytes on the host and on the device:
//   +0        MpColCloud, 128 bytes: counts, the grid's origin / cell / dimensions, r_c, d_max
//   +128      cell_start[cells + 1] (int32): the records of cell c = (iz dim_y + iy) dim_x + ix are cell_start[c] .. cell_start[c + 1]
//   +pts_off  MpCloudPoint[M], 32 bytes each: x, y, z (float64) and the caller's index, sorted by cell (a counting sort: within a cell
//             in the caller's order, which the query does not rely on)
// The header is wave-uniform and read through the constant address space like the other tables; cells and records are per-lane
// gathers through plain global loads.
//
// The query for a point p: its cell, the (2 R + 1)^3 block of cells around it clamped to the grid (p outside the grid is handled by
// the clamp, the block may be empty), R = ceil((d_max + r_c) / cell) in 1..4.  A cell is skipped BEFORE any load when its box is farther
// than the running best (which starts at d_max + r_c); every record of a visited cell is one 32-byte load and three subtractions.
// Equal distances go to the lower caller index by an explicit test, so the result does not depend on the grid or the order of visits.
// Loop state: the best squared distance, its caller index and its record number - no array, nothing indexed at run time.
#pragma once

#include "mp_core.h"

constexpr int MP_CLOUD_MAX_POINTS = 1 << 24, MP_CLOUD_MAX_CELLS = 1 << 22, MP_CLOUD_MAX_RING = 4;

struct alignas(32) MpCloudPoint {
  double x, y, z;
  int i, pad;  // the caller's index
};
struct alignas(32) MpColCloud {
  int M, R, dim[3], cells;
  unsigned pts_off, pad;  // bytes from the header to the records
  double o[3], cell;      // the grid's origin (the points' lowest corner) and edge
  double inv_cell, r_c, d_max;
  double reach2;          // (d_max + r_c)^2 (1 + 1e-9): the prune of the search; the value is decided by d_max itself
  double slack;           // cell 2^-20: a cell's box is widened by it, so a record lies in its box whatever the rounding of the builder
  double pad2[3];
};
static_assert(sizeof(MpCloudPoint) == 32 && sizeof(MpColCloud) == 128, "the image's layout");

// pointer types of the three parts: plain on the host; in the kernels (mp_kernels.hip) constant / global address space
struct MpCloudPtrHost {
  typedef const MpColCloud* Header;
  typedef const int* Cells;
  typedef const MpCloudPoint* Points;
};

// the gap between p and the slab [lo - slack, hi + slack] of cell i along one axis (0 inside)
MP_HD double mp_cloud_gap(double p, double o, int i, double cell, double slack) {
  const double lo = o + (double)i * cell - slack, hi = lo + cell + 2.0 * slack;
  const double a = lo - p, b = p - hi;
  const double g = a > b ? a : b;
  return g > 0.0 ? g : 0.0;
}
// floor((p - o) / cell) as an int in [-(R + 1), dim + R]: whatever lies beyond sees the same cells as the bound does
MP_HD int mp_cloud_cell(double p, double o, double inv_cell, int dim, int R) {
  double f = __builtin_floor((p - o) * inv_cell);
  const double lo = (double)(-(R + 1)), hi = (double)(dim + R);
  f = f > lo ? f : lo;  // (a NaN p: lo)
  f = f < hi ? f : hi;
  return (int)f;
}

// sd = min(d_max, min_i |p - x_i| - r_c); who = the caller's index of the nearest point, M where the value is the truncated one;
// n = the unit vector from that point to p, 0 where truncated or coincident (`tiny`: MP_COL_TINY)
template <typename PT>
MP_HD void mp_cloud_distance(const MpColCloud* cloud, double px, double py, double pz, double tiny, double& sd, double& nx, double& ny,
                             double& nz, int& who) {
  const typename PT::Header h = (typename PT::Header)cloud;
  const typename PT::Cells cs = (typename PT::Cells)((const char*)cloud + sizeof(MpColCloud));
  const typename PT::Points pts = (typename PT::Points)((const char*)cloud + h->pts_off);
  const int R = h->R, dx_ = h->dim[0], dy_ = h->dim[1], dz_ = h->dim[2];
  const double ox = h->o[0], oy = h->o[1], oz = h->o[2], cell = h->cell, inv = h->inv_cell, slack = h->slack;
  const int cx = mp_cloud_cell(px, ox, inv, dx_, R), cy = mp_cloud_cell(py, oy, inv, dy_, R), cz = mp_cloud_cell(pz, oz, inv, dz_, R);
  const int x0 = cx - R > 0 ? cx - R : 0, x1 = cx + R < dx_ - 1 ? cx + R : dx_ - 1;
  const int y0 = cy - R > 0 ? cy - R : 0, y1 = cy + R < dy_ - 1 ? cy + R : dy_ - 1;
  const int z0 = cz - R > 0 ? cz - R : 0, z1 = cz + R < dz_ - 1 ? cz + R : dz_ - 1;
  const double shrink = 1.0 - 0x1p-40;  // the box's squared distance is compared a few ulp low: rounding never skips a holder of the minimum
  double best2 = h->reach2;
  int best_i = 0x7fffffff, best_k = -1;
  for (int iz = z0; iz <= z1; ++iz) {
    const double ez = mp_cloud_gap(pz, oz, iz, cell, slack);
    for (int iy = y0; iy <= y1; ++iy) {
      const double ey = mp_cloud_gap(py, oy, iy, cell, slack);
      const double eyz = ey * ey + ez * ez;
      if (eyz * shrink > best2) continue;
      const int row = (iz * dy_ + iy) * dx_;
      for (int ix = x0; ix <= x1; ++ix) {
        const double ex = mp_cloud_gap(px, ox, ix, cell, slack);
        if ((ex * ex + eyz) * shrink > best2) continue;
        const int k1 = cs[row + ix + 1];
        for (int k = cs[row + ix]; k < k1; ++k) {
          const double ax = px - pts[k].x, ay = py - pts[k].y, az = pz - pts[k].z;  // (members, not a copy: the record's address space)
          const int ri = pts[k].i;
          const double d2 = ax * ax + ay * ay + az * az;
          if (d2 < best2 || (d2 == best2 && ri < best_i)) { best2 = d2; best_i = ri; best_k = k; }
        }
      }
    }
  }
  sd = h->d_max; who = h->M;
  nx = 0.0; ny = 0.0; nz = 0.0;
  if (best_k >= 0) {
    const double dist = mp_sqrt(best2);
    const double m = dist - h->r_c;
    if (m <= h->d_max) {  // equal: the point, the truncated value comes last
      const double iv = dist < tiny ? 0.0 : 1.0 / dist;
      sd = m; who = best_i;
      nx = (px - pts[best_k].x) * iv; ny = (py - pts[best_k].y) * iv; nz = (pz - pts[best_k].z) * iv;
    }
  }
}
