// The host side of the point-cloud world (mp_cloud.h): validation and the grid's image, built once for the kernels and the CPU
// twins alike (mp_collision_set_cloud hands the same bytes to both), and what a handle reports about its cloud.  Plain C++.
#include <cstring>

#include "mp_handles.h"

int mp_cloud_build(const char* fn, int64_t M, const double* points, double radius, double d_max, double cell,
                   std::vector<MpCloudPoint>* image) {
  REQUIRE(M >= 0, "%s: negative point count", fn);
  if (M == 0) {
    image->clear();
    return MP_OK;
  }
  REQUIRE(M <= MP_CLOUD_MAX_POINTS, "%s: %lld points, at most 2^24", fn, (long long)M);
  REQUIRE(points, "%s: null point array", fn);
  REQUIRE(std::isfinite(radius) && radius >= 0.0, "%s: radius must be finite and non-negative", fn);
  REQUIRE(std::isfinite(d_max) && d_max > 0.0, "%s: d_max must be positive and finite", fn);
  const double reach = d_max + radius;
  REQUIRE(std::isfinite(reach), "%s: d_max + radius must be finite", fn);
  if (!(cell > 0.0)) cell = reach;  // (a NaN cell: the default)
  REQUIRE(std::isfinite(cell), "%s: cell must be finite", fn);
  const double rings = std::ceil(reach / cell);
  REQUIRE(rings >= 1.0 && rings <= (double)MP_CLOUD_MAX_RING,
          "%s: ceil((d_max + radius) / cell) must be 1..4: cell between a quarter of d_max + radius = %g and any larger size", fn, reach);
  double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
  for (int64_t i = 0; i < M; ++i)
    for (int a = 0; a < 3; ++a) {
      const double v = points[3 * i + a];
      REQUIRE(std::isfinite(v), "%s: point %lld: non-finite coordinate", fn, (long long)i);
      lo[a] = v < lo[a] ? v : lo[a];
      hi[a] = v > hi[a] ? v : hi[a];
    }
  const double inv = 1.0 / cell;
  double total = 1.0;
  int dim[3];
  for (int a = 0; a < 3; ++a) {
    const double d = std::floor((hi[a] - lo[a]) * inv) + 1.0;
    REQUIRE(d <= (double)MP_CLOUD_MAX_CELLS, "%s: the grid would have more than 2^22 cells: raise cell", fn);
    dim[a] = (int)d;
    total *= d;
  }
  REQUIRE(total <= (double)MP_CLOUD_MAX_CELLS, "%s: the grid would have %.0f cells, more than 2^22: raise cell", fn, total);
  const int cells = (int)total;
  const size_t starts = (((size_t)cells + 1) * sizeof(int) + 31) / 32;  // in 32-byte units
  const size_t head = sizeof(MpColCloud) / 32;
  std::vector<MpCloudPoint> img(head + starts + (size_t)M);
  std::memset(static_cast<void*>(img.data()), 0, img.size() * sizeof(MpCloudPoint));
  MpColCloud H;
  std::memset(&H, 0, sizeof H);
  H.M = (int)M; H.R = (int)rings; H.cells = cells;
  H.pts_off = (unsigned)((head + starts) * 32);
  for (int a = 0; a < 3; ++a) { H.dim[a] = dim[a]; H.o[a] = lo[a]; }
  H.cell = cell; H.inv_cell = inv; H.r_c = radius; H.d_max = d_max;
  H.reach2 = reach * reach * (1.0 + 1e-9);
  H.slack = cell * 0x1p-20;
  std::memcpy(static_cast<void*>(img.data()), &H, sizeof H);
  int* start = reinterpret_cast<int*>(img.data() + head);
  MpCloudPoint* rec = img.data() + head + starts;
  // the counting sort: count per cell, prefix sums, then the records in the caller's order
  std::vector<int> where((size_t)M);
  for (int64_t i = 0; i < M; ++i) {
    int c[3];
    for (int a = 0; a < 3; ++a) {
      const double f = std::floor((points[3 * i + a] - lo[a]) * inv);
      c[a] = f < 0.0 ? 0 : (f > (double)(dim[a] - 1) ? dim[a] - 1 : (int)f);
    }
    where[(size_t)i] = (c[2] * dim[1] + c[1]) * dim[0] + c[0];
    start[where[(size_t)i] + 1] += 1;
  }
  for (int c = 0; c < cells; ++c) start[c + 1] += start[c];
  std::vector<int> fill(start, start + cells);
  for (int64_t i = 0; i < M; ++i) {
    MpCloudPoint& r = rec[fill[(size_t)where[(size_t)i]]++];
    r.x = points[3 * i]; r.y = points[3 * i + 1]; r.z = points[3 * i + 2];
    r.i = (int)i; r.pad = 0;
  }
  image->swap(img);
  return MP_OK;
}

extern "C" {

int mp_collision_cloud_info(const mp_collision* h, int64_t* M, double* radius, double* d_max, double* cell, int32_t* dims) {
  const char* fn = "mp_collision_cloud_info";
  REQUIRE(h, "%s: null collision handle", fn);
  MpColCloud H;
  std::memset(&H, 0, sizeof H);
  {
    std::lock_guard<std::mutex> hl(const_cast<mp_collision*>(h)->mu);
    if (!h->cloud.empty()) std::memcpy(&H, static_cast<const void*>(h->cloud.data()), sizeof H);
  }
  if (M) *M = H.M;
  if (radius) *radius = H.r_c;
  if (d_max) *d_max = H.d_max;
  if (cell) *cell = H.cell;
  if (dims) { dims[0] = H.dim[0]; dims[1] = H.dim[1]; dims[2] = H.dim[2]; }
  return MP_OK;
}

}  // extern "C"
