// lk_cell_grid.hpp - host side of the uniform cell grid over the sector centres (kernels: lk_reseed.hip, through
// lk_launch_reseed_grid), shared by every pass that looks for a sector's neighbours: the device buffers a grid needs and the
// rule that sizes it.  A part of lk_pass.hpp, which defines LkDevBytes and then includes this file: include that header.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "lk_device.hpp"
#include "lk_launch.hpp"

struct LkCellGridBufs { // (freed with their owner: LkDevBytes)
  LkDevBytes cell_of, start, cursor, unordered, members;
};

inline bool lk_cell_grid_bbox_finite(const float bbox[4]) {
  for (int i = 0; i < 4; ++i)
    if (!std::isfinite(bbox[i]))
      return false;
  return true;
}

// The cell grid over the centres, cell size = radius (a hair more, so that two centres within `radius` of each other
// are at most one cell apart whatever the rounding of the quotients).  A radius that is tiny against the domain would
// ask for more cells than there are sectors to put into them: the cells then grow (a larger cell only means more
// candidates per cell) until the table is a few words per sector.  bbox: finite {min x, min y, max x, max y} of the centres.
inline hipError_t lk_cell_grid_build(LkCellGridBufs &b, const float2 *center, int n_sectors, float radius, const float bbox[4],
                                     hipStream_t stream, LkReseedGrid *g) {
  const double w = (double)bbox[2] - (double)bbox[0], h = (double)bbox[3] - (double)bbox[1];
  const double limit = 4.0 * (double)n_sectors + 1024.0;
  double cell = (double)radius * (1.0 + 1e-6);
  double nx = std::floor(w / cell) + 1.0, ny = std::floor(h / cell) + 1.0;
  while (nx * ny > limit) {
    cell *= std::max(1.01, std::sqrt(nx * ny / limit));
    nx = std::floor(w / cell) + 1.0;
    ny = std::floor(h / cell) + 1.0;
  }
  g->x0 = (double)bbox[0];
  g->y0 = (double)bbox[1];
  g->cell = cell;
  g->nx = (int)nx;
  g->ny = (int)ny;
  const size_t n_cells = (size_t)g->nx * (size_t)g->ny, n = (size_t)n_sectors;
  hipError_t err;
  if ((err = b.cell_of.ensure(n * sizeof(uint32_t))) != hipSuccess || (err = b.unordered.ensure(n * sizeof(uint32_t))) != hipSuccess ||
      (err = b.members.ensure(n * sizeof(uint32_t))) != hipSuccess || (err = b.start.ensure((n_cells + 1) * sizeof(uint32_t))) != hipSuccess ||
      (err = b.cursor.ensure((n_cells + 1) * sizeof(uint32_t))) != hipSuccess)
    return err;
  err = lk_launch_reseed_grid(center, n_sectors, g->x0, g->y0, g->cell, g->nx, g->ny, b.cell_of.as<uint32_t>(),
                              b.start.as<uint32_t>(), b.cursor.as<uint32_t>(), b.unordered.as<uint32_t>(),
                              b.members.as<uint32_t>(), stream);
  g->start = b.start.as<uint32_t>();
  g->members = b.members.as<uint32_t>();
  g->cell_of = b.cell_of.as<uint32_t>();
  return err;
}
