// lk_neighbours.hpp - device side of the passes that look for a position's neighbours on the cell grid over the sector
// centres (lk_reseed.hip, lk_strain.hip, lk_outlier.hip, lk_track.hip, lk_field.hip, the residual map of lk_residual.hip): the good rule
// of a record, the cell of a position, the 3 x 3 cells around it, the walk of their members by a lane group, and the sums
// of the windowed plane fit.  The device half of lk_pass.hpp; light on purpose - nothing of the solve (lk_solver_common.hpp)
// comes with it.  A new neighbour pass starts here ("adding a pass").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lk_engine.h"
#include "lk_device.hpp"

namespace {

constexpr int kBlock = 256; // threads of a workgroup of every pass kernel

inline unsigned blocks_for(long long n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// ---- the good rule -------------------------------------------------------------------------------------------------------
__device__ inline bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// include/lk_engine.h, "good": error_none, finite parameters and chi, chi <= chi_max when chi_max > 0
__device__ inline bool reseed_good(const lk_result &r, int n_params, float chi_max) {
  if (r.errorCode != LK_ERROR_NONE || !finite_bits(r.chi))
    return false;
  for (int i = 0; i < n_params; ++i)
    if (!finite_bits(r.resultingParameters[i]))
      return false;
  return !(chi_max > 0.f) || r.chi <= chi_max;
}

__device__ inline int n_params_of(int model) {
  return model == LK_FM_U ? 1 : model == LK_FM_UV ? 2 : model == LK_FM_UVQ ? 3 : 6;
}

// ---- cells ---------------------------------------------------------------------------------------------------------------
// the cell coordinate of a centre: inside the grid whatever the rounding (a NaN lands in cell 0)
__device__ inline int cell_coord(double v, double origin, double cell, int n) {
  const double q = floor((v - origin) / cell);
  return q >= (double)(n - 1) ? n - 1 : (q > 0.0 ? (int)q : 0);
}

// the cell coordinate of a free position: the same expression, clamped to [-2, n + 1].  -1 and n are one cell beyond the
// grid, whose 3-cell range still reaches the grid's edge cells; -2 and n + 1 stand for everything farther out: more than
// a cell (>= radius) from every centre, their range is empty
__device__ inline int free_cell_coord(double v, double origin, double cell, int n) {
  const double q = floor((v - origin) / cell);
  return q >= (double)(n + 1) ? n + 1 : (q > -2.0 ? (int)q : -2);
}

struct CellRange { // cells x_lo .. x_hi of the rows y_lo .. y_hi, inside the grid; y_lo > y_hi: no cell at all
  int x_lo, x_hi, y_lo, y_hi;
};

// the cells within one cell of the cells ix_lo .. ix_hi x iy_lo .. iy_hi (coordinates of cell_coord or free_cell_coord);
// a rectangle two or more cells beyond the grid - in x or in y - has none
__device__ inline CellRange cell_range(const LkReseedGrid &g, int ix_lo, int ix_hi, int iy_lo, int iy_hi) {
  CellRange r;
  r.x_lo = ix_lo > 0 ? ix_lo - 1 : 0, r.x_hi = ix_hi + 1 < g.nx ? ix_hi + 1 : g.nx - 1;
  r.y_lo = iy_lo > 0 ? iy_lo - 1 : 0, r.y_hi = iy_hi + 1 < g.ny ? iy_hi + 1 : g.ny - 1;
  if (r.x_lo > r.x_hi)
    r.y_hi = r.y_lo - 1;
  return r;
}
__device__ inline CellRange cell_range(const LkReseedGrid &g, int ix, int iy) { return cell_range(g, ix, ix, iy, iy); }
// ... around the cell of sector s
__device__ inline CellRange cell_range_of(const LkReseedGrid &g, int s) {
  const int cell = (int)g.cell_of[s];
  return cell_range(g, cell % g.nx, cell / g.nx);
}

// ---- the walk ------------------------------------------------------------------------------------------------------------
// The rows of a range in order: f(b, e), the entries [b, e) of the member table that hold the cells x_lo .. x_hi of a row
// (neighbours in memory), e clipped to the table's S entries; b >= e: nothing.
template <class F> __device__ inline void cell_rows(const LkReseedGrid &g, const CellRange &r, uint32_t S, F f) {
  for (int yy = r.y_lo; yy <= r.y_hi; ++yy) {
    const uint32_t b = g.start[(size_t)yy * (size_t)g.nx + (size_t)r.x_lo];
    uint32_t e = g.start[(size_t)yy * (size_t)g.nx + (size_t)r.x_hi + 1];
    e = e < S ? e : S;
    f(b, e);
  }
}

// the entries of a range
__device__ inline long long cell_range_entries(const LkReseedGrid &g, const CellRange &r, uint32_t S) {
  long long total = 0;
  cell_rows(g, r, S, [&](uint32_t b, uint32_t e) { total += e > b ? (long long)(e - b) : 0; });
  return total;
}

// Lane `lane` of GROUP takes the entries b + lane, b + lane + GROUP, ... of every row: f(at, m), the at-th entry of the
// range (rows concatenated, at < cell_range_entries) and the sector m it names.  m is what the table holds: the caller
// checks m < S before it indexes with it.
template <int GROUP, class F>
__device__ inline void walk_entries(const LkReseedGrid &g, const CellRange &r, uint32_t S, int lane, F f) {
  uint32_t base = 0;
  cell_rows(g, r, S, [&](uint32_t b, uint32_t e) {
    for (uint32_t k = b + (uint32_t)lane; k < e; k += GROUP)
      f(base + (k - b), g.members[k]);
    base += e > b ? e - b : 0;
  });
}

// The walk of a lane group: the members of a range dealt to GROUP lanes, f(m) for every sector m < S this lane is dealt.
// GROUP = 1, lane = 0: one lane visits them all.
template <int GROUP, class F>
__device__ inline void walk_members(const LkReseedGrid &g, const CellRange &r, uint32_t S, int lane, F f) {
  walk_entries<GROUP>(g, r, S, lane, [&](uint32_t, uint32_t m) {
    if (m < S)
      f(m);
  });
}

// ---- the plane fit's sums --------------------------------------------------------------------------------------------------
// Count and sums of a window in coordinates relative to its centre, in the layout lk_plane_fit (lk_strain.hpp) and
// lk_track_step_impl (lk_track.hpp) read.  Every lane adds what it is dealt in the order it meets it; join() is a fixed
// butterfly (xor GROUP / 2 .. 1: both partners add the same two numbers), after which every lane of the group holds the
// same bits.
struct PlaneSums {
  double s[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; // Sx, Sy, Sxx, Sxy, Syy, Su, Sxu, Syu, Sv, Sxv, Syv
  int n = 0;
  __device__ inline void add(double x, double y, double u, double v) {
    s[0] += x;
    s[1] += y;
    s[2] += x * x;
    s[3] += x * y;
    s[4] += y * y;
    s[5] += u;
    s[6] += x * u;
    s[7] += y * u;
    s[8] += v;
    s[9] += x * v;
    s[10] += y * v;
    ++n;
  }
  template <int GROUP> __device__ inline void join() {
    for (int m = GROUP / 2; m >= 1; m >>= 1) {
      for (int i = 0; i < 11; ++i)
        s[i] += __shfl_xor(s[i], m, GROUP);
      n += __shfl_xor(n, m, GROUP);
    }
  }
};

} // namespace
