// lk_field.hip - device side of the field map (include/lk_engine.h: lk_field_map).
//
// Per node of a regular grid of level-0 positions: lk_track_points' windowed least-squares plane of u and v over the good
// sectors within `radius` of a position, optionally weighted, in coordinates relative to that position, all in double; then
// lk_field_fit / lk_field_values (lk_field.hpp) turn the window's count, weight sum and sums into the node's status and its
// twelve floats.  REFERENCE: one fit at the node.  DEFORMED: the node is a position on the deformed frame; K fixed-point
// steps X <- node - u_fit(X) find the material point that moved there, and the fit at that point is reported.
//   prep   lk_strain.hip's pack: {cx or NaN, cy, u, v} in 16 bytes per sector
//   map    one workgroup per tile of 32 x 8 nodes, x fastest, a thread per node.  The cells of the 3 x 3 neighbourhoods of all
//          nodes of a tile form a rectangle of cells; its entries of the member table are staged once in LDS as the packed
//          float4 (up to kLkFieldCapacity) and scanned by every thread - all lanes read the same address at a time, a
//          broadcast.  A thread meets the staged entries in the order of the walk of lk_neighbours.hpp (rows of cells
//          ascending, the table's order within a row), and the entries a superset of its own 3 x 3 cells adds lie farther
//          than a cell = radius away: they fail the distance test and add nothing.  The sums of a node are therefore the same
//          bits whichever tile, window, stride or path it belongs to.  A tile whose rectangle does not fit, and a DEFORMED
//          iterate whose 3 x 3 cells are not inside the staged rectangle, walk those 3 x 3 cells in global memory with one
//          lane (walk_members<1>): the same members in the same order.
// The sums are 12 double accumulators per thread at the full vector rate; a staged entry costs an 8-byte LDS
// broadcast of its centre and, for a member, a second one of its displacement.
// The stores are planar and contiguous along x, made for the selected channels only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lk_device.hpp"
#include "lk_field.hpp"
#include "lk_launch.hpp"
#include "lk_neighbours.hpp"

namespace {

// is the range `in` (not empty) inside `out`?
__device__ inline bool range_inside(const CellRange &in, const CellRange &out) {
  return out.y_lo <= out.y_hi && in.x_lo >= out.x_lo && in.x_hi <= out.x_hi && in.y_lo >= out.y_lo && in.y_hi <= out.y_hi;
}

template <bool BISQUARE, bool DEFORMED> __global__ __launch_bounds__(kBlock) void lk_field_map_kernel(LkFieldArgs a) {
  static_assert(kLkMapTileW * kLkMapTileH == kBlock, "a thread per node of the tile");
  __shared__ float4 s_pack[kLkFieldCapacity];
  const LkReseedGrid &g = a.grid;
  const int tid = (int)threadIdx.x;
  const int tile_x = (int)blockIdx.x % a.tiles_x, tile_y = (int)blockIdx.x / a.tiles_x;
  // the tile's nodes, and the rectangle of cells their 3 x 3 neighbourhoods cover (uniform over the workgroup)
  const int i0 = tile_x * kLkMapTileW, j0 = tile_y * kLkMapTileH;
  const int i1 = min(i0 + kLkMapTileW, a.nx) - 1, j1 = min(j0 + kLkMapTileH, a.ny) - 1;
  const auto node_x = [&](int i) { return (double)((long long)a.x0 + (long long)i * (long long)a.stride); }; // (exact)
  const auto node_y = [&](int j) { return (double)((long long)a.y0 + (long long)j * (long long)a.stride); };
  const uint32_t S = (uint32_t)a.n_sectors;
  const CellRange cells = cell_range(g, free_cell_coord(node_x(i0), g.x0, g.cell, g.nx), free_cell_coord(node_x(i1), g.x0, g.cell, g.nx),
                                     free_cell_coord(node_y(j0), g.y0, g.cell, g.ny), free_cell_coord(node_y(j1), g.y0, g.cell, g.ny));
  const long long total = a.walk ? (long long)kLkFieldCapacity + 1 : cell_range_entries(g, cells, S);
  const bool staged = total <= (long long)kLkFieldCapacity;
  if (staged) {
    walk_entries<kBlock>(g, cells, S, tid, [&](uint32_t at, uint32_t m) { // at < total <= kLkFieldCapacity
      s_pack[at] = m < S ? a.pack[m] : make_float4(__uint_as_float(0x7fc00000u), 0.f, 0.f, 0.f);
    });
    __syncthreads();
  } else if (tid == 0) {
    atomicAdd(a.fallback, 1u);
  }
  const int i = i0 + tid % kLkMapTileW, j = j0 + tid / kLkMapTileW;
  if (i > i1 || j > j1) // (behind the only barrier)
    return;
  const double nx_ = node_x(i), ny_ = node_y(j), r2 = a.r2;

  // the window of a position: count, weight sum and sums, the members met in the walk's order on either path
  const auto window = [&](double px, double py, LkFieldSums &sums) {
    const auto visit = [&](const float4 c) {
      const double x = (double)c.x - px, y = (double)c.y - py;
      const double d2 = x * x + y * y;
      if (d2 <= r2) // (a NaN centre - a sector that is not good, an entry that names none - is outside)
        sums.add(BISQUARE ? lk_field_weight(LK_FIELD_BISQUARE, d2, r2) : 1.0, x, y, (double)c.z, (double)c.w);
    };
    bool in_lds = staged;
    CellRange around = cells;
    if (DEFORMED || !staged) {
      around = cell_range(g, free_cell_coord(px, g.x0, g.cell, g.nx), free_cell_coord(py, g.y0, g.cell, g.ny));
      if (around.y_lo > around.y_hi)
        return; // more than a cell from every centre: no member
      in_lds = staged && range_inside(around, cells);
    }
    if (in_lds) {
      for (int k = 0; k < (int)total; ++k)
        visit(s_pack[k]);
    } else {
      walk_members<1>(g, around, S, 0, [&](uint32_t m) { visit(a.pack[m]); });
    }
  };

  double px = nx_, py = ny_;
  LkPlaneFit pf;
  int status = LK_FIELD_OK, n = 0;
  const int fits = DEFORMED ? a.iterations + 1 : 1;
  for (int k = 0; k < fits; ++k) {
    LkFieldSums sums;
    window(px, py, sums);
    n = sums.n;
    status = lk_field_fit(a.min_neighbours, sums.n, sums.W, sums.s, &pf);
    if (status != LK_FIELD_OK || k + 1 == fits)
      break; // (an iterate without a fit gives the node its status and count)
    px = nx_ - pf.u0; // the plane's value at the position it is centred at
    py = ny_ - pf.v0;
  }

  const float nan = __uint_as_float(0x7fc00000u);
  float f[kLkFieldChannels];
#pragma unroll
  for (int c = 0; c < kLkFieldChannels; ++c)
    f[c] = nan;
  if (status == LK_FIELD_OK) {
    lk_field_values(pf, a.tensor, f);
    f[12] = (float)px;
    f[13] = (float)py;
    if (DEFORMED) {
      const double ex = (px + pf.u0) - nx_, ey = (py + pf.v0) - ny_;
      f[14] = (float)hypot(ex, ey);
    } else {
      f[14] = 0.f;
    }
  }
  const size_t plane = (size_t)a.nx * (size_t)a.ny, at = (size_t)j * (size_t)a.nx + (size_t)i;
  float *out = a.maps + at;
#pragma unroll
  for (int c = 0; c < kLkFieldChannels; ++c)
    if ((a.channels >> c) & 1u) {
      *out = f[c];
      out += plane;
    }
  if (a.neighbours)
    a.neighbours[at] = n;
  if (a.status)
    a.status[at] = (uint8_t)status;
}

} // namespace

hipError_t lk_launch_field_map(const LkFieldArgs &a, int weight, int frame, int *n_tiles, hipStream_t st) {
  if (a.n_sectors <= 0 || a.nx <= 0 || a.ny <= 0 || a.stride <= 0 || a.tiles_x != (a.nx + kLkMapTileW - 1) / kLkMapTileW ||
      (long long)a.nx * (long long)a.ny > 0x7fffffffLL || (a.channels != 0 && !a.maps) || a.channels >> kLkFieldChannels != 0 ||
      (frame == LK_FIELD_DEFORMED && (a.iterations < 1 || a.iterations > kLkFieldMaxIterations)))
    return hipErrorInvalidValue;
  const long long tiles = (long long)a.tiles_x * (long long)((a.ny + kLkMapTileH - 1) / kLkMapTileH);
  if (n_tiles)
    *n_tiles = (int)tiles;
  const dim3 grid((unsigned)tiles), block(kBlock);
  const bool bisquare = weight == LK_FIELD_BISQUARE, deformed = frame == LK_FIELD_DEFORMED;
  if (!bisquare && !deformed)
    hipLaunchKernelGGL((lk_field_map_kernel<false, false>), grid, block, 0, st, a);
  else if (bisquare && !deformed)
    hipLaunchKernelGGL((lk_field_map_kernel<true, false>), grid, block, 0, st, a);
  else if (!bisquare)
    hipLaunchKernelGGL((lk_field_map_kernel<false, true>), grid, block, 0, st, a);
  else
    hipLaunchKernelGGL((lk_field_map_kernel<true, true>), grid, block, 0, st, a);
  return hipGetLastError();
}
