// lk_track.hip - device side of the material-point tracks (include/lk_engine.h: lk_track_points).
//
// Per point q and frame f: the least-squares plane of u and v over the good sectors of frame f whose centre lies within
// `radius` of a position - the point's reference position (TOTAL mode) or where the frame before left it (INCREMENTAL
// mode) - in coordinates relative to that position, all in double; then lk_track_step_impl (lk_track.hpp) turns the
// window's count and sums into the point's new state and its 64-byte record.  The sectors are found on the recovery
// pass's cell grid (lk_reseed.hip's kernels through lk_cell_grid.hpp, built once per call: the centres are the same in
// every frame), in the 3 x 3 cells around the position's cell.
//   prep    lk_strain.hip's pack, a thread per (frame, sector): the good rule once per record, and {cx, cy, u, v} packed into
//           16 bytes (cx = NaN marks a sector that is not good - it then fails the distance test by itself)
//   track   a lane group per point for ALL frames of the call: the point's state {X, Y, x, y, F} stays in registers
//           (double, the same bits in every lane of the group), the frame loop runs inside the kernel.  Per frame the
//           group walks the three cell rows (each contiguous in the member table) GROUP candidates at a time - pass 1 of
//           lk_strain_kernel, no residual pass - joins the count and the 11 sums by their butterfly (lk_neighbours.hpp:
//           every lane holds the same bits) and steps the state in every lane.  Lane 0 writes the
//           record as four float4.
// A point's chain is serial in f (frame f's window is centred where frame f - 1 put the point), the points are
// independent: the launch is Q lane groups wide and F walks long.  What a walk costs is its gather: member index -> 16
// packed bytes; the sums are double at the full vector rate.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lk_device.hpp"
#include "lk_launch.hpp"
#include "lk_neighbours.hpp"
#include "lk_track.hpp"

namespace {

template <int GROUP> __global__ __launch_bounds__(kBlock) void lk_track_kernel(LkTrackArgs a) {
  const int lane = (int)(threadIdx.x & (GROUP - 1));
  const unsigned long long row = ((unsigned long long)blockIdx.x * kBlock + threadIdx.x) / GROUP;
  if (row >= (unsigned long long)a.n_points)
    return; // (the whole group leaves together)
  const size_t q = (size_t)row;
  const LkReseedGrid &g = a.grid;
  const double r2 = a.radius * a.radius;
  const uint32_t S = (uint32_t)a.n_sectors;
  const bool incremental = a.mode == LK_TRACK_INCREMENTAL;
  double st[8];
  for (int i = 0; i < 8; ++i)
    st[i] = a.state[q * 8 + i];

  for (int f = 0; f < a.n_frames; ++f) {
    const float4 *pack = a.pack + (size_t)f * (size_t)S;
    const double px = incremental ? st[2] : st[0], py = incremental ? st[3] : st[1];
    PlaneSums sums;
    // (a position that is not finite - BAD_POINT, LOST - has no window: lk_track_step_impl decides the status itself)
    if (lk_track_finite(px) && lk_track_finite(py)) {
      const CellRange cells = cell_range(g, free_cell_coord(px, g.x0, g.cell, g.nx), free_cell_coord(py, g.y0, g.cell, g.ny));
      walk_members<GROUP>(g, cells, S, lane, [&](uint32_t m) {
        const float4 c = pack[m];
        const double x = (double)c.x - px, y = (double)c.y - py;
        if (x * x + y * y <= r2) // (a NaN centre - a sector that is not good - is outside)
          sums.add(x, y, (double)c.z, (double)c.w);
      });
    }
    sums.template join<GROUP>();
    // the step: the same bits in every lane of the group
    lk_track t;
    lk_track_step_impl(a.mode, a.min_neighbours, sums.n, sums.s, st, a.tensor, &t);
    if (lane == 0) {
      float4 *o = (float4 *)(a.out + (size_t)f * (size_t)a.n_points + q); // (64-byte records in hipMalloc'ed memory: 16-byte aligned)
      o[0] = make_float4(t.x, t.y, t.u, t.v);
      o[1] = make_float4(t.ux, t.uy, t.vx, t.vy);
      o[2] = make_float4(t.exx, t.eyy, t.exy, t.e1);
      o[3] = make_float4(t.e2, t.theta, __int_as_float(t.neighbours), __int_as_float(t.status));
    }
  }
  if (lane == 0)
    for (int i = 0; i < 8; ++i)
      a.state[q * 8 + i] = st[i];
}

} // namespace

hipError_t lk_launch_track(const LkTrackArgs &a, int group, hipStream_t st) {
  if (a.n_points <= 0 || a.n_frames <= 0 || a.n_sectors <= 0)
    return hipSuccess;
  if (group != 16 && group != 64)
    return hipErrorInvalidValue;
  const dim3 grid(blocks_for((long long)a.n_points * group, kBlock)), block(kBlock);
  if (group == 16)
    hipLaunchKernelGGL((lk_track_kernel<16>), grid, block, 0, st, a);
  else
    hipLaunchKernelGGL((lk_track_kernel<64>), grid, block, 0, st, a);
  return hipGetLastError();
}
