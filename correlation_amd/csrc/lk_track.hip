// lk_track.hip - device side of the material-point tracks (include/lk_engine.h: lk_track_points).
//
// Per point q and frame f: the least-squares plane of u and v over the good sectors of frame f whose centre lies within
// `radius` of a position - the point's reference position (TOTAL mode) or where the frame before left it (INCREMENTAL
// mode) - in coordinates relative to that position, all in double; then lk_track_step_impl (lk_track.hpp) turns the
// window's count and sums into the point's new state and its 64-byte record.  The sectors are found on the recovery
// pass's cell grid (lk_reseed.hip's kernels through lk_cell_grid.hpp, built once per call: the centres are the same in
// every frame), in the 3 x 3 cells around the position's cell.
//   prep    a thread per (frame, sector): the good rule once per record, and {cx, cy, u, v} packed into 16 bytes
//           (cx = NaN marks a sector that is not good - it then fails the distance test by itself)
//   track   a lane group per point for ALL frames of the call: the point's state {X, Y, x, y, F} stays in registers
//           (double, the same bits in every lane of the group), the frame loop runs inside the kernel.  Per frame the
//           group walks the three cell rows (each contiguous in the member table) GROUP candidates at a time - pass 1 of
//           lk_strain_kernel, no residual pass - joins the count and the 11 sums by a fixed butterfly (both partners add
//           the same two numbers, so every lane holds the same bits) and steps the state in every lane.  Lane 0 writes the
//           record as four float4.
// A point's chain is serial in f (frame f's window is centred where frame f - 1 put the point), the points are
// independent: the launch is Q lane groups wide and F walks long.  What a walk costs is its gather: member index -> 16
// packed bytes; the sums are double at the full vector rate.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lk_device.hpp"
#include "lk_good.hpp"
#include "lk_launch.hpp"
#include "lk_track.hpp"

namespace {

constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void lk_track_prep_kernel(const lk_result *rec, const float2 *center, int n_sectors,
                                                               long long total, int model, float chi_max, float4 *pack) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= total)
    return;
  const lk_result r = rec[i];
  const bool g = reseed_good(r, n_params_of(model), chi_max);
  const float2 c = center[i % n_sectors];
  pack[i] = make_float4(g ? c.x : __uint_as_float(0x7fc00000u), c.y, r.resultingParameters[0],
                        model == LK_FM_U ? 0.f : r.resultingParameters[1]);
}

// the cell coordinate of a position: the grid kernel's expression for a centre (lk_reseed.hip: floor((v - origin) / cell)),
// clamped to [-2, n + 1].  -1 and n are one cell beyond the grid, whose 3-cell range still reaches the grid's edge cells;
// -2 and n + 1 stand for everything farther out: more than a cell (>= radius) from every centre, their range is empty
__device__ inline int track_cell_coord(double v, double origin, double cell, int n) {
  const double q = floor((v - origin) / cell);
  return q >= (double)(n + 1) ? n + 1 : (q > -2.0 ? (int)q : -2);
}

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
    double Sx = 0, Sy = 0, Sxx = 0, Sxy = 0, Syy = 0, Su = 0, Sxu = 0, Syu = 0, Sv = 0, Sxv = 0, Syv = 0;
    int cnt = 0;
    // (a position that is not finite - BAD_POINT, LOST - has no window: lk_track_step_impl decides the status itself)
    if (lk_track_finite(px) && lk_track_finite(py)) {
      const int ix = track_cell_coord(px, g.x0, g.cell, g.nx), iy = track_cell_coord(py, g.y0, g.cell, g.ny);
      const int x_lo = ix > 0 ? ix - 1 : 0, x_hi = ix + 1 < g.nx ? ix + 1 : g.nx - 1;
      const int y_lo = iy > 0 ? iy - 1 : 0, y_hi = iy + 1 < g.ny ? iy + 1 : g.ny - 1;
      if (x_lo <= x_hi) // (two or more cells beyond the grid in x: nothing to walk; in y the row loop is empty by itself)
        for (int yy = y_lo; yy <= y_hi; ++yy) {
          const uint32_t b = g.start[(size_t)yy * (size_t)g.nx + (size_t)x_lo];
          uint32_t e = g.start[(size_t)yy * (size_t)g.nx + (size_t)x_hi + 1];
          e = e < S ? e : S;
          for (uint32_t k = b + (uint32_t)lane; k < e; k += GROUP) {
            const uint32_t m = g.members[k];
            if (m >= S)
              continue;
            const float4 c = pack[m];
            const double x = (double)c.x - px, y = (double)c.y - py, u = (double)c.z, v = (double)c.w;
            if (!(x * x + y * y <= r2)) // (a NaN centre - a sector that is not good - is outside)
              continue;
            Sx += x;
            Sy += y;
            Sxx += x * x;
            Sxy += x * y;
            Syy += y * y;
            Su += u;
            Sxu += x * u;
            Syu += y * u;
            Sv += v;
            Sxv += x * v;
            Syv += y * v;
            ++cnt;
          }
        }
    }
    for (int m = GROUP / 2; m >= 1; m >>= 1) {
      Sx += __shfl_xor(Sx, m, GROUP);
      Sy += __shfl_xor(Sy, m, GROUP);
      Sxx += __shfl_xor(Sxx, m, GROUP);
      Sxy += __shfl_xor(Sxy, m, GROUP);
      Syy += __shfl_xor(Syy, m, GROUP);
      Su += __shfl_xor(Su, m, GROUP);
      Sxu += __shfl_xor(Sxu, m, GROUP);
      Syu += __shfl_xor(Syu, m, GROUP);
      Sv += __shfl_xor(Sv, m, GROUP);
      Sxv += __shfl_xor(Sxv, m, GROUP);
      Syv += __shfl_xor(Syv, m, GROUP);
      cnt += __shfl_xor(cnt, m, GROUP);
    }
    // the step: the same bits in every lane of the group
    const double sums[11] = {Sx, Sy, Sxx, Sxy, Syy, Su, Sxu, Syu, Sv, Sxv, Syv};
    lk_track t;
    lk_track_step_impl(a.mode, a.min_neighbours, cnt, sums, st, a.tensor, &t);
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

inline unsigned blocks_for(long long n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

} // namespace

hipError_t lk_launch_track_prep(const lk_result *rec, const float2 *center, int n_sectors, int n_frames, int model, float chi_max,
                                float4 *pack, hipStream_t st) {
  if (n_sectors <= 0 || n_frames <= 0)
    return hipSuccess;
  const long long total = (long long)n_sectors * n_frames;
  hipLaunchKernelGGL(lk_track_prep_kernel, dim3(blocks_for(total, kBlock)), dim3(kBlock), 0, st, rec, center, n_sectors, total,
                     model, chi_max, pack);
  return hipGetLastError();
}

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
