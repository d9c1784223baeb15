// lk_stereo.hip - device side of the two-camera rig (include/lk_engine.h: lk_stereo_points, lk_stereo_strain).
//
//   points   a thread per (frame, sector), the reference state as the first frame: the good rule of the records it reads,
//            the two pixels, lk_stereo_triangulate_impl (lk_stereo.hpp - some 600 double operations, no memory but the
//            records), the 64-byte point as four 16-byte stores
//   strain   a lane group per (frame, sector) walks the three cell rows around the sector as lk_strain.hip does, GROUP
//            candidates at a time.  A candidate costs its centre (8 bytes) and, inside the radius, the status and X, Y, Z of
//            its two points (2 x 28 of 2 x 64 bytes).  Pass 1: the count and the 23 sums, joined by a fixed butterfly (every
//            lane then holds the same bits); planes, status and tangents alike in every lane.  Pass 2: the same walk adds
//            the squared misfit of the three displacement planes.  Lane 0 alone forms the tensor, rounds to float and writes
//            the 128-byte record as eight float4.
// The cell grid is over the centres alone: one grid serves every frame of a call (blockIdx.y).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lk_device.hpp"
#include "lk_launch.hpp"
#include "lk_neighbours.hpp"
#include "lk_stereo.hpp"

namespace {

__global__ __launch_bounds__(kBlock) void lk_stereo_points_kernel(LkStereoPointsArgs a) {
  const int s = (int)(blockIdx.x * kBlock + threadIdx.x), frame = (int)blockIdx.y - 1; // (-1: the reference state)
  if (s >= a.n_sectors)
    return;
  const int P = n_params_of(a.model);
  const float2 c = a.center[s];
  const lk_result &r1 = a.ref1[s]; // (read in place: the good rule indexes the parameters by a running number)
  bool good = reseed_good(r1, P, a.chi_max);
  double x0 = (double)c.x, y0 = (double)c.y, x1 = 0.0, y1 = 0.0;
  if (frame < 0) {
    x1 = (double)c.x + (double)r1.resultingParameters[0];
    y1 = (double)c.y + (a.model == LK_FM_U ? 0.0 : (double)r1.resultingParameters[1]);
  } else {
    const size_t i = (size_t)frame * (size_t)a.n_sectors + (size_t)s;
    const lk_result &f0 = a.rec0[i], &f1 = a.rec1[i];
    good = good && reseed_good(f0, P, a.chi_max) && reseed_good(f1, P, a.chi_max);
    x0 = (double)c.x + (double)f0.resultingParameters[0];
    y0 = (double)c.y + (a.model == LK_FM_U ? 0.0 : (double)f0.resultingParameters[1]);
    x1 = (double)c.x + (double)f1.resultingParameters[0];
    y1 = (double)c.y + (a.model == LK_FM_U ? 0.0 : (double)f1.resultingParameters[1]);
  }
  if (!good)
    x0 = y0 = x1 = y1 = 0.0; // (never a NaN into the arithmetic; the status is BAD_RECORD whatever these are)
  const lk_stereo_point p = lk_stereo_triangulate_impl(a.rig, good ? 1 : 0, x0, y0, x1, y1);
  // (64-byte records in hipMalloc'ed memory: 16-byte aligned)
  double2 *o = (double2 *)(a.out + ((size_t)(frame + 1) * (size_t)a.n_sectors + (size_t)s));
  float4 *of = (float4 *)o;
  o[0] = make_double2(p.X, p.Y);
  o[1] = make_double2(p.Z, __hiloint2double(__float_as_int(p.residual[1]), __float_as_int(p.residual[0])));
  of[2] = make_float4(p.residual[2], p.residual[3], p.epipolar, p.angle);
  of[3] = make_float4(__int_as_float(p.status), __int_as_float(0), __int_as_float(0), __int_as_float(0));
}

struct SurfaceSums {
  double s[kLkStereoSums] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  int n = 0;
  __device__ inline void add(double x, double y, const double *f) {
    s[0] += x;
    s[1] += y;
    s[2] += x * x;
    s[3] += x * y;
    s[4] += y * y;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      s[5 + 3 * k] += f[k];
      s[6 + 3 * k] += x * f[k];
      s[7 + 3 * k] += y * f[k];
    }
    ++n;
  }
  template <int GROUP> __device__ inline void join() {
    for (int m = GROUP / 2; m >= 1; m >>= 1) {
#pragma unroll
      for (int i = 0; i < kLkStereoSums; ++i)
        s[i] += __shfl_xor(s[i], m, GROUP);
      n += __shfl_xor(n, m, GROUP);
    }
  }
};

// one candidate of the walk: is it in the window and good, and its (dx, dy) and {X, Y, Z, U, V, W}
__device__ inline bool surface_visit(const LkStereoStrainArgs &a, const lk_stereo_point *pts, uint32_t m, float2 cs, double r2, double &dx,
                                     double &dy, double *f) {
  const float2 c = a.center[m];
  dx = (double)c.x - (double)cs.x;
  dy = (double)c.y - (double)cs.y;
  if (!(dx * dx + dy * dy <= r2))
    return false;
  const lk_stereo_point *p = a.ref + m, *q = pts + m;
  if (p->status != LK_STEREO_OK || q->status != LK_STEREO_OK)
    return false;
  f[0] = p->X, f[1] = p->Y, f[2] = p->Z;
  f[3] = q->X - f[0], f[4] = q->Y - f[1], f[5] = q->Z - f[2];
  return true;
}

template <int GROUP> __global__ __launch_bounds__(kBlock) void lk_stereo_strain_kernel(LkStereoStrainArgs a) {
  const int lane = (int)(threadIdx.x & (GROUP - 1));
  const unsigned long long row = ((unsigned long long)blockIdx.x * kBlock + threadIdx.x) / GROUP;
  if (row >= (unsigned long long)a.n_sectors)
    return; // (the whole group leaves together)
  const int s = (int)row;
  const size_t frame = (size_t)blockIdx.y;
  const lk_stereo_point *pts = a.pts + frame * (size_t)a.n_sectors;
  const LkReseedGrid &g = a.grid;
  const float2 cs = a.center[s];
  const CellRange cells = cell_range_of(g, s);
  const double r2 = a.radius * a.radius;
  const uint32_t S = (uint32_t)a.n_sectors;

  // pass 1: the count and the sums
  SurfaceSums sums;
  walk_members<GROUP>(g, cells, S, lane, [&](uint32_t m) {
    double x, y, f[6];
    if (surface_visit(a, pts, m, cs, r2, x, y, f))
      sums.add(x, y, f);
  });
  sums.template join<GROUP>();

  // planes and status: the same bits in every lane of the group
  const bool self_good = a.ref[s].status == LK_STEREO_OK && pts[s].status == LK_STEREO_OK;
  const LkStereoPlanes pl = lk_stereo_planes(sums.n, sums.s, a.min_neighbours, self_good ? 1 : 0);
  double rr = 0.0;
  if (pl.status == LK_STEREO_SURFACE_OK || pl.status == LK_STEREO_SURFACE_FILLED) {
    // pass 2: the misfit of the three displacement planes over the same window
    walk_members<GROUP>(g, cells, S, lane, [&](uint32_t m) {
      double x, y, f[6];
      if (!surface_visit(a, pts, m, cs, r2, x, y, f))
        return;
      const double ru = f[3] - (pl.f0[3] + pl.fx[3] * x + pl.fy[3] * y);
      const double rv = f[4] - (pl.f0[4] + pl.fx[4] * x + pl.fy[4] * y);
      const double rw = f[5] - (pl.f0[5] + pl.fx[5] * x + pl.fy[5] * y);
      rr += (ru * ru + rv * rv) + rw * rw;
    });
    for (int m = GROUP / 2; m >= 1; m >>= 1)
      rr += __shfl_xor(rr, m, GROUP);
  }
  if (lane != 0)
    return;
  // one lane forms the tensor, rounds to float and writes the record
  const lk_stereo_surface r = lk_stereo_surface_impl(sums.n, pl, rr);
  float4 *o = (float4 *)(a.out + (frame * (size_t)a.n_sectors + (size_t)s)); // (128-byte records in hipMalloc'ed memory)
  o[0] = make_float4(r.X, r.Y, r.Z, r.U);
  o[1] = make_float4(r.V, r.W, r.nx, r.ny);
  o[2] = make_float4(r.nz, r.exx, r.eyy, r.exy);
  o[3] = make_float4(r.e1, r.e2, r.theta, r.biot1);
  o[4] = make_float4(r.biot2, r.normal, r.residual, __int_as_float(r.neighbours));
  o[5] = make_float4(__int_as_float(r.status), __int_as_float(0), __int_as_float(0), __int_as_float(0));
  o[6] = make_float4(__int_as_float(0), __int_as_float(0), __int_as_float(0), __int_as_float(0));
  o[7] = o[6];
}

} // namespace

hipError_t lk_launch_stereo_points(const LkStereoPointsArgs &a, hipStream_t st) {
  if (a.n_sectors <= 0 || a.n_frames < 0)
    return hipSuccess;
  if (a.n_frames > 65534)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(lk_stereo_points_kernel, dim3(blocks_for(a.n_sectors, kBlock), (unsigned)a.n_frames + 1u), dim3(kBlock), 0, st, a);
  return hipGetLastError();
}

hipError_t lk_launch_stereo_strain(const LkStereoStrainArgs &a, int group, hipStream_t st) {
  if (a.n_sectors <= 0 || a.n_frames <= 0)
    return hipSuccess;
  if ((group != 16 && group != 64) || a.n_frames > 65535)
    return hipErrorInvalidValue;
  const dim3 grid(blocks_for((long long)a.n_sectors * group, kBlock), (unsigned)a.n_frames), block(kBlock);
  if (group == 16)
    hipLaunchKernelGGL((lk_stereo_strain_kernel<16>), grid, block, 0, st, a);
  else
    hipLaunchKernelGGL((lk_stereo_strain_kernel<64>), grid, block, 0, st, a);
  return hipGetLastError();
}
