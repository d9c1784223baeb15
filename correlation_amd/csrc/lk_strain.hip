// lk_strain.hip - device side of the strain field (include/lk_engine.h: lk_strain_field).
//
// Per sector s: a least-squares plane fit of u and v over the good sectors whose centre lies within `radius` of c_s
// (s itself included when good), in coordinates relative to c_s, all in double; then the strain tensor of the fitted
// gradients (lk_strain.hpp).  The neighbours are found on the recovery pass's cell grid (lk_reseed.hip's kernels, cell
// size = radius): the window of s lies in the 3 x 3 cells around its own.
//   prep    a thread per sector: the good rule once per record, and {cx, cy, u, v} packed into 16 bytes (cx = NaN marks a
//           failed sector - it then fails the distance test by itself)
//   strain  a lane group per sector walks the three cell rows (each contiguous in the member table), GROUP candidates at a
//           time.  Pass 1: the count and the 11 sums, joined by a fixed butterfly (both partners add the same two numbers,
//           so every lane holds the same bits); moments, status and gradients computed alike in every lane.  Pass 2: the
//           same walk adds the squared residuals of the fitted plane.  Lane 0 alone rounds to float, forms the tensor and writes
//           the 64-byte record as four float4.
// Work split: GROUP = 16 puts four sectors into a wavefront (a window of 2 - 3 pitches has 20 - 60 candidates in its 3 x 3
// cells, one to two trips per cell row); GROUP = 64 gives a sector the whole wavefront (windows of hundreds of candidates).
// The host picks per call (lk_strain.cpp).  The sums are double at full vector rate; what a visit costs is its gather:
// member index -> 16 packed bytes, or (unpacked) centre + flag + the first two words of a 48-byte record.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lk_device.hpp"
#include "lk_good.hpp"
#include "lk_launch.hpp"
#include "lk_strain.hpp"

namespace {

constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void lk_strain_prep_kernel(const lk_result *rec, const float2 *center, int n, int model,
                                                                float chi_max, uint8_t *good, float4 *pack) {
  const int s = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (s >= n)
    return;
  const lk_result r = rec[s];
  const bool g = reseed_good(r, n_params_of(model), chi_max);
  const float2 c = center[s];
  good[s] = g ? 1 : 0;
  pack[s] = make_float4(g ? c.x : __uint_as_float(0x7fc00000u), c.y, r.resultingParameters[0],
                        model == LK_FM_U ? 0.f : r.resultingParameters[1]);
}

// one candidate of the walk: is it in the window, and its (dx, dy, u, v)
template <bool PACKED>
__device__ inline bool strain_visit(const LkStrainArgs &a, uint32_t m, float2 cs, double r2, double &dx, double &dy, double &u,
                                    double &v) {
  float cx, cy, fu, fv;
  if (PACKED) {
    const float4 q = a.pack[m];
    cx = q.x, cy = q.y, fu = q.z, fv = q.w;
  } else {
    if (!a.good[m])
      return false;
    const float2 c = a.center[m];
    const float *p = a.rec[m].resultingParameters;
    cx = c.x, cy = c.y, fu = p[0], fv = a.has_v ? p[1] : 0.f;
  }
  dx = (double)cx - (double)cs.x;
  dy = (double)cy - (double)cs.y;
  u = (double)fu;
  v = (double)fv;
  return dx * dx + dy * dy <= r2; // (a NaN centre - a failed sector of the packed array - is outside)
}

template <int GROUP, bool PACKED> __global__ __launch_bounds__(kBlock) void lk_strain_kernel(LkStrainArgs a) {
  const int lane = (int)(threadIdx.x & (GROUP - 1));
  const unsigned long long row = ((unsigned long long)blockIdx.x * kBlock + threadIdx.x) / GROUP;
  if (row >= (unsigned long long)a.n_sectors)
    return; // (the whole group leaves together)
  const int s = (int)row;
  const LkReseedGrid &g = a.grid;
  const float2 cs = a.center[s];
  const int cell = (int)g.cell_of[s], ix = cell % g.nx, iy = cell / g.nx;
  const int x_lo = ix > 0 ? ix - 1 : 0, x_hi = ix + 1 < g.nx ? ix + 1 : g.nx - 1;
  const int y_lo = iy > 0 ? iy - 1 : 0, y_hi = iy + 1 < g.ny ? iy + 1 : g.ny - 1;
  const double r2 = a.radius * a.radius;
  const uint32_t S = (uint32_t)a.n_sectors;

  // pass 1: the count and the sums
  double Sx = 0, Sy = 0, Sxx = 0, Sxy = 0, Syy = 0, Su = 0, Sxu = 0, Syu = 0, Sv = 0, Sxv = 0, Syv = 0;
  int cnt = 0;
  for (int yy = y_lo; yy <= y_hi; ++yy) {
    const uint32_t b = g.start[(size_t)yy * (size_t)g.nx + (size_t)x_lo];
    uint32_t e = g.start[(size_t)yy * (size_t)g.nx + (size_t)x_hi + 1];
    e = e < S ? e : S;
    for (uint32_t k = b + (uint32_t)lane; k < e; k += GROUP) {
      const uint32_t m = g.members[k];
      double x, y, u, v;
      if (m >= S || !strain_visit<PACKED>(a, m, cs, r2, x, y, u, v))
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

  // moments, status, gradients: the same bits in every lane of the group
  const double n = (double)cnt;
  const double Cxx = Sxx - Sx * Sx / n, Cxy = Sxy - Sx * Sy / n, Cyy = Syy - Sy * Sy / n;
  const double Cxu = Sxu - Sx * Su / n, Cyu = Syu - Sy * Su / n, Cxv = Sxv - Sx * Sv / n, Cyv = Syv - Sy * Sv / n;
  const double CC = Cxx * Cyy, D = CC - Cxy * Cxy;
  int status = LK_STRAIN_OK;
  if (cnt < a.min_neighbours)
    status = LK_STRAIN_TOO_FEW;
  else if (CC == 0.0 || !(D > 1e-6 * CC))
    status = LK_STRAIN_DEGENERATE;
  else if (PACKED ? a.pack[s].x != a.pack[s].x : !a.good[s])
    status = LK_STRAIN_FILLED;

  double fit[6] = {0, 0, 0, 0, 0, 0}, rr = 0; // u, v, ux, uy, vx, vy of the plane; the residual sum
  const bool valid = status == LK_STRAIN_OK || status == LK_STRAIN_FILLED;
  if (valid) {
    const double ux = (Cyy * Cxu - Cxy * Cyu) / D, uy = (Cxx * Cyu - Cxy * Cxu) / D;
    const double vx = (Cyy * Cxv - Cxy * Cyv) / D, vy = (Cxx * Cyv - Cxy * Cxv) / D;
    const double u0 = Su / n - ux * (Sx / n) - uy * (Sy / n), v0 = Sv / n - vx * (Sx / n) - vy * (Sy / n);
    // pass 2: the residuals of the fitted plane over the same window
    for (int yy = y_lo; yy <= y_hi; ++yy) {
      const uint32_t b = g.start[(size_t)yy * (size_t)g.nx + (size_t)x_lo];
      uint32_t e = g.start[(size_t)yy * (size_t)g.nx + (size_t)x_hi + 1];
      e = e < S ? e : S;
      for (uint32_t k = b + (uint32_t)lane; k < e; k += GROUP) {
        const uint32_t m = g.members[k];
        double x, y, u, v;
        if (m >= S || !strain_visit<PACKED>(a, m, cs, r2, x, y, u, v))
          continue;
        const double ru = u - (u0 + ux * x + uy * y), rv = v - (v0 + vx * x + vy * y);
        rr += ru * ru + rv * rv;
      }
    }
    for (int m = GROUP / 2; m >= 1; m >>= 1)
      rr += __shfl_xor(rr, m, GROUP);
    fit[0] = u0, fit[1] = v0, fit[2] = ux, fit[3] = uy, fit[4] = vx, fit[5] = vy;
  }
  if (lane != 0)
    return;
  // one lane rounds to float, forms the tensor of the float gradients and writes the record
  float f[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; // u, v, ux, uy, vx, vy, exx .. theta
  float residual = 0.f;
  if (valid) {
    for (int i = 0; i < 6; ++i)
      f[i] = (float)fit[i];
    (void)lk_strain_tensor_impl(a.tensor, f + 2, f + 6);
    residual = (float)sqrt(rr / n);
  }
  float4 *o = (float4 *)(a.out + s); // (64-byte records in hipMalloc'ed memory: 16-byte aligned)
  o[0] = make_float4(f[0], f[1], f[2], f[3]);
  o[1] = make_float4(f[4], f[5], f[6], f[7]);
  o[2] = make_float4(f[8], f[9], f[10], f[11]);
  o[3] = make_float4(residual, __int_as_float(cnt), __int_as_float(status), __int_as_float(0));
}

inline unsigned blocks_for(long long n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

} // namespace

hipError_t lk_launch_strain_prep(const lk_result *rec, const float2 *center, int n_sectors, int model, float chi_max,
                                 uint8_t *good, float4 *pack, hipStream_t st) {
  if (n_sectors <= 0)
    return hipSuccess;
  hipLaunchKernelGGL(lk_strain_prep_kernel, dim3(blocks_for(n_sectors, kBlock)), dim3(kBlock), 0, st, rec, center, n_sectors,
                     model, chi_max, good, pack);
  return hipGetLastError();
}

hipError_t lk_launch_strain(const LkStrainArgs &a, int group, int packed, hipStream_t st) {
  if (a.n_sectors <= 0)
    return hipSuccess;
  if (group != 16 && group != 64)
    return hipErrorInvalidValue;
  const dim3 grid(blocks_for((long long)a.n_sectors * group, kBlock)), block(kBlock);
  if (group == 16 && packed)
    hipLaunchKernelGGL((lk_strain_kernel<16, true>), grid, block, 0, st, a);
  else if (group == 16)
    hipLaunchKernelGGL((lk_strain_kernel<16, false>), grid, block, 0, st, a);
  else if (packed)
    hipLaunchKernelGGL((lk_strain_kernel<64, true>), grid, block, 0, st, a);
  else
    hipLaunchKernelGGL((lk_strain_kernel<64, false>), grid, block, 0, st, a);
  return hipGetLastError();
}
