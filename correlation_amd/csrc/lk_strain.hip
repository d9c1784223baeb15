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
#include "lk_launch.hpp"
#include "lk_neighbours.hpp"
#include "lk_strain.hpp"

namespace {

// The pack of strain, outlier and track: a thread per record i of [F][S], the good rule once per record.  zero: u + 0 and
// v + 0 (the outlier test's canonical zero: -0 becomes +0).
__global__ __launch_bounds__(kBlock) void lk_pack_prep_kernel(const lk_result *rec, const float2 *center, int n_sectors,
                                                              long long total, int model, float chi_max, int zero,
                                                              uint8_t *good, float4 *pack) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= total)
    return;
  const lk_result r = rec[i];
  const bool g = reseed_good(r, n_params_of(model), chi_max);
  const float2 c = center[total == n_sectors ? i : i % n_sectors];
  if (good)
    good[i] = g ? 1 : 0;
  const float u = r.resultingParameters[0], v = model == LK_FM_U ? 0.f : r.resultingParameters[1];
  pack[i] = make_float4(g ? c.x : __uint_as_float(0x7fc00000u), c.y, zero ? u + 0.0f : u, zero ? v + 0.0f : v);
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
  const CellRange cells = cell_range_of(g, s);
  const double r2 = a.radius * a.radius;
  const uint32_t S = (uint32_t)a.n_sectors;

  // pass 1: the count and the sums
  PlaneSums sums;
  walk_members<GROUP>(g, cells, S, lane, [&](uint32_t m) {
    double x, y, u, v;
    if (strain_visit<PACKED>(a, m, cs, r2, x, y, u, v))
      sums.add(x, y, u, v);
  });
  sums.template join<GROUP>();

  // moments, status, gradients: the same bits in every lane of the group
  const int cnt = sums.n;
  const double n = (double)cnt;
  const LkPlaneFit pf = lk_plane_fit(cnt, sums.s);
  int status = LK_STRAIN_OK;
  if (cnt < a.min_neighbours)
    status = LK_STRAIN_TOO_FEW;
  else if (pf.CC == 0.0 || !(pf.D > 1e-6 * pf.CC))
    status = LK_STRAIN_DEGENERATE;
  else if (PACKED ? a.pack[s].x != a.pack[s].x : !a.good[s])
    status = LK_STRAIN_FILLED;

  double fit[6] = {0, 0, 0, 0, 0, 0}, rr = 0; // u, v, ux, uy, vx, vy of the plane; the residual sum
  const bool valid = status == LK_STRAIN_OK || status == LK_STRAIN_FILLED;
  if (valid) {
    // pass 2: the residuals of the fitted plane over the same window
    walk_members<GROUP>(g, cells, S, lane, [&](uint32_t m) {
      double x, y, u, v;
      if (!strain_visit<PACKED>(a, m, cs, r2, x, y, u, v))
        return;
      const double ru = u - (pf.u0 + pf.ux * x + pf.uy * y), rv = v - (pf.v0 + pf.vx * x + pf.vy * y);
      rr += ru * ru + rv * rv;
    });
    for (int m = GROUP / 2; m >= 1; m >>= 1)
      rr += __shfl_xor(rr, m, GROUP);
    fit[0] = pf.u0, fit[1] = pf.v0, fit[2] = pf.ux, fit[3] = pf.uy, fit[4] = pf.vx, fit[5] = pf.vy;
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

} // namespace

hipError_t lk_launch_pack_prep(const lk_result *rec, const float2 *center, int n_sectors, int n_frames, int model, float chi_max,
                               int canonical_zero, uint8_t *good, float4 *pack, hipStream_t st) {
  if (n_sectors <= 0 || n_frames <= 0)
    return hipSuccess;
  const long long total = (long long)n_sectors * n_frames;
  hipLaunchKernelGGL(lk_pack_prep_kernel, dim3(blocks_for(total, kBlock)), dim3(kBlock), 0, st, rec, center, n_sectors, total,
                     model, chi_max, canonical_zero, good, pack);
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
