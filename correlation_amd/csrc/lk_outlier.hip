// lk_outlier.hip - device side of the outlier flags (include/lk_engine.h: lk_flag_outliers).
//
// Per sector s: the (detrended) normalised median test of its displacement against the good sectors within `radius` of
// c_s, s itself left out.  The neighbours are found as lk_strain.hip finds them: the recovery pass's cell grid (cell size =
// radius), a lane group per sector, three cell rows, GROUP candidates at a time.
//   prep     lk_strain.hip's pack with the canonical zero: the good rule once per record, {cx, cy, u + 0, v + 0} packed
//            into 16 bytes (cx = NaN marks a sector that is not in anybody's window - it fails the distance test by itself)
//   exclude  between two passes: the NaN marks rewritten from the good flags and the flags of the pass before
//   outlier  walk 1: the count and (detrend) the 11 plane sums, joined by their butterfly (lk_neighbours.hpp); status and plane
//            alike in every lane.  Walk 2: the floats e_j of both components.  Then the selections of lk_outlier.hpp - four
//            medians (med and mad of u and v) in 2 x 33 counting rounds, u and v sharing a round - and the ratios.
//   mark     errorCode = LK_ERROR_OUTLIER in the records of the flagged sectors
// Where the e_j live between the rounds: lane l keeps ITS members - the ones its own trips of walk 2 met - in a column of
// LDS, member t at word t * 256 + threadIdx.x.  A lane reads back only what it wrote itself, so no barrier is needed and
// the groups of a block never wait for each other; the 32 lanes that share an LDS cycle (ds_read_b32 / ds_write_b32 bank =
// word mod 32, per 32-lane half) touch 32 consecutive words: no bank conflict for either group width.  A count is a
// lane's loop over its column and a butterfly of two integers.  kLkOutlierRows words per lane and component are there
// (32 KB per block of 256 threads: 16 lanes x 16 = 256 members per sector when the walk deals them evenly, 64 lanes 1024);
// when any lane of the group has met more, the whole group re-walks the window from global memory in every round and forms
// the same floats again - the same answer, 66 times the gathers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lk_device.hpp"
#include "lk_launch.hpp"
#include "lk_neighbours.hpp"
#include "lk_outlier.hpp"
#include "lk_strain.hpp"

namespace {

__global__ __launch_bounds__(kBlock) void lk_outlier_exclude_kernel(const lk_outlier *flags, const float2 *center,
                                                                    const uint8_t *good, int n, float4 *pack) {
  const int s = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (s >= n)
    return;
  const bool in = good[s] && flags[s].status != LK_OUTLIER_FLAGGED;
  pack[s].x = in ? center[s].x : __uint_as_float(0x7fc00000u);
}

__global__ __launch_bounds__(kBlock) void lk_outlier_mark_kernel(const lk_outlier *flags, int n, lk_result *rec) {
  const int s = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (s >= n)
    return;
  if (flags[s].status == LK_OUTLIER_FLAGGED)
    rec[s].errorCode = LK_ERROR_OUTLIER;
}

// the fitted plane of a window (all zero in plain mode: e_j = u_j - 0)
struct Plane {
  double u0, ux, uy, v0, vx, vy;
};

// The window of one sector as its lane group sees it (lk_outlier.hpp: Src).
template <int GROUP> struct GroupWindow {
  const LkOutlierArgs &a;
  int s = 0, lane = 0;
  CellRange cells = {0, 0, 0, -1};
  float2 cs = {0.f, 0.f};
  double r2 = 0;
  bool detrend = false, stashed = false;
  Plane pl = {0, 0, 0, 0, 0, 0};
  const float *col_u = nullptr, *col_v = nullptr; // this lane's LDS columns (stride kBlock words)
  int mine = 0;                                   // members in them
  bool deviation = false;                         // the current selection: of e_j, or of |e_j - med|
  float med_u = 0.f, med_v = 0.f;

  // every member of the window this lane is dealt: f(dx, dy, u, v)
  template <class F> __device__ inline void walk(F f) const {
    walk_members<GROUP>(a.grid, cells, (uint32_t)a.n_sectors, lane, [&](uint32_t m) {
      if (m == (uint32_t)s)
        return;
      const float4 q = a.pack[m];
      const double dx = (double)q.x - (double)cs.x, dy = (double)q.y - (double)cs.y;
      if (dx * dx + dy * dy <= r2) // (a NaN centre - not good, or excluded - is outside)
        f(dx, dy, (double)q.z, (double)q.w);
    });
  }
  __device__ inline float e_u(double dx, double dy, double u) const {
    return detrend ? (float)(u - (pl.u0 + pl.ux * dx + pl.uy * dy)) + 0.0f : (float)u;
  }
  __device__ inline float e_v(double dx, double dy, double v) const {
    return detrend ? (float)(v - (pl.v0 + pl.vx * dx + pl.vy * dy)) + 0.0f : (float)v;
  }
  // every member's values of the current selection: f(value of u, value of v)
  template <class F> __device__ inline void values(F f) const {
    if (stashed) {
      for (int t = 0; t < mine; ++t)
        f(lk_outlier_value(col_u[t * kBlock], deviation, med_u), lk_outlier_value(col_v[t * kBlock], deviation, med_v));
    } else {
      walk([&](double dx, double dy, double u, double v) {
        f(lk_outlier_value(e_u(dx, dy, u), deviation, med_u), lk_outlier_value(e_v(dx, dy, v), deviation, med_v));
      });
    }
  }
  __device__ inline void below(uint32_t tu, uint32_t tv, int &cu, int &cv) const {
    int nu = 0, nv = 0;
    values([&](float fu, float fv) {
      nu += lk_outlier_key(fu) < tu ? 1 : 0;
      nv += lk_outlier_key(fv) < tv ? 1 : 0;
    });
    for (int m = GROUP / 2; m >= 1; m >>= 1) {
      nu += __shfl_xor(nu, m, GROUP);
      nv += __shfl_xor(nv, m, GROUP);
    }
    cu = nu, cv = nv;
  }
  __device__ inline void above(uint32_t xu, uint32_t xv, int &cu, int &cv, uint32_t &mu, uint32_t &mv) const {
    int nu = 0, nv = 0;
    uint32_t lu = 0xffffffffu, lv = 0xffffffffu;
    values([&](float fu, float fv) {
      const uint32_t ku = lk_outlier_key(fu), kv = lk_outlier_key(fv);
      nu += ku <= xu ? 1 : 0;
      nv += kv <= xv ? 1 : 0;
      lu = ku > xu && ku < lu ? ku : lu;
      lv = kv > xv && kv < lv ? kv : lv;
    });
    for (int m = GROUP / 2; m >= 1; m >>= 1) {
      nu += __shfl_xor(nu, m, GROUP);
      nv += __shfl_xor(nv, m, GROUP);
      const uint32_t ou = (uint32_t)__shfl_xor((int)lu, m, GROUP), ov = (uint32_t)__shfl_xor((int)lv, m, GROUP);
      lu = ou < lu ? ou : lu;
      lv = ov < lv ? ov : lv;
    }
    cu = nu, cv = nv, mu = lu, mv = lv;
  }
};

template <int GROUP> __global__ __launch_bounds__(kBlock) void lk_outlier_kernel(LkOutlierArgs a) {
  __shared__ float lds_u[kLkOutlierRows * kBlock], lds_v[kLkOutlierRows * kBlock];
  const int lane = (int)(threadIdx.x & (GROUP - 1));
  const unsigned long long row = ((unsigned long long)blockIdx.x * kBlock + threadIdx.x) / GROUP;
  if (row >= (unsigned long long)a.n_sectors)
    return; // (the whole group leaves together; no barrier follows)
  const int s = (int)row;
  GroupWindow<GROUP> w{a};
  w.s = s, w.lane = lane;
  w.cells = cell_range_of(a.grid, s);
  w.cs = a.center[s];
  w.r2 = a.radius * a.radius;
  w.detrend = a.detrend != 0;

  // walk 1: the count, this lane's share of it, and the plane's sums
  PlaneSums sums;
  if (w.detrend)
    w.walk([&](double x, double y, double u, double v) { sums.add(x, y, u, v); });
  else
    w.walk([&](double, double, double, double) { ++sums.n; });
  const int mine = sums.n;
  if (w.detrend)
    sums.template join<GROUP>();
  int cnt = mine, most = mine;
  for (int m = GROUP / 2; m >= 1; m >>= 1) {
    cnt += __shfl_xor(cnt, m, GROUP);
    const int o = __shfl_xor(most, m, GROUP);
    most = o > most ? o : most;
  }

  const bool self_good = a.good[s] != 0;
  int status = LK_OUTLIER_OK;
  if (cnt < a.min_neighbours) {
    status = LK_OUTLIER_TOO_FEW;
  } else if (w.detrend) {
    // moments, status, plane: the same bits in every lane of the group
    const LkPlaneFit pf = lk_plane_fit(cnt, sums.s);
    if (pf.CC == 0.0 || !(pf.D > 1e-6 * pf.CC))
      status = LK_OUTLIER_DEGENERATE;
    else
      w.pl = Plane{pf.u0, pf.ux, pf.uy, pf.v0, pf.vx, pf.vy};
  }
  lk_outlier rec{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, cnt, status};
  if (status == LK_OUTLIER_OK) { // (uniform over the group)
    // walk 2: this lane's members into its LDS columns, if every lane of the group has room for its own
    float *cu = lds_u + threadIdx.x, *cv = lds_v + threadIdx.x;
    w.col_u = cu, w.col_v = cv;
    w.mine = mine < kLkOutlierRows ? mine : kLkOutlierRows;
    w.stashed = most <= a.lds_rows;
    if (w.stashed) {
      int t = 0;
      w.walk([&](double dx, double dy, double u, double v) {
        if (t < kLkOutlierRows) { // (t < mine <= lds_rows by walk 1; the columns end here whatever happens)
          cu[t * kBlock] = w.e_u(dx, dy, u);
          cv[t * kBlock] = w.e_v(dx, dy, v);
        }
        ++t;
      });
    }
    float med_u, med_v, mad_u, mad_v;
    lk_outlier_medians(w, cnt, &med_u, &med_v);
    w.deviation = true;
    w.med_u = med_u, w.med_v = med_v;
    lk_outlier_medians(w, cnt, &mad_u, &mad_v);
    if (self_good) {
      const float4 q = a.pack[s]; // (u, v of s; its cx may be NaN after an exclusion)
      const float es_u = w.detrend ? (float)((double)q.z - w.pl.u0) : q.z;
      const float es_v = w.detrend ? (float)((double)q.w - w.pl.v0) : q.w;
      lk_outlier_ratios(es_u, es_v, med_u, med_v, mad_u, mad_v, a.eps, a.threshold, &rec);
    } else {
      rec.med_u = med_u, rec.med_v = med_v, rec.mad_u = mad_u, rec.mad_v = mad_v;
      rec.status = LK_OUTLIER_NOT_GOOD;
    }
  }
  if (lane != 0)
    return;
  float4 *o = (float4 *)(a.out + s); // (32-byte records in hipMalloc'ed memory: 16-byte aligned)
  o[0] = make_float4(rec.med_u, rec.med_v, rec.mad_u, rec.mad_v);
  o[1] = make_float4(rec.ratio_u, rec.ratio_v, __int_as_float(rec.neighbours), __int_as_float(rec.status));
}

} // namespace

hipError_t lk_launch_outlier_exclude(const lk_outlier *flags, const float2 *center, const uint8_t *good, int n_sectors,
                                     float4 *pack, hipStream_t st) {
  if (n_sectors <= 0)
    return hipSuccess;
  hipLaunchKernelGGL(lk_outlier_exclude_kernel, dim3(blocks_for(n_sectors, kBlock)), dim3(kBlock), 0, st, flags, center, good,
                     n_sectors, pack);
  return hipGetLastError();
}

hipError_t lk_launch_outlier(const LkOutlierArgs &a, int group, hipStream_t st) {
  if (a.n_sectors <= 0)
    return hipSuccess;
  if ((group != 16 && group != 64) || a.lds_rows < 0 || a.lds_rows > kLkOutlierRows)
    return hipErrorInvalidValue;
  const dim3 grid(blocks_for((long long)a.n_sectors * group, kBlock)), block(kBlock);
  if (group == 16)
    hipLaunchKernelGGL((lk_outlier_kernel<16>), grid, block, 0, st, a);
  else
    hipLaunchKernelGGL((lk_outlier_kernel<64>), grid, block, 0, st, a);
  return hipGetLastError();
}

hipError_t lk_launch_outlier_mark(const lk_outlier *flags, int n_sectors, lk_result *rec, hipStream_t st) {
  if (n_sectors <= 0)
    return hipSuccess;
  hipLaunchKernelGGL(lk_outlier_mark_kernel, dim3(blocks_for(n_sectors, kBlock)), dim3(kBlock), 0, st, flags, n_sectors, rec);
  return hipGetLastError();
}
