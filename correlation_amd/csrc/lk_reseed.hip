// lk_reseed.hip - device side of the recovery pass (include/lk_engine.h: lk_reseed_failed, lk_reseed_plan).
//
// The pass works AROUND the solve: it decides which sectors failed, gives each a guess extrapolated from the good sectors
// near it, lets the engine's own launch code solve exactly those sectors, and merges the retries' records in.  The kernels
// here do everything but the solve:
//   classify   records -> good / failed flags, lk_reseed_info initialised
//   cell grid  a uniform grid of cell size `radius` over the sector centres: count -> exclusive scan -> scatter, then the
//              members of every cell ordered by sector index (once per call: centres do not move)
//   plan       a 16-lane row per failed sector walks the 3 x 3 cells around its own, tests the distance in double, carries
//              each good neighbour's parameters to the sector's centre and averages them in double
//   compact    the sectors to retry, written to the front of their class's own range of a second order table (same layout
//              as the engine's), with per-class counts - what the launch code takes as its sector set
//   merge      the acceptance rule; accepted records go in, everything a rejected retry wrote is put back
// None of it is on a sample-rate path: the work is a few words per sector, and the kernels are sized for latency, not for
// bandwidth (config 5's 200 000 sectors are 9.6 MB of records).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lk_device.hpp"
#include "lk_launch.hpp"
#include "lk_neighbours.hpp"

namespace {

constexpr int kWave = 64;
constexpr int kWide = 1024; // the one-workgroup kernels (bounding box, scan, compaction)

// ---- bounding box of the centres: one workgroup, {min x, min y, max x, max y} ---------------------------------------
__global__ __launch_bounds__(kWide) void lk_reseed_bbox_kernel(const float2 *center, int n, float *out4) {
  __shared__ float s_lo_x[kWide / kWave], s_lo_y[kWide / kWave], s_hi_x[kWide / kWave], s_hi_y[kWide / kWave];
  const int tid = (int)threadIdx.x;
  float lo_x = INFINITY, lo_y = INFINITY, hi_x = -INFINITY, hi_y = -INFINITY;
  for (int i = tid; i < n; i += kWide) {
    const float2 c = center[i];
    lo_x = fminf(lo_x, c.x);
    lo_y = fminf(lo_y, c.y);
    hi_x = fmaxf(hi_x, c.x);
    hi_y = fmaxf(hi_y, c.y);
  }
  for (int m = kWave / 2; m >= 1; m >>= 1) {
    lo_x = fminf(lo_x, __shfl_xor(lo_x, m));
    lo_y = fminf(lo_y, __shfl_xor(lo_y, m));
    hi_x = fmaxf(hi_x, __shfl_xor(hi_x, m));
    hi_y = fmaxf(hi_y, __shfl_xor(hi_y, m));
  }
  if ((tid & (kWave - 1)) == 0) {
    s_lo_x[tid / kWave] = lo_x;
    s_lo_y[tid / kWave] = lo_y;
    s_hi_x[tid / kWave] = hi_x;
    s_hi_y[tid / kWave] = hi_y;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kWide / kWave; ++w) {
      lo_x = fminf(lo_x, s_lo_x[w]);
      lo_y = fminf(lo_y, s_lo_y[w]);
      hi_x = fmaxf(hi_x, s_hi_x[w]);
      hi_y = fmaxf(hi_y, s_hi_y[w]);
    }
    out4[0] = lo_x;
    out4[1] = lo_y;
    out4[2] = hi_x;
    out4[3] = hi_y;
  }
}

// ---- classify ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void lk_reseed_classify_kernel(const lk_result *rec, int n, int n_params, float chi_max,
                                                                    uint8_t *good, int32_t *tried, lk_reseed_info *info,
                                                                    uint32_t *n_failed) {
  const int s = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (s >= n)
    return;
  const lk_result r = rec[s];
  const bool g = reseed_good(r, n_params, chi_max);
  good[s] = g ? 1 : 0;
  tried[s] = 0;
  lk_reseed_info o;
  o.status = g ? LK_RESEED_GOOD : LK_RESEED_NO_NEIGHBOUR;
  o.round = -1;
  o.neighbours = 0;
  o.chi_before = r.chi;
  info[s] = o;
  if (!g)
    atomicAdd(n_failed, 1u); // (one add per wavefront: the compiler folds the lanes' +1 into a count)
}

// ---- cell grid ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void lk_reseed_cell_count_kernel(const float2 *center, int n, double x0, double y0,
                                                                      double cell, int nx, int ny, uint32_t *cell_of,
                                                                      uint32_t *count) {
  const int s = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (s >= n)
    return;
  const float2 c = center[s];
  const uint32_t k = (uint32_t)cell_coord((double)c.y, y0, cell, ny) * (uint32_t)nx + (uint32_t)cell_coord((double)c.x, x0, cell, nx);
  cell_of[s] = k;
  atomicAdd(count + k, 1u);
}

// counts[n] -> exclusive prefix in place, counts[n] = total, cursor[k] = counts[k]: one workgroup, a contiguous chunk per
// thread (the cell table is at most a few words per sector)
__global__ __launch_bounds__(kWide) void lk_reseed_scan_kernel(uint32_t *counts, uint32_t *cursor, int n) {
  __shared__ uint32_t s_part[kWide];
  const int tid = (int)threadIdx.x;
  const int len = (n + kWide - 1) / kWide;
  const int b = tid * len < n ? tid * len : n, e = b + len < n ? b + len : n;
  uint32_t sum = 0;
  for (int i = b; i < e; ++i)
    sum += counts[i];
  s_part[tid] = sum;
  __syncthreads();
  for (int d = 1; d < kWide; d <<= 1) { // Hillis-Steele inclusive scan of the chunk sums
    const uint32_t v = tid >= d ? s_part[tid - d] : 0u;
    __syncthreads();
    s_part[tid] += v;
    __syncthreads();
  }
  uint32_t run = s_part[tid] - sum;
  for (int i = b; i < e; ++i) {
    const uint32_t c = counts[i];
    counts[i] = run;
    cursor[i] = run;
    run += c;
  }
  if (tid == kWide - 1)
    counts[n] = s_part[kWide - 1];
}

__global__ __launch_bounds__(kBlock) void lk_reseed_scatter_kernel(const uint32_t *cell_of, int n, uint32_t *cursor,
                                                                   uint32_t *unordered) {
  const int s = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (s >= n)
    return;
  const uint32_t at = atomicAdd(cursor + cell_of[s], 1u); // < start[cell + 1] <= n: every cell gets exactly its count
  if (at < (uint32_t)n)
    unordered[at] = (uint32_t)s;
}

// The scatter's order within a cell is the atomics' arrival order.  A sector's place among its cell's members is the
// number of members with a smaller index: O(members of the cell) per sector - a cell holds (radius / sector pitch)^2 of
// them, a handful; a layout that puts thousands of sectors into one cell pays for it here.
__global__ __launch_bounds__(kBlock) void lk_reseed_order_kernel(const uint32_t *cell_of, const uint32_t *start, const uint32_t *unordered,
                                                                 int n, uint32_t *members) {
  const int s = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (s >= n)
    return;
  const uint32_t k = cell_of[s], b = start[k], e = start[k + 1];
  uint32_t rank = 0;
  for (uint32_t i = b; i < e && i < (uint32_t)n; ++i)
    rank += unordered[i] < (uint32_t)s;
  if (b + rank < (uint32_t)n)
    members[b + rank] = (uint32_t)s;
}

// ---- plan --------------------------------------------------------------------------------------------------------------
// Work split: a realistic radius (1.5 - 4 sector pitches) gives a failed sector 8 - 50 neighbours, found among the 20 - 150
// members of its 3 x 3 cells.  One lane per failed sector would walk them one after the other, each a dependent chain of
// cell start -> member -> flag -> centre -> record loads; a wavefront per sector would leave three quarters of its lanes
// without a candidate.  A 16-lane row takes a row of three cells (contiguous in the member table) 16 candidates at a
// time - two to three trips per cell row - and four failed sectors share a wavefront.  Lane l of the row sums the candidates
// it is dealt in order; the sixteen partial sums are joined by a fixed butterfly (xor 8, 4, 2, 1: both partners add the
// same two numbers, so all lanes hold the same bits).  Sectors are taken by position (row r of the grid = sector r): a good
// sector's row retires after one byte load, which costs less than building a list of the failed ones first.
__global__ __launch_bounds__(kBlock) void lk_reseed_plan_kernel(LkReseedPlanArgs a) {
  const int lane = (int)(threadIdx.x & (kLkReseedGroup - 1));
  const int s = (int)((blockIdx.x * kBlock + threadIdx.x) / kLkReseedGroup);
  if (s >= a.n_sectors)
    return;
  const int P = n_params_of(a.model);
  if (a.good[s]) { // (the whole row leaves together)
    if (lane == 0) {
      a.retry[s] = 0;
      a.nbrs[s] = 0;
      if (a.plan_info) {
        a.plan_info[s].status = LK_RESEED_GOOD;
        a.plan_info[s].neighbours = 0;
      }
    }
    return;
  }
  const LkReseedGrid &g = a.grid;
  const float2 cs = a.center[s];
  const double r2 = a.radius * a.radius;
  double acc[6] = {0, 0, 0, 0, 0, 0};
  int cnt = 0;
  walk_members<kLkReseedGroup>(g, cell_range_of(g, s), (uint32_t)a.n_sectors, lane, [&](uint32_t m) {
    if (!a.good[m])
      return;
    const float2 cn = a.center[m];
    const double dx = (double)cs.x - (double)cn.x, dy = (double)cs.y - (double)cn.y;
    if (!(dx * dx + dy * dy <= r2))
      return;
    const float *p = a.rec[m].resultingParameters;
    double q[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < P; ++i)
      q[i] = (double)p[i];
    if (a.model == LK_FM_UVUXUYVXVY) { // (lk_guess_kernel's rule, manager_class.cpp:2602-2707)
      q[0] = q[0] + (dx * q[2] + dy * q[3]);
      q[1] = q[1] + (dx * q[4] + dy * q[5]);
    } else if (a.model == LK_FM_UVQ) {
      q[0] = q[0] + (-dy * q[2]);
      q[1] = q[1] + dx * q[2];
    }
    for (int i = 0; i < 6; ++i)
      acc[i] += q[i];
    ++cnt;
  });
  for (int m = kLkReseedGroup / 2; m >= 1; m >>= 1) {
    for (int i = 0; i < 6; ++i)
      acc[i] += __shfl_xor(acc[i], m, kLkReseedGroup);
    cnt += __shfl_xor(cnt, m, kLkReseedGroup);
  }
  if (lane != 0)
    return;
  const bool enough = cnt >= a.min_neighbours;
  const bool retry = enough && cnt > a.tried[s];
  a.nbrs[s] = cnt;
  a.retry[s] = retry ? 1 : 0;
  if (retry)
    for (int i = 0; i < 6; ++i)
      a.guess[(size_t)s * 6 + i] = i < P ? (float)(acc[i] / (double)cnt) : 0.f;
  if (a.plan_info) {
    a.plan_info[s].status = enough ? LK_RESEED_PLANNED : LK_RESEED_NO_NEIGHBOUR;
    a.plan_info[s].neighbours = cnt;
  }
}

// ---- compact -----------------------------------------------------------------------------------------------------------
// One workgroup per range walks it 1024 entries at a time and keeps the flagged sectors in the engine's order (the order
// decides which sectors share a wavefront of the solve, so it must be the same on every run: no atomics here).
__global__ __launch_bounds__(kWide) void lk_reseed_compact_kernel(LkReseedCompactArgs a) {
  __shared__ uint32_t s_wave[kWide / kWave];
  const LkReseedRange r = a.range[blockIdx.x];
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
  uint32_t base = 0;
  for (int i0 = r.begin; i0 < r.end; i0 += kWide) {
    const int i = i0 + tid;
    const uint32_t s = i < r.end ? r.src[i] : 0u;
    const bool f = i < r.end && a.retry[s] != 0;
    const unsigned long long mask = __ballot(f);
    if (lane == 0)
      s_wave[w] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (int k = 0; k < kWide / kWave; ++k) {
      before += k < w ? s_wave[k] : 0u;
      total += s_wave[k];
    }
    if (f) // base + before + ... < the flagged entries so far <= i - r.begin + 1: inside the range
      r.dst[(uint32_t)r.begin + base + before + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = s;
    base += total;
    __syncthreads();
  }
  if (tid == 0)
    a.count[blockIdx.x] = base;
}

// ---- merge -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void lk_reseed_merge_kernel(LkReseedMergeArgs a) {
  const int s = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (s >= a.n_sectors || !a.retry[s])
    return;
  const lk_result fresh = a.fresh[s], old = a.rec[s];
  bool accept = reseed_good(fresh, a.n_params, a.chi_max);
  if (accept && old.errorCode == LK_ERROR_NONE && finite_bits(old.chi))
    accept = fresh.chi < old.chi;
  const int nb = a.nbrs[s];
  a.tried[s] = nb;
  atomicAdd(a.totals + 0, 1ull);
  for (int i = 0; i < 4; ++i)
    atomicAdd(a.totals + 1 + i, (unsigned long long)a.stats[(size_t)s * 4 + i]);
  lk_reseed_info o = a.info[s];
  o.neighbours = nb;
  if (accept) {
    a.rec[s] = fresh;
    a.good[s] = 1;
    o.status = LK_RESEED_RECOVERED;
    o.round = a.round;
    atomicAdd(a.totals + 5, 1ull);
  } else {
    for (int i = 0; i < 6; ++i) {
      a.last_p[(size_t)s * 6 + i] = a.keep_last_p[(size_t)s * 6 + i];
      a.last_eval_p[(size_t)s * 6 + i] = a.keep_last_eval_p[(size_t)s * 6 + i];
    }
    for (int i = 0; i < 4; ++i)
      a.stats[(size_t)s * 4 + i] = a.keep_stats[(size_t)s * 4 + i];
    o.status = LK_RESEED_NOT_IMPROVED;
  }
  a.info[s] = o;
}

} // namespace

hipError_t lk_launch_reseed_bbox(const float2 *center, int n_sectors, float *out4, hipStream_t st) {
  hipLaunchKernelGGL(lk_reseed_bbox_kernel, dim3(1), dim3(kWide), 0, st, center, n_sectors, out4);
  return hipGetLastError();
}

hipError_t lk_launch_reseed_classify(const lk_result *rec, int n_sectors, int n_params, float chi_max, uint8_t *good,
                                     int32_t *tried, lk_reseed_info *info, uint32_t *n_failed, hipStream_t st) {
  if (n_sectors <= 0)
    return hipSuccess;
  hipLaunchKernelGGL(lk_reseed_classify_kernel, dim3(blocks_for(n_sectors, kBlock)), dim3(kBlock), 0, st, rec, n_sectors,
                     n_params, chi_max, good, tried, info, n_failed);
  return hipGetLastError();
}

hipError_t lk_launch_reseed_grid(const float2 *center, int n_sectors, double x0, double y0, double cell, int nx, int ny,
                                 uint32_t *cell_of, uint32_t *start, uint32_t *cursor, uint32_t *unordered, uint32_t *members,
                                 hipStream_t st) {
  if (n_sectors <= 0 || nx <= 0 || ny <= 0)
    return hipErrorInvalidValue;
  const int n_cells = nx * ny;
  hipError_t err = hipMemsetAsync(start, 0, ((size_t)n_cells + 1) * sizeof(uint32_t), st);
  if (err != hipSuccess)
    return err;
  const dim3 grid(blocks_for(n_sectors, kBlock)), block(kBlock);
  hipLaunchKernelGGL(lk_reseed_cell_count_kernel, grid, block, 0, st, center, n_sectors, x0, y0, cell, nx, ny, cell_of, start);
  hipLaunchKernelGGL(lk_reseed_scan_kernel, dim3(1), dim3(kWide), 0, st, start, cursor, n_cells);
  hipLaunchKernelGGL(lk_reseed_scatter_kernel, grid, block, 0, st, cell_of, n_sectors, cursor, unordered);
  hipLaunchKernelGGL(lk_reseed_order_kernel, grid, block, 0, st, cell_of, start, unordered, n_sectors, members);
  return hipGetLastError();
}

hipError_t lk_launch_reseed_plan(const LkReseedPlanArgs &a, hipStream_t st) {
  if (a.n_sectors <= 0)
    return hipSuccess;
  hipLaunchKernelGGL(lk_reseed_plan_kernel, dim3(blocks_for(a.n_sectors, kBlock / kLkReseedGroup)), dim3(kBlock), 0, st, a);
  return hipGetLastError();
}

hipError_t lk_launch_reseed_compact(const LkReseedCompactArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(lk_reseed_compact_kernel, dim3(kLkReseedRanges), dim3(kWide), 0, st, a);
  return hipGetLastError();
}

hipError_t lk_launch_reseed_merge(const LkReseedMergeArgs &a, hipStream_t st) {
  if (a.n_sectors <= 0)
    return hipSuccess;
  hipLaunchKernelGGL(lk_reseed_merge_kernel, dim3(blocks_for(a.n_sectors, kBlock)), dim3(kBlock), 0, st, a);
  return hipGetLastError();
}
