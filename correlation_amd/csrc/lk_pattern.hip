// lk_pattern.hip - device side of the speckle-quality pass (include/lk_engine.h: lk_pattern_quality, lk_suggest_subset;
// DESIGN.md section 21).  Everything is integer arithmetic on the u8 pixels of ONE image slot at level L = py_start; the
// definitions of gx2, gy2 and the sums are in lk_pattern.hpp.
//
// sectors     lk_residual.hip's photometry walk with other sums: one lane group per sector (16 / 64 / 512 lanes from the
//             level-0 sample count), lane j takes the samples j, j + G, ...  A sample is its node (int)(q + 0.5f), clamped,
//             and the node's four clamped neighbours.  The seven integer sums, min and max are carried in int64 per lane and
//             reduced as doubles by reduce_f64: every partial sum is an integer below 2^53 (|Gxy| <= 255^2 n < 2^47 for an
//             int32 count), so each addition is exact and the result does not depend on the order.  The one real double sum,
//             sum sqrt(gx2^2 + gy2^2), takes the eighth slot of the same reduction and has its fixed order.  Lane 0 turns
//             them into the record with the function the host exports (lk_pattern.hpp).
// table       two uint32 planes, the summed-area tables of gx2^2 and gy2^2 over the whole image, built on every call:
//   row step  a workgroup per image row.  A thread forms the squares of kLkSatPixels consecutive pixels on the fly from the
//             u8 rows y - 1, y, y + 1, scans them in registers, the wavefront scans the threads' totals with __shfl_up
//             (wave64), the wavefronts' totals cross through LDS, and a row longer than kLkSatRowTile pixels carries its
//             running total into the next pass.  One aligned 16-byte store per thread and plane.
//   column    the lanes stay across the columns (four columns per lane, a wavefront reads and writes whole 1 KiB row
//   step      pieces), the rows are cut into bands of kLkSatBandRows: (1) the column totals of every band, (2) their
//             exclusive prefix over the bands - rows / kLkSatBandRows serial steps on a table 1 / kLkSatBandRows the
//             size, (3) every band scanned down its rows from its prefix, in place.
//             The kernel boundaries on the stream are the only ordering between workgroups: nothing waits on a flag.
// query       a thread per point: the node, then per candidate half-width the clipped box, its two sums from the four
//             corners (differences modulo 2^32: exact, lk_pattern.hpp), the pass rule on integers; the smallest passing
//             candidate or, without one, the largest.  Without sums_out the scan stops at the first pass.
#include "lk_device.hpp"
#include "lk_launch.hpp"
#include "lk_neighbours.hpp"
#include "lk_pattern.hpp"
#include "lk_sector_eval.hpp"

namespace {

constexpr int kPatAdds = 8;       // the seven integer sums and the gradient-magnitude sum; slots 8, 9 are max I and max -I
constexpr int kPatMaxes = 2;
constexpr int kPatLdsStride = 10; // doubles per wavefront in the cross-wavefront reduction

__device__ __forceinline__ int pixel(gptr<uint8_t> img, int cols, int x, int y) { return (int)img[(size_t)y * (size_t)cols + (size_t)x]; }

template <int GROUP> __global__ void __launch_bounds__(GROUP <= 64 ? 256 : GROUP) lk_pattern_kernel(LkPatternArgs a) {
  constexpr int THREADS = GROUP <= 64 ? 256 : GROUP;
  __shared__ double lds[(GROUP > 64 ? GROUP / kWave : 1) * kPatLdsStride];
  const int gid = (int)blockIdx.x * (THREADS / GROUP) + (int)threadIdx.x / GROUP;
  const int lane = (int)threadIdx.x % GROUP;
  if (gid >= a.n_sectors) // (GROUP == 512: the whole workgroup; GROUP <= 64: whole rows / wavefronts, no barriers below)
    return;
  const int s = (int)a.ev.order[gid];
  const SectorLevel c = sector_level(a.ev, s, a.level, a.ev.center[s]);
  const int n = c.n, rows = c.urows, cols = c.ucols;
  long long t[7] = {0, 0, 0, 0, 0, 0, 0};
  int lo = 255, hi = 0;
  double mig = 0.0;
  for (int k = lane; k < n; k += GROUP) {
    const f32x2 q = sector_sample(c, k);
    int x = (int)(q.x + 0.5f), y = (int)(q.y + 0.5f); // the node rule of sector_und_node
    x = min(max(x, 0), cols - 1);                     // (memory safety only; valid lists never clamp)
    y = min(max(y, 0), rows - 1);
    const int I = pixel(c.und, cols, x, y);
    const int gx2 = pixel(c.und, cols, min(x + 1, cols - 1), y) - pixel(c.und, cols, max(x - 1, 0), y);
    const int gy2 = pixel(c.und, cols, x, min(y + 1, rows - 1)) - pixel(c.und, cols, x, max(y - 1, 0));
    t[0] += I;
    t[1] += I * I;
    t[2] += gx2 * gx2;
    t[3] += gy2 * gy2;
    t[4] += gx2 * gy2;
    t[5] += I <= a.grey_low ? 1 : 0;
    t[6] += I >= a.grey_high ? 1 : 0;
    lo = min(lo, I);
    hi = max(hi, I);
    mig += sqrt((double)(gx2 * gx2 + gy2 * gy2));
  }
  double v[kPatAdds + kPatMaxes];
#pragma unroll
  for (int i = 0; i < 7; ++i)
    v[i] = (double)t[i]; // exact, and so is every partial sum of the reduction
  v[7] = mig;
  v[8] = (double)hi;
  v[9] = (double)-lo;
  reduce_f64<GROUP, kPatAdds, kPatMaxes, kPatLdsStride>(v, lds);
  if (lane != 0)
    return;
  int64_t sums[kLkPatternSums];
#pragma unroll
  for (int i = 0; i < 7; ++i)
    sums[i] = (int64_t)v[i];
  sums[7] = n > 0 ? (int64_t)-v[9] : 0;
  sums[8] = n > 0 ? (int64_t)v[8] : 0;
  struct lk_pattern r;
  lk_pattern_record(n, sums, v[7], a.noise_sigma, a.max_saturated, &r);
  a.out[s] = r;
  if (a.sums) {
#pragma unroll
    for (int i = 0; i < kLkPatternSums; ++i)
      a.sums[(size_t)s * kLkPatternSums + i] = sums[i];
  }
  if (a.mig_sum)
    a.mig_sum[s] = v[7];
}

// ---- the tables: row step --------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_scan_inclusive(uint32_t v, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d *= 2) {
    const uint32_t o = (uint32_t)__shfl_up((int)v, d, kWave);
    if (lane >= d)
      v += o;
  }
  return v;
}

__global__ void __launch_bounds__(kLkSatThreads) lk_sat_rows_kernel(LkSatArgs a) {
  constexpr int WAVES = kLkSatThreads / kWave;
  __shared__ uint32_t wave_total[2][WAVES];
  const int tid = (int)threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const int y = (int)blockIdx.x; // < rows: the grid is the rows
  const int rows = a.rows, cols = a.cols, pitch = a.pitch;
  const gptr<uint8_t> mid = (gptr<uint8_t>)a.img + (size_t)y * (size_t)cols;
  const gptr<uint8_t> up = (gptr<uint8_t>)a.img + (size_t)max(y - 1, 0) * (size_t)cols;
  const gptr<uint8_t> down = (gptr<uint8_t>)a.img + (size_t)min(y + 1, rows - 1) * (size_t)cols;
  uint32_t *const out_x = a.table + (size_t)y * (size_t)pitch;
  uint32_t *const out_y = out_x + (size_t)rows * (size_t)pitch;
  uint32_t carry_x = 0, carry_y = 0;
  for (int x0 = 0; x0 < pitch; x0 += kLkSatRowTile) { // (uniform over the workgroup: the barriers below are met by all)
    const int x = x0 + tid * kLkSatPixels;
    uint32_t sx[kLkSatPixels], sy[kLkSatPixels];
#pragma unroll
    for (int i = 0; i < kLkSatPixels; ++i) {
      const int xi = x + i;
      sx[i] = sy[i] = 0; // (a column of the padding adds nothing)
      if (xi < cols) {
        const int gx2 = (int)mid[min(xi + 1, cols - 1)] - (int)mid[max(xi - 1, 0)];
        const int gy2 = (int)down[xi] - (int)up[xi];
        sx[i] = (uint32_t)(gx2 * gx2);
        sy[i] = (uint32_t)(gy2 * gy2);
      }
    }
#pragma unroll
    for (int i = 1; i < kLkSatPixels; ++i) {
      sx[i] += sx[i - 1];
      sy[i] += sy[i - 1];
    }
    const uint32_t tx = sx[kLkSatPixels - 1], ty = sy[kLkSatPixels - 1];
    const uint32_t ix = wave_scan_inclusive(tx, lane), iy = wave_scan_inclusive(ty, lane);
    if (lane == kWave - 1) {
      wave_total[0][wave] = ix;
      wave_total[1][wave] = iy;
    }
    __syncthreads();
    uint32_t before_x = carry_x + (ix - tx), before_y = carry_y + (iy - ty);
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      const uint32_t wx = wave_total[0][w], wy = wave_total[1][w];
      if (w < wave) {
        before_x += wx;
        before_y += wy;
      }
      carry_x += wx;
      carry_y += wy;
    }
    if (x < pitch) { // (x and pitch are multiples of 4: the four words are inside the row, 16-byte aligned)
      *(uint4 *)(out_x + x) = make_uint4(before_x + sx[0], before_x + sx[1], before_x + sx[2], before_x + sx[3]);
      *(uint4 *)(out_y + x) = make_uint4(before_y + sy[0], before_y + sy[1], before_y + sy[2], before_y + sy[3]);
    }
    __syncthreads(); // the next pass writes wave_total again
  }
}
static_assert(kLkSatPixels == 4, "a thread's pixels are one uint4 of each plane");

// ---- the tables: column step -------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint4 add4(uint4 p, uint4 q) { return make_uint4(p.x + q.x, p.y + q.y, p.z + q.z, p.w + q.w); }

// grid (column pieces, bands, 2 planes); MODE 0: band[plane][b][x] = the column totals of band b; MODE 2: the band scanned
// down its rows, in place, from band[plane][b][x]
template <int MODE> __global__ void __launch_bounds__(kLkSatColThreads) lk_sat_band_kernel(LkSatArgs a) {
  const int x = ((int)blockIdx.x * kLkSatColThreads + (int)threadIdx.x) * 4;
  if (x >= a.pitch) // (no barrier in this kernel)
    return;
  const int b = (int)blockIdx.y, plane = (int)blockIdx.z;
  const int y0 = b * kLkSatBandRows, y1 = min(y0 + kLkSatBandRows, a.rows);
  uint32_t *const t = a.table + (size_t)plane * (size_t)a.rows * (size_t)a.pitch + (size_t)x;
  uint32_t *const tot = a.band + ((size_t)plane * (size_t)a.n_bands + (size_t)b) * (size_t)a.pitch + (size_t)x;
  uint4 acc = MODE == 0 ? make_uint4(0, 0, 0, 0) : *(const uint4 *)tot;
  constexpr int AHEAD = 8; // rows loaded before the first of them is added and stored: the loads of an in-place scan would
                           // otherwise wait behind the stores
  static_assert(kLkSatBandRows % AHEAD == 0, "a band is a whole number of row groups");
  for (int y = y0; y < y1; y += AHEAD) {
    uint4 v[AHEAD];
#pragma unroll
    for (int i = 0; i < AHEAD; ++i)
      v[i] = y + i < y1 ? *(const uint4 *)(t + (size_t)(y + i) * (size_t)a.pitch) : make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < AHEAD; ++i) {
      acc = add4(acc, v[i]);
      if (MODE == 2 && y + i < y1)
        *(uint4 *)(t + (size_t)(y + i) * (size_t)a.pitch) = acc;
    }
  }
  if (MODE == 0)
    *(uint4 *)tot = acc;
}

// grid (column pieces, 1, 2 planes): band[plane][b][x] = the totals of the bands before b
__global__ void __launch_bounds__(kLkSatColThreads) lk_sat_band_prefix_kernel(LkSatArgs a) {
  const int x = ((int)blockIdx.x * kLkSatColThreads + (int)threadIdx.x) * 4;
  if (x >= a.pitch)
    return;
  uint32_t *const tot = a.band + (size_t)blockIdx.z * (size_t)a.n_bands * (size_t)a.pitch + (size_t)x;
  uint4 run = make_uint4(0, 0, 0, 0);
  for (int b = 0; b < a.n_bands; ++b) {
    uint4 *const p = (uint4 *)(tot + (size_t)b * (size_t)a.pitch);
    const uint4 v = *p;
    *p = run;
    run = add4(run, v);
  }
}

// ---- the query ---------------------------------------------------------------------------------------------------------------
// the sum over the box [x0, x1] x [y0, y1] (inside the image) of one plane, modulo 2^32 = exactly (lk_pattern.hpp)
__device__ __forceinline__ uint32_t box_sum(const uint32_t *t, int pitch, int x0, int y0, int x1, int y1) {
  const uint32_t *const r1 = t + (size_t)y1 * (size_t)pitch;
  uint32_t v = r1[x1];
  if (x0 > 0)
    v -= r1[x0 - 1];
  if (y0 > 0) {
    const uint32_t *const r0 = t + (size_t)(y0 - 1) * (size_t)pitch;
    v -= r0[x1];
    if (x0 > 0)
      v += r0[x0 - 1];
  }
  return v;
}

__global__ void __launch_bounds__(kBlock) lk_subset_query_kernel(LkSubsetArgs a) {
  const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (i >= a.n_points)
    return;
  const float2 p = a.points[i];
  const int nx = lk_subset_node(p.x, a.cols), ny = lk_subset_node(p.y, a.rows);
  uint32_t *const sums = a.sums ? a.sums + (size_t)i * (size_t)a.n_cand * 2 : nullptr;
  struct lk_subset r;
  if (nx < 0 || ny < 0) {
    lk_subset_fill(&r, 0, LK_SUBSET_BAD_POINT, 0, 0, 0u, 0u, a.noise_sigma);
    a.out[i] = r;
    if (sums)
      for (int c = 0; c < 2 * a.n_cand; ++c)
        sums[c] = 0;
    return;
  }
  const uint32_t *const tx = a.table, *const ty = a.table + (size_t)a.rows * (size_t)a.pitch;
  bool found = false;
  for (int c = 0; c < a.n_cand; ++c) {
    const int h = a.half_min + c * a.half_step; // <= LK_PATTERN_MAX_HALF (checked by the host)
    const int x0 = max(nx - h, 0), x1 = min(nx + h, a.cols - 1), y0 = max(ny - h, 0), y1 = min(ny + h, a.rows - 1);
    const uint32_t gxx = box_sum(tx, a.pitch, x0, y0, x1, y1), gyy = box_sum(ty, a.pitch, x0, y0, x1, y1);
    if (sums) {
      sums[2 * c] = gxx;
      sums[2 * c + 1] = gyy;
    }
    const bool pass = gxx >= a.threshold && gyy >= a.threshold;
    if (!found && (pass || c == a.n_cand - 1)) { // the smallest passing candidate, or the largest one
      const int clipped = nx - h < 0 || ny - h < 0 || nx + h > a.cols - 1 || ny + h > a.rows - 1 ? 1 : 0;
      lk_subset_fill(&r, h, pass ? LK_SUBSET_OK : LK_SUBSET_NONE, (x1 - x0 + 1) * (y1 - y0 + 1), clipped, gxx, gyy, a.noise_sigma);
      found = pass;
      if (pass && !sums)
        break;
    }
  }
  a.out[i] = r;
}

} // namespace

hipError_t lk_launch_pattern(const LkPatternArgs &a, int group, hipStream_t st) {
  return dispatch_group(group, [&](auto g) {
    constexpr int G = decltype(g)::value;
    return launch_sector_groups<G>(lk_pattern_kernel<G>, a, a.n_sectors, st);
  });
}

hipError_t lk_launch_sat_build(const LkSatArgs &a, hipStream_t st) {
  if (a.rows < 1 || a.cols < 1 || a.pitch < a.cols || a.pitch % 4 != 0 || a.n_bands != (a.rows + kLkSatBandRows - 1) / kLkSatBandRows ||
      a.n_bands > 65535)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(lk_sat_rows_kernel, dim3((unsigned)a.rows), dim3(kLkSatThreads), 0, st, a);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess)
    return err;
  const unsigned pieces = (unsigned)blocks_for(a.pitch / 4, kLkSatColThreads);
  hipLaunchKernelGGL(lk_sat_band_kernel<0>, dim3(pieces, (unsigned)a.n_bands, 2), dim3(kLkSatColThreads), 0, st, a);
  if ((err = hipGetLastError()) != hipSuccess)
    return err;
  hipLaunchKernelGGL(lk_sat_band_prefix_kernel, dim3(pieces, 1, 2), dim3(kLkSatColThreads), 0, st, a);
  if ((err = hipGetLastError()) != hipSuccess)
    return err;
  hipLaunchKernelGGL(lk_sat_band_kernel<2>, dim3(pieces, (unsigned)a.n_bands, 2), dim3(kLkSatColThreads), 0, st, a);
  return hipGetLastError();
}

hipError_t lk_launch_subset_query(const LkSubsetArgs &a, hipStream_t st) {
  if (a.n_points < 1 || a.n_cand < 1)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(lk_subset_query_kernel, dim3(blocks_for(a.n_points, kBlock)), dim3(kBlock), 0, st, a);
  return hipGetLastError();
}
