// lk_lens.hip - device side of the lens distortion (include/lk_engine.h: lk_lens_fit, lk_lens_correct).
//
//   prep     lk_strain.hip's pack, a thread per (frame, sector): the good rule once per record, {cx, cy, u, v} in 16 bytes
//            (cx = NaN marks a sector that is not good)
//   sums     one workgroup per (chunk, frame): sector chunk * size + i goes to lane i mod 256; a lane forms the two rows of
//            lk_lens.hpp for every member it is dealt, in ascending order, and adds their products to its own upper triangle
//            (45, 66 or 91 doubles in registers); the butterfly joins a wavefront, LDS the four wavefronts in ascending order.
//            partial[F][chunks][len] = {n, the triangle, n_outside}.
//   join     a thread per (frame, entry) adds the partials by ascending chunk index
//   correct  a thread per (frame, sector): lk_lens_correct_params on the good records, a copy otherwise
// An evaluation of the fit is sums -> join; the kernel boundary on the stream is the only ordering.  What it costs is its
// read of the pack, 16 bytes per (frame, sector), and some 1500 double operations per member.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lk_device.hpp"
#include "lk_launch.hpp"
#include "lk_lens.hpp"
#include "lk_neighbours.hpp"

namespace {

constexpr int kWaves = kBlock / 64;

template <int Q> __global__ __launch_bounds__(kBlock) void lk_lens_sums_kernel(LkLensFitArgs a) {
  constexpr int W = lk_lens_width(Q), T = lk_lens_triangle(Q), LEN = lk_lens_sums_len(Q);
  __shared__ double lds[kWaves][LEN];
  const int chunk = (int)blockIdx.x, f = (int)blockIdx.y;
  const int tid = (int)threadIdx.x;
  const size_t S = (size_t)a.n_sectors;
  const float4 *pack = a.pack + (size_t)f * S;
  const long long first = (long long)chunk * a.chunk;
  const long long end = first + a.chunk < (long long)S ? first + a.chunk : (long long)S;
  double nu[6];
#pragma unroll
  for (int i = 0; i < 6; ++i)
    nu[i] = a.nuisance[(size_t)f * 6 + i];

  double acc[T];
#pragma unroll
  for (int k = 0; k < T; ++k)
    acc[k] = 0.0;
  double n = 0.0, n_outside = 0.0;
  for (long long j = first + tid; j < end; j += kBlock) {
    const float4 c = pack[j];
    if (c.x == c.x && (!a.fit_mask || a.fit_mask[j])) {
      double ax[W], ay[W];
      if (lk_lens_rows<Q>(a.lens, nu, a.ox, a.oy, (double)c.x, (double)c.y, (double)c.z, (double)c.w, ax, ay)) {
        n_outside += 1.0;
      } else {
        n += 1.0;
        int k = 0;
#pragma unroll
        for (int i = 0; i < W; ++i)
#pragma unroll
          for (int l = i; l < W; ++l)
            acc[k++] += ax[i] * ax[l] + ay[i] * ay[l];
      }
    }
  }

  // join: the butterfly within a wavefront, then the wavefronts in ascending order
  const int wave = tid >> 6, lane = tid & 63;
  for (int m = 32; m >= 1; m >>= 1) {
    n += __shfl_xor(n, m, 64);
    n_outside += __shfl_xor(n_outside, m, 64);
  }
#pragma unroll
  for (int k = 0; k < T; ++k)
    for (int m = 32; m >= 1; m >>= 1)
      acc[k] += __shfl_xor(acc[k], m, 64);
  if (lane == 0) {
    lds[wave][0] = n;
#pragma unroll
    for (int k = 0; k < T; ++k)
      lds[wave][1 + k] = acc[k];
    lds[wave][T + 1] = n_outside;
  }
  __syncthreads();
  if (tid < LEN) {
    double t = lds[0][tid];
    for (int w = 1; w < kWaves; ++w)
      t += lds[w][tid];
    a.partial[((size_t)f * (size_t)a.chunks + (size_t)chunk) * LEN + tid] = t;
  }
}

__global__ __launch_bounds__(kBlock) void lk_lens_join_kernel(LkLensFitArgs a, int len) {
  const int i = (int)(blockIdx.x * kBlock + threadIdx.x), f = (int)blockIdx.y;
  if (i >= len)
    return;
  const double *p = a.partial + (size_t)f * (size_t)a.chunks * (size_t)len + i;
  double t = 0.0;
  for (int c = 0; c < a.chunks; ++c)
    t += p[(size_t)c * (size_t)len];
  a.sums[(size_t)f * (size_t)len + i] = t;
}

__global__ __launch_bounds__(kBlock) void lk_lens_correct_kernel(LkLensCorrectArgs a) {
  const int s = (int)(blockIdx.x * kBlock + threadIdx.x), f = (int)blockIdx.y;
  if (s >= a.n_sectors)
    return;
  const size_t i = (size_t)f * (size_t)a.n_sectors + (size_t)s;
  // a 48-byte record as three float4 (records of hipMalloc'ed arrays: 16-byte aligned): {p0 .. p3}, {p4, p5, chi, points},
  // {iterations, error code, undCenter}
  const float4 *in = (const float4 *)(a.rec + i);
  const float4 r0 = in[0], r1 = in[1], r2 = in[2];
  float p0 = r0.x, p1 = r0.y, p2 = r0.z, p3 = r0.w, p4 = r1.x, p5 = r1.y;
  const float2 c = a.center[s];
  const float x = a.pack[i].x; // (NaN: the record is not good)
  int status = 1;
  if (x == x)
    status = lk_lens_correct_params(a.model, a.lens, c.x, c.y, p0, p1, p2, p3, p4, p5);
  float4 *o = (float4 *)(a.rec_out + i);
  o[0] = make_float4(p0, p1, p2, p3), o[1] = make_float4(p4, p5, r1.z, r1.w), o[2] = r2;
  if (a.status)
    a.status[i] = (uint8_t)status;
  if (f == 0 && a.centres_out) {
    LkLensJac J;
    double xu, yu;
    const bool outside = lk_lens_undistort_point(a.lens, (double)c.x, (double)c.y, xu, yu, J) != 0;
    a.centres_out[s] = outside ? c : make_float2((float)xu, (float)yu);
  }
}

} // namespace

hipError_t lk_launch_lens_sums(const LkLensFitArgs &a, hipStream_t st) {
  if (a.n_frames <= 0 || a.n_sectors <= 0)
    return hipSuccess;
  if (a.chunk < 1 || a.chunks != (int)blocks_for(a.n_sectors, a.chunk) || a.n_frames > 65535)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)a.chunks, (unsigned)a.n_frames), block(kBlock);
  int len = 0;
  switch (a.nuisance_kind) {
  case LK_LENS_TRANSLATION:
    len = lk_lens_sums_len(2);
    hipLaunchKernelGGL((lk_lens_sums_kernel<2>), grid, block, 0, st, a);
    break;
  case LK_LENS_SIMILARITY:
    len = lk_lens_sums_len(4);
    hipLaunchKernelGGL((lk_lens_sums_kernel<4>), grid, block, 0, st, a);
    break;
  case LK_LENS_AFFINE:
    len = lk_lens_sums_len(6);
    hipLaunchKernelGGL((lk_lens_sums_kernel<6>), grid, block, 0, st, a);
    break;
  default:
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(lk_lens_join_kernel, dim3(blocks_for(len, kBlock), (unsigned)a.n_frames), block, 0, st, a, len);
  return hipGetLastError();
}

hipError_t lk_launch_lens_correct(const LkLensCorrectArgs &a, hipStream_t st) {
  if (a.n_frames <= 0 || a.n_sectors <= 0)
    return hipSuccess;
  if (a.n_frames > 65535)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(lk_lens_correct_kernel, dim3(blocks_for(a.n_sectors, kBlock), (unsigned)a.n_frames), dim3(kBlock), 0, st, a);
  return hipGetLastError();
}
