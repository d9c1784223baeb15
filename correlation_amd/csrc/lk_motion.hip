// lk_motion.hip - device side of the global motion per frame (include/lk_engine.h: lk_rigid_motion).
//
// Per frame: the count and the eleven plane-fit sums over the fit set (good sectors under the mask, minus what the pass
// before trimmed), the fit of lk_motion.hpp, the residuals of the fit set to it, and - where asked - every good record with
// the motion taken out.
//   prep     lk_strain.hip's pack, a thread per (frame, sector): the good rule once per record, {cx, cy, u, v} in 16 bytes
//            (cx = NaN marks a sector that is not good)
//   sums     one workgroup per (chunk, frame): sector chunk * size + i goes to lane i mod 256, every lane adds what it is
//            dealt in ascending order; PlaneSums' butterfly joins a wavefront, LDS the four wavefronts in ascending order.
//            RESIDUAL = false: membership (written to `keep`), the count, the 11 sums and the sectors trimmed;
//            RESIDUAL = true: sum r^2 and max r^2 of the kept sectors to the running fit.  partial[F][chunks][14].
//   fit      a thread per frame adds the partials by ascending chunk index and calls lk_motion_fit_impl, or closes the
//            residual pass (rms, max, the next pass's threshold)
//   remove   a thread per (frame, sector): lk_motion_remove_impl on the good records of an OK frame, a copy otherwise
// A pass is sums -> fit -> sums<RESIDUAL> -> fit<RESIDUAL>; the kernel boundaries on the stream are the only ordering.
// What a pass costs is its read of the pack: 16 bytes per (frame, sector) and kernel, plus the keep byte.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lk_device.hpp"
#include "lk_launch.hpp"
#include "lk_motion.hpp"
#include "lk_neighbours.hpp"

namespace {

constexpr int kWaves = kBlock / 64;

template <bool RESIDUAL> __global__ __launch_bounds__(kBlock) void lk_motion_sums_kernel(LkMotionArgs a) {
  __shared__ double lds[kWaves][13];
  const int chunk = (int)blockIdx.x, f = (int)blockIdx.y;
  const int tid = (int)threadIdx.x;
  const size_t S = (size_t)a.n_sectors;
  const float4 *pack = a.pack + (size_t)f * S;
  uint8_t *keep = a.keep + (size_t)f * S;
  const long long first = (long long)chunk * a.chunk;
  const long long end = first + a.chunk < (long long)S ? first + a.chunk : (long long)S;
  // the fit the running pass trims against (pass > 0) or measures its residuals to: the same bits in every lane
  LkMotionFit fit;
  fit.status = LK_MOTION_OK;
  fit.threshold = (double)INFINITY;
  const bool use_fit = RESIDUAL || a.pass > 0;
  if (use_fit)
    fit = a.fit[f];
  const bool fit_ok = fit.status == LK_MOTION_OK;

  PlaneSums sums;
  double rr = 0.0, rmax = 0.0, trimmed = 0.0;
  for (long long j = first + tid; j < end; j += kBlock) {
    const float4 c = pack[j];
    const double x = (double)c.x - a.ox, y = (double)c.y - a.oy, u = (double)c.z, v = (double)c.w;
    if (RESIDUAL) {
      if (keep[j] && fit_ok) {
        const double r2 = lk_motion_residual2(fit, x, y, u, v);
        rr += r2;
        rmax = r2 > rmax ? r2 : rmax;
      }
    } else {
      bool in = c.x == c.x && (!a.fit_mask || a.fit_mask[j]);
      if (in && a.pass > 0 && fit_ok && sqrt(lk_motion_residual2(fit, x, y, u, v)) > fit.threshold) {
        in = false;
        trimmed += 1.0;
      }
      keep[j] = in ? 1 : 0;
      if (in)
        sums.add(x, y, u, v);
    }
  }

  // join: the butterfly within a wavefront, then the wavefronts in ascending order
  const int wave = tid >> 6, lane = tid & 63;
  if (RESIDUAL) {
    for (int m = 32; m >= 1; m >>= 1) {
      rr += __shfl_xor(rr, m, 64);
      const double o = __shfl_xor(rmax, m, 64);
      rmax = o > rmax ? o : rmax;
    }
    if (lane == 0)
      lds[wave][0] = rr, lds[wave][1] = rmax;
  } else {
    sums.template join<64>();
    for (int m = 32; m >= 1; m >>= 1)
      trimmed += __shfl_xor(trimmed, m, 64);
    if (lane == 0) {
      lds[wave][0] = (double)sums.n;
      for (int i = 0; i < 11; ++i)
        lds[wave][1 + i] = sums.s[i];
      lds[wave][12] = trimmed;
    }
  }
  __syncthreads();
  constexpr int kUsed = RESIDUAL ? 2 : 13;
  if (tid < kLkMotionPartial) {
    double t = 0.0;
    if (tid < kUsed) {
      t = lds[0][tid];
      for (int w = 1; w < kWaves; ++w) {
        const double o = lds[w][tid];
        t = RESIDUAL && tid == 1 ? (o > t ? o : t) : t + o;
      }
    }
    a.partial[((size_t)f * (size_t)a.chunks + (size_t)chunk) * kLkMotionPartial + tid] = t;
  }
}

template <bool RESIDUAL> __global__ __launch_bounds__(kBlock) void lk_motion_fit_kernel(LkMotionArgs a) {
  const int f = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (f >= a.n_frames)
    return;
  // a frame that an earlier pass found not OK keeps that pass's record, sums and fit
  if ((RESIDUAL || a.pass > 0) && a.fit[f].status != LK_MOTION_OK)
    return;
  const double *p = a.partial + (size_t)f * (size_t)a.chunks * kLkMotionPartial;
  if (RESIDUAL) {
    double rr = 0.0, rmax = 0.0;
    for (int c = 0; c < a.chunks; ++c) {
      rr += p[(size_t)c * kLkMotionPartial];
      const double o = p[(size_t)c * kLkMotionPartial + 1];
      rmax = o > rmax ? o : rmax;
    }
    const double rms = sqrt(rr / (double)a.fit[f].n);
    a.fit[f].threshold = a.reject > 0.0 ? a.reject * rms : (double)INFINITY;
    a.out[f].rms = (float)rms;
    a.out[f].max_residual = (float)sqrt(rmax);
    return;
  }
  double t[13];
  for (int i = 0; i < 13; ++i)
    t[i] = 0.0;
  for (int c = 0; c < a.chunks; ++c)
    for (int i = 0; i < 13; ++i)
      t[i] += p[(size_t)c * kLkMotionPartial + i];
  const int n = (int)t[0];
  lk_motion m;
  const LkMotionFit fit = lk_motion_fit_impl(a.kind, a.min_sectors, n, t + 1, a.ox, a.oy, &m);
  m.n_rejected = (int)t[12];
  m.passes_run = a.pass + 1;
  a.fit[f] = fit;
  for (int i = 0; i < 12; ++i)
    a.sums[(size_t)f * 12 + i] = t[i];
  float4 *o = (float4 *)(a.out + f); // (64-byte records in hipMalloc'ed memory: 16-byte aligned)
  o[0] = make_float4(m.cx, m.cy, m.tx, m.ty);
  o[1] = make_float4(m.axx, m.axy, m.ayx, m.ayy);
  o[2] = make_float4(m.theta, m.scale, m.rms, m.max_residual);
  o[3] = make_float4(__int_as_float(m.n_fit), __int_as_float(m.n_rejected), __int_as_float(m.status), __int_as_float(m.passes_run));
}

__global__ __launch_bounds__(kBlock) void lk_motion_remove_kernel(LkMotionArgs a) {
  const int s = (int)(blockIdx.x * kBlock + threadIdx.x), f = (int)blockIdx.y;
  if (s >= a.n_sectors)
    return;
  const size_t i = (size_t)f * (size_t)a.n_sectors + (size_t)s;
  // a 48-byte record as three float4 (records of hipMalloc'ed arrays: 16-byte aligned): {p0 .. p3}, {p4, p5, chi, points},
  // {iterations, error code, undCenter}
  const float4 *in = (const float4 *)(a.rec + i);
  const float4 r0 = in[0], r1 = in[1], r2 = in[2];
  float p0 = r0.x, p1 = r0.y, p2 = r0.z, p3 = r0.w, p4 = r1.x, p5 = r1.y;
  const lk_motion &m = a.out[f];
  const float x = a.pack[i].x; // (NaN: the record is not good)
  if (m.status == LK_MOTION_OK && x == x) {
    const float2 c = a.center[s];
    (void)lk_motion_remove_params(a.model, m, c.x, c.y, p0, p1, p2, p3, p4, p5);
  }
  float4 *o = (float4 *)(a.rec_out + i);
  o[0] = make_float4(p0, p1, p2, p3), o[1] = make_float4(p4, p5, r1.z, r1.w), o[2] = r2;
}

} // namespace

hipError_t lk_launch_motion_pass(const LkMotionArgs &a, hipStream_t st) {
  if (a.n_frames <= 0 || a.n_sectors <= 0)
    return hipSuccess;
  if (a.chunk < 1 || a.chunks != (int)blocks_for(a.n_sectors, a.chunk) || a.n_frames > 65535)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)a.chunks, (unsigned)a.n_frames), block(kBlock), frames(blocks_for(a.n_frames, kBlock));
  hipLaunchKernelGGL((lk_motion_sums_kernel<false>), grid, block, 0, st, a);
  hipLaunchKernelGGL((lk_motion_fit_kernel<false>), frames, block, 0, st, a);
  hipLaunchKernelGGL((lk_motion_sums_kernel<true>), grid, block, 0, st, a);
  hipLaunchKernelGGL((lk_motion_fit_kernel<true>), frames, block, 0, st, a);
  return hipGetLastError();
}

hipError_t lk_launch_motion_remove(const LkMotionArgs &a, hipStream_t st) {
  if (a.n_frames <= 0 || a.n_sectors <= 0)
    return hipSuccess;
  if (a.n_frames > 65535)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(lk_motion_remove_kernel, dim3(blocks_for(a.n_sectors, kBlock), (unsigned)a.n_frames), dim3(kBlock), 0, st, a);
  return hipGetLastError();
}
