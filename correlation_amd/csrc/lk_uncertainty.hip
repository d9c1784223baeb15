// lk_uncertainty.hip - per-sector uncertainty of the solved parameters (include/lk_engine.h: lk_parameter_uncertainty;
// DESIGN.md section 16).
//
// One lane group evaluates one sector once, at its record's parameters and at the finest level the solve reaches: a
// 16-lane DPP row, a wavefront or a 512-thread workgroup, chosen from the sector's level-0 sample count alone (lk_bw_group).
// A sample is the forward evaluation's - Warp<>::apply, sample_def<>, the residual against the undeformed node,
// Warp<>::jac, in float - and its products J_a J_b, J_a V, V^2 are formed and summed in double.  Lane j takes the samples
// j, j + G, j + 2G, ...; the reduction (DPP inside rows, readlane across rows, LDS across wavefronts) has one fixed
// order, so a sector's sums and record are the same bytes in any launch.  Lane 0 of the group turns the sums into the
// record with the function the host exports (lk_uncertainty.hpp).
#include "lk_device.hpp"
#include "lk_good.hpp"
#include "lk_launch.hpp"
#include "lk_solver_common.hpp"
#include "lk_uncertainty.hpp"

#include <type_traits>

namespace {

constexpr int kUncLdsStride = 32; // doubles per wavefront in the cross-wavefront reduction (29 used at most)

template <int CTRL> __device__ __forceinline__ double dpp_add_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
  return v + __hiloint2double(hi, lo);
}

__device__ __forceinline__ double readlane_f64(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// Sum of N doubles over the group, in the order of bw_reduce (lk_backward.hip); every lane ends with the same bits.
// GROUP <= 64 uses no barrier; GROUP == 512 is the whole (uniform) workgroup.
template <int GROUP, int N> __device__ __forceinline__ void unc_reduce(double (&v)[N], double *lds) {
#pragma unroll
  for (int i = 0; i < N; ++i)
    v[i] = dpp_add_f64<0xB1>(v[i]); // quad_perm [1,0,3,2]
#pragma unroll
  for (int i = 0; i < N; ++i)
    v[i] = dpp_add_f64<0x4E>(v[i]); // quad_perm [2,3,0,1]
#pragma unroll
  for (int i = 0; i < N; ++i)
    v[i] = dpp_add_f64<0x141>(v[i]); // row_half_mirror
#pragma unroll
  for (int i = 0; i < N; ++i)
    v[i] = dpp_add_f64<0x140>(v[i]); // row_mirror
  if constexpr (GROUP >= 64) {
#pragma unroll
    for (int i = 0; i < N; ++i)
      v[i] = (readlane_f64(v[i], 0) + readlane_f64(v[i], 16)) + (readlane_f64(v[i], 32) + readlane_f64(v[i], 48));
  }
  if constexpr (GROUP > 64) {
    static_assert(N <= kUncLdsStride, "reduction slot");
    constexpr int WAVES = GROUP / kWave;
    const int wave = (int)threadIdx.x / kWave;
    if ((int)threadIdx.x % kWave == 0) {
#pragma unroll
      for (int i = 0; i < N; ++i)
        lds[wave * kUncLdsStride + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) {
      double t = lds[i];
      for (int w = 1; w < WAVES; ++w)
        t += lds[w * kUncLdsStride + i];
      v[i] = t;
    }
  }
}

template <int MODEL, int INTERP, int GROUP>
__global__ void __launch_bounds__(GROUP <= 64 ? 256 : GROUP) lk_uncertainty_kernel(LkUncertaintyArgs a) {
  constexpr int THREADS = GROUP <= 64 ? 256 : GROUP;
  constexpr int P = n_params(MODEL), NA = P * (P + 1) / 2, N = NA + P + 1;
  __shared__ double lds[(GROUP > 64 ? GROUP / kWave : 1) * kUncLdsStride];
  const int gid = (int)blockIdx.x * (THREADS / GROUP) + (int)threadIdx.x / GROUP;
  const int lane = (int)threadIdx.x % GROUP;
  if (gid >= a.n_sectors) // (GROUP == 512: the whole workgroup; GROUP <= 64: whole rows / wavefronts, no barriers below)
    return;
  const int s = (int)a.order[gid];
  const lk_result rec = a.rec[s];
  const bool good = reseed_good(rec, P, 0.f);
  // the sector at level L, as bw_level / bw_coords of lk_backward.hip see it
  const int4 rc = a.rect[s];
  const uint32_t off = a.off[s];
  const gptr<uint8_t> und = (gptr<uint8_t>)a.und, def = (gptr<uint8_t>)a.def;
  const gptr<f32x2> xy = (gptr<f32x2>)(a.xy + off);
  const int rw = rc.z;
  const int n = rw > 0 ? rc.w : (int)(a.off[s + 1] - off);
  const float inv_w = rw > 0 ? 1.f / (float)rw : 0.f;
  const float2 c0 = a.center[s];
  const float inv = 1.f / (float)(1 << a.level); // pyramid_class.cpp:357-361, as the solve kernels
  const float cx = a.level == 0 ? c0.x : c0.x * inv, cy = a.level == 0 ? c0.y : c0.y * inv;
  float p[6];
#pragma unroll
  for (int i = 0; i < 6; ++i)
    p[i] = i < P ? rec.resultingParameters[i] : 0.f;
  translate<P>(p, 0, a.level); // the record is in level-0 scale (pyramid_class.cpp:260-287, as the solve between levels)
  double v[N + 1]; // the sums, and the samples the sampler flagged
#pragma unroll
  for (int i = 0; i <= N; ++i)
    v[i] = 0.0;
  const int umaxr = a.urows - 1, umaxc = a.ucols - 1;
  for (int k = lane; k < (good ? n : 0); k += GROUP) { // (a bad record is not evaluated)
    f32x2 q;
    if (rw > 0) { // implicit rectangle, row by row
      int row = (int)((float)k * inv_w);
      int col = k - row * rw;
      if (col < 0) {
        col += rw;
        --row;
      } else if (col >= rw) {
        col -= rw;
        ++row;
      }
      q.x = (float)(rc.x + col);
      q.y = (float)(rc.y + row);
    } else {
      q = xy[k];
    }
    float xd, yd, dx = 0.f, dy = 0.f;
    Warp<MODEL>::apply(q.x, q.y, cx, cy, p, xd, yd, dx, dy);
    int uix = (int)(q.x + 0.5f), uiy = (int)(q.y + 0.5f); // the node the forward residual reads
    uix = min(max(uix, 0), umaxc);                          // (memory safety only; valid lists never clamp)
    uiy = min(max(uiy, 0), umaxr);
    const float und_w = (float)und[(size_t)uiy * (size_t)a.ucols + (size_t)uix];
    float W, Wx, Wy;
    if (!sample_def<INTERP>(def, a.drows, a.dcols, xd, yd, W, Wx, Wy)) {
      v[N] += 1.0;
      continue; // the sums of an evaluation that hit the error are never used
    }
    const float V = und_w - W;
    float H[P];
    Warp<MODEL>::jac(Wx, Wy, dx, dy, H);
    double Hd[P];
#pragma unroll
    for (int i = 0; i < P; ++i)
      Hd[i] = (double)H[i];
    const double Vd = (double)V;
    int idx = 0;
#pragma unroll
    for (int p1 = 0; p1 < P; ++p1)
#pragma unroll
      for (int p2 = p1; p2 < P; ++p2)
        v[idx] += Hd[p1] * Hd[p2], ++idx; // (no contraction: a rounded product, then a rounded sum)
#pragma unroll
    for (int p1 = 0; p1 < P; ++p1)
      v[NA + p1] += Hd[p1] * Vd;
    v[N - 1] += Vd * Vd;
  }
  unc_reduce<GROUP>(v, lds);
  if (lane != 0)
    return;
  const bool evaluated = good && v[N] == 0.0;
  double sums[kLkUncSums];
#pragma unroll
  for (int i = 0; i < kLkUncSums; ++i)
    sums[i] = i < N && evaluated ? v[i] : 0.0;
  lk_uncertainty r;
  if (!good)
    lk_uncertainty_clear(&r, n, LK_UNC_BAD_RECORD);
  else if (!evaluated)
    lk_uncertainty_clear(&r, n, LK_UNC_OUT_OF_IMAGE);
  else
    lk_uncertainty_record<P>(n, sums, a.level, &r);
  a.out[s] = r;
  if (a.sums) {
#pragma unroll
    for (int i = 0; i < kLkUncSums; ++i)
      a.sums[(size_t)s * kLkUncSums + i] = sums[i];
  }
}

template <int MODEL, int INTERP> hipError_t launch_unc_mi(const LkUncertaintyArgs &a, int group, hipStream_t st) {
  const int per_block = group <= 64 ? 256 / group : 1;
  const int blocks = (a.n_sectors + per_block - 1) / per_block;
  if (blocks <= 0)
    return hipSuccess;
  if (group == 16)
    hipLaunchKernelGGL((lk_uncertainty_kernel<MODEL, INTERP, 16>), dim3(blocks), dim3(256), 0, st, a);
  else if (group == 64)
    hipLaunchKernelGGL((lk_uncertainty_kernel<MODEL, INTERP, 64>), dim3(blocks), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((lk_uncertainty_kernel<MODEL, INTERP, 512>), dim3(blocks), dim3(512), 0, st, a);
  return hipGetLastError();
}

template <int MODEL> hipError_t launch_unc_m(const LkUncertaintyArgs &a, int interp, int group, hipStream_t st) {
  switch (interp) {
  case LK_IM_NEAREST: return launch_unc_mi<MODEL, LK_IM_NEAREST>(a, group, st);
  case LK_IM_BILINEAR: return launch_unc_mi<MODEL, LK_IM_BILINEAR>(a, group, st);
  case LK_IM_BICUBIC: return launch_unc_mi<MODEL, LK_IM_BICUBIC>(a, group, st);
  default: return launch_unc_mi<MODEL, LK_IM_BICUBIC_SEPARABLE>(a, group, st);
  }
}

} // namespace

hipError_t lk_launch_uncertainty(const LkUncertaintyArgs &a, int model, int interp, int group, hipStream_t st) {
  switch (model) {
  case LK_FM_U: return launch_unc_m<LK_FM_U>(a, interp, group, st);
  case LK_FM_UV: return launch_unc_m<LK_FM_UV>(a, interp, group, st);
  case LK_FM_UVQ: return launch_unc_m<LK_FM_UVQ>(a, interp, group, st);
  default: return launch_unc_m<LK_FM_UVUXUYVXVY>(a, interp, group, st);
  }
}
