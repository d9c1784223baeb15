// lk_solver_common.hpp - device pieces that the forward solve kernels (lk_kernels.hip) and the backward
// (inverse-compositional) kernel (lk_backward.hip) share: the deformed-image samplers, the warps of the four models,
// the sums layout, the damped normal-equation solvers and the level-to-level parameter translation.  One definition
// each, so that a residual, a step and a translation mean the same thing in both update modes.  Internal linkage
// (anonymous namespace): every translation unit that includes it gets its own copies, inlined where they are used.
#pragma once
#include "lk_device.hpp"

#include <float.h>
#include <stdint.h>

#include <utility>

// Smallest pivot ratio d_j / A_jj the fast flavour factors through (below it the sector goes to
// the SAFE kernel and the reference's QR).  1e-3 sent 0.4 % of config 4's solves there and, before
// that pass existed, cost its 1 % tail a factor of ten against the reference; root-free Cholesky
// in float32 is fine down to 1e-6.
#ifndef LK_FAST_PIVOT
#define LK_FAST_PIVOT 1e-6f
#endif


namespace {

constexpr int kWave = 64;

// pointers that are known to be global memory (loaded from a struct they would be
// generic and cost flat_load instead of global_load)
template <class T> using gptr = const __attribute__((address_space(1))) T *;
typedef float f32x2 __attribute__((ext_vector_type(2))); // same layout as float2

__host__ __device__ constexpr int n_params(int model) {
  return model == LK_FM_U ? 1 : model == LK_FM_UV ? 2 : model == LK_FM_UVQ ? 3 : 6;
}

// ------------------------------------------------------------------------------------
// wavefront reduction: 4 DPP steps inside each row of 16 lanes, then 4 readlanes.
// Every lane ends with the same bits (the tree is identical for all lanes).
// ------------------------------------------------------------------------------------
template <int CTRL> __device__ __forceinline__ float dpp_add(float v) {
  int t = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true);
  return v + __int_as_float(t);
}

// lane I of the own 16-lane row (row_newbcast, gfx90a and later)
template <int I> __device__ __forceinline__ float dpp_bcast(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x150 + I, 0xF, 0xF, false));
}

// ------------------------------------------------------------------------------------
// reduce-scatter of the 28 sums of a six-parameter model inside a 16-lane row
// ------------------------------------------------------------------------------------
// The all-reduce of evaluate<> sends every sum through the same four DPP stages (quad_perm [1,0,3,2], quad_perm
// [2,3,0,1], row_half_mirror, row_mirror): 4 x 28 adds, after which every lane of the row holds every total.  Here a
// lane keeps, at each stage, only half of the sums it still carries and adds its partner's copy of those:
// 28 -> 16 -> 8 -> 4 -> 2 sums per lane, 12 * 3 + 4 + (8 + 4 + 2) * 3 = 82 instructions instead of 112, and - what
// pays - two sums per lane instead of 28 for the row-to-row additions that follow.  Every sum still goes through
// the additions (v[l] + v[l^1]) -> (.. + ..[l^2]) -> (quad + mirrored quad) -> (half + mirrored half) of the
// all-reduce; which of the two operands of an addition is "own" differs from lane to lane there as well
// (a + b == b + a), so the totals are the all-reduce's, bit for bit.
// The mirrors pair lane l with lane 7 - l / 15 - l, whose low bits differ from l's: which half a lane keeps at a
// stage is therefore decided by the bits e0 = b0 ^ b2, e1 = b1 ^ b2, e2 = b2 ^ b3, e3 = b3 of its lane number b3 b2 b1 b0
// - each stage's partner differs in exactly that stage's bit.  Sum v (of 32: 28..31 do not exist, their places
// hold copies of sums 12..15) ends in the lane with (e0, e1, e2, e3) = bits (4, 3, 2, 1) of v, in slot v & 1.
constexpr int scatter_owner(int v) { // the lane of the 16-lane row that ends with sums v & ~1 and v | 1
  const int e0 = (v >> 4) & 1, e1 = (v >> 3) & 1, e2 = (v >> 2) & 1, e3 = (v >> 1) & 1;
  const int b3 = e3, b2 = e2 ^ b3, b0 = e0 ^ b2, b1 = e1 ^ b2;
  return b0 | (b1 << 1) | (b2 << 2) | (b3 << 3);
}

template <int CTRL, int HALF> __device__ __forceinline__ void scatter_stage(float *t, bool upper) {
#pragma unroll
  for (int i = 0; i < HALF; ++i) {
    const float keep = upper ? t[HALF + i] : t[i], send = upper ? t[i] : t[HALF + i];
    const int got = __builtin_amdgcn_update_dpp(0, __float_as_int(send), CTRL, 0xF, 0xF, true);
    t[i] = keep + __int_as_float(got);
  }
}

// v[0..27] (one lane's partial sums) -> s0, s1: the row's totals of sums 2m and 2m + 1 in lane scatter_owner(2m)
__device__ __forceinline__ void row16_reduce_scatter28(const float (&v)[28], float &s0, float &s1) {
  const int l = (int)threadIdx.x;
  const bool b2 = (l & 4) != 0, b3 = (l & 8) != 0;
  float t[16];
#pragma unroll
  for (int i = 0; i < 12; ++i) { // quad_perm [1,0,3,2]: sums i and 16 + i
    const bool upper = ((l & 1) != 0) != b2;
    const float keep = upper ? v[16 + i] : v[i], send = upper ? v[i] : v[16 + i];
    const int got = __builtin_amdgcn_update_dpp(0, __float_as_int(send), 0xB1, 0xF, 0xF, true);
    t[i] = keep + __int_as_float(got);
  }
#pragma unroll
  for (int i = 12; i < 16; ++i) // (no sums 28..31: both lanes of the pair keep sum i)
    t[i] = dpp_add<0xB1>(v[i]);
  scatter_stage<0x4E, 8>(t, ((l & 2) != 0) != b2); // quad_perm [2,3,0,1]
  scatter_stage<0x141, 4>(t, b2 != b3);            // row_half_mirror
  scatter_stage<0x140, 2>(t, b3);                  // row_mirror
  s0 = t[0];
  s1 = t[1];
}

// v + the same lane's value in the partner row (rows 0/1 and 2/3), and in the partner half of the wavefront:
// one VALU swap and one add, no LDS crossbar (__shfl_xor: address, ds_bpermute, wait, add)
__device__ __forceinline__ float add_partner_row(float v) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float add_partner_half(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// lane scatter_owner(V) of the own row's slot for sum V
template <int V> __device__ __forceinline__ float scattered_sum(float s0, float s1) {
  return dpp_bcast<scatter_owner(V)>((V & 1) ? s1 : s0);
}

template <int... V>
__device__ __forceinline__ void gather_scattered(float *S, float s0, float s1, std::integer_sequence<int, V...>) {
  ((S[V] = scattered_sum<V>(s0, s1)), ...);
}

__device__ __forceinline__ uint32_t load_u32_unaligned(gptr<uint8_t> p) {
  uint32_t v;
  typedef uint32_t __attribute__((aligned(1))) u32_u;
  v = *(const __attribute__((address_space(1))) u32_u *)p;
  return v;
}

__device__ __forceinline__ float ub0(uint32_t v) { return (float)(v & 0xffu); }
__device__ __forceinline__ float ub1(uint32_t v) { return (float)((v >> 8) & 0xffu); }
__device__ __forceinline__ float ub2(uint32_t v) { return (float)((v >> 16) & 0xffu); }
__device__ __forceinline__ float ub3(uint32_t v) { return (float)(v >> 24); }

// ------------------------------------------------------------------------------------
// bicubic (interpolation_class.cpp:79-138, :243-336)
// ------------------------------------------------------------------------------------
// The reference builds, per deformed pixel, a 16-vector of values and central differences
// and multiplies it by a 16x16 integer matrix (:296-333).  That map factors as
//     a[jk][ik] = sum_r sum_c Cm[jk][r] * Cm[ik][c] * Pix[r][c]
// with Pix the 4x4 u8 window (rows iy-1..iy+2, cols ix-1..ix+2) and Cm the 1-D
// "4 pixels -> monomial coefficients on [1,2]" matrix below.  Every product and every
// partial sum is a multiple of 1/4 below 2^24/4 in magnitude, hence exactly representable
// in float32: the factored form, in any order and with FMAs, yields the reference's
// coefficients bit for bit (tests/test_parity_gpu.py::test_bicubic_coefficients_exact).
// c = Cm * p with Cm = [2 -3 3 -1; -4 9.5 -8 2.5; 2.5 -7 6.5 -2; -0.5 1.5 -1.5 0.5] in 11 operations
// instead of 16, through the identities the cubic itself provides (value and slope at dx = 1):
//   e = (p3 - p0) + 3 (p1 - p2),  c3 = e / 2,  c0 = p0 - e,
//   c1 + c2 = p1 - c0 - c3,       c1 + 2 c2 + 3 c3 = (p2 - p0) / 2.
// Exact like the matrix form: every intermediate is a multiple of 1/4 below 2^22 in magnitude.
__device__ __forceinline__ void cubic_1d(float p0, float p1, float p2, float p3, float &c0,
                                         float &c1, float &c2, float &c3) {
  const float e = __builtin_fmaf(3.0f, p1 - p2, p3 - p0);
  c3 = 0.5f * e;
  c0 = p0 - e;
  const float u = (p1 - c0) - c3;
  c2 = __builtin_fmaf(-3.0f, c3, __builtin_fmaf(0.5f, p2 - p0, -u));
  c1 = u - c2;
}

// the 4x4 window as four (unaligned) dwords, rows iy-1..iy+2, columns ix-1..ix+2
struct Window4 {
  uint32_t r0, r1, r2, r3;
};
__device__ __forceinline__ Window4 load_window(gptr<uint8_t> def, int cols, int ix, int iy) {
  gptr<uint8_t> base = def + (size_t)(iy - 1) * (size_t)cols + (size_t)(ix - 1);
  Window4 w;
  w.r0 = load_u32_unaligned(base);
  w.r1 = load_u32_unaligned(base + cols);
  w.r2 = load_u32_unaligned(base + 2 * (size_t)cols);
  w.r3 = load_u32_unaligned(base + 3 * (size_t)cols);
  return w;
}

// Value and gradient of the bicubic at (ix + dx - 1, iy + dy - 1), dx,dy in [1,2).
// The 16 coefficients are produced exactly (see above) by 4 + 4 one-dimensional transforms, and
// then W, dW/dx, dW/dy are accumulated in the reference's order (:94-126): three running sums,
// jk outer / ik inner, each term built left to right.
__device__ __forceinline__ void bicubic_window(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, float dx, float dy,
                                               float &W, float &Wx, float &Wy) {
  // t[r][k]: x-direction transform of image row r
  float t0[4], t1[4], t2[4], t3[4];
  cubic_1d(ub0(r0), ub1(r0), ub2(r0), ub3(r0), t0[0], t0[1], t0[2], t0[3]);
  cubic_1d(ub0(r1), ub1(r1), ub2(r1), ub3(r1), t1[0], t1[1], t1[2], t1[3]);
  cubic_1d(ub0(r2), ub1(r2), ub2(r2), ub3(r2), t2[0], t2[1], t2[2], t2[3]);
  cubic_1d(ub0(r3), ub1(r3), ub2(r3), ub3(r3), t3[0], t3[1], t3[2], t3[3]);
  // y-direction transform, column by column: a[jk][ik] (exact in any order)
  float a0[4], a1[4], a2[4], a3[4];
#pragma unroll
  for (int ik = 0; ik < 4; ++ik)
    cubic_1d(t0[ik], t1[ik], t2[ik], t3[ik], a0[ik], a1[ik], a2[ik], a3[ik]);
  const float px[4] = {1.f, dx, dx * dx, dx * dx * dx};
  const float py[4] = {1.f, dy, dy * dy, dy * dy * dy};
  W = 0.f;
  Wx = 0.f;
  Wy = 0.f;
#pragma unroll
  for (int jk = 0; jk < 4; ++jk) {
#pragma unroll
    for (int ik = 0; ik < 4; ++ik) {
      const float c = jk == 0 ? a0[ik] : jk == 1 ? a1[ik] : jk == 2 ? a2[ik] : a3[ik];
      W += c * py[jk] * px[ik];
      if (ik > 0)
        Wx += (float)ik * c * py[jk] * px[ik - 1];
      if (jk > 0)
        Wy += (float)jk * c * py[jk - 1] * px[ik];
    }
  }
}

__device__ __forceinline__ void bicubic_sample(gptr<uint8_t> def, int cols, int ix, int iy, float dx,
                                               float dy, float &W, float &Wx, float &Wy) {
  const Window4 w = load_window(def, cols, ix, iy);
  bicubic_window(w.r0, w.r1, w.r2, w.r3, dx, dy, W, Wx, Wy);
}

// Catmull-Rom weights of the four samples at -1, 0, 1, 2 for position t in [0, 1) and their
// derivatives (Horner form)
__device__ __forceinline__ void catmull_rom(float t, float (&w)[4], float (&g)[4]) {
  w[0] = t * __builtin_fmaf(t, __builtin_fmaf(t, -0.5f, 1.0f), -0.5f);
  w[1] = __builtin_fmaf(t * t, __builtin_fmaf(t, 1.5f, -2.5f), 1.0f);
  w[2] = t * __builtin_fmaf(t, __builtin_fmaf(t, -1.5f, 2.0f), 0.5f);
  w[3] = t * t * __builtin_fmaf(t, 0.5f, -0.5f);
  g[0] = __builtin_fmaf(t, __builtin_fmaf(t, -1.5f, 2.0f), -0.5f);
  g[1] = t * __builtin_fmaf(t, 4.5f, -5.0f);
  g[2] = __builtin_fmaf(t, __builtin_fmaf(t, -4.5f, 4.0f), 0.5f);
  g[3] = t * __builtin_fmaf(t, 1.5f, -1.0f);
}

// returns false when the sample leaves the image (error_interpolation_out_of_image)
template <int INTERP>
__device__ __forceinline__ bool sample_def(gptr<uint8_t> def, int rows, int cols, float xd,
                                           float yd, float &W, float &Wx, float &Wy) {
  if constexpr (INTERP == LK_IM_BICUBIC) {
    if (!(xd > 1.f && yd > 1.f && xd < (float)cols - 2.f && yd < (float)rows - 2.f))
      return false;
    int ix = (int)xd, iy = (int)yd;
    float dx = xd - (float)ix + 1.f, dy = yd - (float)iy + 1.f;
    bicubic_sample(def, cols, ix, iy, dx, dy, W, Wx, Wy);
    return true;
  } else if constexpr (INTERP == LK_IM_BICUBIC_SEPARABLE) {
    // The reference's bicubic patch (values + central differences on the cell's corners) is
    // the Catmull-Rom spline; evaluated here as two 1-D kernels instead of 16 coefficients and
    // monomials.  Same validity rule, same window; results equal to rounding, not bit for bit.
    if (!(xd > 1.f && yd > 1.f && xd < (float)cols - 2.f && yd < (float)rows - 2.f))
      return false;
    const int ix = (int)xd, iy = (int)yd;
    const float tx = xd - (float)ix, ty = yd - (float)iy;
    const Window4 w = load_window(def, cols, ix, iy);
    float wx[4], gx[4], wy[4], gy[4];
    catmull_rom(tx, wx, gx);
    catmull_rom(ty, wy, gy);
    const uint32_t r[4] = {w.r0, w.r1, w.r2, w.r3};
    float row_v[4], row_g[4]; // per image row: value and x-derivative along x
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float p0 = ub0(r[j]), p1 = ub1(r[j]), p2 = ub2(r[j]), p3 = ub3(r[j]);
      row_v[j] = __builtin_fmaf(wx[3], p3, __builtin_fmaf(wx[2], p2, __builtin_fmaf(wx[1], p1, wx[0] * p0)));
      row_g[j] = __builtin_fmaf(gx[3], p3, __builtin_fmaf(gx[2], p2, __builtin_fmaf(gx[1], p1, gx[0] * p0)));
    }
    W = __builtin_fmaf(wy[3], row_v[3], __builtin_fmaf(wy[2], row_v[2], __builtin_fmaf(wy[1], row_v[1], wy[0] * row_v[0])));
    Wx = __builtin_fmaf(wy[3], row_g[3], __builtin_fmaf(wy[2], row_g[2], __builtin_fmaf(wy[1], row_g[1], wy[0] * row_g[0])));
    Wy = __builtin_fmaf(gy[3], row_v[3], __builtin_fmaf(gy[2], row_v[2], __builtin_fmaf(gy[1], row_v[1], gy[0] * row_v[0])));
    return true;
  } else if constexpr (INTERP == LK_IM_BILINEAR) { // :140-195, :338-374
    if (!(xd > 0.f && yd > 0.f && xd < (float)(cols - 1) && yd < (float)(rows - 1)))
      return false;
    int ix = (int)xd, iy = (int)yd;
    gptr<uint8_t> q = def + (size_t)iy * (size_t)cols + (size_t)ix;
    float w00 = (float)q[0], w10 = (float)q[1], w01 = (float)q[cols], w11 = (float)q[cols + 1];
    float a0 = w00, a1 = w10 - w00, a2 = w01 - w00, a3 = w11 - w10 - w01 + w00;
    float dx = xd - (float)ix, dy = yd - (float)iy;
    // jk outer / ik inner with px = {1,dx}, py = {1,dy}
    W = 0.f + a0;
    W += a1 * dx;
    Wx = 0.f + a1;
    W += a2 * dy;
    Wy = 0.f + a2;
    W += a3 * dy * dx;
    Wx += a3 * dy;
    Wy += a3 * dx;
    return true;
  } else { // nearest :197-226, :376-406
    if (!(xd > 0.f && yd > 0.f && xd < (float)(cols - 1) && yd < (float)(rows - 1)))
      return false;
    int ix = (int)(xd + 0.5f), iy = (int)(yd + 0.5f);
    gptr<uint8_t> q = def + (size_t)iy * (size_t)cols + (size_t)ix;
    float w00 = (float)q[0], w10 = (float)q[1], w01 = (float)q[cols];
    W = w00;
    Wx = w10 - w00;
    Wy = w01 - w00;
    return true;
  }
}

// Value-only form of sample_def (the backward mode's residual T - W): the same function with the gradient left unused, so
// the compiler drops the gradient arithmetic and W is the forward residual's W at the same point, bit for bit.
template <int INTERP>
__device__ __forceinline__ bool sample_def_value(gptr<uint8_t> def, int rows, int cols, float xd, float yd, float &W) {
  float Wx, Wy;
  return sample_def<INTERP>(def, rows, cols, xd, yd, W, Wx, Wy);
}

// ------------------------------------------------------------------------------------
// per-sample body: warp (model_class.cpp:48-202), sample, residual, H
// (interpolation_class.cpp:701-739).  H = dW/dx * dTx/dp + dW/dy * dTy/dp with the zero
// entries of dT/dp dropped (x*1 + y*0 == x exactly for finite y).
// ------------------------------------------------------------------------------------
template <int MODEL> struct Warp;
template <> struct Warp<LK_FM_U> {
  static __device__ __forceinline__ void apply(float x, float y, float, float, const float *p,
                                               float &xd, float &yd, float &, float &) {
    xd = x + p[0];
    yd = y;
  }
  static __device__ __forceinline__ void jac(float Wx, float, float, float, float *H) { H[0] = Wx; }
};
template <> struct Warp<LK_FM_UV> {
  static __device__ __forceinline__ void apply(float x, float y, float, float, const float *p,
                                               float &xd, float &yd, float &, float &) {
    xd = x + p[0];
    yd = y + p[1];
  }
  static __device__ __forceinline__ void jac(float Wx, float Wy, float, float, float *H) {
    H[0] = Wx;
    H[1] = Wy;
  }
};
template <> struct Warp<LK_FM_UVQ> {
  static __device__ __forceinline__ void apply(float x, float y, float cx, float cy,
                                               const float *p, float &xd, float &yd, float &dx,
                                               float &dy) {
    dx = x - cx;
    dy = y - cy;
    xd = x + p[0] - p[2] * dy;
    yd = y + p[1] + p[2] * dx;
  }
  static __device__ __forceinline__ void jac(float Wx, float Wy, float dx, float dy, float *H) {
    H[0] = Wx;
    H[1] = Wy;
    H[2] = Wx * (-dy) + Wy * dx;
  }
};
template <> struct Warp<LK_FM_UVUXUYVXVY> {
  static __device__ __forceinline__ void apply(float x, float y, float cx, float cy,
                                               const float *p, float &xd, float &yd, float &dx,
                                               float &dy) {
    dx = x - cx;
    dy = y - cy;
    xd = x + p[0] + p[2] * dx + p[3] * dy;
    yd = y + p[1] + p[4] * dx + p[5] * dy;
  }
  static __device__ __forceinline__ void jac(float Wx, float Wy, float dx, float dy, float *H) {
    H[0] = Wx;
    H[1] = Wy;
    H[2] = Wx * dx;
    H[3] = Wx * dy;
    H[4] = Wy * dx;
    H[5] = Wy * dy;
  }
};

template <int P> struct Sums { // upper triangle row-major, then b, then chi
  static constexpr int NA = P * (P + 1) / 2;
  static constexpr int N = NA + P + 1;
  float v[N];
};

// ------------------------------------------------------------------------------------
// the damped normal-equation solve (compute_model_parameters + solve,
// correlation_class.cpp:642-768)
// ------------------------------------------------------------------------------------
// The reference hands the symmetric, LM-damped matrix to Eigen's ColPivHouseholderQR
// (correlation_class.cpp:742-747); its CUDA path uses cuSOLVER's Cholesky instead
// (cuda_solver.cu:120-149).  Two solvers live here:
//
//  * fast path - A = sum(H H^T)/n with the diagonal scaled by (1+lambda) is symmetric
//    positive (semi-)definite; it is factored as U^T D U (root-free Cholesky) entirely in
//    registers, ~200 instructions.  Used whenever every pivot is at least 1e-4 of the
//    largest diagonal entry, i.e. the system is well conditioned and any backward-stable
//    solver returns the same step to rounding (tests/test_parity_gpu.py docstring).
//  * reference path - Eigen 3.4.0 ColPivHouseholderQR restated (column norms with
//    LAPACK-style down-dating, first-largest remaining column as pivot, Householder
//    reflectors, rank decision, back-substitution), ~3000 instructions.  Used when a pivot
//    of the fast path is small or non-positive: few samples (fewer than parameters at a
//    coarse pyramid level - BASELINE config 5's level 3 has 4-9 samples for 6 parameters),
//    flat texture.  There the answer is DEFINED by the rank-revealing pivoting (dropped
//    pivots get a zero step), so the engine follows it operation by operation.
//    All indices are compile-time after unrolling; the pivot choice is applied with
//    compare-and-swap so nothing is dynamically indexed (no scratch).  M is column-major.
template <int N>
__device__ __forceinline__ void colpiv_qr_solve(float (&M)[N * N], const float (&bin)[N],
                                                float (&x)[N]) {
#define QR(r, c) M[(c)*N + (r)]
  float hc[N], normU[N], normD[N], cv[N];
  int trans[N];
  const float eps = FLT_EPSILON;
  float maxn = 0.f;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < N; ++r)
      s += QR(r, k) * QR(r, k);
    normD[k] = __builtin_sqrtf(s);
    normU[k] = normD[k];
    if (normU[k] > maxn)
      maxn = normU[k];
  }
  const float threshold_helper = (maxn * eps) * (maxn * eps) / (float)N;
  const float norm_downdate_threshold = __builtin_sqrtf(eps);
  int nonzero_pivots = N;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    int big = k;
    float bigv = normU[k];
#pragma unroll
    for (int j = k + 1; j < N; ++j)
      if (normU[j] > bigv) {
        bigv = normU[j];
        big = j;
      }
    float big_sq = bigv * bigv;
    if (nonzero_pivots == N && big_sq < threshold_helper * (float)(N - k))
      nonzero_pivots = k;
    trans[k] = big;
#pragma unroll
    for (int j = k + 1; j < N; ++j) {
      if (big == j) {
#pragma unroll
        for (int r = 0; r < N; ++r) {
          float t = QR(r, k);
          QR(r, k) = QR(r, j);
          QR(r, j) = t;
        }
        float t = normU[k];
        normU[k] = normU[j];
        normU[j] = t;
        t = normD[k];
        normD[k] = normD[j];
        normD[j] = t;
      }
    }
    float tailSq = 0.f;
#pragma unroll
    for (int r = k + 1; r < N; ++r)
      tailSq += QR(r, k) * QR(r, k);
    float c0 = QR(k, k), beta, tau;
    if (tailSq <= FLT_MIN) {
      tau = 0.f;
      beta = c0;
#pragma unroll
      for (int r = k + 1; r < N; ++r)
        QR(r, k) = 0.f;
    } else {
      beta = __builtin_sqrtf(c0 * c0 + tailSq);
      if (c0 >= 0.f)
        beta = -beta;
      float den = c0 - beta;
#pragma unroll
      for (int r = k + 1; r < N; ++r)
        QR(r, k) = QR(r, k) / den;
      tau = (beta - c0) / beta;
    }
    hc[k] = tau;
    QR(k, k) = beta;
    if (N - k > 1 && tau != 0.f) {
#pragma unroll
      for (int j = k + 1; j < N; ++j) {
        float tmp = 0.f;
#pragma unroll
        for (int r = k + 1; r < N; ++r)
          tmp += QR(r, k) * QR(r, j);
        tmp += QR(k, j);
        QR(k, j) -= tau * tmp;
#pragma unroll
        for (int r = k + 1; r < N; ++r)
          QR(r, j) -= tmp * (tau * QR(r, k));
      }
    }
#pragma unroll
    for (int j = k + 1; j < N; ++j) {
      if (normU[j] != 0.f) {
        float temp = __builtin_fabsf(QR(k, j)) / normU[j];
        temp = (1.f + temp) * (1.f - temp);
        temp = temp < 0.f ? 0.f : temp;
        float ratio = normU[j] / normD[j];
        float temp2 = temp * (ratio * ratio);
        if (temp2 <= norm_downdate_threshold) {
          float s = 0.f;
#pragma unroll
          for (int r = k + 1; r < N; ++r)
            s += QR(r, j) * QR(r, j);
          normD[j] = __builtin_sqrtf(s);
          normU[j] = normD[j];
        } else {
          normU[j] *= __builtin_sqrtf(temp);
        }
      }
    }
  }
  if (nonzero_pivots == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i)
      x[i] = 0.f;
    return;
  }
#pragma unroll
  for (int i = 0; i < N; ++i)
    cv[i] = bin[i];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    if (k < nonzero_pivots) {
      if (N - k == 1) {
        cv[k] *= 1.f - hc[k];
      } else if (hc[k] != 0.f) {
        float tmp = 0.f;
#pragma unroll
        for (int r = k + 1; r < N; ++r)
          tmp += QR(r, k) * cv[r];
        tmp += cv[k];
        cv[k] -= hc[k] * tmp;
#pragma unroll
        for (int r = k + 1; r < N; ++r)
          cv[r] -= tmp * (hc[k] * QR(r, k));
      }
    }
  }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    if (i < nonzero_pivots) {
      cv[i] = cv[i] / QR(i, i);
#pragma unroll
      for (int r = 0; r < i; ++r)
        cv[r] -= cv[i] * QR(r, i);
    } else {
      cv[i] = 0.f; // rank-deficient tail: dst rows of the dropped pivots are zero
    }
  }
  // x[perm[i]] = cv[i], perm = product of the transpositions (k, trans[k]), applied on the
  // right in ascending k.  Equivalent, without a dynamically indexed perm[]: start from
  // y = cv and undo the column swaps in descending k.
#pragma unroll
  for (int i = 0; i < N; ++i)
    x[i] = cv[i];
#pragma unroll
  for (int k = N - 1; k >= 0; --k) {
#pragma unroll
    for (int j = k + 1; j < N; ++j)
      if (trans[k] == j) {
        float t = x[k];
        x[k] = x[j];
        x[j] = t;
      }
  }
#undef QR
}


// The same factorisation and solve, operation for operation, spread over the 16 lanes of a row
// that all hold the same inputs (the finisher of starved levels): lane j owns COLUMN j - its
// six entries, its norms and its current position in the pivot order - instead of every lane
// carrying the whole matrix through ~3000 instructions.  Column swaps become exchanges of
// positions (no data moves); the pivot scan runs on the norms gathered by position, in the
// reference's order (first strictly larger wins, NaN never wins); the Householder vector, tau
// and the triangular factor travel by ds_bpermute from the lane that owns them.  Every
// arithmetic operation is the one colpiv_qr_solve performs, on the same operands, in the same
// order, so the step is bit-identical (tests: lk_damped_solve with reference_solver = 2 against 1
// on random, rank-deficient and non-finite systems; the finisher's end-to-end bit identity).
template <int N>
__device__ __forceinline__ void colpiv_qr_solve_row16(const float (&M)[N * N], const float (&bin)[N],
                                                      float (&x)[N]) {
  const int lane = (int)threadIdx.x & 63, me = lane & 15, row_base = lane & ~15;
  auto from = [&](float v, int src) { return __shfl(v, row_base | src, 64); }; // lane `src` of the own row
  // my column (lanes >= N carry a dummy column that is never selected)
  float col[N];
#pragma unroll
  for (int r = 0; r < N; ++r) {
    float v = 0.f;
#pragma unroll
    for (int c = 0; c < N; ++c)
      v = me == c ? M[c * N + r] : v;
    col[r] = v;
  }
  int pos = me;      // position of my column in the pivot order
  int owner[N];      // replicated: lane that owns the column at each position
#pragma unroll
  for (int q = 0; q < N; ++q)
    owner[q] = q;
  const float eps = FLT_EPSILON;
  float s0 = 0.f;
#pragma unroll
  for (int r = 0; r < N; ++r)
    s0 += col[r] * col[r];
  float normD = __builtin_sqrtf(s0), normU = normD;
  float maxn = 0.f;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const float nk = from(normU, k);
    if (nk > maxn)
      maxn = nk;
  }
  const float threshold_helper = (maxn * eps) * (maxn * eps) / (float)N;
  const float norm_downdate_threshold = __builtin_sqrtf(eps);
  int nonzero_pivots = N;
  float hc[N], vk[N][N]; // replicated: tau of step k and its Householder vector (rows r > k)
  int trans[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    // pivot scan over positions k..N-1, in order
    int big = k;
    float bigv = from(normU, owner[k]);
#pragma unroll
    for (int j = k + 1; j < N; ++j) {
      const float nj = from(normU, owner[j]);
      if (nj > bigv) {
        bigv = nj;
        big = j;
      }
    }
    const float big_sq = bigv * bigv;
    if (nonzero_pivots == N && big_sq < threshold_helper * (float)(N - k))
      nonzero_pivots = k;
    trans[k] = big;
    // exchange positions k and big
    int owner_big = owner[k];
#pragma unroll
    for (int j = k + 1; j < N; ++j)
      owner_big = big == j ? owner[j] : owner_big;
    const int owner_k = owner[k];
#pragma unroll
    for (int j = k + 1; j < N; ++j)
      owner[j] = big == j ? owner_k : owner[j];
    owner[k] = owner_big;
    if (big != k) {
      if (me == owner_big)
        pos = k;
      else if (me == owner_k)
        pos = big;
    }
    // Householder of the column at position k - every lane works on its own column, the
    // pivot's result is what gets used
    float tailSq = 0.f;
#pragma unroll
    for (int r = k + 1; r < N; ++r)
      tailSq += col[r] * col[r];
    const float c0 = col[k];
    // (both sides of every data-dependent branch of this step are computed and the result selected: the row is
    // bound by the LENGTH of this chain of dependent operations, not by their number, and straight-line code lets the
    // square roots and divisions of the Householder vector, of tau and of the norm down-dating overlap)
    float beta, tau, ess[N];
    {
      const bool tiny = tailSq <= FLT_MIN;
      float b = __builtin_sqrtf(c0 * c0 + tailSq);
      b = c0 >= 0.f ? -b : b;
      const float den = c0 - b;
#pragma unroll
      for (int r = k + 1; r < N; ++r) {
        const float e = col[r] / den;
        ess[r] = tiny ? 0.f : e;
      }
      const float t = (b - c0) / b;
      tau = tiny ? 0.f : t;
      beta = tiny ? c0 : b;
    }
    const int pl = owner[k];
    const bool i_am_pivot = me == pl;
    hc[k] = from(tau, pl);
#pragma unroll
    for (int r = k + 1; r < N; ++r)
      vk[k][r] = from(ess[r], pl);
    if (i_am_pivot) {
      col[k] = beta;
#pragma unroll
      for (int r = k + 1; r < N; ++r)
        col[r] = ess[r];
    }
    const bool later = pos > k && me < N; // my column is still to the right of the pivot
    if (N - k > 1) {
      float tmp = 0.f;
#pragma unroll
      for (int r = k + 1; r < N; ++r)
        tmp += vk[k][r] * col[r];
      tmp += col[k];
      const float ck = col[k] - hc[k] * tmp;
      const bool apply = later && hc[k] != 0.f;
      col[k] = apply ? ck : col[k];
#pragma unroll
      for (int r = k + 1; r < N; ++r) {
        const float cr = col[r] - tmp * (hc[k] * vk[k][r]);
        col[r] = apply ? cr : col[r];
      }
    }
    { // norm down-dating of my column
      float temp = __builtin_fabsf(col[k]) / normU;
      temp = (1.f + temp) * (1.f - temp);
      temp = temp < 0.f ? 0.f : temp;
      const float ratio = normU / normD;
      const float temp2 = temp * (ratio * ratio);
      float s = 0.f;
#pragma unroll
      for (int r = k + 1; r < N; ++r)
        s += col[r] * col[r];
      const float fresh = __builtin_sqrtf(s), scaled = normU * __builtin_sqrtf(temp);
      const bool live = later && normU != 0.f, recompute = temp2 <= norm_downdate_threshold;
      normD = live && recompute ? fresh : normD;
      normU = live ? (recompute ? fresh : scaled) : normU;
    }
  }
  if (nonzero_pivots == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i)
      x[i] = 0.f;
    return;
  }
  float cv[N];
#pragma unroll
  for (int i = 0; i < N; ++i)
    cv[i] = bin[i];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    if (k < nonzero_pivots) {
      if (N - k == 1) {
        cv[k] *= 1.f - hc[k];
      } else if (hc[k] != 0.f) {
        float tmp = 0.f;
#pragma unroll
        for (int r = k + 1; r < N; ++r)
          tmp += vk[k][r] * cv[r];
        tmp += cv[k];
        cv[k] -= hc[k] * tmp;
#pragma unroll
        for (int r = k + 1; r < N; ++r)
          cv[r] -= tmp * (hc[k] * vk[k][r]);
      }
    }
  }
  // the triangular factor, gathered from the lanes that own its columns before the (sequential) back-substitution
  // needs it: 21 independent permutes in flight at once instead of one round trip per use
  float R[N][N];
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int r = 0; r <= i; ++r)
      R[i][r] = from(col[r], owner[i]);
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    if (i < nonzero_pivots) {
      cv[i] = cv[i] / R[i][i];
#pragma unroll
      for (int r = 0; r < i; ++r)
        cv[r] -= cv[i] * R[i][r];
    } else {
      cv[i] = 0.f;
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i)
    x[i] = cv[i];
#pragma unroll
  for (int k = N - 1; k >= 0; --k) {
#pragma unroll
    for (int j = k + 1; j < N; ++j)
      if (trans[k] == j) {
        const float t = x[k];
        x[k] = x[j];
        x[j] = t;
      }
  }
}


// S holds the raw sums (upper triangle row-major, b, chi); p += dp.
template <int P, bool SAFE>
__device__ __forceinline__ bool damped_step(const Sums<P> &S, float lambda, float scaling,
                                            float (&p)[6], bool starved, float *dp_out = nullptr,
                                            bool row16 = false) {
  // U[i][j], i <= j: starts as the scaled, damped upper triangle of A
  float U[P][P], d[P], inv_d[P], y[P], x[P];
  int idx = 0;
  float dmax = 0.f;
#pragma unroll
  for (int i = 0; i < P; ++i) {
#pragma unroll
    for (int j = i; j < P; ++j) {
      float a = S.v[idx++] * scaling; // :647-651
      if (i == j) {
        a *= (1.f + lambda); // :664
        dmax = fmaxf(dmax, a);
      }
      U[i][j] = a;
    }
    y[i] = S.v[Sums<P>::NA + i] * scaling;
  }
  // A pivot d_j is what remains of the diagonal entry after eliminating the earlier
  // parameters; d_j / A_jj is scale free.  Healthy speckle gives >= 0.1; a damped singular
  // system gives ~lambda.  The SAFE flavour switches to the reference's QR below 1e-3; the fast
  // flavour factors through down to LK_FAST_PIVOT and hands the sector to the SAFE kernel below.
  // A starved level (see evaluate<>) always takes the reference's solver: its sums are
  // bit-identical to the reference's, so the whole trajectory is.
  bool well_conditioned = !starved;
  if (!(SAFE && starved)) // (a starved level goes straight to the reference's solver)
#pragma unroll
  for (int j = 0; j < P; ++j) {
    float w[P > 1 ? P : 1];
    const float ajj = U[j][j];
    float dj = ajj;
#pragma unroll
    for (int k = 0; k < j; ++k) {
      w[k] = U[k][j] * d[k];
      dj = __builtin_fmaf(-U[k][j], w[k], dj);
    }
    const bool ok = dj > ajj * (SAFE ? 1e-3f : LK_FAST_PIVOT) && dj > dmax * 1e-7f; // false for NaN as well
    well_conditioned = well_conditioned && ok;
    d[j] = (SAFE || ok) ? dj : 0.f;
    // v_rcp_f32 (1 ulp) instead of a correctly rounded division: this factorisation is not
    // bit-matched to anything, and it saves ~55 instructions per solve
    inv_d[j] = (SAFE || ok) ? __builtin_amdgcn_rcpf(dj) : 0.f; // fast flavour: a bad pivot zeroes that parameter's step
#pragma unroll
    for (int i = j + 1; i < P; ++i) {
      float t = U[j][i];
#pragma unroll
      for (int k = 0; k < j; ++k)
        t = __builtin_fmaf(-w[k], U[k][i], t);
      U[j][i] = t * inv_d[j];
    }
  }
  if (!SAFE || well_conditioned) {
    // U^T y' = b (forward), z = y'/d, U x = z (backward)
#pragma unroll
    for (int j = 0; j < P; ++j) {
#pragma unroll
      for (int k = 0; k < j; ++k)
        y[j] = __builtin_fmaf(-U[k][j], y[k], y[j]);
    }
#pragma unroll
    for (int j = P - 1; j >= 0; --j) {
      float t = y[j] * inv_d[j];
#pragma unroll
      for (int i = j + 1; i < P; ++i)
        t = __builtin_fmaf(-U[j][i], x[i], t);
      x[j] = t;
    }
  } else if constexpr (SAFE) {
    // rebuild the damped symmetric matrix exactly as the reference does (:647-665) and
    // solve it the reference's way
    float M[P * P], b[P];
    int q = 0;
#pragma unroll
    for (int p1 = 0; p1 < P; ++p1) {
      b[p1] = S.v[Sums<P>::NA + p1] * scaling;
#pragma unroll
      for (int p2 = p1; p2 < P; ++p2) {
        float a = S.v[q++] * scaling;
        if (p1 == p2)
          a *= (1.f + lambda);
        M[p1 * P + p2] = a;
        M[p2 * P + p1] = a;
      }
    }
    if (row16) // every lane of the 16-lane row holds the same system: spread the QR over them
      colpiv_qr_solve_row16<P>(M, b, x);
    else
      colpiv_qr_solve<P>(M, b, x);
  }
#pragma unroll
  for (int i = 0; i < P; ++i) {
    p[i] += x[i]; // :687-688
    if (dp_out)
      dp_out[i] = x[i];
  }
  return well_conditioned; // false: a pivot was bad (fast flavour: that parameter's step is zero; SAFE: the QR ran)
}

// The fast flavour (damped_step<6, false>) on sums that row16_reduce_scatter28 left spread over the 16-lane row: s0, s1
// are the lane's two totals.  The lane scales its own two sums (2 multiplications instead of 27), every lane then
// collects the 27 scaled values by row_newbcast, and from there on each element sees the operations of damped_step<>
// in the same order: (1 + lambda) on the diagonal, dmax, the fma chains of the root-free Cholesky, the pivot test,
// the zeroed step of a bad pivot, both substitutions.  Same bits in x, p and the returned flag
// (tests/test_distributed_step_gpu.py runs both in one launch).
__device__ __forceinline__ bool damped_step_scattered(float s0, float s1, float lambda, float scaling, float (&p)[6],
                                                      float *dp_out = nullptr) {
  constexpr int P = 6, NA = Sums<P>::NA;
  s0 *= scaling; // :647-651
  s1 *= scaling;
  float S[NA + P];
  gather_scattered(S, s0, s1, std::make_integer_sequence<int, NA + P>{});
  float U[P][P], d[P], inv_d[P], y[P], x[P];
  int idx = 0;
  float dmax = 0.f;
#pragma unroll
  for (int i = 0; i < P; ++i) {
#pragma unroll
    for (int j = i; j < P; ++j) {
      float a = S[idx++];
      if (i == j) {
        a *= (1.f + lambda); // :664
        dmax = fmaxf(dmax, a);
      }
      U[i][j] = a;
    }
    y[i] = S[NA + i];
  }
  bool well_conditioned = true;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    float w[P];
    const float ajj = U[j][j];
    float dj = ajj;
#pragma unroll
    for (int k = 0; k < j; ++k) {
      w[k] = U[k][j] * d[k];
      dj = __builtin_fmaf(-U[k][j], w[k], dj);
    }
    const bool ok = dj > ajj * LK_FAST_PIVOT && dj > dmax * 1e-7f; // false for NaN as well
    well_conditioned = well_conditioned && ok;
    d[j] = ok ? dj : 0.f;
    inv_d[j] = ok ? __builtin_amdgcn_rcpf(dj) : 0.f;
#pragma unroll
    for (int i = j + 1; i < P; ++i) {
      float t = U[j][i];
#pragma unroll
      for (int k = 0; k < j; ++k)
        t = __builtin_fmaf(-w[k], U[k][i], t);
      U[j][i] = t * inv_d[j];
    }
  }
#pragma unroll
  for (int j = 0; j < P; ++j) {
#pragma unroll
    for (int k = 0; k < j; ++k)
      y[j] = __builtin_fmaf(-U[k][j], y[k], y[j]);
  }
#pragma unroll
  for (int j = P - 1; j >= 0; --j) {
    float t = y[j] * inv_d[j];
#pragma unroll
    for (int i = j + 1; i < P; ++i)
      t = __builtin_fmaf(-U[j][i], x[i], t);
    x[j] = t;
  }
#pragma unroll
  for (int i = 0; i < P; ++i) {
    p[i] += x[i]; // :687-688
    if (dp_out)
      dp_out[i] = x[i];
  }
  return well_conditioned;
}

// translate_model_parameters (pyramid_class.cpp:260-287)
template <int P> __device__ __forceinline__ void translate(float (&p)[6], int src, int dst) {
  float mag = (dst - src > 0) ? 1.f / (float)(1 << (dst - src)) : (float)(1 << (src - dst));
  p[0] *= mag;
  if (P > 1)
    p[1] *= mag;
}

} // namespace
