// lk_sector_eval.hpp - device side of the passes in which a lane group evaluates a sector's samples (lk_backward.hip,
// lk_uncertainty.hip, the photometry of lk_residual.hip): the sector as a lane sees it at one pyramid level, its k-th
// sample, the undeformed node of a sample, the fixed-order group reduction in double, and the model x interpolator x
// group dispatch of the launchers.  On top of the solve's own header (warps, samplers, translate<>).  A new pass that
// evaluates records starts here ("adding a pass").
#pragma once
#include "lk_device.hpp"
#include "lk_solver_common.hpp"

#include <type_traits>

namespace {

// ---- the sector at a level -------------------------------------------------------------------------------------------------
struct SectorLevel { // what a lane needs to know about its sector at the current level
  gptr<uint8_t> und, def;
  gptr<f32x2> xy; // explicit list (the reference's order), already offset to the sector's first sample
  int rx, ry, rw; // implicit rectangle: first x, first y, width (rw == 0: explicit list)
  int n;
  int urows, ucols, drows, dcols;
  float cx, cy, inv_w;
};

// C: SectorLevel, or a struct that begins with one (lk_backward.hip adds its template slots); lv: the level's images, lists
// and rectangles - a row of the engine's table (LkLevelView, device memory) or a kernel's own arguments
// (LkSectorEvalArgs), which name them alike; c0: the sector's level-0 centre
template <class C = SectorLevel, class View>
__device__ __forceinline__ C sector_level(const View &lv, int s, int level, float2 c0) {
  C c;
  const int4 rc = lv.rect[s];
  const uint32_t off = lv.off[s];
  c.und = (gptr<uint8_t>)lv.und;
  c.def = (gptr<uint8_t>)lv.def;
  c.xy = (gptr<f32x2>)(lv.xy + off);
  c.rx = rc.x;
  c.ry = rc.y;
  c.rw = rc.z;
  c.n = rc.z > 0 ? rc.w : (int)(lv.off[s + 1] - off);
  c.urows = lv.urows;
  c.ucols = lv.ucols;
  c.drows = lv.drows;
  c.dcols = lv.dcols;
  const float inv = 1.f / (float)(1 << level); // pyramid_class.cpp:357-361, as the forward kernels
  c.cx = level == 0 ? c0.x : c0.x * inv;
  c.cy = level == 0 ? c0.y : c0.y * inv;
  c.inv_w = c.rw > 0 ? 1.f / (float)c.rw : 0.f;
  return c;
}

// sample k of the sector: implicit rectangles row by row (neighbouring lanes read neighbouring pixels), lists in their order
__device__ __forceinline__ f32x2 sector_sample(const SectorLevel &c, int k) {
  if (c.rw > 0) {
    int row = (int)((float)k * c.inv_w);
    int col = k - row * c.rw;
    if (col < 0) {
      col += c.rw;
      --row;
    } else if (col >= c.rw) {
      col -= c.rw;
      ++row;
    }
    f32x2 q;
    q.x = (float)(c.rx + col);
    q.y = (float)(c.ry + row);
    return q;
  }
  return c.xy[k];
}

// the undeformed node of sample q: the node the forward residual reads
__device__ __forceinline__ float sector_und_node(const SectorLevel &c, f32x2 q) {
  int uix = (int)(q.x + 0.5f), uiy = (int)(q.y + 0.5f);
  uix = min(max(uix, 0), c.ucols - 1); // (memory safety only; valid lists never clamp)
  uiy = min(max(uiy, 0), c.urows - 1);
  return (float)c.und[(size_t)uiy * (size_t)c.ucols + (size_t)uix];
}

// ---- the group reduction in double -----------------------------------------------------------------------------------------
template <int CTRL> __device__ __forceinline__ double dpp_get_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_f64(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
__device__ __forceinline__ double max_f64(double a, double b) { return a > b ? a : b; } // (for values that are never a NaN)

// v[0 .. NSUM) summed and v[NSUM .. NSUM + NMAX) maximised over the group, in the order of bw_reduce (lk_backward.hip): four
// DPP stages inside the rows of 16 lanes, four readlanes across the rows of a wavefront, LDS across the wavefronts in
// wavefront order; every lane ends with the same bits.  GROUP <= 64 uses no barrier; GROUP == 512 is the whole (uniform)
// workgroup, which calls this once: one barrier.  lds: (GROUP / 64) * STRIDE doubles when GROUP > 64, else unused.
template <int GROUP, int NSUM, int NMAX, int STRIDE>
__device__ __forceinline__ void reduce_f64(double (&v)[NSUM + NMAX], double *lds) {
  constexpr int N = NSUM + NMAX;
  auto stage = [&](auto ctrl) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const double o = dpp_get_f64<decltype(ctrl)::value>(v[i]);
      v[i] = i < NSUM ? v[i] + o : max_f64(v[i], o);
    }
  };
  stage(std::integral_constant<int, 0xB1>{});  // quad_perm [1,0,3,2]
  stage(std::integral_constant<int, 0x4E>{});  // quad_perm [2,3,0,1]
  stage(std::integral_constant<int, 0x141>{}); // row_half_mirror
  stage(std::integral_constant<int, 0x140>{}); // row_mirror
  if constexpr (GROUP >= 64) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const double r0 = readlane_f64(v[i], 0), r16 = readlane_f64(v[i], 16), r32 = readlane_f64(v[i], 32), r48 = readlane_f64(v[i], 48);
      v[i] = i < NSUM ? (r0 + r16) + (r32 + r48) : max_f64(max_f64(r0, r16), max_f64(r32, r48));
    }
  }
  if constexpr (GROUP > 64) {
    static_assert(N <= STRIDE, "reduction slot");
    constexpr int WAVES = GROUP / kWave;
    const int wave = (int)threadIdx.x / kWave;
    if ((int)threadIdx.x % kWave == 0) {
#pragma unroll
      for (int i = 0; i < N; ++i)
        lds[wave * STRIDE + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) {
      double t = lds[i];
      for (int w = 1; w < WAVES; ++w)
        t = i < NSUM ? t + lds[w * STRIDE + i] : max_f64(t, lds[w * STRIDE + i]);
      v[i] = t;
    }
  }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------
// f(std::integral_constant<int, VALUE>) for the run-time value; an unknown value takes the last case, as the solve's ladders
template <class F> hipError_t dispatch_model(int model, F &&f) {
  switch (model) {
  case LK_FM_U: return f(std::integral_constant<int, LK_FM_U>{});
  case LK_FM_UV: return f(std::integral_constant<int, LK_FM_UV>{});
  case LK_FM_UVQ: return f(std::integral_constant<int, LK_FM_UVQ>{});
  default: return f(std::integral_constant<int, LK_FM_UVUXUYVXVY>{});
  }
}
template <class F> hipError_t dispatch_interp(int interp, F &&f) {
  switch (interp) {
  case LK_IM_NEAREST: return f(std::integral_constant<int, LK_IM_NEAREST>{});
  case LK_IM_BILINEAR: return f(std::integral_constant<int, LK_IM_BILINEAR>{});
  case LK_IM_BICUBIC: return f(std::integral_constant<int, LK_IM_BICUBIC>{});
  default: return f(std::integral_constant<int, LK_IM_BICUBIC_SEPARABLE>{});
  }
}
// the lane groups of lk_bw_group: 16, 64, else 512
template <class F> hipError_t dispatch_group(int group, F &&f) {
  switch (group) {
  case 16: return f(std::integral_constant<int, 16>{});
  case 64: return f(std::integral_constant<int, 64>{});
  default: return f(std::integral_constant<int, 512>{});
  }
}
// f(model, interp, group), each a std::integral_constant
template <class F> hipError_t dispatch_sector_kernel(int model, int interp, int group, F &&f) {
  return dispatch_model(model, [&](auto m) {
    return dispatch_interp(interp, [&](auto i) { return dispatch_group(group, [&](auto g) { return f(m, i, g); }); });
  });
}

// A kernel of `n_sectors` lane groups: rows and wavefronts share workgroups of 256 threads, a 512-lane group is its own.
// From inside dispatch_sector_kernel: launch_sector_groups<GROUP>(the_kernel<MODEL, INTERP, GROUP>, args, n_sectors, stream).
template <int GROUP> constexpr int sector_group_threads() { return GROUP <= 64 ? 256 : GROUP; }
// the workgroups launch_sector_groups makes for n_sectors lane groups (what a launch report records as its grid)
template <int GROUP> constexpr int sector_group_blocks(int n_sectors) {
  constexpr int per_block = sector_group_threads<GROUP>() / GROUP;
  return (n_sectors + per_block - 1) / per_block;
}
template <int GROUP, class Args> hipError_t launch_sector_groups(void (*kernel)(Args), const Args &a, int n_sectors, hipStream_t st) {
  const int blocks = sector_group_blocks<GROUP>(n_sectors);
  if (blocks <= 0)
    return hipSuccess;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(sector_group_threads<GROUP>()), 0, st, a);
  return hipGetLastError();
}

} // namespace
