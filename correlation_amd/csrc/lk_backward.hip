// lk_backward.hip - the backward update (lk_set_update(LK_UPDATE_BACKWARD)): an inverse-compositional Levenberg-Marquardt
// solve, IC-GN in the DIC literature (include/lk_engine.h and DESIGN.md section 13 have the semantics).
//
// One lane group owns one sector for its whole coarse-to-fine solve: a 16-lane DPP row, a wavefront or a 512-thread
// workgroup, chosen from the sector's level-0 sample count alone (lk_bw_group).  Per level the group makes one TEMPLATE
// pass over the undeformed image - T_i, the sampler's gradient at the integer node, H = sum G_i G_i^T with
// G_i = grad T_i . dW/dp - and stages {T_i, grad T_i} of every sample in a per-sector slot of global memory.  Every
// evaluation after that reads the slot back (one 16-byte load per sample), samples the deformed image's VALUE only and
// accumulates b = sum G_i V_i and chi = sum V_i^2: P + 1 FMAs per sample instead of the forward mode's 28, and no
// gradient monomials.  A rejected step needs no evaluation at all: H is fixed, the kept b of the last good parameters
// and the larger lambda give the next step.  Every lane of a group walks the same samples in every pass (lane j: samples
// j, j + G, j + 2G, ...), so a lane reads only the template slots it wrote itself, and the reductions (DPP inside rows,
// readlane across rows, LDS across wavefronts) have one fixed order: a sector's record is the same bits in any launch.
#include "lk_device.hpp"
#include "lk_compose.hpp"
#include "lk_launch.hpp"
#include "lk_sector_eval.hpp"

namespace {

constexpr int kBwLdsStride = 32; // floats per wavefront in the cross-wavefront reduction (22 used at most)

struct BwLevel : SectorLevel {
  float4 *tpl; // the sector's template slots
};

// Sum of N values over the group; every lane of the group ends with the same bits.  GROUP <= 64 uses no barrier (the rows
// of a wavefront may be at different points of their sectors' solves); GROUP == 512 is the whole (uniform) workgroup.
template <int GROUP, int N> __device__ __forceinline__ void bw_reduce(float (&v)[N], float *lds) {
#pragma unroll
  for (int i = 0; i < N; ++i)
    v[i] = dpp_add<0xB1>(v[i]); // quad_perm [1,0,3,2]
#pragma unroll
  for (int i = 0; i < N; ++i)
    v[i] = dpp_add<0x4E>(v[i]); // quad_perm [2,3,0,1]
#pragma unroll
  for (int i = 0; i < N; ++i)
    v[i] = dpp_add<0x141>(v[i]); // row_half_mirror
#pragma unroll
  for (int i = 0; i < N; ++i)
    v[i] = dpp_add<0x140>(v[i]); // row_mirror
  if constexpr (GROUP >= 64) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[i]), 0));
      const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[i]), 16));
      const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[i]), 32));
      const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[i]), 48));
      v[i] = (r0 + r1) + (r2 + r3);
    }
  }
  if constexpr (GROUP > 64) {
    static_assert(N <= kBwLdsStride, "reduction slot");
    constexpr int WAVES = GROUP / kWave;
    const int wave = (int)threadIdx.x / kWave;
    __syncthreads(); // previous readers of lds are done
    if ((int)threadIdx.x % kWave == 0) {
#pragma unroll
      for (int i = 0; i < N; ++i)
        lds[wave * kBwLdsStride + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) {
      float t = lds[i];
      for (int w = 1; w < WAVES; ++w)
        t += lds[w * kBwLdsStride + i];
      v[i] = t;
    }
  }
}

// The template pass of one level: stages {T_i, dT/dx, dT/dy, 0} and returns H (upper triangle, row-major, unscaled);
// true when the sampler flags a node as out of the image.
template <int MODEL, int INTERP, int GROUP>
__device__ __forceinline__ bool bw_template(const BwLevel &c, int lane, float (&H)[n_params(MODEL) * (n_params(MODEL) + 1) / 2],
                                            float *lds) {
  constexpr int P = n_params(MODEL), NA = P * (P + 1) / 2;
  float v[NA + 1];
#pragma unroll
  for (int i = 0; i <= NA; ++i)
    v[i] = 0.f;
  const int umaxr = c.urows - 1, umaxc = c.ucols - 1;
  for (int k = lane; k < c.n; k += GROUP) {
    const f32x2 q = sector_sample(c, k);
    int uix = (int)(q.x + 0.5f), uiy = (int)(q.y + 0.5f); // the node the forward residual reads
    uix = min(max(uix, 0), umaxc);                          // (memory safety only; valid lists never clamp)
    uiy = min(max(uiy, 0), umaxr);
    const float T = (float)c.und[(size_t)uiy * (size_t)c.ucols + (size_t)uix];
    float W, gx, gy;
    if (!sample_def<INTERP>(c.und, c.urows, c.ucols, (float)uix, (float)uiy, W, gx, gy)) {
      v[NA] += 1.f;
      gx = 0.f;
      gy = 0.f;
    }
    c.tpl[k] = make_float4(T, gx, gy, 0.f);
    const float dx = q.x - c.cx, dy = q.y - c.cy; // (Warp<>::apply's)
    float G[P];
    Warp<MODEL>::jac(gx, gy, dx, dy, G);
    int idx = 0;
#pragma unroll
    for (int p1 = 0; p1 < P; ++p1)
#pragma unroll
      for (int p2 = p1; p2 < P; ++p2)
        v[idx] = __builtin_fmaf(G[p1], G[p2], v[idx]), ++idx;
  }
  bw_reduce<GROUP>(v, lds);
#pragma unroll
  for (int i = 0; i < NA; ++i)
    H[i] = v[i];
  return v[NA] != 0.f;
}

// One evaluation at p: b = sum G_i V_i, chi = sum V_i^2 (unscaled); true when a sample leaves the deformed image.
template <int MODEL, int INTERP, int GROUP>
__device__ __forceinline__ bool bw_evaluate(const BwLevel &c, int lane, const float (&p)[6], float (&b)[n_params(MODEL)],
                                            float &chi, float *lds) {
  constexpr int P = n_params(MODEL);
  float v[P + 2];
#pragma unroll
  for (int i = 0; i < P + 2; ++i)
    v[i] = 0.f;
  for (int k = lane; k < c.n; k += GROUP) {
    const f32x2 q = sector_sample(c, k);
    float xd, yd, dx = 0.f, dy = 0.f;
    Warp<MODEL>::apply(q.x, q.y, c.cx, c.cy, p, xd, yd, dx, dy);
    const float4 t = c.tpl[k];
    float W;
    if (!sample_def_value<INTERP>(c.def, c.drows, c.dcols, xd, yd, W)) {
      v[P + 1] += 1.f;
      continue; // the sums of an evaluation that hit the error are never used
    }
    const float V = t.x - W;
    float G[P];
    Warp<MODEL>::jac(t.y, t.z, dx, dy, G);
#pragma unroll
    for (int i = 0; i < P; ++i)
      v[i] = __builtin_fmaf(G[i], V, v[i]);
    v[P] = __builtin_fmaf(V, V, v[P]);
  }
  bw_reduce<GROUP>(v, lds);
#pragma unroll
  for (int i = 0; i < P; ++i)
    b[i] = v[i];
  chi = v[P];
  return v[P + 1] != 0.f;
}

// delta = the damped solve of (H / n, b / n) with lambda (compute_model_parameters' scaling and damping, the SAFE solver:
// root-free Cholesky, the restated QR for ill-conditioned and starved levels); out = W(p) o W(-delta)^-1.  Returns false
// for a singular step (out untouched).  `ill`: the system met a bad pivot outside a starved level.
template <int P>
__device__ __forceinline__ bool bw_step(const float *H, const float (&b)[P], float lambda, float scaling, bool starved,
                                        const float (&p)[6], float (&out)[6], uint32_t &ill, int model) {
  Sums<P> S;
#pragma unroll
  for (int i = 0; i < Sums<P>::NA; ++i)
    S.v[i] = H[i];
#pragma unroll
  for (int i = 0; i < P; ++i)
    S.v[Sums<P>::NA + i] = b[i];
  S.v[Sums<P>::N - 1] = 0.f;
  float dummy[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, delta[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const bool wc = damped_step<P, true>(S, lambda, scaling, dummy, starved, delta);
  if (!wc && !starved)
    ++ill;
  float q[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < P; ++i)
    q[i] = -delta[i];
  return lk_compose_inverse_impl(model, p, q, out) == 0;
}

template <int MODEL, int INTERP, int GROUP>
__global__ void __launch_bounds__(GROUP <= 64 ? 256 : GROUP) lk_backward_kernel(LkBackwardArgs a) {
  constexpr int THREADS = GROUP <= 64 ? 256 : GROUP;
  constexpr int P = n_params(MODEL), NA = P * (P + 1) / 2;
  __shared__ float lds[(GROUP > 64 ? GROUP / kWave : 1) * kBwLdsStride];
  const int gid = (int)blockIdx.x * (THREADS / GROUP) + (int)threadIdx.x / GROUP;
  const int lane = (int)threadIdx.x % GROUP;
  if (gid >= a.n_sectors) // (GROUP == 512: the whole workgroup; GROUP <= 64: whole rows / wavefronts, no barriers below)
    return;
  const int s = (int)a.order[gid];
  const float2 c0 = a.center[s];
  float4 *tpl = a.tpl + a.tpl_base[s];
  float p[6], evaluated[6], lg_p[6], saved[6], tent[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    p[i] = i < P ? a.guess[(size_t)s * 6 + i] : 0.f;
    evaluated[i] = p[i];
    lg_p[i] = saved[i] = tent[i] = 0.f;
  }
  float H[NA], b[P], kb[P];
  const float min_lambda = 1e-9f, max_lambda = 1e9f;
  float lambda = 0.0001f, lg_chi = FLT_MAX;
  int reached = 0, error = LK_ERROR_NONE, level_old = 0;
  int evaluated_level = 0; // the level `evaluated` is scaled for (the guess: level 0)
  uint32_t n_evals = 0, n_sample_evals = 0, n_point_iters = 0, n_ill = 0;
  bool early = false;
  for (int level = a.py_stop; level >= a.py_start; level -= a.py_step) { // Newton_Raphson's level loop (:373-408)
    translate<P>(p, level_old, level);
    error = LK_ERROR_NONE;
    lambda = 0.0001f;
    lg_chi = FLT_MAX;
    BwLevel c = sector_level<BwLevel>(a.lv[level], s, level, c0);
    c.tpl = tpl;
    const float scaling = 1.f / ((float)c.n);
    const bool starved = c.n <= a.starved_max;
    if (bw_template<MODEL, INTERP, GROUP>(c, lane, H, lds)) {
      error = LK_ERROR_INTERPOLATION_OUT_OF_IMAGE; // as a failed evaluation #0 (which counts its point iteration)
      early = true;
      ++n_point_iters;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i)
      lg_p[i] = p[i];
    bool first = true, use_saved = true, saved_ok = false;
    int iteration = 0;
    // one evaluation site: the first pass is evaluation #0, every further one an LM trip (:439-529)
    while (!early) {
      bool ok = true;
      if (first) {
#pragma unroll
        for (int i = 0; i < 6; ++i)
          tent[i] = p[i];
      } else {
        ++iteration;
        if (iteration > a.max_iters || lambda >= max_lambda) {
          error = LK_ERROR_CORRELATION_MAX_ITERS_REACHED;
          break;
        }
        reached = iteration;
        if (use_saved) {
#pragma unroll
          for (int i = 0; i < 6; ++i)
            tent[i] = saved[i];
          ok = saved_ok;
        } else { // rejected: the next step from the kept b of the last good parameters, no evaluation
#pragma unroll
          for (int i = 0; i < 6; ++i)
            p[i] = lg_p[i];
          ok = bw_step<P>(H, kb, lambda, scaling, starved, lg_p, tent, n_ill, MODEL);
        }
      }
      ++n_point_iters;
      float chi = __int_as_float(0x7f800000); // a singular step diverges
      if (ok) {
#pragma unroll
        for (int i = 0; i < 6; ++i)
          p[i] = evaluated[i] = tent[i];
        evaluated_level = level;
        const bool bad = bw_evaluate<MODEL, INTERP, GROUP>(c, lane, tent, b, chi, lds);
        ++n_evals;
        n_sample_evals += (uint32_t)c.n;
        if (bad) {
          error = LK_ERROR_INTERPOLATION_OUT_OF_IMAGE;
          early = first;
          break;
        }
        chi *= scaling;
        float la = lambda;
        if (!first) { // look-ahead step with the lambda an accepted trip will have (:521)
          la = lambda * 0.4f;
          if (!(la > min_lambda))
            la = min_lambda;
        }
        saved_ok = bw_step<P>(H, b, la, scaling, starved, tent, saved, n_ill, MODEL);
        if (saved_ok) {
#pragma unroll
          for (int i = 0; i < 6; ++i)
            p[i] = saved[i];
        }
      }
      if (first) {
        lg_chi = chi;
#pragma unroll
        for (int i = 0; i < P; ++i)
          kb[i] = b[i];
        first = false;
        continue;
      }
      const float lg = lg_chi;
      const float mx = lg < chi ? chi : lg;
      const float delta_chi = fabsf((lg - chi) / (mx + a.precision));
      if (chi <= lg) {
        lg_chi = chi;
        const float la = lambda * 0.4f;
        lambda = la > min_lambda ? la : min_lambda;
#pragma unroll
        for (int i = 0; i < 6; ++i)
          lg_p[i] = tent[i];
#pragma unroll
        for (int i = 0; i < P; ++i)
          kb[i] = b[i];
        use_saved = true;
      } else {
        const float la = lambda * 10.0f;
        lambda = la < max_lambda ? la : max_lambda;
        use_saved = false;
      }
      if (delta_chi < a.precision)
        break;
    }
    if (early) {
      translate<P>(p, level, 0);
      break;
    }
    level_old = level;
  }
  if (!early)
    translate<P>(p, level_old, 0);
  translate<P>(evaluated, evaluated_level, 0); // (the forward kernels' rule: level-0 scale, whichever level it ran at)
  if (lane == 0) {
    lk_result r;
#pragma unroll
    for (int i = 0; i < 6; ++i)
      r.resultingParameters[i] = i < P ? p[i] : 0.f;
    r.chi = lg_chi;
    const int4 rc0 = a.lv[0].rect[s];
    r.numberOfPoints = rc0.z > 0 ? rc0.w : (int)(a.lv[0].off[s + 1] - a.lv[0].off[s]);
    r.iterations = reached;
    r.errorCode = error;
    r.undCenterX = c0.x;
    r.undCenterY = c0.y;
    a.result[s] = r;
    if (a.last_p) {
#pragma unroll
      for (int i = 0; i < 6; ++i)
        a.last_p[(size_t)s * 6 + i] = r.resultingParameters[i];
    }
    if (a.last_eval_p) { // (the forward kernels' rule: the last evaluation's parameters, or the returned ones if py_start > 0)
#pragma unroll
      for (int i = 0; i < 6; ++i)
        a.last_eval_p[(size_t)s * 6 + i] = a.py_start == 0 ? evaluated[i] : r.resultingParameters[i];
    }
    if (a.stats) {
      a.stats[(size_t)s * 4 + 0] = n_evals;
      a.stats[(size_t)s * 4 + 1] = n_sample_evals;
      a.stats[(size_t)s * 4 + 2] = n_point_iters;
      a.stats[(size_t)s * 4 + 3] = n_ill;
    }
  }
}

// lk_evaluate_backward: the template pass and one evaluation of one sector, by the group its solve uses
template <int MODEL, int INTERP, int GROUP>
__global__ void __launch_bounds__(GROUP) lk_backward_eval_kernel(LkBackwardEvalArgs a) {
  constexpr int P = n_params(MODEL), NA = P * (P + 1) / 2;
  __shared__ float lds[(GROUP > 64 ? GROUP / kWave : 1) * kBwLdsStride];
  const int lane = (int)threadIdx.x;
  BwLevel c = sector_level<BwLevel>(a.lv[a.level], a.sector, a.level, a.center[a.sector]);
  c.tpl = a.tpl;
  float H[NA], b[P], chi;
  const bool tbad = bw_template<MODEL, INTERP, GROUP>(c, lane, H, lds);
  float p[6];
#pragma unroll
  for (int i = 0; i < 6; ++i)
    p[i] = a.p[i];
  const bool ebad = bw_evaluate<MODEL, INTERP, GROUP>(c, lane, p, b, chi, lds);
  if (lane == 0) {
    int idx = 0;
    for (int i = 0; i < 36; ++i)
      a.out[i] = 0.f;
    for (int i = 0; i < P; ++i)
      for (int j = i; j < P; ++j) {
        a.out[i * 6 + j] = H[idx];
        a.out[j * 6 + i] = H[idx];
        ++idx;
      }
    for (int i = 0; i < 6; ++i)
      a.out[36 + i] = i < P ? b[i] : 0.f;
    a.out[42] = chi;
    a.out[43] = (tbad || ebad) ? 1.f : 0.f;
  }
}

} // namespace

// What lk_get_launch_report tells about a backward launch, noted where M, I and G are compile-time values: the SAFE solver,
// no frame pipeline, no team, no queue.
template <int M, int I, int G> static inline void bw_report(lk_launch_record *rep, int role, int threads, int sectors, int grid) {
  if (rep)
    *rep = lk_launch_record{M, I, G, threads, LK_FLAVOUR_SAFE, 0, role, sectors, 0, 0, grid, 0};
}

hipError_t lk_launch_backward(const LkBackwardArgs &a, int model, int interp, int group, hipStream_t st, lk_launch_record *rep) {
  return dispatch_sector_kernel(model, interp, group, [&](auto m, auto i, auto g) {
    constexpr int M = decltype(m)::value, I = decltype(i)::value, G = decltype(g)::value;
    bw_report<M, I, G>(rep, LK_LAUNCH_BACKWARD, sector_group_threads<G>(), a.n_sectors, sector_group_blocks<G>(a.n_sectors));
    return launch_sector_groups<G>(lk_backward_kernel<M, I, G>, a, a.n_sectors, st);
  });
}

hipError_t lk_launch_backward_eval(const LkBackwardEvalArgs &a, int model, int interp, int group, hipStream_t st,
                                   lk_launch_record *rep) {
  return dispatch_sector_kernel(model, interp, group, [&](auto m, auto i, auto g) {
    constexpr int M = decltype(m)::value, I = decltype(i)::value, G = decltype(g)::value;
    bw_report<M, I, G>(rep, LK_LAUNCH_BACKWARD_EVAL, G, 1, 1); // (one workgroup of G threads, not sector_group_threads<G>())
    hipLaunchKernelGGL((lk_backward_eval_kernel<M, I, G>), dim3(1), dim3(G), 0, st, a);
    return hipGetLastError();
  });
}
