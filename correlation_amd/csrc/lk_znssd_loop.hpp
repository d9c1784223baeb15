// lk_znssd_loop.hpp - the loop of the ZNSSD refinement, one body for the passes that differ in how the deformed image is
// sampled or in how its samples are weighted: lk_znssd.hip (the engine's interpolator, lk_refine_znssd; DESIGN.md section
// 23), lk_spline.hip (a B-spline of the prefiltered image, lk_refine_spline; section 25) and lk_weighted.hip (the engine's
// interpolator under a Gaussian window and a pixel mask, lk_refine_weighted; section 26).  Device only.
//
// One lane group refines one sector from its seed to the end, at the finest level the solve reaches: a 16-lane DPP row, a
// wavefront or a 512-thread workgroup, chosen from the sector's level-0 sample count alone (lk_bw_group).  An evaluation is
// lk_uncertainty.hip's walk with other sums: per sample, in float, f = the undeformed node, g and its gradient = the
// kernel's sampler at Warp<>::apply, H = Warp<>::jac; the products are formed and summed in double.  Lane j takes the samples j, j + G, ...;
// the reduction (lk_sector_eval.hpp) has one fixed order, so a sector's sums - and with them every decision of its
// Levenberg-Marquardt loop, its trajectory and its record - are the same bytes in any launch.
//
// Lane 0 of the group owns the loop: it keeps the sums of the best state in LDS (45 doubles per group, so the accumulators
// of the evaluation are the only large register array), turns them into the step with the function the host exports
// (lk_znssd.hpp), decides on the trial state, and hands the next trial parameters and the "go on" flag to the other lanes:
// a DPP row share in a 16-lane row, a readlane in a wavefront, LDS and a barrier in the 512-thread workgroup.  Flag and
// parameters are uniform over the group, so the loop's barriers are reached by all of its threads.
#pragma once
#include "lk_device.hpp"
#include "lk_neighbours.hpp"
#include "lk_sector_eval.hpp"
#include "lk_znssd.hpp"

namespace {

constexpr int kZnLdsStride = 48; // doubles per wavefront in the cross-wavefront reduction (46 used at most)

// reduce_f64 over the N sums.  In a 512-thread workgroup only lane 0 goes on to use them, and the compiler then moved the
// seven additions of every sum into lane 0's branch, holding the eight wavefronts' terms of all sums until there: 736
// registers, most of them in scratch.  The empty statement makes every sum a value that is needed here.
template <int GROUP, int N> __device__ __forceinline__ void zn_reduce(double (&v)[N], double *lds) {
  reduce_f64<GROUP, N, 0, kZnLdsStride>(v, lds);
  if constexpr (GROUP > 64) {
#pragma unroll
    for (int i = 0; i < N; ++i)
      asm volatile("" : "+v"(v[i]));
  }
}

// v of the group's lane 0 in every lane of the group (GROUP <= 64)
template <int GROUP> __device__ __forceinline__ float zn_from_lane0(float v) {
  if constexpr (GROUP == 16)
    return dpp_bcast<0>(v);
  else
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
}

// the shared good rule (reseed_good, lk_neighbours.hpp) with its loop over the parameters unrolled: the record stays live to
// the end of the kernel - a bad one is copied out - and an index the compiler does not resolve would move it out of registers
template <int P> __device__ __forceinline__ bool zn_good(const lk_result &r, float chi_max) {
  bool good = r.errorCode == LK_ERROR_NONE && finite_bits(r.chi);
#pragma unroll
  for (int i = 0; i < 6; ++i)
    good = good && (i >= P || finite_bits(r.resultingParameters[i]));
  return good && (!(chi_max > 0.f) || r.chi <= chi_max);
}

__device__ __forceinline__ int zn_error_code(int status) {
  switch (status) {
  case LK_ZN_CONVERGED: return LK_ERROR_NONE;
  case LK_ZN_MAX_ITERS:
  case LK_ZN_STALLED: return LK_ERROR_CORRELATION_MAX_ITERS_REACHED;
  case LK_ZN_OUT_OF_IMAGE: return LK_ERROR_INTERPOLATION_OUT_OF_IMAGE;
  case LK_ZN_BAD_SEED: return LK_ERROR_BAD_DOMAIN; // (a guess that is not finite; a bad record is copied instead)
  default: return LK_ERROR_SOLVER;
  }
}

// The weight policy of the passes that give every sample the weight 1 (lk_znssd.hip, lk_spline.hip): nothing of a weight is
// compiled into their kernels.  A policy with kWeighted = true (lk_weighted.hip) has
//   float of(const SectorLevel &c, f32x2 q) const        the weight of sample q, >= 0; the same float wherever it is asked for
//   bool too_few(int n_valid, int n) const               its own rule on top of n_valid < P + 2
//   void store(int s, const lk_znssd &o, const LkZnWeightSums &w, int level) const      the info record in place of a.out[s]
struct LkZnUnitWeight {
  static constexpr bool kWeighted = false;
};
// what the prologue of a weighted sector leaves: the samples with w > 0, sum w, sum w^2, sum w dx, sum w dy (level-L pixels
// about the committed centre)
struct LkZnWeightSums {
  int n_valid;
  double sw, sww, swx, swy;
};

// The body of a kernel of THREADS = 256 (GROUP <= 64) or GROUP threads.  sample(c, xd, yd, g, gx, gy): the deformed image
// and its gradient at a level-L position of the sector c, false where the sampler's window leaves the image.  weight: the
// policy above; with weights a sample of weight 0 is skipped before anything of it is read, every other term of the sums is
// formed as without weights and multiplied by (double)w before it is added, and N = sum w stands for (double)n.
template <int MODEL, int GROUP, class SAMPLER, class WEIGHT>
__device__ __forceinline__ void lk_znssd_sector(const LkZnssdArgs &a, const SAMPLER &sample, const WEIGHT &weight) {
  constexpr int THREADS = GROUP <= 64 ? 256 : GROUP;
  constexpr int P = n_params(MODEL);
  constexpr bool WEIGHTED = WEIGHT::kWeighted;
  using Y = LkZnLayout<P>;
  constexpr int NS = Y::N; // the sums and the flagged count
  __shared__ double lds[(GROUP > 64 ? GROUP / kWave : 1) * kZnLdsStride];
  __shared__ double s_kept[THREADS / GROUP][NS]; // the sums of the best state; lane 0 of the group alone touches its row
  __shared__ float s_try[8];                     // GROUP == 512: the trial parameters and the flag
  const int slot = (int)threadIdx.x / GROUP;
  const int gid = (int)blockIdx.x * (THREADS / GROUP) + slot;
  const int lane = (int)threadIdx.x % GROUP;
  if (gid >= a.n_sectors) // (GROUP == 512: the whole workgroup; GROUP <= 64: whole rows / wavefronts, no barriers below)
    return;
  const int s = (int)a.ev.order[gid], level = a.level;
  lk_result rec{};
  float seed[6]; // level-0 scale
  bool good;
  if (a.guess) {
    good = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      seed[i] = i < P ? a.guess[(size_t)s * 6 + i] : 0.f;
      good = good && finite_bits(seed[i]);
    }
  } else {
    rec = a.ev.rec[s];
    good = zn_good<P>(rec, a.chi_max);
#pragma unroll
    for (int i = 0; i < 6; ++i)
      seed[i] = i < P ? rec.resultingParameters[i] : 0.f;
  }
  const SectorLevel c = sector_level(a.ev, s, level, a.ev.center[s]);
  const int n = c.n;
  float p_cur[6], p_try[6];
#pragma unroll
  for (int i = 0; i < 6; ++i)
    p_cur[i] = seed[i];
  translate<P>(p_cur, 0, level); // the seed is in level-0 scale (pyramid_class.cpp:260-287, as the solve between levels)
#pragma unroll
  for (int i = 0; i < 6; ++i)
    p_try[i] = p_cur[i];
  double *kept = s_kept[slot];
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < NS; ++i)
      kept[i] = 0.0;
  }
  // the loop's state: lane 0's is the group's
  int status = LK_ZN_BAD_SEED, evals = 0, trips = 0;
  double lambda = (double)a.lambda0, crit = 0.0, last_step = 0.0, wstep = 0.0;
  LkZnCriterion best;
  best.crit = best.gain = best.offset = best.zncc = 0.0;
  float zncc_seed = 0.f;
  bool go = good;
  // with weights, the prologue: one pass over the samples' weights alone, one reduction in the fixed order
  [[maybe_unused]] LkZnWeightSums ws{0, 0.0, 0.0, 0.0, 0.0};
  if constexpr (WEIGHTED) {
    if (good) { // (uniform over the group, as everything the reduction leaves)
      double t[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      for (int k = lane; k < n; k += GROUP) {
        const f32x2 q = sector_sample(c, k);
        const float w = weight.of(c, q);
        if (w > 0.f) {
          const double wd = (double)w;
          t[0] += 1.0;
          t[1] += wd;
          t[2] += wd * wd;
          t[3] += wd * (double)(q.x - c.cx);
          t[4] += wd * (double)(q.y - c.cy);
        }
      }
      zn_reduce<GROUP>(t, lds);
      if constexpr (GROUP > 64)
        __syncthreads(); // (the first evaluation's reduction writes the slots these sums were read from)
      ws.n_valid = (int)t[0];
      ws.sw = t[1];
      ws.sww = t[2];
      ws.swx = t[3];
      ws.swy = t[4];
      if (ws.n_valid < P + 2 || weight.too_few(ws.n_valid, n)) { // nothing of the images is read
        status = LK_ZN_TOO_FEW;
        go = false;
      }
    }
  }
  // criterion and step of `sums`: n samples of weight 1, or the n_valid samples of total weight sum w
  auto criterion = [&](const double *sums, LkZnCriterion *out) {
    if constexpr (WEIGHTED)
      return lk_znssd_criterion<P>(ws.n_valid, ws.sw, sums, out);
    else
      return lk_znssd_criterion<P>(n, sums, out);
  };
  auto step = [&](const double *sums, double lam, double *delta, LkZnCriterion *out) {
    if constexpr (WEIGHTED)
      return lk_znssd_step<P>(ws.n_valid, ws.sw, sums, lam, delta, out);
    else
      return lk_znssd_step<P>(n, sums, lam, delta, out);
  };
  while (go) {
    double v[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i)
      v[i] = 0.0;
    for (int k = lane; k < n; k += GROUP) {
      const f32x2 q = sector_sample(c, k);
      [[maybe_unused]] double wd = 1.0;
      if constexpr (WEIGHTED) {
        const float w = weight.of(c, q);
        if (!(w > 0.f))
          continue; // not part of the sector: never sampled, never flagged
        wd = (double)w;
      }
      // term, or with weights term times w (a rounded product), added to acc
      auto add = [&](double &acc, double term) {
        if constexpr (WEIGHTED)
          acc += term * wd;
        else
          acc += term;
      };
      float xd, yd, dx = 0.f, dy = 0.f;
      Warp<MODEL>::apply(q.x, q.y, c.cx, c.cy, p_try, xd, yd, dx, dy);
      const float f = sector_und_node(c, q);
      float g, gx, gy;
      if (!sample(c, xd, yd, g, gx, gy)) {
        v[Y::FLAGGED] += 1.0;
        continue; // the sums of an evaluation that hit the error are never used
      }
      float H[P];
      Warp<MODEL>::jac(gx, gy, dx, dy, H);
      double Hd[P];
#pragma unroll
      for (int i = 0; i < P; ++i)
        Hd[i] = (double)H[i];
      const double fd = (double)f, gd = (double)g;
      add(v[0], fd);
      add(v[1], gd);
      add(v[2], fd * fd); // (no contraction: a rounded product, then a rounded sum)
      add(v[3], gd * gd);
      add(v[4], fd * gd);
      int idx = 0;
#pragma unroll
      for (int p1 = 0; p1 < P; ++p1) {
        add(v[Y::H + p1], Hd[p1]);
        add(v[Y::HF + p1], Hd[p1] * fd);
        add(v[Y::HG + p1], Hd[p1] * gd);
#pragma unroll
        for (int p2 = p1; p2 < P; ++p2)
          add(v[Y::HH + idx], Hd[p1] * Hd[p2]), ++idx;
      }
    }
    zn_reduce<GROUP>(v, lds);
    ++evals;
    if (lane == 0) {
      LkZnCriterion cr;
      cr.crit = cr.gain = cr.offset = cr.zncc = 0.0;
      const bool flagged = v[Y::FLAGGED] != 0.0;
      const int refused = flagged ? (int)LK_ZN_OUT_OF_IMAGE : criterion(v, &cr);
      bool done = false, keep = false;
      if (evals == 1) { // the seed
        keep = !flagged;
        if (refused != 0) {
          status = refused;
          done = true;
        } else {
          zncc_seed = (float)cr.zncc;
        }
      } else if (refused == 0 && cr.crit < crit) { // accepted
        keep = true;
#pragma unroll
        for (int i = 0; i < 6; ++i)
          p_cur[i] = p_try[i];
        const double down = 0.1 * lambda;
        lambda = down > 1e-9 ? down : 1e-9;
        last_step = wstep;
        if (wstep < (double)a.precision) {
          status = LK_ZN_CONVERGED;
          done = true;
        }
      } else if (refused == 0 && wstep < (double)a.precision) {
        // a step below the precision that does not lower the criterion: the float samples cannot resolve it - p stays
        status = LK_ZN_CONVERGED;
        done = true;
      } else {
        lambda = 10.0 * lambda;
        if (lambda >= 1e9) {
          status = LK_ZN_STALLED;
          done = true;
        }
      }
      if (keep) {
        best = cr;
        crit = cr.crit;
#pragma unroll
        for (int i = 0; i < NS; ++i)
          kept[i] = v[i];
      }
      while (!done) { // the next trial state: a trip that meets a singular matrix raises the damping and evaluates nothing
        if (trips >= a.max_iters) {
          status = LK_ZN_MAX_ITERS;
          done = true;
          break;
        }
        ++trips;
        double delta[P];
        LkZnCriterion again;
        if (step(kept, lambda, delta, &again) != 0) { // LK_ZN_SINGULAR: the kept sums passed the criterion
          lambda = 10.0 * lambda;
          if (lambda >= 1e9) {
            status = LK_ZN_STALLED;
            done = true;
          }
          continue;
        }
        wstep = 0.0;
#pragma unroll
        for (int i = 0; i < P; ++i) {
          p_try[i] = (float)((double)p_cur[i] + delta[i]);
          const double w = lk_znssd_weight(i, P, n) * fabs(delta[i]);
          wstep = w > wstep ? w : wstep;
        }
        break;
      }
      go = !done;
    }
    if constexpr (GROUP > 64) {
      if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i)
          s_try[i] = p_try[i];
        s_try[6] = go ? 1.f : 0.f;
      }
      __syncthreads(); // (the barrier of the next reduction separates these reads from lane 0's next write)
#pragma unroll
      for (int i = 0; i < 6; ++i)
        p_try[i] = s_try[i];
      go = s_try[6] != 0.f;
    } else {
#pragma unroll
      for (int i = 0; i < P; ++i)
        p_try[i] = zn_from_lane0<GROUP>(p_try[i]);
      go = zn_from_lane0<GROUP>(go ? 1.f : 0.f) != 0.f;
    }
  }
  if (lane != 0)
    return;
  const bool evaluated = status != LK_ZN_BAD_SEED && status != LK_ZN_OUT_OF_IMAGE;
  float back[6];
#pragma unroll
  for (int i = 0; i < 6; ++i)
    back[i] = p_cur[i];
  translate<P>(back, level, 0);
  struct lk_znssd o;
  o.n_points = n;
  o.status = status;
  o.iterations = trips;
  o.evaluations = evals;
  o.zncc = (float)best.zncc;
  o.gain = (float)best.gain;
  o.offset = (float)best.offset;
  o.znssd = (float)best.crit;
  o.zncc_seed = zncc_seed;
  o.shift = 0.f;
  if (evaluated) {
    const double du = (double)back[0] - (double)seed[0], dv = P > 1 ? (double)back[1] - (double)seed[1] : 0.0;
    const double uu = du * du, vv = dv * dv;
    o.shift = (float)sqrt(uu + vv);
  }
  o.lambda = good ? (float)lambda : 0.f;
  o.last_step = (float)last_step;
  o.reserved[0] = o.reserved[1] = o.reserved[2] = o.reserved[3] = 0;
  if constexpr (WEIGHTED)
    weight.store(s, o, ws, level);
  else
    a.out[s] = o;
  lk_result r;
  if (!good && !a.guess) {
    r = rec; // a bad seed record passes through
  } else {
#pragma unroll
    for (int i = 0; i < 6; ++i)
      r.resultingParameters[i] = good ? (i < P ? back[i] : 0.f) : seed[i];
    r.chi = 0.f;
    if constexpr (WEIGHTED) {
      if (evaluated && evals > 0) { // sum w (f - g)^2 / sum w (a sector the prologue refused has no sums)
        const double two = 2.0 * kept[4], ssd = (kept[2] - two) + kept[3];
        r.chi = (float)((ssd > 0.0 ? ssd : 0.0) / ws.sw);
      }
    } else if (evaluated) { // sum (f - g)^2 / n from the kept sums: the forward evaluation's chi up to its float rounding
      const double two = 2.0 * kept[4], ssd = (kept[2] - two) + kept[3];
      r.chi = (float)((ssd > 0.0 ? ssd : 0.0) / (double)n);
    }
    r.numberOfPoints = a.count0[s];
    r.iterations = trips;
    r.errorCode = zn_error_code(status);
    const float2 c0 = a.ev.center[s];
    r.undCenterX = c0.x;
    r.undCenterY = c0.y;
  }
  a.rec_out[s] = r;
  if (a.sums) {
#pragma unroll
    for (int i = 0; i < kLkZnSums; ++i)
      a.sums[(size_t)s * kLkZnSums + i] = i < NS ? kept[i] : 0.0;
  }
}

} // namespace
