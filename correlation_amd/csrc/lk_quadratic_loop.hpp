// lk_quadratic_loop.hpp - the loop of the second-order refinement, one body for the passes that differ in how the deformed
// image is sampled or in how its samples are weighted: lk_quadratic.hip (the engine's interpolator, unit weights,
// lk_refine_quadratic) and lk_composed.hip (any sampler under a Gaussian window and a pixel mask,
// lk_refine_composed with order 2; section 27).  Device only.  The move lk_znssd_loop.hpp made for the first-order passes,
// with the same two policies.
//
// lk_znssd_loop.hpp with twelve parameters: one lane group (a 16-lane DPP row, a wavefront or a 512-thread workgroup, from
// the sector's level-0 sample count alone) refines one sector from its seed to the end; lane 0 owns the Levenberg-Marquardt
// loop.  Two things differ.
//
// The sums.  88 doubles per evaluation (lk_quadratic.hpp), and 87 live double accumulators do not fit into a lane's
// registers: lk_znssd_kernel is at 256 VGPRs with 45.  An evaluation is therefore three sweeps over the samples of 30, 27
// and 30 sums.  Every sweep computes a sample's floats - warp, node, sampler, weight - by the same instructions in the same
// order, so which sweep holds a sum does not change a bit of it; each sweep ends in the fixed-order reduction.
//
// The step.  lk_quadratic_step works in LDS: lane 0 keeps the sums of the best state (88), the sums of the trial state (88)
// and the factorisation's workspace there, and swaps the two rows of sums when a trial state is accepted.  Flag and trial
// parameters go to the other lanes as in lk_znssd_loop.hpp, so the loop's barriers are reached by all threads of a workgroup.
//
// No model template: the engine's model only says how a seed is read and how the record is written (a.model).
#pragma once
#include "lk_device.hpp"
#include "lk_neighbours.hpp"
#include "lk_quadratic.hpp"
#include "lk_sector_eval.hpp"
#include "lk_znssd_loop.hpp" // the weight policy's contract: LkZnUnitWeight, LkZnWeightSums

namespace {

constexpr int kQdStride = 32;   // doubles per wavefront in the cross-wavefront reduction of one sweep (30 used at most)
constexpr int kQdSweepA = 30, kQdSweepB = 27, kQdSweepC = 30;
constexpr int P12 = kLkQdParams;

template <int GROUP> __device__ __forceinline__ float qd_from_lane0(float v) {
  if constexpr (GROUP == 16)
    return dpp_bcast<0>(v);
  else
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
}

// the shared good rule (reseed_good, lk_neighbours.hpp) for a model known at run time, unrolled as lk_znssd_loop.hpp's
__device__ __forceinline__ bool qd_good(const lk_result &r, int P, float chi_max) {
  bool good = r.errorCode == LK_ERROR_NONE && finite_bits(r.chi);
#pragma unroll
  for (int i = 0; i < 6; ++i)
    good = good && (i >= P || finite_bits(r.resultingParameters[i]));
  return good && (!(chi_max > 0.f) || r.chi <= chi_max);
}

__device__ __forceinline__ int qd_error_code(int status) {
  switch (status) {
  case LK_ZN_CONVERGED: return LK_ERROR_NONE;
  case LK_ZN_MAX_ITERS:
  case LK_ZN_STALLED: return LK_ERROR_CORRELATION_MAX_ITERS_REACHED;
  case LK_ZN_OUT_OF_IMAGE: return LK_ERROR_INTERPOLATION_OUT_OF_IMAGE;
  case LK_ZN_BAD_SEED: return LK_ERROR_BAD_DOMAIN; // (a seed that is not finite; a bad record is copied instead)
  default: return LK_ERROR_SOLVER;
  }
}

// the seed's translation between levels: u, v as translate<>, the gradients unchanged, the second-order terms the other way
__device__ __forceinline__ void qd_translate(float (&p)[P12], int src, int dst) {
  const float down = (dst - src > 0) ? 1.f / (float)(1 << (dst - src)) : (float)(1 << (src - dst));
  const float up = (dst - src > 0) ? (float)(1 << (dst - src)) : 1.f / (float)(1 << (src - dst));
  p[0] *= down;
  p[1] *= down;
#pragma unroll
  for (int i = 6; i < P12; ++i)
    p[i] *= up;
}

// One sample's weight, the same in every sweep: false for a sample that is not part of the sector (w == 0; unit weights: never)
template <class WEIGHT> __device__ __forceinline__ bool qd_weight(const SectorLevel &c, f32x2 q, const WEIGHT &weight, double &wd) {
  if constexpr (WEIGHT::kWeighted) {
    const float w = weight.of(c, q);
    if (!(w > 0.f))
      return false;
    wd = (double)w;
  }
  return true;
}

// One sample's floats, the same in every sweep: false when the sampler flags the position.
template <class SAMPLER>
__device__ __forceinline__ bool qd_sample(const SectorLevel &c, f32x2 q, const float (&p)[P12], const SAMPLER &sample, float &f, float &g,
                                          float &gx, float &gy, float &dx, float &dy) {
  dx = q.x - c.cx;
  dy = q.y - c.cy;
  const float hxx = 0.5f * (dx * dx), hxy = dx * dy, hyy = 0.5f * (dy * dy);
  const float xd = (((((q.x + p[0]) + p[2] * dx) + p[3] * dy) + p[6] * hxx) + p[7] * hxy) + p[8] * hyy;
  const float yd = (((((q.y + p[1]) + p[4] * dx) + p[5] * dy) + p[9] * hxx) + p[10] * hxy) + p[11] * hyy;
  f = sector_und_node(c, q);
  return sample(c, xd, yd, g, gx, gy);
}

// term, or with weights term times w (a rounded product), added to acc
template <bool WEIGHTED> __device__ __forceinline__ void qd_add(double &acc, double term, [[maybe_unused]] double wd) {
  if constexpr (WEIGHTED)
    acc += term * wd;
  else
    acc += term;
}

// the 15 monomials of (X, Y) in double, each a single rounded product Xa Yb
__device__ __forceinline__ void qd_monomials(float dx, float dy, double (&M)[kLkQdMono]) {
  const double X = (double)dx, Y = (double)dy;
  const double X2 = X * X, X3 = X2 * X, X4 = X2 * X2, Y2 = Y * Y, Y3 = Y2 * Y, Y4 = Y2 * Y2;
  const double Xa[5] = {1.0, X, X2, X3, X4}, Yb[5] = {1.0, Y, Y2, Y3, Y4};
  int k = 0;
#pragma unroll
  for (int d = 0; d <= 4; ++d)
#pragma unroll
    for (int b = 0; b <= d; ++b)
      M[k++] = Xa[d - b] * Yb[b];
}

// the three sweeps; v in the order of the sums each holds (see the sector body for where they go)
template <int GROUP, class SAMPLER, class WEIGHT>
__device__ __forceinline__ void qd_sweep_a(const SectorLevel &c, int lane, const float (&p)[P12], const SAMPLER &sample, const WEIGHT &weight,
                                           double (&v)[kQdSweepA]) {
  constexpr bool WT = WEIGHT::kWeighted;
#pragma unroll
  for (int i = 0; i < kQdSweepA; ++i)
    v[i] = 0.0;
  for (int k = lane; k < c.n; k += GROUP) {
    const f32x2 q = sector_sample(c, k);
    [[maybe_unused]] double wd = 1.0;
    if (!qd_weight(c, q, weight, wd))
      continue; // not part of the sector: never sampled, never flagged
    float f, g, gx, gy, dx, dy;
    if (!qd_sample(c, q, p, sample, f, g, gx, gy, dx, dy)) {
      v[29] += 1.0;
      continue; // the sums of an evaluation that hit the error are never used
    }
    const double fd = (double)f, gd = (double)g, gxd = (double)gx, gyd = (double)gy;
    const double X = (double)dx, Y = (double)dy;
    const double M[kLkQdLow] = {1.0, X, Y, X * X, X * Y, Y * Y};
    qd_add<WT>(v[0], fd, wd);
    qd_add<WT>(v[1], gd, wd);
    qd_add<WT>(v[2], fd * fd, wd); // (no contraction: a rounded product, then a rounded sum)
    qd_add<WT>(v[3], gd * gd, wd);
    qd_add<WT>(v[4], fd * gd, wd);
#pragma unroll
    for (int i = 0; i < kLkQdLow; ++i) {
      const double tx = gxd * M[i], ty = gyd * M[i];
      qd_add<WT>(v[5 + i], tx, wd);
      qd_add<WT>(v[5 + kLkQdLow + i], ty, wd);
      qd_add<WT>(v[17 + i], tx * fd, wd);
      qd_add<WT>(v[17 + kLkQdLow + i], ty * fd, wd);
    }
  }
}

template <int GROUP, class SAMPLER, class WEIGHT>
__device__ __forceinline__ void qd_sweep_b(const SectorLevel &c, int lane, const float (&p)[P12], const SAMPLER &sample, const WEIGHT &weight,
                                           double (&v)[kQdSweepB]) {
  constexpr bool WT = WEIGHT::kWeighted;
#pragma unroll
  for (int i = 0; i < kQdSweepB; ++i)
    v[i] = 0.0;
  for (int k = lane; k < c.n; k += GROUP) {
    const f32x2 q = sector_sample(c, k);
    [[maybe_unused]] double wd = 1.0;
    if (!qd_weight(c, q, weight, wd))
      continue;
    float f, g, gx, gy, dx, dy;
    if (!qd_sample(c, q, p, sample, f, g, gx, gy, dx, dy))
      continue;
    const double gd = (double)g, gxd = (double)gx, gyd = (double)gy;
    double M[kLkQdMono];
    qd_monomials(dx, dy, M);
    const double w = gxd * gxd;
#pragma unroll
    for (int i = 0; i < kLkQdMono; ++i)
      qd_add<WT>(v[i], w * M[i], wd);
#pragma unroll
    for (int i = 0; i < kLkQdLow; ++i) {
      const double tx = gxd * M[i], ty = gyd * M[i];
      qd_add<WT>(v[kLkQdMono + i], tx * gd, wd);
      qd_add<WT>(v[kLkQdMono + kLkQdLow + i], ty * gd, wd);
    }
  }
}

template <int GROUP, class SAMPLER, class WEIGHT>
__device__ __forceinline__ void qd_sweep_c(const SectorLevel &c, int lane, const float (&p)[P12], const SAMPLER &sample, const WEIGHT &weight,
                                           double (&v)[kQdSweepC]) {
  constexpr bool WT = WEIGHT::kWeighted;
#pragma unroll
  for (int i = 0; i < kQdSweepC; ++i)
    v[i] = 0.0;
  for (int k = lane; k < c.n; k += GROUP) {
    const f32x2 q = sector_sample(c, k);
    [[maybe_unused]] double wd = 1.0;
    if (!qd_weight(c, q, weight, wd))
      continue;
    float f, g, gx, gy, dx, dy;
    if (!qd_sample(c, q, p, sample, f, g, gx, gy, dx, dy))
      continue;
    const double gxd = (double)gx, gyd = (double)gy;
    double M[kLkQdMono];
    qd_monomials(dx, dy, M);
    const double wxy = gxd * gyd, wyy = gyd * gyd;
#pragma unroll
    for (int i = 0; i < kLkQdMono; ++i) {
      qd_add<WT>(v[i], wxy * M[i], wd);
      qd_add<WT>(v[kLkQdMono + i], wyy * M[i], wd);
    }
  }
}

// The body of a kernel of THREADS = 256 (GROUP <= 64) or GROUP threads.  sample and weight: the policies of
// lk_znssd_loop.hpp; with weights the info goes to weight.store(s, o, sums of the weights, level) in place of a.out[s], a
// sample of weight 0 is skipped in every sweep before anything of it is read, every other term of the sums is formed as
// without weights and multiplied by (double)w before it is added, and N = sum w stands for (double)n.
template <int GROUP, class SAMPLER, class WEIGHT>
__device__ __forceinline__ void lk_quadratic_sector(const LkQuadraticArgs &a, const SAMPLER &sample, const WEIGHT &weight) {
  constexpr int THREADS = GROUP <= 64 ? 256 : GROUP;
  constexpr int SLOTS = THREADS / GROUP;
  constexpr bool WEIGHTED = WEIGHT::kWeighted;
  using Y = LkQdLayout;
  // one reduction area per sweep: a wavefront that is already in the next sweep writes where no slow reader still reads
  __shared__ double lds[3][(GROUP > 64 ? GROUP / kWave : 1) * kQdStride];
  __shared__ double s_sums[SLOTS][2][kLkQdSums]; // the sums of the best and of the trial state; lane 0 of the group alone
  __shared__ double s_work[SLOTS][kLkQdWork + P12]; // touches its rows; the step's workspace, then its delta: lk_quadratic_step
                                                   // indexes both in loops, which registers do not allow
  __shared__ float s_try[16];                    // GROUP == 512: the trial parameters and the flag
  const int slot = (int)threadIdx.x / GROUP;
  const int gid = (int)blockIdx.x * SLOTS + slot;
  const int lane = (int)threadIdx.x % GROUP;
  if (gid >= a.n_sectors) // (GROUP == 512: the whole workgroup; GROUP <= 64: whole rows / wavefronts, no barriers below)
    return;
  const int s = (int)a.ev.order[gid], level = a.level, model = a.model;
  const int P = n_params(model);
  lk_result rec{};
  float first[6]; // the first-order seed as it came: level-0 scale, the engine model's meaning
  bool good, bad_record = false;
  if (a.guess) {
    good = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      first[i] = i < P ? a.guess[(size_t)s * 6 + i] : 0.f;
      good = good && finite_bits(first[i]);
    }
  } else {
    rec = a.ev.rec[s];
    good = qd_good(rec, P, a.chi_max);
    bad_record = !good;
#pragma unroll
    for (int i = 0; i < 6; ++i)
      first[i] = i < P ? rec.resultingParameters[i] : 0.f;
  }
  float seed[P12]; // level-0 scale
#pragma unroll
  for (int i = 0; i < P12; ++i)
    seed[i] = 0.f;
  seed[0] = first[0];
  seed[1] = first[1];
  if (model == LK_FM_UVQ) { // Warp<LK_FM_UVQ>::apply: xd = x + u - q dy, yd = y + v + q dx
    seed[3] = -first[2];
    seed[4] = first[2];
  } else {
#pragma unroll
    for (int i = 2; i < 6; ++i)
      seed[i] = first[i];
  }
  if (a.second) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      seed[6 + i] = a.second[(size_t)s * 6 + i];
      good = good && finite_bits(seed[6 + i]);
    }
  }
  const SectorLevel c = sector_level(a.ev, s, level, a.ev.center[s]);
  const int n = c.n;
  float p_cur[P12], p_try[P12];
#pragma unroll
  for (int i = 0; i < P12; ++i)
    p_cur[i] = seed[i];
  qd_translate(p_cur, 0, level);
#pragma unroll
  for (int i = 0; i < P12; ++i)
    p_try[i] = p_cur[i];
  double *kept = s_sums[slot][0], *trial = s_sums[slot][1], *work = s_work[slot];
  if (lane == 0) {
    for (int i = 0; i < kLkQdSums; ++i)
      kept[i] = trial[i] = 0.0;
  }
  // the loop's state: lane 0's is the group's
  int status = LK_ZN_BAD_SEED, evals = 0, trips = 0;
  double lambda = (double)a.lambda0, crit = 0.0, last_step = 0.0, wstep = 0.0;
  LkZnCriterion best;
  best.crit = best.gain = best.offset = best.zncc = 0.0;
  float zncc_seed = 0.f;
  bool go = good;
  // with weights, the prologue of lk_znssd_loop.hpp: one pass over the samples' weights alone, one reduction in the fixed order
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
      reduce_f64<GROUP, 5, 0, kQdStride>(t, lds[0]);
      if constexpr (GROUP > 64)
        __syncthreads(); // (the first sweep's reduction writes the slots these sums were read from)
      ws.n_valid = (int)t[0];
      ws.sw = t[1];
      ws.sww = t[2];
      ws.swx = t[3];
      ws.swy = t[4];
      if (ws.n_valid < P12 + 2 || weight.too_few(ws.n_valid, n)) { // nothing of the images is read
        status = LK_ZN_TOO_FEW;
        go = false;
      }
    }
  }
  while (go) {
    {
      double v[kQdSweepA];
      qd_sweep_a<GROUP>(c, lane, p_try, sample, weight, v);
      reduce_f64<GROUP, kQdSweepA, 0, kQdStride>(v, lds[0]);
      if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 5; ++i)
          trial[i] = v[i];
#pragma unroll
        for (int i = 0; i < 2 * kLkQdLow; ++i) {
          trial[Y::T + i] = v[5 + i];
          trial[Y::TF + i] = v[17 + i];
        }
        trial[Y::FLAGGED] = v[29];
      }
    }
    {
      double v[kQdSweepB];
      qd_sweep_b<GROUP>(c, lane, p_try, sample, weight, v);
      reduce_f64<GROUP, kQdSweepB, 0, kQdStride>(v, lds[1]);
      if (lane == 0) {
#pragma unroll
        for (int i = 0; i < kLkQdMono; ++i)
          trial[Y::W + i] = v[i];
#pragma unroll
        for (int i = 0; i < 2 * kLkQdLow; ++i)
          trial[Y::TG + i] = v[kLkQdMono + i];
      }
    }
    {
      double v[kQdSweepC];
      qd_sweep_c<GROUP>(c, lane, p_try, sample, weight, v);
      reduce_f64<GROUP, kQdSweepC, 0, kQdStride>(v, lds[2]);
      if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 2 * kLkQdMono; ++i)
          trial[Y::W + kLkQdMono + i] = v[i];
      }
    }
    ++evals;
    if (lane == 0) {
      LkZnCriterion cr;
      cr.crit = cr.gain = cr.offset = cr.zncc = 0.0;
      const bool flagged = trial[Y::FLAGGED] != 0.0;
      int refused; // the criterion of n samples of weight 1, or of the n_valid samples of total weight sum w
      if constexpr (WEIGHTED)
        refused = flagged ? (int)LK_ZN_OUT_OF_IMAGE : lk_znssd_criterion<P12>(ws.n_valid, ws.sw, trial, &cr);
      else
        refused = flagged ? (int)LK_ZN_OUT_OF_IMAGE : lk_znssd_criterion<P12>(n, trial, &cr);
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
        for (int i = 0; i < P12; ++i)
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
        double *t = kept; // the trial state's sums are the kept ones now; the next evaluation overwrites the others
        kept = trial;
        trial = t;
      }
      while (!done) { // the next trial state: a trip that meets a singular matrix raises the damping and evaluates nothing
        if (trips >= a.max_iters) {
          status = LK_ZN_MAX_ITERS;
          done = true;
          break;
        }
        ++trips;
        double *delta = work + kLkQdWork;
        LkZnCriterion again;
        int singular; // LK_ZN_SINGULAR: the kept sums passed the criterion
        if constexpr (WEIGHTED)
          singular = lk_quadratic_step(ws.n_valid, ws.sw, kept, lambda, delta, &again, work);
        else
          singular = lk_quadratic_step(n, kept, lambda, delta, &again, work);
        if (singular != 0) {
          lambda = 10.0 * lambda;
          if (lambda >= 1e9) {
            status = LK_ZN_STALLED;
            done = true;
          }
          continue;
        }
        wstep = 0.0;
#pragma unroll
        for (int i = 0; i < P12; ++i) {
          p_try[i] = (float)((double)p_cur[i] + delta[i]);
          const double w = lk_quadratic_weight(i, n) * fabs(delta[i]);
          wstep = w > wstep ? w : wstep;
        }
        break;
      }
      go = !done;
    }
    if constexpr (GROUP > 64) {
      if (lane == 0) {
#pragma unroll
        for (int i = 0; i < P12; ++i)
          s_try[i] = p_try[i];
        s_try[P12] = go ? 1.f : 0.f;
      }
      __syncthreads(); // (the barriers of the next evaluation separate these reads from lane 0's next write)
#pragma unroll
      for (int i = 0; i < P12; ++i)
        p_try[i] = s_try[i];
      go = s_try[P12] != 0.f;
    } else {
#pragma unroll
      for (int i = 0; i < P12; ++i)
        p_try[i] = qd_from_lane0<GROUP>(p_try[i]);
      go = qd_from_lane0<GROUP>(go ? 1.f : 0.f) != 0.f;
    }
  }
  if (lane != 0)
    return;
  const bool evaluated = status != LK_ZN_BAD_SEED && status != LK_ZN_OUT_OF_IMAGE;
  float back[P12];
#pragma unroll
  for (int i = 0; i < P12; ++i)
    back[i] = p_cur[i];
  qd_translate(back, level, 0);
  const int n0 = a.count0[s];
  struct lk_quadratic o;
  o.n_points = n;
  o.status = status;
  o.iterations = trips;
  o.evaluations = evals;
#pragma unroll
  for (int i = 0; i < P12; ++i)
    o.p[i] = evaluated ? back[i] : 0.f;
  o.zncc = (float)best.zncc;
  o.gain = (float)best.gain;
  o.offset = (float)best.offset;
  o.znssd = (float)best.crit;
  o.zncc_seed = zncc_seed;
  o.shift = 0.f;
  o.bend = 0.f;
  if (evaluated) {
    const double du = (double)back[0] - (double)seed[0], dv = (double)back[1] - (double)seed[1];
    const double uu = du * du, vv = dv * dv;
    o.shift = (float)sqrt(uu + vv);
    o.bend = (float)lk_quadratic_bend(back, n0);
  }
  o.lambda = good ? (float)lambda : 0.f;
  o.last_step = (float)last_step;
#pragma unroll
  for (int i = 0; i < 7; ++i)
    o.reserved[i] = 0;
  if constexpr (WEIGHTED)
    weight.store(s, o, ws, level);
  else
    a.out[s] = o;
  lk_result r;
  if (bad_record) {
    r = rec; // a bad seed record passes through
  } else {
    if (!good) { // a guess or a second-order seed that is not finite: the first-order seed as it came
#pragma unroll
      for (int i = 0; i < 6; ++i)
        r.resultingParameters[i] = first[i];
    } else { // the engine model's own layout
#pragma unroll
      for (int i = 0; i < 6; ++i)
        r.resultingParameters[i] = i < P ? back[i] : 0.f;
      if (model == LK_FM_UVQ)
        r.resultingParameters[2] = (back[4] - back[3]) * 0.5f;
    }
    r.chi = 0.f;
    if constexpr (WEIGHTED) {
      if (evaluated && evals > 0) { // sum w (f - g)^2 / sum w (a sector the prologue refused has no sums)
        const double two = 2.0 * kept[4], ssd = (kept[2] - two) + kept[3];
        r.chi = (float)((ssd > 0.0 ? ssd : 0.0) / ws.sw);
      }
    } else if (evaluated) { // sum (f - g)^2 / n from the kept sums, as lk_znssd_loop.hpp
      const double two = 2.0 * kept[4], ssd = (kept[2] - two) + kept[3];
      r.chi = (float)((ssd > 0.0 ? ssd : 0.0) / (double)n);
    }
    r.numberOfPoints = n0;
    r.iterations = trips;
    r.errorCode = qd_error_code(status);
    const float2 c0 = a.ev.center[s];
    r.undCenterX = c0.x;
    r.undCenterY = c0.y;
  }
  a.rec_out[s] = r;
  if (a.sums) {
    for (int i = 0; i < kLkQdSums; ++i)
      a.sums[(size_t)s * kLkQdSums + i] = kept[i];
  }
}

} // namespace
