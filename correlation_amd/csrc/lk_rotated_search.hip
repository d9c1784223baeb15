// lk_rotated_search.hip - the rotation-aware automatic initial guess: lk_guess_search.hip's integer-pixel ZNCC search run at
// every angle of a table (include/lk_engine.h, lk_search_rotated, has the semantics).
//
// lk_rotated_search_kernel: one workgroup of 256 lanes per (sector, angle).  The template is the plain search's; its
// sample (x, y) reads the deformed pixel at the sample's position rotated about the sector's level-L centre by the
// table's {c, s} - float32 products and sums, each rounded on its own, nearest neighbour - so the bounding box, the shift
// rectangle and the offsets of the staged template are the rotated ones and everything else is the shared candidate loop
// of lk_search_common.hpp.  Each workgroup leaves one 32-byte record for its angle.
// lk_rotated_reduce_kernel: one group of 64 lanes per sector picks the winner across the angles under the tie rule, forms
// the runner-up across angles, the parabola through the winner's neighbours and the count over all angles, and writes the
// guess, the sequence history, the match and the per-angle profile.
// Every sum is an integer and no float step is contracted: a sector's match does not depend on what else is in the launch.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "lk_device.hpp"
#include "lk_launch.hpp"
#include "lk_search_common.hpp"

static_assert(sizeof(lk_rotated_match) == 64 && offsetof(lk_rotated_match, score) == 32 &&
                  offsetof(lk_rotated_match, angle_runner_up) == 48 && offsetof(lk_rotated_match, angle) == 56,
              "lk_rotated_match layout");
static_assert(sizeof(LkRotAngleRecord) == 32, "LkRotAngleRecord layout");

namespace {

// (int)floorf(t) with out-of-range and NaN going to INT_MIN: such a sample leaves no valid shift
__device__ __forceinline__ int rs_floor(float t) {
  const float f = floorf(t);
  return fabsf(f) < 2147483648.f ? (int)f : (int)0x80000000;
}

// The position template sample (x, y) reads before the shift, rotated about (Cx, Cy): every step rounded to float32
struct RsRotate {
  float Cx, Cy, c, s;
  __device__ __forceinline__ void operator()(int x, int y, int &X, int &Y) const {
    const float dx = __fsub_rn((float)x, Cx), dy = __fsub_rn((float)y, Cy);
    const float rx = __fsub_rn(__fmul_rn(c, dx), __fmul_rn(s, dy));
    const float ry = __fadd_rn(__fmul_rn(s, dx), __fmul_rn(c, dy));
    X = rs_floor(__fadd_rn(__fadd_rn(Cx, rx), 0.5f));
    Y = rs_floor(__fadd_rn(__fadd_rn(Cy, ry), 0.5f));
  }
};

// angle a before angle b: higher score, then smaller |k|, then smaller k
__device__ __forceinline__ bool rs_better(double sa, int ka, double sb, int kb) {
  if (sa != sb)
    return sa > sb;
  if (abs(ka) != abs(kb))
    return abs(ka) < abs(kb);
  return ka < kb;
}

__device__ __forceinline__ long long rs_clamp(long long v, long long lo, long long hi) { return v < lo ? lo : v > hi ? hi : v; }

} // namespace

__global__ __launch_bounds__(kLkGsThreads) void lk_rotated_search_kernel(LkRotatedSearchArgs ra) {
  extern __shared__ __align__(16) unsigned char gs_lds[];
  __shared__ long long r64a[kLkGsThreads], r64b[kLkGsThreads];
  __shared__ int r32a[kLkGsThreads], r32b[kLkGsThreads];
  const LkGuessSearchArgs &a = ra.gs;
  const int s = (int)blockIdx.x, ka = (int)blockIdx.y, tid = (int)threadIdx.x;
  const int R = a.radius;
  GsSector sec;
  sec.init(a.rect, a.off, a.xy, s, a.ucols, a.urows);
  const int n = sec.n;
  int cx, cy;
  const bool centre_ok = gs_centre(a.guess + (size_t)s * 6, a.level, true, cx, cy);
  const float inv = 1.f / (float)(1 << a.level);
  const float2 c0 = ra.center[s], cs = ra.cos_sin[ka];
  const RsRotate rot{__fmul_rn(c0.x, inv), __fmul_rn(c0.y, inv), cs.x, cs.y};
  // every branch below depends on block-wide values only: all lanes reach every barrier
  int status = -1;
  if (n > LK_GS_MAX_SAMPLES)
    status = LK_GS_TOO_LARGE;
  else if (n < a.min_samples)
    status = LK_GS_TOO_FEW;
  long long St = 0, Stt = 0, varT = 0;
  int minx = 0x7fffffff, miny = 0x7fffffff, maxx = -0x7fffffff, maxy = -0x7fffffff;
  if (status < 0) {
    for (int k = tid; k < n; k += kLkGsThreads) {
      int x, y, X, Y;
      sec.sample(k, x, y);
      const long long t = a.und[(size_t)y * (size_t)a.ucols + (size_t)x];
      St += t;
      Stt += t * t;
      rot(x, y, X, Y);
      minx = min(minx, X);
      miny = min(miny, Y);
      maxx = max(maxx, max(X, -0x7fffffff)); // (so that the negation below stays in range)
      maxy = max(maxy, max(Y, -0x7fffffff));
    }
    gs_block_sum2(r64a, r64b, tid, St, Stt);
    gs_block_min2(r32a, r32b, tid, minx, miny);
    maxx = -maxx;
    maxy = -maxy;
    gs_block_min2(r32a, r32b, tid, maxx, maxy);
    maxx = -maxx;
    maxy = -maxy;
    varT = (long long)n * Stt - St * St;
    if (varT == 0)
      status = LK_GS_TEXTURELESS;
  }
  // candidates whose every rotated, shifted sample is inside the deformed image: a rectangle of shifts (in 64 bits: a
  // rotated position may be anywhere)
  int ilo = 0, ihi = -1, jlo = 0, jhi = -1;
  if (status < 0) {
    ilo = (int)rs_clamp(-(long long)cx - (long long)minx, -R, (long long)R + 1);
    ihi = (int)rs_clamp((long long)a.dcols - 1 - (long long)cx - (long long)maxx, -(long long)R - 1, R);
    jlo = (int)rs_clamp(-(long long)cy - (long long)miny, -R, (long long)R + 1);
    jhi = (int)rs_clamp((long long)a.drows - 1 - (long long)cy - (long long)maxy, -(long long)R - 1, R);
    if (!centre_ok || ilo > ihi || jlo > jhi)
      status = LK_GS_NO_CANDIDATE;
  }
  int win_i = 0, win_j = 0, n_valid = 0;
  double best = kGsNone, runner = kGsNone;
  if (status < 0) {
    n_valid = gs_search_candidates(a, gs_lds, r64a, r64b, r32a, r32b, tid, sec, rot, cx, cy, minx, miny, maxx, maxy, ilo, ihi,
                                   jlo, jhi, St, varT, best, runner, win_i, win_j);
    status = n_valid == 0 ? LK_GS_NO_CANDIDATE : LK_GS_OK;
  }
  if (tid != 0)
    return;
  LkRotAngleRecord &r = ra.angle[(size_t)s * (size_t)ra.n_angles + (size_t)ka];
  r.best = best;
  r.runner_up = runner;
  r.shift_x = win_i;
  r.shift_y = win_j;
  r.n_valid = n_valid;
  r.status = status;
}

__global__ __launch_bounds__(kLkRsReduceThreads) void lk_rotated_reduce_kernel(LkRotatedSearchArgs ra) {
  __shared__ double sc_[kLkRsReduceThreads];
  __shared__ int k_[kLkRsReduceThreads], nv_[kLkRsReduceThreads];
  const LkGuessSearchArgs &a = ra.gs;
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int nA = ra.n_angles, K = (nA - 1) / 2;
  const LkRotAngleRecord *rec = ra.angle + (size_t)s * (size_t)nA;
  double *prof = ra.profile + (size_t)s * (size_t)nA;
  // winner across the angles (+ the count of scored candidates over all of them, the profile)
  double my_best = kGsInvalid;
  int my_k = 1 << 20, my_valid = 0;
  for (int q = tid; q < nA; q += kLkRsReduceThreads) {
    const LkRotAngleRecord r = rec[q];
    const bool has = r.n_valid > 0;
    prof[q] = has ? r.best : kGsNone;
    my_valid += r.n_valid;
    if (has && rs_better(r.best, q - K, my_best, my_k)) {
      my_best = r.best;
      my_k = q - K;
    }
  }
  sc_[tid] = my_best;
  k_[tid] = my_k;
  nv_[tid] = my_valid;
  __syncthreads();
  for (int st = kLkRsReduceThreads / 2; st > 0; st >>= 1) {
    if (tid < st) {
      if (rs_better(sc_[tid + st], k_[tid + st], sc_[tid], k_[tid])) {
        sc_[tid] = sc_[tid + st];
        k_[tid] = k_[tid + st];
      }
      nv_[tid] += nv_[tid + st];
    }
    __syncthreads();
  }
  const int n_valid = nv_[0];
  const int k_win = n_valid > 0 ? k_[0] : 0;
  __syncthreads();
  // runner-up across the angles: the best per-angle score at |k - k_win| >= 2
  double my_ru = kGsNone;
  if (n_valid > 0)
    for (int q = tid; q < nA; q += kLkRsReduceThreads) {
      const LkRotAngleRecord r = rec[q];
      if (r.n_valid > 0 && abs(q - K - k_win) >= 2)
        my_ru = fmax(my_ru, r.best);
    }
  sc_[tid] = my_ru;
  __syncthreads();
  for (int st = kLkRsReduceThreads / 2; st > 0; st >>= 1) {
    if (tid < st)
      sc_[tid] = fmax(sc_[tid], sc_[tid + st]);
    __syncthreads();
  }
  if (tid != 0)
    return;
  const double angle_ru = sc_[0];
  const LkRotAngleRecord first = rec[0]; // TOO_LARGE, TOO_FEW and TEXTURELESS are the sector's: the same at every angle
  int status = first.status;
  if (status != LK_GS_TOO_LARGE && status != LK_GS_TOO_FEW && status != LK_GS_TEXTURELESS)
    status = n_valid == 0 ? LK_GS_NO_CANDIDATE : LK_GS_OK;
  LkRotAngleRecord w{};
  w.best = kGsNone;
  w.runner_up = kGsNone;
  double t = 0.0;
  if (status == LK_GS_OK) {
    w = rec[k_win + K];
    if (!(w.best > (double)a.min_score))
      status = LK_GS_WEAK;
    if (k_win > -K && k_win < K && rec[k_win + K - 1].n_valid > 0 && rec[k_win + K + 1].n_valid > 0) {
      const double sm = rec[k_win + K - 1].best, sp = rec[k_win + K + 1].best;
      const double den = sm - 2.0 * w.best + sp;
      if (den < 0.0)
        t = fmin(fmax(0.5 * (sm - sp) / den, -0.5), 0.5);
    }
  }
  const double theta = ra.angle_center + (double)k_win * ra.angle_step;
  float *g = a.guess + (size_t)s * 6;
  int cx, cy;
  (void)gs_centre(g, a.level, true, cx, cy);
  if (status == LK_GS_OK) {
    const double scale = (double)(1 << a.level);
    const float2 cs = ra.cos_sin[k_win + K];
    g[0] = (float)((double)(cx + w.shift_x) * scale);
    g[1] = (float)((double)(cy + w.shift_y) * scale);
    if (ra.model == LK_FM_UVUXUYVXVY) {
      g[2] = __fsub_rn(cs.x, 1.f);
      g[3] = __fsub_rn(0.f, cs.y);
      g[4] = cs.y;
      g[5] = __fsub_rn(cs.x, 1.f);
    } else { // LK_FM_UVQ: the linearised warp's best q
      g[2] = cs.y;
    }
  }
  float *pp = a.prev_p + (size_t)s * 6;
  for (int k = 0; k < 6; ++k)
    pp[k] = g[k];
  const int4 rc = a.rect[s];
  lk_rotated_match &m = ra.match[s];
  m.center_x = cx;
  m.center_y = cy;
  m.shift_x = w.shift_x;
  m.shift_y = w.shift_y;
  m.n_samples = rc.z > 0 ? rc.w : (int)(a.off[s + 1] - a.off[s]);
  m.n_valid = n_valid;
  m.status = status;
  m.angle_index = k_win;
  m.score = w.best;
  m.runner_up = w.runner_up;
  m.angle_runner_up = angle_ru;
  m.angle = (float)theta;
  m.angle_refined = (float)(theta + t * ra.angle_step);
}

hipError_t lk_launch_rotated_search(const LkRotatedSearchArgs &ra, hipStream_t st) {
  if (ra.gs.n_sectors <= 0)
    return hipSuccess;
  const int ncand = (2 * ra.gs.radius + 1) * (2 * ra.gs.radius + 1);
  const size_t lds = (size_t)ncand * sizeof(double) + (size_t)kLkGsChunk * 5 + (size_t)ra.gs.win_bytes;
  hipLaunchKernelGGL(lk_rotated_search_kernel, dim3((unsigned)ra.gs.n_sectors, (unsigned)ra.n_angles), dim3(kLkGsThreads), lds, st,
                     ra);
  return hipGetLastError();
}

hipError_t lk_launch_rotated_reduce(const LkRotatedSearchArgs &ra, hipStream_t st) {
  if (ra.gs.n_sectors <= 0)
    return hipSuccess;
  hipLaunchKernelGGL(lk_rotated_reduce_kernel, dim3((unsigned)ra.gs.n_sectors), dim3(kLkRsReduceThreads), 0, st, ra);
  return hipGetLastError();
}
