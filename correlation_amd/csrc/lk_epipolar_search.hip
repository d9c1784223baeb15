// lk_epipolar_search.hip - the stereo initial guess: lk_guess_search.hip's integer-pixel ZNCC search run along the epipolar
// curve of a calibrated rig instead of over a square of shifts (include/lk_engine.h, lk_search_epipolar, has the semantics).
//
// lk_epipolar_search_kernel: one workgroup of 256 lanes per (sector, run).  The curve table is built on the host
// (lk_epipolar_search.cpp), which also cuts every curve into runs of stations whose candidates - the stations of the run
// times the band across the curve - share one template map.  shape 1: the run of stations whose node is the workgroup's, the
// map the node's 2 x 2 matrix about the sector's level-L centre (float32 products and sums, each rounded on its own, nearest
// neighbour, lk_rotated_search.hip's form with a full matrix).  shape 0: the map is the identity at every station, so a run is
// a stretch of the curve of up to 1024 candidates - a short curve is one workgroup's, which is what makes the pass cheaper
// than the square search and not dearer (DESIGN.md section 33 has both measurements).  The template is the plain search's;
// the candidates are a list of displacements, scored by the listed candidate loop of lk_search_common.hpp.  Each workgroup
// leaves one 32-byte record for its run and the best score of each of its stations in the profile.
// lk_epipolar_reduce_kernel: one group of 64 lanes per sector picks the winner across the runs under the tie rule, forms the
// count, the runner-up along the curve and the parabola through the winner's neighbours from the profile, and writes the
// guess, the sequence history and the match.
// Every sum is an integer and no float step is contracted: a sector's match does not depend on what else is in the launch.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "lk_device.hpp"
#include "lk_launch.hpp"
#include "lk_search_common.hpp"

static_assert(sizeof(lk_epipolar_match) == 64 && offsetof(lk_epipolar_match, n_samples) == 20 && offsetof(lk_epipolar_match, score) == 32 &&
                  offsetof(lk_epipolar_match, station_refined) == 48 && offsetof(lk_epipolar_match, reserved) == 56,
              "lk_epipolar_match layout");
static_assert(sizeof(lk_epipolar_curve) == 32 && sizeof(lk_epipolar_search) == 80 && offsetof(lk_epipolar_search, z_near) == 40,
              "lk_epipolar_curve / lk_epipolar_search layout");
static_assert(sizeof(LkEpNodeRecord) == 32, "LkEpNodeRecord layout");
static_assert(LK_EP_MAX_GROUP * 8 + LK_EP_MAX_GROUP * 4 + kLkGsChunk * 5 + kLkGsThreads * 24 < 65536,
              "the scores and stations of the longest run fit the LDS of a workgroup");

namespace {

// (int)floorf(t) with out-of-range and NaN going to INT_MIN: such a sample leaves no valid candidate
__device__ __forceinline__ int ep_floor(float t) {
  const float f = floorf(t);
  return fabsf(f) < 2147483648.f ? (int)f : (int)0x80000000;
}

// The position template sample (x, y) reads before the displacement, mapped by A about (Cx, Cy): every step rounded to float32
struct EpAffine {
  float Cx, Cy, a11, a12, a21, a22;
  __device__ __forceinline__ void operator()(int x, int y, int &X, int &Y) const {
    const float dx = __fsub_rn((float)x, Cx), dy = __fsub_rn((float)y, Cy);
    const float rx = __fadd_rn(__fmul_rn(a11, dx), __fmul_rn(a12, dy));
    const float ry = __fadd_rn(__fmul_rn(a21, dx), __fmul_rn(a22, dy));
    X = ep_floor(__fadd_rn(__fadd_rn(Cx, rx), 0.5f));
    Y = ep_floor(__fadd_rn(__fadd_rn(Cy, ry), 0.5f));
  }
};
struct EpSame {
  __device__ __forceinline__ void operator()(int x, int y, int &X, int &Y) const {
    X = x;
    Y = y;
  }
};

// Candidate q = ml * nb + (b + B) of a run -> its level-L displacement: station t0 + ml along the axis, other[ml] + b across
struct EpDisp {
  const int *other; // [stations of the run] (LDS)
  int t0, nb, B, axis;
  __device__ __forceinline__ void operator()(int q, int &dx, int &dy) const {
    const int ml = q / nb, b = q - ml * nb - B;
    const int along = t0 + ml, across = other[ml] + b;
    dx = axis == 0 ? along : across;
    dy = axis == 0 ? across : along;
  }
};

template <bool kShape> __device__ __forceinline__ void ep_search(const LkEpipolarSearchArgs &ea, unsigned char *gs_lds, long long *r64a,
                                                                  long long *r64b, int *r32a, int *r32b) {
  const LkGuessSearchArgs &a = ea.gs;
  const int s = (int)blockIdx.x, kn = (int)blockIdx.y, tid = (int)threadIdx.x;
  const int B = a.radius, nb = 2 * B + 1;
  const lk_epipolar_curve cv = ea.curve[s];
  const int2 run = ea.run[(size_t)s * (size_t)ea.n_runs + (size_t)kn];
  LkEpNodeRecord &rec = ea.rec[(size_t)s * (size_t)ea.n_runs + (size_t)kn];
  // every branch below depends on block-wide values only: all lanes reach every barrier
  const int nst = run.y;
  if (nst <= 0 || cv.status != 0) { // (a curve with a status has no stations)
    if (tid == 0) {
      rec.best = kGsNone;
      rec.station = rec.band_offset = rec.n_valid = 0;
      rec.status = -1;
      rec.pad[0] = rec.pad[1] = 0;
    }
    return;
  }
  double *score = (double *)gs_lds;
  int *other = (int *)(score + ea.max_cand);
  uint32_t *toff = (uint32_t *)(other + ea.max_run);
  uint8_t *tval = (uint8_t *)(toff + kLkGsChunk);
  uint8_t *win = tval + kLkGsChunk;
  const size_t st0 = (size_t)cv.first_index + (size_t)run.x;
  double *profile = ea.profile + st0;
  for (int q = tid; q < nst; q += kLkGsThreads)
    other[q] = ea.other[st0 + (size_t)q];
  GsSector sec;
  sec.init(a.rect, a.off, a.xy, s, a.ucols, a.urows);
  const int n = sec.n;
  EpAffine map{0.f, 0.f, 1.f, 0.f, 0.f, 1.f};
  if (kShape) {
    const float inv = 1.f / (float)(1 << a.level);
    const float2 c0 = ea.center[s];
    const float4 A = ea.shape[(size_t)s * (size_t)ea.n_nodes + (size_t)kn];
    map = EpAffine{__fmul_rn(c0.x, inv), __fmul_rn(c0.y, inv), A.x, A.y, A.z, A.w};
  }
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
      if (kShape)
        map(x, y, X, Y);
      else
        X = x, Y = y;
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
  int n_valid = 0, win_q = 0;
  double best = kGsNone;
  if (status < 0) {
    const EpDisp disp{other, cv.first_station + run.x, nb, B, cv.axis};
    if (kShape)
      n_valid = gs_search_listed(a, score, toff, tval, win, r64a, r64b, r32a, r32b, tid, sec, map, disp, minx, miny, maxx, maxy, nst, B,
                                 run.x, St, varT, profile, best, win_q);
    else
      n_valid = gs_search_listed(a, score, toff, tval, win, r64a, r64b, r32a, r32b, tid, sec, EpSame{}, disp, minx, miny, maxx, maxy, nst,
                                 B, run.x, St, varT, profile, best, win_q);
    status = n_valid == 0 ? LK_GS_NO_CANDIDATE : LK_GS_OK;
  } else {
    for (int q = tid; q < nst; q += kLkGsThreads)
      profile[q] = kGsNone;
  }
  if (tid != 0)
    return;
  const int ml = win_q / nb;
  rec.best = best;
  rec.station = n_valid > 0 ? run.x + ml : 0;
  rec.band_offset = n_valid > 0 ? win_q - ml * nb - B : 0;
  rec.n_valid = n_valid;
  rec.status = status;
  rec.pad[0] = rec.pad[1] = 0;
}

} // namespace

template <bool kShape> __global__ __launch_bounds__(kLkGsThreads) void lk_epipolar_search_kernel(LkEpipolarSearchArgs ea) {
  extern __shared__ __align__(16) unsigned char gs_lds[];
  __shared__ long long r64a[kLkGsThreads], r64b[kLkGsThreads];
  __shared__ int r32a[kLkGsThreads], r32b[kLkGsThreads];
  ep_search<kShape>(ea, gs_lds, r64a, r64b, r32a, r32b);
}

__global__ __launch_bounds__(kLkRsReduceThreads) void lk_epipolar_reduce_kernel(LkEpipolarSearchArgs ea) {
  __shared__ double sc_[kLkRsReduceThreads];
  __shared__ int m_[kLkRsReduceThreads], b_[kLkRsReduceThreads], nv_[kLkRsReduceThreads], st_[kLkRsReduceThreads];
  const LkGuessSearchArgs &a = ea.gs;
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int N = ea.n_runs;
  const LkEpNodeRecord *rec = ea.rec + (size_t)s * (size_t)N;
  const lk_epipolar_curve cv = ea.curve[s];
  const double *prof = ea.profile + (size_t)cv.first_index;
  // winner across the nodes (+ the count of scored candidates over all of them, the status of the sector's template)
  double my_best = kGsInvalid;
  int my_m = 0x7fffffff, my_b = 30000, my_valid = 0, my_status = 0;
  for (int q = tid; q < N; q += kLkRsReduceThreads) {
    const LkEpNodeRecord r = rec[q];
    my_valid += r.n_valid;
    if (r.status == LK_GS_TOO_LARGE || r.status == LK_GS_TOO_FEW || r.status == LK_GS_TEXTURELESS)
      my_status = r.status; // (the sector's: the same in every run that is not empty)
    if (r.n_valid > 0 && gs_listed_better(r.best, r.station, r.band_offset, my_best, my_m, my_b)) {
      my_best = r.best;
      my_m = r.station;
      my_b = r.band_offset;
    }
  }
  sc_[tid] = my_best;
  m_[tid] = my_m;
  b_[tid] = my_b;
  nv_[tid] = my_valid;
  st_[tid] = my_status;
  __syncthreads();
  for (int st = kLkRsReduceThreads / 2; st > 0; st >>= 1) {
    if (tid < st) {
      if (gs_listed_better(sc_[tid + st], m_[tid + st], b_[tid + st], sc_[tid], m_[tid], b_[tid])) {
        sc_[tid] = sc_[tid + st];
        m_[tid] = m_[tid + st];
        b_[tid] = b_[tid + st];
      }
      nv_[tid] += nv_[tid + st];
      st_[tid] = max(st_[tid], st_[tid + st]);
    }
    __syncthreads();
  }
  const int n_valid = nv_[0];
  const int m_win = n_valid > 0 ? m_[0] : 0, b_win = n_valid > 0 ? b_[0] : 0;
  const double best = n_valid > 0 ? sc_[0] : kGsNone;
  const int template_status = st_[0];
  __syncthreads();
  // runner-up along the curve: the best station at |m - m_win| >= 2
  double my_ru = kGsNone;
  if (n_valid > 0)
    for (int q = tid; q < cv.n_stations; q += kLkRsReduceThreads)
      if (abs(q - m_win) >= 2)
        my_ru = fmax(my_ru, prof[q]);
  sc_[tid] = my_ru;
  __syncthreads();
  for (int st = kLkRsReduceThreads / 2; st > 0; st >>= 1) {
    if (tid < st)
      sc_[tid] = fmax(sc_[tid], sc_[tid + st]);
    __syncthreads();
  }
  if (tid != 0)
    return;
  int status = cv.status;
  if (status == 0)
    status = template_status != 0 ? template_status : n_valid == 0 ? LK_GS_NO_CANDIDATE : LK_GS_OK;
  if (status == LK_GS_OK && !(best > (double)a.min_score))
    status = LK_GS_WEAK;
  const bool has = n_valid > 0 && (status == LK_GS_OK || status == LK_GS_WEAK);
  const double runner = has ? sc_[0] : kGsNone;
  const int4 rc = a.rect[s];
  lk_epipolar_match &m = ea.match[s];
  float *g = a.guess + (size_t)s * 6;
  int dx = 0, dy = 0, node = 0;
  double t = 0.0, rho = 0.0;
  if (has) {
    const size_t at = (size_t)cv.first_index + (size_t)m_win;
    const int along = cv.first_station + m_win, across = ea.other[at] + b_win;
    dx = cv.axis == 0 ? along : across;
    dy = cv.axis == 0 ? across : along;
    node = ea.node[at];
    if (m_win > 0 && m_win < cv.n_stations - 1 && prof[m_win - 1] > kGsInvalid + 1.5 && prof[m_win + 1] > kGsInvalid + 1.5) {
      const double sm = prof[m_win - 1], sp = prof[m_win + 1]; // (-2 marks a station without a score; scores are >= -1)
      const double den = sm - 2.0 * best + sp;
      if (den < 0.0)
        t = fmin(fmax(0.5 * (sm - sp) / den, -0.5), 0.5);
    }
    rho = ea.inv_depth[at];
    if (t > 0.0)
      rho = rho + t * (ea.inv_depth[at + 1] - rho);
    else if (t < 0.0)
      rho = rho + (0.0 - t) * (ea.inv_depth[at - 1] - rho);
  }
  if (status == LK_GS_OK) {
    const double scale = (double)(1 << a.level);
    g[0] = (float)((double)dx * scale);
    g[1] = (float)((double)dy * scale);
    if (ea.with_shape) {
      const float4 A = ea.shape[(size_t)s * (size_t)ea.n_nodes + (size_t)node];
      g[2] = __fsub_rn(A.x, 1.f);
      g[3] = A.y;
      g[4] = A.z;
      g[5] = __fsub_rn(A.w, 1.f);
    }
  }
  float *pp = a.prev_p + (size_t)s * 6;
  for (int k = 0; k < 6; ++k)
    pp[k] = g[k];
  m.shift_x = dx;
  m.shift_y = dy;
  m.station = m_win;
  m.band_offset = b_win;
  m.node = node;
  m.n_samples = rc.z > 0 ? rc.w : (int)(a.off[s + 1] - a.off[s]);
  m.n_valid = has ? n_valid : 0;
  m.status = status;
  m.score = has ? best : kGsNone;
  m.runner_up = runner;
  m.station_refined = has ? (float)((double)m_win + t) : 0.f;
  m.inv_depth = (float)rho;
  m.reserved[0] = m.reserved[1] = 0;
}

// what a workgroup's LDS holds before the window: the scores and stations of the longest run and a template chunk
static size_t ep_fixed_lds(int max_run, int max_cand) {
  return (size_t)max_cand * sizeof(double) + ((size_t)max_run * sizeof(int) + 7) / 8 * 8 + (size_t)kLkGsChunk * 5;
}

hipError_t lk_launch_epipolar_search(const LkEpipolarSearchArgs &ea, hipStream_t st) {
  if (ea.gs.n_sectors <= 0)
    return hipSuccess;
  const size_t lds = ep_fixed_lds(ea.max_run, ea.max_cand) + (size_t)ea.gs.win_bytes;
  const dim3 grid((unsigned)ea.gs.n_sectors, (unsigned)ea.n_runs);
  if (ea.with_shape)
    hipLaunchKernelGGL(lk_epipolar_search_kernel<true>, grid, dim3(kLkGsThreads), lds, st, ea);
  else
    hipLaunchKernelGGL(lk_epipolar_search_kernel<false>, grid, dim3(kLkGsThreads), lds, st, ea);
  return hipGetLastError();
}

hipError_t lk_launch_epipolar_reduce(const LkEpipolarSearchArgs &ea, hipStream_t st) {
  if (ea.gs.n_sectors <= 0)
    return hipSuccess;
  hipLaunchKernelGGL(lk_epipolar_reduce_kernel, dim3((unsigned)ea.gs.n_sectors), dim3(kLkRsReduceThreads), 0, st, ea);
  return hipGetLastError();
}

// LDS left for the staged window: 64 KB per workgroup minus the scores, the stations, the template chunk and the reduction arrays
int lk_epipolar_search_window_budget(int max_run, int max_cand) {
  const int fixed = (int)ep_fixed_lds(max_run, max_cand) + kLkGsThreads * (2 * 8 + 2 * 4);
  return ((65536 - fixed) / 4) * 4;
}
