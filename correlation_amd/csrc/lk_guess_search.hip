// lk_guess_search.hip - the automatic initial guess: integer-pixel ZNCC search of every sector's level-L template over
// (2R+1)^2 shifts of the deformed image (include/lk_engine.h, lk_search_guesses, has the semantics).
//
// One workgroup of 256 lanes per sector.  The sector's samples are rounded and reduced to their bounding box and the
// template sums (St, Stt); the deformed window every valid candidate reads - (bbox + 2R)^2 bytes for small sectors - is
// staged in LDS (larger windows are read from global memory in place), the template in chunks of kLkGsChunk samples as
// {offset into the window, value}.  Lanes own candidates: each walks the chunk with one LDS byte read and three integer
// multiply-adds per sample (the template reads are LDS broadcasts), uint32 partial sums per chunk - exact, 1024 * 255^2
// < 2^32 - added into uint64.  Scores land in LDS; a tree reduction picks the winner under the tie rule, a second walk
// over the scores the runner-up.  Every sum is an integer: the result does not depend on lane count or order.
// The sample walk, the candidate loop and the tie rule live in lk_search_common.hpp, shared with lk_rotated_search.hip.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "lk_device.hpp"
#include "lk_launch.hpp"
#include "lk_search_common.hpp"

static_assert(offsetof(lk_guess_match, score) == 32 && sizeof(lk_guess_match) == 48, "lk_guess_match layout");

__global__ __launch_bounds__(kLkGsThreads) void lk_guess_search_kernel(LkGuessSearchArgs a) {
  extern __shared__ __align__(16) unsigned char gs_lds[];
  __shared__ long long r64a[kLkGsThreads], r64b[kLkGsThreads];
  __shared__ int r32a[kLkGsThreads], r32b[kLkGsThreads];
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int R = a.radius, jR = a.has_v ? R : 0;
  GsSector sec;
  sec.init(a.rect, a.off, a.xy, s, a.ucols, a.urows);
  const int n = sec.n;
  float *g = a.guess + (size_t)s * 6;
  const float scale = (float)(1 << a.level);
  int cx, cy;
  const bool centre_ok = gs_centre(g, a.level, a.has_v != 0, cx, cy);
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
      int x, y;
      sec.sample(k, x, y);
      const long long t = a.und[(size_t)y * (size_t)a.ucols + (size_t)x];
      St += t;
      Stt += t * t;
      minx = min(minx, x);
      miny = min(miny, y);
      maxx = max(maxx, x);
      maxy = max(maxy, y);
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
  // candidates whose every shifted sample is inside the deformed image: a rectangle of shifts
  int ilo = 0, ihi = -1, jlo = 0, jhi = -1;
  if (status < 0) {
    ilo = max(-R, -cx - minx);
    ihi = min(R, a.dcols - 1 - cx - maxx);
    jlo = max(-jR, -cy - miny);
    jhi = min(jR, a.drows - 1 - cy - maxy);
    if (!centre_ok || ilo > ihi || jlo > jhi)
      status = LK_GS_NO_CANDIDATE;
  }
  int win_i = 0, win_j = 0, n_valid = 0;
  double best = kGsNone, runner = kGsNone;
  if (status < 0) {
    auto same = [](int x, int y, int &X, int &Y) {
      X = x;
      Y = y;
    };
    n_valid = gs_search_candidates(a, gs_lds, r64a, r64b, r32a, r32b, tid, sec, same, cx, cy, minx, miny, maxx, maxy, ilo, ihi,
                                   jlo, jhi, St, varT, best, runner, win_i, win_j);
    status = n_valid == 0 ? LK_GS_NO_CANDIDATE : best > (double)a.min_score ? LK_GS_OK : LK_GS_WEAK;
  }
  if (tid != 0)
    return;
  if (status == LK_GS_OK) {
    g[0] = (float)((double)(cx + win_i) * (double)scale);
    if (a.has_v)
      g[1] = (float)((double)(cy + win_j) * (double)scale);
  }
  float *pp = a.prev_p + (size_t)s * 6;
  for (int k = 0; k < 6; ++k)
    pp[k] = g[k];
  lk_guess_match &m = a.match[s];
  m.center_x = cx;
  m.center_y = cy;
  m.shift_x = win_i;
  m.shift_y = win_j;
  m.n_samples = n;
  m.n_valid = n_valid;
  m.status = status;
  reinterpret_cast<int *>(&m)[7] = 0; // the padding before `score`: records compare byte for byte
  m.score = best;
  m.runner_up = runner;
}

hipError_t lk_launch_guess_search(const LkGuessSearchArgs &a, hipStream_t st) {
  if (a.n_sectors <= 0)
    return hipSuccess;
  const int ncand = (2 * a.radius + 1) * (a.has_v ? 2 * a.radius + 1 : 1);
  const size_t lds = (size_t)ncand * sizeof(double) + (size_t)kLkGsChunk * 5 + (size_t)a.win_bytes;
  hipLaunchKernelGGL(lk_guess_search_kernel, dim3((unsigned)a.n_sectors), dim3(kLkGsThreads), lds, st, a);
  return hipGetLastError();
}

// LDS left for the staged window: 64 KB per workgroup minus the scores, the template chunk and the reduction arrays
int lk_guess_search_window_budget(int radius, int has_v) {
  const int ncand = (2 * radius + 1) * (has_v ? 2 * radius + 1 : 1);
  const int fixed = ncand * (int)sizeof(double) + kLkGsChunk * 5 + kLkGsThreads * (2 * 8 + 2 * 4);
  return ((65536 - fixed) / 4) * 4;
}
