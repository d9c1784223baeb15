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
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "lk_device.hpp"
#include "lk_launch.hpp"

static_assert(offsetof(lk_guess_match, score) == 32 && sizeof(lk_guess_match) == 48, "lk_guess_match layout");

namespace {

constexpr double kGsInvalid = -3.0; // score slot of a candidate without a score (valid scores are in [-1, 1])
constexpr double kGsNone = -2.0;    // reported score / runner-up where there is none

// (int)(v + 0.5f) as the host code computes it: out-of-range and NaN give INT_MIN (cvttss2si)
__device__ __forceinline__ int gs_round(float v) {
  const float t = v + 0.5f;
  return fabsf(t) < 2147483648.f ? (int)t : (int)0x80000000;
}

// a before b: higher score, then smaller i^2 + j^2, then smaller j, then smaller i
__device__ __forceinline__ bool gs_better(double sa, int ia, int ja, double sb, int ib, int jb) {
  if (sa != sb)
    return sa > sb;
  const int ra = ia * ia + ja * ja, rb = ib * ib + jb * jb;
  if (ra != rb)
    return ra < rb;
  if (ja != jb)
    return ja < jb;
  return ia < ib;
}

__device__ __forceinline__ void gs_accumulate(const uint8_t *src, uint32_t base, const uint32_t *toff, const uint8_t *tval,
                                              int cnt, uint32_t &sd, uint32_t &sdd, uint32_t &std_) {
  for (int k = 0; k < cnt; ++k) {
    const uint32_t d = src[base + toff[k]], t = tval[k];
    sd += d;
    sdd += d * d;
    std_ += t * d;
  }
}

} // namespace

__global__ __launch_bounds__(kLkGsThreads) void lk_guess_search_kernel(LkGuessSearchArgs a) {
  extern __shared__ __align__(16) unsigned char gs_lds[];
  __shared__ long long r64a[kLkGsThreads], r64b[kLkGsThreads];
  __shared__ int r32a[kLkGsThreads], r32b[kLkGsThreads];
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int R = a.radius, jR = a.has_v ? R : 0;
  const int nci = 2 * R + 1, ncand = nci * (2 * jR + 1);
  double *score = (double *)gs_lds;
  uint32_t *toff = (uint32_t *)(score + ncand);
  uint8_t *tval = (uint8_t *)(toff + kLkGsChunk);
  uint8_t *win = tval + kLkGsChunk;

  const int4 rc = a.rect[s];
  const uint32_t off = a.off[s];
  const int n = rc.z > 0 ? rc.w : (int)(a.off[s + 1] - off);
  const int rh = rc.z > 0 ? rc.w / rc.z : 1;
  float *g = a.guess + (size_t)s * 6;
  const float scale = (float)(1 << a.level), inv = 1.f / scale;
  const float fx = floorf(g[0] * inv + 0.5f), fy = a.has_v ? floorf(g[1] * inv + 0.5f) : 0.f;
  const bool centre_ok = fabsf(fx) < 1e8f && fabsf(fy) < 1e8f; // (NaN: no candidate)
  const int cx = centre_ok ? (int)fx : 0, cy = centre_ok ? (int)fy : 0;

  auto sample = [&](int k, int &x, int &y) { // level-L sample k, rounded and clamped like the solve's template read
    if (rc.z > 0) { // x outer, y inner (manager_class.cpp:1607-1611)
      const int col = k / rh;
      x = rc.x + col;
      y = rc.y + (k - col * rh);
    } else {
      const float2 q = a.xy[off + (uint32_t)k];
      x = gs_round(q.x);
      y = gs_round(q.y);
    }
    x = min(max(x, 0), a.ucols - 1);
    y = min(max(y, 0), a.urows - 1);
  };
  auto sum2 = [&](long long &x, long long &y) {
    r64a[tid] = x;
    r64b[tid] = y;
    __syncthreads();
    for (int st = kLkGsThreads / 2; st > 0; st >>= 1) {
      if (tid < st) {
        r64a[tid] += r64a[tid + st];
        r64b[tid] += r64b[tid + st];
      }
      __syncthreads();
    }
    x = r64a[0];
    y = r64b[0];
    __syncthreads();
  };
  auto min2 = [&](int &x, int &y) {
    r32a[tid] = x;
    r32b[tid] = y;
    __syncthreads();
    for (int st = kLkGsThreads / 2; st > 0; st >>= 1) {
      if (tid < st) {
        r32a[tid] = min(r32a[tid], r32a[tid + st]);
        r32b[tid] = min(r32b[tid], r32b[tid + st]);
      }
      __syncthreads();
    }
    x = r32a[0];
    y = r32b[0];
    __syncthreads();
  };

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
      sample(k, x, y);
      const long long t = a.und[(size_t)y * (size_t)a.ucols + (size_t)x];
      St += t;
      Stt += t * t;
      minx = min(minx, x);
      miny = min(miny, y);
      maxx = max(maxx, x);
      maxy = max(maxy, y);
    }
    sum2(St, Stt);
    min2(minx, miny);
    maxx = -maxx;
    maxy = -maxy;
    min2(maxx, maxy);
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
    const int wi = ihi - ilo + 1, nv = wi * (jhi - jlo + 1);
    const int Wx = wi + (maxx - minx), Wy = (jhi - jlo + 1) + (maxy - miny);
    const bool in_lds = (long long)Wx * Wy <= (long long)a.win_bytes;
    const int X0 = cx + ilo + minx, Y0 = cy + jlo + miny;
    const uint32_t pitch = in_lds ? (uint32_t)Wx : (uint32_t)a.dcols;
    for (int q = tid; q < ncand; q += kLkGsThreads)
      score[q] = kGsInvalid;
    if (in_lds)
      for (int q = tid; q < Wx * Wy; q += kLkGsThreads) {
        const int r = q / Wx;
        win[q] = a.def[(size_t)(Y0 + r) * (size_t)a.dcols + (size_t)(X0 + (q - r * Wx))];
      }
    auto stage = [&](int k0, int cnt) {
      for (int q = tid; q < cnt; q += kLkGsThreads) {
        int x, y;
        sample(k0 + q, x, y);
        toff[q] = (uint32_t)(y - miny) * pitch + (uint32_t)(x - minx);
        tval[q] = a.und[(size_t)y * (size_t)a.ucols + (size_t)x];
      }
    };
    const int nchunks = (n + kLkGsChunk - 1) / kLkGsChunk;
    if (nchunks == 1)
      stage(0, n);
    __syncthreads();
    double my_best = kGsInvalid;
    int my_i = 30000, my_j = 30000, my_valid = 0;
    for (int c0 = 0; c0 < nv; c0 += kLkGsThreads) {
      const int c = c0 + tid;
      const bool act = c < nv;
      const int jj = act ? c / wi : 0, ii = act ? c - jj * wi : 0;
      const int i = ilo + ii, j = jlo + jj;
      const uint32_t base = in_lds ? (uint32_t)(jj * Wx + ii)
                                   : (uint32_t)(cy + j + miny) * pitch + (uint32_t)(cx + i + minx);
      unsigned long long Sd = 0, Sdd = 0, Std = 0;
      for (int ch = 0; ch < nchunks; ++ch) {
        const int k0 = ch * kLkGsChunk, cnt = min(kLkGsChunk, n - k0);
        if (nchunks > 1) {
          __syncthreads();
          stage(k0, cnt);
          __syncthreads();
        }
        if (act) {
          uint32_t sd = 0, sdd = 0, std_ = 0;
          if (in_lds)
            gs_accumulate(win, base, toff, tval, cnt, sd, sdd, std_);
          else
            gs_accumulate(a.def, base, toff, tval, cnt, sd, sdd, std_);
          Sd += sd;
          Sdd += sdd;
          Std += std_;
        }
      }
      if (act) {
        const long long varD = (long long)n * (long long)Sdd - (long long)Sd * (long long)Sd;
        if (varD > 0) {
          const long long num = (long long)n * (long long)Std - St * (long long)Sd;
          const double sc = (double)num / sqrt((double)varT * (double)varD);
          score[(j + jR) * nci + (i + R)] = sc;
          ++my_valid;
          if (gs_better(sc, i, j, my_best, my_i, my_j)) {
            my_best = sc;
            my_i = i;
            my_j = j;
          }
        }
      }
    }
    // winner: tree reduction under the tie rule (+ the count of scored candidates)
    r64a[tid] = __double_as_longlong(my_best);
    r64b[tid] = my_valid;
    r32a[tid] = my_i;
    r32b[tid] = my_j;
    __syncthreads();
    for (int st = kLkGsThreads / 2; st > 0; st >>= 1) {
      if (tid < st) {
        const double o = __longlong_as_double(r64a[tid + st]);
        if (gs_better(o, r32a[tid + st], r32b[tid + st], __longlong_as_double(r64a[tid]), r32a[tid], r32b[tid])) {
          r64a[tid] = r64a[tid + st];
          r32a[tid] = r32a[tid + st];
          r32b[tid] = r32b[tid + st];
        }
        r64b[tid] += r64b[tid + st];
      }
      __syncthreads();
    }
    n_valid = (int)r64b[0];
    if (n_valid > 0) {
      best = __longlong_as_double(r64a[0]);
      win_i = r32a[0];
      win_j = r32b[0];
    }
    __syncthreads();
    if (n_valid == 0) {
      status = LK_GS_NO_CANDIDATE;
    } else {
      double my_ru = kGsNone;
      for (int q = tid; q < ncand; q += kLkGsThreads) {
        const double sc = score[q];
        const int j = q / nci - jR, i = q - (q / nci) * nci - R;
        if (sc > kGsInvalid && max(abs(i - win_i), abs(j - win_j)) >= 2)
          my_ru = fmax(my_ru, sc);
      }
      r64a[tid] = __double_as_longlong(my_ru);
      __syncthreads();
      for (int st = kLkGsThreads / 2; st > 0; st >>= 1) {
        if (tid < st)
          r64a[tid] = __double_as_longlong(fmax(__longlong_as_double(r64a[tid]), __longlong_as_double(r64a[tid + st])));
        __syncthreads();
      }
      runner = __longlong_as_double(r64a[0]);
      status = best > (double)a.min_score ? LK_GS_OK : LK_GS_WEAK;
    }
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
