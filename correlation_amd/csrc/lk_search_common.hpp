// lk_search_common.hpp - the device code the automatic-guess searches share (lk_guess_search.hip: translation only;
// lk_rotated_search.hip: angle and translation; lk_epipolar_search.hip: along the epipolar curve of a rig): the rounding
// rules, the walk over a sector's level-L samples, the rounded centre of a guess, the accumulate loop over a staged template
// chunk, the tie rule and the two candidate loops (a rectangle of shifts; a list of displacements).  Device only: included
// by the three .hip files and nothing else.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lk_device.hpp"

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

// A sector's level-L samples in the reference's order, rounded and clamped like the solve's template read.
struct GsSector {
  int4 rc;      // the implicit rectangle (z = width; 0: an explicit list)
  uint32_t off; // the list's first entry
  int n, rh;    // samples; the rectangle's height
  const float2 *xy;
  int ucols, urows;
  __device__ __forceinline__ void init(const int4 *rect, const uint32_t *offs, const float2 *xy_, int s, int ucols_, int urows_) {
    rc = rect[s];
    off = offs[s];
    n = rc.z > 0 ? rc.w : (int)(offs[s + 1] - off);
    rh = rc.z > 0 ? rc.w / rc.z : 1;
    xy = xy_;
    ucols = ucols_;
    urows = urows_;
  }
  __device__ __forceinline__ void sample(int k, int &x, int &y) const {
    if (rc.z > 0) { // x outer, y inner (manager_class.cpp:1607-1611)
      const int col = k / rh;
      x = rc.x + col;
      y = rc.y + (k - col * rh);
    } else {
      const float2 q = xy[off + (uint32_t)k];
      x = gs_round(q.x);
      y = gs_round(q.y);
    }
    x = min(max(x, 0), ucols - 1);
    y = min(max(y, 0), urows - 1);
  }
};

// The rounded level-L centre of a guess, floor(g / 2^L + 0.5); false: not a usable centre (huge or NaN: no candidate)
__device__ __forceinline__ bool gs_centre(const float *g, int level, bool has_v, int &cx, int &cy) {
  const float inv = 1.f / (float)(1 << level);
  const float fx = floorf(g[0] * inv + 0.5f), fy = has_v ? floorf(g[1] * inv + 0.5f) : 0.f;
  const bool ok = fabsf(fx) < 1e8f && fabsf(fy) < 1e8f;
  cx = ok ? (int)fx : 0;
  cy = ok ? (int)fy : 0;
  return ok;
}

// Block-wide sums / minima of two values per lane over kLkGsThreads lanes (every lane calls; every lane gets the result)
__device__ __forceinline__ void gs_block_sum2(long long *ra, long long *rb, int tid, long long &x, long long &y) {
  ra[tid] = x;
  rb[tid] = y;
  __syncthreads();
  for (int st = kLkGsThreads / 2; st > 0; st >>= 1) {
    if (tid < st) {
      ra[tid] += ra[tid + st];
      rb[tid] += rb[tid + st];
    }
    __syncthreads();
  }
  x = ra[0];
  y = rb[0];
  __syncthreads();
}
__device__ __forceinline__ void gs_block_min2(int *ra, int *rb, int tid, int &x, int &y) {
  ra[tid] = x;
  rb[tid] = y;
  __syncthreads();
  for (int st = kLkGsThreads / 2; st > 0; st >>= 1) {
    if (tid < st) {
      ra[tid] = min(ra[tid], ra[tid + st]);
      rb[tid] = min(rb[tid], rb[tid + st]);
    }
    __syncthreads();
  }
  x = ra[0];
  y = rb[0];
  __syncthreads();
}

// The candidates of one workgroup: the shifts ilo..ihi x jlo..jhi (not empty, every one with all its samples inside the
// deformed image) of a template whose sample (x, y) reads the deformed pixel pos(x, y) + (cx, cy) + shift; (minx, miny) ..
// (maxx, maxy) is the bounding box of pos over the sector.  gs_lds: the dynamic LDS {scores [ncand], chunk offsets, chunk
// values, window}.  The deformed window every candidate reads is staged in LDS where it fits a.win_bytes (else read in
// place), the template in chunks of kLkGsChunk samples as {offset into the window, value}; lanes own candidates, uint32
// partial sums per chunk - exact, 1024 * 255^2 < 2^32 - added into uint64.  Returns the count of scored candidates and,
// where it is > 0, the winner under the tie rule and its runner-up.
template <class Pos>
__device__ __forceinline__ int gs_search_candidates(const LkGuessSearchArgs &a, unsigned char *gs_lds, long long *r64a,
                                                    long long *r64b, int *r32a, int *r32b, int tid, const GsSector &sec, Pos pos,
                                                    int cx, int cy, int minx, int miny, int maxx, int maxy, int ilo, int ihi,
                                                    int jlo, int jhi, long long St, long long varT, double &best, double &runner,
                                                    int &win_i, int &win_j) {
  const int n = sec.n, R = a.radius, jR = a.has_v ? R : 0;
  const int nci = 2 * R + 1, ncand = nci * (2 * jR + 1);
  double *score = (double *)gs_lds;
  uint32_t *toff = (uint32_t *)(score + ncand);
  uint8_t *tval = (uint8_t *)(toff + kLkGsChunk);
  uint8_t *win = tval + kLkGsChunk;
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
      int x, y, X, Y;
      sec.sample(k0 + q, x, y);
      pos(x, y, X, Y);
      toff[q] = (uint32_t)(Y - miny) * pitch + (uint32_t)(X - minx);
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
    const uint32_t base = in_lds ? (uint32_t)(jj * Wx + ii) : (uint32_t)(cy + j + miny) * pitch + (uint32_t)(cx + i + minx);
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
  const int n_valid = (int)r64b[0];
  if (n_valid > 0) {
    best = __longlong_as_double(r64a[0]);
    win_i = r32a[0];
    win_j = r32b[0];
  }
  __syncthreads();
  if (n_valid == 0)
    return 0;
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
  return n_valid;
}

// a before b on a curve (m: the station, b: the offset across): higher score, then smaller |b|, then smaller b, then smaller m
__device__ __forceinline__ bool gs_listed_better(double sa, int ma, int ba, double sb, int mb, int bb) {
  if (sa != sb)
    return sa > sb;
  if (abs(ba) != abs(bb))
    return abs(ba) < abs(bb);
  if (ba != bb)
    return ba < bb;
  return ma < mb;
}

// gs_search_candidates' sibling for candidates that are a list and no rectangle: candidate q = ml * nb + (b + B), nb = 2B + 1,
// of the stations ml = 0 .. nst-1 of one workgroup has the displacement disp(q) -> (dx, dy), and its template sample (x, y)
// reads the deformed pixel pos(x, y) + (dx, dy); (minx, miny) .. (maxx, maxy) is the bounding box of pos over the sector, so a
// candidate has all its samples inside the deformed image exactly when the displaced box is (in 64 bits: a mapped position
// may be anywhere).  score [nst * nb], toff and tval [kLkGsChunk] and win [a.win_bytes] are the workgroup's LDS.  The window
// staged is the one the candidates that are inside read, in LDS where it fits a.win_bytes (else read in place); the chunks,
// the lanes' candidates and the exact sums are gs_search_candidates'.  profile [nst] (global) receives the best score of every
// station over b, -2 where it has none.  Returns the count of scored candidates and, where it is > 0, the winner under
// gs_listed_better (m0: the index of station 0 on the sector's curve).
template <class Pos, class Disp>
__device__ __forceinline__ int gs_search_listed(const LkGuessSearchArgs &a, double *score, uint32_t *toff, uint8_t *tval, uint8_t *win,
                                                long long *r64a, long long *r64b, int *r32a, int *r32b, int tid, const GsSector &sec,
                                                Pos pos, Disp disp, int minx, int miny, int maxx, int maxy, int nst, int B, int m0,
                                                long long St, long long varT, double *profile, double &best, int &win_q) {
  const int n = sec.n, nb = 2 * B + 1, ncand = nst * nb;
  auto inside = [&](int dx, int dy) {
    return (long long)minx + dx >= 0 && (long long)maxx + dx <= (long long)a.dcols - 1 && (long long)miny + dy >= 0 &&
           (long long)maxy + dy <= (long long)a.drows - 1;
  };
  // the displacements of the candidates that are inside: their bounding box (block-wide, so that every branch below is)
  int dxlo = 0x7fffffff, dylo = 0x7fffffff, dxhi = -0x7fffffff, dyhi = -0x7fffffff;
  for (int q = tid; q < ncand; q += kLkGsThreads) {
    int dx, dy;
    disp(q, dx, dy);
    score[q] = kGsInvalid;
    if (inside(dx, dy)) {
      dxlo = min(dxlo, dx);
      dylo = min(dylo, dy);
      dxhi = max(dxhi, dx);
      dyhi = max(dyhi, dy);
    }
  }
  gs_block_min2(r32a, r32b, tid, dxlo, dylo);
  dxhi = -dxhi;
  dyhi = -dyhi;
  gs_block_min2(r32a, r32b, tid, dxhi, dyhi);
  dxhi = -dxhi;
  dyhi = -dyhi;
  if (dxlo > dxhi) { // no candidate is inside
    for (int q = tid; q < nst; q += kLkGsThreads)
      profile[q] = kGsNone;
    return 0;
  }
  const int Wx = (maxx - minx) + (dxhi - dxlo) + 1, Wy = (maxy - miny) + (dyhi - dylo) + 1; // (inside the image: no overflow)
  const bool in_lds = (long long)Wx * Wy <= (long long)a.win_bytes;
  const int X0 = minx + dxlo, Y0 = miny + dylo;
  const uint32_t pitch = in_lds ? (uint32_t)Wx : (uint32_t)a.dcols;
  if (in_lds)
    for (int q = tid; q < Wx * Wy; q += kLkGsThreads) {
      const int r = q / Wx;
      win[q] = a.def[(size_t)(Y0 + r) * (size_t)a.dcols + (size_t)(X0 + (q - r * Wx))];
    }
  auto stage = [&](int k0, int cnt) {
    for (int q = tid; q < cnt; q += kLkGsThreads) {
      int x, y, X, Y;
      sec.sample(k0 + q, x, y);
      pos(x, y, X, Y);
      toff[q] = (uint32_t)(Y - miny) * pitch + (uint32_t)(X - minx);
      tval[q] = a.und[(size_t)y * (size_t)a.ucols + (size_t)x];
    }
  };
  const int nchunks = (n + kLkGsChunk - 1) / kLkGsChunk;
  if (nchunks == 1)
    stage(0, n);
  __syncthreads();
  double my_best = kGsInvalid;
  int my_q = 0x7fffffff, my_m = 0x7fffffff, my_b = 30000, my_valid = 0;
  for (int c0 = 0; c0 < ncand; c0 += kLkGsThreads) {
    const int c = c0 + tid;
    int dx = 0, dy = 0;
    if (c < ncand)
      disp(c, dx, dy);
    const bool act = c < ncand && inside(dx, dy);
    const uint32_t base = !act     ? 0u
                          : in_lds ? (uint32_t)((dy - dylo) * Wx + (dx - dxlo))
                                   : (uint32_t)(dy + miny) * pitch + (uint32_t)(dx + minx);
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
        const int ml = c / nb, b = c - ml * nb - B;
        score[c] = sc;
        ++my_valid;
        if (gs_listed_better(sc, m0 + ml, b, my_best, my_m, my_b)) {
          my_best = sc;
          my_q = c;
          my_m = m0 + ml;
          my_b = b;
        }
      }
    }
  }
  // winner: tree reduction under the tie rule (+ the count of scored candidates)
  r64a[tid] = __double_as_longlong(my_best);
  r64b[tid] = my_valid;
  r32a[tid] = my_q;
  __syncthreads();
  for (int st = kLkGsThreads / 2; st > 0; st >>= 1) {
    if (tid < st) {
      const int qo = r32a[tid + st], qm = r32a[tid];
      // (a lane without a candidate holds kGsInvalid, below every score: its q is never read as a candidate)
      const int mo = qo / nb, bo = qo - mo * nb - B, mm = qm / nb, bm = qm - mm * nb - B;
      if (gs_listed_better(__longlong_as_double(r64a[tid + st]), mo, bo, __longlong_as_double(r64a[tid]), mm, bm)) {
        r64a[tid] = r64a[tid + st];
        r32a[tid] = qo;
      }
      r64b[tid] += r64b[tid + st];
    }
    __syncthreads();
  }
  const int n_valid = (int)r64b[0];
  if (n_valid > 0) {
    best = __longlong_as_double(r64a[0]);
    win_q = r32a[0];
  }
  // (the scores are complete: the reduction's barriers lie behind the last write)
  for (int q = tid; q < nst; q += kLkGsThreads) {
    double p = kGsNone;
    for (int bb = 0; bb < nb; ++bb) {
      const double sc = score[q * nb + bb];
      if (sc > kGsInvalid)
        p = fmax(p, sc);
    }
    profile[q] = p;
  }
  __syncthreads();
  return n_valid;
}

} // namespace
